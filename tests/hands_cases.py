"""Cases for awr_detect_hands (csrc/awr_hands.hip) and its numpy statements awr_amd.detect.components / hand_seeds: numpy
only, fixed seeds.  A case is a frame and the detector's knobs; cases that share a shape and knobs form a group, which the GPU test sends
through one call.  The references are computed once per case (for K = MAX_HANDS: the slots of a smaller K are its first rows) and shared,
read-only.  `two_hands` builds the 32 two-hand composites of the anchor property."""
import functools

import numpy as np

NEAR = 700
DEFAULT = dict(depth_range=(1.0, 2000.0), reach=300.0, slab=150.0, min_pixels=6)
SHAPES = [(1, 1), (1, 64), (64, 1), (17, 23), (33, 130), (48, 64)]          # 33 x 130 crosses the 64 x 16 tiles both ways with remainders
FULL = (480, 640)
KS = (1, 2, 4)


def same(a, b):
    """np.array_equal with NaN positions equal"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def _frame(mask, depth=NEAR):
    return np.where(mask, depth, 0).astype(np.uint16)


def serpentine(h, w):
    """every other row full, the rows between them one pixel at alternating ends: one corridor from index 0 to the last row"""
    m = np.zeros((h, w), bool)
    m[0::2] = True
    m[1::4, w - 1] = True
    m[3::4, 0] = True
    return m


def spiral(h, w):
    """a one-pixel corridor winding inwards from (0, 0), one pixel of background between its arms"""
    m = np.zeros((h, w), bool)
    v, u, dv, du = 0, 0, 0, 1
    m[0, 0] = True
    while True:
        for _ in range(2):
            nv, nu, fv, fu = v + dv, u + du, v + 2 * dv, u + 2 * du
            if 0 <= nv < h and 0 <= nu < w and not m[nv, nu] and not (0 <= fv < h and 0 <= fu < w and m[fv, fu]):
                v, u = nv, nu
                m[v, u] = True
                break
            dv, du = du, -dv
        else:
            return m


def comb(h, w):
    """teeth on every other column that join only in the last row"""
    m = np.zeros((h, w), bool)
    m[:, 0::2] = True
    m[h - 1] = True
    return m


def _patterns(h, w, seed):
    r = np.random.RandomState(seed)
    out = {"empty": np.zeros((h, w), np.uint16), "full": _frame(np.ones((h, w), bool)),
           "checker": _frame((np.add.outer(np.arange(h), np.arange(w)) % 2) == 0),
           "random": _frame(r.uniform(size=(h, w)) < 0.5, NEAR + r.randint(0, 200, (h, w)))}
    if h >= 5 and w >= 5:
        out["serpentine"] = _frame(serpentine(h, w), NEAR + np.arange(h)[:, None])          # the nearest pixel is at the corridor's start
        out["serpentine_far"] = _frame(serpentine(h, w), NEAR + h - np.arange(h)[:, None])  # ... at its end
        out["spiral"] = _frame(spiral(h, w))
        out["comb"] = _frame(comb(h, w), NEAR + r.randint(0, 100, (h, w)))
        holes = r.uniform(size=(h, w)) < 0.12
        out["holes"] = _frame(~holes, NEAR + r.randint(0, 250, (h, w)))                     # holes of depth 0, a slab that cuts
    return out


def _add(cases, name, frame, **knobs):
    frame = np.ascontiguousarray(frame, dtype=np.uint16)
    frame.setflags(write=False)
    k = dict(DEFAULT)
    k.update(knobs)
    cases[name] = dict(name=name, frame=frame, **k)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(name, frame (read-only), depth_range, reach, slab, min_pixels)"""
    out = {}
    for i, (h, w) in enumerate(SHAPES):
        for pat, frame in _patterns(h, w, 100 + i).items():
            _add(out, "%dx%d_%s" % (h, w, pat), frame)
    h, w = 33, 130
    # two blobs that touch only diagonally, across the tile corner (16, 64): two components
    f = np.zeros((h, w), np.uint16)
    f[8:16, 56:64], f[16:24, 64:72] = 705, 700
    _add(out, "diagonal_blobs", f)
    # one component through that tile corner: three tiles, the fourth only touched diagonally
    f = np.zeros((h, w), np.uint16)
    f[15, 60:65], f[15:18, 64], f[17, 64:70], f[16, 62] = 700, 701, 702, 703
    _add(out, "tile_corner", f, min_pixels=1)
    f = np.zeros((h, w), np.uint16)
    f[15:17, 63:65] = 700
    _add(out, "tile_corner_block", f, min_pixels=4)
    h, w = 48, 64
    # pixels at exactly dmin + reach belong to the mask, one millimetre past it they do not
    f = np.zeros((h, w), np.uint16)
    f[10:20, 0:20], f[10:20, 20:40], f[10:20, 40:60], f[30:40, 5:15] = 700, 1000, 1001, 1001
    _add(out, "reach_exact", f)
    _add(out, "reach_fraction", f, reach=300.5)
    _add(out, "reach_zero", f, reach=0.0)
    # zmax cuts before the reach does, and cuts the slab too
    f = np.zeros((h, w), np.uint16)
    f[5:15, 5:25], f[5:15, 25:45], f[5:15, 45:60], f[20:30, 5:25] = 700, 900, 901, 2500
    _add(out, "zmax_cut", f, depth_range=(1.0, 900.0))
    _add(out, "zmin_cut", f, depth_range=(800.0, 2000.0))
    # two components with the same nearest depth: the smaller root comes first, whatever the sizes
    f = np.zeros((h, w), np.uint16)
    f[30:40, 2:8], f[4:20, 30:60], f[4, 30], f[39, 7] = 730, 760, 700, 700
    _add(out, "equal_zc", f)
    # a component of exactly min_pixels pixels counts, one of min_pixels - 1 does not -- although it is the nearer one
    f = np.zeros((h, w), np.uint16)
    f[2:6, 2:7], f[10, 10:29], f[20:30, 20:30] = 720, 700, 800
    _add(out, "min_pixels_edge", f, min_pixels=20)
    # six candidates at six depths (more than any K), none of them in raster order of depth; and a slab that cuts each of them
    f = np.zeros((h, w), np.uint16)
    for i, z in enumerate((860, 700, 990, 760, 910, 705)):
        f[4 + 22 * (i // 3):20 + 22 * (i // 3), 2 + 21 * (i % 3):18 + 21 * (i % 3)] = z + 12 * np.arange(16)[:, None]
    _add(out, "six_candidates", f)
    _add(out, "six_candidates_none_large", f, min_pixels=257)
    # near the percolation threshold of the square lattice (0.593): large tortuous components
    for dens in (0.55, 0.6):
        r = np.random.RandomState(int(dens * 100))
        _add(out, "percolation_%d" % int(dens * 100), _frame(r.uniform(size=(40, 56)) < dens, NEAR + r.randint(0, 280, (40, 56))))
    return out


@functools.lru_cache(maxsize=None)
def full_cases():
    """480 x 640: the serpentine (the worst case for propagation: 40 x 30 tiles, one corridor), a percolating random mask, two hand-sized
    blobs and debris"""
    out = {}
    h, w = FULL
    _add(out, "full_serpentine", _frame(serpentine(h, w), NEAR + (np.arange(h)[:, None] // 2)), min_pixels=400)
    r = np.random.RandomState(7)
    _add(out, "full_percolation", _frame(r.uniform(size=(h, w)) < 0.6, NEAR + r.randint(0, 290, (h, w))), min_pixels=400)
    f = np.zeros((h, w), np.uint16)
    vv, uu = np.indices((h, w))
    f[(vv - 200) ** 2 + (uu - 150) ** 2 < 60 ** 2] = 820
    f[(vv - 260) ** 2 + (uu - 490) ** 2 < 50 ** 2] = 760
    f[r.uniform(size=(h, w)) < 0.01] = 750
    _add(out, "full_blobs", f, min_pixels=400)
    return out


def groups(which=None):
    """(shape, knobs) -> the names of the cases that share them, in a fixed order"""
    out = {}
    for name, c in (cases() if which is None else which).items():
        key = (c["frame"].shape, c["depth_range"], c["reach"], c["slab"], c["min_pixels"])
        out.setdefault(key, []).append(name)
    return out


def knobs(c):
    return dict(depth_range=c["depth_range"], reach=c["reach"], slab=c["slab"], min_pixels=c["min_pixels"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (labels (fh, fw) int32, centres (4, 3), status (4,), info (4, 4), count) of the statement, read-only"""
    import awr_amd  # noqa: F401
    from awr_amd import detect as D
    c = cases()[name] if name in cases() else full_cases()[name]
    labels = D.components(c["frame"], c["depth_range"], c["reach"])
    centers, status, info, count = D.hand_seeds(c["frame"], D.MAX_HANDS, **knobs(c))
    for a in (labels, centers, status, info):
        a.setflags(write=False)
    return labels, centers, status, info, count


def batch_reference(names, idx, K, n_frames):
    """the statement for a batch: frame indices `idx` into the stacked cases `names` -> hand-major (labels (B, fh, fw), centres (K, B, 3),
    status (K, B), info (K, B, 4), count (B,)); an index outside [0, n_frames) is a bad frame"""
    B = len(idx)
    shape = reference(names[0])[0].shape
    labels = np.full((B,) + shape, -1, np.int32)
    centers, status = np.full((K, B, 3), np.nan), np.full((K, B), 2, np.int32)
    info, count = np.tile(np.array((-1, -1, 0, 0), np.int32), (K, B, 1)), np.zeros(B, np.int32)
    for b, i in enumerate(idx):
        if 0 <= i < n_frames:
            lab, c, s, inf, n = reference(names[i])
            labels[b], centers[:, b], status[:, b], info[:, b], count[b] = lab, c[:K], s[:K], inf[:K], n
    return labels, centers, status, info, count


# ---- the two-hand composites ------------------------------------------------------------------------------------------------------------
N_TWO, U_A, U_B = 32, 150.0, 490.0


@functools.lru_cache(maxsize=None)
def two_hands():
    """The 32 composites' ingredients: -> (prims_a, bbox_a, prims_b, bbox_b).  HandModel(forearm=False); poses sample_poses(32, 21) and
    sample_poses(32, 22); RandomState(5) draws va, za, vb, zb in this order, v = 200 + 80 U, z = 700 + 200 U; hand a at u = 150, hand b
    at u = 490."""
    import awr_amd  # noqa: F401
    from awr_amd import synth as SY
    model = SY.HandModel(forearm=False)
    pa, pb = SY.sample_poses(N_TWO, 21, model), SY.sample_poses(N_TWO, 22, model)
    rs = np.random.RandomState(5)
    va, za = 200.0 + 80.0 * rs.uniform(size=N_TWO), 700.0 + 200.0 * rs.uniform(size=N_TWO)
    vb, zb = 200.0 + 80.0 * rs.uniform(size=N_TWO), 700.0 + 200.0 * rs.uniform(size=N_TWO)
    pa, pb = SY.place_poses(pa, U_A, va, za, model), SY.place_poses(pb, U_B, vb, zb, model)
    _, prims_a, bbox_a = SY.forward_kinematics(pa, model)
    _, prims_b, bbox_b = SY.forward_kinematics(pb, model)
    return prims_a, bbox_a, prims_b, bbox_b


@functools.lru_cache(maxsize=None)
def two_hands_host():
    """-> (frames_a, frames_b, composites) (32, 480, 640) uint16 by the numpy renderer, read-only"""
    from awr_amd import synth as SY
    prims_a, bbox_a, prims_b, bbox_b = two_hands()
    fa, fb = SY.render(prims_a, bbox_a), SY.render(prims_b, bbox_b)
    both = SY.compose(fa, fb)
    for a in (fa, fb, both):
        a.setflags(write=False)
    return fa, fb, both
