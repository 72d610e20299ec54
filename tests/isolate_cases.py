"""Cases for awr_hands_isolate (csrc/awr_isolate.hip) and its numpy statement awr_amd.detect.isolate: numpy only, fixed
seeds.  A case is a frame, its labels (awr_amd.detect.components on the frame, computed once and shared read-only) and a (4,) list of
roots; K = 1, 2, 4 take its first K roots.  The frame shapes are tests/hands_cases.py's: 1 x 1, 1 x 64, 64 x 1, 17 x 23, 33 x 130 and
48 x 64 -- fh * fw = 1, 391 and 4290 are no multiple of 8 (the scalar form), 64 and 3072 are (the 8-pixel form), 17 x 23 has an odd fw.
`near_hands` builds the near-hand composites of the anchor property: two hands so close that each stands in the other's crop cube."""
import functools

import numpy as np

import hands_cases as HC

SHAPES = HC.SHAPES
KS = (1, 2, 4)
KNOBS = dict(depth_range=(1.0, 2000.0), reach=300.0)


def _add(out, name, frame, roots=None, **knobs):
    """roots: None -- the roots of the frame's components in raster order, padded with -1 -- or a list of up to four"""
    import awr_amd  # noqa: F401
    from awr_amd import detect as D
    frame = np.ascontiguousarray(frame, dtype=np.uint16)
    k = dict(KNOBS)
    k.update(knobs)
    labels = D.components(frame, k["depth_range"], k["reach"])
    if roots is None:
        roots = np.unique(labels[labels >= 0]).tolist()[:4]
    roots = np.array((list(roots) + [-1] * 4)[:4], np.int32)
    for a in (frame, labels, roots):
        a.setflags(write=False)
    out[name] = dict(name=name, frame=frame, labels=labels, roots=roots, **k)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(name, frame, labels, roots (4,), depth_range, reach), all read-only"""
    out = {}
    for i, (h, w) in enumerate(SHAPES):
        r = np.random.RandomState(300 + i)
        tag = "%dx%d_" % (h, w)
        _add(out, tag + "empty", np.zeros((h, w), np.uint16))
        _add(out, tag + "empty_no_roots", np.zeros((h, w), np.uint16), roots=[-1, -1, -1, -1])
        _add(out, tag + "one_component", np.full((h, w), 700, np.uint16))                         # its root is index 0
        _add(out, tag + "one_component_other_root", np.full((h, w), 700, np.uint16), roots=[h * w - 1, -1, 0, 5])
        checker = np.where((np.add.outer(np.arange(h), np.arange(w)) % 2) == 0, 700 + r.randint(0, 200, (h, w)), 0)
        _add(out, tag + "checker", checker)                                                       # every pixel a component of its own
        _add(out, tag + "checker_gaps", checker, roots=[-1, 0, -1, 2 if h * w > 2 else 0])
        _add(out, tag + "random", np.where(r.uniform(size=(h, w)) < 0.5, 700 + r.randint(0, 400, (h, w)), 0))      # some beyond the reach
    h, w = 33, 130
    vv, uu = np.indices((h, w))
    # two blobs plus debris: the debris is labelled, so it leaves EVERY hand's frame; the root of blob a is index 0
    f = np.zeros((h, w), np.uint16)
    f[0:14, 0:30], f[10:30, 70:120] = 720, 760
    r = np.random.RandomState(11)
    clear = np.ones((h, w), bool)
    clear[0:15, 0:31], clear[9:31, 69:121] = False, False                                          # (no debris on or next to a blob)
    deb = (r.uniform(size=(h, w)) < 0.04) & clear
    f[deb] = (700 + r.randint(0, 250, (h, w)))[deb]
    lab_a, lab_b = 0, 10 * w + 70
    _add(out, "two_blobs_debris", f, roots=[lab_a, lab_b, -1, lab_a])
    _add(out, "two_blobs_debris_swapped", f, roots=[lab_b, -1, lab_a, 3])                          # 3: background or debris, nobody's root
    # a hole of depth 0 inside a hand, a far pixel inside the hole that is beyond the reach, and a second hand
    f = np.zeros((h, w), np.uint16)
    f[(vv - 16) ** 2 + (uu - 30) ** 2 < 14 ** 2] = 700
    f[(vv - 16) ** 2 + (uu - 30) ** 2 < 5 ** 2] = 0
    f[16, 30] = 1001
    f[4:28, 80:110] = 800
    _add(out, "hole_in_a_hand", f)
    # pixels at dmin + reach are labelled; one millimetre beyond it they are not, and must survive in every output (so must depth > zmax)
    h, w = 48, 64
    f = np.zeros((h, w), np.uint16)
    f[10:20, 0:20], f[10:20, 24:40], f[10:20, 40:60], f[30:40, 5:15], f[42:46, 40:50] = 700, 1000, 1001, 1001, 2500
    _add(out, "beyond_the_reach_survives", f)
    _add(out, "beyond_the_reach_survives_no_roots", f, roots=[-1, -1, -1, -1])
    f = np.zeros((h, w), np.uint16)
    for i, z in enumerate((860, 700, 990, 760, 910, 705)):
        f[4 + 22 * (i // 3):20 + 22 * (i // 3), 2 + 21 * (i % 3):18 + 21 * (i % 3)] = z + 12 * np.arange(16)[:, None]
    _add(out, "six_blobs", f, roots=[4 * w + 23, 26 * w + 44, 26 * w + 2, 4 * w + 2])
    return out


def groups():
    """shape -> the names of the cases of that shape, in a fixed order"""
    out = {}
    for name, c in cases().items():
        out.setdefault(c["frame"].shape, []).append(name)
    return out


def loop_reference(frame, labels, roots):
    """the rule, pixel by pixel in plain Python: what awr_amd.detect.isolate states"""
    fh, fw = frame.shape
    out = np.zeros((len(roots), fh, fw), np.uint16)
    for k, root in enumerate(int(r) for r in roots):
        for v in range(fh):
            for u in range(fw):
                label = int(labels[v, u])
                out[k, v, u] = 0 if (root >= 0 and label >= 0 and label != root) else frame[v, u]
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (4, fh, fw) uint16 of the statement for the case's four roots, read-only (the outputs of a smaller K are its first rows)"""
    import awr_amd  # noqa: F401
    from awr_amd import detect as D
    c = cases()[name]
    out = D.isolate(c["frame"], c["labels"], c["roots"])
    out.setflags(write=False)
    return out


def batch_reference(names, idx, K):
    """frame indices `idx` into the stacked cases `names`, batch row b taking the roots of case names[idx[b]] -> (out (K * B, fh, fw)
    hand-major, status (B,)); an index outside the stack is a bad frame: zero frames, status BAD_FRAME (2)"""
    B = len(idx)
    shape = cases()[names[0]]["frame"].shape
    out, status = np.zeros((K, B) + shape, np.uint16), np.zeros(B, np.int32)
    for b, i in enumerate(idx):
        if 0 <= i < len(names):
            out[:, b] = reference(names[i])[:K]
        else:
            status[b] = 2
    return out.reshape((K * B,) + shape), status


# ---- the near-hand composites -------------------------------------------------------------------------------------------------------------
# FIXED: one seed per case.  The seeds are those whose composite satisfies the preconditions tests/test_isolate_cpu.py asserts (two components,
# each one hand's own silhouette, every foreground pixel labelled, each palm point inside the other hand's crop cube).
NEAR_SEEDS = (2, 6, 7, 9)
N_NEAR, NEAR_GAP_MM, FULL = len(NEAR_SEEDS), 130.0, HC.FULL


@functools.lru_cache(maxsize=None)
def near_hands():
    """The composites' ingredients: -> (prims_a, bbox_a, prims_b, bbox_b, palm_a (N, 3), palm_b (N, 3) uvd).  HandModel(forearm=False); per
    case of seed s the poses sample_poses(1, s) and sample_poses(1, s + 1000); RandomState(s) draws va, za, vb, zb in this order,
    v = 200 + 80 U, z = 700 + 200 U (tests/hands_cases.py two_hands' ranges); the palm points NEAR_GAP_MM apart sideways at the mean of
    the two depths, about the image centre -- hands_cases' are 340 px apart."""
    import awr_amd  # noqa: F401
    from awr_amd import nyu_data as ND
    from awr_amd import synth as SY
    model = SY.HandModel(forearm=False)
    parts = {"a": [], "b": []}
    palms = {"a": [], "b": []}
    for s in NEAR_SEEDS:
        rs = np.random.RandomState(s)
        va, za, vb, zb = (lo + span * rs.uniform() for lo, span in ((200.0, 80.0), (700.0, 200.0), (200.0, 80.0), (700.0, 200.0)))
        half = 0.5 * NEAR_GAP_MM * ND.PARAS[0] / (0.5 * (za + zb))
        for key, seed, (u, v, z) in (("a", s, (320.0 - half, va, za)), ("b", s + 1000, (320.0 + half, vb, zb))):
            parts[key].append(SY.place_poses(SY.sample_poses(1, seed, model), u, v, z, model))
            palms[key].append((u, v, z))
    join = lambda ps: {k: np.concatenate([p[k] for p in ps]) for k in ps[0]}
    _, prims_a, bbox_a = SY.forward_kinematics(join(parts["a"]), model)
    _, prims_b, bbox_b = SY.forward_kinematics(join(parts["b"]), model)
    return prims_a, bbox_a, prims_b, bbox_b, np.array(palms["a"]), np.array(palms["b"])


@functools.lru_cache(maxsize=None)
def near_hands_host():
    """-> (frames_a, frames_b, composites) (N_NEAR, 480, 640) uint16 by the numpy renderer, read-only"""
    from awr_amd import synth as SY
    prims_a, bbox_a, prims_b, bbox_b = near_hands()[:4]
    fa, fb = SY.render(prims_a, bbox_a), SY.render(prims_b, bbox_b)
    both = SY.compose(fa, fb)
    for a in (fa, fb, both):
        a.setflags(write=False)
    return fa, fb, both


def near_first(fa, fb):
    """(N,) bool: hand a's smallest depth is the smaller one -- slot 0 is the nearest hand; the two must differ"""
    za = np.where(fa == 0, 1 << 20, fa.astype(np.int64)).reshape(len(fa), -1).min(1)
    zb = np.where(fb == 0, 1 << 20, fb.astype(np.int64)).reshape(len(fb), -1).min(1)
    assert (za != zb).all()
    return za < zb
