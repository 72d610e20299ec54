"""Cases for awr_detect and awr_detect_samples (csrc/awr_detect.hip) and their numpy statements awr_amd.detect.detect / sample_blocks:
numpy only, fixed seeds.  What is here: frame stores whose frames start at every offset from a 16-byte boundary, a numpy model of the index
arithmetic by which detect_pass_kernel splits a window's rows into 16-byte loads and two pixel loops (with four mutants of it), a sweep of
GIVEN centres chosen by the window they produce, a blob on which every refinement pass moves the centre, depth-range cases at the edges of
depth_bounds, and crop-block centres at the boundaries where awr_detect_samples' refusal tests flip.  The references are computed once and
shared, read-only.  The model states the kernel's index arithmetic so that tests/test_detect_cases_cpu.py can say what the cases reach; it
makes no claim about the kernel's results."""
import functools
from fractions import Fraction

import numpy as np

ODD, EVEN, N_FRAMES = (41, 51), (40, 52), 8          # 41 * 51 = 2091 = 3 mod 8: frames 0 ... 7 start 0, 3, 6, 1, 4, 7, 2, 5 pixels past a boundary
PARAS = (66.0, 65.5, 25.5, 20.5)                     # a 300 mm cube spans about 23 pixels at 850 mm (the detector reads fx and fy alone)
FLIP, DSIZE = -1, 32
D0 = 850.0
NARROW, WIDE = (60.0, 200.0, 400.0), (300.0, 200.0, 400.0)          # about 4 and 23 pixels wide at D0; depths D0 +- 200
PAD = 16                                             # pixels behind a store: mutant 1 of the model reads up to 7 pixels past the last row
OK, EMPTY, BAD_FRAME, BAD_WINDOW = 0, 1, 2, 3
VEC, HEAD, TAIL = 0, 1, 2                            # a group's branch: the 16-byte load, the pixel loop at a row's head, the one at its tail


def _detect():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def dense_frames(shape):
    """(8, fh, fw) uint16: every pixel random in [660, 1040] -- inside the depth range D0 +- 200 of every sweep window, so that one pixel
    missed, counted twice or given the wrong column changes an integer sum -- and about 10 % zeros"""
    r = np.random.RandomState(1000 + shape[0])
    f = r.randint(660, 1041, (N_FRAMES,) + tuple(shape)).astype(np.uint16)
    f[r.uniform(size=f.shape) < 0.1] = 0
    return _frozen(f)


def origin_offset(shape, f, shift=0):
    """pixels by which frame f of a store that starts `shift` pixels past a 16-byte boundary is itself past one"""
    return (shift + f * shape[0] * shape[1]) & 7


# ---- the pass's decomposition ----------------------------------------------------------------------------------------------------------
def decompose(mis, fw, window, gpr_short=0):
    """detect_pass_kernel's (row, group) pairs for the clipped window (u0, u1, v0, v1) of a frame whose origin is `mis` pixels past a 16-byte
    boundary: -> dict of (rows, gpr) arrays: live (the pair does any work), branch (VEC / HEAD / TAIL), align (gs & 7, the row's start
    alignment), lo, hi (the pixels [lo, hi) it reads, counted from the boundary before the origin), g0, colbase, v.  A window inside one
    group that starts after the group does is HEAD.  gpr_short: mutant 3."""
    u0, u1, v0, v1 = window
    if u0 >= u1 or v0 >= v1:
        return None
    gpr = ((u1 - u0) >> 3) + 2 - gpr_short
    v = np.arange(v0, v1, dtype=np.int64)[:, None]
    gi = np.arange(gpr, dtype=np.int64)[None, :]
    colbase = mis + v * fw
    gs, ge = colbase + u0, colbase + u1
    g0 = ((gs >> 3) + gi) << 3
    live = g0 < ge
    vec = live & (g0 >= gs) & (g0 + 8 <= ge)
    head = live & ~vec & (g0 < gs)
    branch = np.where(vec, VEC, np.where(head, HEAD, TAIL))
    return dict(live=live, branch=branch, align=np.broadcast_to(gs & 7, g0.shape), lo=np.maximum(g0, gs), hi=np.minimum(g0 + 8, ge), g0=g0,
                colbase=np.broadcast_to(colbase, g0.shape), v=np.broadcast_to(v, g0.shape))


MUTANTS = {0: "the kernel's arithmetic", 1: "the load address without - mis", 2: "the column without - mis", 3: "gpr smaller by one",
           4: "the tail loop one pixel short"}


def model_pass(mem, origin, fw, window, zstart, zend, mutant=0):
    """One pass over a window by the decomposition: mem is the flat store (index 0 on a 16-byte boundary, PAD pixels behind the last frame),
    origin the frame's first pixel in it.  -> ((u, v, d) float64, n) as center_of_mass gives them."""
    mis = origin & 7
    dc = decompose(mis, fw, window, gpr_short=int(mutant == 3))
    if dc is None:
        return (np.nan,) * 3, 0
    k = np.arange(8, dtype=np.int64)
    pos = dc["g0"][..., None] + k
    hi = dc["hi"] - ((dc["branch"] == TAIL) & (mutant == 4))
    valid = dc["live"][..., None] & (pos >= dc["lo"][..., None]) & (pos < hi[..., None])
    addr = origin + pos - mis
    if mutant == 1:
        addr = np.where((dc["branch"] == VEC)[..., None], origin + pos, addr)
    col = pos - dc["colbase"][..., None] + (mis if mutant == 2 else 0)
    d = mem[np.where(valid, addr, 0)].astype(np.int64)
    inside = valid & (d >= zstart) & (d <= zend) & (d != 0)
    n = int(inside.sum())
    if n == 0:
        return (np.nan,) * 3, 0
    su, sv, sd = int(col[inside].sum()), int(np.broadcast_to(dc["v"][..., None], pos.shape)[inside].sum()), int(d[inside].sum())
    return (float(su) / float(n), float(sv) / float(n), float(sd) / float(n)), n


def flat_store(frames, shift=0):
    """the store as the model addresses it: `shift` pixels, the frames, PAD pixels (non-zero, in range)"""
    return np.concatenate([np.full(shift, 901, np.uint16), np.ascontiguousarray(frames).ravel(), np.full(PAD, 901, np.uint16)])


def model_sweep(shape, mutant=0, shift=0):
    """the sweep's one GIVEN refinement pass by the model -> (centres (B, 3) float64, status (B,) int32)"""
    D = _detect()
    frames, (frame, centers, cubes) = dense_frames(shape), sweep(shape)
    mem = flat_store(frames, shift)
    out, status = np.full((len(frame), 3), np.nan), np.zeros(len(frame), np.int32)
    for b in range(len(frame)):
        w = D._window(tuple(centers[b]), cubes[b], PARAS, shape[0], shape[1])
        c, n = model_pass(mem, shift + int(frame[b]) * shape[0] * shape[1], shape[1], w[0], w[1], w[2], mutant) if w is not None else ((np.nan,) * 3, 0)
        out[b], status[b] = c, OK if n else EMPTY
    return out, status


# ---- the window sweep -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sweep(shape):
    """GIVEN centres for one refinement pass on dense_frames(shape), chosen by the window they produce: -> (frame (B,) int64, centres (B, 3),
    cubes (B, 3)) float64, B > 256.  At D0 a cube of w * D0 / fx mm around u = s + w / 2 gives the columns [s, s + w): both bounds lie half
    a pixel from where int() changes."""
    fh, fw = shape
    fx = PARAS[0]
    rows = []
    add = lambda f, u, v, cube: rows.append((f, (u, v, D0), cube))
    for f in range(N_FRAMES):
        # windows of about 4 and 23 pixels stepped over the frame and past its left and right edges, the rows moving with the columns
        for cube in (NARROW, WIDE):
            for k, u in enumerate(np.arange(-3.0, 54.01, 2.5)):
                add(f, float(u), float((5 + 7 * k + 3 * f) % (fh + 6) - 3) + 0.25 * (k % 4), cube)
        # 1 ... 7 pixels wide, starting anywhere in a group
        for w in range(1, 8):
            s = (3 * f + 5 * w) % 30 + 5
            add(f, s + w / 2.0, 20.0, (w * D0 / fx, 200.0, 400.0))
        # exactly 8 pixels wide from every column 16 ... 23: with 8 or more rows of an odd width, or with every start, one row is one aligned group
        add(f, 16 + f + 4.0, 20.0, (8 * D0 / fx, 200.0, 400.0))
        # as wide as the frame: clipped left and right, and at the top or the bottom too
        for v in (2.0, 20.0, fh - 2.5):
            add(f, fw / 2.0, v, (2000.0, 200.0, 400.0))
        # as high as the frame: clipped at the top and the bottom, and at the left or the right too; and the whole frame
        for u in (-1.0, 25.0, fw - 1.5):
            add(f, u, fh / 2.0, (60.0, 2000.0, 400.0))
        add(f, fw / 2.0, fh / 2.0, (2000.0, 2000.0, 400.0))
        # the four corners and the four sides alone
        for u, v in ((1.0, 1.0), (fw - 2.0, 1.5), (1.5, fh - 2.0), (fw - 1.5, fh - 1.5), (25.0, 2.0), (25.0, fh - 3.0), (3.0, 20.0), (fw - 4.0, 20.0)):
            add(f, u, v, WIDE)
    return _frozen(np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.float64), np.array([r[2] for r in rows], np.float64))


def sweep_windows(shape):
    """per sweep row: (the unclipped bounds (ustart, uend, vstart, vend) of center2bounds, the clipped window (u0, u1, v0, v1))"""
    import awr_amd  # noqa: F401
    from awr_amd import nyu_data as ND
    _, centers, cubes = sweep(shape)
    out = []
    for c, cube in zip(centers, cubes):
        b = ND.center2bounds(c, cube, PARAS)[:4]
        out.append((b, (max(b[0], 0), min(b[1], shape[1]), max(b[2], 0), min(b[3], shape[0]))))
    return out


def clipped_sides(bounds, shape):
    """the sides of the frame that cut a non-empty window: a frozenset of "left", "right", "top", "bottom" """
    us, ue, vs, ve = bounds
    return frozenset(name for name, cut in (("left", us < 0), ("right", ue > shape[1]), ("top", vs < 0), ("bottom", ve > shape[0])) if cut)


def reference_rows(frames, frame, seed, centers, cubes, iters, **kw):
    """detect.detect for every batch row alone -> (centres (B, 3) float64, status (B,) int32); a frame index outside the store: NaN, BAD_FRAME"""
    D = _detect()
    cubes = np.broadcast_to(np.asarray(cubes, np.float64), (len(frame), 3))
    out, status = np.full((len(frame), 3), np.nan), np.full(len(frame), BAD_FRAME, np.int32)
    for b, f in enumerate(frame):
        if 0 <= f < len(frames):
            out[b], status[b] = D.detect(frames[f], seed=seed, center=None if centers is None else centers[b], cube=cubes[b], paras=PARAS, iters=iters, **kw)
    return _frozen(out, status)


@functools.lru_cache(maxsize=None)
def sweep_reference(shape, iters=1):
    frame, centers, cubes = sweep(shape)
    return reference_rows(dense_frames(shape), frame, "given", centers, cubes, iters)


# ---- refinement to the limit ------------------------------------------------------------------------------------------------------------
SLOPE_CUBE, SLOPE_START = (120.0, 120.0, 100.0), (6.0, 19.0, 620.0)


@functools.lru_cache(maxsize=None)
def slope_frame():
    """40 x 52: a wedge that opens from its tip at column 4 towards the right, rows |v - 20| <= (u - 4) / 3, its depth rising 9 mm a column
    and 1 mm a row, over a far plane.  A window of SLOPE_CUBE is about 12 pixels wide and 100 mm deep: from SLOPE_START near the tip every
    window holds more wedge to the right of its centre than to the left, so the centre climbs the slope pass after pass."""
    f = np.full(EVEN, 3000, np.uint16)
    vv, uu = np.mgrid[0:EVEN[0], 0:EVEN[1]]
    m = (uu >= 4) & (3 * np.abs(vv - 20) <= uu - 4)
    f[m] = (600 + 9 * (uu - 4) + vv)[m].astype(np.uint16)
    return _frozen(f)


@functools.lru_cache(maxsize=None)
def slope_reference():
    """-> [(centre, status) of detect(seed="given", iters=i) for i = 0 ... 8]"""
    D = _detect()
    return [D.detect(slope_frame(), seed="given", center=SLOPE_START, cube=SLOPE_CUBE, paras=PARAS, iters=i) for i in range(D.MAX_ITERS + 1)]


# ---- depth bounds -------------------------------------------------------------------------------------------------------------------------
PIXEL = 800                                                                  # a value the depth frame holds: depth_range (PIXEL, PIXEL)
DEPTH_CUBES = ((300.0, 300.0, 300.5), (250.0, 320.0, 120.25), (420.0, 380.0, 0.5), (300.0, 300.0, 99.99))      # fractional depth half-extents


@functools.lru_cache(maxsize=None)
def depth_frame():
    """40 x 52 of known values: random in [300, 1700] with zeros, and 1, 450, 451, 1499, 1500, PIXEL and 65535 at known places"""
    r = np.random.RandomState(31)
    f = r.randint(300, 1701, EVEN).astype(np.uint16)
    f[r.uniform(size=f.shape) < 0.1] = 0
    f[np.isin(f, (450, 1500, PIXEL))] += 2                                     # (these three only where they are put)
    f[3, 5], f[3, 6], f[10, 20], f[10, 21], f[30, 40], f[39, 51] = 450, 451, 1499, 1500, 1, 65535
    f[12:15, 30:34] = PIXEL
    return _frozen(f)


def depth_cases():
    """(seed, depth_range, slab): every range with "range" and with "nearest" at each slab; the last slab of each range is one zmax cuts
    (dmin + slab > zmax)"""
    ranges = {(450.5, 1499.5): (0.0, 0.5, 119.99, 2000.0), (float(PIXEL), float(PIXEL)): (0.0, 0.5, 119.99), (1.0, 65535.0): (0.0, 0.5, 119.99, 70000.0),
              (0.25, 0.75): (0.0, 0.5, 119.99)}
    out = []
    for rng, slabs in ranges.items():
        out.append(("range", rng, 0.0))
        out += [("nearest", rng, s) for s in slabs]
    return out


@functools.lru_cache(maxsize=None)
def depth_reference(seed, rng, slab, iters):
    frame = np.zeros(len(DEPTH_CUBES), np.int64)
    return reference_rows(depth_frame()[None], frame, seed, None, np.array(DEPTH_CUBES), iters, depth_range=rng, slab=slab)


# ---- a large mixed batch ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_batch():
    """320 rows over dense_frames(ODD): duplicate frames, per-row cubes, and the bad indices -1, n and n + 5 in both halves of the batch
    (rows below and above 256) -> (frame (B,), cubes (B, 3))"""
    r = np.random.RandomState(77)
    B = 320
    frame = r.randint(0, N_FRAMES, B).astype(np.int64)
    for b, bad in ((5, -1), (100, N_FRAMES), (255, N_FRAMES + 5), (256, -1), (290, N_FRAMES + 5), (319, N_FRAMES)):
        frame[b] = bad
    cubes = np.stack([r.choice([150.0, 300.0, 420.5], B), r.choice([180.0, 300.0, 333.25], B), r.choice([100.5, 300.0, 400.0], B)], 1)
    return _frozen(frame, cubes)


MIXED_KW = dict(depth_range=(700.0, 1000.5), slab=60.5)


@functools.lru_cache(maxsize=None)
def mixed_reference(seed="nearest", iters=2):
    frame, cubes = mixed_batch()
    return reference_rows(dense_frames(ODD), frame, seed, None, cubes, iters, **MIXED_KW)


# ---- crop-block centres -------------------------------------------------------------------------------------------------------------------
# (cube[0] / 2) / d * fx with cube[0] = 200 and d = 800 is 0.125 * 66 = 8.25 and, in v, 0.125 * 65.5 = 8.1875: dyadic, so us = u - 7.75,
# ue = u + 8.75, vs = v - 7.6875 and ve = v + 8.6875 are exact wherever u and v are multiples of 1 / 16
EXACT_CUBE, EXACT_D, EXACT_HU, EXACT_HV = (200.0, 200.0, 300.0), 800.0, 8.25, 8.1875


def boundary_pairs(shape=ODD):
    """The refusal boundaries of set_crop's window tests, each as a pair of centres (refused, accepted) one pixel apart whose bound is an
    exact integer: -> list of (name, which bound, its value at the refused centre, refused centre, its value at the accepted one, accepted)"""
    fh, fw = shape
    um, vm = 20.0, 16.0
    return [("uend > 0", "ue", 0, (0 - EXACT_HU - 0.5, vm, EXACT_D), 1, (1 - EXACT_HU - 0.5, vm, EXACT_D)),
            ("ustart < fw", "us", fw, (fw + EXACT_HU - 0.5, vm, EXACT_D), fw - 1, (fw - 1 + EXACT_HU - 0.5, vm, EXACT_D)),
            ("vend > 0", "ve", 0, (um, 0 - EXACT_HV - 0.5, EXACT_D), 1, (um, 1 - EXACT_HV - 0.5, EXACT_D)),
            ("vstart < fh", "vs", fh, (um, fh + EXACT_HV - 0.5, EXACT_D), fh - 1, (um, fh - 1 + EXACT_HV - 0.5, EXACT_D))]


def exact_bounds(center, cube=EXACT_CUBE):
    """center2bounds before its int() in rational arithmetic: -> dict us, ue, vs, ve of Fractions"""
    u, v, d = (Fraction(float(x)) for x in center)
    hu = Fraction(float(cube[0])) / 2 / d * Fraction(PARAS[0])
    hv = Fraction(float(cube[1])) / 2 / d * Fraction(PARAS[1])
    half = Fraction(1, 2)
    return dict(us=u - hu + half, ue=u + hu + half, vs=v - hv + half, ve=v + hv + half)


@functools.lru_cache(maxsize=None)
def sample_rows(shape=ODD):
    """-> (centres (B, 3), cubes (B, 3) float64, frame (B,) int64, incoming status (B,) int32, first row of the boundary pairs), B > 256"""
    fh, fw = shape
    nan, inf = float("nan"), float("inf")
    rows = []
    add = lambda c, cube=(300.0, 300.0, 300.0): rows.append((tuple(float(x) for x in c), tuple(float(x) for x in cube)))
    # centres stepped across the four edges in half pixels: far enough out for the small cube's window to leave the frame
    for cube in ((60.0, 60.0, 300.0), (300.0, 300.0, 300.0)):
        for u in np.arange(-5.0, 5.01, 0.5):
            add((u, 16.25, D0), cube)
            add((fw + u, 16.25, D0), cube)
        for v in np.arange(-5.0, 5.01, 0.5):
            add((20.25, v, D0), cube)
            add((20.25, fh + v, D0), cube)
        for t in np.arange(-4.0, 4.01, 1.0):                                  # through the four corners
            for cu, cv, su, sv in ((0, 0, 1, 1), (fw, 0, -1, 1), (0, fh, 1, -1), (fw, fh, -1, -1)):
                add((cu + su * t, cv + sv * t * 0.75, D0), cube)
    # from a window larger than the frame to one of no pixel or one
    for d in (200.0, 300.0, 500.0, 1000.0, 3000.0, 10000.0, 30000.0, 60000.0):
        for u, v in ((20.0, 16.0), (20.4, 16.4), (20.4, 16.0)):
            add((u, v, d))
    # cw or ch so small beside the other that it resizes to nothing: rw = int(cw * 32 / ch)
    for c0 in (5.0, 20.0, 26.0, 45.0, 60.0):
        add((20.4, 16.4, D0), (c0, 500.0, 300.0))
        add((20.4, 16.4, D0), (500.0, c0, 300.0))
    first_pair = len(rows)
    for _, _, _, bad, _, good in boundary_pairs(shape):
        add(bad, EXACT_CUBE)
        add(good, EXACT_CUBE)
    for c in ((nan, 16.0, D0), (20.0, nan, D0), (20.0, 16.0, nan), (nan, nan, nan), (inf, 16.0, D0), (20.0, -inf, D0), (20.0, 16.0, inf),
              (20.0, 16.0, -inf), (20.0, 16.0, 0.0), (20.0, 16.0, -0.0), (0.0, 0.0, 0.0), (20.0, 16.0, -D0), (1e300, 16.0, D0), (3e9, 16.0, D0),
              (20.0, -3e9, D0)):
        add(c)
    add((20.0, 16.0, 0.0), (0.0, 0.0, 300.0))
    add((20.0, 16.0, D0), (0.0, 300.0, 300.0))
    add((20.0, 16.0, D0), (inf, 300.0, 300.0))
    centers, cubes = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    B = len(rows)
    r = np.random.RandomState(5)
    frame = r.randint(0, N_FRAMES, B).astype(np.int64)
    status = np.zeros(B, np.int32)
    # bad frame indices in both workgroups of the launch; incoming codes on windows that hold and on windows refused
    frame[[3, 40, 130, 260, 290, first_pair + 1]] = [-1, N_FRAMES, N_FRAMES + 5, -1, N_FRAMES + 5, N_FRAMES]
    status[[0, 7, 20, 41, 86, 270, first_pair, first_pair + 3, B - 3]] = [EMPTY, EMPTY, BAD_WINDOW, EMPTY, EMPTY, 7, EMPTY, EMPTY, EMPTY]
    return _frozen(centers, cubes, frame, status) + (first_pair,)


@functools.lru_cache(maxsize=None)
def sample_reference(shape=ODD):
    """sample_blocks row by row, then what awr_detect_samples adds to it: a frame index outside the store is BAD_FRAME with no block and a
    NaN matrix, whatever came in; otherwise an incoming code is kept.  -> (blocks or None, M, center_xyz, cube float32, status)"""
    D = _detect()
    centers, cubes, frame, status_in, _ = sample_rows(shape)
    blocks, M, cxyz, cube32, status = D.sample_blocks(centers, cubes, DSIZE, PARAS, FLIP, shape, frames=frame)
    status = np.where(status_in != 0, status_in, status).astype(np.int32)
    for b in np.flatnonzero((frame < 0) | (frame >= N_FRAMES)):
        blocks[b], M[b], status[b] = None, np.nan, BAD_FRAME
    return blocks, M, cxyz, cube32, status


# ---- rendered crops -----------------------------------------------------------------------------------------------------------------------
def render_rows(shape=ODD):
    """windows of about 23 pixels over each edge and corner and inside -> (centres (B, 3), frame (B,))"""
    fh, fw = shape
    cs = [(1.0, 20.0), (fw - 1.5, 20.5), (25.0, 0.5), (25.5, fh - 1.0), (0.5, 0.5), (fw - 1.0, 1.0), (1.0, fh - 0.5), (fw - 0.5, fh - 1.5), (25.0, 20.0),
          (-9.0, 20.0), (fw + 9.5, fh + 8.0), (-14.0, 20.0), (fw + 13.5, fh + 13.0)]          # (the last two: wholly outside, refused)
    return np.array([(u, v, D0 + 7.5 * i) for i, (u, v) in enumerate(cs)]), np.arange(len(cs), dtype=np.int64) % N_FRAMES
