"""Hand detection from a raw depth frame (csrc/awr_detect.hip; include/awr_hip.h "Hand detection on the device").

What lives here: the numpy statements the kernels are tested against bit for bit, one group per entry point, and behind them thin
operator-level wrappers over the entry points for tests and tools.

  * the numpy restatement of the detector -- `center_of_mass`, `detect`, `sample_blocks` -- written to the definition in the header.  It is
    the yardstick of awr_detect and awr_detect_samples, and a usable host fallback for a machine without a GPU;
  * the wrappers (`detect_device`, `palm_device`, `hands_device`, `isolate_device`, `denoise_device`, `samples_device`, `unproject_device`,
    `joints_center_device`, `select_device`, `view_centers_device`, `view_rotate_device`, `fuse_views_device`): they validate, allocate and
    launch through `awr_amd.detect_calls`, where each entry point's argument list is stated once -- the list `awr_amd.predictor.Predictor`,
    the product path, launches through as well;
  * `joints_center` and `select`: the statements of awr_joints_center (predicted joints -> the next crop centre, with a gate) and
    awr_centers_select (a tracked centre where it is usable, the detector's otherwise); DESIGN.md 4.19.
  * `palm_center` and `distance_transform`: the statement of awr_detect_palm (csrc/awr_palm.hip) -- a detector centre ->
    the centre of the palm disc of an exact integer distance transform, which a forearm does not drag up the arm; `palm_device` wraps it.
  * `components` and `hand_seeds`: the statements of awr_detect_hands (csrc/awr_hands.hip) -- the near foreground split
    into 4-connected components with canonical labels, the K nearest large ones seeded per component; `hands_device` wraps it.  With
    `edge` they are the statements of awr_detect_hands_edge: neighbours join only within `edge` millimetres of depth.
    With `link` and `gap` besides they are the statements of awr_detect_hands_link: a rear pixel is joined with the
    first pixel behind at most `gap` occluders, so the fragments a front hand cuts a rear hand into are one component again.
  * `denoise`: the statement of awr_frames_denoise (csrc/awr_denoise.hip) -- an edge-preserving lower median with
    speckle removal and hole filling in front of every stage; `denoise_device` wraps it.
  * `make_views`, `check_views`, `view_table`, `view_centers`, `view_rotate` and `fuse_views`: test-time views -- the host
    table of the views' rotations and the statements of awr_view_centers, awr_view_rotate and awr_views_fuse.

Definition.  Centre of mass of a pixel set: n, sum of columns u, sum of rows v and sum of raw uint16 depths d as int64, centre =
(su / n, sv / n, sd / n) as three double divisions.  Integer sums do not depend on the order of summation, so the device, which splits a
frame over workgroups and combines them with 64-bit integer atomics, gives these bits exactly; that is why frames must be uint16.
Seed: "given" | "range" (pixels of the whole frame with zmin <= d <= zmax) | "nearest" (dmin = smallest such d, then the pixels with
dmin <= d <= min(dmin + slab, zmax)).  Refinement, `iters` times with no convergence test: window and depth range from
nyu_data.center2bounds(centre, cube, paras), clipped to the frame; centre of mass of its pixels with zstart <= d <= zend.  A pixel with
d == 0 never counts.  A pass that finds no pixel makes the centre NaN and the status EMPTY; later passes keep the NaN.
"""
import ctypes as C
import warnings

import numpy as np

from . import nyu_data as ND
from .evaluator import uvd2xyz

OK, EMPTY, BAD_FRAME, BAD_WINDOW = 0, 1, 2, 3
STATUS_NAMES = {OK: "ok", EMPTY: "no pixel in the depth range / window (AWR_DET_EMPTY)", BAD_FRAME: "frame index outside the store (AWR_DET_BAD_FRAME)",
                BAD_WINDOW: "crop window misses the frame or resizes to nothing (AWR_DET_BAD_WINDOW)"}
SEED_GIVEN, SEED_RANGE, SEED_NEAREST = 0, 1, 2
SEEDS = {"given": SEED_GIVEN, "range": SEED_RANGE, "nearest": SEED_NEAREST}
MAX_ITERS = 8
# Engineering defaults, not measured on NYU frames (none are available where this was written): the sensor's useful range, a slab as deep
# as a hand seen end-on, two refinement passes.
DEPTH_RANGE, SLAB, REFINE_ITERS = (1.0, 2000.0), 150.0, 2
_NAN3 = (float("nan"),) * 3
# awr_joints_center's codes (include/awr_hip.h AWR_RECENTER_*)
KEPT_FRAME, MOVED, KEPT_NONFINITE, KEPT_DEPTH, KEPT_SHIFT = 0, 1, 2, 3, 4
RECENTER_NAMES = {KEPT_FRAME: "kept: the frame has a status code", MOVED: "moved", KEPT_NONFINITE: "kept: the joint mean is not finite",
                  KEPT_DEPTH: "kept: the joint mean is outside the depth range", KEPT_SHIFT: "kept: the joint mean is too far from the centre"}
MAX_JOINTS = 256
# test-time views (include/awr_hip.h AWR_VIEWS_MAX, AWR_VIEW_TABLE_DOUBLES, AWR_FUSE_*)
MAX_VIEWS, VIEW_TABLE_DOUBLES = 8, 20
FUSE_MEAN, FUSE_CONF, FUSE_MEDIAN = 0, 1, 2
FUSE_MODES = {"mean": FUSE_MEAN, "conf": FUSE_CONF, "median": FUSE_MEDIAN}


def _u16(frame):
    frame = np.asarray(frame)
    if frame.dtype != np.uint16 or frame.ndim != 2:
        raise ValueError("a frame is a (h, w) uint16 array of millimetres (integer sums make the centre of mass exact), not %s %s"
                         % (frame.dtype, frame.shape))
    return frame


def center_of_mass(frame, window=None, zstart=-np.inf, zend=np.inf):
    """-> ((u, v, d) float64, n).  window = (ustart, uend, vstart, vend), already clipped to the frame (None: the whole frame); pixels with
    zstart <= d <= zend and d != 0 count.  n == 0 -> (nan, nan, nan)."""
    frame = _u16(frame)
    u0, u1, v0, v1 = (0, frame.shape[1], 0, frame.shape[0]) if window is None else window
    if u0 >= u1 or v0 >= v1:
        return _NAN3, 0
    win = frame[v0:v1, u0:u1]
    mask = (win >= zstart) & (win <= zend) & (win != 0)      # uint16 against a float64 scalar compares in float64
    n = int(np.count_nonzero(mask))
    if n == 0:
        return _NAN3, 0
    vv, uu = np.nonzero(mask)
    su = int(uu.astype(np.int64).sum()) + n * u0
    sv = int(vv.astype(np.int64).sum()) + n * v0
    sd = int(win[mask].astype(np.int64).sum())
    return (float(su) / float(n), float(sv) / float(n), float(sd) / float(n)), n


def _window(center, cube, paras, fh, fw):
    """center2bounds clipped to the frame, or None where it has no integer window (a NaN / infinite centre or bound)."""
    try:
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ustart, uend, vstart, vend, zstart, zend = ND.center2bounds(center, cube, paras)
    except (ValueError, OverflowError):
        return None
    if not np.isfinite(center[2]):
        return None
    return (max(ustart, 0), min(uend, fw), max(vstart, 0), min(vend, fh)), zstart, zend


def detect(frame, seed="nearest", center=None, cube=(300, 300, 300), paras=ND.PARAS, depth_range=DEPTH_RANGE, slab=SLAB, iters=REFINE_ITERS):
    """-> ((u, v, d) float64 centre, status).  seed: "given" (centre = `center`) | "range" | "nearest"."""
    frame = _u16(frame)
    fh, fw = frame.shape
    if seed not in SEEDS:
        raise ValueError("seed is one of %s, not %r" % (sorted(SEEDS), seed))
    if not 0 <= int(iters) <= MAX_ITERS:
        raise ValueError("iters = %r is outside [0, %d]" % (iters, MAX_ITERS))
    zmin, zmax = float(depth_range[0]), float(depth_range[1])
    if not zmin <= zmax:
        raise ValueError("depth_range needs zmin <= zmax")
    status = OK
    if seed == "given":
        c = tuple(float(x) for x in center)
    else:
        if seed == "nearest":
            m = (frame >= zmin) & (frame <= zmax) & (frame != 0)
            if m.any():
                dmin = float(frame[m].min())
                c, n = center_of_mass(frame, None, dmin, min(dmin + float(slab), zmax))
            else:
                c, n = _NAN3, 0
        else:
            c, n = center_of_mass(frame, None, zmin, zmax)
        if n == 0:
            status = EMPTY
    for _ in range(int(iters)):
        w = _window(c, cube, paras, fh, fw)
        c, n = center_of_mass(frame, *w) if w is not None else (_NAN3, 0)
        if n == 0:
            status = EMPTY
    return c, status


def sample_blocks(centers, cube, dsize, paras=ND.PARAS, flip=-1, frame_shape=(480, 640), frames=None):
    """The host's blocks for float64 centres: -> (list of L.NyuSample or None where set_crop refuses the window, M (B, 3, 3) float32 (NaN there),
    center_xyz (B, 3) float32, cube (B, 3) float32, status (B,) int32).  What awr_detect_samples is tested against."""
    from . import _lib as L
    from . import nyu_device as DV
    centers = np.asarray(centers, np.float64).reshape(-1, 3)
    B = centers.shape[0]
    cubes = np.broadcast_to(np.asarray(cube, np.float64), (B, 3))
    fh, fw = frame_shape
    blocks, M, status = [], np.full((B, 3, 3), np.nan, np.float32), np.zeros(B, np.int32)
    for b in range(B):
        blk = L.NyuSample()
        try:
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                M[b] = DV.set_crop(blk, b if frames is None else frames[b], centers[b], cubes[b], (dsize, dsize), paras, fh, fw)
            DV.set_normalize(blk, centers[b], cubes[b])
            blocks.append(blk)
        except (ValueError, OverflowError, ZeroDivisionError):
            blocks.append(None)
            status[b] = BAD_WINDOW
    with np.errstate(all="ignore"):
        cxyz = uvd2xyz(centers, paras, flip)
    return blocks, M, cxyz, np.ascontiguousarray(cubes, dtype=np.float32), status      # (cubes may be a broadcast view: stride 0)


def joints_center(xyz, center_uvd, center_xyz, cube, status, ustatus, paras, flip, joints=None, depth_range=DEPTH_RANGE, max_shift=1.0):
    """The statement of awr_joints_center (include/awr_hip.h): predicted joints -> the next crop centre, per frame, with a gate.
    xyz (B, J, 3) float32 camera mm; center_uvd (B, 3) float64, the centres this pass was cropped at; center_xyz, cube (B, 3) float32;
    status, ustatus (B,) the detector's and the un-projection's codes; joints: indices into [0, J) (None: all of them).
    -> (center_out (B, 3) float64: the new centre where MOVED, center_uvd's row otherwise; next (B, 3): the new centre where MOVED, NaN
    otherwise; code (B,) int32).  An explicit loop in IEEE double, in the header's order."""
    xyz = np.asarray(xyz, np.float32)
    B, J = xyz.shape[0], xyz.shape[1]
    center_uvd = np.asarray(center_uvd, np.float64).reshape(B, 3)
    center_xyz, cube = np.asarray(center_xyz, np.float32).reshape(B, 3), np.asarray(cube, np.float32).reshape(B, 3)
    sel = list(range(J)) if joints is None or len(joints) == 0 else [int(j) for j in joints]
    fx, fy, u0, v0 = (np.float64(p) for p in paras)
    zmin, zmax, max_shift, fl = np.float64(depth_range[0]), np.float64(depth_range[1]), np.float64(max_shift), np.float64(flip)
    if not (1 <= J <= MAX_JOINTS and len(sel) <= J and int(flip) in (1, -1) and zmin <= zmax and max_shift >= 0):
        raise ValueError("joints_center: J in [1, %d], at most J indices, flip = +-1, zmin <= zmax and max_shift >= 0 are required" % MAX_JOINTS)
    out, nxt, code = center_uvd.copy(), np.full((B, 3), np.nan), np.zeros(B, np.int32)
    with np.errstate(all="ignore"):
        for b in range(B):
            if status[b] != 0 or ustatus[b] != 0:
                code[b] = KEPT_FRAME
                continue
            m, in_range = [np.float64(0.0)] * 3, True
            for j in sel:
                if not 0 <= j < J:
                    in_range = False
                    break
                m = [m[a] + np.float64(xyz[b, j, a]) for a in range(3)]
            m = [m[a] / np.float64(len(sel)) for a in range(3)]
            if not in_range or not all(np.isfinite(m)):
                code[b] = KEPT_NONFINITE
            elif not (zmin <= m[2] <= zmax):
                code[b] = KEPT_DEPTH
            elif not all(abs(m[a] - np.float64(center_xyz[b, a])) <= max_shift * (np.float64(cube[b, a]) / np.float64(2.0)) for a in range(3)):
                code[b] = KEPT_SHIFT
            else:
                code[b] = MOVED
                y = m[1] * fl                                         # evaluator.xyz2uvd (util.py:3-10), kept in double
                nxt[b] = (m[0] * fx / m[2] + u0, y * fy / m[2] + v0, m[2])
                out[b] = nxt[b]
    return out, nxt, code


def select(a_center, a_status, b_center, b_status):
    """The statement of awr_centers_select: per frame `a` where a_status == OK and a's centre is finite, otherwise `b` with b's status.
    -> (center (B, 3) float64, status (B,) int32, which (B,) int32: 0 = a, 1 = b)."""
    a_center, b_center = np.asarray(a_center, np.float64).reshape(-1, 3), np.asarray(b_center, np.float64).reshape(-1, 3)
    a_status, b_status = np.asarray(a_status, np.int32), np.asarray(b_status, np.int32)
    B = a_center.shape[0]
    out, status, which = b_center.copy(), b_status.copy(), np.ones(B, np.int32)
    for b in range(B):
        if a_status[b] == OK and all(np.isfinite(a_center[b])):
            out[b], status[b], which[b] = a_center[b], a_status[b], 0
    return out, status, which


# ---- forearm-robust palm centre from an exact distance transform (include/awr_hip.h awr_detect_palm) -------------------
# Integers only: with frame sides up to PALM_MAX_SIDE = 16384, D2 <= 2^28, L <= 2^29, |t|, |s| <= 2^30, so s * s <= 2^60, m * L <= 2^57 and
# tau * D2, rho2 * |p - p*|^2 (tau, rho2 below 2^31) <= 2^60: every product stays below 2^62 in int64.
PALM_SEARCH, PALM_TAU, PALM_RHO2, PALM_MAX_SIDE = 2.0, (1, 3), (25, 4), 16384
_NO_INFO = (-1, -1, 0, 0)


def _ratio(x, what, order):
    """(a, b) ints in [1, 2^31): order "le" needs a <= b (tau), "ge" needs a >= b (rho2)"""
    if isinstance(x, (str, bytes)) or not hasattr(x, "__len__") or len(x) != 2 or any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) for t in x):
        raise TypeError("%s is a pair of ints (numerator, denominator), not %r" % (what, x))
    a, b = int(x[0]), int(x[1])
    if not (0 < a < 2 ** 31 and 0 < b < 2 ** 31 and (a <= b if order == "le" else a >= b)):
        raise ValueError("%s = %r needs %s, both below 2^31" % (what, x, "0 < %s[0] <= %s[1]" % (what, what) if order == "le" else "0 < %s[1] <= %s[0]" % (what, what)))
    return a, b


def check_palm(search=PALM_SEARCH, tau=PALM_TAU, rho2=PALM_RHO2):
    """Validate palm_center's three knobs: -> (search float, (tau0, tau1), (rho0, rho1))."""
    search = _number(search, "search")
    if not search > 0.0:
        raise ValueError("search = %r must be > 0" % (search,))
    return search, _ratio(tau, "tau", "le"), _ratio(rho2, "rho2", "ge")


def distance_transform(mask):
    """Exact squared Euclidean distance transform of a (h, w) boolean window, int64: D2(p) = min over background q of |p - q|^2, where
    everything outside the window -- the one-pixel ring around it and beyond -- is background; 0 on background.  Two passes: g, the
    distance along the column to the nearest background row (the ring rows count), then D2(v, u) = min over u' of (u - u')^2 + g(v, u')^2
    (g = 0 on the ring columns and beyond).  Only |u - u'| < max g can lower a pixel's own g^2, and rows without foreground stay 0."""
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    g = np.zeros((h, w), np.int64)
    run = np.zeros(w, np.int64)
    for i in range(h):
        run = np.where(mask[i], run + 1, 0)
        g[i] = run
    run = np.zeros(w, np.int64)
    for i in range(h - 1, -1, -1):
        run = np.where(mask[i], run + 1, 0)
        np.minimum(g[i], run, out=g[i])
    d2 = g * g
    rows = np.nonzero(mask.any(axis=1))[0]
    if rows.size:
        gm = int(g.max())
        G = np.zeros((rows.size, w + 2 * gm), np.int64)
        G[:, gm:gm + w] = d2[rows]
        best = d2[rows]
        for k in range(1, gm):
            np.minimum(best, G[:, gm - k:gm - k + w] + k * k, out=best)
            np.minimum(best, G[:, gm + k:gm + k + w] + k * k, out=best)
        d2[rows] = best
    return d2


def _first_argmax(values, where):
    """(row, col) of the first maximum of the non-negative `values` over `where`, in raster order"""
    return np.unravel_index(int(np.argmax(np.where(where, values, -1))), values.shape)


def palm_center(frame, center, status=OK, cube=(300, 300, 300), paras=ND.PARAS, depth_range=DEPTH_RANGE, search=PALM_SEARCH, tau=PALM_TAU,
                rho2=PALM_RHO2):
    """The statement of awr_detect_palm (include/awr_hip.h): a detector centre -> the centre of the palm disc, which a
    forearm does not drag up the arm.  -> ((u, v, d) float64, status, info = (pu, pv, r2, n_disc) ints: the palm point in frame pixels,
    its squared distance to the background and the pixels of the disc; (-1, -1, 0, 0) where there is none).
      1. status != OK: centre and status pass through.
      2. window W = center2bounds(centre, search * cube, paras) clipped to the frame; mask = pixels of W with d != 0 whose depth lies in
         that call's [zstart, zend] and in depth_range.  No window or no pixel: NaN, EMPTY.
      3. D2 = distance_transform(mask).     4. m = max D2; S = {tau[1] * D2 >= tau[0] * m}, the medial set.
      5. every argmax takes the first maximum in raster order: e0 = argmax_S D2, e1 = argmax_S |p - e0|^2, e2 = argmax_S |p - e1|^2,
         a = e2 - e1, L = |a|^2.
      6. L == 0: p* = e0.  Otherwise t(p) = (p - e1) . a, b1 = mask pixels with t < 0, b2 = mask pixels with t > L (what lies beyond
         either end: fingers beyond the hand's), s = L - t if b2 >= b1 else t, N = {p in S: s <= 0 or s * s <= m * L}, p* = argmax_N D2.
      7. r2 = D2(p*); disc = mask pixels with rho2[1] * |p - p*|^2 <= rho2[0] * r2; centre = (su / n, sv / n, sd / n) of the disc.
    All arithmetic is int64 up to the last three double divisions."""
    frame = _u16(frame)
    fh, fw = frame.shape
    if fh > PALM_MAX_SIDE or fw > PALM_MAX_SIDE:
        raise ValueError("a frame of %d x %d is outside [1, %d]^2" % (fh, fw, PALM_MAX_SIDE))
    search, (tau0, tau1), (rho0, rho1) = check_palm(search, tau, rho2)
    zmin, zmax = float(depth_range[0]), float(depth_range[1])
    if not zmin <= zmax:
        raise ValueError("depth_range needs zmin <= zmax")
    c = tuple(float(x) for x in center)
    if int(status) != OK:
        return c, int(status), _NO_INFO
    w = _window(c, tuple(search * float(x) for x in cube), paras, fh, fw)
    if w is None or w[0][0] >= w[0][1] or w[0][2] >= w[0][3]:
        return _NAN3, EMPTY, _NO_INFO
    (u0, u1, v0, v1), zstart, zend = w
    win = frame[v0:v1, u0:u1]
    mask = (win >= zstart) & (win <= zend) & (win >= zmin) & (win <= zmax) & (win != 0)
    if not mask.any():
        return _NAN3, EMPTY, _NO_INFO
    D2 = distance_transform(mask)
    m = int(D2.max())
    S = tau1 * D2 >= tau0 * m
    vv, uu = np.indices(mask.shape, dtype=np.int64)
    e0 = _first_argmax(D2, S)
    e1 = _first_argmax((vv - e0[0]) ** 2 + (uu - e0[1]) ** 2, S)
    e2 = _first_argmax((vv - e1[0]) ** 2 + (uu - e1[1]) ** 2, S)
    av, au = int(e2[0]) - int(e1[0]), int(e2[1]) - int(e1[1])
    L = av * av + au * au
    if L == 0:
        pv, pu = int(e0[0]), int(e0[1])
    else:
        t = (vv - e1[0]) * av + (uu - e1[1]) * au
        b1, b2 = int(np.count_nonzero(mask & (t < 0))), int(np.count_nonzero(mask & (t > L)))
        s = L - t if b2 >= b1 else t
        N = S & ((s <= 0) | (s * s <= m * L))
        pv, pu = (int(x) for x in _first_argmax(D2, N))
    r2 = int(D2[pv, pu])
    disc = mask & (rho1 * ((vv - pv) ** 2 + (uu - pu) ** 2) <= rho0 * r2)
    n = int(np.count_nonzero(disc))
    su, sv = int(uu[disc].sum()) + n * u0, int(vv[disc].sum()) + n * v0
    sd = int(win[disc].astype(np.int64).sum())
    return (float(su) / float(n), float(sv) / float(n), float(sd) / float(n)), OK, (pu + u0, pv + v0, r2, n)


# ---- several hands per frame from connected components (include/awr_hip.h awr_detect_hands) ---------------------------
# Engineering defaults, not measured on real frames (none are available where this was written): at most four hands, a mask as deep as an
# arm's reach behind the nearest pixel, and a component of fewer than 400 pixels (a 20 x 20 patch; a hand at 1.5 m covers some 2000) is
# debris, not a hand.
MAX_HANDS, REACH, MIN_PIXELS = 4, 300.0, 400
# links across an occluder: a walk crosses at most LINK_GAP occluders unless told otherwise -- an engineering choice,
# UNMEASURED on real frames -- and never more than MAX_GAP (AWR_HANDS_MAX_GAP)
LINK_GAP, MAX_GAP = 32, 64


def _check_hands(hands, reach, slab, min_pixels):
    if isinstance(hands, bool) or not isinstance(hands, (int, np.integer)):
        raise TypeError("hands is an int in [1, %d], not %r" % (MAX_HANDS, hands))
    if not 1 <= int(hands) <= MAX_HANDS:
        raise ValueError("hands = %d is outside [1, %d]" % (hands, MAX_HANDS))
    if isinstance(min_pixels, bool) or not isinstance(min_pixels, (int, np.integer)):
        raise TypeError("min_pixels is an int >= 1, not %r" % (min_pixels,))
    if int(min_pixels) < 1:
        raise ValueError("min_pixels = %d must be at least 1" % min_pixels)
    for x, what in ((reach, "reach"), (slab, "slab")):
        if isinstance(x, (bool, str, bytes)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise TypeError("%s is a number of millimetres >= 0, not %r" % (what, x))
        if not float(x) >= 0.0:
            raise ValueError("%s = %r must be >= 0" % (what, x))
    return int(hands), float(reach), float(slab), int(min_pixels)


def _check_edge(edge, value=True):
    """edge: None (no depth test on the join) | a number of millimetres >= 0, infinity allowed, NaN not -> None | float.  value=False
    checks the type alone (hands_device: a value the entry point refuses gets its message from there)."""
    if edge is None:
        return None
    if isinstance(edge, (bool, str, bytes)) or not isinstance(edge, (int, float, np.integer, np.floating)):
        raise TypeError("edge is None or a number of millimetres >= 0, not %r" % (edge,))
    if value and not float(edge) >= 0.0:
        raise ValueError("edge = %r must be >= 0 (infinity: no depth test)" % (edge,))
    return float(edge)


def _check_link(link, gap=LINK_GAP, edge=None, value=True):
    """link: None (no links: `gap` is not looked at) | a number of millimetres >= 0, infinity allowed, NaN not; gap: an int in
    [1, MAX_GAP] -> (None | float, int).  A link needs an edge: without one no pixel is an occluder.  value=False checks the types alone
    (hands_device: a value the entry point refuses gets its message from there)."""
    if link is None:
        return None, LINK_GAP
    if isinstance(link, (bool, str, bytes)) or not isinstance(link, (int, float, np.integer, np.floating)):
        raise TypeError("link is None or a number of millimetres >= 0, not %r" % (link,))
    if isinstance(gap, bool) or not isinstance(gap, (int, np.integer)):
        raise TypeError("gap is an int in [1, %d], not %r" % (MAX_GAP, gap))
    if edge is None:
        raise ValueError("link = %r needs an edge: an occluder is a pixel more than `edge` millimetres nearer" % (link,))
    if value and not float(link) >= 0.0:
        raise ValueError("link = %r must be >= 0 (infinity: any two depths agree)" % (link,))
    if value and not 1 <= int(gap) <= MAX_GAP:
        raise ValueError("gap = %d is outside [1, %d]" % (gap, MAX_GAP))
    return float(link), int(gap)


def _links(frame, mask, edge, link, gap):
    """The links of `components`: -> (p, q) int64 raster indices, a pair per link.  One pass per direction and step t over shifted views:
    `walking` holds the mask pixels whose q_1 ... q_{t-1} were all occluders; those whose q_t lies outside the frame stop (nothing), those
    whose q_t is an occluder go on (past t = gap + 1: nothing), and the others end at q = q_t -- a link when t >= 2, q is in the mask and
    |d_q - d_p| <= link."""
    fh, fw = frame.shape
    d = frame.astype(np.float64)
    index = np.arange(fh * fw, dtype=np.int64).reshape(fh, fw)
    ps, qs = [], []
    for axis, forward in ((1, True), (1, False), (0, True), (0, False)):          # right, left, down, up
        n = frame.shape[axis]
        walking = mask
        for t in range(1, min(gap + 1, n - 1) + 1):
            near, far = slice(0, n - t), slice(t, n)
            sp, sq = (near, far) if forward else (far, near)
            sp, sq = ((slice(None), sp), (slice(None), sq)) if axis == 1 else ((sp, slice(None)), (sq, slice(None)))
            occluder = (d[sq] != 0) & (d[sp] - d[sq] > edge)
            if t >= 2:
                hit = walking[sp] & ~occluder & mask[sq] & (np.abs(d[sq] - d[sp]) <= link)
                ps.append(index[sp][hit])
                qs.append(index[sq][hit])
            on = np.zeros((fh, fw), bool)
            on[sp] = walking[sp] & occluder
            walking = on
            if not walking.any():
                break
    return np.concatenate(ps) if ps else np.zeros(0, np.int64), np.concatenate(qs) if qs else np.zeros(0, np.int64)


def components(frame, depth_range=DEPTH_RANGE, reach=REACH, edge=None, link=None, gap=LINK_GAP):
    """-> labels (fh, fw) int32.  Foreground: zmin <= d <= zmax and d != 0; dmin its smallest depth; the mask is the foreground with
    d <= min(dmin + reach, zmax) (float64 comparisons, as in `detect`).  Two mask pixels are connected when they are 4-neighbours -- no
    depth test.  A pixel's label is the smallest raster index v * fw + u of its component, -1 on background: canonical, so any correct
    algorithm gives these integers.  Here: the rows' runs, joined where the runs of two neighbouring rows share a column.
    edge: a number of millimetres -- two mask pixels are JOINED when they are 4-neighbours and |d_a - d_b| <= edge, the
    raw depths compared as float64, and the components are the transitive closure of that (a ramp of small steps is one component).
    Then a run also starts where the left neighbour is in the mask but more than `edge` away in depth, and a vertical pair joins two
    runs only if the two pixels pass the test.  An edge of 65535 or more gives the labels of edge=None.
    link, gap (only with edge): the components are the transitive closure of the joins above AND of these links.  For
    every mask pixel p (raw depth d_p) and each of the four directions (right, left, down, up), q_t being the pixel t steps from p:
      1. a pixel o is an OCCLUDER of p when d_o != 0 and d_p - d_o > edge.  Raw depths only: o need not lie in the mask and may be nearer
         than zmin;
      2. n is the number of consecutive occluders q_1 ... q_n, counted up to gap.  Nothing happens when n == 0, when q_1 ... q_gap and
         q_{gap+1} are all occluders, or when the walk leaves the frame before it ends;
      3. otherwise q = q_{n+1} is the first pixel that is no occluder, 1 <= n <= gap; when q is a mask pixel and |d_q - d_p| <= link
         (float64), p and q are joined.
    The test is p's alone: one direction of a pair may hold and the other not; either one joins.  A zero pixel inside the gap is no
    occluder and ends the walk, so sensor shadows break links.  An edge of 65535 or more makes no pixel an occluder: the labels of
    edge=None.  Two DIFFERENT hands at similar depth with a nearer object between them, gap pixels or fewer wide, are linked.
    link=None: no links.  A link without an edge raises ValueError."""
    frame = _u16(frame)
    edge = _check_edge(edge)
    link, gap = _check_link(link, gap, edge)
    fh, fw = frame.shape
    zmin, zmax = float(depth_range[0]), float(depth_range[1])
    if not zmin <= zmax:
        raise ValueError("depth_range needs zmin <= zmax")
    if not float(reach) >= 0.0:
        raise ValueError("reach = %r must be >= 0" % (reach,))
    labels = np.full((fh, fw), -1, np.int32)
    fg = (frame >= zmin) & (frame <= zmax) & (frame != 0)
    if not fg.any():
        return labels
    dmin = float(frame[fg].min())
    mask = fg & (frame <= min(dmin + float(reach), zmax))
    # a run starts where a mask pixel has no mask pixel to its left; runs are numbered in raster order, so a smaller number is a smaller
    # first index, and the smallest run of a component starts at the component's smallest index
    start = mask.copy()
    both = mask[:-1] & mask[1:]
    if edge is None:
        start[:, 1:] &= ~mask[:, :-1]
    else:
        d = frame.astype(np.float64)
        start[:, 1:] &= ~(mask[:, :-1] & (np.abs(d[:, 1:] - d[:, :-1]) <= edge))
        both &= np.abs(d[1:] - d[:-1]) <= edge
    run = np.cumsum(start.ravel()).reshape(fh, fw) - 1          # on a mask pixel: the number of its own run
    first = np.flatnonzero(start.ravel())
    parent = np.arange(first.size)
    pairs = run[:-1][both].astype(np.int64) * first.size + run[1:][both]
    if link is not None:                                          # a link joins the runs of its two pixels, as a vertical pair does
        lp, lq = _links(frame, mask, edge, link, gap)
        pairs = np.concatenate([pairs, run.ravel()[lp].astype(np.int64) * first.size + run.ravel()[lq]])
    pairs = np.unique(pairs)
    p = parent.tolist()
    for a, b in zip((pairs // first.size).tolist(), (pairs % first.size).tolist()):
        while p[a] != a:
            p[a] = p[p[a]]
            a = p[a]
        while p[b] != b:
            p[b] = p[p[b]]
            b = p[b]
        if a < b:
            p[b] = a
        elif b < a:
            p[a] = b
    parent = np.asarray(p, np.int64)
    while True:
        up = parent[parent]
        if np.array_equal(up, parent):
            break
        parent = up
    labels[mask] = first[parent[run[mask]]]
    return labels


def hand_seeds(frame, hands, depth_range=DEPTH_RANGE, reach=REACH, slab=SLAB, min_pixels=MIN_PIXELS, edge=None, link=None, gap=LINK_GAP):
    """The statement of awr_detect_hands (edge=None), awr_detect_hands_edge (edge: `components`' depth test on the join) and
    awr_detect_hands_link (link, gap: `components`' links across an occluder; everything below reads its labels) for one frame: -> (centers (K, 3) float64, status (K,) int32, info (K, 4) int32, count).
    Candidates: the components of `components` with n >= min_pixels pixels; a candidate's key is (zc, root), zc its smallest raw depth
    and root its label; the K = hands smallest keys fill the slots in ascending order (slot 0: the nearest hand; a tie in depth goes to
    the smaller root).  A slot's seed is the centre of mass of its component's pixels with d <= min(zc + slab, zmax) -- the "nearest"
    rule per component, int64 sums and three double divisions as center_of_mass does; status OK; info = (root % fw, root // fw, n, zc).
    Slots past the candidates: NaN, EMPTY, (-1, -1, 0, 0).  count: the number of candidates, which may exceed K.  A seed is then refined
    by detect(seed="given", center=...), unchanged."""
    K, reach, slab, min_pixels = _check_hands(hands, reach, slab, min_pixels)
    frame = _u16(frame)
    fw = frame.shape[1]
    zmax = float(depth_range[1])
    labels = components(frame, depth_range, reach, edge, link, gap)
    centers, status, info = np.full((K, 3), np.nan), np.full(K, EMPTY, np.int32), np.tile(np.array(_NO_INFO, np.int32), (K, 1))
    on = labels >= 0
    if not on.any():
        return centers, status, info, 0
    roots, inv, n = np.unique(labels[on], return_inverse=True, return_counts=True)
    zc = np.full(roots.size, 65536, np.int64)
    np.minimum.at(zc, inv.ravel(), frame[on].astype(np.int64))
    cand = np.flatnonzero(n >= min_pixels)
    cand = cand[np.lexsort((roots[cand], zc[cand]))]
    for k, i in enumerate(cand[:K].tolist()):
        root = int(roots[i])
        c, _ = center_of_mass(np.where(labels == root, frame, np.uint16(0)), None, -np.inf, min(float(zc[i]) + slab, zmax))
        centers[k], status[k], info[k] = c, OK, (root % fw, root // fw, int(n[i]), int(zc[i]))
    return centers, status, info, int(cand.size)


def isolate(frame, labels, roots):
    """The statement of awr_hands_isolate for one frame: -> (K, fh, fw) uint16, a frame per hand slot that holds only the slot's own
    component.  labels: `components`' (fh, fw) int32; roots: (K,) ints, slot k's root = info[1] * fw + info[0] of the info
    row hand_seeds returns, negative for an EMPTY slot.  Output k equals the frame with every pixel set to 0 where labels >= 0 and
    labels != roots[k]; when roots[k] < 0, output k is the unchanged frame.  Unlabelled pixels stay: background, depth 0, and foreground
    beyond dmin + reach.  Debris components below min_pixels are labelled, so they are removed from EVERY hand's frame."""
    frame = _u16(frame)
    labels = np.asarray(labels)
    roots = np.asarray(roots)
    if labels.shape != frame.shape or labels.dtype.kind != "i":
        raise ValueError("labels must be integers of the frame's shape %s, got %s %s" % (frame.shape, labels.dtype, labels.shape))
    if roots.ndim != 1 or roots.dtype.kind != "i" or not 1 <= roots.size <= MAX_HANDS:
        raise ValueError("roots must be 1 ... %d integers, got %s %s" % (MAX_HANDS, roots.dtype, roots.shape))
    out = np.repeat(frame[None], roots.size, 0)
    for k, root in enumerate(roots.tolist()):
        if root >= 0:
            out[k][(labels >= 0) & (labels != root)] = 0
    return out


# ---- edge-preserving depth pre-filter in front of the detector (include/awr_hip.h awr_frames_denoise) -----------------
# Engineering choices, not measured on real frames (none are available where this was written): a 3 x 3 window, the 40 mm edge DESIGN.md
# 4.29 measured on procedural composites, no speckle removal and no hole filling -- a pure edge-preserving median.
DENOISE_DEFAULTS = dict(radius=1, edge=40.0, support=0, fill=None)
DENOISE_MAX_RADIUS = 2


def _check_denoise(radius=1, edge=None, support=0, fill=None, value=True):
    """Validate denoise's four knobs: -> (radius int, edge None | float, support int, fill None | int).  value=False checks the types
    alone (denoise_device: a value the entry point refuses gets its message from there)."""
    for x, what in ((radius, "radius"), (support, "support")) + (((fill, "fill"),) if fill is not None else ()):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise TypeError("%s is an int%s, not %r" % (what, " or None" if what == "fill" else "", x))
    most = (2 * int(radius) + 1) ** 2 - 1
    if value and not 1 <= int(radius) <= DENOISE_MAX_RADIUS:
        raise ValueError("radius = %d must be 1 or 2 (a 3 x 3 or a 5 x 5 window)" % radius)
    if value and not 0 <= int(support) <= most:
        raise ValueError("support = %d is outside [0, %d], the neighbours of a radius-%d window" % (support, most, radius))
    if value and fill is not None and not 1 <= int(fill) <= most:
        raise ValueError("fill = %d is outside [1, %d], the neighbours of a radius-%d window (None: no filling)" % (fill, most, radius))
    return int(radius), _check_edge(edge, value), int(support), None if fill is None else int(fill)


def check_denoise_option(denoise):
    """Predictor(denoise=...) and FrameStore.denoised(**options): None | True (DENOISE_DEFAULTS) | a dict with any of the keys radius /
    edge / support / fill over those defaults -> None | a dict of the four checked values."""
    if denoise is None:
        return None
    if denoise is True:
        denoise = {}
    if not isinstance(denoise, dict):
        raise TypeError("denoise is None, True or a dict with the keys radius / edge / support / fill, not %r" % (denoise,))
    extra = set(denoise) - set(DENOISE_DEFAULTS)
    if extra:
        raise ValueError("denoise has unknown keys %s (radius, edge, support and fill exist)" % sorted(extra))
    return dict(zip(("radius", "edge", "support", "fill"), _check_denoise(**dict(DENOISE_DEFAULTS, **denoise))))


def denoise(frame, radius=1, edge=None, support=0, fill=None):
    """The statement of awr_frames_denoise for one frame: -> (fh, fw) uint16.  The rule:

    Every output pixel is a function of the INPUT frame alone. It is a single pass: not iterated, not in place.
    Definitions for pixel p with depth d_p:
      - W is the set of in-frame pixels of the (2 * radius + 1)^2 window around p, without p itself.
      - elim = 65535 for edge=None, else floor(min(edge, 65535)). This is awr_frame.h's depth_floor, the integer form 4.29 already uses.
      - A pixel is valid when its depth is not 0.
      - The lower median of n values is element (n - 1) // 2 of the ascending sort. It is a value that occurs in the window, never an
        average.
    Output:
      - If d_p != 0: let S = { q in W : d_q != 0 and |d_q - d_p| <= elim }.
          - If |S| < support the output is 0. This removes a flying pixel or speckle.
          - Otherwise the output is the lower median of S and p together, which is element |S| // 2 of its sort.
      - If d_p == 0: let V = { q in W : d_q != 0 }.
          - If fill is given and |V| >= fill, the output is the lower median of V.
          - Otherwise the output is 0.
    Out-of-frame positions and zero pixels are indistinguishable under this rule, because both thresholds are absolute counts. The frame
    behaves as if surrounded by zeros, and the kernel may stage its halo that way.

    Here: the window as zero-padded shifts of the frame, the pixels that do not count replaced by a sentinel above every depth, one sort
    along the window axis and one take_along_axis."""
    frame = _u16(frame)
    r, edge, support, fill = _check_denoise(radius, edge, support, fill)
    elim = 65535 if edge is None else int(np.floor(min(edge, 65535.0)))
    fh, fw = frame.shape
    padded = np.zeros((fh + 2 * r, fw + 2 * r), np.int32)
    padded[r:r + fh, r:r + fw] = frame
    shifts = [(dv, du) for dv in range(2 * r + 1) for du in range(2 * r + 1) if (dv, du) != (r, r)]
    win = np.stack([padded[dv:dv + fh, du:du + fw] for dv, du in shifts])          # W, one plane per neighbour
    d = frame.astype(np.int32)
    seen = d != 0
    counts = (win != 0) & (~seen | (np.abs(win - d) <= elim))                        # S where d_p != 0, V where it is 0
    n = counts.sum(0)
    keys = np.concatenate([np.where(counts, win, 65536), np.where(seen, d, 65536)[None]])
    keys.sort(axis=0)
    k = np.where(seen, n // 2, np.maximum(n - 1, 0) // 2)
    median = np.take_along_axis(keys, k[None], 0)[0]
    keep = np.where(seen, n >= support, (n >= fill) if fill is not None else False)
    return np.where(keep, median, 0).astype(np.uint16)


# ---- test-time views: the same hand under rotations, cube scales and centre shifts ----------------------------------
def _number(x, what):
    if isinstance(x, (bool, str, bytes)) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise TypeError("%s is a number, not %r" % (what, x))
    x = float(x)
    if not np.isfinite(x):
        raise ValueError("%s = %r is not finite" % (what, x))
    return x


def check_views(views, fuse="mean"):
    """Validate what Predictor(views=..., fuse=...) is handed: -> a list of (rot, scale, (sx, sy, sz)) floats.  views: 2 ... MAX_VIEWS views,
    each a dict with any of the keys rot / scale / shift or a (rot, scale, shift) tuple; view 0 must be the identity."""
    if fuse not in FUSE_MODES:
        raise ValueError("fuse is one of %s, not %r" % (sorted(FUSE_MODES), fuse))
    if isinstance(views, (str, bytes, dict)) or not hasattr(views, "__len__"):
        raise TypeError("views is a sequence of views (awr_amd.detect.make_views builds one), not %r" % (views,))
    if not 2 <= len(views) <= MAX_VIEWS:
        raise ValueError("views holds %d views: 2 ... %d are possible (views=None predicts from the one identity view)" % (len(views), MAX_VIEWS))
    out = []
    for i, v in enumerate(views):
        if isinstance(v, dict):
            extra = set(v) - {"rot", "scale", "shift"}
            if extra:
                raise ValueError("view %d has unknown keys %s (rot, scale and shift exist)" % (i, sorted(extra)))
            rot, scale, shift = v.get("rot", 0.0), v.get("scale", 1.0), v.get("shift", (0.0, 0.0, 0.0))
        elif isinstance(v, (tuple, list)) and len(v) == 3:
            rot, scale, shift = v
        else:
            raise TypeError("view %d is a dict or a (rot, scale, shift) tuple, not %r" % (i, v))
        rot, scale = _number(rot, "view %d: rot" % i), _number(scale, "view %d: scale" % i)
        if not scale > 0.0:
            raise ValueError("view %d: scale = %r must be > 0" % (i, scale))
        if isinstance(shift, (str, bytes)) or not hasattr(shift, "__len__") or len(shift) != 3:
            raise TypeError("view %d: shift is 3 numbers (camera millimetres), not %r" % (i, shift))
        shift = tuple(_number(x, "view %d: shift" % i) for x in shift)
        out.append((rot, scale, shift))
    if out[0] != (0.0, 1.0, (0.0, 0.0, 0.0)):
        raise ValueError("view 0 must be the identity (rot = 0, scale = 1, shift = 0): center_xyz, M and status of a prediction are its, got %r"
                         % (out[0],))
    return out


def make_views(rot=(), scale=(), shift=()):
    """The identity view, then one view per rotation (degrees), per cube scale and per centre shift (3 camera millimetres each):
    make_views(rot=(-15, 15), scale=(0.9, 1.1)) -> five views, as a list of dicts for Predictor(views=...)."""
    views = [dict(rot=0.0, scale=1.0, shift=(0.0, 0.0, 0.0))]
    views += [dict(rot=r, scale=1.0, shift=(0.0, 0.0, 0.0)) for r in rot]
    views += [dict(rot=0.0, scale=s, shift=(0.0, 0.0, 0.0)) for s in scale]
    views += [dict(rot=0.0, scale=1.0, shift=tuple(t) if hasattr(t, "__len__") else t) for t in shift]
    return [dict(rot=r, scale=s, shift=t) for r, s, t in check_views(views)]


def parse_views(spec):
    """predict.py's --views: "rot=-15,15;scale=0.9,1.1;shift=0:0:10,5:0:0" -> make_views(...) (a shift is three numbers joined by colons)"""
    kw = {}
    for part in filter(None, (p.strip() for p in spec.split(";"))):
        key, _, vals = part.partition("=")
        key = key.strip()
        if key not in ("rot", "scale", "shift") or key in kw or not vals.strip():
            raise ValueError("--views is like \"rot=-15,15;scale=0.9,1.1;shift=0:0:10\", not %r" % (spec,))
        items = [v.strip() for v in vals.split(",")]
        kw[key] = [tuple(float(x) for x in v.split(":")) for v in items] if key == "shift" else [float(v) for v in items]
    return make_views(**kw)


def view_table(views, dsize):
    """-> (V, VIEW_TABLE_DOUBLES) float64, the table the three view kernels read (include/awr_hip.h "Test-time views"): per view R (9), the
    forward rotation in crop pixels exactly as Augmenter.rotate builds it (loader.py:140-160) with the row 0 0 1; iR (6), cv2.warpAffine's
    inverse of it; scale; shift (3); rotates (1.0 / 0.0: the reference's own `not np.allclose(rot, 0)`).  cos and sin are evaluated here and
    nowhere else."""
    views = check_views(views)
    table = np.zeros((len(views), VIEW_TABLE_DOUBLES), np.float64)
    for i, (rot, scale, shift) in enumerate(views):
        rotates = not np.allclose(rot, 0.0)
        R2 = ND.rotation_matrix_2d((int(dsize) // 2, int(dsize) // 2), -np.mod(rot, 360), 1) if rotates else np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
        table[i, 0:6], table[i, 6:9] = R2.ravel(), (0.0, 0.0, 1.0)
        table[i, 9:15] = ND._invert_affine(R2).ravel()
        table[i, 15], table[i, 16:19], table[i, 19] = scale, shift, float(rotates)
    return table


def view_centers(centers_uvd, status, cube, table, paras, flip):
    """The statement of awr_view_centers: centres (n, 3) float64, status (n,), cube (3,) or (n, 3) -> view-major (V * n, ...) arrays:
    centres float64, cubes float64, frame rows int64, status int32.  Scalar IEEE double, in the header's order."""
    c_in = np.asarray(centers_uvd, np.float64).reshape(-1, 3)
    n, V = c_in.shape[0], table.shape[0]
    cubes = np.broadcast_to(np.asarray(cube, np.float64), (n, 3))
    status = np.asarray(status, np.int32)
    fx, fy, u0, v0 = (np.float64(p) for p in paras)
    fl = np.float64(flip)
    centers, cubes_out = np.empty((V * n, 3), np.float64), np.empty((V * n, 3), np.float64)
    frame, st = np.empty(V * n, np.int64), np.empty(V * n, np.int32)
    with np.errstate(all="ignore"):
        for v in range(V):
            scale, (sx, sy, sz) = np.float64(table[v, 15]), (np.float64(t) for t in table[v, 16:19])
            for b in range(n):
                r = v * n + b
                u, w, d = c_in[b]
                if sx == 0.0 and sy == 0.0 and sz == 0.0:
                    centers[r] = c_in[b]
                else:
                    x = (u - u0) * d / fx + sx                      # evaluator.uvd2xyz, the shift, evaluator.xyz2uvd: loader.py:112 in double
                    y = (w - v0) * d / fy * fl + sy
                    z = d + sz
                    yf = y * fl
                    centers[r] = (x * fx / z + u0, yf * fy / z + v0, z)
                cubes_out[r] = (cubes[b, 0] * scale, cubes[b, 1] * scale, cubes[b, 2] * scale)
                frame[r], st[r] = b, status[b]
    return centers, cubes_out, frame, st


def view_rotate(blocks, M, status, table):
    """The statement of awr_view_rotate: blocks, a list of V * n L.NyuSample (None where there is none), is patched in place; -> M (V * n, 3, 3)
    float32, a copy with the rotating views' AWR_DET_OK rows replaced by float32(R . float64(M))."""
    M = np.array(M, np.float32).reshape(-1, 3, 3)
    V, n = table.shape[0], M.shape[0] // table.shape[0]
    for v in range(V):
        if table[v, 19] == 0.0:
            continue
        R, iR = table[v, 0:9], table[v, 9:15]
        for b in range(n):
            r = v * n + b
            if status[r] != OK:
                continue
            if blocks is not None and blocks[r] is not None:
                blocks[r].op = 2                                        # AWR_NYU_AFFINE
                blocks[r].m[:] = [float(x) for x in iR] + [0.0, 0.0, 1.0]
            a = M[r].astype(np.float64)
            for i in range(3):
                for k in range(3):
                    M[r, i, k] = np.float32(((R[3 * i] * a[0, k]) + (R[3 * i + 1] * a[1, k])) + (R[3 * i + 2] * a[2, k]))
    return M


def fuse_views(xyz, status, ustatus, weights, mode, paras, flip):
    """The statement of awr_views_fuse: xyz (V, n, J, 3) float32, status / ustatus (V, n), weights (V, n, J) float32 or None (read by "conf"
    only), mode "mean" | "conf" | "median" -> (xyz (n, J, 3) float32, uvd (n, J, 3) float32, view_spread_mm (n, J) float32, views_used (n, J)
    int32).  The header's steps 1 ... 8 in IEEE double: every line below is ONE elementwise operation over the (n, J) joints at a time (numpy
    fuses nothing across ufuncs), and the views are walked sequentially in view order."""
    mode = FUSE_MODES[mode] if mode in FUSE_MODES else int(mode)
    xyz = np.asarray(xyz, np.float32)
    V, n, J = xyz.shape[:3]
    status, ustatus = np.asarray(status).reshape(V, n), np.asarray(ustatus).reshape(V, n)
    x = xyz.astype(np.float64)
    fx, fy, u0, v0 = (np.float64(p) for p in paras)
    with np.errstate(all="ignore"):
        frame_ok = ((status[0] == 0) & (ustatus[0] == 0))[:, None]
        used_v, w_v = [], []
        for v in range(V):
            ok = frame_ok & ((status[v] == 0) & (ustatus[v] == 0))[:, None] & np.isfinite(x[v]).all(-1)
            w = np.ones((n, J), np.float64)
            if mode == FUSE_CONF:
                w = np.asarray(weights, np.float32).reshape(V, n, J)[v].astype(np.float64)
                ok = ok & np.isfinite(w) & (w > 0.0)
            used_v.append(ok)
            w_v.append(w)
        used = np.zeros((n, J), np.int32)
        sw, s = np.zeros((n, J)), [np.zeros((n, J)) for _ in range(3)]
        for v in range(V):
            used = used + used_v[v]
            sw = np.where(used_v[v], sw + w_v[v], sw)
            for a in range(3):
                s[a] = np.where(used_v[v], s[a] + w_v[v] * x[v, :, :, a], s[a])
        if mode == FUSE_MEDIAN:
            m = []
            for a in range(3):
                t = np.sort(np.stack([np.where(used_v[v], x[v, :, :, a], np.inf) for v in range(V)]), axis=0, kind="stable")
                mid = np.take_along_axis(t, np.minimum(used // 2, V - 1)[None], 0)[0]
                below = np.take_along_axis(t, np.maximum(used // 2 - 1, 0)[None], 0)[0]
                m.append(np.where(used % 2 == 1, mid, (below + mid) / 2.0))
        else:
            m = [s[a] / sw for a in range(3)]
        q = np.zeros((n, J))
        for v in range(V):
            dx, dy, dz = x[v, :, :, 0] - m[0], x[v, :, :, 1] - m[1], x[v, :, :, 2] - m[2]
            q = np.where(used_v[v], q + w_v[v] * ((dx * dx + dy * dy) + dz * dz), q)
        spread = np.sqrt(q / sw)
        none = used == 0
        m = [np.where(none, np.nan, m[a]) for a in range(3)]
        spread = np.where(none, np.nan, spread)
        yf = m[1] * np.float64(flip)                                    # evaluator.xyz2uvd (util.py:3-10), in double
        uvd = np.stack([np.where(none, np.nan, m[0] * fx / m[2] + u0), np.where(none, np.nan, yf * fy / m[2] + v0), m[2]], -1)
    return np.stack(m, -1).astype(np.float32), uvd.astype(np.float32), spread.astype(np.float32), used.astype(np.int32)


# ---- operator-level wrappers over the entry points (tests, tools) ------------------------------------------------------------------
def _f64(x, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)


def _source(store):
    """A FrameStore-like object's five parts, as the entry points take a frame source."""
    return store.data.data_ptr(), store.ftype, store.data.shape[0], store.fh, store.fw


def _frame_index(frame_idx, dev):
    """The frame of every batch row as the entry points read it: a device int64 tensor (one handed in is used as it is)."""
    import torch
    return frame_idx if isinstance(frame_idx, torch.Tensor) else torch.as_tensor(np.asarray(frame_idx, np.int64)).to(dev)


def detect_device(store, frame_idx, seed="nearest", centers=None, cube=(300, 300, 300), paras=ND.PARAS, depth_range=DEPTH_RANGE, slab=SLAB,
                  iters=REFINE_ITERS, parts=0):
    """awr_detect on a nyu_device.FrameStore-like object (.data (n, fh, fw) uint16 on the device, .ftype, .fh, .fw): -> (centres (B, 3) float64,
    status (B,) int32) on the device, nothing synchronised."""
    import torch
    from . import _lib as L, detect_calls as DC
    dev = store.data.device
    idx = _frame_index(frame_idx, dev)
    B = int(idx.shape[0])
    cb = _f64(cube, dev)
    seed_t = None
    if seed == "given":
        seed_t = centers if isinstance(centers, torch.Tensor) else _f64(centers, dev)
    scratch = L.scratch("awr_detect_scratch", B, dtype=torch.int64, device=dev)
    out = torch.empty((B, 3), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    DC.awr_detect(*_source(store), idx.data_ptr(), B, seed, L.ptr(seed_t), depth_range, slab, cb.data_ptr(), cb.dim() == 2, paras, iters, parts,
                  scratch.data_ptr(), out.data_ptr(), status.data_ptr())
    return out, status


def palm_device(store, frame_idx, centers, status, cube=(300, 300, 300), paras=ND.PARAS, depth_range=DEPTH_RANGE, search=PALM_SEARCH,
                tau=PALM_TAU, rho2=PALM_RHO2, center_out=None, status_out=None, info=True, scratch=None):
    """awr_detect_palm on a FrameStore-like object: centres (B, 3) float64 and status (B,) int32 on the device, as detect_device returns them
    -> (centres (B, 3) float64, status (B,) int32, info (B, 4) int32 or None) on the device, nothing synchronised.  center_out / status_out:
    tensors to write into (they may be the inputs); info: True (allocated), False (NULL) or a tensor; scratch: an int32 tensor of at least
    awr_detect_palm_scratch(B, fh, fw) bytes."""
    import torch
    from . import _lib as L, detect_calls as DC
    search, tau, rho2 = check_palm(search, tau, rho2)
    dev = store.data.device
    idx = _frame_index(frame_idx, dev)
    B = int(idx.shape[0])
    cb = cube if isinstance(cube, torch.Tensor) else _f64(cube, dev)
    if scratch is None:
        scratch = L.scratch("awr_detect_palm_scratch", B, store.fh, store.fw, dtype=torch.int32, device=dev)
    center_out = torch.empty((B, 3), dtype=torch.float64, device=dev) if center_out is None else center_out
    status_out = torch.empty(B, dtype=torch.int32, device=dev) if status_out is None else status_out
    if info is True:
        info = torch.empty((B, 4), dtype=torch.int32, device=dev)
    elif info is False:
        info = None
    DC.awr_detect_palm(*_source(store), idx.data_ptr(), B, L.ptr(centers), L.ptr(status), depth_range, cb.data_ptr(), cb.dim() == 2, paras, search,
                       tau, rho2, scratch.data_ptr(), L.ptr(center_out), L.ptr(status_out), L.ptr(info))
    return center_out, status_out, info


def hands_device(store, frame_idx, hands, depth_range=DEPTH_RANGE, reach=REACH, slab=SLAB, min_pixels=MIN_PIXELS, labels=False, scratch=None,
                 edge=None, link=None, gap=LINK_GAP):
    """awr_detect_hands on a FrameStore-like object: -> (centres (K, B, 3) float64, status (K, B) int32, info (K, B, 4) int32, count (B,)
    int32, labels (B, fh, fw) int32 or None) on the device, hand-major, nothing synchronised.  labels: True (allocated), False (NULL) or
    a tensor; scratch: an int64 tensor of at least awr_detect_hands_scratch(B, fh, fw) bytes.  edge: None issues awr_detect_hands,
    anything else awr_detect_hands_edge (a type that is no number raises here; a value the entry point refuses gets its message there).
    link, gap: with a link (which needs an edge) awr_detect_hands_link is issued instead; link=None is the call without them."""
    import torch
    from . import _lib as L, detect_calls as DC
    edge = _check_edge(edge, value=False)
    link, gap = _check_link(link, gap, edge, value=False)
    dev = store.data.device
    idx = _frame_index(frame_idx, dev)
    B, K = int(idx.shape[0]), int(hands)
    if scratch is None:
        scratch = L.scratch("awr_detect_hands_scratch", B, store.fh, store.fw, dtype=torch.int64, device=dev)
    rows = max(K, 1)                                         # (a K the entry point refuses still gets its message from there)
    centers = torch.empty((rows, B, 3), dtype=torch.float64, device=dev)
    status = torch.empty((rows, B), dtype=torch.int32, device=dev)
    info = torch.empty((rows, B, 4), dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    if labels is True:
        labels = torch.empty((B, store.fh, store.fw), dtype=torch.int32, device=dev)
    elif labels is False:
        labels = None
    DC.awr_detect_hands(*_source(store), idx.data_ptr(), B, K, depth_range, reach, edge, slab, min_pixels, scratch.data_ptr(), L.ptr(labels),
                        centers.data_ptr(), status.data_ptr(), info.data_ptr(), count.data_ptr(), link=link, gap=gap)
    return centers, status, info, count, labels


def isolate_device(store, frame_idx, labels, roots=None, info=None, out=None):
    """awr_hands_isolate on a FrameStore-like object: labels (B, fh, fw) int32 and either info (K, B, 4) int32 (hands_device's) or roots
    (K, B) ints (negative: an EMPTY slot), on the device or numpy -> (out (K * B, fh, fw) uint16, row k * B + b, status (B,) int32) on the
    device, nothing synchronised.  out: a tensor to write into."""
    import torch
    from . import _lib as L, detect_calls as DC
    dev = store.data.device
    idx = _frame_index(frame_idx, dev)
    B = int(idx.shape[0])
    if (roots is None) == (info is None):
        raise ValueError("isolate_device takes either roots or info")
    if info is None:
        r = torch.as_tensor(np.asarray(roots, np.int64)).to(dev) if not isinstance(roots, torch.Tensor) else roots.to(torch.int64)
        fw = max(int(store.fw), 1)
        none = r < 0
        info = torch.stack([torch.where(none, -1, r % fw), torch.where(none, -1, r // fw), torch.zeros_like(r), torch.zeros_like(r)], -1).to(torch.int32)
    if not isinstance(labels, torch.Tensor):
        labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev)
    info = (info if isinstance(info, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(info, dtype=np.int32)).to(dev)).contiguous()
    K = int(info.shape[0]) if info.dim() == 3 else 0          # (a K the entry point refuses still gets its message from there)
    if out is None:
        out = torch.empty((max(K, 1) * B, store.fh, store.fw), dtype=torch.uint16, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    DC.awr_hands_isolate(*_source(store), idx.data_ptr(), B, K, L.ptr(labels), L.ptr(info), L.ptr(out), status.data_ptr())
    return out, status


def denoise_device(store, frame_idx, radius=1, edge=None, support=0, fill=None, out=None):
    """awr_frames_denoise on a FrameStore-like object: -> (out (B, fh, fw) uint16, row b the filtered frame frame_idx[b], status (B,)
    int32) on the device, nothing synchronised.  out: a tensor to write into; it must not overlap the store.  The types are checked here
    (edge as hands_device does); a value the entry point refuses gets its message from there."""
    import torch
    from . import _lib as L, detect_calls as DC
    radius, edge, support, fill = _check_denoise(radius, edge, support, fill, value=False)
    dev = store.data.device
    idx = _frame_index(frame_idx, dev)
    B = int(idx.shape[0])
    if out is None:
        out = torch.empty((B, store.fh, store.fw), dtype=torch.uint16, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    DC.awr_frames_denoise(*_source(store), idx.data_ptr(), B, radius, edge, support, fill, L.ptr(out), status.data_ptr())
    return out, status


def samples_device(centers, cube, dsize, frame_idx, n_frames, frame_shape, paras=ND.PARAS, flip=-1, status=None):
    """awr_detect_samples: centres (B, 3) float64 on the device -> (blocks (B, BLOCK_BYTES) uint8, M (B, 3, 3), center_xyz (B, 3), cube (B, 3)
    float32, status (B,) int32) on the device."""
    import torch
    from . import _lib as L, detect_calls as DC
    dev = centers.device
    B = int(centers.shape[0])
    idx = _frame_index(frame_idx, dev)
    cb = _f64(cube, dev)
    blocks = torch.empty((B, C.sizeof(L.NyuSample)), dtype=torch.uint8, device=dev)
    M = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    cxyz = torch.empty((B, 3), dtype=torch.float32, device=dev)
    cube32 = torch.empty((B, 3), dtype=torch.float32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev) if status is None else status
    DC.awr_detect_samples(L.ptr(centers), cb.data_ptr(), cb.dim() == 2, n_frames, idx.data_ptr(), B, dsize, frame_shape[0], frame_shape[1], paras, flip,
                          blocks.data_ptr(), L.ptr(M), L.ptr(cxyz), L.ptr(cube32), status.data_ptr())
    return blocks, M, cxyz, cube32, status


def unproject_device(jt_pred, center_xyz, M, cube, img_size, paras=ND.PARAS, flip=-1, n_valid=None, uvd_out=None, xyz_out=None, status=None):
    """awr_joints_unproject: -> (uvd (B, J, 3), xyz (B, J, 3), status (B,)); rows >= n_valid of the outputs are left as they are."""
    import torch
    from . import _lib as L, detect_calls as DC
    B, J = int(jt_pred.shape[0]), int(jt_pred.shape[1])
    n = B if n_valid is None else int(n_valid)
    uvd = torch.empty_like(jt_pred) if uvd_out is None else uvd_out
    xyz = torch.empty_like(jt_pred) if xyz_out is None else xyz_out
    status = torch.zeros(B, dtype=torch.int32, device=jt_pred.device) if status is None else status
    DC.awr_joints_unproject(L.ptr(jt_pred), L.ptr(center_xyz), L.ptr(M), L.ptr(cube), B, J, n, img_size, paras, flip, L.ptr(uvd), L.ptr(xyz),
                            status.data_ptr())
    return uvd, xyz, status


def joints_center_device(xyz, center_uvd, center_xyz, cube, status, ustatus, paras=ND.PARAS, flip=-1, joints=None, depth_range=DEPTH_RANGE,
                         max_shift=1.0, n_valid=None, center_out=None, next_out=None, code=None):
    """awr_joints_center on device tensors: -> (center_out (B, 3) float64, next (B, 3) float64, code (B,) int32); rows >= n_valid of the
    outputs are left as they are.  joints: a device int32 tensor, a list of indices or None (all joints); center_out may be center_uvd."""
    import torch
    from . import _lib as L, detect_calls as DC
    B, J = int(xyz.shape[0]), int(xyz.shape[1])
    dev = xyz.device
    n = B if n_valid is None else int(n_valid)
    if joints is not None and not isinstance(joints, torch.Tensor):
        joints = torch.tensor([int(j) for j in joints], dtype=torch.int32, device=dev)
    center_out = torch.empty((B, 3), dtype=torch.float64, device=dev) if center_out is None else center_out
    next_out = torch.empty((B, 3), dtype=torch.float64, device=dev) if next_out is None else next_out
    code = torch.empty(B, dtype=torch.int32, device=dev) if code is None else code
    DC.awr_joints_center(L.ptr(xyz), L.ptr(center_uvd), L.ptr(center_xyz), L.ptr(cube), L.ptr(status), L.ptr(ustatus), B, J, n,
                         None if joints is None else (L.ptr(joints), joints.numel()), paras, flip, depth_range, max_shift, L.ptr(center_out),
                         L.ptr(next_out), L.ptr(code))
    return center_out, next_out, code


def select_device(a_center, a_status, b_center, b_status):
    """awr_centers_select on device tensors: -> (center (B, 3) float64, status (B,) int32, which (B,) int32)."""
    import torch
    from . import _lib as L, detect_calls as DC
    B, dev = int(a_center.shape[0]), a_center.device
    out = torch.empty((B, 3), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    which = torch.empty(B, dtype=torch.int32, device=dev)
    DC.awr_centers_select(L.ptr(a_center), L.ptr(a_status), L.ptr(b_center), L.ptr(b_status), B, L.ptr(out), L.ptr(status), L.ptr(which))
    return out, status, which


def view_centers_device(centers, status, cube, table, B=None, n_valid=None, paras=ND.PARAS, flip=-1, out=None):
    """awr_view_centers on device tensors: centres (B, 3) float64, status (B,) int32, cube 3 or (B, 3) numbers, table (V, VIEW_TABLE_DOUBLES)
    float64 -> (centres (V * B, 3) float64, cubes (V * B, 3) float64, frame (V * B,) int64, status (V * B,) int32); out: these four, to write
    into (rows with b >= n_valid are left as they are)."""
    import torch
    from . import _lib as L, detect_calls as DC
    dev = centers.device
    B = int(centers.shape[0]) if B is None else int(B)
    n = B if n_valid is None else int(n_valid)
    table = table if isinstance(table, torch.Tensor) else _f64(table, dev)
    V = int(table.shape[0])
    cb = cube if isinstance(cube, torch.Tensor) else _f64(cube, dev)
    if out is None:
        out = (torch.empty((V * B, 3), dtype=torch.float64, device=dev), torch.empty((V * B, 3), dtype=torch.float64, device=dev),
               torch.empty(V * B, dtype=torch.int64, device=dev), torch.empty(V * B, dtype=torch.int32, device=dev))
    DC.awr_view_centers(L.ptr(centers), L.ptr(status), L.ptr(cb), cb.dim() == 2, L.ptr(table), V, B, n, paras, flip, L.ptr(out[0]), L.ptr(out[1]),
                        L.ptr(out[2]), L.ptr(out[3]))
    return out


def view_rotate_device(blocks, M, status, table, n_valid=None):
    """awr_view_rotate: blocks (V * B, BLOCK_BYTES) uint8 and M (V * B, 3, 3) float32 are patched in place; status (V * B,) int32 the rows' codes
    after awr_detect_samples."""
    import torch
    from . import _lib as L, detect_calls as DC
    table = table if isinstance(table, torch.Tensor) else _f64(table, M.device)
    V = int(table.shape[0])
    B = int(M.shape[0]) // V
    DC.awr_view_rotate(L.ptr(blocks), L.ptr(M), L.ptr(status), L.ptr(table), V, B, B if n_valid is None else n_valid)
    return blocks, M


def fuse_views_device(xyz, status, ustatus, weights, mode, paras=ND.PARAS, flip=-1, n_valid=None, out=None):
    """awr_views_fuse: xyz (V, B, J, 3) float32, status / ustatus (V, B) or (V * B,) int32, weights (V, B, J) float32 or None ->
    (xyz (B, J, 3), uvd (B, J, 3), view_spread_mm (B, J) float32, views_used (B, J) int32); rows >= n_valid are left as they are."""
    import torch
    from . import _lib as L, detect_calls as DC
    V, B, J = (int(x) for x in xyz.shape[:3])
    dev = xyz.device
    if out is None:
        out = (torch.empty((B, J, 3), dtype=torch.float32, device=dev), torch.empty((B, J, 3), dtype=torch.float32, device=dev),
               torch.empty((B, J), dtype=torch.float32, device=dev), torch.empty((B, J), dtype=torch.int32, device=dev))
    DC.awr_views_fuse(L.ptr(xyz), L.ptr(status), L.ptr(ustatus), L.ptr(weights), mode, V, B, J, B if n_valid is None else n_valid, paras, flip,
                      L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]))
    return out
