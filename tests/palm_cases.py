"""Inputs shared by tests/test_palm_cpu.py and tests/test_palm_gpu.py: hand-made silhouettes with known answers, procedural hands, an
independent brute-force form of the statement, and the statement's outputs computed once per process.

Hand-made frames are 48 x 64 (64 x 48 for the shapes whose arm runs along the rows: an arm of 40, a palm of 16 and fingers of 6 pixels need
62 pixels along the arm) with the NYU intrinsics scaled by 0.1: at 500 mm a window of two 300 mm cubes is 70 pixels wide, so a centre in the
middle of the frame gives a window that is clipped to the whole frame; at 1000 mm it is 36 pixels and lies inside the frame."""
import functools

import numpy as np

SMALL, TALL, MID, FULL = (48, 64), (64, 48), (96, 128), (480, 640)
DEPTH = 500
ARM, PALM, FINGER = (10, 40), 16, (2, 6)


def paras_for(scale):
    from awr_amd import nyu_data as ND
    return tuple(scale * p for p in ND.PARAS)


def frame_of(mask, depth=DEPTH):
    return np.where(mask, depth, 0).astype(np.uint16)


def middle(shape, depth=DEPTH):
    return (shape[1] / 2.0, shape[0] / 2.0, float(depth))


def lollipop(orient, mirror=False, border=False):
    """-> (mask, palm box (v_lo, v_hi, u_lo, u_hi), half-open).  Canonical form on 48 x 64: the arm runs along +u from column 1 (from the
    frame border, column 0, with border=True), 10 wide and 40 long, then the 16 x 16 palm, then three fingers 2 wide and 6 long at rows that
    are not symmetric about the arm's axis (so the mirrored shape is another shape)."""
    m = np.zeros(SMALL, bool)
    vc, a0 = SMALL[0] // 2, 1
    a1 = a0 + ARM[1]
    m[vc - ARM[0] // 2:vc + ARM[0] // 2, (0 if border else a0):a1] = True
    m[vc - PALM // 2:vc + PALM // 2, a1:a1 + PALM] = True
    for r in (vc - 8, vc - 2, vc + 3):
        m[r:r + FINGER[0], a1 + PALM:a1 + PALM + FINGER[1]] = True
    box = np.zeros(SMALL, bool)
    box[vc - PALM // 2:vc + PALM // 2, a1:a1 + PALM] = True
    if mirror:
        m, box = m[::-1], box[::-1]
    if orient == "W":
        m, box = m[:, ::-1], box[:, ::-1]
    elif orient == "S":
        m, box = m.T, box.T
    elif orient == "N":
        m, box = m.T[::-1], box.T[::-1]
    vv, uu = np.nonzero(box)
    return np.ascontiguousarray(m), (int(vv.min()), int(vv.max()) + 1, int(uu.min()), int(uu.max()) + 1)


def _disc(shape, cv, cu, r):
    vv, uu = np.indices(shape)
    return (vv - cv) ** 2 + (uu - cu) ** 2 <= r * r


def _case(name, frame, center, status=0, palm_box=None, point=None):
    frame = np.ascontiguousarray(frame, dtype=np.uint16)
    frame.setflags(write=False)
    return dict(name=name, frame=frame, center=tuple(float(c) for c in center), status=int(status), palm_box=palm_box, point=point,
                paras=paras_for(0.1))


@functools.lru_cache(maxsize=None)
def hand_cases():
    """name -> case.  point: the palm point (pu, pv) worked out by hand; palm_box: where it must lie."""
    out = [_case("disc", frame_of(_disc(SMALL, 22, 30, 10)), middle(SMALL), point=(30, 22))]
    for orient in "EWSN":
        for mirror in (False, True):
            m, box = lollipop(orient, mirror)
            out.append(_case("lollipop_%s%s" % (orient, "_mirror" if mirror else ""), frame_of(m), middle(m.shape), palm_box=box))
        m, box = lollipop(orient, border=True)
        out.append(_case("lollipop_%s_border" % orient, frame_of(m), middle(m.shape), palm_box=box))
    # ties in every argmax.  An 8 x 20 rectangle at rows 20 ... 27, columns 22 ... 41: D2 is the squared distance to the nearest edge, m = 16
    # on rows 3 and 4, columns 3 ... 16 of it; S (3 * D2 >= 16: distance >= 3) is rows 2 ... 5, columns 2 ... 17; e0 = (3, 3) is the first of
    # the 28 maxima; e1 = (5, 17) (distance^2 200, against 197 at (2, 17)); e2 = (2, 2); the shape is point-symmetric, so b1 == b2 and the
    # far end, e2's, is taken; s = 15 u + 3 v - 36 there, (3, 3) has s = 18 <= sqrt(16 * 234): p* = (3, 3), the first maximum again.
    rect = np.zeros(SMALL, bool)
    rect[20:28, 22:42] = True
    out.append(_case("tie_rectangle", frame_of(rect), middle(SMALL), point=(25, 23)))
    plus = np.zeros(SMALL, bool)
    plus[21:27, 10:54] = True
    plus[4:44, 29:35] = True
    out.append(_case("tie_plus", frame_of(plus), middle(SMALL)))
    out.append(_case("tie_two_discs", frame_of(_disc(SMALL, 24, 14, 9) | _disc(SMALL, 24, 49, 9) | (np.abs(np.indices(SMALL)[0] - 24) <= 1)
                                               & (np.abs(np.indices(SMALL)[1] - 31.5) < 18)), middle(SMALL)))
    out.append(_case("square_diagonal_ties", frame_of(_disc(SMALL, 24, 32, 0) | (np.maximum(np.abs(np.indices(SMALL)[0] - 24),
                                                                                   np.abs(np.indices(SMALL)[1] - 32)) <= 7)), middle(SMALL)))
    # the mask fills the window: D2 comes from the ring alone -- a window inside the frame (1000 mm: 36 pixels) and one clipped to the frame
    out.append(_case("full_window_inside", np.full(SMALL, 1000, np.uint16), middle(SMALL, 1000)))
    out.append(_case("full_window_clipped", np.full(SMALL, DEPTH, np.uint16), middle(SMALL)))
    one = np.zeros(SMALL, bool)
    one[17, 41] = True
    out.append(_case("single_pixel", frame_of(one), middle(SMALL), point=(41, 17)))
    out.append(_case("empty_mask", np.zeros(SMALL, np.uint16), middle(SMALL)))
    out.append(_case("out_of_depth", np.full(SMALL, 900, np.uint16), middle(SMALL)))
    out.append(_case("nan_centre", frame_of(_disc(SMALL, 22, 30, 10)), (float("nan"), 24.0, 500.0)))
    out.append(_case("inf_depth", frame_of(_disc(SMALL, 22, 30, 10)), (32.0, 24.0, float("inf"))))
    out.append(_case("zero_depth", frame_of(_disc(SMALL, 22, 30, 10)), (32.0, 24.0, 0.0)))
    out.append(_case("window_off_frame", frame_of(_disc(SMALL, 22, 30, 10)), (-400.0, 24.0, 500.0)))
    out.append(_case("status_empty", frame_of(_disc(SMALL, 22, 30, 10)), (float("nan"),) * 3, status=1))
    out.append(_case("status_bad_window", frame_of(_disc(SMALL, 22, 30, 10)), (31.0, 23.0, 500.0), status=3))
    return {c["name"]: c for c in out}


@functools.lru_cache(maxsize=None)
def synth_frames(n, seed, frame_shape, scale, forearm=True):
    """procedural hands (awr_amd.synth, numpy): -> (frames (n, fh, fw) uint16, label centres (n, 3) camera mm, paras, flip), read-only"""
    from awr_amd import synth
    paras, flip = paras_for(scale), -1
    model = synth.HandModel(forearm=forearm)
    poses = synth.sample_poses(n, seed, model, frame_shape=frame_shape, paras=paras, flip=flip)
    joints, prims, bbox = synth.forward_kinematics(poses, model, frame_shape, paras, flip)
    frames = synth.render(prims, bbox, frame_shape=frame_shape, paras=paras, flip=flip)
    _, centers = synth.labels(joints)
    frames.setflags(write=False)
    centers.setflags(write=False)
    return frames, centers, paras, flip


@functools.lru_cache(maxsize=None)
def synth_reference(n, seed, frame_shape, scale, forearm=True):
    """the statements on synth_frames(...): -> (detector centres (n, 3), detector status (n,), palm centres (n, 3), palm status (n,), info
    (n, 4)), computed once per process, read-only"""
    from awr_amd import detect as D
    frames, _, paras, _ = synth_frames(n, seed, frame_shape, scale, forearm)
    det = [D.detect(f, paras=paras) for f in frames]
    palm = [D.palm_center(f, c, s, paras=paras) for f, (c, s) in zip(frames, det)]
    out = (np.array([c for c, _ in det], np.float64), np.array([s for _, s in det], np.int32), np.array([c for c, _, _ in palm], np.float64),
           np.array([s for _, s, _ in palm], np.int32), np.array([i for _, _, i in palm], np.int32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hand_reference(name):
    """the statement on a hand-made case: (centre (3,) float64, status, info (4,) int32)"""
    from awr_amd import detect as D
    c = hand_cases()[name]
    center, status, info = D.palm_center(c["frame"], c["center"], c["status"], paras=c["paras"])
    return np.array(center, np.float64), int(status), np.array(info, np.int32)


def brute_d2(mask):
    """the definition, literally: the smallest squared distance from each pixel to a background position, the one-pixel ring included"""
    h, w = mask.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = mask
    bv, bu = np.nonzero(~pad)
    out = np.zeros((h, w), np.int64)
    for v, u in zip(*np.nonzero(mask)):
        out[v, u] = int(((bv - (v + 1)) ** 2 + (bu - (u + 1)) ** 2).min())
    return out


def brute_palm(frame, window, dlo, dhi, tau=(1, 3), rho2=(25, 4)):
    """Steps 3 ... 7 of the statement in plain Python integers over a list of pixels in raster order, every argmax an explicit loop that
    keeps the FIRST maximum: -> (centre, info) for a window (u0, u1, v0, v1) that holds at least one pixel with dlo <= d <= dhi."""
    u0, u1, v0, v1 = window
    win = frame[v0:v1, u0:u1].astype(np.int64)
    mask = (win >= dlo) & (win <= dhi) & (win != 0)
    D2 = brute_d2(mask)
    pix = [(int(v), int(u)) for v, u in zip(*np.nonzero(mask))]                       # np.nonzero lists in raster order
    m = max(int(D2[p]) for p in pix)
    S = [p for p in pix if tau[1] * int(D2[p]) >= tau[0] * m]

    def first_max(points, f):
        best, arg = None, None
        for p in points:
            if best is None or f(p) > best:
                best, arg = f(p), p
        return arg
    e0 = first_max(S, lambda p: int(D2[p]))
    e1 = first_max(S, lambda p: (p[0] - e0[0]) ** 2 + (p[1] - e0[1]) ** 2)
    e2 = first_max(S, lambda p: (p[0] - e1[0]) ** 2 + (p[1] - e1[1]) ** 2)
    a = (e2[0] - e1[0], e2[1] - e1[1])
    L = a[0] ** 2 + a[1] ** 2
    if L == 0:
        ps = e0
    else:
        t = lambda p: (p[0] - e1[0]) * a[0] + (p[1] - e1[1]) * a[1]
        b1, b2 = sum(1 for p in pix if t(p) < 0), sum(1 for p in pix if t(p) > L)
        s = (lambda p: L - t(p)) if b2 >= b1 else t
        ps = first_max([p for p in S if s(p) <= 0 or s(p) ** 2 <= m * L], lambda p: int(D2[p]))
    r2 = int(D2[ps])
    disc = [p for p in pix if rho2[1] * ((p[0] - ps[0]) ** 2 + (p[1] - ps[1]) ** 2) <= rho2[0] * r2]
    n = len(disc)
    su, sv, sd = sum(p[1] + u0 for p in disc), sum(p[0] + v0 for p in disc), sum(int(win[p]) for p in disc)
    return (float(su) / float(n), float(sv) / float(n), float(sd) / float(n)), (ps[1] + u0, ps[0] + v0, r2, n)


def same(a, b):
    """np.array_equal on the bits, NaN equal to NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
