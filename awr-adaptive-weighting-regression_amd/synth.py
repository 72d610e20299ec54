"""Synthetic hands: a procedural, articulated hand with ground-truth joints, rendered as raw uint16 depth frames (csrc/awr_synth.hip;
include/awr_hip.h "Synthetic hand frames").

These are procedural hands.  They give every layer of the project one labelled input that needs no download; they say nothing about NYU.

  * `HandModel`, `sample_poses`, `forward_kinematics`, `labels`: the model and its kinematics, numpy float64 on the host.  All
    trigonometry happens here, once; the renderer only sees a table of capsules.  `sample_sequences` eases between key poses drawn by
    `sample_poses`: temporally coherent sequences for the tracker and the temporal joint filter.
  * `render`: the statement of the renderer, vectorised numpy over one frame.  `render_device` runs the same sequence of float64
    operations in one kernel launch per chunk of frames (awr_synth_render) and writes into an HBM-resident frame store.
  * `SyntheticFrames`: poses -> kinematics -> frames -> a dataset (`DeviceNYU` over a `FrameStore`, or with device=None the host `NYU`).

Definition of the renderer.  A frame is a union of at most MAX_PRIMS capsules, rows `ax ay az bx by bz r 0` of a (K, 8) float64 table in
camera millimetres; r <= 0 marks an unused row; a sphere is a capsule with a == b.  Pixel (u, v) casts the ray t * d from the camera
centre, d = ((u - u0) / fx, flip * ((v - v0) / fy), 1), so t IS the depth z.  Per capsule the candidate depth is the point where the ray
ENTERS the capsule (a capsule that holds the camera centre on that ray contributes nothing):

    oa = -a, ob = -b, ba = b - a, rr = r r
    baba = ba.ba, baoa = ba.oa, oaoa = oa.oa, obob = ob.ob              every dot product (x x' + y y') + z z'
    cc = (baba oaoa - baoa baoa) - rr baba, ca = oaoa - rr, cb = obob - rr
    dd = (dx dx + dy dy) + 1, bard = (bax dx + bay dy) + baz, rdoa = (dx oax + dy oay) + oaz, rdob likewise
    A = baba dd - bard bard, B = baba rdoa - baoa bard, H = B B - A cc                    the infinite cylinder: A t^2 + 2 B t + cc = 0
    A > 0 and H > 0:  tc = (-B - sqrt(H)) / A, y = baoa + tc bard
                      0 < y < baba: the body, a candidate iff B < 0 and cc > 0 (t > 0 without consulting the root);
                      y <= 0: end a's sphere; y >= baba: end b's sphere
    A > 0 and H <= 0: the ray misses the cylinder the capsule lies in: nothing
    A <= 0 (the ray runs along the axis, or a == b): both spheres
    sphere at o* (= oa or ob, c* = ca or cb, rd = rdoa or rdob): Hs = rd rd - dd c*; a candidate iff Hs > 0 and rd < 0 and c* > 0, at
                      ts = (-rd - sqrt(Hs)) / dd

Whether a capsule is hit is therefore decided by signs of polynomials in the inputs alone; the square roots only place the hit.  The
frame's depth is the smallest candidate (`t < best` against +inf: a NaN is never taken); the pixel's value is floor(z + 0.5) clipped to
[1, 65535], and with a wall (background_mm > 0) a value >= background_mm is the wall's.  A pixel without a candidate, or outside the
frame's box [u_lo, u_hi) x [v_lo, v_hi), gets the background: 0 (no return) or the wall.  noise_mm = a > 0 adds an integer of [-a, a],
`hash_u32(seed, global frame index, v * fw + u) % (2 a + 1) - a`, to hit pixels and to the wall, and clips to [1, 65535] again.
"""
import numpy as np

from . import nyu_data as ND

MAX_PRIMS = 32
OK, EMPTY, BAD_PRIM = 0, 1, 2
STATUS_NAMES = {OK: "ok", EMPTY: "no pixel of the frame was hit (AWR_SYNTH_EMPTY)",
                BAD_PRIM: "a used row of the primitive table is not finite (AWR_SYNTH_BAD_PRIM)"}
MAX_FRAME_EDGE = 16384            # awr_synth_render's bound on fh and fw
MAX_CALL_FRAMES = 65535           # ... and on the frames of one call (the grid's third dimension)

# ---- the hand ------------------------------------------------------------------------------------------------------------------------
# joints21: 0 wrist, then per finger f (0 thumb, 1 index, 2 middle, 3 ring, 4 pinky) 1 + 4 f ... 4 + 4 f = base, mid, far, tip
WRIST = 0
THUMB, INDEX, MIDDLE, RING, PINKY = range(5)
PARENT = np.array([-1] + [p for f in range(5) for p in (0, 1 + 4 * f, 2 + 4 * f, 3 + 4 * f)])


def _base(f):
    return 1 + 4 * f


# joints21 -> the 14 of the NYU evaluation order (vis_tool._SKELETON["nyu"]); 11, 12 (wrist points) and 13 (palm) are derived in labels()
_NYU_FROM21 = [_base(PINKY) + 3, _base(PINKY) + 1, _base(RING) + 3, _base(RING) + 1, _base(MIDDLE) + 3, _base(MIDDLE) + 1,
               _base(INDEX) + 3, _base(INDEX) + 1, _base(THUMB) + 3, _base(THUMB) + 1, _base(THUMB)]


class HandModel:
    """A wrist and five fingers of three phalanges each: 21 joints, lengths and radii in millimetres of an adult hand.  Palm frame: x
    across the palm towards the thumb, y along the fingers, z out of the back of the hand; the wrist is the origin."""

    # wrist -> finger base in the palm frame (index ... pinky: the metacarpals, rigid; the thumb's is articulated, only its length counts)
    MCP = np.array([[0.0, 0.0, 0.0], [26.0, 88.0, 0.0], [6.0, 92.0, 0.0], [-13.0, 86.0, 0.0], [-31.0, 76.0, 0.0]])
    THUMB_METACARPAL = 42.0
    PHALANGES = np.array([[27.0, 23.0, 20.0], [42.0, 25.0, 21.0], [46.0, 29.0, 22.0], [42.0, 27.0, 22.0], [33.0, 20.0, 19.0]])
    RADII = np.array([[10.5, 9.5, 8.5], [9.0, 8.0, 7.0], [9.5, 8.5, 7.5], [9.0, 8.0, 7.0], [8.0, 7.0, 6.0]])
    THUMB_METACARPAL_RADIUS = 13.0
    PALM_RADIUS = np.array([0.0, 14.0, 14.5, 14.0, 13.0])        # the four wrist -> base capsules
    KNUCKLE_RADIUS = 11.0                                        # the fifth palm capsule: index base -> pinky base
    FOREARM_LENGTH, FOREARM_RADIUS = 250.0, 26.0
    # anatomical ranges in degrees: flexion of base / mid / far joint, abduction of the base joint; the thumb's two base angles
    FLEX = ((-10.0, 80.0), (0.0, 95.0), (0.0, 70.0))
    ABDUCT = (-12.0, 12.0)
    THUMB_FLEX = ((-5.0, 45.0), (0.0, 60.0), (0.0, 70.0))
    THUMB_BASE = ((15.0, 50.0), (-10.0, 45.0))                   # away from the index metacarpal in the palm plane; out of the palm
    FINGER_SPLAY = np.array([0.0, 8.0, 0.0, -7.0, -15.0])       # rest direction of each finger in the palm plane, degrees towards the thumb

    def __init__(self, forearm=True, knuckles=True):
        self.forearm, self.knuckles = bool(forearm), bool(knuckles)
        self.K = 15 + 1 + 4 + int(self.knuckles) + int(self.forearm)
        assert self.K <= MAX_PRIMS

    def bone_lengths(self):
        """(21,) length of the bone from PARENT[j] to j at scale 1 (entry 0 unused)"""
        out = np.zeros(21)
        for f in range(5):
            b = _base(f)
            out[b] = self.THUMB_METACARPAL if f == THUMB else float(np.sqrt((self.MCP[f] ** 2).sum()))
            out[b + 1:b + 4] = self.PHALANGES[f]
        return out


def _rot(axis, deg):
    """(n,) degrees about a coordinate axis -> (n, 3, 3)"""
    a = np.deg2rad(np.asarray(deg, np.float64))
    c, s, o, z = np.cos(a), np.sin(a), np.ones_like(a), np.zeros_like(a)
    m = {"x": [[o, z, z], [z, c, -s], [z, s, c]], "y": [[c, z, s], [z, o, z], [-s, z, c]], "z": [[c, -s, z], [s, c, z], [z, z, o]]}[axis]
    return np.stack([np.stack(r, -1) for r in m], -2)


def sample_poses(n, seed, model=None, z_range=(500.0, 900.0), scale_range=(0.85, 1.15), rot_range=(50.0, 50.0, 180.0), edge=False,
                 cube=(300, 300, 300), frame_shape=(480, 640), paras=ND.PARAS, flip=-1):
    """n poses from numpy.random.RandomState(seed): a dict of float64 arrays -- flex (n, 5, 3) and abduct (n, 5) degrees, thumb_base (n, 2),
    euler (n, 3) the global rotation (about x, y, then z, degrees), scale (n,), position (n, 3) of the wrist in camera millimetres.  The
    position is drawn so that the centre of the crop cube around the hand projects at least half a projected cube edge inside the frame
    (edge=True: anywhere up to a quarter edge OUTSIDE it, so some hands are cut by the border).  The same arguments give the same arrays."""
    model = model or HandModel()
    rs = np.random.RandomState(seed)
    n = int(n)
    u = rs.uniform(size=(n, 5, 3))
    flex = np.empty((n, 5, 3))
    for f in range(5):
        rng = model.THUMB_FLEX if f == THUMB else model.FLEX
        for k in range(3):
            flex[:, f, k] = rng[k][0] + u[:, f, k] * (rng[k][1] - rng[k][0])
    # fingers curl together more often than not: pull the four fingers' flexion towards a common draw
    common = rs.uniform(size=(n, 1, 1))
    mix = rs.uniform(0.0, 0.8, size=(n, 1, 1))
    for k in range(3):
        lo, hi = model.FLEX[k]
        flex[:, 1:, k] = (1 - mix[:, :, 0]) * flex[:, 1:, k] + mix[:, :, 0] * (lo + common[:, :, 0] * (hi - lo))
    abduct = model.ABDUCT[0] + rs.uniform(size=(n, 5)) * (model.ABDUCT[1] - model.ABDUCT[0])
    tb = rs.uniform(size=(n, 2))
    thumb_base = np.stack([model.THUMB_BASE[k][0] + tb[:, k] * (model.THUMB_BASE[k][1] - model.THUMB_BASE[k][0]) for k in range(2)], -1)
    euler = (rs.uniform(size=(n, 3)) * 2 - 1) * np.asarray(rot_range, np.float64)
    scale = scale_range[0] + rs.uniform(size=n) * (scale_range[1] - scale_range[0])
    z = z_range[0] + rs.uniform(size=n) * (z_range[1] - z_range[0])
    fh, fw = frame_shape
    fx, fy, u0, v0 = (float(p) for p in paras)
    half_u, half_v = 0.5 * cube[0] * fx / z, 0.5 * cube[1] * fy / z            # half a projected cube edge in pixels
    m = -0.5 if edge else 1.0
    pu, pv = rs.uniform(size=n), rs.uniform(size=n)
    lo_u, hi_u = np.minimum(m * half_u, fw / 2.0), np.maximum(fw - 1 - m * half_u, fw / 2.0)
    lo_v, hi_v = np.minimum(m * half_v, fh / 2.0), np.maximum(fh - 1 - m * half_v, fh / 2.0)
    cu, cv = lo_u + pu * (hi_u - lo_u), lo_v + pv * (hi_v - lo_v)
    # the hand's middle sits about 0.6 metacarpals up the palm from the wrist: place the wrist so that this point is the drawn one
    poses = dict(flex=flex, abduct=abduct, thumb_base=thumb_base, euler=euler, scale=scale, position=np.zeros((n, 3)))
    mid = _palm_point(poses, model)
    target = np.stack([(cu - u0) * z / fx, flip * (cv - v0) * z / fy, z], -1)
    poses["position"] = target - mid
    return poses


def place_poses(poses, u, v, z, model=None, paras=ND.PARAS, flip=-1):
    """-> a copy of the pose dict whose palm point (the point sample_poses places: 0.6 middle metacarpals up the palm from the wrist)
    projects to pixel (u, v) at depth z millimetres; u, v, z are numbers or (n,) arrays.  sample_poses' own last lines, for a caller that
    decides where each hand goes -- two hands side by side, say (`compose`)."""
    model = model or HandModel()
    out = {k: np.array(a, dtype=np.float64) for k, a in poses.items()}
    n = len(out["scale"])
    fx, fy, u0, v0 = (float(p) for p in paras)
    u, v, z = (np.broadcast_to(np.asarray(x, np.float64), (n,)) for x in (u, v, z))
    out["position"] = np.zeros((n, 3))
    mid = _palm_point(out, model)
    target = np.stack([(u - u0) * z / fx, flip * (v - v0) * z / fy, z], -1)
    out["position"] = target - mid
    return out


def compose(*frames):
    """The per-pixel NEAREST NON-ZERO depth of equally shaped uint16 frames (0: no frame has a return there): what one camera sees of
    scenes rendered apart.  numpy arrays -> a numpy array, device (or host) tensors -> a tensor of the same kind."""
    if not frames:
        raise ValueError("compose needs at least one frame")
    if all(isinstance(f, np.ndarray) for f in frames):
        if any(f.dtype != np.uint16 or f.shape != frames[0].shape for f in frames):
            raise ValueError("compose takes equally shaped uint16 frames")
        out = frames[0].copy()
        for f in frames[1:]:
            out = np.where(out == 0, f, np.where(f == 0, out, np.minimum(out, f)))
        return out
    import torch
    if any(not isinstance(f, torch.Tensor) or f.dtype != torch.uint16 or f.shape != frames[0].shape or f.device != frames[0].device for f in frames):
        raise ValueError("compose takes equally shaped uint16 frames, all numpy arrays or all tensors of one device")
    wide = [f.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF for f in frames]          # (uint16 tensors have no arithmetic)
    out = wide[0]
    for f in wide[1:]:
        out = torch.where(out == 0, f, torch.where(f == 0, out, torch.minimum(out, f)))
    return torch.where(out >= 32768, out - 65536, out).to(torch.int16).view(torch.uint16)


def sample_sequences(n_seq, length, seed, key_every=15, model=None, rot_range=(50.0, 50.0, 60.0), **pose_options):
    """n_seq temporally coherent sequences of `length` frames each: a pose dict with sample_poses' keys and n_seq * length rows,
    SEQUENCE-MAJOR (frame t of sequence s is row s * length + t).  One sample_poses(n_seq * K, seed, ...) call draws K =
    (length - 2) // key_every + 2 key poses per sequence (key k of sequence s is its row s * K + k; a key every key_every frames, and one
    past the last frame); frame t lies between keys k = t // key_every and k + 1 at f = (t % key_every) / key_every, eased by the
    smoothstep s = f f (3 - 2 f), and EVERY field is a + s (b - a): a frame on a key equals that key bit for bit.  The default rot_range
    keeps the in-plane rotation of two neighbouring keys within a hand's reach (angles are interpolated as numbers, not on the circle).
    forward_kinematics, labels, render and render_device take the result unchanged."""
    n_seq, length, key_every = int(n_seq), int(length), int(key_every)
    if n_seq < 1 or length < 1 or key_every < 1:
        raise ValueError("sample_sequences needs n_seq, length and key_every >= 1, got %d, %d, %d" % (n_seq, length, key_every))
    K = (length - 2) // key_every + 2
    keys = sample_poses(n_seq * K, seed, model, rot_range=rot_range, **pose_options)
    t = np.arange(length)
    k = t // key_every
    f = (t % key_every) / np.float64(key_every)
    s = f * f * (3.0 - 2.0 * f)
    out = {}
    for name, v in keys.items():
        v = v.reshape((n_seq, K) + v.shape[1:])
        a, b = v[:, k], v[:, np.minimum(k + 1, K - 1)]          # (a last frame ON the last key has s = 0: the clamp only names a row)
        w = s.reshape((1, length) + (1,) * (v.ndim - 2))
        out[name] = np.ascontiguousarray((a + w * (b - a)).reshape((n_seq * length,) + v.shape[2:]))
    return out


def _global_rotation(poses):
    e = poses["euler"]
    return _rot("z", e[:, 2]) @ _rot("y", e[:, 1]) @ _rot("x", e[:, 0])


def _palm_point(poses, model):
    R = _global_rotation(poses)
    return np.einsum("nij,j->ni", R, 0.6 * model.MCP[MIDDLE]) * poses["scale"][:, None]


def forward_kinematics(poses, model=None, frame_shape=(480, 640), paras=ND.PARAS, flip=-1, margin=2):
    """-> joints21 (n, 21, 3) camera millimetres in the camera convention of evaluator.xyz2uvd / uvd2xyz, prims (n, K, 8) float64 rows
    `ax ay az bx by bz r 0`, bbox (n, 4) int32 `u_lo v_lo u_hi v_hi`: a conservative (half-open) pixel box of the projected primitives,
    clipped to the frame."""
    model = model or HandModel()
    n = len(poses["scale"])
    R = _global_rotation(poses)
    s = poses["scale"][:, None]
    J = np.zeros((n, 21, 3))
    rad = np.zeros((n, 21))                                       # radius of the capsule PARENT[j] -> j
    ey = np.array([0.0, 1.0, 0.0])
    for f in range(5):
        b = _base(f)
        if f == THUMB:
            # the metacarpal leaves the wrist in the palm plane, turned from the fingers' direction towards the thumb side, then out of the palm
            F = _rot("z", -poses["thumb_base"][:, 0] - 20.0) @ _rot("x", -poses["thumb_base"][:, 1])
            J[:, b] = np.einsum("nij,j->ni", F, ey) * model.THUMB_METACARPAL
            rad[:, b] = model.THUMB_METACARPAL_RADIUS
            F = F @ _rot("y", np.full(n, -50.0))                  # the thumb flexes across the palm, not into it
        else:
            J[:, b] = model.MCP[f]
            rad[:, b] = model.PALM_RADIUS[f]
            F = _rot("z", -(model.FINGER_SPLAY[f] + poses["abduct"][:, f]))
        for k in range(3):
            F = F @ _rot("x", -poses["flex"][:, f, k])            # flexion curls towards -z, the palm side
            J[:, b + k + 1] = J[:, b + k] + np.einsum("nij,j->ni", F, ey) * model.PHALANGES[f, k]
            rad[:, b + k + 1] = model.RADII[f, k]
    J = np.einsum("nij,nkj->nki", R, J) * s[:, :, None] + poses["position"][:, None, :]
    K = model.K
    prims = np.zeros((n, K, 8))
    k = 0
    for j in range(1, 21):            # every bone is a capsule: 15 phalanges, the thumb metacarpal, four palm capsules
        prims[:, k, 0:3], prims[:, k, 3:6], prims[:, k, 6] = J[:, PARENT[j]], J[:, j], rad[:, j] * s[:, 0]
        k += 1
    if model.knuckles:
        prims[:, k, 0:3], prims[:, k, 3:6], prims[:, k, 6] = J[:, _base(INDEX)], J[:, _base(PINKY)], model.KNUCKLE_RADIUS * s[:, 0]
        k += 1
    if model.forearm:
        back = np.einsum("nij,j->ni", R, -ey) * (model.FOREARM_LENGTH * s)
        prims[:, k, 0:3], prims[:, k, 3:6], prims[:, k, 6] = J[:, WRIST], J[:, WRIST] + back, model.FOREARM_RADIUS * s[:, 0]
        k += 1
    assert k == K
    return J, prims, prim_boxes(prims, frame_shape, paras, flip, margin)


def prim_boxes(prims, frame_shape=(480, 640), paras=ND.PARAS, flip=-1, margin=2, near=1.0):
    """Conservative pixel boxes (n, 4) int32 of primitive tables (n, K, 8).  An end sphere lies in the box [x - r, x + r] x [z - r, z + r];
    x' / z' is monotonic in each variable, so its projection lies between the four corner values; a capsule is the convex hull of its end
    spheres and projection keeps convexity in front of the camera.  A capsule with one end nearer than `near` mm takes the whole frame; one
    wholly behind the camera takes nothing.  `margin` pixels are added all round.  A table with a non-finite used row takes the whole frame."""
    prims = np.asarray(prims, np.float64)
    n = prims.shape[0]
    fh, fw = frame_shape
    fx, fy, u0, v0 = (float(p) for p in paras)
    out = np.zeros((n, 4), np.int32)
    for i in range(n):
        P = prims[i][~(prims[i][:, 6] <= 0)]
        if not np.isfinite(P).all():
            out[i] = (0, 0, fw, fh)
            continue
        lo_u = lo_v = np.inf
        hi_u = hi_v = -np.inf
        for ax, ay, az, bx, by, bz, r, _ in P:
            if az + r <= 0 and bz + r <= 0:
                continue
            if az - r < near or bz - r < near:
                lo_u, lo_v, hi_u, hi_v = 0, 0, fw, fh
                break
            for x, y, z in ((ax, ay, az), (bx, by, bz)):
                us = [u0 + fx * (x + sx * r) / (z + sz * r) for sx in (-1, 1) for sz in (-1, 1)]
                vs = [v0 + flip * fy * (y + sy * r) / (z + sz * r) for sy in (-1, 1) for sz in (-1, 1)]
                lo_u, hi_u, lo_v, hi_v = min(lo_u, min(us)), max(hi_u, max(us)), min(lo_v, min(vs)), max(hi_v, max(vs))
        if not (lo_u <= hi_u and lo_v <= hi_v):
            continue                                              # nothing in front of the camera: an empty box
        a = int(np.clip(np.floor(lo_u) - margin, 0, fw)), int(np.clip(np.floor(lo_v) - margin, 0, fh))
        b = int(np.clip(np.ceil(hi_u) + margin + 1, 0, fw)), int(np.clip(np.ceil(hi_v) + margin + 1, 0, fh))
        out[i] = (a[0], a[1], b[0], b[1])
    return out


def labels(joints21, jt_num=14, center_jitter_mm=0.0, seed=0):
    """-> (labels_xyz (n, jt_num, 3), centers (n, 3)).  jt_num = 14: the NYU evaluation order vis_tool._SKELETON["nyu"] draws -- tip and mid
    joint of pinky, ring, middle and index; thumb tip, mid and base; two wrist points (the wrist moved 0.3 of the index-base -> pinky-base
    vector to either side); the palm centre (mean of the wrist and the four finger bases) last.  jt_num = 21: all skeletal joints.  Centres
    are the mean of the labelled joints (the analogue of the refined-centre files), plus seeded uniform jitter of +-center_jitter_mm."""
    J = np.asarray(joints21, np.float64)
    if jt_num == 21:
        lab = J.copy()
    elif jt_num == 14:
        across = J[:, _base(INDEX)] - J[:, _base(PINKY)]
        palm = (J[:, WRIST] + J[:, _base(INDEX)] + J[:, _base(MIDDLE)] + J[:, _base(RING)] + J[:, _base(PINKY)]) / 5.0
        lab = np.concatenate([J[:, _NYU_FROM21], (J[:, WRIST] + 0.3 * across)[:, None], (J[:, WRIST] - 0.3 * across)[:, None], palm[:, None]], 1)
    else:
        raise ValueError("jt_num is 14 (the NYU evaluation joints) or 21 (all skeletal joints), not %r" % (jt_num,))
    centers = lab.mean(1)
    if center_jitter_mm:
        centers = centers + (np.random.RandomState(seed).uniform(size=centers.shape) * 2 - 1) * float(center_jitter_mm)
    return lab, centers


# ---- the renderer's statement --------------------------------------------------------------------------------------------------------
def _mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def hash_u32(seed, frame, pixel):
    """32-bit hash of (seed, global frame index, pixel index): uint32 arithmetic only, as csrc/awr_synth.hip writes it."""
    with np.errstate(over="ignore"):
        pixel = np.asarray(pixel).astype(np.uint32)
        h = np.full(pixel.shape, (int(seed) & 0xFFFFFFFF), np.uint32) ^ (np.full(pixel.shape, int(frame) & 0xFFFFFFFF, np.uint32) * np.uint32(0x9E3779B1))
        h = _mix32(h)
        h = h ^ (pixel * np.uint32(0x85EBCA77))
        return _mix32(h)


def _check_render_args(K, fh, fw, paras, flip, background_mm, noise_mm):
    if K > MAX_PRIMS:
        raise ValueError("a frame has at most %d primitives, not %d" % (MAX_PRIMS, K))
    if not (0 < fh <= MAX_FRAME_EDGE and 0 < fw <= MAX_FRAME_EDGE):
        raise ValueError("frame shape %r is outside [1, %d]" % ((fh, fw), MAX_FRAME_EDGE))
    if flip not in (1, -1) or float(paras[0]) == 0.0 or float(paras[1]) == 0.0:
        raise ValueError("flip is +1 or -1 and the focal lengths are not zero")
    if not (0 <= int(background_mm) <= 65535 and 0 <= int(noise_mm) <= 32767):
        raise ValueError("background_mm is in [0, 65535] and noise_mm in [0, 32767]")


def render_frame(prims, bbox, frame_shape=(480, 640), paras=ND.PARAS, flip=-1, background_mm=0, noise_mm=0, seed=0, frame=0):
    """One frame of the statement: -> (uint16 (fh, fw), unrounded float64 (fh, fw) with +inf where nothing was hit, status)."""
    fh, fw = frame_shape
    P = np.asarray(prims, np.float64).reshape(-1, 8)
    _check_render_args(len(P), fh, fw, paras, flip, background_mm, noise_mm)
    fx, fy, u0, v0 = (np.float64(p) for p in paras)
    bg, a = int(background_mm), int(noise_mm)
    ulo, vlo, uhi, vhi = (int(x) for x in bbox)
    ulo, vlo, uhi, vhi = max(ulo, 0), max(vlo, 0), min(uhi, fw), min(vhi, fh)
    best = np.full((fh, fw), np.inf)
    used = P[~(P[:, 6] <= 0)]
    bad = not np.isfinite(used).all()
    if not bad and ulo < uhi and vlo < vhi:
        with np.errstate(all="ignore"):
            uu = np.arange(ulo, uhi, dtype=np.float64)[None, :]
            vv = np.arange(vlo, vhi, dtype=np.float64)[:, None]
            dx = np.broadcast_to((uu - u0) / fx, (vhi - vlo, uhi - ulo))
            dy = np.broadcast_to(np.float64(flip) * ((vv - v0) / fy), (vhi - vlo, uhi - ulo))
            dd = (dx * dx + dy * dy) + 1.0
            t = np.full(dx.shape, np.inf)
            for ax, ay, az, bx, by, bz, r, _ in used:
                oax, oay, oaz, obx, oby, obz = -ax, -ay, -az, -bx, -by, -bz
                bax, bay, baz = bx - ax, by - ay, bz - az
                rr = r * r
                baba = (bax * bax + bay * bay) + baz * baz
                baoa = (bax * oax + bay * oay) + baz * oaz
                oaoa = (oax * oax + oay * oay) + oaz * oaz
                obob = (obx * obx + oby * oby) + obz * obz
                cc = (baba * oaoa - baoa * baoa) - rr * baba
                ca, cb = oaoa - rr, obob - rr
                bard = (bax * dx + bay * dy) + baz
                rdoa = (dx * oax + dy * oay) + oaz
                rdob = (dx * obx + dy * oby) + obz
                A = baba * dd - bard * bard
                B = baba * rdoa - baoa * bard
                H = B * B - A * cc
                cyl = (A > 0) & (H > 0)
                tc = (-B - np.sqrt(np.where(cyl, H, 0.0))) / np.where(cyl, A, 1.0)
                y = baoa + tc * bard
                body = cyl & (y > 0) & (y < baba) & (B < 0) & (cc > 0)
                t = np.where(body & (tc < t), tc, t)
                for use, rd, c in ((~(A > 0) | (cyl & (y <= 0)), rdoa, ca), (~(A > 0) | (cyl & (y >= baba)), rdob, cb)):
                    Hs = rd * rd - dd * c
                    hit = use & (Hs > 0) & (rd < 0) & (c > 0)
                    ts = (-rd - np.sqrt(np.where(hit, Hs, 0.0))) / dd
                    t = np.where(hit & (ts < t), ts, t)
            best[vlo:vhi, ulo:uhi] = t
    zr = np.floor(np.where(best < np.inf, best, 0.0) + 0.5)
    zi = np.minimum(np.maximum(zr, 1.0), 65535.0).astype(np.int64)
    hit = best < np.inf
    if bg > 0:
        hit &= zi < bg
    out = np.where(hit, zi, bg)
    if a > 0:
        pix = (np.arange(fh, dtype=np.int64)[:, None] * fw + np.arange(fw, dtype=np.int64)[None, :])
        nz = (hash_u32(seed, frame, pix) % np.uint32(2 * a + 1)).astype(np.int64) - a
        noisy = np.minimum(np.maximum(out + nz, 1), 65535)
        out = np.where(hit | (bg > 0), noisy, out)
    status = BAD_PRIM if bad else (OK if hit.any() else EMPTY)
    return out.astype(np.uint16), np.where(hit, best, np.inf), status


def render(prims, bbox, frame_shape=(480, 640), paras=ND.PARAS, flip=-1, background_mm=0, noise_mm=0, seed=0, frame0=0, return_unrounded=False,
           return_status=False):
    """The statement: prims (n, K, 8), bbox (n, 4) -> frames (n, fh, fw) uint16 [, unrounded depths (n, fh, fw) float64, +inf where no
    capsule counts][, status (n,) int32].  Frame i hashes its noise with the GLOBAL index frame0 + i: chunks equal one call."""
    prims = np.asarray(prims, np.float64)
    bbox = np.asarray(bbox)
    if prims.ndim != 3 or prims.shape[2] != 8 or bbox.shape != (prims.shape[0], 4):
        raise ValueError("prims is (n, K, 8) and bbox (n, 4), got %s and %s" % (prims.shape, bbox.shape))
    n = prims.shape[0]
    fh, fw = frame_shape
    frames = np.empty((n, fh, fw), np.uint16)
    raw = np.empty((n, fh, fw), np.float64) if return_unrounded else None
    status = np.zeros(n, np.int32)
    for i in range(n):
        f, z, status[i] = render_frame(prims[i], bbox[i], frame_shape, paras, flip, background_mm, noise_mm, seed, frame0 + i)
        frames[i] = f
        if raw is not None:
            raw[i] = z
    res = (frames,) + ((raw,) if return_unrounded else ()) + ((status,) if return_status else ())
    return res if len(res) > 1 else frames


def render_device(prims, bbox, out, row=0, paras=ND.PARAS, flip=-1, background_mm=0, noise_mm=0, seed=0, frame0=0, status=None):
    """awr_synth_render: prims (n, K, 8) float64 and bbox (n, 4) int32 (numpy arrays are uploaded; device tensors are used in place) ->
    rows [row, row + n) of `out`, an (N, fh, fw) uint16 device tensor.  -> status (n,) int32 on the device, nothing synchronised."""
    import torch
    from . import _lib as L
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint16 or out.dim() != 3 or not out.is_cuda or not out.is_contiguous():
        raise L.AwrError("out must be a contiguous (N, fh, fw) uint16 device tensor")
    dev = out.device
    if not isinstance(prims, torch.Tensor):
        prims = torch.from_numpy(np.ascontiguousarray(prims, dtype=np.float64)).to(dev)
    if not isinstance(bbox, torch.Tensor):
        bbox = torch.from_numpy(np.ascontiguousarray(bbox, dtype=np.int32)).to(dev)
    if prims.dtype != torch.float64 or prims.dim() != 3 or prims.shape[2] != 8 or bbox.dtype != torch.int32 or tuple(bbox.shape) != (prims.shape[0], 4):
        raise L.AwrError("prims is (n, K, 8) float64 and bbox (n, 4) int32")
    n, K = int(prims.shape[0]), int(prims.shape[1])
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=dev)
    elif status.dtype != torch.int32 or status.numel() < n:
        raise L.AwrError("status must hold n int32 values")
    N, fh, fw = (int(v) for v in out.shape)
    fx, fy, u0, v0 = (float(p) for p in paras)
    L.call("awr_synth_render", L.ptr(prims), L.ptr(bbox), n, K, fh, fw, fx, fy, u0, v0, int(flip), int(background_mm), int(noise_mm),
           int(seed) & 0xFFFFFFFF, int(frame0), out.data_ptr(), int(row), N, L.ptr(status), L.stream())
    return status


# ---- the dataset ---------------------------------------------------------------------------------------------------------------------
class SyntheticFrames:
    """n procedural hands: poses (sample_poses(n, seed, **pose_options)) -> kinematics -> raw (n, fh, fw) uint16 frames -> a dataset.

    device: "cuda" -- the frames are rendered chunk by chunk into one device tensor; `.frame_store` is a nyu_device.FrameStore over it and
    `.dataset` a DeviceNYU (hand it to Trainer: a dataset that carries `frame_store` gets its Renderer).  None -- the frames are rendered by
    the numpy statement into host memory (`.frames`) and `.dataset` is the host nyu_data.NYU: for small n on a machine without a GPU.
    `.labels_xyz` (n, jt_num, 3), `.centers` (n, 3), `.joints21` (n, 21, 3), `.prims`, `.bbox` are numpy arrays; `.status` (n,) int32 holds
    the renderer's code per frame (a device tensor with a device).  The dataset's test cube is the same for every frame: the NYU rule that
    shrinks it for frames >= 2440 describes that dataset's second subject and does not apply here.
    poses: a pose dict of n rows (sample_poses' keys, e.g. sample_sequences' output) used INSTEAD of the class's own sample_poses call."""

    def __init__(self, n, seed, phase, jt_num=14, img_size=128, cube=(300, 300, 300), aug_para=None, frame_shape=(480, 640), paras=ND.PARAS,
                 flip=-1, device="cuda", chunk=256, forearm=True, background_mm=0, noise_mm=0, center_jitter_mm=0.0, poses=None, **pose_options):
        self.n, self.seed, self.phase = int(n), int(seed), phase
        self.frame_shape, self.paras, self.flip = (int(frame_shape[0]), int(frame_shape[1])), tuple(float(p) for p in paras), int(flip)
        fh, fw = self.frame_shape
        if device is not None:
            import torch
            from . import _lib as L
            from . import nyu_device as DV
            if not torch.cuda.is_available():
                raise L.AwrError("SyntheticFrames(device=%r) renders with a HIP kernel and needs a GPU: none is visible -- device=None renders "
                                 "small sets on the host" % (device,))
            need = self.n * fh * fw * 2
            free = torch.cuda.mem_get_info(torch.device(device))[0]
            if need > free:           # before anything is drawn or allocated
                raise L.AwrError("%d frames of %d x %d need %.1f GB of device memory and %.1f GB are free" % (self.n, fh, fw, need / 1e9, free / 1e9))
        self.model = HandModel(forearm=forearm)
        if poses is None:
            poses = sample_poses(self.n, self.seed, self.model, cube=cube, frame_shape=self.frame_shape, paras=self.paras, flip=self.flip,
                                 **pose_options)
        elif pose_options:
            raise ValueError("poses= replaces the sample_poses call: its options %s have nothing to act on" % sorted(pose_options))
        elif any(len(v) != self.n for v in poses.values()):
            raise ValueError("poses holds %s rows, not n = %d" % (sorted({len(v) for v in poses.values()}), self.n))
        self.poses = poses
        self.joints21, self.prims, self.bbox = forward_kinematics(self.poses, self.model, self.frame_shape, self.paras, self.flip)
        self.labels_xyz, self.centers = labels(self.joints21, jt_num, center_jitter_mm, self.seed)
        kw = dict(paras=self.paras, flip=self.flip, background_mm=background_mm, noise_mm=noise_mm, seed=self.seed)
        ds_kw = dict(img_size=img_size, aug_para=aug_para, cube=cube, jt_num=jt_num)
        if device is None:
            self.frames, self.status = render(self.prims, self.bbox, self.frame_shape, return_status=True, **kw)
            self.frame_store = None
            self.dataset = ND.NYU.from_arrays(self.frames, self.labels_xyz, self.centers, phase, **ds_kw)
        else:
            data = torch.empty((self.n, fh, fw), dtype=torch.uint16, device=device)
            self.status = torch.empty(self.n, dtype=torch.int32, device=data.device)
            chunk = max(1, min(int(chunk), MAX_CALL_FRAMES))
            for lo in range(0, self.n, chunk):
                hi = min(self.n, lo + chunk)
                render_device(self.prims[lo:hi], self.bbox[lo:hi], data, row=lo, frame0=lo, status=self.status[lo:hi], **kw)
            self.frames = None
            self.frame_store = DV.FrameStore.from_device(data)
            self.dataset = DV.DeviceNYU.from_arrays((self.n, fh, fw), self.labels_xyz, self.centers, phase, **ds_kw)
            self.dataset.frame_store = self.frame_store
        ds = self.dataset
        ds.paras, ds.flip = self.paras, self.flip
        ds.aug.paras, ds.aug.flip = self.paras, self.flip
        ds.test_cube = np.ones([self.n, 3]) * ds.cube

    def __len__(self):
        return self.n

    def frames_host(self):
        """the frames as a numpy array (downloads them from the device)"""
        return self.frames if self.frames is not None else self.frame_store.data.cpu().numpy()

    def check(self):
        """Synchronising: raise if any frame's primitive table was refused (BAD_PRIM); -> the number of EMPTY frames."""
        st = np.asarray(self.status.cpu() if hasattr(self.status, "cpu") else self.status)
        if (st == BAD_PRIM).any():
            raise ValueError("frames %s: %s" % (np.nonzero(st == BAD_PRIM)[0].tolist(), STATUS_NAMES[BAD_PRIM]))
        return int((st == EMPTY).sum())
