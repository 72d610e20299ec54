"""A label-free check of joints against the depth frame: per joint, and per sample along a bone, whether the surface the
sensor saw at the point's pixel is roughly there (ON), something much nearer covers it (OCCLUDED) or only background or nothing is there
(OFF).  A depth frame is a second witness next to `confidence=`, which is the network's opinion of itself, and it needs no labels.

  * `joints_surface`: the numpy statement of awr_joints_surface (csrc/awr_surface.hip); the kernel equals it bit for bit.
  * `joints_surface_device`: the entry point on a FrameStore-like object, shaped like awr_amd.detect.denoise_device.
  * `check_surface_option`, `bone_table`: what Predictor(surface=...) and predict.py --surface validate with.
  * `awr_joints_surface`: the entry point's argument list, stated once; the module's one L.call.

The defaults (SURFACE_DEFAULTS) are engineering choices.  The rule separates true from displaced joints on the project's procedural hands
(profiles/surface_check.txt); on real frames it is UNMEASURED."""
import numpy as np

ON, OCCLUDED, OFF, OUTSIDE, SKIPPED = 0, 1, 2, 3, 4
CODE_NAMES = {ON: "on", OCCLUDED: "occluded", OFF: "off", OUTSIDE: "outside", SKIPPED: "skipped"}
ROW_OK, ROW_SKIPPED, ROW_BAD_FRAME = 0, 1, 2
MAX_RADIUS, MAX_JOINTS, MAX_BONES, MAX_SAMPLES = 3, 256, 64, 7
# Engineering choices, not measured on real frames: a 3 x 3 window, a joint at most 40 mm behind and 15 mm in front of a seen surface,
# one such pixel is enough, three samples along each bone of vis_tool's skeleton.
SURFACE_DEFAULTS = dict(radius=1, in_mm=40.0, out_mm=15.0, min_on=1, bones=None, samples=3)
_LIMIT = 1073741824.0          # awr_frame.h's trunc_clamped


def _int(x, what, none=False):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise TypeError("%s is an int%s, not %r" % (what, " or None" if none else "", x))
    return int(x)


def _mm(x, what, value):
    if isinstance(x, (bool, str, bytes)) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise TypeError("%s is a number of millimetres >= 0, not %r" % (what, x))
    if value and not (np.isfinite(float(x)) and float(x) >= 0.0):
        raise ValueError("%s = %r must be finite and >= 0" % (what, x))
    return float(x)


def _check_surface(radius=1, in_mm=40.0, out_mm=15.0, min_on=1, bones=None, samples=3, value=True):
    """Validate the six knobs: -> (radius, in_mm, out_mm, min_on, bones None | a list of (from, to) int pairs, samples).  value=False
    checks the types alone (joints_surface_device: a value the entry point refuses gets its message from there)."""
    radius, min_on, samples = _int(radius, "radius"), _int(min_on, "min_on"), _int(samples, "samples")
    in_mm, out_mm = _mm(in_mm, "in_mm", value), _mm(out_mm, "out_mm", value)
    if value and not 0 <= radius <= MAX_RADIUS:
        raise ValueError("radius = %d is outside [0, %d]" % (radius, MAX_RADIUS))
    if value and not 1 <= min_on <= (2 * radius + 1) ** 2:
        raise ValueError("min_on = %d is outside [1, %d], the pixels of a radius-%d window" % (min_on, (2 * radius + 1) ** 2, radius))
    if value and not 1 <= samples <= MAX_SAMPLES:
        raise ValueError("samples = %d is outside [1, %d]" % (samples, MAX_SAMPLES))
    if bones is not None:
        if isinstance(bones, (str, bytes, dict)) or not hasattr(bones, "__len__"):
            raise TypeError("bones is None or a sequence of (from, to) joint index pairs, not %r" % (bones,))
        pairs = []
        for b in bones:
            if isinstance(b, (str, bytes)) or not hasattr(b, "__len__") or len(b) != 2:
                raise TypeError("a bone is a (from, to) pair of joint indices, not %r" % (b,))
            pairs.append((_int(b[0], "a bone's joint index"), _int(b[1], "a bone's joint index")))
        if len(pairs) > MAX_BONES:
            raise ValueError("bones holds %d pairs: at most %d are possible" % (len(pairs), MAX_BONES))
        bones = pairs
    return radius, in_mm, out_mm, min_on, bones, samples


def check_surface_option(surface):
    """Predictor(surface=...): None | True (SURFACE_DEFAULTS) | a dict with any of the keys radius / in_mm / out_mm / min_on / bones /
    samples over those defaults -> None | a dict of the six checked values (bones: None or a list of pairs; bone_table resolves it)."""
    if surface is None:
        return None
    if surface is True:
        surface = {}
    if not isinstance(surface, dict):
        raise TypeError("surface is None, True or a dict with the keys radius / in_mm / out_mm / min_on / bones / samples, not %r" % (surface,))
    extra = set(surface) - set(SURFACE_DEFAULTS)
    if extra:
        raise ValueError("surface has unknown keys %s (radius, in_mm, out_mm, min_on, bones and samples exist)" % sorted(extra))
    return dict(zip(("radius", "in_mm", "out_mm", "min_on", "bones", "samples"), _check_surface(**dict(SURFACE_DEFAULTS, **surface))))


def default_bones(J):
    """The flattened (from, to) pairs of vis_tool._SKELETON: "nyu" for J = 14, "hands" for J = 21, no bones for any other J."""
    from .vis_tool import _SKELETON
    key = {14: "nyu", 21: "hands"}.get(int(J))
    return [] if key is None else [(int(a), int(b)) for _, bones in _SKELETON[key] for a, b in bones]


def bone_table(bones, J):
    """bones (None: default_bones(J)) -> an (n_bones, 2) int32 array; an index outside [0, J) is refused here, before any launch."""
    pairs = default_bones(J) if bones is None else _check_surface(bones=bones)[4]
    for a, b in pairs:
        if not (0 <= a < J and 0 <= b < J):
            raise ValueError("bone (%d, %d) has a joint index outside [0, J = %d)" % (a, b, J))
    return np.asarray(pairs, np.int32).reshape(-1, 2)


def _round_clamped(x):
    """floor(x + 0.5) of finite doubles as integers, clamped before the conversion as awr_frame.h's trunc_clamped is"""
    return np.clip(np.floor(x + 0.5), -_LIMIT, _LIMIT).astype(np.int64)


def _statement(frames, frame_idx, uvd, status, ustatus, bones, samples, radius, in_mm, out_mm, min_on):
    """The rule itself over n rows, nothing validated: bones an (n_bones, 2) integer array whose indices may lie outside [0, J), as the
    entry point tolerates them."""
    frames = np.asarray(frames)
    uvd = np.asarray(uvd)
    n, J = uvd.shape[:2]
    n_frames, fh, fw = frames.shape
    fidx = np.asarray(frame_idx, np.int64).reshape(n)
    status, ustatus = np.asarray(status).reshape(n), np.asarray(ustatus).reshape(n)
    P = uvd.astype(np.float64)                                            # a joint's point: its float32 values converted exactly
    bones = np.asarray(bones, np.int64).reshape(-1, 2)
    if len(bones):
        ok = ((bones >= 0) & (bones < J)).all(1)
        ia, ib = np.clip(bones[:, 0], 0, J - 1), np.clip(bones[:, 1], 0, J - 1)
        A, B = P[:, ia], P[:, ib]                                         # (n, n_bones, 3)
        with np.errstate(invalid="ignore", over="ignore"):
            S = np.stack([A + (B - A) * (s / (samples + 1)) for s in range(1, samples + 1)], 2)          # (n, n_bones, samples, 3)
        S[:, ~ok] = np.nan                                                # a bone with a bad index: OUTSIDE samples
        P = np.concatenate([P, S.reshape(n, -1, 3)], 1)                   # sample s of bone b is point J + b * samples + (s - 1)
    T = P.shape[1]
    u, v, d = P[..., 0], P[..., 1], P[..., 2]
    finite = np.isfinite(u) & np.isfinite(v) & np.isfinite(d)
    pu, pv = _round_clamped(np.where(finite, u, 0.0)), _round_clamped(np.where(finite, v, 0.0))
    inside = finite & (pu >= 0) & (pu < fw) & (pv >= 0) & (pv < fh)
    row_status = np.where((status != 0) | (ustatus != 0), ROW_SKIPPED, np.where((fidx < 0) | (fidx >= n_frames), ROW_BAD_FRAME, ROW_OK)).astype(np.int32)
    frow = np.where(row_status == ROW_OK, fidx, 0)[:, None]
    n_on, n_front = np.zeros((n, T), np.int64), np.zeros((n, T), np.int64)
    seen = np.zeros((n, T), bool)
    best, best_abs = np.zeros((n, T)), np.zeros((n, T))
    for dv in range(-radius, radius + 1):
        for du in range(-radius, radius + 1):
            x, y = pu + du, pv + dv
            inframe = inside & (x >= 0) & (x < fw) & (y >= 0) & (y < fh)
            dq = frames[frow, np.clip(y, 0, fh - 1), np.clip(x, 0, fw - 1)]
            valid = inframe & (dq != 0)
            with np.errstate(invalid="ignore", over="ignore"):
                g = np.where(valid, d, 0.0) - dq.astype(np.float64)
            ag = np.abs(g)
            n_on += valid & (-out_mm <= g) & (g <= in_mm)
            n_front += valid & (g > in_mm)
            better = valid & (~seen | (ag < best_abs) | ((ag == best_abs) & (g > best)))
            best, best_abs = np.where(better, g, best), np.where(better, ag, best_abs)
            seen |= valid
    codes = np.where(n_on >= min_on, ON, np.where(n_front >= 1, OCCLUDED, OFF))
    codes = np.where(inside, codes, OUTSIDE).astype(np.int32)
    gap = np.full((n, T), np.nan, np.float32)
    gap[seen] = best[seen].astype(np.float32)
    live = row_status == ROW_OK
    codes[~live] = SKIPPED
    gap[~live] = np.nan
    counts = np.zeros((n, 8), np.int32)
    for c in (ON, OCCLUDED, OFF, OUTSIDE):
        counts[:, c] = (codes[:, :J] == c).sum(1)
        counts[:, 4 + c] = (codes[:, J:] == c).sum(1)
    counts[~live] = 0
    return codes[:, :J].copy(), gap[:, :J].copy(), counts, row_status


def joints_surface(frames, frame_idx, uvd, status, ustatus, radius=1, in_mm=40.0, out_mm=15.0, min_on=1, bones=None, samples=3):
    """The statement of awr_joints_surface, batched over rows: frames (n_frames, fh, fw) uint16 millimetres (0: no measurement),
    frame_idx (n,) the frame of every row, uvd (n, J, 3) float32 original-image pixel u, v and depth in millimetres (what a prediction's
    `uvd` holds), status, ustatus (n,) the rows' codes -> (codes (n, J) int32, gap_mm (n, J) float32, counts (n, 8) int32, row_status (n,)
    int32).  bones: None -- vis_tool._SKELETON's pairs, "nyu" for J = 14, "hands" for J = 21, none otherwise -- or up to 64 (from, to)
    pairs.  The rule:

    A point is a triple (u, v, d) in float64. A joint's point is its float32 values converted exactly. Sample s = 1 ... samples of bone
    (a, b) is p = A + (B - A) * (s / (samples + 1)), per component in float64, in exactly this order. It is linear in uvd, not in camera
    space. That is good enough at a hand's size.
    For one point:
      1. If u, v or d is not finite, the code is OUTSIDE.
      2. Otherwise pu = floor(u + 0.5) and pv = floor(v + 0.5), clamped before the integer conversion as awr_frame.h's trunc_clamped
         does. If pu is not in [0, fw) or pv is not in [0, fh), the code is OUTSIDE.
      3. W is the set of in-frame pixels of the (2 * radius + 1)^2 window around (pu, pv). The centre is included and the window is
         clipped at the frame's edges.
      4. For q in W with d_q != 0: g_q = d - (double)d_q. This is exact in double.
      5. n_on = #{-out_mm <= g_q <= in_mm}, n_front = #{g_q > in_mm}.
      6. The code is ON (0) if n_on >= min_on; else OCCLUDED (1) if n_front >= 1; else OFF (2). A window of zeros only is OFF too.
      7. The gap is the g_q of smallest |g_q|, the positive one on a tie of +g and -g, rounded to float32. It is NaN if no pixel of W
         is valid, and NaN for OUTSIDE. It is a value, not a position, so the scan order cannot matter.
    A row whose status is not OK or whose ustatus is not 0 is SKIPPED: every code of the row is 4, its gaps are NaN, its counts are 0 and
    its row_status is 1 (its frame index is not looked at). Otherwise a row whose frame index lies outside the store gets row_status 2
    and the same outputs.
    counts: joints ON / OCCLUDED / OFF / OUTSIDE, then bone samples ON / OCCLUDED / OFF / OUTSIDE."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint16 or frames.ndim != 3:
        raise ValueError("frames is an (n_frames, h, w) uint16 array of millimetres, not %s %s" % (frames.dtype, frames.shape))
    uvd = np.asarray(uvd)
    if uvd.dtype != np.float32 or uvd.ndim != 3 or uvd.shape[2] != 3 or not 1 <= uvd.shape[1] <= MAX_JOINTS:
        raise ValueError("uvd is an (n, J, 3) float32 array with J in [1, %d], not %s %s" % (MAX_JOINTS, uvd.dtype, uvd.shape))
    radius, in_mm, out_mm, min_on, bones, samples = _check_surface(radius, in_mm, out_mm, min_on, bones, samples)
    return _statement(frames, frame_idx, uvd, status, ustatus, bone_table(bones, uvd.shape[1]), samples, radius, in_mm, out_mm, min_on)


def awr_joints_surface(frames, ftype, n_frames, fh, fw, frame_idx, uvd, status, ustatus, n, J, n_valid, bones, n_bones, samples, radius, in_mm,
                       out_mm, min_on, codes, gap_mm, counts, row_status):
    """The entry point's argument list, stated once (as detect_calls states the detector's): buffers are device addresses (int; None:
    NULL), the values in ABI order, the stream, one L.call.  Nothing is allocated, validated or computed."""
    from . import _lib as L
    L.call("awr_joints_surface", frames, int(ftype), int(n_frames), int(fh), int(fw), frame_idx, uvd, status, ustatus, int(n), int(J), int(n_valid),
           bones, int(n_bones), int(samples), int(radius), float(in_mm), float(out_mm), int(min_on), codes, gap_mm, counts, row_status, L.stream())


def joints_surface_device(store, frame_idx, uvd, status, ustatus, radius=1, in_mm=40.0, out_mm=15.0, min_on=1, bones=None, samples=3,
                          n_valid=None, out=None):
    """awr_joints_surface on a FrameStore-like object: uvd (n, J, 3) float32, status, ustatus (n,) int32 on the device -> (codes (n, J)
    int32, gap_mm (n, J) float32, counts (n, 8) int32, row_status (n,) int32) on the device, nothing synchronised.  n_valid: rows that
    count (default: all); rows at or past it are not written.  out: the four tensors to write into.  The types and the bone table's
    indices are checked here; a value the entry point refuses gets its message from there."""
    import torch
    from . import _lib as L
    from .detect import _frame_index, _source
    radius, in_mm, out_mm, min_on, bones, samples = _check_surface(radius, in_mm, out_mm, min_on, bones, samples, value=False)
    dev = store.data.device
    idx = _frame_index(frame_idx, dev)
    n = int(idx.shape[0])
    if uvd.dim() != 3 or uvd.shape[0] != n or uvd.shape[2] != 3 or uvd.dtype != torch.float32:
        raise ValueError("uvd is an (n = %d, J, 3) float32 tensor, not %s %s" % (n, uvd.dtype, tuple(uvd.shape)))
    J = int(uvd.shape[1])
    table = bone_table(bones, J) if J >= 1 else np.zeros((0, 2), np.int32)
    bones_t = torch.from_numpy(table).to(dev) if len(table) else None
    if out is None:
        out = (torch.empty((n, J), dtype=torch.int32, device=dev), torch.empty((n, J), dtype=torch.float32, device=dev),
               torch.empty((n, 8), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    codes, gap, counts, row_status = out
    awr_joints_surface(*_source(store), idx.data_ptr(), L.ptr(uvd), L.ptr(status), L.ptr(ustatus), n, J, n if n_valid is None else n_valid,
                       L.ptr(bones_t), len(table), samples, radius, in_mm, out_mm, min_on, L.ptr(codes), L.ptr(gap), L.ptr(counts), L.ptr(row_status))
    return codes, gap, counts, row_status
