"""A static-scene background model in front of every stage of the prediction path.  Every other stage assumes that the
hand is the nearest thing in the frame; with a fixed sensor over a desk, or facing a seated person, a table edge, a monitor, a knee or a
torso is nearer.  The classical answer for a fixed depth camera: learn one depth per pixel from frames of the scene without a hand, and
keep of every later frame only what is clearly nearer than that.

  * `learn`, `foreground`: the numpy statements of awr_background_learn and awr_frames_foreground (csrc/awr_background.hip); the kernels
    equal them bit for bit.
  * `learn_device`, `foreground_device`: the entry points on a FrameStore-like object, shaped like awr_amd.detect.denoise_device.
  * `check_background_option`: what Predictor(background=...), FrameStore.foreground and predict.py --background validate with.
  * `awr_background_learn`, `awr_frames_foreground`: the entry points' argument lists, stated once; the module's two L.calls.  The
    wrappers and the Predictor launch through them.

The defaults (BACKGROUND_DEFAULTS) are engineering choices.  The effect is measured on procedural cluttered scenes alone
(profiles/background_accuracy.txt); on real frames it is UNMEASURED."""
import numpy as np

RANKS = {"min": 0, "median": 1, "max": 2}          # AWR_BG_MIN, AWR_BG_MEDIAN, AWR_BG_MAX
UNKNOWN = {"drop": 0, "keep": 1}                   # unknown_keep: what a pixel without a known background (model 0) does
MAX_FRAMES = 64                                    # AWR_BG_MAX_FRAMES
MAX_STEP = 65535
# Engineering choices, not measured on real frames: 30 mm in front of the background counts as foreground (a few sigma of a consumer
# sensor's range noise at desk distance), a pixel whose background was never seen stays, the model is not adapted, one model for every
# batch slot, the lower median of the learning frames, one valid frame is enough.
BACKGROUND_DEFAULTS = dict(margin=30.0, unknown="keep", adapt=None, shared=True, rank="median", min_valid=1)


def _int(x, what, none=False):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise TypeError("%s is an int%s, not %r" % (what, " or None" if none else "", x))
    return int(x)


def _check_apply(margin=30.0, unknown="keep", adapt=None, value=True):
    """Validate foreground's three knobs: -> (margin float, unknown "keep" | "drop", adapt None | int).  value=False checks the types alone
    (foreground_device: a value the entry point refuses gets its message from there)."""
    if isinstance(margin, (bool, str, bytes)) or not isinstance(margin, (int, float, np.integer, np.floating)):
        raise TypeError("margin is a number of millimetres >= 0, not %r" % (margin,))
    if value and not float(margin) >= 0.0:
        raise ValueError("margin = %r must be >= 0 (infinity: nothing in front of a known background is kept)" % (margin,))
    if unknown not in UNKNOWN:
        raise ValueError("unknown is \"keep\" or \"drop\" (a pixel whose model is 0), not %r" % (unknown,))
    if adapt is not None:
        adapt = _int(adapt, "adapt", none=True)
        if value and not 1 <= adapt <= MAX_STEP:
            raise ValueError("adapt = %d is outside [1, %d] millimetres per call (None: the model is only read)" % (adapt, MAX_STEP))
    return float(margin), unknown, adapt


def _check_learn(rank="median", min_valid=1, n=None, value=True):
    """Validate learn's two knobs (against n listed frames where n is given): -> (rank name, min_valid int)"""
    if rank not in RANKS:
        raise ValueError("rank is one of %s, not %r" % (sorted(RANKS), rank))
    min_valid = _int(min_valid, "min_valid")
    if value and not 1 <= min_valid <= (MAX_FRAMES if n is None else n):
        raise ValueError("min_valid = %d is outside [1, %d]%s" % (min_valid, MAX_FRAMES if n is None else n, "" if n is None else ", the listed frames"))
    return rank, min_valid


def check_background_option(background):
    """Predictor(background=...): None | True (BACKGROUND_DEFAULTS) | a dict with any of the keys margin / unknown / adapt / shared / rank /
    min_valid over those defaults -> None | a dict of the six checked values."""
    if background is None:
        return None
    if background is True:
        background = {}
    if not isinstance(background, dict):
        raise TypeError("background is None, True or a dict with the keys margin / unknown / adapt / shared / rank / min_valid, not %r" % (background,))
    extra = set(background) - set(BACKGROUND_DEFAULTS)
    if extra:
        raise ValueError("background has unknown keys %s (margin, unknown, adapt, shared, rank and min_valid exist)" % sorted(extra))
    o = dict(BACKGROUND_DEFAULTS, **background)
    if not isinstance(o["shared"], bool):
        raise TypeError("shared is True (one model for every batch slot) or False (one per batch slot), not %r" % (o["shared"],))
    margin, unknown, adapt = _check_apply(o["margin"], o["unknown"], o["adapt"])
    rank, min_valid = _check_learn(o["rank"], o["min_valid"])
    return dict(margin=margin, unknown=unknown, adapt=adapt, shared=o["shared"], rank=rank, min_valid=min_valid)


def _frame(x, what):
    x = np.asarray(x)
    if x.dtype != np.uint16 or x.ndim != 2:
        raise ValueError("%s is a (h, w) uint16 array of millimetres, not %s %s" % (what, x.dtype, x.shape))
    return x


def learn(frames, rank="median", min_valid=1):
    """The statement of awr_background_learn over frames that are all inside the store: frames (n, fh, fw) uint16 -> the model (fh, fw)
    uint16.  The rule:

    The model is one uint16 depth per pixel, and 0 means "no background known here".
    Input: n listed frames of the store, 1 <= n <= AWR_BG_MAX_FRAMES = 64, a rank in {MIN, MEDIAN, MAX}, min_valid in [1, n].
    For pixel p: V = the multiset { frame_i[p] : frame_i[p] != 0 }, over the listed frames whose index lies inside the store.
      - If |V| < min_valid the model is 0.
      - Otherwise the model is element k of the ascending sort of V: k = 0 (MIN), (|V| - 1) // 2 (MEDIAN, the lower median), |V| - 1 (MAX).
        It is a value that occurs, never an average.
    A listed frame index outside the store contributes no value to any pixel; the call's one status word is then AWR_DET_BAD_FRAME, else
    AWR_DET_OK.

    (A listed index outside the store is, for the model, a frame of zeros: hand this statement such a frame in its place.)
    Here: zeros replaced by a sentinel above every depth, one sort along the frame axis and one take_along_axis."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint16 or frames.ndim != 3:
        raise ValueError("frames is an (n, h, w) uint16 array of millimetres, not %s %s" % (frames.dtype, frames.shape))
    n = frames.shape[0]
    if not 1 <= n <= MAX_FRAMES:
        raise ValueError("a model is learnt from 1 ... %d frames, not %d" % (MAX_FRAMES, n))
    rank, min_valid = _check_learn(rank, min_valid, n)
    keys = np.where(frames != 0, frames.astype(np.int32), 65536)
    keys.sort(axis=0)
    nv = (frames != 0).sum(0)
    k = {"min": np.zeros_like(nv), "median": np.maximum(nv - 1, 0) // 2, "max": np.maximum(nv - 1, 0)}[rank]
    picked = np.take_along_axis(keys, k[None], 0)[0]
    return np.where(nv >= min_valid, picked, 0).astype(np.uint16)


def foreground(frame, model, margin=30.0, unknown="keep", adapt=None):
    """The statement of awr_frames_foreground for one frame and its model row: -> (out (fh, fw) uint16, new_model (fh, fw) uint16; with
    adapt=None a copy of the model).  The rule:

    The pass is pointwise. Every output pixel depends on that pixel of the input frame and of the model alone.
    d = input depth, m = model depth, both as int. margin = floor(min(margin_mm, 65535)) (awr_frame.h's depth_floor, the integer form 4.29
    and 4.30 use; negative or NaN is refused before any launch). unknown_keep in {0, 1}.
      keep = d != 0 and ( m == 0 ? unknown_keep == 1 : d + margin < m )        -- int arithmetic: d + margin may reach 131070 and must not wrap
      out  = keep ? d : 0
    With adapt = step >= 1, for rows b < n_valid only, and only at pixels with d != 0, m != 0 and not keep (a valid background pixel):
      m' = m + min(max(d - m, -step), step)                                    -- between m and d, so it stays in [1, 65535]
    Every other model pixel keeps its value. adapt = 0: the model is only read.

    So an all-zero model with unknown="keep" passes every frame through unchanged; a hand is foreground and is never absorbed; furniture
    moved NEARER after learning stays foreground until the model is learnt again."""
    frame, model = _frame(frame, "a frame"), _frame(model, "a model")
    if frame.shape != model.shape:
        raise ValueError("the frame is %s and the model %s" % (frame.shape, model.shape))
    margin, unknown, adapt = _check_apply(margin, unknown, adapt)
    mg = int(np.floor(min(margin, 65535.0)))
    d, m = frame.astype(np.int64), model.astype(np.int64)
    keep = (d != 0) & np.where(m == 0, UNKNOWN[unknown] == 1, d + mg < m)
    out = np.where(keep, d, 0).astype(np.uint16)
    new = m
    if adapt is not None:
        new = np.where((d != 0) & (m != 0) & ~keep, m + np.clip(d - m, -adapt, adapt), m)
    return out, new.astype(np.uint16)


def awr_background_learn(frames, ftype, n_frames, fh, fw, frame_idx, n, rank, min_valid, model_out, status):
    """The entry point's argument list, stated once (as detect_calls states the detector's): buffers are device addresses (int; None:
    NULL), the values in ABI order, the stream, one L.call.  rank is a name of RANKS.  Nothing is allocated, validated or computed."""
    from . import _lib as L
    L.call("awr_background_learn", frames, int(ftype), int(n_frames), int(fh), int(fw), frame_idx, int(n), RANKS[rank], int(min_valid), model_out,
           status, L.stream())


def awr_frames_foreground(frames, ftype, n_frames, fh, fw, frame_idx, n, n_valid, model, model_rows, per_row, margin, unknown, adapt, out, status):
    """The same for awr_frames_foreground.  unknown is a name of UNKNOWN; adapt=None -> 0 (the model is only read)."""
    from . import _lib as L
    L.call("awr_frames_foreground", frames, int(ftype), int(n_frames), int(fh), int(fw), frame_idx, int(n), int(n_valid), model, int(model_rows),
           1 if per_row else 0, float(margin), UNKNOWN[unknown], 0 if adapt is None else int(adapt), out, status, L.stream())


def learn_device(store, frame_idx, rank="median", min_valid=1, out=None):
    """awr_background_learn on a FrameStore-like object: the frames frame_idx (n,) of the store -> (model (fh, fw) uint16, status (1,) int32)
    on the device, nothing synchronised.  out: a tensor to write into; it must not overlap the store.  The types are checked here; a value
    the entry point refuses gets its message from there."""
    import torch
    from . import _lib as L
    from .detect import _frame_index, _source
    rank, min_valid = _check_learn(rank, min_valid, value=False)
    dev = store.data.device
    idx = _frame_index(frame_idx, dev)
    if out is None:
        out = torch.empty((store.fh, store.fw), dtype=torch.uint16, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    awr_background_learn(*_source(store), idx.data_ptr(), int(idx.shape[0]), rank, min_valid, L.ptr(out), status.data_ptr())
    return out, status


def foreground_device(store, frame_idx, model, margin=30.0, unknown="keep", adapt=None, per_row=False, n_valid=None, out=None):
    """awr_frames_foreground on a FrameStore-like object: model a contiguous (fh, fw) or (rows, fh, fw) uint16 device tensor; per_row: row b
    of the batch reads (and with adapt steps) model row b, else every row reads row 0 -> (out (B, fh, fw) uint16, row b the frame
    frame_idx[b] without its background, status (B,) int32) on the device, nothing synchronised.  With adapt the model tensor is updated
    in place, for rows below n_valid (default: all).  out: a tensor to write into; out, the model and the store must not overlap.  The
    types are checked here; a value the entry point refuses gets its message from there."""
    import torch
    from . import _lib as L
    from .detect import _frame_index, _source
    margin, unknown, adapt = _check_apply(margin, unknown, adapt, value=False)
    dev = store.data.device
    idx = _frame_index(frame_idx, dev)
    B = int(idx.shape[0])
    if not isinstance(model, torch.Tensor) or model.dtype != torch.uint16 or model.dim() not in (2, 3) or tuple(model.shape[-2:]) != (store.fh, store.fw):
        raise ValueError("model is a (%d, %d) or (rows, %d, %d) uint16 device tensor" % (store.fh, store.fw, store.fh, store.fw))
    rows = 1 if model.dim() == 2 else int(model.shape[0])
    if out is None:
        out = torch.empty((B, store.fh, store.fw), dtype=torch.uint16, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    awr_frames_foreground(*_source(store), idx.data_ptr(), B, B if n_valid is None else n_valid, L.ptr(model), rows, per_row, margin, unknown, adapt,
                          L.ptr(out), status.data_ptr())
    return out, status
