"""Temporal joint filter: the numpy statement of awr_joints_filter (csrc/awr_track.hip; include/awr_hip.h "Temporal joint filter";
DESIGN.md 4.25) and its thin device wrapper.

A One-Euro filter (Casiez, Roussel, Vogel 2012) per batch slot, joint and axis over camera-space joints: a first-order low-pass whose
cut-off rises with the filtered speed, so a still hand is smoothed hard and a fast one lags little.  Around it sit the three answers a
consumer of live joints needs: a GATE (a measurement further than gate_mm from the filtered joint is not taken), COASTING (a frame
without a usable measurement yields the held joint for up to max_coast calls, then the track is dropped or re-initialised) and a
constant-velocity LOOK-AHEAD (x + d dt), which Predictor(lead=True) crops the next frame at.

    cfg = OneEuro(beta=0.05, gate_mm=60.0)
    state, count = filter_state(B, J)
    xyz_f, uvd_f, ahead, code = filter_step(state, count, xyz, status, ustatus, conf, cfg, dt, n_valid, paras, flip)

`filter_step` is an explicit loop in IEEE double using + - * /, fabs and comparisons only, in the order the header writes out; the kernel
equals it bit for bit, NaN payloads and signed zeros included.  Whether the filter lowers the joint error on real frames is UNMEASURED;
profiles/track_accuracy.txt holds what it does on procedural sequences.
"""
import collections
import math

import numpy as np

from . import nyu_data as ND

# awr_joints_filter's codes (include/awr_hip.h AWR_FILTER_*)
NONE, INIT, UPDATED, GATED, HELD, REINIT, LOST = 0, 1, 2, 3, 4, 5, 6
FILTER_NAMES = {NONE: "no track and no usable measurement: NaN", INIT: "track started at the measurement", UPDATED: "measurement filtered in",
                GATED: "measurement outside the gate: held", HELD: "no usable measurement: held", REINIT: "coasted too long: restarted at the measurement",
                LOST: "coasted too long without a measurement: track dropped, NaN"}
MAX_JOINTS, MAX_BATCH = 256, 1 << 20
WEIGHTS = {None: 0, "conf": 1}
INT32_MAX = 2 ** 31 - 1

# Units: min_cutoff and d_cutoff in Hz, beta in 1/mm (Hz per mm/s), fps in Hz, gate_mm in mm.  The defaults are ENGINEERING CHOICES --
# the One-Euro paper's starting point (1 Hz, a small beta) at a depth camera's 30 fps, coasting for a sixth of a second -- and are
# unmeasured on real frames: none are available where this was written.
_OneEuro = collections.namedtuple("OneEuro", "min_cutoff beta d_cutoff fps gate_mm max_coast weight conf_floor lead")


class OneEuro(_OneEuro):
    """The filter's configuration, an immutable record.  min_cutoff (Hz): the cut-off of a joint at rest; beta (1/mm): how fast the cut-off
    rises with the filtered speed in mm/s; d_cutoff (Hz): the cut-off of the velocity's own low-pass; fps: 1 / the default dt of a call;
    gate_mm: None, or the largest distance between a measurement and the filtered joint that is still taken; max_coast: calls a track
    survives without an accepted measurement; weight: None | "conf" (the step is scaled by clip(conf, conf_floor, 1)); conf_floor in
    (0, 1]; lead: Predictor crops the next call at the look-ahead joints (needs track=True)."""
    __slots__ = ()

    def __new__(cls, min_cutoff=1.0, beta=0.02, d_cutoff=1.0, fps=30.0, gate_mm=None, max_coast=5, weight=None, conf_floor=0.25, lead=False):
        return super().__new__(cls, min_cutoff, beta, d_cutoff, fps, gate_mm, max_coast, weight, conf_floor, lead)


def _number(name, v):
    if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise TypeError("%s is a number, not %r" % (name, v))
    return float(v)


def check_filter(cfg):
    """True (the defaults) | a dict of OneEuro's fields | a OneEuro -> a validated OneEuro with plain Python values (the rules are
    awr_joints_filter's argument rules)."""
    if cfg is True:
        cfg = OneEuro()
    elif isinstance(cfg, dict):
        unknown = sorted(set(cfg) - set(OneEuro._fields))
        if unknown:
            raise ValueError("unknown filter option(s) %s: the options are %s" % (unknown, list(OneEuro._fields)))
        cfg = OneEuro(**cfg)
    elif not isinstance(cfg, OneEuro):
        raise TypeError("smooth is None, True, a dict or a track.OneEuro, not %r" % (cfg,))
    min_cutoff, beta, d_cutoff, fps = (_number(n, getattr(cfg, n)) for n in ("min_cutoff", "beta", "d_cutoff", "fps"))
    conf_floor = _number("conf_floor", cfg.conf_floor)
    if not (min_cutoff > 0.0 and math.isfinite(min_cutoff)):
        raise ValueError("min_cutoff = %r must be finite and positive (Hz)" % (cfg.min_cutoff,))
    if not (beta >= 0.0 and math.isfinite(beta)):
        raise ValueError("beta = %r must be finite and >= 0 (1/mm)" % (cfg.beta,))
    if not (d_cutoff > 0.0 and math.isfinite(d_cutoff)):
        raise ValueError("d_cutoff = %r must be finite and positive (Hz)" % (cfg.d_cutoff,))
    if not (fps > 0.0 and math.isfinite(fps)):
        raise ValueError("fps = %r must be finite and positive" % (cfg.fps,))
    gate_mm = cfg.gate_mm
    if gate_mm is not None:
        gate_mm = _number("gate_mm", gate_mm)
        if not gate_mm > 0.0:
            raise ValueError("gate_mm = %r must be positive (None: no gate)" % (cfg.gate_mm,))
    if isinstance(cfg.max_coast, bool) or not isinstance(cfg.max_coast, (int, np.integer)):
        raise TypeError("max_coast is an int >= 0, not %r" % (cfg.max_coast,))
    if not 0 <= int(cfg.max_coast) <= INT32_MAX:
        raise ValueError("max_coast = %r is outside [0, %d]" % (cfg.max_coast, INT32_MAX))
    if cfg.weight not in (None, "conf"):
        raise ValueError("weight is None or \"conf\", not %r" % (cfg.weight,))
    if not 0.0 < conf_floor <= 1.0:
        raise ValueError("conf_floor = %r is outside (0, 1]" % (cfg.conf_floor,))
    if not isinstance(cfg.lead, bool):
        raise TypeError("lead is True or False, not %r" % (cfg.lead,))
    return OneEuro(min_cutoff, beta, d_cutoff, fps, gate_mm, int(cfg.max_coast), cfg.weight, conf_floor, cfg.lead)


def check_dt(dt):
    dt = _number("dt", dt)
    if not (dt > 0.0 and math.isfinite(dt)):
        raise ValueError("dt = %r must be finite and positive (seconds)" % (dt,))
    return dt


def filter_state(B, J):
    """-> (state (B, J, 6) float64 `x0 x1 x2 d0 d1 d2`, count (B, J, 2) int32 `age coast`), zeroed: no track anywhere."""
    B, J = int(B), int(J)
    if not (1 <= B <= MAX_BATCH and 1 <= J <= MAX_JOINTS):
        raise ValueError("filter_state: B in [1, %d] and J in [1, %d] are required, got %d and %d" % (MAX_BATCH, MAX_JOINTS, B, J))
    return np.zeros((B, J, 6), np.float64), np.zeros((B, J, 2), np.int32)


def call_constants(cfg, dt):
    """-> (w, alpha_d, gate2) of one call, in the header's order, as numpy float64"""
    dt = np.float64(dt)
    w = (np.float64(2.0) * np.float64(math.pi)) * dt
    alpha_d = np.float64(1.0) / (np.float64(1.0) + np.float64(1.0) / (w * np.float64(cfg.d_cutoff)))
    gate2 = np.float64(np.inf) if cfg.gate_mm is None else np.float64(cfg.gate_mm) * np.float64(cfg.gate_mm)
    return w, alpha_d, gate2


def filter_step(state, count, xyz, status, ustatus, conf, cfg, dt=None, n_valid=None, paras=ND.PARAS, flip=-1):
    """The statement of awr_joints_filter (include/awr_hip.h): one step of the filter.  state (B, J, 6) float64 and count (B, J, 2) int32
    (filter_state) are updated IN PLACE; xyz (B, J, 3) float32 camera mm; status, ustatus (B,) the frame's codes; conf (B, J) float32, read
    only with cfg.weight == "conf" (may be None otherwise); dt seconds (default 1 / cfg.fps); rows >= n_valid keep their state and their
    output rows are unspecified (here: NaN and NONE).
    -> (xyz_f, uvd_f, ahead (B, J, 3) float32, code (B, J) int32).  An explicit loop in IEEE double, in the header's order."""
    cfg = check_filter(cfg)
    dt = check_dt(1.0 / cfg.fps if dt is None else dt)
    if not (isinstance(state, np.ndarray) and state.dtype == np.float64 and state.ndim == 3 and state.shape[2] == 6 and state.flags.c_contiguous):
        raise ValueError("state is a contiguous (B, J, 6) float64 array (filter_state)")
    B, J = state.shape[0], state.shape[1]
    if not (isinstance(count, np.ndarray) and count.dtype == np.int32 and count.shape == (B, J, 2) and count.flags.c_contiguous):
        raise ValueError("count is a contiguous (%d, %d, 2) int32 array (filter_state)" % (B, J))
    xyz = np.asarray(xyz, np.float32)
    if xyz.shape != (B, J, 3):
        raise ValueError("xyz is (%d, %d, 3), got %s" % (B, J, xyz.shape))
    status, ustatus = np.asarray(status).reshape(-1), np.asarray(ustatus).reshape(-1)
    nv = B if n_valid is None else int(n_valid)
    fx, fy, u0, v0 = (np.float64(p) for p in paras)
    if not (1 <= J <= MAX_JOINTS and 1 <= B <= MAX_BATCH and 0 <= nv <= B and status.shape[0] >= B and ustatus.shape[0] >= B
            and int(flip) in (1, -1) and fx != 0 and fy != 0):
        raise ValueError("filter_step: J in [1, %d], n_valid in [0, B], B status codes, flip = +-1 and non-zero focal lengths are required" % MAX_JOINTS)
    weighted = cfg.weight == "conf"
    if weighted:
        if conf is None:
            raise ValueError("weight=\"conf\" needs conf (B, J)")
        conf = np.asarray(conf, np.float32)
        if conf.shape != (B, J):
            raise ValueError("conf is (%d, %d), got %s" % (B, J, conf.shape))
    w, alpha_d, gate2 = call_constants(cfg, dt)
    dt, fl = np.float64(dt), np.float64(flip)
    min_cutoff, beta, conf_floor, max_coast = np.float64(cfg.min_cutoff), np.float64(cfg.beta), np.float64(cfg.conf_floor), int(cfg.max_coast)
    one, zero = np.float64(1.0), np.float64(0.0)
    xyz_f, uvd_f, ahead = (np.full((B, J, 3), np.nan, np.float32) for _ in range(3))
    code = np.zeros((B, J), np.int32)
    with np.errstate(all="ignore"):
        for b in range(nv):
            frame_ok = status[b] == 0 and ustatus[b] == 0
            for j in range(J):
                z = [np.float64(xyz[b, j, a]) for a in range(3)]
                ok = bool(frame_ok and np.isfinite(z[0]) and np.isfinite(z[1]) and np.isfinite(z[2]))
                x, d = [state[b, j, a] for a in range(3)], [state[b, j, 3 + a] for a in range(3)]
                age, coast = int(count[b, j, 0]), int(count[b, j, 1])
                if age == 0:
                    if not ok:
                        code[b, j] = NONE
                        continue                                  # NaN outputs, state untouched
                    x, d, age, coast, cd = list(z), [zero] * 3, 1, 0, INIT
                else:
                    accepted = False
                    if ok:
                        y = [z[a] - x[a] for a in range(3)]
                        g2 = (y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]
                        accepted = bool(g2 <= gate2)
                    if accepted:
                        wgt = one
                        if weighted:
                            c = np.float64(conf[b, j])
                            wgt = conf_floor
                            if c > conf_floor:
                                wgt = c
                            if c > one:
                                wgt = one
                        for a in range(3):
                            dx = y[a] / dt
                            d[a] = d[a] + alpha_d * (dx - d[a])
                            cut = min_cutoff + beta * np.fabs(d[a])
                            al = one / (one + one / (w * cut))
                            x[a] = x[a] + (al * wgt) * y[a]
                        age, coast, cd = min(age + 1, INT32_MAX), 0, UPDATED
                    else:
                        coast += 1
                        if coast > max_coast:
                            if ok:
                                x, d, age, coast, cd = list(z), [zero] * 3, 1, 0, REINIT
                            else:
                                x, d, age, coast, cd = [zero] * 3, [zero] * 3, 0, 0, LOST
                        else:
                            cd = GATED if ok else HELD
                state[b, j, 0:3], state[b, j, 3:6] = x, d
                count[b, j, 0], count[b, j, 1] = age, coast
                code[b, j] = cd
                if age > 0:
                    for a in range(3):
                        xyz_f[b, j, a] = np.float32(x[a])
                        ahead[b, j, a] = np.float32(x[a] + d[a] * dt)
                    uvd_f[b, j, 0] = np.float32(x[0] * fx / x[2] + u0)          # evaluator.xyz2uvd as detect.joints_center spells it
                    uvd_f[b, j, 1] = np.float32((x[1] * fl) * fy / x[2] + v0)
                    uvd_f[b, j, 2] = np.float32(x[2])
    return xyz_f, uvd_f, ahead, code


def filter_state_device(B, J, device="cuda"):
    """filter_state as device tensors"""
    import torch
    state, count = filter_state(B, J)
    return torch.from_numpy(state).to(device), torch.from_numpy(count).to(device)


def filter_step_device(state, count, xyz, status, ustatus, conf, cfg, dt=None, n_valid=None, paras=ND.PARAS, flip=-1, out=None):
    """awr_joints_filter on device tensors: state (B, J, 6) float64 and count (B, J, 2) int32 stay on the device and are updated in place;
    -> (xyz_f, uvd_f, ahead (B, J, 3) float32, code (B, J) int32) device tensors (`out`: these four, to write into); rows >= n_valid are
    left as they are.  Nothing synchronises.  There is no host fall-back: filter_step is the statement for a machine without a GPU."""
    import torch
    from . import _lib as L
    cfg = check_filter(cfg)
    dt = check_dt(1.0 / cfg.fps if dt is None else dt)
    if state.dtype != torch.float64 or state.dim() != 3 or state.shape[2] != 6:
        raise L.AwrError("state is a (B, J, 6) float64 device tensor")
    B, J = int(state.shape[0]), int(state.shape[1])
    if count.dtype != torch.int32 or tuple(count.shape) != (B, J, 2):
        raise L.AwrError("count is a (%d, %d, 2) int32 device tensor" % (B, J))
    if xyz.dtype != torch.float32 or tuple(xyz.shape) != (B, J, 3):
        raise L.AwrError("xyz is a (%d, %d, 3) float32 device tensor" % (B, J))
    if status.dtype != torch.int32 or ustatus.dtype != torch.int32 or status.numel() < B or ustatus.numel() < B:
        raise L.AwrError("status and ustatus hold B = %d int32 codes" % B)
    weighted = cfg.weight == "conf"
    if weighted and (conf is None or conf.dtype != torch.float32 or tuple(conf.shape) != (B, J)):
        raise L.AwrError("weight=\"conf\" needs conf, a (%d, %d) float32 device tensor" % (B, J))
    dev = state.device
    if out is None:
        out = tuple(torch.empty((B, J, 3), dtype=torch.float32, device=dev) for _ in range(3)) + (torch.empty((B, J), dtype=torch.int32, device=dev),)
    for t, shape, dtype in zip(out, ((B, J, 3),) * 3 + ((B, J),), (torch.float32,) * 3 + (torch.int32,)):
        if tuple(t.shape) != shape or t.dtype != dtype:
            raise L.AwrError("out is (xyz_f, uvd_f, ahead (B, J, 3) float32, code (B, J) int32)")
    L.call("awr_joints_filter", L.ptr(state), L.ptr(count), L.ptr(xyz), L.ptr(status), L.ptr(ustatus), L.ptr(conf) if weighted else None, B, J,
           B if n_valid is None else int(n_valid), dt, cfg.min_cutoff, cfg.beta, cfg.d_cutoff, -1.0 if cfg.gate_mm is None else cfg.gate_mm,
           cfg.max_coast, WEIGHTS[cfg.weight], cfg.conf_floor, float(paras[0]), float(paras[1]), float(paras[2]), float(paras[3]), int(flip),
           L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]), L.stream())
    return out
