"""Temporal joint filter: the numpy statement of awr_joints_filter (csrc/awr_track.hip; include/awr_hip.h "Temporal joint filter";
DESIGN.md 4.25) and its thin device wrapper; further down, hand identities across calls: the numpy statement of awr_hands_assign
(csrc/awr_assign.hip; include/awr_hip.h "Hand identities across calls"), `assign_step`, and its wrapper.

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
    from . import _lib as L, detect_calls as DC
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
    DC.awr_joints_filter(L.ptr(state), L.ptr(count), L.ptr(xyz), L.ptr(status), L.ptr(ustatus), L.ptr(conf) if weighted else None, B, J,
                         B if n_valid is None else n_valid, dt, cfg, paras, flip, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]))
    return out


# ---- hand identities across calls (include/awr_hip.h awr_hands_assign; csrc/awr_assign.hip) --------------------------------
# Predictor(hands=K) reports "the k-th nearest component of this frame" in slot k.  assign_step decides which of this call's detected hands
# is which identity of the previous call: an exact assignment over all K! permutations (K <= 4: at most 24), largest number of pairs inside
# the gate first, smallest summed squared distance second, first permutation third.  Positions are compared in camera millimetres; the
# arithmetic is IEEE double + - * / and comparisons only, no square root: squared distances against gate_mm^2 and merge_mm^2.
# awr_hands_assign's codes (include/awr_hip.h AWR_ASSIGN_*)
FREE, BORN, MATCHED, TRACKED, COASTING, ID_LOST, MERGED = 0, 1, 2, 3, 4, 5, 6
ASSIGN_NAMES = {FREE: "no identity in this slot", BORN: "a new identity started at a candidate", MATCHED: "the identity took a candidate inside the gate",
                TRACKED: "the identity's tracked centre found the hand", COASTING: "no candidate inside the gate: the identity waits",
                ID_LOST: "waited too long: the identity was released", MERGED: "two tracked centres on one hand: the younger identity was released"}
SOURCE_NONE, SOURCE_TRACKED = -1, -2
MAX_HANDS = 4
_OK, _EMPTY = 0, 1                      # awr_amd.detect's status codes (AWR_DET_OK, AWR_DET_EMPTY)

# gate_mm: the furthest a hand's centre may move between two calls and keep its identity; merge_mm: two TRACKED centres closer than this are
# one hand; max_miss: calls an identity waits without a candidate before it is released.  ENGINEERING CHOICES -- half a crop cube, a palm's
# width, a sixth of a second at 30 fps -- and unmeasured on real frames: none are available where this was written.
_Identity = collections.namedtuple("Identity", "gate_mm merge_mm max_miss")


class Identity(_Identity):
    """The identity assignment's configuration, an immutable record.  gate_mm (> 0): a candidate further than this from an identity's last
    centre (camera mm) is not that identity; merge_mm (>= 0): two tracked centres within this distance are one hand and the younger identity
    is released; max_miss (int >= 0): calls an identity survives without a candidate.  The defaults are unmeasured engineering choices."""
    __slots__ = ()

    def __new__(cls, gate_mm=150.0, merge_mm=60.0, max_miss=5):
        return super().__new__(cls, gate_mm, merge_mm, max_miss)


def check_identity(cfg):
    """True (the defaults) | a dict of Identity's fields | an Identity -> a validated Identity with plain Python values (the rules are
    awr_hands_assign's argument rules)."""
    if cfg is True:
        cfg = Identity()
    elif isinstance(cfg, dict):
        unknown = sorted(set(cfg) - set(Identity._fields))
        if unknown:
            raise ValueError("unknown identity option(s) %s: the options are %s" % (unknown, list(Identity._fields)))
        cfg = Identity(**cfg)
    elif not isinstance(cfg, Identity):
        raise TypeError("identity is None, True, a dict or a track.Identity, not %r" % (cfg,))
    gate_mm, merge_mm = _number("gate_mm", cfg.gate_mm), _number("merge_mm", cfg.merge_mm)
    if not (gate_mm > 0.0 and math.isfinite(gate_mm)):
        raise ValueError("gate_mm = %r must be finite and positive (mm)" % (cfg.gate_mm,))
    if not (merge_mm >= 0.0 and math.isfinite(merge_mm)):
        raise ValueError("merge_mm = %r must be finite and >= 0 (mm)" % (cfg.merge_mm,))
    if isinstance(cfg.max_miss, bool) or not isinstance(cfg.max_miss, (int, np.integer)):
        raise TypeError("max_miss is an int >= 0, not %r" % (cfg.max_miss,))
    if not 0 <= int(cfg.max_miss) <= INT32_MAX - 1:
        raise ValueError("max_miss = %r is outside [0, %d]" % (cfg.max_miss, INT32_MAX - 1))
    return Identity(gate_mm, merge_mm, int(cfg.max_miss))


def identity_state(K, B):
    """-> (last_uvd (K, B, 3) float64 NaN, ids (K, B) int32 0, miss (K, B) int32 0, next_id (B,) int32 1): no identity anywhere.  Hand-major,
    like every buffer of Predictor(hands=K); an identity is a positive int, unique within its batch slot and never used again."""
    K, B = int(K), int(B)
    if not (1 <= K <= MAX_HANDS and 1 <= B <= MAX_BATCH):
        raise ValueError("identity_state: K in [1, %d] and B in [1, %d] are required, got %d and %d" % (MAX_HANDS, MAX_BATCH, K, B))
    return np.full((K, B, 3), np.nan, np.float64), np.zeros((K, B), np.int32), np.zeros((K, B), np.int32), np.ones(B, np.int32)


def permutation(p, K):
    """the p-th permutation of range(K) in lexicographic order, decoded in the factorial number system (as the kernel's lanes do)"""
    left, out = list(range(K)), []
    for i in range(K):
        f = math.factorial(K - 1 - i)
        out.append(left.pop(p // f))
        p %= f
    return out


def _finite3(row):
    return bool(np.isfinite(row[0]) and np.isfinite(row[1]) and np.isfinite(row[2]))


def _state_arrays(last_uvd, ids, miss, next_id):
    if not (isinstance(last_uvd, np.ndarray) and last_uvd.dtype == np.float64 and last_uvd.ndim == 3 and last_uvd.shape[2] == 3 and last_uvd.flags.c_contiguous):
        raise ValueError("last_uvd is a contiguous (K, B, 3) float64 array (identity_state)")
    K, B = last_uvd.shape[0], last_uvd.shape[1]
    for a, name, shape in ((ids, "ids", (K, B)), (miss, "miss", (K, B)), (next_id, "next_id", (B,))):
        if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.shape == shape and a.flags.c_contiguous):
            raise ValueError("%s is a contiguous %s int32 array (identity_state)" % (name, shape))
    return K, B


def assign_step(last_uvd, ids, miss, next_id, cand_uvd, cand_status, trk_uvd=None, trk_status=None, cfg=True, n_valid=None, paras=ND.PARAS, flip=-1,
                filter_state=None, filter_count=None):
    """The statement of awr_hands_assign (include/awr_hip.h): one step of the identity assignment.  last_uvd (K, B, 3) float64, ids, miss
    (K, B) int32 and next_id (B,) int32 (identity_state) are updated IN PLACE.  cand_uvd (K, B, 3) float64 / cand_status (K, B): this call's
    detected hands, awr_detect's outputs over awr_detect_hands' seeds; trk_uvd / trk_status: awr_detect's outputs over last_uvd as given
    seeds, or None without a tracker.  filter_state ((K * B, J, 6) float64) / filter_count ((K * B, J, 2) int32): the temporal filter's state,
    whose rows of every slot that starts or loses an identity are zeroed in place; None without one.  Rows >= n_valid keep their state.
    -> (centers (K, B, 3) float64, status (K, B) int32, code (K, B) int32, reset (K, B) int32, source (K, B) int32, dropped (B,) int32).
    An explicit loop in IEEE double, in the header's order."""
    cfg = check_identity(cfg)
    K, B = _state_arrays(last_uvd, ids, miss, next_id)
    cand_uvd, cand_status = np.asarray(cand_uvd, np.float64), np.asarray(cand_status)
    if cand_uvd.shape != (K, B, 3) or cand_status.shape != (K, B):
        raise ValueError("cand_uvd is (%d, %d, 3) and cand_status (%d, %d), got %s and %s" % (K, B, K, B, cand_uvd.shape, cand_status.shape))
    tracked = trk_uvd is not None
    if tracked:
        trk_uvd, trk_status = np.asarray(trk_uvd, np.float64), np.asarray(trk_status)
        if trk_uvd.shape != (K, B, 3) or trk_status.shape != (K, B):
            raise ValueError("trk_uvd is (%d, %d, 3) and trk_status (%d, %d), got %s and %s" % (K, B, K, B, trk_uvd.shape, trk_status.shape))
    nv = B if n_valid is None else int(n_valid)
    fx, fy, u0, v0 = (np.float64(p) for p in paras)
    if not (1 <= K <= MAX_HANDS and 1 <= B <= MAX_BATCH and 0 <= nv <= B and int(flip) in (1, -1) and fx != 0 and fy != 0):
        raise ValueError("assign_step: K in [1, %d], n_valid in [0, B], flip = +-1 and non-zero focal lengths are required" % MAX_HANDS)
    if (filter_state is None) != (filter_count is None):
        raise ValueError("filter_state and filter_count come together")
    if filter_state is not None:
        J = filter_state.shape[1] if filter_state.ndim == 3 else 0
        if not (filter_state.dtype == np.float64 and filter_state.shape == (K * B, J, 6) and filter_count.dtype == np.int32
                and filter_count.shape == (K * B, J, 2) and 1 <= J <= MAX_JOINTS):
            raise ValueError("filter_state is (K * B, J, 6) float64 and filter_count (K * B, J, 2) int32")
    fl = np.float64(flip)
    gate2, merge2, max_miss = np.float64(cfg.gate_mm) * np.float64(cfg.gate_mm), np.float64(cfg.merge_mm) * np.float64(cfg.merge_mm), int(cfg.max_miss)
    nan = np.float64(np.nan)

    def xyz(c):                                                   # evaluator.uvd2xyz in its operation order, kept in double
        return ((c[0] - u0) * c[2] / fx, (c[1] - v0) * c[2] / fy * fl, c[2])

    def dist2(a, b):
        d = [a[0] - b[0], a[1] - b[1], a[2] - b[2]]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]

    centers = np.full((K, B, 3), np.nan, np.float64)
    status = np.full((K, B), _EMPTY, np.int32)
    code, reset, dropped = np.zeros((K, B), np.int32), np.zeros((K, B), np.int32), np.zeros(B, np.int32)
    source = np.full((K, B), SOURCE_NONE, np.int32)
    with np.errstate(all="ignore"):
        for b in range(nv):
            ident = [int(ids[i, b]) for i in range(K)]
            ms = [int(miss[i, b]) for i in range(K)]
            cd, released = [FREE] * K, [False] * K
            # 1. held slots; two tracked centres on one hand: the younger identity goes
            held = [bool(tracked and ident[i] > 0 and trk_status[i, b] == _OK and _finite3(trk_uvd[i, b])) for i in range(K)]
            r = [xyz(trk_uvd[i, b]) if held[i] else xyz(last_uvd[i, b]) for i in range(K)]
            for i in range(K):
                for j in range(i + 1, K):
                    if held[i] and held[j] and dist2(r[i], r[j]) <= merge2:
                        g = j if ident[j] > ident[i] else i
                        held[g], ident[g], ms[g], cd[g], released[g] = False, 0, 0, MERGED, True
            # 2. usable candidates, admissible pairs
            usable = [bool(cand_status[j, b] == _OK and _finite3(cand_uvd[j, b])) for j in range(K)]
            q = [xyz(cand_uvd[j, b]) for j in range(K)]
            c = [[dist2(r[i], q[j]) for j in range(K)] for i in range(K)]
            adm = [[bool(ident[i] > 0 and usable[j] and c[i][j] <= gate2) for j in range(K)] for i in range(K)]
            # 3. the permutation: most pairs, then the smallest sum, then the first
            best = None
            for p in range(math.factorial(K)):
                perm = permutation(p, K)
                m, s = 0, np.float64(0.0)
                for i in range(K):
                    if adm[i][perm[i]]:
                        m, s = m + 1, s + c[i][perm[i]]
                if best is None or m > best[0] or (m == best[0] and s < best[1]):
                    best = (m, s, perm)
            perm = best[2]
            # 4. every live slot
            consumed = [False] * K
            out = [None] * K                                      # the candidate index, SOURCE_TRACKED, or None
            for i in range(K):
                if ident[i] <= 0:
                    continue
                j = perm[i] if adm[i][perm[i]] else -1
                if held[i]:
                    out[i], ms[i], cd[i] = SOURCE_TRACKED, 0, TRACKED
                    if j >= 0:
                        consumed[j] = True                        # the same hand, seen twice
                elif j >= 0:
                    out[i], ms[i], cd[i], consumed[j] = j, 0, MATCHED, True
                else:
                    ms[i] += 1
                    if ms[i] <= max_miss:
                        cd[i] = COASTING
                    else:
                        ident[i], ms[i], cd[i], released[i] = 0, 0, ID_LOST, True
            # 5. births: the lowest free slot, else the slot that has coasted longest
            nid = int(next_id[b])
            for j in range(K):
                if not usable[j] or consumed[j]:
                    continue
                slot = -1
                for i in range(K):
                    if ident[i] == 0:
                        slot = i
                        break
                if slot < 0:
                    for i in range(K):
                        if cd[i] == COASTING and (slot < 0 or ms[i] > ms[slot]):
                            slot = i
                if slot < 0:
                    dropped[b] += 1
                    continue
                ident[slot], ms[slot], cd[slot], out[slot], reset[slot, b] = nid, 0, BORN, j, 1
                nid = min(nid + 1, INT32_MAX)
            next_id[b] = nid
            # 6. outputs and state
            for i in range(K):
                if out[i] is not None:
                    centers[i, b] = trk_uvd[i, b] if out[i] == SOURCE_TRACKED else cand_uvd[out[i], b]
                    status[i, b], source[i, b] = _OK, out[i]
                    last_uvd[i, b] = centers[i, b]
                elif ident[i] == 0:
                    last_uvd[i, b] = nan
                ids[i, b], miss[i, b], code[i, b] = ident[i], ms[i], cd[i]
                if filter_state is not None and (reset[i, b] or released[i]):
                    filter_state[i * B + b], filter_count[i * B + b] = 0.0, 0
    return centers, status, code, reset, source, dropped


def identity_state_device(K, B, device="cuda"):
    """identity_state as device tensors"""
    import torch
    return tuple(torch.from_numpy(a).to(device) for a in identity_state(K, B))


def assign_step_device(last_uvd, ids, miss, next_id, cand_uvd, cand_status, trk_uvd=None, trk_status=None, cfg=True, n_valid=None, paras=ND.PARAS,
                       flip=-1, filter_state=None, filter_count=None, out=None):
    """awr_hands_assign on device tensors: the state (identity_state_device) stays on the device and is updated in place, as are the rows of
    filter_state / filter_count that start or lose an identity; -> (centers (K, B, 3) float64, status, code, reset, source (K, B) int32,
    dropped (B,) int32) device tensors (`out`: these six, to write into).  Nothing synchronises.  There is no host fall-back: assign_step is
    the statement for a machine without a GPU."""
    import torch
    from . import _lib as L, detect_calls as DC
    cfg = check_identity(cfg)
    if last_uvd.dtype != torch.float64 or last_uvd.dim() != 3 or last_uvd.shape[2] != 3:
        raise L.AwrError("last_uvd is a (K, B, 3) float64 device tensor")
    K, B = int(last_uvd.shape[0]), int(last_uvd.shape[1])
    for t, name, shape in ((ids, "ids", (K, B)), (miss, "miss", (K, B)), (next_id, "next_id", (B,)), (cand_status, "cand_status", (K, B))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape:
            raise L.AwrError("%s is a %s int32 device tensor" % (name, shape))
    if cand_uvd.dtype != torch.float64 or tuple(cand_uvd.shape) != (K, B, 3):
        raise L.AwrError("cand_uvd is a (%d, %d, 3) float64 device tensor" % (K, B))
    if (trk_uvd is None) != (trk_status is None):
        raise L.AwrError("trk_uvd and trk_status come together")
    if trk_uvd is not None and (trk_uvd.dtype != torch.float64 or tuple(trk_uvd.shape) != (K, B, 3) or trk_status.dtype != torch.int32
                                or tuple(trk_status.shape) != (K, B)):
        raise L.AwrError("trk_uvd is a (%d, %d, 3) float64 and trk_status a (%d, %d) int32 device tensor" % (K, B, K, B))
    J = 0
    if (filter_state is None) != (filter_count is None):
        raise L.AwrError("filter_state and filter_count come together")
    if filter_state is not None:
        J = int(filter_state.shape[1]) if filter_state.dim() == 3 else 0
        if (filter_state.dtype != torch.float64 or tuple(filter_state.shape) != (K * B, J, 6) or filter_count.dtype != torch.int32
                or tuple(filter_count.shape) != (K * B, J, 2)):
            raise L.AwrError("filter_state is a (K * B, J, 6) float64 and filter_count a (K * B, J, 2) int32 device tensor")
    dev = last_uvd.device
    if out is None:
        out = ((torch.empty((K, B, 3), dtype=torch.float64, device=dev),) + tuple(torch.empty((K, B), dtype=torch.int32, device=dev) for _ in range(4))
               + (torch.empty(B, dtype=torch.int32, device=dev),))
    for t, shape, dtype in zip(out, ((K, B, 3),) + ((K, B),) * 4 + ((B,),), (torch.float64,) + (torch.int32,) * 5):
        if tuple(t.shape) != shape or t.dtype != dtype:
            raise L.AwrError("out is (centers (K, B, 3) float64, status, code, reset, source (K, B) int32, dropped (B,) int32)")
    DC.awr_hands_assign(L.ptr(last_uvd), L.ptr(ids), L.ptr(miss), L.ptr(next_id), L.ptr(cand_uvd), L.ptr(cand_status), L.ptr(trk_uvd),
                        L.ptr(trk_status), K, B, B if n_valid is None else n_valid, cfg, paras, flip, L.ptr(filter_state), L.ptr(filter_count), J,
                        L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]), L.ptr(out[4]), L.ptr(out[5]))
    return out
