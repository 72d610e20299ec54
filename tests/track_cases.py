"""Inputs shared by tests/test_track_cpu.py and tests/test_track_gpu.py: bit comparison, a chained scenario generator for the temporal joint
filter (awr_amd/track.py) and the statement run over a chain.

The scenario is a camera-space joint set around z = 600 mm (never near z = 0: the uvd projection divides by the filtered depth) moving
smoothly with a little noise, with every kind of event the filter has an answer for mixed in at times drawn per slot and joint."""
import numpy as np

E_PARAS = (147.0, 146.8, 80.0, 60.0)                # NYU's intrinsics scaled to a 160 x 120 frame (tests/test_recenter_gpu.py)
FLIP = -1


def bits(a):
    """the 64- or 32-bit patterns of a tensor or array: NaN payloads and signed zeros count"""
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a).view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def scenario(B, J, T=48, seed=0, max_coast=5):
    """-> a list of T steps (xyz (B, J, 3) float32, status (B,) int32, ustatus (B,) int32, conf (B, J) float32), from RandomState(seed).
    Per slot and joint: smooth motion (a sine of 40 mm per axis over about a second) plus N(0, 2 mm) noise; ONE frame 200 mm off at a
    step in [4, 6]; a PERMANENT 150 mm jump from a step in [12, 14]; a NaN, a +Inf and a -Inf coordinate at steps in [22, 26].  Per slot:
    a run of 2 bad frames from step 8 (status on even slots, ustatus on odd ones: shorter than max_coast) and a run of max_coast + 2 bad
    frames from step 30 + slot % 3 (longer: the track is lost, and starts again when the frames return).  conf is uniform in [0.3, 1)
    with a tenth of the entries each below the floor (0.1), negative, above one (1.5) and NaN.  With more than one (slot, joint), joint
    J - 1 of the last slot is never valid."""
    rs = np.random.RandomState(seed)
    p0 = np.stack([rs.uniform(-100, 100, (B, J)), rs.uniform(-100, 100, (B, J)), rs.uniform(550, 700, (B, J))], -1)
    amp, phase, period = rs.uniform(10, 40, (B, J, 3)), rs.uniform(0, 2 * np.pi, (B, J, 3)), rs.uniform(25, 40, (B, J, 3))
    t_out, t_jump, t_nan = rs.randint(4, 7, (B, J)), rs.randint(12, 15, (B, J)), rs.randint(22, 25, (B, J))
    axis = rs.randint(0, 3, (B, J, 3))
    sign = rs.choice([-1.0, 1.0], (B, J, 2))
    long_run = max_coast + 2
    steps = []
    for t in range(T):
        xyz = p0 + amp * np.sin(2 * np.pi * t / period + phase) + rs.normal(0.0, 2.0, (B, J, 3))
        status, ustatus = np.zeros(B, np.int32), np.zeros(B, np.int32)
        conf = rs.uniform(0.3, 1.0, (B, J))
        kind = rs.randint(0, 10, (B, J))
        conf[kind == 0], conf[kind == 1], conf[kind == 2], conf[kind == 3] = 0.1, -0.5, 1.5, np.nan
        for b in range(B):
            if 8 <= t < 10:
                (status if b % 2 == 0 else ustatus)[b] = 1 + b % 3
            if 30 + b % 3 <= t < 30 + b % 3 + long_run:
                status[b] = 1
            for j in range(J):
                if t == t_out[b, j]:
                    xyz[b, j, axis[b, j, 0]] += 200.0 * sign[b, j, 0]
                if t >= t_jump[b, j]:
                    xyz[b, j, axis[b, j, 1]] += 150.0 * sign[b, j, 1]
                if t == t_nan[b, j]:
                    xyz[b, j, axis[b, j, 2]] = np.nan
                elif t == t_nan[b, j] + 1:
                    xyz[b, j, axis[b, j, 2]] = np.inf
                elif t == t_nan[b, j] + 2:
                    xyz[b, j, (axis[b, j, 2] + 1) % 3] = -np.inf
        if B * J > 1:
            xyz[B - 1, J - 1, t % 3] = (np.nan, np.inf, -np.inf)[t % 3]
        steps.append((xyz.astype(np.float32), status, ustatus, conf.astype(np.float32)))
    return steps


def run_chain(T, cfg, steps, dt=None, n_valid=None, state=None, count=None, paras=E_PARAS, flip=FLIP):
    """the statement over a chain: -> a list of (xyz_f, uvd_f, ahead, code, state copy, count copy), one entry per step"""
    B, J = steps[0][0].shape[:2]
    if state is None:
        state, count = T.filter_state(B, J)
    out = []
    for xyz, status, ustatus, conf in steps:
        r = T.filter_step(state, count, xyz, status, ustatus, conf, cfg, dt, n_valid, paras, flip)
        out.append(r + (state.copy(), count.copy()))
    return out


def single_joint_steps(points, bad=()):
    """(T, 3) positions of one joint -> steps for B = J = 1; `bad`: the steps whose frame has status 1"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    return [(points[t].astype(np.float32).reshape(1, 1, 3), np.array([1 if t in bad else 0], np.int32), np.zeros(1, np.int32),
             np.ones((1, 1), np.float32)) for t in range(len(points))]
