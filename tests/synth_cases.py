"""Inputs shared by tests/test_synth_cpu.py and tests/test_synth_gpu.py: primitive tables, boxes and renderer parameters.

The GPU tests demand np.array_equal against the numpy statement although the device's float64 square root is only specified to 1 ulp;
that is sound because the CPU file checks, on exactly these inputs (and on the golden table), that no pixel's unrounded depth lies within
1e-6 mm of a half-integer -- a 1 ulp difference (about 1e-13 mm) cannot change a rounded value then.  So every input either file renders
comes from here.  Shapes are the smallest that still exercise the kernel: several 64 x 16 pixel tiles per frame, frames whose box covers a
part of a tile, a width that is no multiple of the four pixels a thread packs, and one pair of full 480 x 640 frames."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synth_hand_48x64.npz")
SMALL = (48, 64)
FULL = (480, 640)


def small_paras():
    from awr_amd import nyu_data as ND
    return tuple(0.1 * p for p in ND.PARAS)


def _tables(n, seed, frame_shape, paras, flip, edge=False, forearm=True):
    from awr_amd import synth
    model = synth.HandModel(forearm=forearm)
    poses = synth.sample_poses(n, seed, model, edge=edge, frame_shape=frame_shape, paras=paras, flip=flip)
    joints, prims, bbox = synth.forward_kinematics(poses, model, frame_shape, paras, flip)
    return joints, prims, bbox, model


def pad_rows(prims, K):
    """(n, k, 8) -> (n, K, 8) with unused rows (r = 0, r = -1 and a row whose only oddity is r = -2 beside huge coordinates) INTERLEAVED
    between the used ones, not appended"""
    n, k, _ = prims.shape
    out = np.zeros((n, K, 8))
    slots = np.sort(np.random.RandomState(K).permutation(K)[:k])
    out[:, slots] = prims
    for j, s in enumerate(sorted(set(range(K)) - set(slots.tolist()))):
        out[:, s, 6] = (0.0, -1.0, -2.0)[j % 3]
        if j % 3 == 2:
            out[:, s, :6] = 1e30
    return out


def shift(prims, d):
    out = prims.copy()
    used = ~(out[..., 6] <= 0)
    out[..., 0:3] += np.asarray(d, np.float64) * used[..., None]
    out[..., 3:6] += np.asarray(d, np.float64) * used[..., None]
    return out


def case(name, prims, frame_shape, paras, flip, bbox=None, background_mm=0, noise_mm=0, seed=0, frame0=0):
    from awr_amd import synth
    prims = np.ascontiguousarray(prims, dtype=np.float64)
    if bbox is None:
        bbox = synth.prim_boxes(prims, frame_shape, paras, flip)
    return dict(name=name, prims=prims, bbox=np.ascontiguousarray(bbox, dtype=np.int32), frame_shape=tuple(frame_shape), paras=tuple(paras), flip=flip,
                background_mm=background_mm, noise_mm=noise_mm, seed=seed, frame0=frame0)


def render_kw(c):
    return {k: c[k] for k in ("frame_shape", "paras", "flip", "background_mm", "noise_mm", "seed", "frame0")}


def device_kw(c):
    return {k: c[k] for k in ("paras", "flip", "background_mm", "noise_mm", "seed", "frame0")}


# frame order of the "special" cases
SPECIAL = ("cut_left", "cut_right", "cut_top", "cut_bottom", "outside", "nan_row", "neighbour", "crosses_z0", "thin_far")


def special_tables(paras, flip):
    """(9, 22, 8): one hand cut by each frame border, one wholly outside the frame (EMPTY), one with a NaN in a used row (BAD_PRIM) followed
    by an ordinary neighbour, a capsule that crosses z = 0 and a far capsule thinner than a pixel."""
    joints, prims, _, _ = _tables(1, 41, SMALL, paras, flip)
    fx, fy = paras[0], paras[1]
    hand = prims[0]
    c = joints[0].mean(0)
    z = c[2]
    to_u = lambda u: (u - paras[2]) * z / fx - c[0]                 # shift in x that puts the hand's middle at column u
    to_v = lambda v: flip * (v - paras[3]) * z / fy - c[1]
    frames = [shift(hand, (to_u(0.0), 0, 0)), shift(hand, (to_u(SMALL[1] - 1.0), 0, 0)), shift(hand, (0, to_v(0.0), 0)),
              shift(hand, (0, to_v(SMALL[0] - 1.0), 0)), shift(hand, (to_u(-400.0), 0, 0))]
    bad = hand.copy()
    bad[3, 4] = np.nan
    frames += [bad, hand.copy()]
    cross = np.zeros((22, 8))
    cross[5] = (150.0, 20.0, -100.0, 150.0, -30.0, 300.0, 20.0, 0.0)
    cross[9] = (-40.0, 0.0, 0.0, -40.0, 0.0, 0.0, -1.0, 0.0)        # an unused row
    thin = np.zeros((22, 8))
    thin[0] = (-2500.0, 310.0, 5000.0, 2400.0, -290.0, 5100.0, 30.0, 0.0)      # 0.7 pixels across at this depth
    frames += [cross, thin]
    return np.stack(frames)


@functools.lru_cache(maxsize=None)
def cases():
    sp = small_paras()
    from awr_amd import nyu_data as ND
    out = []
    _, p, b, _ = _tables(3, 11, SMALL, sp, -1)
    out.append(case("small_n3_K22", p, SMALL, sp, -1, b))
    _, p, _, _ = _tables(17, 12, SMALL, sp, 1, edge=True)
    out.append(case("small_n17_K32_flip_wall_noise", pad_rows(p, 32), SMALL, sp, 1, background_mm=1100, noise_mm=3, seed=5, frame0=7))
    out.append(case("small_n1_K1_sphere", np.array([[[30.0, -20.0, 600.0, 30.0, -20.0, 600.0, 45.0, 0.0]]]), SMALL, sp, -1))
    out.append(case("small_n1_K1_capsule_noise", np.array([[[-60.0, -50.0, 650.0, 70.0, 40.0, 520.0, 25.0, 0.0]]]), SMALL, sp, 1, noise_mm=3, seed=9))
    out.append(case("special", special_tables(sp, -1), SMALL, sp, -1))
    out.append(case("special_flip_wall_noise", special_tables(sp, 1), SMALL, sp, 1, background_mm=900, noise_mm=3, seed=3, frame0=100))
    _, p, _, _ = _tables(3, 13, (48, 62), sp, -1, edge=True)
    out.append(case("width62_n3_noise", p, (48, 62), sp, -1, noise_mm=3, seed=2))
    _, p, b, _ = _tables(2, 18, FULL, ND.PARAS, -1)
    out.append(case("full_n2_K22_noise", p, FULL, ND.PARAS, -1, b, noise_mm=3, seed=1, frame0=3))
    _, p, _, _ = _tables(2, 15, FULL, ND.PARAS, 1, forearm=False)
    out.append(case("full_n2_K32_flip_wall", pad_rows(p, 32), FULL, ND.PARAS, 1, background_mm=1500))
    return {c["name"]: c for c in out}


def golden_cases():
    """the golden file's tables with its three parameter sets (plain, one noisy, one with a wall) -> [(case, expected frames)]"""
    g = np.load(GOLDEN)
    paras, flip, shape = tuple(float(p) for p in g["paras"]), int(g["flip"]), tuple(int(s) for s in g["frame_shape"])
    out = []
    for tag in ("plain", "noise", "wall"):
        bg, a, seed, frame0 = (int(v) for v in g["params_" + tag])
        out.append((case("golden_" + tag, g["prims"], shape, paras, flip, g["bbox"], bg, a, seed, frame0), g["frames_" + tag]))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the statement's frames, unrounded depths and status of a case: computed once per process, never modified"""
    from awr_amd import synth
    c = cases()[name]
    frames, raw, status = synth.render(c["prims"], c["bbox"], return_unrounded=True, return_status=True, **render_kw(c))
    for a in (frames, raw, status):
        a.setflags(write=False)
    return frames, raw, status
