#!/usr/bin/env python
"""Regenerate tests/golden/synth_hand_48x64.npz: primitive TABLES (not poses: no libm sine takes part when the file is replayed), their
boxes, the camera, and the frames awr_amd.synth.render makes of them -- plain, one parameter set with noise and one with a wall.

    python tools/make_synth_golden.py [--check]

--check renders the stored tables again and compares, without writing.  A regenerated file must keep passing the half-integer guard of
tests/test_synth_cpu.py (pick another --seed if a pixel lands within 1e-6 mm of k + 0.5)."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "synth_hand_48x64.npz")
PARAMS = {"plain": (0, 0, 0, 0), "noise": (0, 3, 17, 5), "wall": (1000, 2, 4, 0)}      # background_mm, noise_mm, seed, frame0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    from awr_amd import nyu_data as ND
    from awr_amd import synth
    if a.check:
        g = np.load(OUT)
        prims, bbox, paras, flip, shape = g["prims"], g["bbox"], tuple(g["paras"]), int(g["flip"]), tuple(int(s) for s in g["frame_shape"])
    else:
        shape, paras, flip = (48, 64), tuple(0.1 * p for p in ND.PARAS), -1
        model = synth.HandModel()
        poses = synth.sample_poses(3, a.seed, model, frame_shape=shape, paras=paras, flip=flip)
        _, prims, bbox = synth.forward_kinematics(poses, model, shape, paras, flip)
    frames = {}
    for tag, (bg, noise, seed, frame0) in PARAMS.items():
        frames[tag] = synth.render(prims, bbox, shape, paras, flip, bg, noise, seed, frame0)
    if a.check:
        for tag in PARAMS:
            assert np.array_equal(frames[tag], g["frames_" + tag]) and tuple(g["params_" + tag]) == PARAMS[tag], tag
        print("golden ok")
        return
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, prims=prims, bbox=bbox, paras=np.asarray(paras, np.float64), flip=np.int32(flip), frame_shape=np.asarray(shape, np.int32),
                        **{"frames_" + t: f for t, f in frames.items()}, **{"params_" + t: np.asarray(p, np.int64) for t, p in PARAMS.items()})
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
