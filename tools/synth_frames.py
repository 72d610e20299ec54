#!/usr/bin/env python
"""Write N synthetic hand frames and their labels to disk, so that predict.py has something to chew on.

    python tools/synth_frames.py N OUT [--seed S] [--jt-num 14] [--noise-mm 0] [--background-mm 0] [--no-forearm] [--edge] [--host]

writes OUT_frames.npy ((N, 480, 640) uint16 millimetres: `python predict.py OUT_frames.npy --load-model X.pth`) and OUT_labels.npz
(labels_xyz (N, J, 3), centers (N, 3), joints21 (N, 21, 3) camera millimetres; prims, bbox: the capsule tables the frames were rendered
from; status).  The frames are rendered on the GPU (awr_synth_render); --host renders them with the numpy statement instead.
These are procedural hands (awr_amd/synth.py): they say nothing about NYU."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", type=int)
    ap.add_argument("out")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--jt-num", type=int, default=14, choices=(14, 21))
    ap.add_argument("--noise-mm", type=int, default=0)
    ap.add_argument("--background-mm", type=int, default=0)
    ap.add_argument("--no-forearm", action="store_true")
    ap.add_argument("--edge", action="store_true", help="also draw hands that the frame border cuts")
    ap.add_argument("--host", action="store_true", help="render with the numpy statement (small N, no GPU)")
    a = ap.parse_args(argv)
    import awr_amd  # noqa: F401
    from awr_amd import synth
    sf = synth.SyntheticFrames(a.n, a.seed, "test", jt_num=a.jt_num, device=None if a.host else "cuda", forearm=not a.no_forearm,
                               noise_mm=a.noise_mm, background_mm=a.background_mm, edge=a.edge)
    empty = sf.check()
    status = np.asarray(sf.status.cpu() if hasattr(sf.status, "cpu") else sf.status)
    np.save(a.out + "_frames.npy", sf.frames_host())
    np.savez_compressed(a.out + "_labels.npz", labels_xyz=sf.labels_xyz, centers=sf.centers, joints21=sf.joints21, prims=sf.prims, bbox=sf.bbox,
                        status=status, paras=np.asarray(sf.paras), flip=np.int32(sf.flip))
    print("%d frames -> %s_frames.npy, labels -> %s_labels.npz (%d empty)" % (a.n, a.out, a.out, empty))


if __name__ == "__main__":
    main()
