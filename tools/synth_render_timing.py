"""What rendering synthetic hand frames costs on one MI355X -> profiles/synth_render.txt

    python tools/synth_render_timing.py [--frames 256] [--reps 20] [--runs 5] [--host-frames 2] [--parent HASH] [--out profiles/synth_render.txt]

  (a) awr_synth_render, milliseconds per 480 x 640 frame, for K = 22 (the hand model's table) and K = 32 (the same table with ten of its
      capsules repeated: 32 used rows), in two cases: hands at their usual distance, rendered inside their boxes, and a hand that fills the
      frame (z about 280 mm, the box is the whole frame).  `frames` frames per call, `reps` back-to-back calls between two HIP events, the
      four cases alternating over `runs` repeats after a warm-up: median and min - max.  The tables and boxes are on the device before the
      clock starts: this is the kernel pair (status + render), not the upload.
  (b) the bytes the kernel writes (frames * 480 * 640 * 2) per second against the HBM write rate plain stores reach on this chip
      (about 6 TB/s; 8 TB/s is the specified peak).
  (c) the numpy statement on this host over `host-frames` of the same frames, and the ratio.
  (d) the parent commit hash.
There is no fall-back: without a GPU the tool fails.  Nothing in the tests depends on these numbers."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import awr_amd  # noqa: E402,F401
from awr_amd import synth  # noqa: E402

FH, FW = 480, 640
HBM_STORE_TBS, HBM_PEAK_TBS = 6.0, 8.0


def tables(n, fill, K):
    model = synth.HandModel()
    kw = dict(z_range=(270.0, 290.0), scale_range=(1.0, 1.0), rot_range=(20.0, 20.0, 180.0)) if fill else {}
    poses = synth.sample_poses(n, 3, model, **kw)
    _, prims, bbox = synth.forward_kinematics(poses, model)
    if fill:
        bbox[:] = (0, 0, FW, FH)
    if K > prims.shape[1]:
        prims = np.concatenate([prims, prims[:, :K - prims.shape[1]]], 1)
    return prims, bbox


def call_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=2)
    ap.add_argument("--parent", default=None, help="hash of the commit the measured tree sits on (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "synth_render.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/synth_render_timing.py needs a GPU: nothing is measured without one")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    n = a.frames
    say("synthetic hand frames: awr_synth_render, %d frames of %d x %d uint16 per call, one %s" % (n, FH, FW, torch.cuda.get_device_name(0)))
    say("parent commit: %s" % head)
    say("procedural hands (awr_amd/synth.py): these numbers say what generating them costs and nothing about NYU")
    say()
    dev = torch.device("cuda")
    out = torch.empty((n, FH, FW), dtype=torch.uint16, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    cases, host = [], {}
    for fill in (False, True):
        for K in (22, 32):
            prims, bbox = tables(n, fill, K)
            host[(fill, K)] = (prims, bbox)
            p, b = torch.from_numpy(prims).to(dev), torch.from_numpy(bbox).to(dev)
            name = "K = %d, %s" % (K, "hand fills the frame" if fill else "usual box")
            area = float(((bbox[:, 2] - bbox[:, 0]) * (bbox[:, 3] - bbox[:, 1])).mean()) / (FH * FW)
            cases.append((name, area, lambda p=p, b=b: synth.render_device(p, b, out, status=status, noise_mm=0)))
    for _, _, fn in cases:
        call_ms(fn, 3)
    assert int((status != 0).sum()) == 0
    ms = {name: [] for name, _, _ in cases}
    for _ in range(a.runs):
        for name, _, fn in cases:
            ms[name].append(call_ms(fn, a.reps) / n)
    say("(a) milliseconds per frame (HIP events over %d back-to-back calls of %d frames; %d repeats, the cases alternating; tables on the device)"
        % (a.reps, n, a.runs))
    nbytes = FH * FW * 2
    for name, area, _ in cases:
        med = statistics.median(ms[name])
        say("  %-32s box = %5.1f %% of the frame   %s   median %.5f ms   min - max %.5f - %.5f   %6.0f frames/s   written %5.2f TB/s"
            % (name, 100 * area, "  ".join("%.5f" % t for t in ms[name]), med, min(ms[name]), max(ms[name]), 1e3 / med, nbytes / (med * 1e-3) * 1e-12))
    say()
    say("(b) a frame is %d bytes of output; plain stores reach about %.1f TB/s on this chip (%.1f TB/s specified peak) = %.5f ms per frame:"
        % (nbytes, HBM_STORE_TBS, HBM_PEAK_TBS, nbytes / (HBM_STORE_TBS * 1e12) * 1e3))
    for name, _, _ in cases:
        med = statistics.median(ms[name])
        say("  %-32s %5.1f %% of that store rate%s" % (name, 100 * nbytes / (med * 1e-3) / (HBM_STORE_TBS * 1e12),
                                                     "" if nbytes / (med * 1e-3) > 0.5 * HBM_STORE_TBS * 1e12 else "  (bound by the float64 ray arithmetic, not by the stores)"))
    say("  (%d frames are %.0f MB: a call's output fits the 256 MiB Infinity Cache only for fewer than about 400 frames)" % (n, n * nbytes / 1e6))
    say()
    say("(c) the numpy statement (awr_amd.synth.render) on this host, %d frames, one thread of %s" % (a.host_frames, os.uname().machine))
    for (fill, K), (prims, bbox) in host.items():
        if K != 22:
            continue
        t0 = time.perf_counter()
        want = synth.render(prims[:a.host_frames], bbox[:a.host_frames])
        dt = (time.perf_counter() - t0) / a.host_frames * 1e3
        name = "K = %d, %s" % (K, "hand fills the frame" if fill else "usual box")
        synth.render_device(prims, bbox, out, status=status)
        same = np.array_equal(out[:a.host_frames].cpu().numpy(), want)
        say("  %-32s %9.1f ms per frame = %7.0f x the kernel's %.5f ms; frames equal: %s" % (name, dt, dt / statistics.median(ms[name]),
                                                                                       statistics.median(ms[name]), same))
    say()
    say("65 536 frames at the usual-box rate: %.2f s of rendering (plus the host's kinematics)" % (65536 * statistics.median(ms[cases[0][0]]) * 1e-3))
    say("not measured here: the host side (sample_poses + forward_kinematics), any multi-GPU timing")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
