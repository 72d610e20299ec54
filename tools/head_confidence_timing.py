"""What per-joint confidence costs, on one MI355X with synthetic data -> profiles/head_confidence.txt

    python tools/head_confidence_timing.py [--runs 3] [--reps 200] [--batches 30] [--parent HASH] [--out profiles/head_confidence.txt]

  (a) the head pass alone (HIP events around `reps` back-to-back calls, arms alternating, median of `runs` rounds, spread = max - min over
      the rounds): awr_head_forward_nhwc with its statistics, and the same followed by awr_head_confidence_nhwc, at B = 64 / 128 (J = 14,
      F = 64) and B = 128 (J = 21, F = 128).
  (b) Predictor.predict frames/s with confidence off and on, ResNet18, 480 x 640 frames, B = 1 and 64 (median of `runs` rounds of `batches`
      calls after one untimed call per arm, arms alternating)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import awr_amd  # noqa: E402,F401
from awr_amd import _lib as L  # noqa: E402
from awr_amd.trainer import SyntheticHands  # noqa: E402

KERNEL_SHAPES = [(64, 14, 64), (128, 14, 64), (128, 21, 128)]      # (B, J, F); H = 2 F


def kernel_arms(B, J, F, dev):
    H, cp = 2 * F, (4 * J + 31) // 32 * 32
    g = torch.Generator().manual_seed(B + J + F)
    img = SyntheticHands(B, img_size=H, jt_num=J, seed=3).img.to(dev)
    pred = (torch.rand(B, F * F, cp, generator=g) * 0.4 - 0.2).to(dev)
    pred[:, :, 4 * J:] = 0
    scratch = torch.zeros(int(L.lib.awr_head_nhwc_scratch(B, J, F)), device=dev)
    jt, stat, conf = torch.zeros(B, J, 3, device=dev), torch.zeros(B, J, 2, device=dev), torch.zeros(B, J, 4, device=dev)
    s = L.stream()
    P = (L.ptr(pred), cp, L.ptr(img))

    def head():
        L.call("awr_head_forward_nhwc", *P, B, J, F, H, 0.4, L.ptr(scratch), L.ptr(jt), L.ptr(stat), s)

    def both():
        head()
        L.call("awr_head_confidence_nhwc", *P, L.ptr(jt), L.ptr(stat), B, J, F, H, 0.4, L.ptr(scratch), L.ptr(conf), s)
    return {"head": head, "head+conf": both}, (pred, img, scratch, jt, stat, conf)


def time_arms(arms, runs, reps):
    us = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(10):
            fn()
    for _ in range(runs):
        for k, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            us[k].append(1e3 * a.elapsed_time(b) / reps)
    return us


def blob_frames(n):
    f = np.full((n, 480, 640), 1500, np.uint16)
    vv, uu = np.mgrid[0:480, 0:640]
    for b in range(n):
        cu, cv = 200 + (37 * b) % 240, 160 + (23 * b) % 160
        m = (np.abs(uu - cu) <= 60) & (np.abs(vv - cv) <= 60)
        f[b][m] = (680 + (uu[m] + vv[m]) % 41).astype(np.uint16)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--parent", default=None, help="hash of the commit the measured tree sits on (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "head_confidence.txt"))
    a = ap.parse_args()
    assert a.runs >= 3
    dev, lines, med = torch.device("cuda"), [], statistics.median

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("head_confidence timing: one %s, synthetic data" % torch.cuda.get_device_name(0))
    say("parent commit: %s" % head)
    say()
    say("(a) the head pass alone, us per call (median of %d rounds of %d back-to-back calls; arms alternate; +- = max - min over the rounds)" % (a.runs, a.reps))
    say("    head = awr_head_forward_nhwc (joints + statistics), head+conf = the same followed by awr_head_confidence_nhwc")
    for B, J, F in KERNEL_SHAPES:
        arms, keep = kernel_arms(B, J, F, dev)
        us = time_arms(arms, a.runs, a.reps)
        m = {k: med(v) for k, v in us.items()}
        sp = {k: max(v) - min(v) for k, v in us.items()}
        say("    B=%3d J=%2d F=%3d   head %8.2f +- %5.2f   head+conf %8.2f +- %5.2f   conf alone %8.2f   (head+conf)/head %.3f"
            % (B, J, F, m["head"], sp["head"], m["head+conf"], sp["head+conf"], m["head+conf"] - m["head"], m["head+conf"] / m["head"]))
        del arms, keep
    say()
    say("(b) Predictor.predict, ResNet18, 480 x 640 uint16 frames on the host, frames/s (median of %d rounds of %d calls, arms alternate)" % (a.runs, a.batches))
    net = awr_amd.get_deconv_net(18, 14, 2).cuda().eval()
    for B in (1, 64):
        frames = blob_frames(B)
        prs = {c: awr_amd.Predictor(net, 128, 0.4, max_batch=B, depth_range=(200.0, 1200.0), slab=100.0, confidence=c) for c in (False, True)}
        rates = {c: [] for c in prs}
        for p in prs.values():
            p.predict(frames)               # untimed: plan build, tile autotune
            torch.cuda.synchronize()
        for _ in range(a.runs):
            for c, p in prs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.batches):
                    p.predict(frames)
                torch.cuda.synchronize()
                rates[c].append(a.batches * B / (time.perf_counter() - t0))
        off, on = med(rates[False]), med(rates[True])
        say("    B=%2d confidence=False  %s   median %9.1f +- %.1f" % (B, "  ".join("%9.1f" % r for r in rates[False]), off, max(rates[False]) - min(rates[False])))
        say("    B=%2d confidence=True   %s   median %9.1f +- %.1f   on/off %.3f" % (B, "  ".join("%9.1f" % r for r in rates[True]), on,
                                                                                    max(rates[True]) - min(rates[True]), on / off))
        del prs
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
