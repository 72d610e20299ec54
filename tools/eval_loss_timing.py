"""What the validation loss of a scoring pass costs, on one MI355X with synthetic data -> profiles/eval_loss.txt

    python tools/eval_loss_timing.py [--frames 2048] [--runs 3] [--reps 200] [--parent HASH] [--out profiles/eval_loss.txt]

  (a) the kernel alone (HIP events around `reps` back-to-back calls, arms alternating, median of `runs` rounds, spread = max - min over the
      rounds): awr_head_eval_nhwc against awr_head_forward_nhwc -- what an eval pass pays without the loss -- and against
      awr_head_loss_step_nhwc, the training form, which does the same loads plus a full store stream.  Condition: the value-only form is not
      slower than the training form beyond the training form's own spread.
  (b) Trainer.test images/s on SyntheticHands with config.test_loss off and on, ResNet18 and Hourglass-1 at batch 128 (median of `runs`
      passes after one untimed pass per arm, arms alternating)."""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import awr_amd  # noqa: E402,F401
from awr_amd import _lib as L  # noqa: E402
from awr_amd.config import Config  # noqa: E402
from awr_amd.trainer import SyntheticHands, Trainer  # noqa: E402

KERNEL_SHAPES = [(64, 14, 64), (128, 14, 64), (128, 21, 128)]      # (B, J, F); H = 2 F


def kernel_arms(B, J, F, dev):
    H, cp = 2 * F, (4 * J + 31) // 32 * 32
    g = torch.Generator().manual_seed(B + J + F)
    data = SyntheticHands(B, img_size=H, jt_num=J, seed=3)
    img, jt_gt = data.img.to(dev), data.jt_uvd.to(dev).contiguous()
    pred = (torch.rand(B, F * F, cp, generator=g) * 0.4 - 0.2).to(dev)
    pred[:, :, 4 * J:] = 0
    scratch = torch.zeros(int(L.lib.awr_head_nhwc_scratch(B, J, F)), device=dev)
    jt, stat, g_jt = torch.zeros(B, J, 3, device=dev), torch.zeros(B, J, 2, device=dev), torch.zeros(B, J, 3, device=dev)
    acc, grad = torch.zeros(2, device=dev, dtype=torch.float64), torch.empty_like(pred)
    s = L.stream()
    P = (L.ptr(pred), cp, L.ptr(img))
    return {
        "forward": lambda: L.call("awr_head_forward_nhwc", *P, B, J, F, H, 0.4, L.ptr(scratch), L.ptr(jt), None, s),
        "eval": lambda: L.call("awr_head_eval_nhwc", *P, L.ptr(jt_gt), B, J, F, H, B, 0.4, 0.01, 0.0, 1.0, L.ptr(scratch), L.ptr(jt), None, L.ptr(acc), s),
        "train": lambda: L.call("awr_head_loss_step_nhwc", *P, L.ptr(jt_gt), B, J, F, H, 0.4, 0.01, 0.0, 1.0, L.ptr(scratch), L.ptr(jt), L.ptr(stat),
                                L.ptr(g_jt), L.ptr(acc), L.ptr(grad), s),
    }, (pred, img, jt_gt, scratch, jt, stat, g_jt, acc, grad)


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


def make_cfg(out_dir, net, ks, test_loss):
    class Cfg(Config):
        kernel_size = ks
        batch_size = 128
        num_workers = 0
        vis_freq = 0
        output_dir = out_dir
        load_model = ""
        exp_id = "%s_%d" % (net, test_loss)
        device_loader = False
    Cfg.net, Cfg.test_loss = net, test_loss
    return Cfg()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--parent", default=None, help="hash of the commit the measured tree sits on (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_loss.txt"))
    a = ap.parse_args()
    assert a.runs >= 3
    dev, lines, med = torch.device("cuda"), [], statistics.median

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("eval_loss timing: one %s, synthetic data" % torch.cuda.get_device_name(0))
    say("parent commit: %s" % head)
    say()
    say("(a) the head pass alone, us per call (median of %d rounds of %d back-to-back calls; arms alternate; +- = max - min over the rounds)" % (a.runs, a.reps))
    say("    forward = awr_head_forward_nhwc (joints), eval = awr_head_eval_nhwc (joints + loss, read-only), train = awr_head_loss_step_nhwc (joints + loss + gradient)")
    slower = []
    for B, J, F in KERNEL_SHAPES:
        arms, keep = kernel_arms(B, J, F, dev)
        us = time_arms(arms, a.runs, a.reps)
        m = {k: med(v) for k, v in us.items()}
        sp = {k: max(v) - min(v) for k, v in us.items()}
        say("    B=%3d J=%2d F=%3d   forward %8.2f +- %5.2f   eval %8.2f +- %5.2f   train %8.2f +- %5.2f   eval/forward %.3f   eval/train %.3f"
            % (B, J, F, m["forward"], sp["forward"], m["eval"], sp["eval"], m["train"], sp["train"], m["eval"] / m["forward"], m["eval"] / m["train"]))
        if m["eval"] > m["train"] + sp["train"]:
            slower.append((B, J, F))
        del arms, keep
    say("    condition (eval not slower than train beyond train's spread): %s" % ("MISSED at %s" % slower if slower else "met on every shape"))
    say()
    say("(b) Trainer.test, %d SyntheticHands images, batch 128, images/s per pass (median of %d, arms alternate)" % (a.frames, a.runs))
    tmp = tempfile.mkdtemp(prefix="eval_loss_")
    data = SyntheticHands(a.frames, seed=2)
    for net, ks in (("resnet_18", 1.0), ("hourglass_1", 0.4)):
        trs = {tl: Trainer(make_cfg(tmp, net, ks, tl), None, data) for tl in (False, True)}
        rates = {tl: [] for tl in trs}
        for tr in trs.values():
            tr.test(1)                      # untimed: plan build, tile autotune
        for _ in range(a.runs):
            for tl, tr in trs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.test(1)
                torch.cuda.synchronize()
                rates[tl].append(a.frames / (time.perf_counter() - t0))
        off, on = med(rates[False]), med(rates[True])
        say("    %-12s test_loss=False  %s   median %9.1f" % (net, "  ".join("%9.1f" % r for r in rates[False]), off))
        say("    %-12s test_loss=True   %s   median %9.1f   on/off %.3f   (%s)" % (net, "  ".join("%9.1f" % r for r in rates[True]), on, on / off,
                                                                                  {k: round(v, 5) for k, v in trs[True].last_test_loss.items()}))
        del trs
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
