"""What TrainEngine's clip_grad_norm / grad_norm / accum_steps cost, on one MI355X with synthetic data (ResNet18, batch 64) -> profiles/grad_clip.txt

    python tools/grad_clip_timing.py [--steps 100] [--runs 5] [--reps 200] [--parent HASH] [--out profiles/grad_clip.txt]

  * the train step (HIP events around `steps` step() calls, median of `runs` rounds) of four engines built alike in the same process: the
    options off, clip_grad_norm, grad_norm=True alone, accum_steps=2 (reported per micro-step: half of its calls accumulate, half apply);
  * the new launches alone (HIP events around `reps` back-to-back launches over arenas of the network's size): microseconds, bytes moved per
    second and that rate as a fraction of the 6.3 TB/s a float4 copy reaches on this part (8.0 TB/s specified).
The arms alternate (off, clip, norm, accum, off, ...) so that clock drift lands on all of them.  What to check: clipping adds one read of the
gradient arena and two small launches, accumulation one read-modify-write of it per non-applying micro-step."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle")]
import awr_amd  # noqa: E402
import awr_oracle as O  # noqa: E402
from awr_amd import _lib as L  # noqa: E402
from awr_amd.trainer import TrainEngine  # noqa: E402

B, S, J = 64, 128, 14
HBM_COPY = 6.29e12      # bytes/s of a float4 copy on the MI355X (79 % of the 8.0 TB/s specified)
ARMS = [("options off", {}), ("clip_grad_norm=1.0", dict(clip_grad_norm=1.0)), ("grad_norm=True", dict(grad_norm=True)),
        ("accum_steps=2", dict(accum_steps=2))]


def build(kw):
    torch.manual_seed(0)
    net = awr_amd.get_deconv_net(18, J, 2).cuda()
    return TrainEngine(net, B, S, 1.0, coord_weight=1.0, dense_weight=1.0, use_graph=False, **kw)


def step_ms(eng, batch, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        eng.step(*batch)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def launch_us(fn, reps):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--parent", default=None, help="hash of the commit the measured tree sits on (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grad_clip.txt"))
    a = ap.parse_args()
    assert a.steps % 2 == 0, "an even number of steps: whole accumulation windows"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("gradient clipping / accumulation timing: ResNet18, batch %d, %d^2, synthetic data, one %s" % (B, S, torch.cuda.get_device_name(0)))
    say("parent commit: %s" % head)
    say()
    img, jt = O.synth_batch(B, S, J, seed=5)
    batch = (img.cuda(), jt.cuda())
    engines = []
    for name, kw in ARMS:
        eng = build(kw)
        step_ms(eng, batch, 4)          # untimed: plan build, tile autotune, kernel load; whole windows
        engines.append((name, eng))
    n = engines[0][1].net.n_active
    say("gradient arena: %d floats = %.1f MB" % (n, 4e-6 * n))
    say()
    times = {name: [] for name, _ in engines}
    for _ in range(a.runs):
        for name, eng in engines:
            times[name].append(step_ms(eng, batch, a.steps))
    say("train step, ms per step() call (HIP events over %d calls; %d rounds, arms alternating)" % (a.steps, a.runs))
    base = statistics.median(times[engines[0][0]])
    for name, _ in engines:
        med = statistics.median(times[name])
        say("  %-20s %s   median %8.3f ms   (%+.3f ms, %+.2f %% vs options off)"
            % (name, "  ".join("%8.3f" % t for t in times[name]), med, med - base, 100.0 * (med / base - 1)))
    spread = max(times[engines[0][0]]) - min(times[engines[0][0]])
    say("  (the options-off arm's own spread over its rounds: %.3f ms)" % spread)
    say("  accum_steps=2 is per micro-step: one of two calls ends in awr_grad_accumulate (no optimiser), the other in the optimiser with g2")
    say()
    # the launches alone, on scratch arenas of the network's size
    dev = batch[0].device
    p, g, g2, m, v, acc = (torch.randn(n, device=dev) * 0.01 for _ in range(6))
    v.abs_()
    scr = torch.zeros(int(L.lib.awr_grad_norm_scratch(n)) // 8, dtype=torch.float64, device=dev)
    norm, scale = torch.zeros(1, dtype=torch.float64, device=dev), torch.ones(1, device=dev)
    s = L.stream()
    P = L.ptr
    cases = [
        ("awr_adam_step", 7, lambda: L.call("awr_adam_step", P(p), P(g), P(m), P(v), n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 10, 1.0, s)),
        ("awr_adam_step_dev (dev_scale)", 7, lambda: L.call("awr_adam_step_dev", P(p), P(g), None, P(scale), P(m), P(v), n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 10, 1.0, s)),
        ("awr_adam_step_dev (g2, dev_scale)", 8, lambda: L.call("awr_adam_step_dev", P(p), P(g), P(g2), P(scale), P(m), P(v), n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 10, 1.0, s)),
        ("awr_grad_norm", 1, lambda: L.call("awr_grad_norm", P(g), None, n, 1.0, 1.0, P(scr), P(norm), P(scale), s)),
        ("awr_grad_norm (g2)", 2, lambda: L.call("awr_grad_norm", P(g), P(g2), n, 1.0, 1.0, P(scr), P(norm), P(scale), s)),
        ("awr_grad_accumulate (first=0)", 3, lambda: L.call("awr_grad_accumulate", P(acc), P(g), n, 0, s)),
        ("awr_grad_accumulate (first=1)", 2, lambda: L.call("awr_grad_accumulate", P(acc), P(g), n, 1, s)),
    ]
    say("the launches alone, %d floats per arena (HIP events over %d back-to-back launches; awr_grad_norm is its two launches)" % (n, a.reps))
    for name, arenas, fn in cases:
        us = launch_us(fn, a.reps)
        rate = arenas * 4.0 * n / (us * 1e-6)
        say("  %-36s %8.2f us   %d arena passes = %6.1f MB   %6.2f TB/s = %3.0f %% of the %.2f TB/s copy rate"
            % (name, us, arenas, arenas * 4e-6 * n, rate * 1e-12, 100.0 * rate / HBM_COPY, HBM_COPY * 1e-12))
    say("  (arenas of this size fit the 256 MiB Infinity Cache: back-to-back launches over the same arenas can read above the HBM rate;")
    say("   inside a step the gradient arena was just written by the backward and the same holds)")
    say()
    say("not measured here: any effect on accuracy, any multi-GPU timing, the cost of all-reducing every micro-step")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
