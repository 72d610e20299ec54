"""What TrainEngine's ema_decay costs, on one MI355X with synthetic data (ResNet18, batch 64) -> profiles/ema_update.txt

    python tools/ema_timing.py [--steps 100] [--runs 5] [--reps 200] [--parent HASH] [--out profiles/ema_update.txt]

  (a) the kernel against its yardstick: awr_ema_update and awr_grad_accumulate(first=0) move the same 12 bytes per element (two reads, one
      write).  Both run over scratch arenas of n = n_params floats, `reps` back-to-back launches between two HIP events, the two alternating
      over `runs` repeats after a warm-up; median, min - max and the achieved TB/s from 12 * n bytes of each.
  (b) the train step (HIP events around `steps` step() calls) of two engines built alike in the same process, ema_decay set and not, alternating
      over `runs` rounds: the medians, their difference and the plain arm's own spread.
  (c) the parent commit hash.
There is no fall-back: without a GPU the tool fails."""
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
ARMS = [("ema off", {}), ("ema_decay=0.999", dict(ema_decay=0.999))]


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ema_update.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ema_timing.py needs a GPU: nothing is measured without one")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("weight EMA timing: ResNet18, batch %d, %d^2, synthetic data, one %s" % (B, S, torch.cuda.get_device_name(0)))
    say("parent commit: %s" % head)
    say()
    img, jt = O.synth_batch(B, S, J, seed=5)
    batch = (img.cuda(), jt.cuda())
    engines = []
    for name, kw in ARMS:
        eng = build(kw)
        step_ms(eng, batch, 4)          # untimed: plan build, tile autotune, kernel load
        engines.append((name, eng))
    net = engines[0][1].net
    n = net.n_params
    say("parameter arena: %d floats = %.1f MB (buffer arena: %d floats)" % (n, 4e-6 * n, net._barena.numel()))
    say()
    # (a) the kernel and its yardstick on scratch arenas of the network's size
    dev = batch[0].device
    ema, src, acc, g = (torch.randn(n, device=dev) * 0.01 for _ in range(4))
    s, P = L.stream(), L.ptr
    cases = [("awr_ema_update (w = 1e-3)", lambda: L.call("awr_ema_update", P(ema), P(src), n, 1e-3, s)),
             ("awr_grad_accumulate (first=0)", lambda: L.call("awr_grad_accumulate", P(acc), P(g), n, 0, s))]
    for _, fn in cases:
        launch_us(fn, 20)
    us = {name: [] for name, _ in cases}
    for _ in range(a.runs):
        for name, fn in cases:
            us[name].append(launch_us(fn, a.reps))
    say("(a) the launches alone, %d floats per arena, 12 bytes per element (HIP events over %d back-to-back launches; %d repeats, alternating)"
        % (n, a.reps, a.runs))
    for name, _ in cases:
        med = statistics.median(us[name])
        say("  %-32s %s   median %7.2f us   min - max %7.2f - %7.2f   %5.2f TB/s"
            % (name, "  ".join("%7.2f" % t for t in us[name]), med, min(us[name]), max(us[name]), 12.0 * n / (med * 1e-6) * 1e-12))
    (k_name, _), (y_name, _) = cases
    diff = statistics.median(us[k_name]) - statistics.median(us[y_name])
    spread = max(us[y_name]) - min(us[y_name])
    say("  awr_ema_update - yardstick: %+.2f us (medians); the yardstick's own min - max spread: %.2f us -> %s"
        % (diff, spread, "within it" if diff <= spread else "EXCEEDS it: see the compiler's resource report"))
    say("  (arenas of this size fit the 256 MiB Infinity Cache: back-to-back launches over the same arenas can read above the HBM rate)")
    say()
    # (b) the step with and without the EMA
    times = {name: [] for name, _ in engines}
    for _ in range(a.runs):
        for name, eng in engines:
            times[name].append(step_ms(eng, batch, a.steps))
    say("(b) train step, ms per step() call (HIP events over %d calls; %d rounds, arms alternating)" % (a.steps, a.runs))
    base = statistics.median(times[engines[0][0]])
    for name, _ in engines:
        med = statistics.median(times[name])
        say("  %-18s %s   median %8.3f ms   min - max %8.3f - %8.3f   (%+.3f ms, %+.2f %% vs ema off)"
            % (name, "  ".join("%8.3f" % t for t in times[name]), med, min(times[name]), max(times[name]), med - base, 100.0 * (med / base - 1)))
    say("  (the ema-off arm's own spread over its rounds: %.3f ms; an applying step adds two awr_ema_update launches)"
        % (max(times[engines[0][0]]) - min(times[engines[0][0]])))
    say()
    say("not measured here: any effect on accuracy, any multi-GPU timing")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
