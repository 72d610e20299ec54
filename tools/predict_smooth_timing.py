"""What the temporal joint filter costs on one MI355X -> profiles/predict_smooth.txt

    python tools/predict_smooth_timing.py [--reps 9] [--inner 50] [--out profiles/predict_smooth.txt]

  * awr_joints_filter alone (track.filter_step_device on resident tensors) at B x J = 1 x 14, 64 x 14 and 64 x 21, weight off and "conf";
  * Predictor.predict without and with smooth=True at max_batch 1 and 64 (ResNet18, img_size 128, 480 x 640 frames resident on the device),
    and with track=True without and with smooth lead=True, in the SAME run on the same box.
Method (tools/predict_timing.py's): every figure is a HIP-event time of `inner` back-to-back calls, repeated `reps` times after a warm-up
that covers plan build and tile autotuning; median and min ... max over the repetitions.  The two predictors of a comparison ALTERNATE
repetition by repetition, so drift of the box falls on both.  No threshold: the kernel touches a few kilobytes and is bound by its launch; the
record is the increment and the spread it has to be read against."""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tools")]
import awr_amd  # noqa: E402
from awr_amd import track as T  # noqa: E402
from predict_timing import DET, FH, FW, J, S, event_ms, fmt, synthetic_frames  # noqa: E402


def window_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fns, inner, reps, warm=3):
    """time several callables, one window each per repetition, in turn -> a list of per-call times for each"""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            out[k].append(window_ms(fn, inner))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "predict_smooth.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/predict_smooth_timing.py needs a GPU: nothing is measured without one")
    import awr_oracle as O
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("temporal joint filter (awr_joints_filter, DESIGN.md 4.25): what it costs; one %s" % torch.cuda.get_device_name(0))
    say("parent commit: %s" % head)
    say("method: HIP events over %d back-to-back calls, %d repetitions after warm-up; the rows of one comparison alternate repetition by repetition" % (a.inner, a.reps))
    say("no threshold: the kernel is bound by its launch; read each increment against the min ... max of the rows it is a difference of")
    say()
    say("awr_joints_filter alone (state resident, inputs resident, outputs preallocated)")
    rs = np.random.RandomState(0)
    for B, nj in ((1, 14), (64, 14), (64, 21)):
        xyz = torch.from_numpy((np.array([0.0, 0.0, 600.0]) + rs.normal(0, 5, (B, nj, 3))).astype(np.float32)).to(dev)
        conf = torch.from_numpy(rs.uniform(0.2, 1.0, (B, nj)).astype(np.float32)).to(dev)
        ok = torch.zeros(B, dtype=torch.int32, device=dev)
        for cfg in (dict(), dict(weight="conf", gate_mm=60.0)):
            state, count = T.filter_state_device(B, nj, dev)
            out = tuple(torch.empty((B, nj, 3), dtype=torch.float32, device=dev) for _ in range(3)) + (torch.empty((B, nj), dtype=torch.int32, device=dev),)
            ms = event_ms(lambda: T.filter_step_device(state, count, xyz, ok, ok, conf, cfg, None, None, out=out), a.inner * 4, a.reps)
            say("  B x J = %2d x %2d = %4d threads, %-28s %s" % (B, nj, B * nj, ("weight conf, gate 60 mm" if cfg else "defaults") + ":", fmt(ms)))
    say("  (a launch through ctypes from Python: the time is the enqueue rate of the host as much as the kernel)")
    say()
    frames = synthetic_frames(64)
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    for B in (1, 64):
        data = torch.from_numpy(frames[:B]).to(dev)
        kw = dict(max_batch=B, frame_shape=(FH, FW), seed="nearest", refine_iters=2, **DET)
        rows = (("plain", dict()), ("smooth=True", dict(smooth=True)), ("smooth weight=\"conf\"", dict(smooth=dict(weight="conf"))),
                ("track=True", dict(track=True)), ("track=True, smooth lead=True", dict(track=True, smooth=dict(lead=True))))
        preds = [awr_amd.Predictor(net, S, 1.0, **kw, **opt) for _, opt in rows]
        times = alternate([lambda p=p: p.predict(data) for p in preds], a.inner, a.reps)
        preds[0].check()
        say("Predictor.predict, frames resident on the device, max_batch = %d" % B)
        for (name, _), ms in zip(rows, times):
            say("  %-30s %s   = %.1f frames/s" % (name + ":", fmt(ms), B / (statistics.median(ms) * 1e-3)))
        med = [statistics.median(ms) for ms in times]
        say("  increments of the medians: smooth %+.3f ms, weight=\"conf\" %+.3f ms (the engine's confidence pass included) over plain; lead %+.3f ms over track=True"
            % (med[1] - med[0], med[2] - med[0], med[4] - med[3]))
        say("  the spread they are read against: plain min ... max = %.3f ms, track=True %.3f ms" % (max(times[0]) - min(times[0]), max(times[3]) - min(times[3])))
        say()
        del preds
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
