"""What hand identities cost on one MI355X -> appended to profiles/hands_identity.txt (tools/hands_identity_accuracy.py writes its first part)

    python tools/hands_assign_timing.py [--reps 9] [--inner 50] [--out profiles/hands_identity.txt]

  * awr_hands_assign alone (track.assign_step_device on resident tensors) at K x B = 2 x 1, 2 x 64 and 4 x 64, without and with the tracked
    inputs and the filter pointers, next to the two launches of its kind: awr_centers_select and awr_joints_filter;
  * Predictor(hands=2).predict without and with identity=True at max_batch 1 and 64 (ResNet18, img_size 128, two procedural hands per
    480 x 640 frame, resident on the device), and with identity, track=True and smooth=True together, in the SAME run on the same box.
Method (tools/predict_smooth_timing.py's): HIP-event time of `inner` back-to-back calls, `reps` repetitions after a warm-up; the predictors of
a comparison alternate repetition by repetition.  No threshold: the kernel reads and writes a few hundred bytes per frame and is bound by
its launch."""
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
from awr_amd import detect as D  # noqa: E402
from awr_amd import synth as SY  # noqa: E402
from awr_amd import track as T  # noqa: E402
from predict_smooth_timing import alternate  # noqa: E402
from predict_timing import DET, FH, FW, J, S, event_ms, fmt  # noqa: E402


def two_hand_frames(n, dev):
    model = SY.HandModel(forearm=False)
    rs = np.random.RandomState(3)
    frames = []
    for seed, u in ((31, 170.0), (32, 470.0)):
        poses = SY.place_poses(SY.sample_poses(n, seed, model), u, 200.0 + 80.0 * rs.uniform(size=n), 650.0 + 250.0 * rs.uniform(size=n), model)
        _, prims, bbox = SY.forward_kinematics(poses, model)
        out = torch.empty((n, FH, FW), dtype=torch.uint16, device=dev)
        SY.render_device(prims, bbox, out)
        frames.append(out)
    return SY.compose(*frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hands_identity.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hands_assign_timing.py needs a GPU: nothing is measured without one")
    import awr_oracle as O
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("what it costs; one %s" % torch.cuda.get_device_name(0))
    say("method: HIP events over %d back-to-back calls, %d repetitions after warm-up; the rows of one comparison alternate repetition by repetition" % (a.inner, a.reps))
    say("no threshold: read each increment against the min ... max of the rows it is a difference of")
    say()
    say("awr_hands_assign alone (state, inputs and outputs resident), next to awr_centers_select and awr_joints_filter")
    rs = np.random.RandomState(0)
    for K, B in ((2, 1), (2, 64), (4, 64)):
        cand = torch.from_numpy(np.array([300.0, 240.0, 700.0]) + rs.uniform(-100, 100, (K, B, 3))).to(dev)
        ok = torch.zeros((K, B), dtype=torch.int32, device=dev)
        for tracked, filtered in ((False, False), (True, True)):
            state = T.identity_state_device(K, B, dev)
            fs, fc = T.filter_state_device(K * B, J, dev) if filtered else (None, None)
            out = T.assign_step_device(*state, cand, ok)
            ms = event_ms(lambda: T.assign_step_device(*state, cand, ok, cand if tracked else None, ok if tracked else None, True, None,
                                                       filter_state=fs, filter_count=fc, out=out), a.inner * 4, a.reps)
            say("  K x B = %d x %2d (%2d waves), %-36s %s" % (K, B, B, ("tracked inputs, filter pointers" if tracked else "candidates only") + ":", fmt(ms)))
    B = 64
    c = torch.from_numpy(rs.uniform(100, 500, (B, 3))).to(dev)
    ok = torch.zeros(B, dtype=torch.int32, device=dev)
    ms = event_ms(lambda: D.select_device(c, ok, c, ok), a.inner * 4, a.reps)
    say("  awr_centers_select, B = 64 (its wrapper allocates the outputs):%s %s" % ("", fmt(ms)))
    xyz = torch.from_numpy((np.array([0.0, 0.0, 600.0]) + rs.normal(0, 5, (B, J, 3))).astype(np.float32)).to(dev)
    state, count = T.filter_state_device(B, J, dev)
    fout = tuple(torch.empty((B, J, 3), dtype=torch.float32, device=dev) for _ in range(3)) + (torch.empty((B, J), dtype=torch.int32, device=dev),)
    ms = event_ms(lambda: T.filter_step_device(state, count, xyz, ok, ok, None, True, None, None, out=fout), a.inner * 4, a.reps)
    say("  awr_joints_filter, B x J = 64 x 14, defaults:                  %s" % fmt(ms))
    say("  (a launch through ctypes from Python: the time is the enqueue rate of the host as much as the kernel)")
    say()
    frames = two_hand_frames(64, dev)
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    for B in (1, 64):
        data = frames[:B].contiguous()
        kw = dict(max_batch=B, frame_shape=(FH, FW), hands=2, refine_iters=2, **DET)
        rows = (("hands=2", dict()), ("hands=2, identity=True", dict(identity=True)),
                ("identity, track=True, smooth=True", dict(identity=True, track=True, smooth=True)))
        preds = [awr_amd.Predictor(net, S, 1.0, **kw, **opt) for _, opt in rows]
        times = alternate([lambda p=p: p.predict(data) for p in preds], a.inner if B == 1 else max(a.inner // 5, 4), a.reps)
        preds[0].check()
        say("Predictor(hands=2).predict, two hands per frame, frames resident on the device, max_batch = %d (plan of %d rows); n_hands of the first "
            "frames: %s" % (B, 2 * B, preds[1].predict(data).n_hands[:4].tolist()))
        for (name, _), ms in zip(rows, times):
            say("  %-36s %s   = %.1f frames/s" % (name + ":", fmt(ms), B / (statistics.median(ms) * 1e-3)))
        med = [statistics.median(ms) for ms in times]
        say("  increments of the medians over hands=2: identity %+.3f ms; identity with the tracker's second awr_detect, the final awr_joints_center, "
            "awr_centers_select and two awr_joints_filter launches %+.3f ms" % (med[1] - med[0], med[2] - med[0]))
        say("  the spread they are read against: hands=2 min ... max = %.3f ms" % (max(times[0]) - min(times[0])))
        say()
        del preds
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
