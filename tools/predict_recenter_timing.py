"""What re-centring and tracking cost on one MI355X, synthetic 480 x 640 frames -> profiles/predict_recenter.txt

    python tools/predict_recenter_timing.py [--reps 7] [--inner 20] [--parent PARENT.txt ...] [--this THIS.txt ...] [--parent-commit SHA]
                                            [--out profiles/predict_recenter.txt]

The frames, the net and the method are tools/predict_timing.py's: HIP events around `inner` back-to-back calls, `reps` repetitions after a
warm-up that covers plan build and tile autotuning, median and min ... max.  At B = 1 and B = 64:
  * Predictor.predict (frames resident on the device -> joints) with recenter 0, 1, 2 and with track off and on;
  * awr_joints_center and awr_centers_select alone.
--parent / --this: files tools/predict_timing.py (the same, unchanged tool) wrote at the PARENT commit and in THIS tree, on the same box in
the same session, runs alternating; their detector and "frames -> joints on the device" lines are copied in as the answer to "does the
default path (recenter=0, track=False) cost what it did", and the parent's figures give the expected cost of one more pass (predict minus
the detector).  Both questions are read off the min ... max spreads, no bar is fixed in advance.  Whether re-centring improves ACCURACY on real frames is not measured here or
anywhere: there are no NYU frames and no trained checkpoint where this runs; the net has procedural weights and the blobs are synthetic."""
import argparse
import os
import re
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tools")]
import awr_amd  # noqa: E402
from awr_amd import detect as D  # noqa: E402
from predict_timing import DET, FH, FW, J, S, event_ms, fmt, synthetic_frames  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--parent", nargs="*", default=[], help="tools/predict_timing.py's outputs at the parent commit, same box, same session")
    ap.add_argument("--this", nargs="*", default=[], help="the same tool's outputs in this tree, runs alternating with the parent's")
    ap.add_argument("--parent-commit", default=None, help="the commit --parent was measured at (default: git HEAD)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "predict_recenter.txt"))
    a = ap.parse_args()
    import awr_oracle as O
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent_commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    prop = torch.cuda.get_device_properties(0)
    say("re-centring and tracking: synthetic %d x %d uint16 frames, ResNet18, img_size %d" % (FH, FW, S))
    say("box: one %s (%s, %d CUs, %.0f GB), torch %s, HIP %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
                                                             prop.total_memory / 2 ** 30, torch.__version__, torch.version.hip))
    say("parent commit: %s" % head)
    say("method: HIP events over %d back-to-back calls, %d repetitions after warm-up; frames resident on the device" % (a.inner, a.reps))
    say("whether re-centring or tracking improves accuracy on real NYU frames is UNMEASURED: no NYU frames and no trained checkpoint exist on")
    say("this machine; the net has procedural weights (its joints are arbitrary, so the gate is opened wide below) and the blobs are synthetic")
    say()
    parent = {}          # B -> [(detector median, predict median)] of the parent's runs
    if not a.parent:
        say("baseline: NOT MEASURED (no --parent file: run tools/predict_timing.py at the parent commit on the same box and pass its output)")
    for kind, files in (("the parent commit", a.parent), ("this tree, default options", a.this)):
        for path in files:
            say("tools/predict_timing.py at %s, same box, same session (%s):" % (kind, os.path.basename(path)))
            B = det = None
            for ln in open(path).read().splitlines():
                m = re.search(r"median\s+([0-9.]+) ms", ln)
                if ln.startswith("B = "):
                    B = int(ln[4:])
                    say("    " + ln)
                elif "+ 2 refinement passes" in ln and m:
                    det = float(m.group(1))
                    say("    " + ln.strip())
                elif "frames -> joints on the device" in ln and m:
                    say("    " + ln.strip())
                    if files is a.parent:
                        parent.setdefault(B, []).append((det, float(m.group(1))))
    say()
    frames = synthetic_frames(64)
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    # procedural weights put the joints anywhere: a wide-open gate makes every finite frame move, which is the costlier case (a moved
    # frame is cropped anew; a kept one repeats its pass, for the same launches)
    gate = dict(max_shift=1e9)
    for B in (1, 64):
        data = torch.from_numpy(frames[:B]).to(dev)
        say("B = %d" % B)
        base = None
        for recenter, track in ((0, False), (1, False), (2, False), (0, True), (1, True), (2, True)):
            pred = awr_amd.Predictor(net, S, 1.0, max_batch=B, frame_shape=(FH, FW), seed="nearest", refine_iters=2, recenter=recenter,
                                     track=track, **gate, **DET)
            ms = event_ms(lambda: pred.predict(data), a.inner, a.reps)
            m = statistics.median(ms)
            base = m if base is None else base
            note = ""
            if recenter or track:
                codes = pred.recenter_codes.cpu()
                note = "   %+.3f ms; moved per awr_joints_center call: %s of %d" % (m - base, (codes == D.MOVED).sum(1).tolist(), B)
            say("  predict, recenter=%d track=%-5s  %s   = %.1f frames/s%s" % (recenter, track, fmt(ms), B / (m * 1e-3), note))
            if (recenter, track) == (1, False) and parent.get(B):
                say("      expected for one more pass, from the parent's figures (predict - awr_detect = crop blocks + render + engine + un-projection): %s ms"
                    % ", ".join("%.3f" % (p - d) for d, p in parent[B]))
        # the two new launches alone, on the last predictor's buffers
        out = pred.predict(data)
        st, ust = pred._last[0], pred._last[1]
        cen, cube32 = pred.centers_uvd.clone(), pred._cube32
        co, nx, cd = (torch.empty((B, 3), dtype=torch.float64, device=dev), torch.empty((B, 3), dtype=torch.float64, device=dev),
                      torch.empty(B, dtype=torch.int32, device=dev))
        ms = event_ms(lambda: D.joints_center_device(out.xyz, cen, out.center_xyz, cube32, st, ust, pred.paras, pred.flip, max_shift=1e9,
                                                     depth_range=pred.depth_range, center_out=co, next_out=nx, code=cd), a.inner, a.reps)
        say("  awr_joints_center alone (J = %d):      %s" % (J, fmt(ms)))
        ms = event_ms(lambda: D.select_device(cen, st, co, st), a.inner, a.reps)
        say("  awr_centers_select alone:              %s   (the wrapper allocates its three outputs)" % fmt(ms))
        say()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
