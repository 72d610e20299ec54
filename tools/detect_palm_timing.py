"""What the palm pass (awr_detect_palm) costs on one MI355X, procedural 480 x 640 hands -> profiles/detect_palm.txt

    python tools/detect_palm_timing.py [--reps 7] [--inner 20] [--out profiles/detect_palm.txt]

  * awr_detect alone (seed "nearest" + 2 refinement passes), awr_detect followed by awr_detect_palm, and awr_detect_palm alone on the
    detector's centres, at B = 1 and B = 64;
  * Predictor.predict (ResNet18, img_size 128, frames resident on the device) at max_batch = 1 with palm off and on, the two measured
    alternately, twice.
The frames are awr_amd.synth hands with the forearm (seed 202), rendered on the device: the silhouettes the pass was designed for, so the
window, the medial set and the loop lengths of the row pass are the realistic ones.  Method: tools/predict_timing.py's -- HIP events around
`inner` back-to-back calls, `reps` repetitions after a warm-up, median and min ... max.  No bar is fixed: the palm figures are to be read
against awr_detect and the plain Predictor of the same run.  The net has procedural weights: this tool says nothing about accuracy
(tools/synth_accuracy.py does, on procedural hands; nothing does on real frames)."""
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
from awr_amd import _lib as L  # noqa: E402
from awr_amd import detect as D  # noqa: E402
from awr_amd import synth  # noqa: E402
from predict_timing import FH, FW, J, S, event_ms, fmt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "detect_palm.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/detect_palm_timing.py needs a GPU: nothing is measured without one")
    import awr_oracle as O
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent_commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    prop = torch.cuda.get_device_properties(0)
    say("the palm pass: procedural %d x %d uint16 hands with the forearm (awr_amd.synth, seed 202), ResNet18, img_size %d" % (FH, FW, S))
    say("box: one %s (%s, %d CUs), torch %s, HIP %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
                                                       torch.__version__, torch.version.hip))
    say("parent commit: %s" % head)
    say("method: HIP events over %d back-to-back calls, %d repetitions after warm-up; frames resident on the device" % (a.inner, a.reps))
    say("awr_detect_palm is nine launches, a frame split by rows over several workgroups; its figures are to be read against awr_detect's in the same run")
    say()
    sf = synth.SyntheticFrames(64, 202, "test")
    assert sf.check() == 0
    store = sf.frame_store
    for B in (1, 64):
        idx = torch.arange(B, dtype=torch.int64, device=dev)
        scratch = torch.empty(int(L.lib.awr_detect_palm_scratch(B, FH, FW)) // 4, dtype=torch.int32, device=dev)
        co, so = torch.empty((B, 3), dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        info = torch.empty((B, 4), dtype=torch.int32, device=dev)
        c, s = D.detect_device(store, idx)

        def palm(c, s):
            return D.palm_device(store, idx, c, s, center_out=co, status_out=so, info=info, scratch=scratch)
        palm(c, s)
        i = info.cpu().numpy()
        say("B = %d   (palm radius %s px, disc %s px: median over the batch; %d of %d frames OK)"
            % (B, np.median(np.sqrt(i[:, 2])).round(1), int(np.median(i[:, 3])), int((so == 0).sum()), B))
        ms_d = event_ms(lambda: D.detect_device(store, idx), a.inner, a.reps)
        say("  awr_detect, seed \"nearest\" + 2 refinement passes:   %s" % fmt(ms_d))
        ms_b = event_ms(lambda: palm(*D.detect_device(store, idx)), a.inner, a.reps)
        say("  awr_detect, then awr_detect_palm:                   %s" % fmt(ms_b))
        ms_p = event_ms(lambda: palm(c, s), a.inner, a.reps)
        say("  awr_detect_palm alone:                              %s   = %.3f ms per frame" % (fmt(ms_p), statistics.median(ms_p) / B))
        say()
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    data = store.data[:1]
    preds = {False: awr_amd.Predictor(net, S, 1.0, max_batch=1, frame_shape=(FH, FW)), True: awr_amd.Predictor(net, S, 1.0, max_batch=1,
                                                                                                            frame_shape=(FH, FW), palm=True)}
    say("Predictor.predict, max_batch = 1, frames -> joints on the device, palm off and on alternately")
    for _ in range(2):
        for on in (False, True):
            ms = event_ms(lambda: preds[on].predict(data), a.inner, a.reps)
            say("  palm=%-5s  %s   = %.1f frames/s" % (on, fmt(ms), 1.0 / (statistics.median(ms) * 1e-3)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
