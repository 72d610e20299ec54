"""What the depth pre-filter (awr_frames_denoise, Predictor(denoise=...)) costs on one MI355X -> profiles/denoise.txt

    python tools/denoise_timing.py [--reps 7] [--inner 20] [--out profiles/denoise.txt]

  * awr_frames_denoise alone at B = 1 and 64 for both radii, next to awr_hands_isolate (K = 2) and awr_detect at the same B, alternately in
    one run, on two kinds of frame: two-hand composites (most pixels are 0: a zero pixel without `fill` selects nothing) and wall frames
    (every pixel is valid and selects a median).  The bytes the algorithm needs -- 2 read and 2 written per pixel -- over the kernel time;
  * the 5 x 5 form on wall frames next to the same launch on all-zero frames, which stages, reads LDS and stores the same bytes but selects
    nothing: the difference is the selection arithmetic;
  * Predictor.predict with and without denoise at max_batch 1 and 64, alternately.  The predictor WITHOUT denoise issues the parent
    commit's launches with the parent's arguments (tests/test_predictor_trace_gpu.py holds them to the recorded ones): those rows are the
    parent's predictor, timed in this run.
Method: tools/predict_timing.py's -- HIP events around `inner` back-to-back calls, `reps` repetitions after a warm-up, median and
min ... max; the arms of a comparison alternate.  No bar is fixed: read an increment against the spread of its rows.  UNMEASURED: real
frames."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tools"), os.path.join(REPO, "tests")]
import awr_amd  # noqa: E402
from awr_amd import _lib as L  # noqa: E402
from awr_amd import detect as D  # noqa: E402
from detect_hands_timing import composites, store_of  # noqa: E402
from predict_timing import FH, FW, J, event_ms, fmt, synthetic_frames  # noqa: E402

HBM_SPEC_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/denoise_timing.py needs a GPU: nothing is measured without one")
    import awr_oracle as O
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent_commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    prop = torch.cuda.get_device_properties(0)
    say("depth pre-filter (awr_frames_denoise, DESIGN.md 4.30): %d x %d uint16 frames, ResNet18" % (FH, FW))
    say("box: one %s (%s, %d CUs), torch %s, HIP %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
                                                       torch.__version__, torch.version.hip))
    say("parent commit: %s" % head)
    say("method: HIP events over %d back-to-back calls, %d repetitions after warm-up; frames resident on the device; the arms alternate" % (a.inner, a.reps))
    say("UNMEASURED: real frames")
    say()
    _, _, hands = composites(64, False, dev)
    wall = torch.from_numpy(synthetic_frames(64)).to(dev)
    zeros = torch.zeros_like(wall.view(torch.int16)).view(torch.uint16)
    say("awr_frames_denoise alone (one launch; edge 40, support 0, no fill) next to awr_hands_isolate (K = 2, one launch) and awr_detect (seed nearest,")
    say("2 refinement passes), the same B, alternately.  GB/s: the 4 bytes per pixel the algorithm needs (2 read, 2 written) over the kernel time;")
    say("HBM roof %.1f TB/s spec.  hands: two-hand composites, %.1f %% of the pixels valid; wall: every pixel valid" % (HBM_SPEC_TBS, 100.0 * float((hands.view(torch.int16) != 0).double().mean())))
    for B in (1, 64):
        idx = torch.arange(B, dtype=torch.int64, device=dev)
        out = torch.empty((B, FH, FW), dtype=torch.uint16, device=dev)
        iso_out = torch.empty((2 * B, FH, FW), dtype=torch.uint16, device=dev)
        two = store_of(hands)
        _, _, info, _, labels = D.hands_device(two, idx, 2, labels=True)
        arms = {}
        for kind, frames in (("hands", hands), ("wall ", wall)):
            for r in (1, 2):
                arms["awr_frames_denoise r=%d %s" % (r, kind)] = (lambda f=frames, r=r: D.denoise_device(store_of(f), idx, r, 40.0, 0, None, out=out), True)
        arms["awr_hands_isolate K=2 hands "] = (lambda: D.isolate_device(two, idx, labels, info=info, out=iso_out), False)
        arms["awr_detect        hands      "] = (lambda: D.detect_device(two, idx), False)
        arms["awr_detect        wall       "] = (lambda: D.detect_device(store_of(wall), idx, depth_range=(200.0, 1200.0)), False)
        for _ in range(2):
            for name, (fn, mine) in arms.items():
                ms = event_ms(fn, a.inner, a.reps)
                extra = ""
                if mine:
                    gbs = B * FH * FW * 4 / (statistics.median(ms) * 1e-3) / 1e9
                    extra = "   %7.1f GB/s = %.1f %% of the spec roof" % (gbs, 0.1 * gbs / HBM_SPEC_TBS)
                say("  B = %2d  %-28s %s%s" % (B, name, fmt(ms), extra))
        say()
        del out, iso_out, labels
    say("  (times include the wrapper's host work and one small status allocation per call; at B = 1 a call is a launch's latency, not a bandwidth)")
    say()
    say("what bounds the 5 x 5 form: the same launch (r = 2, B = 64, edge 40, support 0, no fill) on wall frames, where every pixel selects a")
    say("median of up to 25 keys in 16 counting steps, and on all-zero frames, where the staging, the LDS reads and the stores are the same bytes")
    say("and nothing is selected; and r = 1 on the same two")
    idx = torch.arange(64, dtype=torch.int64, device=dev)
    out = torch.empty((64, FH, FW), dtype=torch.uint16, device=dev)
    med = {}
    for _ in range(2):
        for r in (2, 1):
            for kind, frames in (("wall ", wall), ("zeros", zeros)):
                ms = event_ms(lambda: D.denoise_device(store_of(frames), idx, r, 40.0, 0, None, out=out), a.inner, a.reps)
                med[(r, kind)] = statistics.median(ms)
                say("  r = %d  %s  %s" % (r, kind, fmt(ms)))
    for r in (2, 1):
        say("  r = %d: selection is %.0f %% of the wall-frame time (last pass): the form is bound by %s"
            % (r, 100.0 * (1.0 - med[(r, "zeros")] / med[(r, "wall ")]),
               "the selection arithmetic" if med[(r, "zeros")] < 0.5 * med[(r, "wall ")] else "staging and stores"))
    say()
    del out
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    say("Predictor.predict, frames -> joints on the device, img_size 64, two-hand composites on the device: no denoise (the parent commit's launches)")
    say("against denoise=True and denoise=dict(radius=2, edge=40, support=6, fill=18), alternately")
    for B in (1, 64):
        preds = {"denoise=None (the parent's)  max_batch %2d" % B: awr_amd.Predictor(net, 64, 1.0, max_batch=B),
                 "denoise=True                 max_batch %2d" % B: awr_amd.Predictor(net, 64, 1.0, max_batch=B, denoise=True),
                 "denoise=(2, 40, 6, 18)       max_batch %2d" % B: awr_amd.Predictor(net, 64, 1.0, max_batch=B, denoise=dict(radius=2, edge=40, support=6, fill=18))}
        for _ in range(2):
            for name, p in preds.items():
                ms = event_ms(lambda: p.predict(hands[:B]), a.inner if B == 1 else max(2, a.inner // 4), a.reps)
                say("  %-44s %s" % (name, fmt(ms)))
        del preds
        say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
