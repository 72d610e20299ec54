"""What the links across an occluder (awr_detect_hands_link) cost on one MI355X -> profiles/detect_hands_link.txt

    python tools/detect_hands_link_timing.py [--reps 9] [--inner 50] [--out profiles/detect_hands_link.txt]

Two rows per input and batch, taken ALTERNATELY in the same run: `edge 40` is awr_detect_hands_edge -- the parent commit's entry point
and launches, the yardstick -- and `link 40, gap G` is awr_detect_hands_link, the same launches and one more.  The ratio of the medians
is stated next to the spread of each row; no bar is fixed.  Inputs, all 480 x 640 and resident on the device: the overlapping two-hand
composites of tests/edge_cases.py (16 frames, repeated to fill a batch), the two-hand composites of tools/detect_hands_timing.py that do
not overlap, and a constructed worst case: vertical stripes of ONE rear column to `gap` front columns, where every rear pixel walks the
full gap to the right and to the left (gap 32 and gap 64).  B = 1 and B = 64, K = 2.  Then the link kernel's own time from the profiler's
kernel records at B = 1, and Predictor(hands=2, isolate=True, edge_mm=40) with and without link_mm=40 at max_batch 1 and 64.  Method:
tools/predict_timing.py's -- HIP events around `inner` back-to-back calls, `reps` repetitions after a warm-up, median and min ... max."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tools"), os.path.join(REPO, "tests")]
import awr_amd  # noqa: E402
import awr_oracle as O  # noqa: E402
from awr_amd import _lib as L  # noqa: E402
from awr_amd import detect as D  # noqa: E402
from awr_amd import synth  # noqa: E402
from detect_hands_timing import composites, kernel_times, store_of  # noqa: E402
from predict_timing import FH, FW, event_ms, fmt  # noqa: E402

EDGE, LINK, S, J = 40.0, 40.0, 128, 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "detect_hands_link.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/detect_hands_link_timing.py needs a GPU: nothing is measured without one")
    import edge_cases as EC
    import link_cases as LC
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent_commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    prop = torch.cuda.get_device_properties(0)
    say("links across an occluder: awr_detect_hands_edge (edge 40) against awr_detect_hands_link (edge 40, link 40, gap G), %d x %d uint16 frames, K = 2"
        % (FH, FW))
    say("box: one %s (%s, %d CUs), torch %s, HIP %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
                                                       torch.__version__, torch.version.hip))
    say("parent commit: %s (awr_detect_hands_edge issues the launches it issued there: the `edge 40` rows are the yardstick)" % head)
    say("method: HIP events over %d back-to-back calls, %d repetitions after warm-up, the two rows of a pair taken alternately; frames resident "
        "on the device; min_pixels = %d" % (a.inner, a.reps, D.MIN_PIXELS))
    say()
    prims_a, bbox_a, prims_b, bbox_b = EC.overlap_hands()
    fa, fb = (torch.empty((EC.N_OVER, FH, FW), dtype=torch.uint16, device=dev) for _ in range(2))
    synth.render_device(prims_a, bbox_a, fa)
    synth.render_device(prims_b, bbox_b, fb)
    over = store_of(synth.compose(fa, fb))
    apart = store_of(composites(64, False, dev)[2])
    stripes = {g: store_of(torch.from_numpy(LC.stripes((FH, FW), g)).to(dev)[None]) for g in (32, 64)}
    inputs = (("overlapping two-hand composites", over, 32), ("two-hand composites that do not overlap", apart, 32),
              ("stripes of one rear column to 32 front columns (every rear pixel walks 32 occluders both ways)", stripes[32], 32),
              ("stripes of one rear column to 64 front columns (every rear pixel walks 64 occluders both ways)", stripes[64], 64))
    for name, store, gap in inputs:
        say("awr_detect_hands_edge / awr_detect_hands_link on %s" % name)
        knobs = {False: dict(edge=EDGE), True: dict(edge=EDGE, link=LINK, gap=gap)}
        for B in (1, 64):
            idx = torch.arange(B, dtype=torch.int64, device=dev) % store.n
            scratch = torch.empty(int(L.lib.awr_detect_hands_scratch(B, FH, FW)) // 8, dtype=torch.int64, device=dev)
            rows = {False: [], True: []}
            for _ in range(2):                                 # alternately: edge, link, edge, link
                for link in (False, True):
                    rows[link] += event_ms(lambda: D.hands_device(store, idx, 2, scratch=scratch, **knobs[link]), a.inner, a.reps)
            for link in (False, True):
                say("  B = %2d  %-22s %s   = %.3f ms per frame" % (B, "link %g, gap %d" % (LINK, gap) if link else "edge %g" % EDGE, fmt(rows[link]),
                                                                  statistics.median(rows[link]) / B))
            ratio = statistics.median(rows[True]) / statistics.median(rows[False])
            say("  B = %2d  link / edge, ratio of the medians: %.3f%s" % (B, ratio, "   (the link stage costs more than the whole parent call)" if ratio > 2 else ""))
        scratch = torch.empty(int(L.lib.awr_detect_hands_scratch(1, FH, FW)) // 8, dtype=torch.int64, device=dev)
        idx1 = torch.zeros(1, dtype=torch.int64, device=dev)
        kt = kernel_times(lambda: D.hands_device(store, idx1, 2, scratch=scratch, **knobs[True]))
        if kt:
            say("  per kernel at B = 1 with the link (profiler kernel records, median us): "
                + ", ".join("%s %.1f" % (k, v) for k, v in sorted(kt.items(), key=lambda x: -x[1])))
        say()
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    say("Predictor(hands=2, isolate=True, edge_mm=40).predict on the overlapping composites, frames -> joints on the device, without and with link_mm=40 "
        "(link_gap 32), alternately")
    for B in (1, 64):
        frames = over.data.view(torch.int16)[torch.arange(B, device=dev) % over.n].view(torch.uint16)
        preds = {False: awr_amd.Predictor(net, S, 1.0, max_batch=B, hands=2, isolate=True, edge_mm=EDGE),
                 True: awr_amd.Predictor(net, S, 1.0, max_batch=B, hands=2, isolate=True, edge_mm=EDGE, link_mm=LINK)}
        rows = {False: [], True: []}
        inner = max(2, a.inner // (1 if B == 1 else 10))
        for _ in range(2):
            for link in (False, True):
                rows[link] += event_ms(lambda: preds[link].predict(frames), inner, a.reps)
        for link in (False, True):
            say("  max_batch %2d  %-12s %s" % (B, "link_mm=40" if link else "no link", fmt(rows[link])))
        say("  max_batch %2d  link / no link, ratio of the medians: %.3f" % (B, statistics.median(rows[True]) / statistics.median(rows[False])))
        del preds
    say()
    say("the link stage is ONE launch between the tile borders and the flattening; the other nine launches are awr_detect_hands_edge's kernels")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
