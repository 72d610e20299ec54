"""What the depth test on the join (awr_detect_hands_edge) costs on one MI355X -> profiles/detect_hands_edge.txt

    python tools/detect_hands_edge_timing.py [--reps 9] [--inner 50] [--out profiles/detect_hands_edge.txt]

Two rows per input and batch, taken ALTERNATELY in the same run: `edge None` is awr_detect_hands -- the kernels without the test, whose
instruction streams are the parent commit's -- and `edge 40` (the serpentine: `edge 1`) is awr_detect_hands_edge.  The row `edge None` is
the baseline; the ratio of the medians is stated next to the spread of each row, and no bar is fixed.  Inputs, all 480 x 640 and resident
on the device: the overlapping two-hand composites of tests/edge_cases.py (16 frames, repeated to fill a batch), the two-hand composites
of tools/detect_hands_timing.py that do not overlap, and the serpentine with a depth ramp (one corridor through all 1200 tiles: the worst
case for the joins).  B = 1 and B = 64, K = 2.  Then the time of the tile and the border kernel of both forms from the profiler's kernel
records at B = 1.  Method: tools/predict_timing.py's -- HIP events around `inner` back-to-back calls, `reps` repetitions after a
warm-up, median and min ... max."""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tools"), os.path.join(REPO, "tests")]
import awr_amd  # noqa: E402, F401
from awr_amd import _lib as L  # noqa: E402
from awr_amd import detect as D  # noqa: E402
from awr_amd import synth  # noqa: E402
from detect_hands_timing import composites, kernel_times, store_of  # noqa: E402
from predict_timing import FH, FW, event_ms, fmt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "detect_hands_edge.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/detect_hands_edge_timing.py needs a GPU: nothing is measured without one")
    import edge_cases as EC
    import hands_cases as HC
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent_commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    prop = torch.cuda.get_device_properties(0)
    say("the depth test on the join: awr_detect_hands (edge None) against awr_detect_hands_edge, %d x %d uint16 frames, K = 2" % (FH, FW))
    say("box: one %s (%s, %d CUs), torch %s, HIP %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
                                                       torch.__version__, torch.version.hip))
    say("parent commit: %s (its kernels are the `edge None` rows: the forms without the test compile to the parent's instruction streams)" % head)
    say("method: HIP events over %d back-to-back calls, %d repetitions after warm-up, the two rows of a pair taken alternately; frames resident "
        "on the device; min_pixels = %d" % (a.inner, a.reps, D.MIN_PIXELS))
    say()
    prims_a, bbox_a, prims_b, bbox_b = EC.overlap_hands()
    fa, fb = (torch.empty((EC.N_OVER, FH, FW), dtype=torch.uint16, device=dev) for _ in range(2))
    synth.render_device(prims_a, bbox_a, fa)
    synth.render_device(prims_b, bbox_b, fb)
    over = store_of(synth.compose(fa, fb))
    apart = store_of(composites(64, False, dev)[2])
    serp = store_of(torch.from_numpy(np.array(HC.full_cases()["full_serpentine"]["frame"])).to(dev)[None])
    inputs = (("overlapping two-hand composites", over, 40.0), ("two-hand composites that do not overlap", apart, 40.0),
              ("the serpentine with a depth ramp (one corridor through all 1200 tiles)", serp, 1.0))
    for name, store, edge in inputs:
        say("awr_detect_hands / awr_detect_hands_edge on %s" % name)
        for B in (1, 64):
            idx = torch.arange(B, dtype=torch.int64, device=dev) % store.n
            scratch = torch.empty(int(L.lib.awr_detect_hands_scratch(B, FH, FW)) // 8, dtype=torch.int64, device=dev)
            rows = {None: [], edge: []}
            for _ in range(2):                                 # alternately: none, edge, none, edge
                for e in (None, edge):
                    rows[e] += event_ms(lambda: D.hands_device(store, idx, 2, scratch=scratch, edge=e), a.inner, a.reps)
            for e in (None, edge):
                say("  B = %2d  edge %-5s  %s   = %.3f ms per frame" % (B, "None" if e is None else "%g" % e, fmt(rows[e]), statistics.median(rows[e]) / B))
            say("  B = %2d  edge %g / edge None, ratio of the medians: %.3f" % (B, edge, statistics.median(rows[edge]) / statistics.median(rows[None])))
        scratch = torch.empty(int(L.lib.awr_detect_hands_scratch(1, FH, FW)) // 8, dtype=torch.int64, device=dev)
        idx1 = torch.zeros(1, dtype=torch.int64, device=dev)
        for e in (None, edge):
            kt = kernel_times(lambda: D.hands_device(store, idx1, 2, scratch=scratch, edge=e))
            kt = {k: v for k, v in kt.items() if "tile" in k or "border" in k}
            if kt:
                say("  per kernel at B = 1, edge %s (profiler kernel records, median us): " % ("None" if e is None else "%g" % e)
                    + ", ".join("%s %.1f" % (k, v) for k, v in sorted(kt.items())))
        say()
    say("only the tile and the border stage differ between the two entry points; the other seven launches are the same kernels")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
