"""What the background model (awr_frames_foreground, awr_background_learn, Predictor(background=...)) costs on one MI355X
-> profiles/background.txt

    python tools/background_timing.py [--reps 7] [--inner 20] [--out profiles/background.txt]

  * awr_frames_foreground alone at B = 1 and 64, 480 x 640: the 16-byte form and the scalar form (the same buffers, the output's base moved
    by one pixel), with and without adapt, next to awr_hands_isolate (K = 2) and awr_frames_denoise (radius 1) at the same B, alternately in
    one run.  The bytes the algorithm needs -- 2 read of the frame, 2 of the model, 2 written, 2 more of the model with adapt -- over the
    call time, next to the HBM figures of the microarchitecture guide;
  * awr_background_learn at n = 8 and n = 64;
  * Predictor.predict with and without background at max_batch 1 and 64, alternately.  The predictor WITHOUT the option issues the parent
    commit's launches with the parent's arguments (tests/test_predictor_trace_gpu.py holds them to the recorded ones): those rows are the
    parent's predictor, timed in this run;
  * registers, LDS and scratch of every kernel form from the compiler's resource report.
Method: tools/predict_timing.py's -- HIP events around `inner` back-to-back calls, `reps` repetitions after a warm-up, median and
min ... max; the arms of a comparison alternate.  No bar is fixed: read an increment against the spread of its rows.  UNMEASURED: real
frames."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tools"), os.path.join(REPO, "tests")]
import awr_amd  # noqa: E402
from awr_amd import background as BG  # noqa: E402
from awr_amd import build as AB  # noqa: E402
from awr_amd import detect as D  # noqa: E402
from detect_hands_timing import composites, store_of  # noqa: E402
from predict_timing import FH, FW, J, event_ms, fmt, synthetic_frames  # noqa: E402

HBM_SPEC_TBS, HBM_COPY_TBS, LLC_MIB = 8.0, 6.29, 256          # the guide's: spec, measured float4 copy, last-level cache


def resources():
    """-> lines: registers, LDS, scratch and occupancy of every kernel of csrc/awr_background.hip, from the compiler's resource report"""
    src = os.path.join(AB.CSRC, "awr_background.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [AB._hipcc(), "-x", "hip", "--offload-arch=" + AB.ARCH, "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", os.path.join(tmp, "bg.o"),
               "-Rpass-analysis=kernel-resource-usage"] + AB.SOURCES["awr_background.hip"]
        text = subprocess.run(cmd, capture_output=True, text=True).stderr
    names = {"ILb1ELb0E": "frames_foreground_kernel<VEC, no adapt>", "ILb1ELb1E": "frames_foreground_kernel<VEC, ADAPT>",
             "ILb0ELb0E": "frames_foreground_kernel<scalar, no adapt>", "ILb0ELb1E": "frames_foreground_kernel<scalar, ADAPT>",
             "background_learn_kernel": "background_learn_kernel"}
    out, cur = [], {}
    for line in text.splitlines():
        m = re.search(r"remark: \s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = {"name": next((v for k, v in names.items() if k in val), val)}
            out.append(cur)
        else:
            cur[key] = val
    return ["  %-44s VGPRs %3s  SGPRs %3s  scratch %s bytes/lane  LDS %5s bytes/block  occupancy %s waves/SIMD"
            % (k["name"], k.get("VGPRs", "?"), k.get("TotalSGPRs", "?"), k.get("ScratchSize", "?"), k.get("LDS Size", "?"), k.get("Occupancy", "?"))
            for k in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "background.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/background_timing.py needs a GPU: nothing is measured without one")
    import awr_oracle as O
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent_commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    prop = torch.cuda.get_device_properties(0)
    say("background model (awr_frames_foreground, awr_background_learn, DESIGN.md 4.32): %d x %d uint16 frames, ResNet18" % (FH, FW))
    say("box: one %s (%s, %d CUs), torch %s, HIP %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
                                                       torch.__version__, torch.version.hip))
    say("parent commit: %s" % head)
    say("method: HIP events over %d back-to-back calls, %d repetitions after warm-up; frames resident on the device; the arms alternate" % (a.inner, a.reps))
    say("UNMEASURED: real frames")
    say()
    say("the compiler's resource report (hipcc -Rpass-analysis=kernel-resource-usage, %s):" % AB.ARCH)
    for line in resources():
        say(line)
    say()
    _, _, hands = composites(64, False, dev)
    wall = torch.from_numpy(synthetic_frames(64)).to(dev)                    # a noisy wall at 1500 ... 1540 mm and a blob at 600 ... 700 mm
    # the model: the wall without the blobs (MAX over 8 frames: the blob sits elsewhere in each), learnt on the device
    model64 = torch.empty((64, FH, FW), dtype=torch.uint16, device=dev)
    BG.learn_device(store_of(wall), torch.arange(8, dtype=torch.int64, device=dev), rank="max", out=model64[0])
    model64[1:].copy_(model64[:1].expand(63, FH, FW))
    pad = torch.empty(64 * FH * FW + 8, dtype=torch.uint16, device=dev)
    say("awr_frames_foreground alone (one launch; margin 30, unknown keep; a model row per batch row) next to awr_hands_isolate (K = 2, one launch)")
    say("and awr_frames_denoise (radius 1, edge 40, one launch), the same B, alternately.  GB/s: the bytes the algorithm needs -- 6 per pixel, 8 with")
    say("adapt -- over the call time; the guide's HBM figures: %.1f TB/s spec, %.2f TB/s measured (float4 copy).  The buffers of a B = 64 call are" % (HBM_SPEC_TBS, HBM_COPY_TBS))
    say("%.0f MiB (frames, model, output): they fit the %d MiB last-level cache, so back-to-back calls over the SAME buffers may be" % (3 * 64 * FH * FW * 2 / 2 ** 20, LLC_MIB))
    say("served from it -- the rate is a call rate over warm buffers, as the neighbours' rows in this table are, not an HBM rate.")
    say("vec: fw % 8 == 0 and 16-byte aligned bases; scalar: the same call with the output's base one pixel further")
    for B in (1, 64):
        idx = torch.arange(B, dtype=torch.int64, device=dev)
        out = torch.empty((B, FH, FW), dtype=torch.uint16, device=dev)
        out_odd = pad[1:1 + B * FH * FW].view(B, FH, FW)
        iso_out = torch.empty((2 * B, FH, FW), dtype=torch.uint16, device=dev)
        two = store_of(hands)
        _, _, info, _, labels = D.hands_device(two, idx, 2, labels=True)
        model = model64[:B]
        arms = {}
        for form, o in (("vec   ", out), ("scalar", out_odd)):
            for adapt in (None, 2):
                arms["awr_frames_foreground %s adapt=%-4s" % (form, adapt)] = (
                    lambda o=o, adapt=adapt: BG.foreground_device(store_of(wall), idx, model, 30.0, "keep", adapt, per_row=True, out=o), 6 if adapt is None else 8)
        arms["awr_hands_isolate K=2 (hands)        "] = (lambda: D.isolate_device(two, idx, labels, info=info, out=iso_out), 0)
        arms["awr_frames_denoise r=1 (wall)        "] = (lambda: D.denoise_device(store_of(wall), idx, 1, 40.0, 0, None, out=out), 0)
        for _ in range(2):
            for name, (fn, nbytes) in arms.items():
                ms = event_ms(fn, a.inner, a.reps)
                extra = ""
                if nbytes:
                    gbs = B * FH * FW * nbytes / (statistics.median(ms) * 1e-3) / 1e9
                    extra = "   %7.1f GB/s = %.1f %% of spec, %.1f %% of the measured copy rate" % (gbs, 0.1 * gbs / HBM_SPEC_TBS, 0.1 * gbs / HBM_COPY_TBS)
                say("  B = %2d  %-38s %s%s" % (B, name, fmt(ms), extra))
        say()
        del out, iso_out, labels
    say("  (times include the wrapper's host work and one small status allocation per call; at B = 1 a call is a launch's latency, not a bandwidth;")
    say("   with adapt=2 the model settles on the frames after a few calls and later calls rewrite the same values: the traffic is the same)")
    say()
    say("awr_background_learn (one launch; once per scene, off the hot path): n frames of the wall -> one model; rank median, min_valid 1")
    m = torch.empty((FH, FW), dtype=torch.uint16, device=dev)
    for _ in range(2):
        for n in (8, 64):
            listed = torch.arange(n, dtype=torch.int64, device=dev)
            ms = event_ms(lambda: BG.learn_device(store_of(wall), listed, out=m), a.inner, a.reps)
            gbs = (n + 1) * FH * FW * 2 / (statistics.median(ms) * 1e-3) / 1e9
            say("  n = %2d  %s   %7.1f GB/s of the (n + 1) x 2 bytes per pixel it reads and writes" % (n, fmt(ms), gbs))
    say()
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    say("Predictor.predict, frames -> joints on the device, img_size 64, wall-and-blob frames on the device, depth_range (200, 1200) for the plain")
    say("predictor as tools/predict_timing.py uses it: no background (the parent commit's launches) against background=True with the learnt wall")
    say("and against background=dict(shared=False, adapt=2), alternately")
    for B in (1, 64):
        kw = dict(max_batch=B, depth_range=(200.0, 1200.0))
        preds = {"background=None (the parent's)          max_batch %2d" % B: awr_amd.Predictor(net, 64, 1.0, **kw),
                 "background=True                         max_batch %2d" % B: awr_amd.Predictor(net, 64, 1.0, background=True, **kw),
                 "background=dict(shared=False, adapt=2)  max_batch %2d" % B: awr_amd.Predictor(net, 64, 1.0, background=dict(shared=False, adapt=2), **kw)}
        for p in list(preds.values())[1:]:
            p.set_background(model64[0])
        for _ in range(2):
            for name, p in preds.items():
                ms = event_ms(lambda: p.predict(wall[:B]), a.inner if B == 1 else max(2, a.inner // 4), a.reps)
                say("  %-54s %s" % (name, fmt(ms)))
        del preds
        say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
