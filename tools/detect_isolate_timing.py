"""What a frame per hand (awr_hands_isolate) costs and changes on one MI355X -> profiles/detect_isolate.txt

    python tools/detect_isolate_timing.py [--reps 7] [--inner 20] [--frames 512] [--checkpoint epoch_N.pth] [--out profiles/detect_isolate.txt]

  * awr_hands_isolate alone at K x B = 2 x 1, 2 x 64 and 4 x 64 on two-hand composites, next to awr_detect_hands (with labels) at the same
    B and K, alternately in one run; the bytes it moves ((6 + 2 K) per pixel) and the bandwidth that is, against the HBM roof;
  * Predictor(hands=2) with and without isolate at max_batch 1 and 64, alternately.  The predictor WITHOUT isolate issues the parent
    commit's launches with the parent's arguments (tests/test_predictor_trace_gpu.py holds them to the recorded ones): those rows are the
    parent's, timed in this run;
  * with --checkpoint (a network trained by tools/synth_accuracy.py; ResNet18, img_size 128): the mean joint error on `--frames` near-hand
    composites -- tests/isolate_cases.py's construction with more frames, kept where the two hands are two components that equal their
    own silhouettes -- for hands=2, for hands=2 with isolate, and for a plain predictor on each hand's OWN frame, which is the reference.
Method: tools/predict_timing.py's -- HIP events around `inner` back-to-back calls, `reps` repetitions after a warm-up, median and
min ... max; the arms of a comparison alternate.  No bar is fixed: read an increment against the spread of its rows.  UNMEASURED: real
frames; touching hands (ONE component, ONE hand, with or without isolate); the raw-frame tracker branch of identity + track."""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tools"), os.path.join(REPO, "tests")]
import awr_amd  # noqa: E402
from awr_amd import _lib as L  # noqa: E402
from awr_amd import detect as D  # noqa: E402
from awr_amd import nyu_data as ND  # noqa: E402
from awr_amd import synth  # noqa: E402
from detect_hands_timing import composites, store_of  # noqa: E402
from predict_timing import FH, FW, J, event_ms, fmt  # noqa: E402

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.3          # the spec figure, and what a 16-byte copy kernel reaches on this part
GAP_MM = 130.0


def near_composites(n, dev, seed=31):
    """-> (frames_a, frames_b, composites (n, 480, 640) uint16 on the device, labels_a, labels_b (n, 14, 3) camera mm): two hands without
    forearm, palm points GAP_MM apart sideways at the mean of their depths, v in 200 ... 280, z in 700 ... 900 mm"""
    model = synth.HandModel(forearm=False)
    pa, pb = synth.sample_poses(n, seed, model), synth.sample_poses(n, seed + 1, model)
    rs = np.random.RandomState(seed)
    va, za = 200.0 + 80.0 * rs.uniform(size=n), 700.0 + 200.0 * rs.uniform(size=n)
    vb, zb = 200.0 + 80.0 * rs.uniform(size=n), 700.0 + 200.0 * rs.uniform(size=n)
    half = 0.5 * GAP_MM * ND.PARAS[0] / (0.5 * (za + zb))
    frames, labels = [], []
    for poses, u, v, z in ((pa, 320.0 - half, va, za), (pb, 320.0 + half, vb, zb)):
        joints21, prims, bbox = synth.forward_kinematics(synth.place_poses(poses, u, v, z, model), model)
        f = torch.empty((n, FH, FW), dtype=torch.uint16, device=dev)
        for lo in range(0, n, 256):
            synth.render_device(prims[lo:lo + 256], bbox[lo:lo + 256], f, row=lo, frame0=lo)
        frames.append(f)
        labels.append(synth.labels(joints21, J)[0])
    return frames[0], frames[1], synth.compose(*frames), labels[0], labels[1]


def wide(t):
    return t.view(torch.int16).to(torch.int32) & 0xFFFF


def separable(fa, fb, both, dev, B=64):
    """-> (keep (n,) bool: awr_detect_hands finds exactly two candidates, they hold as many pixels as the hands' own silhouettes and every
    foreground pixel is labelled -- each component IS one hand; a_first (n,) bool: hand a is the nearer one)"""
    n = int(both.shape[0])
    keep, first = [], []
    for lo in range(0, n, B):
        idx = torch.arange(lo, min(n, lo + B), dtype=torch.int64, device=dev)
        _, st, info, count, lab = D.hands_device(store_of(both), idx, 2, labels=True)
        hi = min(n, lo + B)
        a, b, c = wide(fa[lo:hi]), wide(fb[lo:hi]), wide(both[lo:hi])
        na, nb = (a > 0).flatten(1).sum(1), (b > 0).flatten(1).sum(1)
        za = torch.where(a == 0, 1 << 20, a).flatten(1).min(1).values
        zb = torch.where(b == 0, 1 << 20, b).flatten(1).min(1).values
        af = za < zb
        n0, n1 = torch.where(af, na, nb), torch.where(af, nb, na)
        ok = (count == 2) & (st == 0).all(0) & (info[0, :, 2] == n0) & (info[1, :, 2] == n1) & (za != zb)
        ok &= ((lab >= 0) == (c > 0)).flatten(1).all(1) & ((a > 0) & (b > 0)).flatten(1).sum(1).eq(0)
        keep.append(ok)
        first.append(af)
    return torch.cat(keep), torch.cat(first)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--checkpoint", default=None, help="a checkpoint of tools/synth_accuracy.py's train step (ResNet18, 14 joints, img_size 128)")
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "detect_isolate.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/detect_isolate_timing.py needs a GPU: nothing is measured without one")
    import awr_oracle as O
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent_commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    prop = torch.cuda.get_device_properties(0)
    say("a frame per hand (awr_hands_isolate, DESIGN.md 4.28): procedural %d x %d uint16 two-hand composites (awr_amd.synth), ResNet18" % (FH, FW))
    say("box: one %s (%s, %d CUs), torch %s, HIP %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
                                                       torch.__version__, torch.version.hip))
    say("parent commit: %s" % head)
    say("method: HIP events over %d back-to-back calls, %d repetitions after warm-up; frames resident on the device; the arms alternate" % (a.inner, a.reps))
    say("UNMEASURED: real frames; touching hands (ONE component and ONE hand, with or without isolate); the raw-frame tracker branch (identity + track)")
    say()
    _, _, both = composites(64, False, dev)
    two = store_of(both)
    say("awr_hands_isolate alone (one launch) next to awr_detect_hands with labels (nine launches), the same B and K, alternately")
    say("  bytes moved: (2 + 4 + 2 K) per pixel -- the frame and its labels read once, K frames written; HBM roof %.1f TB/s spec, %.1f TB/s for a 16-byte copy"
        % (HBM_SPEC_TBS, HBM_COPY_TBS))
    for K, B in ((2, 1), (2, 64), (4, 64)):
        idx = torch.arange(B, dtype=torch.int64, device=dev)
        scratch = torch.empty(int(L.lib.awr_detect_hands_scratch(B, FH, FW)) // 8, dtype=torch.int64, device=dev)
        labels = torch.empty((B, FH, FW), dtype=torch.int32, device=dev)
        _, _, info, _, _ = D.hands_device(two, idx, K, labels=labels, scratch=scratch)
        out = torch.empty((K * B, FH, FW), dtype=torch.uint16, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        args = (two.data.data_ptr(), 0, two.n, FH, FW, idx.data_ptr(), B, K, labels.data_ptr(), info.data_ptr(), out.data_ptr(), status.data_ptr())
        arms = {"awr_hands_isolate": lambda: L.call("awr_hands_isolate", *args, L.stream()),
                "awr_detect_hands ": lambda: D.hands_device(two, idx, K, labels=labels, scratch=scratch)}
        nbytes = B * FH * FW * (6 + 2 * K)
        for _ in range(2):
            for name, fn in arms.items():
                ms = event_ms(fn, a.inner, a.reps)
                extra = ""
                if name.startswith("awr_hands_isolate"):
                    tbs = nbytes / (statistics.median(ms) * 1e-3) / 1e12
                    extra = "   %.1f MB moved = %.2f TB/s = %.0f %% of the spec roof" % (nbytes / 1e6, tbs, 100 * tbs / HBM_SPEC_TBS)
                say("  K = %d  B = %2d  %s %s%s" % (K, B, name, fmt(ms), extra))
        del out, labels, scratch
    say("  (at B = 1 the %.1f MB of a frame's traffic fit the caches and the time is a launch's: read its rate as a latency, not a bandwidth;"
        % (FH * FW * 10 / 1e6))
    say("   at B = 64 the calls run back to back over the same %.0f MB of frames and labels, which fit the 256 MB last-level cache: the reads are partly"
        % (64 * FH * FW * 6 / 1e6))
    say("   served from it, so these rates are an UPPER reading of what a call on cold inputs reaches; in the predictor the labels were just written)")
    say()
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    say("Predictor.predict, frames -> joints on the device, img_size 64: hands=2 (the parent commit's launches) against hands=2, isolate=True, alternately")
    for B in (1, 64):
        preds = {"hands=2               max_batch %2d" % B: awr_amd.Predictor(net, 64, 1.0, max_batch=B, hands=2),
                 "hands=2, isolate=True  max_batch %2d" % B: awr_amd.Predictor(net, 64, 1.0, max_batch=B, hands=2, isolate=True)}
        for _ in range(2):
            for name, p in preds.items():
                ms = event_ms(lambda: p.predict(both[:B]), a.inner if B == 1 else max(2, a.inner // 4), a.reps)
                say("  %-36s %s" % (name, fmt(ms)))
        del preds
    say()
    del both, two
    if a.checkpoint is None:
        say("joint error on a trained network: not measured in this run (no --checkpoint)")
    else:
        pth = torch.load(a.checkpoint, map_location="cpu", weights_only=False)
        net = awr_amd.get_deconv_net(18, J, 2)
        net.load_state_dict(pth["model"])
        net = net.cuda().eval()
        n, B = a.frames, 64
        fa, fb, both, la, lb = near_composites(n, dev)
        keep, a_first = separable(fa, fb, both, dev)
        sel = torch.nonzero(keep).flatten()
        sel = sel[:(int(sel.numel()) // B) * B]
        say("joint error on a network trained by tools/synth_accuracy.py (%s; trained on single hands WITH a forearm), img_size 128" % os.path.basename(a.checkpoint))
        say("  near-hand composites: palm points %.0f mm apart sideways, no forearm; %d of %d are two components that equal the hands' own silhouettes, %d used"
            % (GAP_MM, int(keep.sum()), n, int(sel.numel())))
        if sel.numel():
            af = a_first[sel].cpu().numpy()
            la, lb = la[sel.cpu().numpy()], lb[sel.cpu().numpy()]
            want = np.stack([np.where(af[:, None, None], la, lb), np.where(af[:, None, None], lb, la)], 1)          # (m, 2, J, 3): the nearer hand first
            ia, ib = fa.view(torch.int16)[sel], fb.view(torch.int16)[sel]          # (uint16 tensors cannot be indexed)
            first = torch.where(a_first[sel, None, None], ia, ib).view(torch.uint16)
            second = torch.where(a_first[sel, None, None], ib, ia).view(torch.uint16)
            comp = both.view(torch.int16)[sel].view(torch.uint16)
            rows = (("hands=2 (raw frames)", awr_amd.Predictor(net, 128, 1.0, max_batch=B, hands=2), None),
                    ("hands=2, isolate=True", awr_amd.Predictor(net, 128, 1.0, max_batch=B, hands=2, isolate=True), None),
                    ("each hand's OWN frame, plain", awr_amd.Predictor(net, 128, 1.0, max_batch=2 * B), (first, second)))
            got = {}
            for name, pred, own in rows:
                xyz, ok = [], []
                for lo in range(0, int(sel.numel()), B):
                    if own is None:
                        out = pred.predict(comp[lo:lo + B])
                        x, s = out.xyz, out.status
                    else:
                        out = pred.predict(torch.cat([own[0][lo:lo + B].view(torch.int16), own[1][lo:lo + B].view(torch.int16)]).view(torch.uint16))
                        x, s = out.xyz.view(2, B, J, 3).transpose(0, 1), out.status.view(2, B).transpose(0, 1)
                    xyz.append(x.cpu().numpy().astype(np.float64))
                    ok.append((s == 0).cpu().numpy())
                xyz, ok = np.concatenate(xyz), np.concatenate(ok)
                e = np.linalg.norm(xyz - want, axis=3)
                ok &= np.isfinite(e).all(2)
                got[name] = xyz
                say("  %-30s mean joint error %8.2f mm, median %8.2f mm over %d hands with status OK (%d not OK)"
                    % (name + ":", float(e[ok].mean()), float(np.median(e[ok])), int(ok.sum()), int((~ok).sum())))
            same = lambda x, y: int(np.all((x == y) | (np.isnan(x) & np.isnan(y)), axis=(2, 3)).sum())
            m = 2 * int(sel.numel())
            say("  hands whose joints equal the own-frame predictor's bit for bit: isolate=True %d of %d, raw frames %d of %d"
                % (same(got["hands=2, isolate=True"], got["each hand's OWN frame, plain"]), m, same(got["hands=2 (raw frames)"], got["each hand's OWN frame, plain"]), m))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
