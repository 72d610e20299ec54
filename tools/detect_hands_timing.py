"""What several hands per frame (awr_detect_hands) cost and find on one MI355X -> profiles/detect_hands.txt

    python tools/detect_hands_timing.py [--reps 7] [--inner 20] [--frames 2048] [--out profiles/detect_hands.txt]

  * awr_detect (seed "nearest" + 2 refinement passes) and awr_detect_palm at B = 1, the parent commit's entry points, timed in this run:
    every figure below is to be read against them;
  * awr_detect_hands at B = 1, 8 and 64 for K = 2 and 4 on two-hand composites and on the 480 x 640 serpentine (one corridor through all
    1200 tiles: the worst case for the joins), and the time of each of its kernels from the profiler's kernel records at B = 1;
  * Predictor(hands=2) against a plain Predictor at plan batch 2 * max_batch -- the same network rows;
  * on `--frames` device-rendered two-hand composites, with the forearm off and on: the share of frames with both hands found, each
    hand's refined centre against the single detector on that hand's own frame, and what the single detector does on the composites.
The composites are tests/hands_cases.py's construction with more frames: two awr_amd.synth hands placed at u = 150 and u = 490, v in
200 ... 280, z in 700 ... 900 mm, rendered apart on the device and composed.  Method: tools/predict_timing.py's -- HIP events around
`inner` back-to-back calls, `reps` repetitions after a warm-up, median and min ... max.  No bar is fixed.  These are procedural hands:
behaviour on real frames is UNMEASURED, and so are the defaults reach = 300 mm and min_pixels = 400."""
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
from awr_amd import synth  # noqa: E402
from predict_timing import FH, FW, J, S, event_ms, fmt  # noqa: E402


def composites(n, forearm, dev, seed=21):
    """-> (frames_a, frames_b, composites) (n, 480, 640) uint16 on the device: tests/hands_cases.two_hands with n frames"""
    model = synth.HandModel(forearm=forearm)
    pa, pb = synth.sample_poses(n, seed, model), synth.sample_poses(n, seed + 1, model)
    rs = np.random.RandomState(5)
    va, za = 200.0 + 80.0 * rs.uniform(size=n), 700.0 + 200.0 * rs.uniform(size=n)
    vb, zb = 200.0 + 80.0 * rs.uniform(size=n), 700.0 + 200.0 * rs.uniform(size=n)
    out = []
    for poses, u, v, z in ((pa, 150.0, va, za), (pb, 490.0, vb, zb)):
        _, prims, bbox = synth.forward_kinematics(synth.place_poses(poses, u, v, z, model), model)
        f = torch.empty((n, FH, FW), dtype=torch.uint16, device=dev)
        for lo in range(0, n, 256):
            synth.render_device(prims[lo:lo + 256], bbox[lo:lo + 256], f, row=lo, frame0=lo)
        out.append(f)
    return out[0], out[1], synth.compose(out[0], out[1])


def store_of(data):
    import types
    return types.SimpleNamespace(data=data, ftype=0, fh=int(data.shape[1]), fw=int(data.shape[2]), n=int(data.shape[0]))


def kernel_times(fn, calls=20):
    """median microseconds per call of every hands_* kernel, from the profiler's kernel records; {} where it records none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            if "hands_" in e.name:
                name = e.name[e.name.index("hands_"):].split("(")[0].split("E")[0] if e.name.startswith("_Z") else e.name.split("(")[0]
                out.setdefault(name, []).append(float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0)))
        return {k: statistics.median(v) for k, v in out.items()}
    except Exception as e:          # a profiler that cannot record here is no reason to lose the other figures
        print("kernel records unavailable: %r" % (e,), flush=True)
        return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "detect_hands.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/detect_hands_timing.py needs a GPU: nothing is measured without one")
    import awr_oracle as O
    import hands_cases as HC
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent_commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    prop = torch.cuda.get_device_properties(0)
    say("several hands per frame: procedural %d x %d uint16 two-hand composites (awr_amd.synth), ResNet18, img_size %d" % (FH, FW, S))
    say("box: one %s (%s, %d CUs), torch %s, HIP %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
                                                       torch.__version__, torch.version.hip))
    say("parent commit: %s" % head)
    say("method: HIP events over %d back-to-back calls, %d repetitions after warm-up; frames resident on the device" % (a.inner, a.reps))
    say("awr_detect_hands is nine launches; reach = %g mm, slab = %g mm, min_pixels = %d (engineering defaults, UNMEASURED on real frames)"
        % (D.REACH, D.SLAB, D.MIN_PIXELS))
    say()
    fa, fb, both = composites(64, False, dev)
    two = store_of(both)
    serp = store_of(torch.from_numpy(np.array(HC.full_cases()["full_serpentine"]["frame"])).to(dev)[None])
    idx1 = torch.zeros(1, dtype=torch.int64, device=dev)
    c, s = D.detect_device(two, idx1)
    say("the parent commit's entry points on a composite, B = 1, in this run")
    say("  awr_detect, seed \"nearest\" + 2 refinement passes:   %s" % fmt(event_ms(lambda: D.detect_device(two, idx1), a.inner, a.reps)))
    hc, hs, _, _, _ = D.hands_device(two, idx1, 2)
    c1, s1 = D.detect_device(two, idx1, seed="given", centers=hc[0])
    say("  awr_detect_palm on a refined hand centre:           %s" % fmt(event_ms(lambda: D.palm_device(two, idx1, c1, s1), a.inner, a.reps)))
    say()
    for name, store in (("two-hand composites", two), ("the serpentine (one corridor through all 1200 tiles)", serp)):
        say("awr_detect_hands on %s" % name)
        for B in (1, 8, 64):
            idx = torch.arange(B, dtype=torch.int64, device=dev) % store.n
            scratch = torch.empty(int(L.lib.awr_detect_hands_scratch(B, FH, FW)) // 8, dtype=torch.int64, device=dev)
            for K in (2, 4):
                ms = event_ms(lambda: D.hands_device(store, idx, K, scratch=scratch), a.inner, a.reps)
                say("  B = %2d  K = %d   %s   = %.3f ms per frame" % (B, K, fmt(ms), statistics.median(ms) / B))
        scratch = torch.empty(int(L.lib.awr_detect_hands_scratch(1, FH, FW)) // 8, dtype=torch.int64, device=dev)
        kt = kernel_times(lambda: D.hands_device(store, idx1, 2, scratch=scratch))
        if kt:
            say("  per kernel at B = 1, K = 2 (profiler kernel records, median us): " + ", ".join("%s %.1f" % (k, v) for k, v in sorted(kt.items(), key=lambda x: -x[1])))
        say()
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    say("Predictor.predict, frames -> joints on the device: hands=2 at max_batch B against a plain predictor at max_batch 2 B (the same network rows), alternately")
    for B in (1, 8):
        tiled = torch.cat([both[:B].view(torch.int16)] * 2).view(torch.uint16)
        preds = {"hands=2, max_batch %d" % B: (awr_amd.Predictor(net, S, 1.0, max_batch=B, hands=2), both[:B]),
                 "plain,   max_batch %d" % (2 * B): (awr_amd.Predictor(net, S, 1.0, max_batch=2 * B), tiled)}
        for _ in range(2):
            for name, (p, data) in preds.items():
                ms = event_ms(lambda: p.predict(data), a.inner, a.reps)
                say("  %-24s %s" % (name, fmt(ms)))
        del preds
    say()
    del fa, fb, both, two
    n = a.frames
    for forearm in (False, True):
        fa, fb, both = composites(n, forearm, dev)
        sa, sb, sc = store_of(fa), store_of(fb), store_of(both)
        found, err, single = [], [], []
        for lo in range(0, n, 256):
            idx = torch.arange(lo, min(n, lo + 256), dtype=torch.int64, device=dev)
            B = int(idx.numel())
            ca, _ = D.detect_device(sa, idx)
            cb, _ = D.detect_device(sb, idx)
            seeds, st, info, count, _ = D.hands_device(sc, idx, 2)
            c, s = D.detect_device(sc, idx.repeat(2), seed="given", centers=seeds.view(2 * B, 3))
            c, s = c.view(2, B, 3), s.view(2, B)
            both_ok = (s == 0).all(0) & (count >= 2)
            # a hand is matched to the single frame on its side of the image
            left = c[:, :, 0] < FW / 2.0
            want = torch.where(left[:, :, None], ca[None], cb[None])
            d = (c - want)[:, :, :2].norm(dim=2)
            found.append(torch.stack([both_ok, both_ok & (left[0] != left[1]), count > 2]).cpu())
            err.append(d[:, both_ok].flatten().cpu())
            c1, s1 = D.detect_device(sc, idx)
            near = torch.minimum((c1 - ca)[:, :2].norm(dim=1), (c1 - cb)[:, :2].norm(dim=1))
            single.append(torch.stack([(s1 != 0).float(), ((s1 == 0) & (near < 1.0)).float(), ((s1 == 0) & (near >= 1.0)).float()]).cpu())
        found, err, single = torch.cat(found, 1).float().mean(1), torch.cat(err), torch.cat(single, 1).mean(1)
        say("%d composites, forearm %s" % (n, "on" if forearm else "off"))
        say("  both slots OK and count >= 2: %.1f %% of the frames; one on each side of the image: %.1f %%; more than two candidates: %.1f %%"
            % (100 * found[0], 100 * found[1], 100 * found[2]))
        if err.numel():
            say("  refined centre of a found hand against awr_detect on that hand's own frame, image plane: equal bit for bit %.1f %%, median %.3f px, "
                "95th percentile %.3f px, max %.3f px" % (100 * float((err == 0).float().mean()), float(err.median()), float(err.quantile(0.95)), float(err.max())))
        say("  the single detector (awr_detect, seed \"nearest\") on the composites: EMPTY %.1f %%, within 1 px of one hand's own centre %.1f %%, "
            "elsewhere %.1f %%; it never reports a second hand" % (100 * single[0], 100 * single[1], 100 * single[2]))
        say()
        del fa, fb, both, sa, sb, sc
    say("without the depth test on the join (edge, DESIGN.md 4.29) touching or overlapping hands form ONE component and count as one hand; identity of a hand across calls is not tracked")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
