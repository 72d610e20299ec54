"""What prediction from raw frames costs on one MI355X, synthetic 480 x 640 frames -> profiles/predict.txt

    python tools/predict_timing.py [--reps 7] [--inner 20] [--out profiles/predict.txt]

  * the detector alone (awr_detect: seed "nearest" + 2 refinement passes, and the seed passes alone) at B = 1 and B = 64: time per call,
    time per full-frame pass, GB/s against the frame bytes each full-frame pass reads;
  * frames resident on the device -> joints (Predictor.predict, ResNet18, img_size 128), B = 1 and B = 64, everything on the device;
  * the same pipeline with the host doing the glue: detect.detect in numpy on frames downloaded from the device, set_crop blocks uploaded,
    predictions downloaded and un-projected with EvalUtil's arithmetic.
Method: every figure is a HIP-event (device pipelines) or perf_counter-around-a-sync (host-glue pipeline) time of `inner` back-to-back calls,
repeated `reps` times after a warm-up that covers plan build and tile autotuning; median and min ... max over the repetitions are reported."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle")]
import awr_amd  # noqa: E402
from awr_amd import detect as D  # noqa: E402
from awr_amd import nyu_data as ND  # noqa: E402
from awr_amd import nyu_device as DV  # noqa: E402
from awr_amd.evaluator import uvd2xyz  # noqa: E402

FH, FW, S, J = 480, 640, 128, 14
DET = dict(depth_range=(200.0, 1200.0), slab=150.0)


def synthetic_frames(n, seed=0):
    """a noisy far wall and a hand-sized blob (about 150 x 150 pixels at 600 ... 700 mm) at a random place per frame"""
    r = np.random.RandomState(seed)
    f = (1500 + r.randint(0, 40, (n, FH, FW))).astype(np.uint16)
    vv, uu = np.mgrid[0:FH, 0:FW]
    for b in range(n):
        cu, cv = r.randint(150, FW - 150), r.randint(120, FH - 120)
        m = (uu - cu) ** 2 + (vv - cv) ** 2 <= 75 ** 2
        f[b][m] = (600 + r.randint(0, 100, int(m.sum()))).astype(np.uint16)
    return f


def event_ms(fn, inner, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return out


def wall_ms(fn, inner, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / inner)
    return out


def fmt(ms):
    return "median %9.3f ms   (min %9.3f ... max %9.3f over %d repetitions)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def host_glue_predict(store, engine, frames_dev, B):
    """frames on the device -> joints with the glue on the host: two syncs (frames down, predictions down)"""
    frames = frames_dev.cpu().numpy()
    cs = np.array([D.detect(f, seed="nearest", iters=2, **DET)[0] for f in frames])
    blocks, M, cxyz, cube, _ = D.sample_blocks(cs, (300, 300, 300), S, frame_shape=(FH, FW))
    img = store.render(DV.blocks_to_tensor(blocks))
    jt = engine(img).cpu().numpy()
    jt[:, :, :2] = (jt[:, :, :2] + 1) * S / 2.0                                     # EvalUtil.feed_batch, eval_tool.py:38-41
    jt[:, :, 2] = jt[:, :, 2] * cube[:, None, 2] / 2.0 + cxyz[:, None, 2]
    hom = np.concatenate([jt[:, :, :2], np.ones(jt.shape[:2] + (1,), np.float64)], -1)
    jt[:, :, :2] = np.einsum("bij,bkj->bki", np.linalg.inv(M).astype(np.float64), hom)[:, :, :2]
    return jt, uvd2xyz(jt, ND.PARAS, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "predict.txt"))
    a = ap.parse_args()
    import awr_oracle as O
    from awr_amd.trainer import InferEngine
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("prediction from raw frames: synthetic %d x %d uint16 frames, ResNet18, img_size %d, one %s" % (FH, FW, S, torch.cuda.get_device_name(0)))
    say("parent commit: %s" % head)
    say("method: HIP events (device pipelines) / perf_counter around a sync (host glue) over %d back-to-back calls, %d repetitions after warm-up" % (a.inner, a.reps))
    say("detection quality on real NYU frames is NOT measured here: no NYU frames exist on this machine; the blobs are synthetic")
    say()
    frames = synthetic_frames(64)
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    for B in (1, 64):
        data = torch.from_numpy(frames[:B]).to(dev)
        store = DV.FrameStore.__new__(DV.FrameStore)
        store.data, store.ftype, store.n, store.fh, store.fw = data, 0, B, FH, FW
        idx = torch.arange(B, dtype=torch.int64, device=dev)
        nbytes = B * FH * FW * 2
        say("B = %d" % B)
        # detector alone
        for name, kw, full in (("seed \"nearest\" + 2 refinement passes", dict(seed="nearest", iters=2), 2),
                               ("seed \"nearest\" alone (2 full-frame passes)", dict(seed="nearest", iters=0), 2),
                               ("seed \"range\" alone (1 full-frame pass)", dict(seed="range", iters=0), 1)):
            ms = event_ms(lambda: D.detect_device(store, idx, **kw, **DET), a.inner, a.reps)
            say("  awr_detect, %-44s %s" % (name + ":", fmt(ms)))
            if kw["iters"] == 0:
                m = statistics.median(ms)
                say("      -> %.3f ms per full-frame pass, %.1f GB/s against the %.2f MB a pass reads (init + finalize launches included)"
                    % (m / full, full * nbytes / (m * 1e-3) / 1e9, nbytes / 1e6))
        # frames -> joints, all on the device
        pred = awr_amd.Predictor(net, S, 1.0, max_batch=B, frame_shape=(FH, FW), seed="nearest", refine_iters=2, **DET)
        ms = event_ms(lambda: pred.predict(data), a.inner, a.reps)
        pred.check()
        say("  frames -> joints on the device (Predictor.predict):       %s   = %.1f frames/s" % (fmt(ms), B / (statistics.median(ms) * 1e-3)))
        # the same with the host doing the glue
        engine = InferEngine(net, B, S, 1.0)
        store.render = DV.Renderer(store, S, B)
        ms_h = wall_ms(lambda: host_glue_predict(store, engine, data, B), max(2, a.inner // 4), a.reps)
        say("  frames -> joints, glue on the host (numpy detect, set_crop): %s   = %.1f frames/s" % (fmt(ms_h), B / (statistics.median(ms_h) * 1e-3)))
        ms_w = wall_ms(lambda: pred.predict(data), a.inner, a.reps)
        say("  Predictor.predict, wall clock around a sync (same clock as the host-glue line): %s" % fmt(ms_w))
        say()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
