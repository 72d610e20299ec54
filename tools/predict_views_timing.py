"""What test-time views cost on one MI355X, synthetic 480 x 640 frames -> profiles/predict_views.txt

    python tools/predict_views_timing.py [--reps 7] [--inner 20] [--out profiles/predict_views.txt]

The frames, the net and the method are tools/predict_timing.py's: HIP events around `inner` back-to-back calls, `reps` repetitions after a
warm-up that covers plan build and tile autotuning, median and min ... max.  ResNet18, img_size 128, max_batch 1 and 16, V = 2, 4, 8 views:
  * Predictor.predict with views (frames resident on the device -> fused joints), fuse="mean";
  * the baselines, from the same checkout with views=None, measured in the same process right before each view run: the plain predictor
    at max_batch, the plain predictor at max_batch * V (the same plan batch, V times the frames) and recenter=1 at max_batch (the
    existing way to spend a second pass);
  * awr_view_centers, awr_view_rotate and awr_views_fuse alone.
No bar is fixed in advance: the ratios are reported whatever they are.  Whether fusing views lowers the joint error on real frames is not
measured here or anywhere: there are no NYU frames and no trained checkpoint where this runs; the net has procedural weights and the blobs
are synthetic."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tools")]
import awr_amd  # noqa: E402
from awr_amd import detect as D  # noqa: E402
from predict_timing import DET, FH, FW, J, S, event_ms, fmt, synthetic_frames  # noqa: E402

# rotations first (they are the views that add a warp to the renderer), then scales, then a shift
POOL = [dict(rot=15.0), dict(rot=-15.0), dict(scale=1.1), dict(scale=0.9), dict(rot=30.0), dict(rot=-30.0), dict(shift=(0.0, 0.0, 10.0))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "predict_views.txt"))
    a = ap.parse_args()
    import awr_oracle as O
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    say("test-time views: synthetic %d x %d uint16 frames, ResNet18, img_size %d, fuse=\"mean\"" % (FH, FW, S))
    say("box: one %s (%s, %d CUs, %.0f GB), torch %s, HIP %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
                                                             prop.total_memory / 2 ** 30, torch.__version__, torch.version.hip))
    say("method: HIP events over %d back-to-back calls, %d repetitions after warm-up; frames resident on the device; every baseline is built" % (a.inner, a.reps))
    say("from this checkout with views=None and timed in this process")
    say("whether fusing views lowers the joint error on real NYU frames is UNMEASURED: no NYU frames and no trained checkpoint exist on this")
    say("machine; the net has procedural weights and the blobs are synthetic")
    say()
    frames = synthetic_frames(128)
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    kw = dict(frame_shape=(FH, FW), seed="nearest", refine_iters=2, **DET)

    def timed(pred, data):
        ms = event_ms(lambda: pred.predict(data), a.inner, a.reps)
        return statistics.median(ms), ms
    for B in (1, 16):
        data = torch.from_numpy(frames[:B]).to(dev)
        say("max_batch = %d" % B)
        plain, ms = timed(awr_amd.Predictor(net, S, 1.0, max_batch=B, **kw), data)
        say("  plain predictor, %3d frames:                 %s" % (B, fmt(ms)))
        rec, ms = timed(awr_amd.Predictor(net, S, 1.0, max_batch=B, recenter=1, max_shift=1e9, **kw), data)
        say("  recenter=1, %3d frames:                      %s   %+.3f ms: one more pass" % (B, fmt(ms), rec - plain))
        for V in (2, 4, 8):
            wide_data = torch.from_numpy(frames[:B * V]).to(dev)
            wide, ms = timed(awr_amd.Predictor(net, S, 1.0, max_batch=B * V, **kw), wide_data)
            say("  plain predictor, %3d frames (plan batch %3d): %s" % (B * V, B * V, fmt(ms)))
            pred = awr_amd.Predictor(net, S, 1.0, max_batch=B, views=[dict()] + POOL[:V - 1], fuse="mean", **kw)
            views, ms = timed(pred, data)
            say("  V = %d views, %3d frames (plan batch %3d):    %s" % (V, B, B * V, fmt(ms)))
            say("      %+.3f ms over the plain predictor = %.2f of one more pass (recenter=1: %+.3f ms); %.2f x the plain predictor at plan batch %d"
                % (views - plain, (views - plain) / (rec - plain), rec - plain, views / wide, B * V))
            # the three new launches alone, on the last call's buffers
            out = pred.predict(data)
            vo = pred.view_outputs
            st = torch.zeros(B, dtype=torch.int32, device=dev)
            bufs = (pred._vcenters, pred._vcubes, pred._vframe, torch.empty(B * V, dtype=torch.int32, device=dev))
            ms = event_ms(lambda: D.view_centers_device(pred._centers, st, pred._cube, pred._vtable, paras=pred.paras, flip=pred.flip, out=bufs),
                          a.inner, a.reps)
            say("      awr_view_centers alone:                  %s" % fmt(ms))
            M = vo.M.reshape(B * V, 3, 3).clone()
            ms = event_ms(lambda: D.view_rotate_device(pred._blocks, M, bufs[3], pred._vtable), a.inner, a.reps)
            say("      awr_view_rotate alone:                   %s" % fmt(ms))
            xyz, fst, ust = vo.xyz.reshape(V, B, J, 3).contiguous(), vo.status.contiguous(), vo.ustatus.contiguous()
            outs = (torch.empty_like(out.xyz), torch.empty_like(out.uvd), torch.empty_like(out.view_spread_mm), torch.empty_like(out.views_used))
            ms = event_ms(lambda: D.fuse_views_device(xyz, fst, ust, None, "mean", pred.paras, pred.flip, out=outs), a.inner, a.reps)
            say("      awr_views_fuse alone (J = %d):            %s" % (J, fmt(ms)))
            del pred, out, vo
        say()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
