"""What the label-free surface check (awr_joints_surface, Predictor(surface=...)) costs on one MI355X -> profiles/surface_check.txt

    python tools/surface_timing.py [--reps 7] [--inner 50] [--out profiles/surface_check.txt]

  * awr_joints_surface alone at K x B = 1 x 1, 1 x 64 and 4 x 64 rows for radius 1 and 3, with the NYU skeleton's 13 bones (3 samples each)
    and without bones, next to awr_joints_filter and awr_confidence_fields at the same rows, alternately in one run.  The joints are the
    true joints of procedural hands over the frames they were rendered into, so every window is read where a hand's joints lie;
  * Predictor.predict with and without surface at max_batch 1 and 64, alternately.  The predictor WITHOUT surface issues the parent
    commit's launches with the parent's arguments (tests/test_predictor_trace_gpu.py holds them to the recorded ones): those rows are the
    parent's predictor, timed in this run.
Method: tools/predict_timing.py's -- HIP events around `inner` back-to-back calls, `reps` repetitions after a warm-up, median and
min ... max; the arms of a comparison alternate and every comparison runs twice.  The three small launches are issued through their
entry points' argument lists on buffers allocated once, so a row is a launch's latency and not a wrapper's allocations.  No bar is fixed:
read an increment against the spread of its rows.  tools/surface_accuracy.py appends what the check says about a trained network.
UNMEASURED: real frames."""
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
from awr_amd import detect_calls as DC  # noqa: E402
from awr_amd import evaluator as EV  # noqa: E402
from awr_amd import nyu_data as ND  # noqa: E402
from awr_amd import surface as SF  # noqa: E402
from awr_amd import synth as SY  # noqa: E402
from awr_amd import track as T  # noqa: E402
from predict_timing import FH, FW, J, event_ms, fmt  # noqa: E402

NF = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "surface_check.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/surface_timing.py needs a GPU: nothing is measured without one")
    import awr_oracle as O
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent_commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    prop = torch.cuda.get_device_properties(0)
    say("label-free surface check (awr_joints_surface, DESIGN.md 4.31): %d x %d uint16 frames, %d joints, ResNet18" % (FH, FW, J))
    say("box: one %s (%s, %d CUs), torch %s, HIP %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
                                                       torch.__version__, torch.version.hip))
    say("parent commit: %s" % head)
    say("method: HIP events over %d back-to-back calls, %d repetitions after warm-up; everything resident on the device; the arms alternate, twice" % (a.inner, a.reps))
    say("UNMEASURED: real frames")
    say()
    # 64 procedural hands on the device and their true joints as uvd
    joints21, prims, bbox = SY.forward_kinematics(SY.sample_poses(NF, 7))
    frames = torch.empty((NF, FH, FW), dtype=torch.uint16, device=dev)
    SY.render_device(prims, bbox, frames)
    lab = SY.labels(joints21, J)[0].astype(np.float32)
    bones = torch.from_numpy(SF.bone_table(None, J)).to(dev)
    cfg = T.check_filter(True)
    say("the three small launches behind the final pass, alone, rows = K x B (hand-major rows over B frames; the true joints of procedural hands):")
    say("awr_joints_surface (in_mm 40, out_mm 15, min_on 1; bones: the NYU skeleton's 13 with 3 samples each, 14 + 39 points a row),")
    say("awr_joints_filter (the defaults) and awr_confidence_fields, one launch each, no allocation in the timed call")
    for K, B in ((1, 1), (1, 64), (4, 64)):
        n = K * B
        rows = np.arange(n) % B
        uvd = torch.from_numpy(EV.xyz2uvd(lab[rows], ND.PARAS, -1)).to(dev)
        xyz = torch.from_numpy(lab[rows]).to(dev)
        idx = torch.from_numpy(rows.astype(np.int64)).to(dev)
        zero = torch.zeros(n, dtype=torch.int32, device=dev)
        out = (torch.empty((n, J), dtype=torch.int32, device=dev), torch.empty((n, J), dtype=torch.float32, device=dev),
               torch.empty((n, 8), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
        state, count = T.filter_state_device(n, J, dev)
        fout = [torch.empty((n, J, 3), dtype=torch.float32, device=dev) for _ in range(3)] + [torch.empty((n, J), dtype=torch.int32, device=dev)]
        conf4, stat = torch.rand((n, J, 4), device=dev), torch.rand((n, J, 2), device=dev)
        cube = torch.full((n, 3), 300.0, device=dev)
        fields = torch.empty((3, n, J), dtype=torch.float32, device=dev)

        def surface(radius, with_bones):
            SF.awr_joints_surface(frames.data_ptr(), 0, NF, FH, FW, idx.data_ptr(), uvd.data_ptr(), zero.data_ptr(), zero.data_ptr(), n, J, n,
                                  bones.data_ptr() if with_bones else None, len(bones) if with_bones else 0, 3, radius, 40.0, 15.0, 1,
                                  *(t.data_ptr() for t in out))
        arms = {"awr_joints_surface r=%d %s" % (r, "13 bones" if wb else "no bones"): (lambda r=r, wb=wb: surface(r, wb)) for r in (1, 3) for wb in (True, False)}
        arms["awr_joints_filter"] = lambda: DC.awr_joints_filter(state.data_ptr(), count.data_ptr(), xyz.data_ptr(), zero.data_ptr(), zero.data_ptr(), None, n, J, n,
                                                                 1.0 / cfg.fps, cfg, ND.PARAS, -1, *(t.data_ptr() for t in fout))
        arms["awr_confidence_fields"] = lambda: DC.awr_confidence_fields(conf4.data_ptr(), stat.data_ptr(), cube.data_ptr(), zero.data_ptr(), zero.data_ptr(), n, J, n,
                                                                         fields[0].data_ptr(), fields[1].data_ptr(), fields[2].data_ptr())
        for _ in range(2):
            for name, fn in arms.items():
                say("  K x B = %d x %2d  %-34s %s" % (K, B, name, fmt(event_ms(fn, a.inner, a.reps))))
        torch.cuda.synchronize()
        c = out[0].cpu().numpy()
        say("  (the codes of these rows, r = 3 without bones: %.1f %% ON, %.1f %% OCCLUDED, %.1f %% OFF)"
            % tuple(100.0 * float((c == k).mean()) for k in (SF.ON, SF.OCCLUDED, SF.OFF)))
        say()
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    say("Predictor.predict, frames -> joints on the device, img_size 64, procedural hands resident on the device: surface=None (the parent commit's")
    say("launches) against surface=True and surface=dict(radius=3, samples=7), alternately")
    med = {}
    for B in (1, 64):
        preds = {"surface=None (the parent's)": awr_amd.Predictor(net, 64, 1.0, max_batch=B),
                 "surface=True": awr_amd.Predictor(net, 64, 1.0, max_batch=B, surface=True),
                 "surface=(r 3, 7 samples)": awr_amd.Predictor(net, 64, 1.0, max_batch=B, surface=dict(radius=3, samples=7))}
        for _ in range(2):
            for name, p in preds.items():
                ms = event_ms(lambda: p.predict(frames[:B]), a.inner if B == 1 else max(2, a.inner // 5), a.reps)
                med[(B, name)] = statistics.median(ms)
                say("  max_batch %2d  %-30s %s" % (B, name, fmt(ms)))
        base = med[(B, "surface=None (the parent's)")]
        say("  max_batch %2d: surface=True is %+.3f ms (%+.2f %%) against the parent's predictor, (r 3, 7 samples) %+.3f ms (%+.2f %%), in the last pass; read it"
            % (B, med[(B, "surface=True")] - base, 100.0 * (med[(B, "surface=True")] / base - 1.0), med[(B, "surface=(r 3, 7 samples)")] - base,
               100.0 * (med[(B, "surface=(r 3, 7 samples)")] / base - 1.0)))
        say("  against the min ... max of the rows above")
        del preds
        say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
