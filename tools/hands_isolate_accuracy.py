"""Does a frame per hand (Predictor(isolate=True)) keep identities and centres where two hands come close?
-> appended to profiles/detect_isolate.txt

    python tools/hands_isolate_accuracy.py [--seqs 8] [--length 40] [--gaps 260,200,170] [--out profiles/detect_isolate.txt]

tools/hands_identity_accuracy.py's sequences and counting, unchanged (two procedural hands that swap depth order in the middle of every
sequence, where their palm points are `gap` mm apart sideways; a label switch = a hand seen under another label than the last time it was
seen), with two more rows per gap -- `identity, isolate` and `identity, track, isolate` -- next to that tool's own rows from the same
run.  Then, per gap, the CENTRE error: every OK slot of Predictor(hands=2), with and without isolate, against awr_detect's centre on
the OWN frame of the hand it is nearest to (camera millimetres; 0 means the crop stands where the single-hand detector would put it).
An untrained network is enough for both: identities and centres are the detector's.  No bar is fixed; a row that isolation does not help
is reported as it is.  UNMEASURED: real frames; touching hands (ONE component and ONE hand); the raw-frame tracker branch on its own."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tools")]
import awr_amd  # noqa: E402
from awr_amd import detect as D  # noqa: E402
from awr_amd import nyu_data as ND  # noqa: E402
from awr_amd import synth as SY  # noqa: E402
from awr_amd.evaluator import uvd2xyz  # noqa: E402
from hands_identity_accuracy import FH, FW, J, S, run  # noqa: E402


def sequences(n_seq, length, gap_mm, seed):
    """tools/hands_identity_accuracy.py's `sequences`, which also hands back each hand's own frames: -> (composites, gt, (frames_a, frames_b))"""
    model = SY.HandModel(forearm=False)
    f = np.tile(np.arange(length) / float(length - 1), n_seq)
    rs = np.random.RandomState(seed)
    per_seq = lambda lo, hi: np.repeat(rs.uniform(lo, hi, n_seq), length)
    z_a, z_b = 650.0 + 200.0 * f, per_seq(840.0, 860.0) - 200.0 * f
    close = np.sin(np.pi * f)
    half_far, half_near = 150.0, 0.5 * gap_mm * ND.PARAS[0] / 750.0
    half = half_far + (half_near - half_far) * close
    u_a, u_b = 320.0 - half, 320.0 + half
    v_a, v_b = per_seq(220.0, 260.0), per_seq(220.0, 260.0)
    frames, gt = [], []
    for s, (u, v, z) in enumerate(((u_a, v_a, z_a), (u_b, v_b, z_b))):
        poses = SY.place_poses(SY.sample_sequences(n_seq, length, seed + 1 + s, model=model), u, v, z, model)
        _, prims, bbox = SY.forward_kinematics(poses, model)
        out = torch.empty((n_seq * length, FH, FW), dtype=torch.uint16, device="cuda")
        SY.render_device(prims, bbox, out)
        frames.append(out)
        gt.append(np.stack([u, v, z], -1).reshape(n_seq, length, 3))
    return SY.compose(*frames), np.stack(gt, 2), frames


def centre_error(pred, frames, own, gt, B):
    """-> (errors (m,) mm of every OK slot against the own-frame detector centre of the ground-truth hand nearest to it, slots not OK)"""
    import types
    n = int(frames.shape[0])
    gt_xyz = uvd2xyz(gt.reshape(-1, 3).astype(np.float64), ND.PARAS, -1).reshape(n, 2, 3)
    ref = []
    for f in own:
        store = types.SimpleNamespace(data=f, ftype=0, fh=FH, fw=FW, n=n)
        c, st = D.detect_device(store, torch.arange(n, dtype=torch.int64, device=f.device))
        ref.append(np.where((st.cpu().numpy() == 0)[:, None], uvd2xyz(c.cpu().numpy(), ND.PARAS, -1), np.nan))
    ref = np.stack(ref, 1)                                                         # (n, 2, 3)
    err, bad = [], 0
    for lo in range(0, n, B):
        out = pred.predict(frames[lo:lo + B])
        cxyz, status = out.center_xyz.cpu().numpy().astype(np.float64), out.status.cpu().numpy()
        for b in range(cxyz.shape[0]):
            for k in range(2):
                if status[b, k] != 0:
                    bad += 1
                    continue
                h = int(np.argmin(((gt_xyz[lo + b] - cxyz[b, k]) ** 2).sum(-1)))
                err.append(np.linalg.norm(cxyz[b, k] - ref[lo + b, h]))
    return np.asarray(err), bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--length", type=int, default=40)
    ap.add_argument("--gaps", default="260,200,170", help="sideways distances of the palm points at the crossing, mm")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "detect_isolate.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hands_isolate_accuracy.py needs a GPU: nothing is measured without one")
    import awr_oracle as O
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("label switches and centre errors with a frame per hand (DESIGN.md 4.28): procedural two-hand sequences; one %s" % torch.cuda.get_device_name(0))
    say("parent commit: %s" % head)
    say("%d sequences of %d frames per row, tools/hands_identity_accuracy.py's construction and counting; untrained ResNet18 (procedural weights)" % (a.seqs, a.length))
    say("UNMEASURED: real frames, touching hands (ONE component and ONE hand), the raw-frame tracker branch on its own")
    say()
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    kw = dict(max_batch=a.seqs, frame_shape=(FH, FW), hands=2)
    ids = lambda p, o: o.ids
    for gap in (float(g) for g in a.gaps.split(",")):
        frames, gt, own = sequences(a.seqs, a.length, gap, seed=int(gap))
        rows = (("identity=True", dict(identity=True)), ("identity, isolate", dict(identity=True, isolate=True)),
                ("identity=True, track=True", dict(identity=True, track=True)), ("identity, track, isolate", dict(identity=True, track=True, isolate=True)),
                ("identity, track, max_shift=0", dict(identity=True, track=True, max_shift=0.0)),
                ("identity, track, max_shift=0, isolate", dict(identity=True, track=True, max_shift=0.0, isolate=True)))
        say("gap %.0f mm" % gap)
        for name, opt in rows:
            pred = awr_amd.Predictor(net, S, 1.0, **kw, **opt)
            sw, swaps, seen, short, dropped = run(pred, frames, gt, a.seqs, a.length, ids)
            n = a.seqs * a.length
            say("  %-38s label switches %4d (swaps %3d) in %5d hand observations; frames with fewer than two hands %4d of %d (%.1f %%); with a dropped candidate %d"
                % (name + ":", sw, swaps, seen, short, n, 100.0 * short / n, dropped))
            del pred
        for name, opt in (("hands=2", dict()), ("hands=2, isolate=True", dict(isolate=True))):
            pred = awr_amd.Predictor(net, S, 1.0, **kw, **opt)
            e, bad = centre_error(pred, frames, own, gt, a.seqs)
            e = e[np.isfinite(e)]
            say("  %-38s centre against awr_detect on the hand's own frame: equal to 1e-3 mm %5.1f %%, mean %7.2f mm, 95th percentile %7.2f mm, max %7.2f mm over %d slots (%d not OK)"
                % (name + ":", 100.0 * float((e < 1e-3).mean()), float(e.mean()), float(np.percentile(e, 95)), float(e.max()), e.size, bad))
            del pred
        say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
