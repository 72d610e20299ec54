"""Do hand identities survive two hands that swap depth order?  -> profiles/hands_identity.txt (the first part; tools/hands_assign_timing.py
appends the timings)

    python tools/hands_identity_accuracy.py [--seqs 8] [--length 40] [--out profiles/hands_identity.txt]

Procedural two-hand sequences (awr_amd.synth: sample_sequences for the articulation, place_poses for the paths, compose for the two hands
in one frame): hand a starts the nearer one on the left, hand b the farther one on the right; over the sequence a recedes and b
approaches, so they cross in depth order around the middle, where they are also closest to each other sideways (--gap mm between the
palm points, about one gate and a bit: nearer and the silhouettes touch and become ONE component).  Every sequence is one batch slot
of Predictor(hands=2, max_batch=seqs) and every call is one frame time.  Per call and sequence each OK slot is given the ground-truth hand
whose palm point (place_poses' (u, v, z), in camera millimetres) is nearest to the slot's crop centre; a hand's LABEL is the slot index for
the plain predictor ("slot = depth rank") and the id for identity=True.  Counted: label switches (a hand seen with another label than the
last time it was seen), and among them SWAPS (the new label is the one the other hand was last seen with: the two hands were taken for
each other; the rest are fresh ids: the identity broke and started again), frames where fewer than two hands are reported (merged into
one component, or missed), frames with a dropped candidate.  An untrained network is enough: identities are decided on the detector's centres.  Joint jitter per identity with smooth= on a
TRAINED network is not measured here."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle")]
import awr_amd  # noqa: E402
from awr_amd import nyu_data as ND  # noqa: E402
from awr_amd import synth as SY  # noqa: E402
from awr_amd.evaluator import uvd2xyz  # noqa: E402

FH, FW, S, J = 480, 640, 64, 14


def sequences(n_seq, length, gap_mm, seed):
    """-> frames (n_seq * length, FH, FW) uint16 on the device, sequence-major, and gt (n_seq, length, 2, 3) palm points in uvd"""
    model = SY.HandModel(forearm=False)
    f = np.tile(np.arange(length) / float(length - 1), n_seq)                     # 0 ... 1 along every sequence
    rs = np.random.RandomState(seed)
    per_seq = lambda lo, hi: np.repeat(rs.uniform(lo, hi, n_seq), length)
    z_a, z_b = 650.0 + 200.0 * f, per_seq(840.0, 860.0) - 200.0 * f               # they cross in depth near f = 0.5
    close = np.sin(np.pi * f)                                                     # 0 at both ends, 1 in the middle
    half_far, half_near = 150.0, 0.5 * gap_mm * ND.PARAS[0] / 750.0               # half the sideways distance in pixels (the gap at 750 mm)
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
    return SY.compose(*frames), np.stack(gt, 2)


def run(pred, frames, gt, n_seq, length, label_of):
    """-> (label switches, swaps among them, hand observations, frames with fewer than two hands, frames with a dropped candidate)"""
    gt_xyz = uvd2xyz(gt.reshape(-1, 3).astype(np.float64), ND.PARAS, -1).reshape(gt.shape)
    last = {}
    switches = swaps = seen = short = dropped = 0
    view = frames.view(n_seq, length, FH, FW)
    for t in range(length):
        out = pred.predict(view[:, t].contiguous())
        cxyz, status, labels = out.center_xyz.cpu().numpy(), out.status.cpu().numpy(), label_of(pred, out).cpu().numpy()
        if getattr(pred, "hands_dropped", None) is not None:
            dropped += int((pred.hands_dropped.cpu().numpy() > 0).sum())
        for s in range(n_seq):
            ok = [k for k in range(2) if status[s, k] == 0]
            short += len(ok) < 2
            for k in ok:
                h = int(np.argmin(((gt_xyz[s, t] - cxyz[s, k]) ** 2).sum(-1)))
                seen += 1
                if (s, h) in last and last[(s, h)] != labels[s, k]:
                    switches += 1
                    swaps += last.get((s, 1 - h)) == labels[s, k]
                last[(s, h)] = labels[s, k]
    return switches, swaps, seen, short, dropped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--length", type=int, default=40)
    ap.add_argument("--gaps", default="260,200,170", help="sideways distances of the palm points at the crossing, mm")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hands_identity.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hands_identity_accuracy.py needs a GPU: nothing is measured without one")
    import awr_oracle as O
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("hand identities across calls (awr_hands_assign, DESIGN.md 4.27): procedural two-hand sequences; one %s" % torch.cuda.get_device_name(0))
    say("parent commit: %s" % head)
    say("%d sequences of %d frames per row; the hands swap depth order in the middle of every sequence, where their palm points are `gap` mm apart sideways"
        % (a.seqs, a.length))
    say("label = slot index (plain: slot = depth rank) or id (identity=True, the defaults: gate 150 mm, merge 60 mm, max_miss 5); a switch = a hand seen "
        "under another label than the last time it was seen, a swap = under the label the OTHER hand was last seen with")
    say("untrained ResNet18 (procedural weights): the assignment reads the detector's centres only, but track=True follows the JOINTS' centre, which is "
        "noise here -- the max_shift=0 row keeps the tracker on the detector's centre instead")
    say("UNMEASURED: real frames, every default, joint "
        "jitter per identity with smooth= on a trained network")
    say()
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=0))
    net = net.cuda().eval()
    kw = dict(max_batch=a.seqs, frame_shape=(FH, FW), hands=2)
    for gap in (float(g) for g in a.gaps.split(",")):
        frames, gt = sequences(a.seqs, a.length, gap, seed=int(gap))
        rows = (("plain (slot = depth rank)", dict(), lambda p, o: torch.arange(2, device=o.status.device).expand_as(o.status)),
                ("identity=True", dict(identity=True), lambda p, o: o.ids),
                ("identity=True, track=True", dict(identity=True, track=True), lambda p, o: o.ids),
                # max_shift=0: no joint centre is ever accepted, so a tracked centre is the detector's own refined one (the joints of an
                # untrained network are noise, and the row above follows them up to half a cube per axis and call)
                ("identity, track, max_shift=0", dict(identity=True, track=True, max_shift=0.0), lambda p, o: o.ids))
        say("gap %.0f mm" % gap)
        for name, opt, label_of in rows:
            pred = awr_amd.Predictor(net, S, 1.0, **kw, **opt)
            sw, swaps, seen, short, dropped = run(pred, frames, gt, a.seqs, a.length, label_of)
            n = a.seqs * a.length
            say("  %-30s label switches %4d (swaps %3d) in %5d hand observations; frames with fewer than two hands %4d of %d (%.1f %%); with a dropped candidate %d"
                % (name + ":", sw, swaps, seen, short, n, 100.0 * short / n, dropped))
            del pred
        say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
