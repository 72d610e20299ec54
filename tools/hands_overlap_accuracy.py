"""What the depth test on the join (Predictor(hands=K, edge_mm=E), awr_detect_hands_edge) finds where two hands OVERLAP in
the image, and what it leaves -> profiles/hands_overlap.txt

    python tools/hands_overlap_accuracy.py [--frames 256] [--offsets 0,40,60,100] [--gaps 80,120,150] [--out profiles/hands_overlap.txt]

Procedural composites, rendered on the device: awr_amd.synth hands without a forearm, poses sample_poses(n, 21) and sample_poses(n, 22);
hand a (the front one) at (u, v, z) = (320 - offset / 2, 240, 700), hand b at (320 + offset / 2, 250, 700 + gap) -- tests/edge_cases.py's
composites are the cell offset 60 px, gap 150 mm.  A cell is a lateral offset and a depth gap; per cell and edge in {None, 20, 40, 80}
(min_pixels = 400, K = 4), over the cell's frames:
  both     the share of frames where slots 0 and 1 are OK and the majority owners of their components differ ("both hands found");
  merged   the share with ONE candidate;   frag   the share with more than two candidates;
  purity   per slot, the mean share of the slot's component that belongs to its majority owner (over the frames where the slot is OK);
  cover    per hand, the mean share of the hand's visible pixels that lie in the component of the slot it owns (over the `both` frames).
Ownership comes from the two hands' own frames: a pixel belongs to the hand whose own frame is nearer there.  Then, once per cell and
edge, the cost of combining edge_mm with isolate: over the `both` frames with more than two candidates, the share of the REAR hand's
visible pixels that are labelled but not in its slot's component -- awr_hands_isolate removes exactly those from that hand's own frame.
No network and no threshold is involved: everything here is the hands stage.  No bar is fixed.  UNMEASURED: real frames, sensor noise
(which decides the right edge), hands with forearms."""
import argparse
import os
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tools")]
import awr_amd  # noqa: E402, F401
from awr_amd import detect as D  # noqa: E402
from awr_amd import synth as SY  # noqa: E402

FH, FW, K, MIN_PIXELS = 480, 640, 4, 400
EDGES = (None, 20.0, 40.0, 80.0)


def wide(t):
    """uint16 depths as int32"""
    return t.view(torch.int16).to(torch.int32) & 0xFFFF


def cell_frames(n, offset, gap, dev):
    """-> (frames_a, frames_b, composites) (n, 480, 640) uint16 on the device"""
    model = SY.HandModel(forearm=False)
    out = []
    for seed, place in ((21, (320.0 - offset / 2.0, 240.0, 700.0)), (22, (320.0 + offset / 2.0, 250.0, 700.0 + gap))):
        poses = SY.place_poses(SY.sample_poses(n, seed, model), *place, model)
        _, prims, bbox = SY.forward_kinematics(poses, model)
        f = torch.empty((n, FH, FW), dtype=torch.uint16, device=dev)
        for lo in range(0, n, 256):
            SY.render_device(prims[lo:lo + 256], bbox[lo:lo + 256], f, row=lo, frame0=lo)
        out.append(f)
    return out[0], out[1], SY.compose(out[0], out[1])


def measure(fa, fb, both, edge):
    """-> dict of the cell's figures at one edge (floats; NaN where no frame qualifies)"""
    import types
    n = int(both.shape[0])
    a, b = wide(fa), wide(fb)
    own_a = (a > 0) & ((b == 0) | (a <= b))
    own_b = (b > 0) & ~own_a
    store = types.SimpleNamespace(data=both, ftype=0, fh=FH, fw=FW, n=n)
    acc = {k: [] for k in ("both", "merged", "frag", "ok0", "ok1", "pur0", "pur1", "cov_a", "cov_b", "lost", "fragboth")}
    for lo in range(0, n, 256):
        idx = torch.arange(lo, min(n, lo + 256), dtype=torch.int64, device=both.device)
        _, status, info, count, labels = D.hands_device(store, idx, K, min_pixels=MIN_PIXELS, labels=True, edge=edge)
        oa, ob = own_a[lo:lo + 256], own_b[lo:lo + 256]
        root = info[:, :, 1] * FW + info[:, :, 0]                                     # (K, B); negative for an EMPTY slot
        na, nb, nn = [], [], []
        for k in range(2):
            mine = labels == root[k][:, None, None]
            na.append((mine & oa).flatten(1).sum(1).double())
            nb.append((mine & ob).flatten(1).sum(1).double())
            nn.append(mine.flatten(1).sum(1).double())
        ok = [(status[k] == 0) for k in range(2)]
        owner_a = [na[k] > nb[k] for k in range(2)]                                  # the slot's majority owner is hand a
        found = ok[0] & ok[1] & (owner_a[0] != owner_a[1])
        acc["both"].append(found.double())
        acc["merged"].append((count == 1).double())
        acc["frag"].append((count > 2).double())
        for k in range(2):
            acc["ok%d" % k].append(ok[k].double())
            acc["pur%d" % k].append(torch.where(ok[k], torch.maximum(na[k], nb[k]) / nn[k].clamp(min=1), torch.zeros_like(nn[k])))
        # the slot each hand owns, where both are found
        in_a = torch.where(owner_a[0], na[0], na[1])
        in_b = torch.where(owner_a[0], nb[1], nb[0])
        vis_a, vis_b = oa.flatten(1).sum(1).double(), ob.flatten(1).sum(1).double()
        acc["cov_a"].append(torch.where(found, in_a / vis_a.clamp(min=1), torch.zeros_like(in_a)))
        acc["cov_b"].append(torch.where(found, in_b / vis_b.clamp(min=1), torch.zeros_like(in_b)))
        # the rear hand (b) fragmented: its visible pixels that are labelled but not in its slot's component are what isolate removes
        root_b = torch.where(owner_a[0], root[1], root[0])
        removed = (ob & (labels >= 0) & (labels != root_b[:, None, None])).flatten(1).sum(1).double()
        fragboth = found & (count > 2)
        acc["fragboth"].append(fragboth.double())
        acc["lost"].append(torch.where(fragboth, removed / vis_b.clamp(min=1), torch.zeros_like(removed)))
    s = {k: float(torch.cat(v).sum()) for k, v in acc.items()}
    nan = float("nan")
    ratio = lambda x, y: x / y if y else nan
    return dict(both=s["both"] / n, merged=s["merged"] / n, frag=s["frag"] / n, pur0=ratio(s["pur0"], s["ok0"]), pur1=ratio(s["pur1"], s["ok1"]),
                cov_a=ratio(s["cov_a"], s["both"]), cov_b=ratio(s["cov_b"], s["both"]), n_frag=int(s["fragboth"]), lost=ratio(s["lost"], s["fragboth"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256, help="composites per cell")
    ap.add_argument("--offsets", default="0,40,60,100", help="lateral offsets of the two palm points, pixels")
    ap.add_argument("--gaps", default="80,120,150", help="depth gaps between the two palm points, mm")
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hands_overlap.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hands_overlap_accuracy.py needs a GPU: the composites are rendered and labelled on the device")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent_commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("overlapping hands and the depth test on the join (DESIGN.md 4.29): procedural two-hand composites; one %s" % torch.cuda.get_device_name(0))
    say("parent commit: %s" % head)
    say("%d composites per cell, %d x %d, rendered on the device; hand a at (320 - offset / 2, 240, 700 mm), hand b at (320 + offset / 2, 250, 700 mm + gap); "
        "K = %d, min_pixels = %d, reach = %g mm" % (a.frames, FH, FW, K, MIN_PIXELS, D.REACH))
    say("both: slots 0 and 1 OK with different majority owners; merged: one candidate; frag: more than two; purity: the majority owner's share of a slot's "
        "component; cover: a hand's visible pixels inside the component of the slot it owns (over the `both` frames)")
    say("UNMEASURED: real frames, sensor noise, forearms.  No bar is fixed; edge None is awr_detect_hands, the parent commit's behaviour")
    say()
    for offset in (float(x) for x in a.offsets.split(",")):
        for gap in (float(x) for x in a.gaps.split(",")):
            fa, fb, both = cell_frames(a.frames, offset, gap, dev)
            overlap = ((wide(fa) > 0) & (wide(fb) > 0)).flatten(1).sum(1)
            say("offset %3.0f px, gap %3.0f mm: silhouettes overlap by %d ... %d pixels (median %d)"
                % (offset, gap, int(overlap.min()), int(overlap.max()), int(overlap.median())))
            cost = []
            for edge in EDGES:
                m = measure(fa, fb, both, edge)
                say("  edge %-4s  both %5.1f %%  merged %5.1f %%  frag %5.1f %%   purity slot 0 %.3f, slot 1 %.3f   cover front %.3f, rear %.3f"
                    % ("None" if edge is None else "%g" % edge, 100 * m["both"], 100 * m["merged"], 100 * m["frag"], m["pur0"], m["pur1"], m["cov_a"], m["cov_b"]))
                if edge is not None:
                    cost.append("edge %g: %d frames, %.1f %% of the rear hand's visible pixels" % (edge, m["n_frag"], 100 * m["lost"]))
            say("  isolate on a fragmented rear hand (both found, more than two candidates) removes from that hand's own frame -- " + "; ".join(cost))
            say()
            del fa, fb, both
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
