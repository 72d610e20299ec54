"""What the links across an occluder (Predictor(hands=K, edge_mm=E, link_mm=L), awr_detect_hands_link) repair where a hand in
front cuts a rear hand into fragments, and what they wrongly join -> profiles/hands_link.txt

    python tools/hands_link_accuracy.py [--frames 256] [--offsets 0,40,60,100] [--gaps 80,120,150] [--out profiles/hands_link.txt]

The protocol of tools/hands_overlap_accuracy.py: procedural composites rendered on the device, hand a (the front one) at
(320 - offset / 2, 240, 700), hand b at (320 + offset / 2, 250, 700 + gap); a cell is a lateral offset and a depth gap; edge = 40,
min_pixels = 400, K = 4.  Per cell, without a link and with link = 40 at gap 16, 32 and 64 pixels, over the cell's frames:
  both     the share of frames where slots 0 and 1 are OK and the majority owners of their components differ ("both hands found");
  frag     the share with more than two candidates;   merged   the share with ONE candidate;
  cover    the mean share of the REAR hand's visible pixels inside the component of the slot it owns, and purity, the share of that
           component that is the rear hand's (both over the `both` frames);
  lost     the mean share of the rear hand's visible pixels that are labelled but not in its slot's component -- what awr_hands_isolate
           removes from that hand's own frame (over the `both` frames).
Ownership comes from the hands' own frames: a pixel belongs to the hand whose own frame is nearer there.  Then the cell of the false link:
TWO rear hands side by side at the same depth (850 mm, `--apart` pixels between their palm points) and a front hand (700 mm) between
them; the share of frames in which the two rear hands are ONE component.  No network and no threshold is involved.  No bar is fixed; every
row is printed as it comes out.  UNMEASURED: real frames, sensor noise and shadows (zero pixels break links), hands with forearms."""
import argparse
import os
import subprocess
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tools")]
import awr_amd  # noqa: E402, F401
from awr_amd import detect as D  # noqa: E402
from awr_amd import synth as SY  # noqa: E402
from hands_overlap_accuracy import FH, FW, K, MIN_PIXELS, cell_frames, wide  # noqa: E402

EDGE, LINK, GAPS = 40.0, 40.0, (16, 32, 64)
SETTINGS = ((None, None),) + tuple((LINK, g) for g in GAPS)


def name_of(link, gap):
    return "no link        " if link is None else "link %g, gap %2d" % (link, gap)


def labelled(both, lo, link, gap):
    store = types.SimpleNamespace(data=both, ftype=0, fh=FH, fw=FW, n=int(both.shape[0]))
    idx = torch.arange(lo, min(store.n, lo + 256), dtype=torch.int64, device=both.device)
    _, status, info, count, labels = D.hands_device(store, idx, K, min_pixels=MIN_PIXELS, labels=True, edge=EDGE, link=link, gap=D.LINK_GAP if gap is None else gap)
    return status, info, count, labels


def measure(fa, fb, both, link, gap):
    """-> dict of the cell's figures at one setting (floats; NaN where no frame qualifies)"""
    n = int(both.shape[0])
    a, b = wide(fa), wide(fb)
    own_a = (a > 0) & ((b == 0) | (a <= b))
    own_b = (b > 0) & ~own_a
    acc = {k: [] for k in ("both", "merged", "frag", "cov_b", "pur_b", "lost")}
    for lo in range(0, n, 256):
        status, info, count, labels = labelled(both, lo, link, gap)
        oa, ob = own_a[lo:lo + 256], own_b[lo:lo + 256]
        root = info[:, :, 1] * FW + info[:, :, 0]                                     # (K, B); negative for an EMPTY slot
        na, nb, nn = [], [], []
        for k in range(2):
            mine = labels == root[k][:, None, None]
            na.append((mine & oa).flatten(1).sum(1).double())
            nb.append((mine & ob).flatten(1).sum(1).double())
            nn.append(mine.flatten(1).sum(1).double())
        owner_a = [na[k] > nb[k] for k in range(2)]
        found = (status[0] == 0) & (status[1] == 0) & (owner_a[0] != owner_a[1])
        zero = torch.zeros_like(nn[0])
        acc["both"].append(found.double())
        acc["merged"].append((count == 1).double())
        acc["frag"].append((count > 2).double())
        in_b = torch.where(owner_a[0], nb[1], nb[0])                                  # the rear hand's pixels in the slot it owns
        size_b = torch.where(owner_a[0], nn[1], nn[0])
        vis_b = ob.flatten(1).sum(1).double()
        root_b = torch.where(owner_a[0], root[1], root[0])
        removed = (ob & (labels >= 0) & (labels != root_b[:, None, None])).flatten(1).sum(1).double()
        acc["cov_b"].append(torch.where(found, in_b / vis_b.clamp(min=1), zero))
        acc["pur_b"].append(torch.where(found, in_b / size_b.clamp(min=1), zero))
        acc["lost"].append(torch.where(found, removed / vis_b.clamp(min=1), zero))
    s = {k: float(torch.cat(v).sum()) for k, v in acc.items()}
    ratio = lambda x, y: x / y if y else float("nan")          # noqa: E731
    return dict(both=s["both"] / n, merged=s["merged"] / n, frag=s["frag"] / n, cov_b=ratio(s["cov_b"], s["both"]), pur_b=ratio(s["pur_b"], s["both"]),
                lost=ratio(s["lost"], s["both"]))


def three_hands(n, apart, dev):
    """-> (front, rear left, rear right, composite) (n, 480, 640) uint16: the rear hands at 850 mm, `apart` pixels between their palm points,
    the front hand at 700 mm between them"""
    model = SY.HandModel(forearm=False)
    out = []
    for seed, place in ((21, (320.0, 240.0, 700.0)), (22, (320.0 - apart / 2.0, 250.0, 850.0)), (23, (320.0 + apart / 2.0, 250.0, 850.0))):
        poses = SY.place_poses(SY.sample_poses(n, seed, model), *place, model)
        _, prims, bbox = SY.forward_kinematics(poses, model)
        f = torch.empty((n, FH, FW), dtype=torch.uint16, device=dev)
        for lo in range(0, n, 256):
            SY.render_device(prims[lo:lo + 256], bbox[lo:lo + 256], f, row=lo, frame0=lo)
        out.append(f)
    return out[0], out[1], out[2], SY.compose(out[0], SY.compose(out[1], out[2]))


def false_links(front, left, right, both, link, gap):
    """-> (the share of frames in which the component that holds most of the left rear hand holds most of the right one too, the share of
    frames with exactly three candidates)"""
    n = int(both.shape[0])
    f, l, r = wide(front), wide(left), wide(right)
    vis = lambda x, y, z: (x > 0) & ((y == 0) | (x <= y)) & ((z == 0) | (x <= z))          # noqa: E731
    own_l, own_r = vis(l, f, r), vis(r, f, l) & ~vis(l, f, r)
    same, three = 0.0, 0.0
    for lo in range(0, n, 256):
        _, _, count, labels = labelled(both, lo, link, gap)
        tops = []
        for own in (own_l[lo:lo + 256], own_r[lo:lo + 256]):
            lab = torch.where(own, labels, torch.full_like(labels, -1)).flatten(1)
            top = torch.stack([(row[row >= 0].mode().values if bool((row >= 0).any()) else torch.tensor(-1 - i, device=row.device)) for i, row in enumerate(lab)])
            tops.append(top)
        same += float((tops[0] == tops[1]).double().sum())
        three += float((count == 3).double().sum())
    return same / n, three / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256, help="composites per cell")
    ap.add_argument("--offsets", default="0,40,60,100", help="lateral offsets of the two palm points, pixels")
    ap.add_argument("--gaps", default="80,120,150", help="depth gaps between the two palm points, mm")
    ap.add_argument("--apart", default="120,160,200", help="the false-link cells: pixels between the two rear hands' palm points")
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hands_link.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hands_link_accuracy.py needs a GPU: the composites are rendered and labelled on the device")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent_commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("a rear hand's fragments and the links across the occluder (DESIGN.md 4.33): procedural two-hand composites; one %s" % torch.cuda.get_device_name(0))
    say("parent commit: %s (`no link` is awr_detect_hands_edge, its behaviour)" % head)
    say("%d composites per cell, %d x %d, rendered on the device; hand a at (320 - offset / 2, 240, 700 mm), hand b at (320 + offset / 2, 250, 700 mm + gap); "
        "K = %d, min_pixels = %d, reach = %g mm, edge = %g mm" % (a.frames, FH, FW, K, MIN_PIXELS, D.REACH, EDGE))
    say("both: slots 0 and 1 OK with different majority owners; frag: more than two candidates; merged: one; cover / purity: the rear hand's visible pixels in "
        "the component of the slot it owns, and that component's share that is the rear hand's; lost: the rear hand's visible pixels isolate removes from its "
        "own frame (cover, purity, lost: means over the `both` frames)")
    say("UNMEASURED: real frames, sensor noise and shadows, forearms.  No bar is fixed")
    say()
    for offset in (float(x) for x in a.offsets.split(",")):
        for gap_mm in (float(x) for x in a.gaps.split(",")):
            fa, fb, both = cell_frames(a.frames, offset, gap_mm, dev)
            say("offset %3.0f px, gap %3.0f mm" % (offset, gap_mm))
            for link, gap in SETTINGS:
                m = measure(fa, fb, both, link, gap)
                say("  %s  both %5.1f %%  frag %5.1f %%  merged %5.1f %%   rear slot: cover %.3f, purity %.3f   isolate removes %5.1f %% of the rear hand"
                    % (name_of(link, gap), 100 * m["both"], 100 * m["frag"], 100 * m["merged"], m["cov_b"], m["pur_b"], 100 * m["lost"]))
            say()
            del fa, fb, both
    say("the false link: two rear hands side by side at 850 mm and a front hand at 700 mm between them -- the share of frames in which the two rear hands "
        "are ONE component (and the share with exactly three candidates)")
    for apart in (float(x) for x in a.apart.split(",")):
        front, left, right, both = three_hands(a.frames, apart, dev)
        touch = float((((wide(left) > 0) & (wide(right) > 0)).flatten(1).sum(1) > 0).double().mean())
        say("rear hands %3.0f px apart (their silhouettes overlap in %.1f %% of the frames)" % (apart, 100 * touch))
        for link, gap in SETTINGS:
            same, three = false_links(front, left, right, both, link, gap)
            say("  %s  rear hands in one component %5.1f %%   three candidates %5.1f %%" % (name_of(link, gap), 100 * same, 100 * three))
        say()
        del front, left, right, both
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
