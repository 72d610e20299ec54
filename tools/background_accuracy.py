"""What the background model (Predictor(background=...)) does to the detector on PROCEDURAL cluttered scenes
-> profiles/background_accuracy.txt

    python tools/background_accuracy.py [--frames 256] [--out profiles/background_accuracy.txt]

The scene: SyntheticFrames hands at 500 ... 900 mm, synth.compose'd with ONE static clutter frame -- a capsule table rendered once by
synth.render_device: a bar across the lower frame at 450 mm (nearer than every hand) and a "torso" capsule at 800 mm (in the middle of the
hands' depth range), in front of a wall (background_mm) -- with noise_mm 0 and 8 on hand and clutter alike.  The model is learnt from 16
hand-free noisy frames of the clutter (awr_background_learn, rank median).  Per noise level:
  * the detector's ("nearest", the Predictor's default seed and refinement) centre against its centre on the clutter-free noise-free
    hand frame, and its status, for: plain | background (margin 30) | background + denoise(radius 1, edge 40, support 3) | hands=2 without
    a model (the better of the two nearest components);
  * per margin 10 / 30 / 60: the share of TRUE hand pixels (visible in the composite) the pass removes, and the share of clutter and wall
    pixels it leaves.
Procedural frames only.  UNMEASURED: real frames (a sensor's noise grows with depth and at edges, and real furniture is not a capsule), and
the joint error of a trained network -- no trained checkpoint exists where this was written."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tools")]
import awr_amd  # noqa: E402, F401
from awr_amd import background as BG  # noqa: E402
from awr_amd import detect as D  # noqa: E402
from awr_amd import nyu_data as ND  # noqa: E402
from awr_amd import synth as SY  # noqa: E402
from denoise_accuracy import render, store_of  # noqa: E402
from hands_overlap_accuracy import FH, FW, wide  # noqa: E402

NOISES, MARGINS = (0, 8), (10.0, 30.0, 60.0)
WALL_MM, BAR_MM, TORSO_MM, N_LEARN = 1500, 450, 800, 16
DENOISE = dict(radius=1, edge=40.0, support=3, fill=None)
CLOSE_PX, CLOSE_MM = 20.0, 40.0          # a centre counts as "on the hand" within these of the reference centre
CLEAR_SHARE = 0.02                       # a frame is "clear" where clutter hides or cuts (at margin 30) at most this share of the hand's pixels


def clutter_prims():
    y = -(440.0 - ND.PARAS[3]) * BAR_MM / ND.PARAS[1]
    prims = np.zeros((1, 2, 8))
    prims[0, 0] = (-400.0, y, BAR_MM, 400.0, y, BAR_MM, 25.0, 0.0)
    prims[0, 1] = (-150.0, 150.0, TORSO_MM, -150.0, -400.0, TORSO_MM, 120.0, 0.0)
    return prims


def clutter(n, noise, seed, dev):
    """n frames of the static clutter in front of the wall, each with its own noise"""
    out = torch.empty((n, FH, FW), dtype=torch.uint16, device=dev)
    box = np.array([[0, 0, FW, FH]] * n, np.int32)
    SY.render_device(np.repeat(clutter_prims(), n, 0), box, out, background_mm=WALL_MM, noise_mm=noise, seed=seed)
    return out


def all_rows(fn, n, dev, chunk=256):
    outs = [fn(torch.arange(lo, min(n, lo + chunk), dtype=torch.int64, device=dev)) for lo in range(0, n, chunk)]
    return tuple(torch.cat([o[i] for o in outs]) for i in range(len(outs[0])))


def masked(frames, model, margin, dev):
    out = torch.empty_like(frames)
    n = int(frames.shape[0])
    all_rows(lambda idx: BG.foreground_device(store_of(frames), idx, model, margin=margin, out=out[int(idx[0]):int(idx[-1]) + 1]), n, dev)
    return out


def denoised(frames, dev):
    out = torch.empty_like(frames)
    n = int(frames.shape[0])
    all_rows(lambda idx: D.denoise_device(store_of(frames), idx, out=out[int(idx[0]):int(idx[-1]) + 1], **DENOISE), n, dev)
    return out


def centres(frames, dev):
    return all_rows(lambda idx: D.detect_device(store_of(frames), idx), int(frames.shape[0]), dev)


def two_hands(frames, dev):
    """hands=2 without a model: the two nearest components' refined centres -> (centres (2, n, 3), status (2, n))"""
    def fn(idx):
        B = int(idx.numel())
        seeds, st, _, _, _ = D.hands_device(store_of(frames), idx, 2)
        c, s = D.detect_device(store_of(frames), idx.repeat(2), seed="given", centers=seeds.view(2 * B, 3))
        return c.view(2, B, 3).transpose(0, 1), s.view(2, B).transpose(0, 1)
    c, s = all_rows(fn, int(frames.shape[0]), dev)
    return c.transpose(0, 1), s.transpose(0, 1)


def row(name, c, s, c0, ok0, clear):
    """clear (n,) bool: the frames whose hand the clutter neither hides nor stands within the margin of (CLEAR_SHARE of its pixels at most)"""
    ok = (s == 0) & ok0
    diff = (c - c0).abs()
    close = ok & (diff[:, 0] <= CLOSE_PX) & (diff[:, 1] <= CLOSE_PX) & (diff[:, 2] <= CLOSE_MM)
    d = diff[close]
    mean = "|du| %5.2f px, |dv| %5.2f px, |dd| %5.2f mm over those" % tuple(float(d[:, i].mean()) for i in range(3)) if bool(close.any()) else "none"
    share = lambda m: 100.0 * float((close & m).sum()) / max(1, int((ok0 & m).sum()))
    return "  %-44s status OK %5.1f %%; centre on the hand: %5.1f %% of all frames, %5.1f %% of the clear ones, %5.1f %% of the others; %s" % (
        name, 100.0 * float((s == 0).double().mean()), share(torch.ones_like(clear)), share(clear), share(~clear), mean)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "background_accuracy.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/background_accuracy.py needs a GPU: the frames are rendered, masked and labelled on the device")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    n = a.frames
    head = a.parent_commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("background model on PROCEDURAL cluttered scenes (awr_background_learn, awr_frames_foreground, DESIGN.md 4.32); one %s" % torch.cuda.get_device_name(0))
    say("parent commit: %s" % head)
    say("%d frames per row, %d x %d: SyntheticFrames hands at 500 ... 900 mm (seed 41, with forearm) composed with ONE static clutter scene -- a bar across"
        % (n, FH, FW))
    say("the lower frame at %d mm, a torso-sized capsule at %d mm left of the centre, a wall at %d mm; the model: the lower median of %d hand-free frames"
        % (BAR_MM, TORSO_MM, WALL_MM, N_LEARN))
    say("with the same noise.  \"on the hand\": status OK and within %.0f px and %.0f mm of the detector's centre on the clutter-free, noise-free hand frame."
        % (CLOSE_PX, CLOSE_MM))
    say("The hands are placed anywhere in the frame, so many stand in front of, behind or next to the clutter; the rows split the frames by that.")
    say("PROCEDURAL ONLY.  UNMEASURED: real frames; the joint error of a trained network (no trained checkpoint exists where this was written)")
    say()
    hands = SY.SyntheticFrames(n, 41, "test", z_range=(500.0, 900.0))
    clean = hands.frame_store.data
    c0, s0 = centres(clean, dev)
    ok0 = s0 == 0
    for noise in NOISES:
        noisy = render(hands.prims, hands.bbox, noise, 5, dev)
        scene = clutter(1, noise, 7, dev)
        frames = SY.compose(noisy, scene.expand(n, FH, FW).contiguous())
        model, st = BG.learn_device(store_of(clutter(N_LEARN, noise, 9, dev)), torch.arange(N_LEARN, dtype=torch.int64, device=dev))
        assert st.tolist() == [0]
        fg = masked(frames, model, 30.0, dev)
        whole = wide(noisy) > 0                                              # the hand as it would be seen without clutter
        gone = whole & (wide(fg) != wide(noisy))                             # hidden behind clutter, or cut by the margin
        clear = gone.sum((1, 2)).double() / whole.sum((1, 2)).clamp(min=1).double() <= CLEAR_SHARE
        say("noise_mm %d: %d of %d frames are clear (clutter hides or cuts at most %.0f %% of the hand's pixels)" % (noise, int(clear.sum()), n, 100 * CLEAR_SHARE))
        say(row("plain (no model)", *centres(frames, dev), c0, ok0, clear))
        say(row("background=True (margin 30)", *centres(fg, dev), c0, ok0, clear))
        say(row("background=True + denoise(1, 40, support 3)", *centres(denoised(fg, dev), dev), c0, ok0, clear))
        c2, s2 = two_hands(frames, dev)
        d2 = (c2 - c0[None]).abs()
        near = (s2 == 0) & (d2[..., 0] <= CLOSE_PX) & (d2[..., 1] <= CLOSE_PX) & (d2[..., 2] <= CLOSE_MM)
        say("  %-44s slot 0 OK %5.1f %%; one of the two centres on the hand: %5.1f %% of all frames, %5.1f %% of the clear ones (which of the two is not known without labels)"
            % ("hands=2, no model", 100.0 * float((s2[0] == 0).double().mean()), 100.0 * float((near.any(0) & ok0).sum()) / max(1, int(ok0.sum())),
               100.0 * float((near.any(0) & ok0 & clear).sum()) / max(1, int((ok0 & clear).sum()))))
        hand = (wide(noisy) > 0) & (wide(frames) == wide(noisy))             # true hand pixels the composite shows
        other = ~hand & (wide(frames) > 0)
        for margin in MARGINS:
            d = wide(masked(frames, model, margin, dev))
            lost = float((hand & (d == 0)).sum()) / float(hand.sum())
            left = float((other & (d > 0)).sum()) / float(other.sum())
            say("  margin %2.0f: %6.3f %% of the true hand pixels removed; %7.4f %% of the clutter and wall pixels left (%.1f per frame)"
                % (margin, 100.0 * lost, 100.0 * left, float((other & (d > 0)).sum()) / n))
        behind = hand & (wide(noisy) + 30 >= wide(model)[None])
        say("  hand pixels less than 30 mm in front of, or behind, the learnt depth at their pixel -- what margin 30 cannot keep: %.3f %% of the hand's pixels"
            % (100.0 * float(behind.sum()) / float(hand.sum())))
        say("  (a hand further than %d mm stands behind the torso's learnt depth where the two overlap in the image, and is cut there)" % (TORSO_MM - 30))
        say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
