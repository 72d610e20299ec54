"""What the depth pre-filter (awr_frames_denoise) does to noisy PROCEDURAL hands -> profiles/denoise_accuracy.txt

    python tools/denoise_accuracy.py [--frames 256] [--out profiles/denoise_accuracy.txt]

Procedural frames only (awr_amd.synth, rendered on the device): there are no real frames where this was written, and the renderer's noise
is independent per pixel, which a real sensor's is not.  Inputs: noise_mm in {0, 4, 8}, as rendered and with 2 % of the hand's pixels
set to 0 (holes) and 0.2 % of all pixels set to a depth of 500 ... 1100 mm (speckles) by `corrupt`, a seeded torch helper.  Filters: none,
denoise=True (1, 40, 0, None) and (2, 40, 6, 18).  Reported per input and filter:
  (1) the RMS depth error on the hand's pixels against the noise-free render (over pixels valid in both), the hand's pixels that are 0
      and the pixels off the hand that are not;
  (2) single hands (with a forearm) through awr_detect_hands_edge at edge_mm in {10, 20, 40}, K = 4, min_pixels = 400: the share of
      frames whose hand is ONE candidate, and the mean number of candidates;
  (3) DESIGN.md 4.29's overlapping composites (offset 60 px, gap 150 mm; tools/hands_overlap_accuracy.py's `measure`): both hands found,
      merged, fragmented, at the same edges;
  (4) the detector's centre (awr_detect, seed nearest, 2 passes) against its centre on the noise-free frame: mean |du, dv| in pixels and
      |dd| in millimetres over the frames where both are OK.
  (5) the joint error of a trained network is NOT measured here: no checkpoint exists where this was written.
A row that the filter makes worse is reported as it is.  No bar is fixed.  UNMEASURED: real frames."""
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
from hands_overlap_accuracy import FH, FW, K, MIN_PIXELS, measure, wide  # noqa: E402

NOISES = (0, 4, 8)
EDGES = (10.0, 20.0, 40.0)
FILTERS = (("none", None), ("(1, 40, 0, None)", dict(radius=1, edge=40.0, support=0, fill=None)), ("(2, 40, 6, 18)", dict(radius=2, edge=40.0, support=6, fill=18)))


def u16(t):
    """int32 depths below 32768 as uint16"""
    return t.to(torch.int16).view(torch.uint16)


def store_of(data):
    import types
    return types.SimpleNamespace(data=data, ftype=0, fh=int(data.shape[1]), fw=int(data.shape[2]), n=int(data.shape[0]))


def corrupt(frames, seed):
    """2 % of the valid pixels -> 0; 0.2 % of all pixels -> a depth of 500 ... 1100 mm.  Seeded, integer operations, not on the hot path."""
    g = torch.Generator(device=frames.device)
    g.manual_seed(seed)
    d = wide(frames)
    r = torch.randint(0, 1000, d.shape, generator=g, device=d.device, dtype=torch.int32)
    d = torch.where((d > 0) & (r < 20), torch.zeros_like(d), d)
    depth = torch.randint(500, 1101, d.shape, generator=g, device=d.device, dtype=torch.int32)
    r = torch.randint(0, 1000, d.shape, generator=g, device=d.device, dtype=torch.int32)
    return u16(torch.where(r < 2, depth, d))


def render(prims, bbox, noise_mm, seed, dev):
    n = len(prims)
    f = torch.empty((n, FH, FW), dtype=torch.uint16, device=dev)
    for lo in range(0, n, 256):
        SY.render_device(prims[lo:lo + 256], bbox[lo:lo + 256], f, row=lo, frame0=lo, noise_mm=noise_mm, seed=seed)
    return f


def filtered(frames, options):
    if options is None:
        return frames
    out = torch.empty_like(frames)
    n = int(frames.shape[0])
    for lo in range(0, n, 256):
        D.denoise_device(store_of(frames), torch.arange(lo, min(n, lo + 256), dtype=torch.int64, device=frames.device), out=out[lo:lo + 256], **options)
    return out


def candidates(frames, edge):
    n = int(frames.shape[0])
    counts = []
    for lo in range(0, n, 256):
        idx = torch.arange(lo, min(n, lo + 256), dtype=torch.int64, device=frames.device)
        counts.append(D.hands_device(store_of(frames), idx, K, min_pixels=MIN_PIXELS, edge=edge)[3])
    c = torch.cat(counts).double()
    return 100.0 * float((c == 1).double().mean()), float(c.mean())


def centres(frames):
    idx = torch.arange(int(frames.shape[0]), dtype=torch.int64, device=frames.device)
    return D.detect_device(store_of(frames), idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise_accuracy.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/denoise_accuracy.py needs a GPU: the frames are rendered, filtered and labelled on the device")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    n = a.frames
    head = a.parent_commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("depth pre-filter on PROCEDURAL hands (awr_frames_denoise, DESIGN.md 4.30); one %s" % torch.cuda.get_device_name(0))
    say("parent commit: %s" % head)
    say("%d frames per row, %d x %d, rendered on the device with per-pixel independent noise; `+hs`: 2 %% of the valid pixels set to 0 and 0.2 %% of all "
        "pixels set to 500 ... 1100 mm.  K = %d, min_pixels = %d" % (n, FH, FW, K, MIN_PIXELS))
    say("UNMEASURED: real frames (a sensor's noise is correlated between neighbours and grows with depth and at edges), the joint error of a trained network")
    say()
    single = SY.HandModel(forearm=True)
    _, sp, sb = SY.forward_kinematics(SY.sample_poses(n, 41, single), single)
    model = SY.HandModel(forearm=False)
    over = []
    for seed, place in ((21, (320.0 - 30.0, 240.0, 700.0)), (22, (320.0 + 30.0, 250.0, 850.0))):
        _, prims, bbox = SY.forward_kinematics(SY.place_poses(SY.sample_poses(n, seed, model), *place, model), model)
        over.append((prims, bbox))
    clean = render(sp, sb, 0, 0, dev)
    c0, s0 = centres(clean)
    own = [render(p, b, 0, 0, dev) for p, b in over]
    hand = wide(clean) > 0
    for noise in NOISES:
        for tag, spoil in (("   ", False), ("+hs", True)):
            noisy = render(sp, sb, noise, 5, dev)
            both = SY.compose(*[render(p, b, noise, 6 + i, dev) for i, (p, b) in enumerate(over)])
            if spoil:
                noisy, both = corrupt(noisy, 100 + noise), corrupt(both, 200 + noise)
            say("noise_mm %d %s" % (noise, tag))
            for name, options in FILTERS:
                f, fo = filtered(noisy, options), filtered(both, options)
                d, ref = wide(f), wide(clean)
                valid = hand & (d > 0)
                rms = float(((d - ref)[valid].double() ** 2).mean().sqrt()) if bool(valid.any()) else float("nan")
                say("  filter %-17s (1) RMS on the hand %6.2f mm; %6.3f %% of the hand's pixels are 0; %6.3f %% of the pixels off the hand are not"
                    % (name, rms, 100.0 * float((hand & (d == 0)).sum()) / float(hand.sum()), 100.0 * float((~hand & (d > 0)).sum()) / float((~hand).sum())))
                row = []
                for edge in EDGES:
                    one, mean = candidates(f, edge)
                    row.append("edge %2.0f: ONE candidate %5.1f %%, mean %.2f" % (edge, one, mean))
                say("  %-24s (2) single hands -- %s" % ("", "; ".join(row)))
                row = []
                for edge in EDGES:
                    m = measure(own[0], own[1], fo, edge)
                    row.append("edge %2.0f: both %5.1f %%, merged %5.1f %%, frag %5.1f %%" % (edge, 100 * m["both"], 100 * m["merged"], 100 * m["frag"]))
                say("  %-24s (3) overlapping -- %s" % ("", "; ".join(row)))
                c, s = centres(f)
                ok = (s == 0) & (s0 == 0)
                diff = (c - c0)[ok].abs()
                say("  %-24s (4) detector centre against the noise-free frame's: |du| %.3f px, |dv| %.3f px, |dd| %.3f mm over %d frames (%d not OK)"
                    % ("", float(diff[:, 0].mean()), float(diff[:, 1].mean()), float(diff[:, 2].mean()), int(ok.sum()), int((~ok).sum())))
            say()
    say("(5) joint error of a trained network: NOT measured (no checkpoint exists where this was written)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
