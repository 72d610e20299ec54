"""Joints from raw depth frames, no dataset needed:

    python predict.py FRAMES.npy --load-model X.pth [--net resnet_18] [--set key=value ...]

FRAMES.npy holds (n, h, w) uint16 depth frames in millimetres.  Writes pred_uvd.txt (original-image uvd, "%.3f", J * 3 columns: the format
of the reference's results file, test.py:105-108) and pred_xyz.txt (camera millimetres) into --out (default: the current directory).
--confidence adds pred_conf.txt, pred_peak.txt and pred_spread_mm.txt (J columns each: the expected closeness under the head's weights, the
largest masked heat value, the vote scatter in nominal millimetres).
--recenter N crops again around the predicted joints and predicts again, N times; --track treats the file as ONE sequence (batch size 1, so
batch slot 0 is the stream) and starts each frame's crop at the previous frame's joint centre, falling back to the detector when the hand is
lost.  With either, pred_center_uvd.txt (the final crop centres) and pred_recenter_code.txt (one column per
awr_joints_center call: 1 = moved, 0 / 2 / 3 / 4 = kept, awr_amd.detect.RECENTER_NAMES) are written too.
--views "rot=-15,15;scale=0.9,1.1;shift=0:0:10" predicts every frame from several views in one pass -- the identity, then one view per
in-plane rotation (degrees), per cube scale and per centre shift (x:y:z camera millimetres) -- and fuses their joints with --fuse mean |
conf | median; pred_uvd.txt / pred_xyz.txt then hold the fused joints, and pred_view_spread_mm.txt and pred_views_used.txt
(J columns each) are written too.
--palm sends the detector's centres through awr_detect_palm first: the centre of the palm disc of the silhouette's exact distance transform,
which a forearm at the hand's depth does not drag up the arm (measured on procedural hands only).
--smooth [MIN_CUTOFF,BETA,D_CUTOFF] puts the temporal joint filter behind the joints (a One-Euro low-pass per joint with coasting over lost
frames; defaults 1.0,0.02,1.0 in Hz, 1/mm, Hz): like --track it treats the file as ONE sequence (batch size 1) at --fps F
(default 30); --gate-mm G ignores a measurement further than G mm from the filtered joint; --lead (with --track) starts the next frame's crop
at the constant-velocity look-ahead of the joints.  pred_uvd.txt / pred_xyz.txt then hold the FILTERED joints, and pred_raw_uvd.txt,
pred_raw_xyz.txt (the network's own) and pred_filter_code.txt (J columns, awr_amd.track.FILTER_NAMES) are written too.
--hands K (2 ... 4) looks for up to K hands per frame: awr_detect_hands splits the near foreground into connected components and seeds the K
nearest large ones (--reach MM: how far behind the nearest pixel that foreground goes, default 300; --min-pixels N: the smallest component
that counts, default 400; DESIGN.md 4.26 -- both UNMEASURED on real frames; without --edge-mm touching or overlapping hands are one hand).  The saved arrays gain the hand
axis: pred_uvd.txt / pred_xyz.txt hold n * K rows (frame-major, the nearest hand first; an absent hand's row is nan), and pred_n_hands.txt
(one count per frame), pred_hand_status.txt (K columns, awr_amd.detect's codes) and pred_hand_info.txt (n * K rows: the component's first
pixel u, v, its pixels, its nearest depth) are written too.  Not combined with --views, --track or --smooth yet -- unless:
--identity [GATE_MM,MERGE_MM,MAX_MISS] (with --hands K) keeps every hand in ITS slot from frame to frame (awr_hands_assign, an exact
assignment of each frame's detected hands to the previous frame's; defaults 150,60,5, UNMEASURED on real frames): the file
is ONE sequence (batch size 1), --track and --smooth then work per hand, and pred_hand_id.txt (K columns, 0: a free slot) and
pred_hand_code.txt (K columns, awr_amd.track.ASSIGN_NAMES) are written too; pred_hand_info.txt stays in detection order.
--isolate (with --hands K) gives every hand a frame that holds only its own connected component before the refinement, the palm pass and
the crop (awr_hands_isolate): two hands nearer than half a crop cube no longer stand in each other's crop.  Touching hands
remain one component and one hand unless --edge-mm separates them; UNMEASURED on real frames.
--edge-mm E (with --hands K) joins two neighbouring pixels of the near foreground only when their depths differ by at most E millimetres
(awr_detect_hands_edge): a hand held in front of another one becomes a component of its own.  Hands that touch in depth
stay one hand, and a rear hand that the front one cuts into pieces gives one candidate per piece of --min-pixels or more
(profiles/hands_overlap.txt).  There is no default: the right E depends on the sensor's noise, UNMEASURED on real frames.
--link-mm L [--link-gap G] (with --hands K --edge-mm E) joins those pieces again (awr_detect_hands_link): a pixel beside
1 ... G pixels that are more than E millimetres nearer is joined with the first pixel behind them when the two depths differ by at most L
millimetres.  G is 32 unless given, 64 at the most.  A zero pixel in the gap breaks the link, and two different hands at similar depth
behind one narrow nearer object are linked (profiles/hands_link.txt).  No default for L; UNMEASURED on real frames.
--denoise [RADIUS,EDGE,SUPPORT,FILL] filters every frame on the device before anything else reads it (awr_frames_denoise):
per pixel the lower median of the window's valid depths within EDGE millimetres of its own; a pixel with fewer than SUPPORT such
neighbours becomes 0; a zero pixel with at least FILL valid neighbours takes their lower median.  Without a value: 1,40,0,none (a 3 x 3
edge-preserving median); EDGE and FILL may be "none".  Combines with every other option; the defaults are UNMEASURED on real frames.
--surface [RADIUS,IN_MM,OUT_MM] checks every predicted joint against the depth frame it was predicted from (awr_joints_surface, DESIGN.md
4.31): ON (0) where a valid pixel of the (2 RADIUS + 1)^2 window around the joint's pixel lies at most IN_MM in front of the joint and at
most OUT_MM behind it, OCCLUDED (1) where something much nearer covers the pixel, OFF (2) where only background or nothing is there,
OUTSIDE (3) off the frame, SKIPPED (4) for a frame or hand without a prediction.  Without a value: 1,40,15.  Writes pred_surface_code.txt
and pred_surface_gap_mm.txt (a row per frame and hand, a column per joint) and pred_surface_counts.txt (joints ON / OCCLUDED / OFF /
OUTSIDE, then the same for three samples along each bone of the skeleton).  It needs no labels; it changes no prediction.  Combines with
every other option; the defaults are engineering choices, UNMEASURED on real frames.
--background EMPTY.npy learns a static-scene background model from the (n, h, w) uint16 frames of EMPTY.npy (1 ... 64 frames of the scene
WITHOUT a hand, as many as 64 are used) before the first prediction, and every frame then reaches the detector without it
(awr_background_learn, awr_frames_foreground): a pixel stays where it is at least --background-margin MM (default 30)
nearer than the learnt depth, or where no background was ever seen.  For a FIXED sensor with a table edge, a monitor or a body nearer
than the hand.  --background-adapt STEP treats the file as one sequence and lets the model follow the background STEP millimetres per
frame.  Combines with every other option; the defaults are engineering choices, UNMEASURED on real frames.
--ema predicts with the checkpoint's averaged weights ("model_ema", written by a run with config.ema_decay) instead of "model".
`--set` overrides config entries as train.py does (img_size, kernel_size, cube, batch_size, jt_num, downsample, winograd ...)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("frames")
    ap.add_argument("--load-model", required=True)
    ap.add_argument("--net", default=None)
    ap.add_argument("--out", default=".")
    ap.add_argument("--set", nargs="*", default=[], metavar="key=value")
    ap.add_argument("--confidence", action="store_true", help="also write per-joint conf / peak / spread_mm")
    ap.add_argument("--recenter", type=int, default=0, metavar="N", help="extra passes cropped around the predicted joints (0 ... 4)")
    ap.add_argument("--track", action="store_true", help="the file is one sequence: start each crop at the previous frame's joint centre")
    ap.add_argument("--views", default=None, metavar="SPEC", help="test-time views, e.g. \"rot=-15,15;scale=0.9,1.1;shift=0:0:10\" (the identity view comes first by itself)")
    ap.add_argument("--fuse", default="mean", choices=("mean", "conf", "median"), help="how the views' joints are fused (with --views)")
    ap.add_argument("--palm", action="store_true", help="move each detector centre to the palm disc of the silhouette's distance transform")
    ap.add_argument("--smooth", nargs="?", const="", default=None, metavar="MIN_CUTOFF,BETA,D_CUTOFF",
                    help="filter the joints over time (the file is one sequence); optionally the One-Euro constants in Hz, 1/mm, Hz")
    ap.add_argument("--fps", type=float, default=None, metavar="F", help="frame rate of the sequence (with --smooth; default 30)")
    ap.add_argument("--gate-mm", type=float, default=None, metavar="G", help="with --smooth: ignore a measurement further than G mm from the filtered joint")
    ap.add_argument("--lead", action="store_true", help="with --smooth and --track: crop the next frame at the look-ahead joints")
    ap.add_argument("--hands", type=int, default=1, metavar="K", help="look for up to K hands per frame (1 ... 4); the outputs gain a hand axis")
    ap.add_argument("--reach", type=float, default=None, metavar="MM", help="with --hands: depth of the foreground behind the nearest pixel (default 300)")
    ap.add_argument("--min-pixels", type=int, default=None, metavar="N", help="with --hands: the smallest component that counts as a hand (default 400)")
    ap.add_argument("--isolate", action="store_true", help="with --hands: refine and crop every hand on a frame that holds only its own component")
    ap.add_argument("--edge-mm", type=float, default=None, metavar="E", help="with --hands: join neighbouring foreground pixels only within E mm of depth, so a hand in front of another one splits off")
    ap.add_argument("--link-mm", type=float, default=None, metavar="L", help="with --hands and --edge-mm: rejoin the pieces a nearer hand cuts a rear hand into, where their depths agree within L mm")
    ap.add_argument("--link-gap", type=int, default=None, metavar="G", help="with --link-mm: the widest occluder, in pixels, a link crosses (default 32, at most 64)")
    ap.add_argument("--identity", nargs="?", const="", default=None, metavar="GATE_MM,MERGE_MM,MAX_MISS",
                    help="with --hands: keep each hand in its slot across frames (the file is one sequence); optionally the gate, the merge distance and the misses allowed")
    ap.add_argument("--denoise", nargs="?", const="", default=None, metavar="RADIUS,EDGE,SUPPORT,FILL",
                    help="filter every frame on the device first: edge-preserving median, speckle removal, hole filling (default 1,40,0,none)")
    ap.add_argument("--surface", nargs="?", const="", default=None, metavar="RADIUS,IN_MM,OUT_MM",
                    help="check every predicted joint against the depth frame: on the seen surface, occluded or off it (default 1,40,15)")
    ap.add_argument("--background", default=None, metavar="EMPTY.npy",
                    help="learn a background model from these frames of the empty scene first; only what is nearer than it is looked at")
    ap.add_argument("--background-margin", type=float, default=None, metavar="MM", help="with --background: how much nearer than the model a pixel must be (default 30)")
    ap.add_argument("--background-adapt", type=int, default=None, metavar="STEP", help="with --background: the file is one sequence; the model follows the background STEP mm per frame")
    ap.add_argument("--ema", action="store_true", help="load the checkpoint's \"model_ema\" (the EMA of the weights) instead of \"model\"")
    return ap.parse_args(argv)


def denoise_config(args):
    """--denoise -> what Predictor(denoise=...) takes, or None"""
    if args.denoise is None:
        return None
    if not args.denoise:
        return True
    vals = [v.strip().lower() for v in args.denoise.split(",")]
    try:
        if len(vals) != 4:
            raise ValueError
        return dict(radius=int(vals[0]), edge=None if vals[1] == "none" else float(vals[1]), support=int(vals[2]),
                    fill=None if vals[3] == "none" else int(vals[3]))
    except ValueError:
        raise SystemExit("--denoise takes RADIUS,EDGE,SUPPORT,FILL (an int, a number or none, an int, an int or none), not %r" % args.denoise)


def background_config(args):
    """--background / --background-margin / --background-adapt -> what Predictor(background=...) takes, or None"""
    if args.background is None:
        if args.background_margin is not None or args.background_adapt is not None:
            raise SystemExit("--background-margin and --background-adapt belong to --background EMPTY.npy")
        return None
    cfg = {}
    if args.background_margin is not None:
        cfg["margin"] = args.background_margin
    if args.background_adapt is not None:
        cfg["adapt"] = args.background_adapt
    return cfg or True


def surface_config(args):
    """--surface -> what Predictor(surface=...) takes, or None"""
    if args.surface is None:
        return None
    if not args.surface:
        return True
    vals = [v.strip() for v in args.surface.split(",")]
    try:
        if len(vals) != 3:
            raise ValueError
        return dict(radius=int(vals[0]), in_mm=float(vals[1]), out_mm=float(vals[2]))
    except ValueError:
        raise SystemExit("--surface takes RADIUS,IN_MM,OUT_MM (an int and two numbers), not %r" % args.surface)


def smooth_config(args):
    """--smooth / --fps / --gate-mm / --lead -> the dict Predictor(smooth=...) takes, or None"""
    if args.smooth is None:
        if args.fps is not None or args.gate_mm is not None or args.lead:
            raise SystemExit("--fps, --gate-mm and --lead belong to --smooth")
        return None
    cfg = {}
    if args.smooth:
        try:
            vals = [float(v) for v in args.smooth.split(",")]
        except ValueError:
            vals = []
        if len(vals) != 3:
            raise SystemExit("--smooth takes MIN_CUTOFF,BETA,D_CUTOFF (three numbers), not %r" % args.smooth)
        cfg.update(min_cutoff=vals[0], beta=vals[1], d_cutoff=vals[2])
    if args.fps is not None:
        cfg["fps"] = args.fps
    if args.gate_mm is not None:
        cfg["gate_mm"] = args.gate_mm
    if args.lead:
        cfg["lead"] = True
    return cfg


def identity_config(args):
    """--identity -> what Predictor(identity=...) takes, or None"""
    if args.identity is None:
        return None
    if args.hands < 2:
        raise SystemExit("--identity belongs to --hands K with K >= 2")
    if not args.identity:
        return True
    vals = args.identity.split(",")
    try:
        return dict(gate_mm=float(vals[0]), merge_mm=float(vals[1]), max_miss=int(vals[2])) if len(vals) == 3 else None
    except ValueError:
        return None


def main(argv=None):
    args = parse_args(argv)
    smooth = smooth_config(args)
    identity = identity_config(args)
    denoise = denoise_config(args)
    surface = surface_config(args)
    background = background_config(args)
    if args.identity and identity is None:
        raise SystemExit("--identity takes GATE_MM,MERGE_MM,MAX_MISS (two numbers and an int), not %r" % args.identity)

    import numpy as np
    import torch
    import awr_amd
    from awr_amd import detect, hourglass, resnet_deconv
    from awr_amd.config import Config
    from train import parse_overrides

    over = parse_overrides(args.set)
    if args.net:
        over["net"] = args.net
    cfg = Config(load_model=args.load_model, **over)
    frames = np.load(args.frames, mmap_mode="r")
    if "resnet" in cfg.net:
        net = resnet_deconv.get_deconv_net(int(cfg.net.split("_")[1]), cfg.jt_num, cfg.downsample)
    else:
        net = hourglass.PoseNet(cfg.net, cfg.jt_num)
    pth = torch.load(cfg.load_model, map_location="cpu", weights_only=False)
    key = "model_ema" if args.ema else "model"
    if key not in pth:
        raise awr_amd._lib.AwrError("{} holds no \"{}\" entry{}".format(cfg.load_model, key, " (--ema needs a checkpoint written with ema_decay)" if args.ema else ""))
    net.load_state_dict(pth[key])
    bs = 1 if args.track or smooth is not None or identity is not None or args.background_adapt is not None else min(cfg.batch_size, len(frames))
    views = None if args.views is None else detect.parse_views(args.views)
    if args.hands == 1 and (args.reach is not None or args.min_pixels is not None):
        raise SystemExit("--reach and --min-pixels belong to --hands K with K >= 2")
    if args.isolate and (args.hands == 1 or args.views is not None):
        raise SystemExit("--isolate belongs to --hands K with K >= 2, without --views")
    if args.edge_mm is not None and args.hands == 1:
        raise SystemExit("--edge-mm belongs to --hands K with K >= 2")
    if args.link_mm is not None and (args.hands == 1 or args.edge_mm is None):
        raise SystemExit("--link-mm belongs to --hands K with K >= 2 and --edge-mm E")
    if args.link_gap is not None and args.link_mm is None:
        raise SystemExit("--link-gap belongs to --link-mm L")
    link_kw = {} if args.link_mm is None else dict(link_mm=args.link_mm, link_gap=detect.LINK_GAP if args.link_gap is None else args.link_gap)
    hands_kw = {} if args.hands == 1 else dict(isolate=args.isolate, edge_mm=args.edge_mm, hands=args.hands, reach=detect.REACH if args.reach is None else args.reach,
                                               min_pixels=detect.MIN_PIXELS if args.min_pixels is None else args.min_pixels)
    K = args.hands
    pred = awr_amd.Predictor(net.cuda(), cfg.img_size, cfg.kernel_size, cube=cfg.cube, max_batch=bs, frame_shape=frames.shape[1:],
                             winograd=cfg.winograd, parity=cfg.parity_infer, confidence=args.confidence,
                             recenter=args.recenter, track=args.track, views=views, fuse=args.fuse, palm=args.palm,
                             smooth=smooth, identity=identity, denoise=denoise, surface=surface, background=background, **hands_kw, **link_kw)
    if background is not None:
        from awr_amd import background as BG
        empty = np.load(args.background, mmap_mode="r")
        if empty.ndim != 3 or empty.dtype != np.uint16 or empty.shape[1:] != frames.shape[1:]:
            raise SystemExit("--background: %s holds %s %s, not uint16 frames of %s" % (args.background, empty.dtype, empty.shape, tuple(frames.shape[1:])))
        pred.learn_background(np.array(empty[:BG.MAX_FRAMES]))
    hands = {"n_hands": [], "hand_status": [], "hand_info": []}
    if identity is not None:
        hands.update(hand_id=[], hand_code=[])
    stateful = bool(args.recenter or args.track)
    centers, codes = [], []
    uvd, xyz, extra = [], [], {"conf": [], "peak": [], "spread_mm": []}
    fused = {"view_spread_mm": [], "views_used": []}
    raw = {"raw_uvd": [], "raw_xyz": [], "filter_code": []}
    seen = {"surface_code": [], "surface_gap_mm": [], "surface_counts": []}
    for lo in range(0, len(frames), bs):
        out = pred.predict(np.array(frames[lo:lo + bs]))
        uvd.append(out.uvd.cpu().numpy())
        xyz.append(out.xyz.cpu().numpy())
        if args.confidence:
            for k in extra:
                extra[k].append(getattr(out, k).cpu().numpy())
        if views is not None:
            for k in fused:
                fused[k].append(getattr(out, k).cpu().numpy())
        if smooth is not None:
            for k, t in (("raw_uvd", pred.raw_uvd), ("raw_xyz", pred.raw_xyz), ("filter_code", pred.filter_codes)):
                raw[k].append(t.cpu().numpy())
        if surface is not None:
            for k, t in (("surface_code", pred.surface_codes), ("surface_gap_mm", pred.surface_gap_mm), ("surface_counts", pred.surface_counts)):
                seen[k].append(t.cpu().numpy().reshape(-1, t.shape[-1]))
        if K > 1:
            hands["n_hands"].append(out.n_hands.cpu().numpy())
            hands["hand_status"].append(out.status.cpu().numpy())
            hands["hand_info"].append(pred.hand_info.cpu().numpy().reshape(-1, 4))
            if identity is not None:
                hands["hand_id"].append(out.ids.cpu().numpy())
                hands["hand_code"].append(pred.hand_codes.cpu().numpy())
        if stateful:
            centers.append(pred.centers_uvd.cpu().numpy().reshape(-1, 3))
            codes.append(pred.recenter_codes.cpu().numpy().reshape(args.recenter + 1, -1).T)
        try:
            pred.check()
        except awr_amd._lib.AwrError as e:
            print("frames %d...: %s" % (lo, e), file=sys.stderr)
    os.makedirs(args.out, exist_ok=True)
    for name, rows in (("pred_uvd.txt", uvd), ("pred_xyz.txt", xyz)):
        np.savetxt(os.path.join(args.out, name), np.concatenate(rows, 0).reshape(len(frames) * K, cfg.jt_num * 3), fmt="%.3f")
    if args.confidence:
        for k, rows in extra.items():
            np.savetxt(os.path.join(args.out, "pred_%s.txt" % k), np.concatenate(rows, 0).reshape(len(frames) * K, cfg.jt_num), fmt="%.6g")
    if K > 1:
        for k, rows in hands.items():
            np.savetxt(os.path.join(args.out, "pred_%s.txt" % k), np.concatenate(rows, 0), fmt="%d")
    if views is not None:
        np.savetxt(os.path.join(args.out, "pred_view_spread_mm.txt"), np.concatenate(fused["view_spread_mm"], 0), fmt="%.6g")
        np.savetxt(os.path.join(args.out, "pred_views_used.txt"), np.concatenate(fused["views_used"], 0), fmt="%d")
    if smooth is not None:
        for k in ("raw_uvd", "raw_xyz"):
            np.savetxt(os.path.join(args.out, "pred_%s.txt" % k), np.concatenate(raw[k], 0).reshape(len(frames) * K, cfg.jt_num * 3), fmt="%.3f")
        np.savetxt(os.path.join(args.out, "pred_filter_code.txt"), np.concatenate(raw["filter_code"], 0).reshape(len(frames) * K, cfg.jt_num), fmt="%d")
    if surface is not None:
        for k, rows in seen.items():
            np.savetxt(os.path.join(args.out, "pred_%s.txt" % k), np.concatenate(rows, 0), fmt="%.6g" if k == "surface_gap_mm" else "%d")
    if stateful:
        np.savetxt(os.path.join(args.out, "pred_center_uvd.txt"), np.concatenate(centers, 0), fmt="%.6f")
        np.savetxt(os.path.join(args.out, "pred_recenter_code.txt"), np.concatenate(codes, 0), fmt="%d")


if __name__ == "__main__":
    main()
