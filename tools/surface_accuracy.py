"""What the label-free surface check (Predictor(surface=True)) says about a TRAINED network's errors, on one MI355X
-> appended to profiles/surface_check.txt

    python tools/surface_accuracy.py [--train 32768] [--test 2048] [--epochs 4] [--work output/synth_accuracy] [--out profiles/surface_check.txt]

THESE ARE PROCEDURAL HANDS (awr_amd/synth.py: capsules, uniform pose draws, no sensor model): the only labelled frames there are.  The
numbers say whether the label-free codes rank errors and options the way the labelled error does ON THEM; real frames stay UNMEASURED.

The tool is a driver, as tools/synth_accuracy.py is: each GPU step is a child process under its own time limit, and the driver stops at
the first step that fails or times out.
  train: tools/synth_accuracy.py's own training step (ResNet18, 4 epochs over 32 768 synthetic frames), skipped where its checkpoint
         already lies under --work;
  score: (0) the rule on 96 procedural hands and their TRUE joints, displaced in x and in z (the numpy statement; no network): the share
         of each code; (1) Predictor(surface=True) from RAW held-out frames, plain, recenter=2 and palm=True: per joint, Spearman's rank
         correlation of OFF (0 / 1) and of |gap - median ON gap| with the joint's error; the mean error of ON, OCCLUDED and OFF joints;
         the mean error of frames by their number of OFF joints and of OFF bone samples; (2) per option the mean error next to the mean
         OFF counts, so that a reader sees whether the label-free counts rank the options the way the labelled error does.
No thresholds: the tool records, also what is unflattering.  There is no fall-back: without a GPU it fails."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]
LIMITS = {"train": 600, "score": 300}          # seconds per step
OPTIONS = (("plain (recenter=0)", dict()), ("recenter=2", dict(recenter=2)), ("palm=True", dict(palm=True)))
MOVES = (("true joints", (0, 0, 0)), ("+40 mm in x", (40, 0, 0)), ("+20 mm in x", (20, 0, 0)), ("-20 mm in x", (-20, 0, 0)), ("60 mm deeper", (0, 0, 60)),
         ("40 mm nearer", (0, 0, -40)))


def step_score(a):
    import numpy as np
    import torch
    import awr_amd
    from awr_amd import evaluator, nyu_data, surface as SF, synth
    from synth_accuracy import sets, spearman
    res = {"rule": {}, "options": {}}
    # (0) the rule itself on true and displaced joints
    joints21, prims, bbox = synth.forward_kinematics(synth.sample_poses(96, 7))
    frames = synth.render(prims, bbox)
    lab = synth.labels(joints21, 14)[0]
    zero = np.zeros(96, np.int32)
    for name, move in MOVES:
        uvd = evaluator.xyz2uvd((lab + np.asarray(move, np.float64)).astype(np.float32), nyu_data.PARAS, -1)
        codes, gap, counts, _ = SF.joints_surface(frames, np.arange(96), uvd, zero, zero)
        on = gap[codes == SF.ON].astype(np.float64)
        res["rule"][name] = dict(share=[float((codes == k).mean()) for k in range(4)], min_off=int(counts[:, SF.OFF].min()), max_off=int(counts[:, SF.OFF].max()),
                                 samples_off=float(counts[:, 4 + SF.OFF].sum() / max(1, counts[:, 4:].sum())), frames_with_off_sample=float((counts[:, 4 + SF.OFF] > 0).mean()),
                                 on_gap=[float(np.percentile(on, p)) for p in (1, 50, 99)] if len(on) else None)
    # (1), (2) a trained network
    info = json.load(open(os.path.join(a.work, "train.json")))
    pth = torch.load(info["checkpoint"], map_location="cpu", weights_only=False)
    net = awr_amd.get_deconv_net(18, 14, 2)
    net.load_state_dict(pth["model"])
    net = net.cuda().eval()
    test = sets(a, "test")
    n, B = test.n, 64
    for name, kw in OPTIONS:
        pred = awr_amd.Predictor(net, 128, 1.0, max_batch=B, surface=True, **kw)
        err, codes, gaps, counts, bad = [], [], [], [], 0
        for lo in range(0, n, B):
            hi = min(n, lo + B)
            out = pred.predict(test.frame_store.data[lo:hi])
            e = np.linalg.norm(out.xyz.cpu().numpy().astype(np.float64) - test.labels_xyz[lo:hi], axis=2)
            ok = (out.status == 0).cpu().numpy() & np.isfinite(e).all(1) & (pred.surface_status == 0).cpu().numpy()
            bad += int((~ok).sum())
            err.append(e[ok])
            codes.append(pred.surface_codes.cpu().numpy()[ok])
            gaps.append(pred.surface_gap_mm.cpu().numpy()[ok].astype(np.float64))
            counts.append(pred.surface_counts.cpu().numpy()[ok])
        err, codes, gaps, counts = (np.concatenate(x) for x in (err, codes, gaps, counts))
        r = dict(frames=int(err.shape[0]), not_ok=bad, mean=float(err.mean()), median=float(np.median(err)))
        off = (codes == SF.OFF).astype(np.float64)
        r["spearman_off_error"] = spearman(off.ravel(), err.ravel()) if 0 < off.sum() < off.size else None
        on_gap = float(np.median(gaps[codes == SF.ON])) if (codes == SF.ON).any() else float("nan")
        have = np.isfinite(gaps)
        r["median_on_gap"] = on_gap
        r["spearman_gap_error"] = spearman(np.abs(gaps[have] - on_gap), err[have]) if have.sum() > 2 else None
        r["gap_joints"] = int(have.sum())
        r["by_code"] = {k: dict(joints=int((codes == c).sum()), mean=float(err[codes == c].mean()) if (codes == c).any() else None)
                        for k, c in (("ON", SF.ON), ("OCCLUDED", SF.OCCLUDED), ("OFF", SF.OFF), ("OUTSIDE", SF.OUTSIDE))}
        frame_err = err.mean(1)
        r["by_off_joints"] = [dict(off=lab_, frames=int(m.sum()), mean=float(frame_err[m].mean()) if m.any() else None)
                              for lab_, m in (("0", counts[:, 2] == 0), ("1", counts[:, 2] == 1), ("2", counts[:, 2] == 2), ("3 or more", counts[:, 2] >= 3))]
        r["by_off_samples"] = [dict(off=lab_, frames=int(m.sum()), mean=float(frame_err[m].mean()) if m.any() else None)
                               for lab_, m in (("0", counts[:, 6] == 0), ("1 ... 2", (counts[:, 6] >= 1) & (counts[:, 6] <= 2)),
                                               ("3 ... 5", (counts[:, 6] >= 3) & (counts[:, 6] <= 5)), ("6 or more", counts[:, 6] >= 6))]
        r["mean_off_joints"], r["mean_off_samples"] = float(counts[:, 2].mean()), float(counts[:, 6].mean())
        r["mean_occluded_joints"] = float(counts[:, 1].mean())
        r["spearman_frame_off_error"] = spearman(counts[:, 2] + counts[:, 6], frame_err) if len(frame_err) > 2 else None
        res["options"][name] = r
        del pred
    json.dump(res, open(os.path.join(a.work, "surface_score.json"), "w"))


def num(x, f="%.3f"):
    return "none" if x is None else f % x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=32768)
    ap.add_argument("--test", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--work", default=os.path.join(REPO, "output", "synth_accuracy"))
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "surface_check.txt"))
    ap.add_argument("--step", choices=("score",), default=None, help="(internal) run the GPU step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/surface_accuracy.py needs a GPU: nothing is measured without one")
        step_score(a)
        return
    os.makedirs(a.work, exist_ok=True)
    sizes = ["--train", str(a.train), "--test", str(a.test), "--epochs", str(a.epochs), "--workers", str(a.workers), "--work", a.work]
    steps = [("score", [sys.executable, os.path.abspath(__file__)] + sizes + ["--step", "score"])]
    trained = os.path.exists(os.path.join(a.work, "train.json")) and os.path.exists(json.load(open(os.path.join(a.work, "train.json")))["checkpoint"])
    if not trained:
        steps.insert(0, ("train", [sys.executable, os.path.join(REPO, "tools", "synth_accuracy.py")] + sizes + ["--step", "train"]))
    for step, cmd in steps:
        log = os.path.join(a.work, "surface_" + step + ".log")
        print("[surface_accuracy] step %s (limit %d s) -> %s" % (step, LIMITS[step], log), flush=True)
        with open(log, "w") as f:
            proc = subprocess.Popen(["timeout", "-k", "10", str(LIMITS[step])] + cmd, stdout=f, stderr=subprocess.STDOUT)
            while True:                          # (a line a minute, so that whoever watches this process sees it is alive)
                try:
                    rc = proc.wait(timeout=60)
                    break
                except subprocess.TimeoutExpired:
                    print("[surface_accuracy] step %s is running" % step, flush=True)
        if rc != 0:
            raise SystemExit("[surface_accuracy] step %s ended with status %d: stopping here (see %s)" % (step, rc, log))
    tr, sc = (json.load(open(os.path.join(a.work, f))) for f in ("train.json", "surface_score.json"))
    head = a.parent or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    T = []
    T.append("---- tools/surface_accuracy.py: what the codes say about errors ----")
    T.append("")
    T.append("PROCEDURAL HANDS (awr_amd/synth.py: capsules, uniform pose draws, no sensor model).  They say NOTHING about any real camera: UNMEASURED on real frames.")
    T.append("parent commit: %s" % head)
    T.append("")
    T.append("(0) the rule (radius 1, in_mm 40, out_mm 15, min_on 1) on 96 procedural hands (sample_poses(96, 7), forearm on) and their 1 344 labelled joints,")
    T.append("    the numpy statement, no network: share of ON / OCCLUDED / OFF / OUTSIDE; OFF joints per frame min ... max; bone samples (3 per bone) that are OFF")
    for name, _ in MOVES:
        r = sc["rule"][name]
        T.append("  %-14s ON %.3f  OCCLUDED %.3f  OFF %.3f  OUTSIDE %.3f   OFF joints per frame %d ... %d   OFF samples %.1f %% (%.0f %% of the frames have one)"
                 % (name, r["share"][0], r["share"][1], r["share"][2], r["share"][3], r["min_off"], r["max_off"], 100 * r["samples_off"], 100 * r["frames_with_off_sample"]))
    g = sc["rule"]["true joints"]["on_gap"]
    T.append("  gaps of the true ON joints: 1st percentile %.1f mm, median %.1f mm, 99th percentile %.1f mm" % tuple(g))
    T.append("")
    T.append("(1) a trained network: ResNet18, %d synthetic training frames, %d epochs (tools/synth_accuracy.py's training step; Trainer.test %.3f mm at the LABEL"
             % (a.train, a.epochs, tr["test_mpe"]))
    T.append("    centres); Predictor(surface=True) from RAW frames on the %d held-out frames, its own detector; errors in mm over the frames with status OK" % a.test)
    for name, _ in OPTIONS:
        r = sc["options"][name]
        T.append("  %s: %d frames (%d not OK), mean joint error %.3f mm, median %.3f mm" % (name, r["frames"], r["not_ok"], r["mean"], r["median"]))
        T.append("    Spearman, per joint: OFF (0 / 1) with the error %s;  |gap - median ON gap (%.1f mm)| with the error %s (%d joints with a gap)"
                 % (num(r["spearman_off_error"], "%+.3f"), r["median_on_gap"], num(r["spearman_gap_error"], "%+.3f"), r["gap_joints"]))
        T.append("    mean error by code: " + ";  ".join("%s %s mm (%d joints)" % (k, num(v["mean"]), v["joints"]) for k, v in r["by_code"].items()))
        T.append("    mean frame error by OFF joints:  " + ";  ".join("%s: %s mm (%d frames)" % (b["off"], num(b["mean"]), b["frames"]) for b in r["by_off_joints"]))
        T.append("    mean frame error by OFF samples: " + ";  ".join("%s: %s mm (%d frames)" % (b["off"], num(b["mean"]), b["frames"]) for b in r["by_off_samples"]))
        T.append("    Spearman, per frame: OFF joints + OFF samples with the frame's mean error %s" % num(r["spearman_frame_off_error"], "%+.3f"))
    T.append("")
    T.append("(2) do the label-free counts rank the options as the labelled error does?  per option: mean joint error | OFF joints, OFF samples, OCCLUDED joints per frame")
    for name, _ in OPTIONS:
        r = sc["options"][name]
        T.append("  %-20s %8.3f mm | %.4f  %.4f  %.4f" % (name, r["mean"], r["mean_off_joints"], r["mean_off_samples"], r["mean_occluded_joints"]))
    by_err = sorted(sc["options"], key=lambda k: sc["options"][k]["mean"])
    by_off = sorted(sc["options"], key=lambda k: sc["options"][k]["mean_off_joints"] + sc["options"][k]["mean_off_samples"])
    T.append("  order by error: %s;  order by OFF joints + samples: %s -- %s" % (" < ".join(by_err), " < ".join(by_off), "the same order" if by_err == by_off else "NOT the same order"))
    T.append("  (one run, one seed: differences of a few tenths of a millimetre between options are within what another seed would move)")
    text = "\n".join(T) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    before = open(a.out).read() + "\n" if os.path.exists(a.out) else ""
    with open(a.out, "w") as f:
        f.write(before + text)


if __name__ == "__main__":
    main()
