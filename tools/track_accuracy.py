"""Tracking, the temporal joint filter and its look-ahead on synthetic SEQUENCES, on one MI355X -> profiles/track_accuracy.txt

    python tools/track_accuracy.py [--train 32768] [--epochs 4] [--seqs 64] [--length 120] [--work DIR] [--parent HASH]
                                   [--out profiles/track_accuracy.txt]

THESE ARE PROCEDURAL HANDS (awr_amd/synth.py: capsules, uniform pose draws eased between key poses, no sensor model).  The numbers say how
the project's own pieces behave on a labelled input they can all consume; they say NOTHING about NYU or about any real camera.

A driver like tools/synth_accuracy.py, whose training step it runs unchanged (imported, not copied): each GPU step is a child process
under its own time limit, and the driver stops at the first step that fails or times out.
  train: tools/synth_accuracy.py's `train` step (ResNet18 on SyntheticFrames, independent poses).
  score: for key_every in 30, 15, 8 (slow, medium, fast motion): `seqs` sequences of `length` frames at 30 fps from
         synth.sample_sequences, rendered on the device, ONE SEQUENCE PER BATCH SLOT, frame t of every sequence in call t.  Per
         configuration of Predictor -- per-frame palm=True; + track=True; + smooth (defaults); + weight="conf"; + lead=True; + a gate; a
         small sweep of beta and min_cutoff; the filter without the tracker; the tracker with refine_iters=0 (its centre taken as it
         is), alone, smoothed and with lead -- the mean and median joint error against the labels over the finite joints, the jitter (mean
         norm of the second difference over time of prediction - label), frames whose status is not OK, joints that are NaN, and the
         counts of each filter code.
No thresholds: the tool records what comes out, rows where the filter loses included.  There is no fall-back: without a GPU it fails."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]
import synth_accuracy as SA  # noqa: E402

SEED_SEQ, FPS = 303, 30.0
KEY_EVERY = (30, 15, 8)
LIMITS = {"train": SA.LIMITS["train"], "score": 900}          # seconds per step
BASE = dict(palm=True)
CONFIGS = [("per-frame, palm=True", dict()),
           ("+ track=True", dict(track=True)),
           ("+ smooth (defaults)", dict(track=True, smooth=dict())),
           ("+ weight=\"conf\"", dict(track=True, smooth=dict(weight="conf"))),
           ("+ lead=True", dict(track=True, smooth=dict(lead=True))),
           ("+ gate_mm=60", dict(track=True, smooth=dict(gate_mm=60.0))),
           ("smooth, beta=0.005", dict(track=True, smooth=dict(beta=0.005))),
           ("smooth, beta=0.05", dict(track=True, smooth=dict(beta=0.05))),
           ("smooth, beta=0.1", dict(track=True, smooth=dict(beta=0.1))),
           ("smooth, min_cutoff=0.5", dict(track=True, smooth=dict(min_cutoff=0.5))),
           ("smooth, min_cutoff=2", dict(track=True, smooth=dict(min_cutoff=2.0))),
           ("smooth only (no track)", dict(smooth=dict())),
           # the tracked centre taken as it is: with refine_iters=0 no centre-of-mass pass moves it (or the detector's seed) before the crop
           ("track, refine_iters=0", dict(track=True, refine_iters=0)),
           ("  + smooth", dict(track=True, refine_iters=0, smooth=dict())),
           ("  + smooth, lead=True", dict(track=True, refine_iters=0, smooth=dict(lead=True)))]


def step_score(a):
    import numpy as np
    import torch
    import awr_amd
    from awr_amd import synth
    from awr_amd import track as T
    info = json.load(open(os.path.join(a.work, "train.json")))
    pth = torch.load(info["checkpoint"], map_location="cpu", weights_only=False)
    net = awr_amd.get_deconv_net(18, 14, 2)
    net.load_state_dict(pth["model"])
    net = net.cuda().eval()
    n_seq, length = a.seqs, a.length
    res = {}
    for ke in KEY_EVERY:
        poses = synth.sample_sequences(n_seq, length, SEED_SEQ + ke, key_every=ke)
        # time-major rows, so that frame t of every sequence is one contiguous slice of the frame store: call t's batch
        order = (np.arange(n_seq)[None, :] * length + np.arange(length)[:, None]).ravel()
        sf = synth.SyntheticFrames(n_seq * length, SEED_SEQ + ke, "test", poses={k: np.ascontiguousarray(v[order]) for k, v in poses.items()})
        assert sf.check() == 0
        lab = sf.labels_xyz.reshape(length, n_seq, 14, 3)                                 # (t, sequence, joint, 3)
        speed = float((np.linalg.norm(np.diff(lab, axis=0), axis=-1) * FPS).mean())
        block = {"mean_joint_speed_mm_s": speed, "rows": {}}
        for name, opt in CONFIGS:
            pred = awr_amd.Predictor(net, 128, 1.0, max_batch=n_seq, **BASE, **opt)
            xyz, status, codes = [], [], []
            for t in range(length):
                out = pred.predict(sf.frame_store.data[t * n_seq:(t + 1) * n_seq])
                xyz.append(out.xyz)
                status.append(out.status)
                if pred.smooth is not None:
                    codes.append(pred.filter_codes)
            xyz = torch.stack(xyz).cpu().numpy().astype(np.float64)
            status = torch.stack(status).cpu().numpy()
            d = xyz - lab
            e = np.linalg.norm(d, axis=-1)
            fin = np.isfinite(e)
            jit = np.linalg.norm(d[2:] - 2.0 * d[1:-1] + d[:-2], axis=-1)
            r = dict(mean=float(e[fin].mean()), median=float(np.median(e[fin])), jitter=float(jit[np.isfinite(jit)].mean()),
                     frames=int(status.size), not_ok=int((status != 0).sum()), nan_joints=int((~fin).sum()))
            if codes:
                r["codes"] = np.bincount(torch.stack(codes).cpu().numpy().ravel(), minlength=len(T.FILTER_NAMES)).tolist()
            block["rows"][name] = r
            print(ke, name, r, flush=True)
            del pred
        res[str(ke)] = block
        del sf
        torch.cuda.empty_cache()
    json.dump(res, open(os.path.join(a.work, "track_score.json"), "w"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=32768)
    ap.add_argument("--test", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--length", type=int, default=120)
    ap.add_argument("--work", default=os.path.join(REPO, "output", "track_accuracy"))
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "track_accuracy.txt"))
    ap.add_argument("--step", choices=("train", "score"), default=None, help="(internal) run one GPU step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/track_accuracy.py needs a GPU: nothing is measured without one")
        {"train": SA.step_train, "score": step_score}[a.step](a)
        return
    os.makedirs(a.work, exist_ok=True)
    base = [sys.executable, os.path.abspath(__file__), "--train", str(a.train), "--test", str(a.test), "--epochs", str(a.epochs), "--workers",
            str(a.workers), "--seqs", str(a.seqs), "--length", str(a.length), "--work", a.work]
    for step in ("train", "score"):
        log = os.path.join(a.work, step + ".log")
        print("[track_accuracy] step %s (limit %d s) -> %s" % (step, LIMITS[step], log), flush=True)
        with open(log, "w") as f:
            proc = subprocess.Popen(["timeout", "-k", "10", str(LIMITS[step])] + base + ["--step", step], stdout=f, stderr=subprocess.STDOUT)
            while True:                          # (a line a minute, so that whoever watches this process sees it is alive)
                try:
                    rc = proc.wait(timeout=60)
                    break
                except subprocess.TimeoutExpired:
                    print("[track_accuracy] step %s is running" % step, flush=True)
        if rc != 0:
            raise SystemExit("[track_accuracy] step %s ended with status %d: stopping here (see %s)" % (step, rc, log))
    tr, sc = (json.load(open(os.path.join(a.work, f))) for f in ("train.json", "track_score.json"))
    head = a.parent or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    from awr_amd import track as T
    L = []
    L.append("PROCEDURAL HANDS (awr_amd/synth.py: capsules, uniform pose draws, no sensor model).  These numbers say how the project's own pieces")
    L.append("behave on a labelled input all of them can consume.  They say NOTHING about NYU or about any real camera.")
    L.append("")
    L.append("parent commit: %s" % head)
    L.append("ResNet18, kernel_size 1, batch 64, device loader, default augmentation, ema_decay 0.999, Adam at the config's learning rate;")
    L.append("%d training frames of independent poses (seed %d), %d epochs (%.0f s of Trainer.train); Trainer.test on %d held-out frames, crops at"
             % (a.train, SA.SEED_TRAIN, a.epochs, tr["train_seconds"], a.test))
    L.append("the LABEL centres: mean joint error %.3f mm.  Scored: %d sequences x %d frames at %.0f fps (synth.sample_sequences, seed %d + key_every,"
             % (tr["test_mpe"], a.seqs, a.length, FPS, SEED_SEQ))
    L.append("smoothstep between key poses), 480 x 640 uint16 frames, forearm on, no noise, no wall, cube 300 mm, 14 joints; one sequence per batch")
    L.append("slot, every Predictor from RAW frames with palm=True (DESIGN.md 4.24); one MI355X; one run, no repeats: differences of a few tenths of a")
    L.append("millimetre between rows are within what another seed would move.  Without noise in the frames the jitter below is the NETWORK's")
    L.append("frame-to-frame inconsistency, not a sensor's.")
    L.append("")
    L.append("error: mean / median joint error in mm over the finite joints; jitter: mean norm of the second difference over time of")
    L.append("(prediction - label), mm; not OK: frames with a status code; NaN: joints without a value;")
    L.append("codes: " + ", ".join("%d %s" % (k, n) for k, n in zip(range(7), ("NONE", "INIT", "UPDATED", "GATED", "HELD", "REINIT", "LOST"))))
    assert len(T.FILTER_NAMES) == 7
    for ke in KEY_EVERY:
        b = sc[str(ke)]
        L.append("")
        L.append("key_every = %d: a key pose every %.2f s, mean joint speed %.1f mm/s" % (ke, ke / FPS, b["mean_joint_speed_mm_s"]))
        for name, _ in CONFIGS:
            r = b["rows"][name]
            L.append("  %-24s mean %7.3f   median %7.3f   jitter %7.3f   %d of %d frames not OK   %d NaN joints%s"
                     % (name, r["mean"], r["median"], r["jitter"], r["not_ok"], r["frames"], r["nan_joints"],
                        ("   codes %s" % r["codes"]) if "codes" in r else ""))
    text = "\n".join(L) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
