"""Train on synthetic hand frames, then score every predictor option against ground truth, on one MI355X -> profiles/synth_accuracy.txt

    python tools/synth_accuracy.py [--train 32768] [--test 2048] [--epochs 4] [--workers 4] [--work DIR] [--parent HASH]
                                   [--out profiles/synth_accuracy.txt] [--append]

THESE ARE PROCEDURAL HANDS (awr_amd/synth.py: capsules, uniform pose draws, no sensor model).  The numbers below say how the project's
own pieces behave on a labelled input they can all consume; they say NOTHING about NYU or about any real camera.

The tool is a driver: each GPU step is a child process (`--step train`, `--step score`) under its own time limit, and the driver stops
at the first step that fails or times out.
  train: ResNet18, kernel_size 1, batch 64, the device loader over SyntheticFrames(train) with the default augmentation, ema_decay 0.999,
         `epochs` epochs; Trainer.test after each epoch on the held-out SyntheticFrames(test) with the LABEL centres; the last checkpoint
         is what `score` loads.
  score: on the held-out frames, (1) the detector's centre against the label centre in mm, with the forearm and with the same poses
         rendered without it, (2) Predictor from RAW frames (its own detector, no label centre): plain, recenter=1, recenter=2, views
         (rot -15, +15) fused by mean and by conf, and the plain predictor over the EMA weights -- mean joint error in mm over the frames
         whose status is OK, (3) Spearman's rank correlation of `conf` with the per-joint error (negative = confident joints are better),
         (4) the same detector centres after awr_detect_palm, and Predictor(palm=True) plain, recenter=1 and recenter=2.
No thresholds: the tool records.  There is no fall-back: without a GPU it fails."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SEED_TRAIN, SEED_TEST = 101, 202
LIMITS = {"train": 600, "score": 300}          # seconds per step


def sets(a, which):
    from awr_amd import synth
    from awr_amd.config import Config
    if which == "train":
        return synth.SyntheticFrames(a.train, SEED_TRAIN, "train", aug_para=Config().augment_para)
    return synth.SyntheticFrames(a.test, SEED_TEST, "test", forearm=(which != "test_no_forearm"))


def step_train(a):
    import torch
    from awr_amd.config import Config
    from awr_amd.trainer import Trainer

    class Cfg(Config):
        net, kernel_size, batch_size, num_workers, max_epoch, output_dir, load_model, exp_id, use_hipgraph, vis_freq, device_eval, ema_decay = \
            "resnet_18", 1.0, 64, a.workers, a.epochs, a.work, "", "synth", False, 0, True, 0.999
    torch.manual_seed(0)
    train, test = sets(a, "train"), sets(a, "test")
    assert train.check() == 0 and test.check() == 0
    tr = Trainer(Cfg(), train.dataset, test.dataset)
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    tr.train()
    t1.record()
    torch.cuda.synchronize()
    mpe = tr.test(-1)
    res = dict(test_mpe=float(mpe), test_mpe_ema=float(tr.last_test_mpe_ema), train_seconds=t0.elapsed_time(t1) / 1e3,
               checkpoint=os.path.join(tr.work_dir, "epoch_%d.pth" % a.epochs), lr=float(tr.engine.lr))
    json.dump(res, open(os.path.join(a.work, "train.json"), "w"))


def spearman(x, y):
    import numpy as np

    def rank(v):
        order = np.argsort(v, kind="stable")
        r = np.empty(len(v))
        r[order] = np.arange(len(v))
        return r
    rx, ry = rank(x), rank(y)
    return float(np.corrcoef(rx, ry)[0, 1])


def step_score(a):
    import numpy as np
    import torch
    import awr_amd
    from awr_amd import detect as D
    from awr_amd.evaluator import uvd2xyz
    info = json.load(open(os.path.join(a.work, "train.json")))
    pth = torch.load(info["checkpoint"], map_location="cpu", weights_only=False)
    res = {}
    test = sets(a, "test")
    n, B = test.n, 64
    # (1) the detector's centre against the label centre
    for tag, sf in (("forearm", test), ("no_forearm", sets(a, "test_no_forearm"))):
        c, st = D.detect_device(sf.frame_store, np.arange(n))
        c, st = c.cpu().numpy(), st.cpu().numpy()
        ok = st == 0
        d = uvd2xyz(c[ok], sf.paras, sf.flip).astype(np.float64) - sf.centers[ok]
        e = np.linalg.norm(d, axis=1)
        res["detector_" + tag] = dict(ok=int(ok.sum()), n=n, mean=float(e.mean()), median=float(np.median(e)), p90=float(np.percentile(e, 90)),
                                      mean_offset=[float(v) for v in d.mean(0)], over100=int((e > 100.0).sum()))
        # the same centres after the palm pass, in batches: its scratch is one word per pixel and frame
        pc, pst = [], []
        for lo in range(0, n, B):
            idx = np.arange(lo, min(n, lo + B))
            c0, s0 = D.detect_device(sf.frame_store, idx)
            c1, s1, _ = D.palm_device(sf.frame_store, idx, c0, s0)
            pc.append(c1.cpu().numpy())
            pst.append(s1.cpu().numpy())
        c, st = np.concatenate(pc), np.concatenate(pst)
        ok = st == 0
        d = uvd2xyz(c[ok], sf.paras, sf.flip).astype(np.float64) - sf.centers[ok]
        e = np.linalg.norm(d, axis=1)
        res["palm_" + tag] = dict(ok=int(ok.sum()), n=n, mean=float(e.mean()), median=float(np.median(e)), p90=float(np.percentile(e, 90)),
                                  mean_offset=[float(v) for v in d.mean(0)], over100=int((e > 100.0).sum()))

    def load(key):
        net = awr_amd.get_deconv_net(18, 14, 2)
        net.load_state_dict(pth[key])
        return net.cuda().eval()

    def run(net, **kw):
        pred = awr_amd.Predictor(net, 128, 1.0, max_batch=B, **kw)
        err, conf, bad = [], [], 0
        for lo in range(0, n, B):
            hi = min(n, lo + B)
            out = pred.predict(test.frame_store.data[lo:hi])
            ok = (out.status == 0).cpu().numpy()
            e = np.linalg.norm(out.xyz.cpu().numpy().astype(np.float64) - test.labels_xyz[lo:hi], axis=2)
            ok &= np.isfinite(e).all(1)
            bad += int((~ok).sum())
            err.append(e[ok])
            if kw.get("confidence"):
                conf.append(out.conf.cpu().numpy()[ok])
        err = np.concatenate(err)
        r = dict(mean=float(err.mean()), median=float(np.median(err)), frames=int(err.shape[0]), not_ok=bad)
        if conf:
            cf = np.concatenate(conf)
            r["spearman_conf_error"] = spearman(cf.ravel(), err.ravel())
            r["mean_error_most_confident_quarter"] = float(err.ravel()[cf.ravel() >= np.percentile(cf, 75)].mean())
            r["mean_error_least_confident_quarter"] = float(err.ravel()[cf.ravel() <= np.percentile(cf, 25)].mean())
        return r
    net = load("model")
    views = D.make_views(rot=(-15.0, 15.0))
    res["plain"] = run(net, confidence=True)
    res["recenter=1"] = run(net, recenter=1)
    res["recenter=2"] = run(net, recenter=2)
    res["views mean"] = run(net, views=views, fuse="mean")
    res["views conf"] = run(net, views=views, fuse="conf")
    res["palm, plain"] = run(net, palm=True)
    res["palm, recenter=1"] = run(net, palm=True, recenter=1)
    res["palm, recenter=2"] = run(net, palm=True, recenter=2)
    del net
    res["plain, EMA weights"] = run(load("model_ema"))
    json.dump(res, open(os.path.join(a.work, "score.json"), "w"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=32768)
    ap.add_argument("--test", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--work", default=os.path.join(REPO, "output", "synth_accuracy"))
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "synth_accuracy.txt"))
    ap.add_argument("--append", action="store_true", help="write the new run below what --out already holds instead of replacing it")
    ap.add_argument("--step", choices=("train", "score"), default=None, help="(internal) run one GPU step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/synth_accuracy.py needs a GPU: nothing is measured without one")
        {"train": step_train, "score": step_score}[a.step](a)
        return
    os.makedirs(a.work, exist_ok=True)
    base = [sys.executable, os.path.abspath(__file__), "--train", str(a.train), "--test", str(a.test), "--epochs", str(a.epochs), "--workers",
            str(a.workers), "--work", a.work]
    for step in ("train", "score"):
        log = os.path.join(a.work, step + ".log")
        print("[synth_accuracy] step %s (limit %d s) -> %s" % (step, LIMITS[step], log), flush=True)
        with open(log, "w") as f:
            proc = subprocess.Popen(["timeout", "-k", "10", str(LIMITS[step])] + base + ["--step", step], stdout=f, stderr=subprocess.STDOUT)
            while True:                          # (a line a minute, so that whoever watches this process sees it is alive)
                try:
                    rc = proc.wait(timeout=60)
                    break
                except subprocess.TimeoutExpired:
                    print("[synth_accuracy] step %s is running" % step, flush=True)
        if rc != 0:
            raise SystemExit("[synth_accuracy] step %s ended with status %d: stopping here (see %s)" % (step, rc, log))
    tr, sc = (json.load(open(os.path.join(a.work, f))) for f in ("train.json", "score.json"))
    head = a.parent or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    L = []
    L.append("PROCEDURAL HANDS (awr_amd/synth.py: capsules, uniform pose draws, no sensor model).  These numbers say how the project's own pieces")
    L.append("behave on a labelled input all of them can consume.  They say NOTHING about NYU or about any real camera.")
    L.append("")
    L.append("parent commit: %s" % head)
    L.append("ResNet18, kernel_size 1, batch 64, device loader, default augmentation, ema_decay 0.999, Adam at the config's learning rate;")
    L.append("%d training frames (seed %d), %d epochs (%.0f s of Trainer.train, its per-epoch test passes included); %d held-out frames (seed %d);"
             % (a.train, SEED_TRAIN, a.epochs, tr["train_seconds"], a.test, SEED_TEST))
    L.append("480 x 640 uint16 frames, forearm on, no noise, no wall, cube 300 mm, 14 joints; one MI355X; one run, no repeats: differences of a few")
    L.append("tenths of a millimetre between rows are within what another seed would move")
    L.append("")
    L.append("(1) Trainer.test, crops at the LABEL centres: mean joint error %.3f mm; the EMA weights: %.3f mm" % (tr["test_mpe"], tr["test_mpe_ema"]))
    L.append("")
    L.append("(2) the detector's centre (seed \"nearest\", defaults) against the label centre, mm")
    for tag, name in (("forearm", "with the forearm"), ("no_forearm", "same poses, no forearm")):
        d = sc["detector_" + tag]
        L.append("  %-24s mean %6.2f   median %6.2f   90th percentile %6.2f   mean offset (x, y, z) = (%+.1f, %+.1f, %+.1f)   %d of %d frames OK"
                 % (name, d["mean"], d["median"], d["p90"], d["mean_offset"][0], d["mean_offset"][1], d["mean_offset"][2], d["ok"], d["n"]))
    L.append("")
    L.append("(3) Predictor from RAW frames (its own detector; no label centre), mean / median joint error in mm over the frames with status OK")
    for k in ("plain", "recenter=1", "recenter=2", "views mean", "views conf", "plain, EMA weights"):
        r = sc[k]
        L.append("  %-22s mean %7.3f   median %7.3f   (%d frames, %d not OK)" % (k, r["mean"], r["median"], r["frames"], r["not_ok"]))
    L.append("  (views: the identity and rotations of -15 and +15 degrees)")
    L.append("")
    r = sc["plain"]
    L.append("(4) conf against the per-joint error, plain predictor, %d joints: Spearman's rank correlation %+.3f" % (r["frames"] * 14, r["spearman_conf_error"]))
    L.append("  mean error of the most confident quarter of the joints %.3f mm, of the least confident quarter %.3f mm"
             % (r["mean_error_most_confident_quarter"], r["mean_error_least_confident_quarter"]))
    L.append("")
    L.append("(5) palm=True (awr_detect_palm after the detector; DESIGN.md 4.24): the centre against the label centre, mm, to be read against (2)")
    for tag, name in (("forearm", "with the forearm"), ("no_forearm", "same poses, no forearm")):
        for key, what in (("detector_", "detector"), ("palm_", "palm")):
            d = sc[key + tag]
            L.append("  %-24s %-9s mean %6.2f   median %6.2f   90th percentile %6.2f   %4d frames over 100 mm   %d of %d frames OK"
                     % (name, what, d["mean"], d["median"], d["p90"], d["over100"], d["ok"], d["n"]))
    L.append("  Predictor(palm=True) from RAW frames, mean / median joint error in mm over the frames with status OK, to be read against (3)")
    for k in ("palm, plain", "palm, recenter=1", "palm, recenter=2"):
        r = sc[k]
        L.append("  %-22s mean %7.3f   median %7.3f   (%d frames, %d not OK)" % (k, r["mean"], r["median"], r["frames"], r["not_ok"]))
    text = "\n".join(L) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.append and os.path.exists(a.out):          # keep the earlier runs: a new run goes below them, under its own parent-commit line
        text = open(a.out).read() + "\n---- a later run of tools/synth_accuracy.py (--append): every row measured again, section (5) added ----\n\n" + text
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
