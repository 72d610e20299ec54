"""What config.device_eval costs or saves, on one MI355X with synthetic data (ResNet18, batch 128) -> profiles/device_eval.txt

    python tools/device_eval_timing.py [--frames 4096] [--nyu-frames 512] [--runs 3] [--steps 200] [--parent HASH] [--out profiles/device_eval.txt]

  * Trainer.test: images/s over the whole pass (its own timer, construction of the scoring engine included), config.device_eval off and on,
    median of `runs` passes after one untimed pass per arm -- with the device loader off in both arms (SyntheticHands: host tensors, copied per
    batch) and on in both arms (an NYU-layout directory of synthetic frames, rendered from HBM by nyu_device);
  * the training step rate over `steps` steps with print_freq = 100, off and on;
  * the kernel's own time per batch (HIP events around awr_eval_batch, B = 128, J = 14).
The arms of a pair alternate (off, on, off, on, ...) so that clock drift lands on both."""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import awr_amd  # noqa: E402,F401
from awr_amd.config import Config  # noqa: E402
from awr_amd.evaluator import DeviceEvalUtil  # noqa: E402
from awr_amd.trainer import SyntheticHands, Trainer  # noqa: E402


def make_cfg(out_dir, tag, device_eval, **kw):
    class Cfg(Config):
        net = "resnet_18"
        kernel_size = 1.0
        batch_size = 128
        num_workers = 0
        max_epoch = 1
        print_freq = 100
        vis_freq = 0
        output_dir = out_dir
        load_model = ""
        exp_id = tag
        use_hipgraph = False
        device_loader = False
    Cfg.device_eval = device_eval
    for k, v in kw.items():
        setattr(Cfg, k, v)
    return Cfg()


class Repeated(torch.utils.data.Dataset):
    """`n` samples that cycle through a small base dataset (an epoch of any length without holding its images)"""

    def __init__(self, base, n):
        self.base, self.n = base, n
        self.img_size, self.jt_num, self.paras, self.flip = base.img_size, base.jt_num, base.paras, base.flip

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.base[i % len(self.base)]


def time_test_passes(trainers, n_images, runs):
    """trainers: {arm: Trainer}; -> {arm: [images/s per pass]}"""
    rates = {arm: [] for arm in trainers}
    for arm, tr in trainers.items():
        tr.test(1)                      # untimed: plan build, tile autotune, frame cache
    for _ in range(runs):
        for arm, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.test(1)
            torch.cuda.synchronize()
            rates[arm].append(n_images / (time.perf_counter() - t0))
    return rates


def time_train_steps(tr, steps):
    """One epoch of exactly `steps` full batches through Trainer.train -> steps/s (the epoch-end metric read included)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def kernel_ms(reps=200):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    B, J = 128, 14
    jt, gt = torch.rand(B, J, 3, generator=g).to(dev) * 2 - 1, torch.rand(B, J, 3, generator=g).to(dev) * 2 - 1
    c = torch.tensor([0.0, 0.0, 750.0]).expand(B, 3).contiguous().to(dev)
    cube = torch.full((B, 3), 300.0, device=dev)
    M = torch.tensor([[0.45, 0.0, -80.0], [0.0, 0.45, -44.0], [0.0, 0.0, 1.0]]).expand(B, 3, 3).contiguous().to(dev)
    out = {}
    for store in (True, False):
        ev = DeviceEvalUtil(128, (588.03, 587.07, 320.0, 240.0), -1, J, capacity=B * (reps + 10), device=dev, store=store)
        for _ in range(10):
            ev.feed_batch(jt, gt, c, M, cube)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            ev.feed_batch(jt, gt, c, M, cube)
        b.record()
        torch.cuda.synchronize()
        out[store] = a.elapsed_time(b) / reps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--nyu-frames", type=int, default=512)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--parent", default=None, help="hash of the commit the measured tree sits on (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_eval.txt"))
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="device_eval_")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    head = a.parent or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    say("device_eval timing: ResNet18, batch 128, synthetic data, one %s" % torch.cuda.get_device_name(0))
    say("parent commit: %s" % head)
    say()
    med = statistics.median

    def pair(title, rates, unit):
        off, on = med(rates[False]), med(rates[True])
        say("%s" % title)
        say("  device_eval=False  %s   median %10.1f %s" % ("  ".join("%10.1f" % r for r in rates[False]), off, unit))
        say("  device_eval=True   %s   median %10.1f %s   (%+.2f %% vs False)" % ("  ".join("%10.1f" % r for r in rates[True]), on, unit, 100.0 * (on / off - 1)))
        return on / off

    ratios = {}
    # Trainer.test, host tensors in (device loader off)
    data = SyntheticHands(a.frames, seed=2)
    trs = {de: Trainer(make_cfg(tmp, "t%d" % de, de), None, data) for de in (False, True)}
    ratios["test, device loader off"] = pair("Trainer.test, %d images, device loader off (images/s per pass)" % a.frames,
                                             time_test_passes(trs, a.frames, a.runs), "images/s")
    del trs
    # Trainer.test, device loader on: frames resident in HBM, parameter blocks from the dataset
    from test_nyu_data_cpu import _write_fake_nyu
    root = os.path.join(tmp, "data", "nyu")
    os.makedirs(root)
    _write_fake_nyu(root, a.nyu_frames, np.random.RandomState(21))
    trs = {de: Trainer(make_cfg(tmp, "d%d" % de, de, device_loader=True, data_dir=os.path.join(tmp, "data"))) for de in (False, True)}
    say()
    ratios["test, device loader on"] = pair("Trainer.test, %d images, device loader on (images/s per pass)" % a.nyu_frames,
                                            time_test_passes(trs, a.nyu_frames, a.runs), "images/s")
    del trs
    # training step rate
    say()
    train = Repeated(SyntheticHands(1024, seed=1), a.steps * 128)
    rates = {False: [], True: []}
    trs = {de: Trainer(make_cfg(tmp, "w%d" % de, de), SyntheticHands(256, seed=1), None) for de in (False, True)}
    for tr in trs.values():
        tr.train()                      # untimed: plan build, tile autotune
        tr.trainData = train
    for _ in range(a.runs):
        for de, tr in trs.items():
            rates[de].append(time_train_steps(tr, a.steps))
    del trs
    ratios["train"] = pair("Trainer.train, %d steps per epoch, print_freq = 100 (steps/s per epoch)" % a.steps, rates, "steps/s")
    say()
    k = kernel_ms()
    say("awr_eval_batch, B = 128, J = 14 (HIP events, back-to-back launches): %.2f us per batch with per-frame rows, %.2f us with running sums only"
        % (1e3 * k[True], 1e3 * k[False]))
    say()
    slow = [name for name, r in ratios.items() if r < 0.98]
    if slow:
        say("SLOWER than the device_eval=False arm by more than the +-2 %% box spread: %s" % ", ".join(slow))
    else:
        say("no device_eval=True arm is slower than its device_eval=False arm by more than the +-2 % box spread")
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
