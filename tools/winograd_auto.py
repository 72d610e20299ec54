"""winograd="auto" on the MI355X: for each workload, the candidate times the search measured and its choice, the auto engine's step time against
every fixed mode measured in the same process, and what the search adds to the one-off set-up with a cold and with a warm AWR_TUNE_CACHE.

    python tools/winograd_auto.py [--steps 20] [--warmup 5] [--only NAME ...] [--config5]

Set-up time = engine construction + compile() (training) / + the first call (inference).  Overhead, cold: the auto engine's set-up on an empty
cache minus the set-up of a fixed engine of the chosen mode on an empty cache (its own tile tuning); warm: both again on the cache the first
runs wrote (decision and tiles reloaded).  One JSON line per workload, then a summary table.
"""
import argparse
import gc
import json
import os
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# name, net, training, batch, image size, joints, kernel size
WORKLOADS = [("resnet18_train_b64", "resnet_18", True, 64, 128, 14, 1.0),
             ("resnet18_train_b256", "resnet_18", True, 256, 128, 14, 1.0),
             ("hg1_train_b64", "hourglass_1", True, 64, 128, 14, 0.4),
             ("config3_infer_b128", "hourglass_1", False, 128, 128, 14, 0.4)]
CONFIG5 = ("config5_train", "hourglass_2", True, 128, 256, 21, 0.4)        # BASELINE config 5: a 152 GB plan


def make_net(awr_amd, name, J):
    torch.manual_seed(0)
    return (awr_amd.get_deconv_net(int(name.split("_")[1]), J, 2) if name.startswith("resnet") else awr_amd.PoseNet(name, J)).cuda()


def batch(B, H, J, dev):
    g = torch.Generator().manual_seed(977)
    img = torch.rand(B, 1, H, H, generator=g) * 2 - 1
    jt = torch.rand(B, J, 3, generator=g) * 1.6 - 0.8
    return img.to(dev), jt.to(dev)


def free(net):
    for p in list(net._plans.values()):
        net.release_plan(p)
    gc.collect()
    torch.cuda.empty_cache()


def run(net, training, B, H, ks, winograd, img, jt, steps, warmup):
    """-> (set-up seconds, ms per step, engine)"""
    from awr_amd.trainer import InferEngine, TrainEngine
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if training:
        net.train()
        eng = TrainEngine(net, B, H, ks, coord_weight=0.0, dense_weight=1.0, lr=1e-3, use_graph=False, winograd=winograd)
        eng.compile(img, jt)
        fn = lambda: eng.step(img, jt)          # noqa: E731
    else:
        net.eval()
        eng = InferEngine(net, B, H, ks, use_graph=False, winograd=winograd)
        eng(img)
        fn = lambda: eng(img)                   # noqa: E731
    torch.cuda.synchronize()
    setup = time.perf_counter() - t0
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return setup, 1e3 * (time.perf_counter() - t0) / steps, eng


def workload(awr_amd, w, steps, warmup, dev):
    from awr_amd import winograd_auto as WA
    name, netname, training, B, H, J, ks = w
    net = make_net(awr_amd, netname, J)
    img, jt = batch(B, H, J, dev)
    os.environ.pop("AWR_TUNE_CACHE", None)
    fixed, fixed_setup, nw = {}, {}, {}
    for mode in (WA.TRAIN_CANDIDATES if training else WA.INFER_CANDIDATES):
        s, ms, eng = run(net, training, B, H, ks, mode, img, jt, steps, warmup)
        fixed[mode], fixed_setup[mode], nw[mode] = ms, s, eng.plan.n_winograd
        del eng
        free(net)
    with tempfile.TemporaryDirectory() as d:
        os.environ["AWR_TUNE_CACHE"] = os.path.join(d, "tune.json")
        cold, ms_auto, eng = run(net, training, B, H, ks, "auto", img, jt, steps, warmup)
        mode, timings, source = eng.winograd_mode, eng.winograd_timings, eng.winograd_source
        del eng
        free(net)
        fixed_warm, _, eng = run(net, training, B, H, ks, mode, img, jt, 1, 0)
        del eng
        free(net)
        warm, ms_auto_warm, eng = run(net, training, B, H, ks, "auto", img, jt, steps, warmup)
        warm_source = eng.winograd_source
        del eng
        free(net)
        os.environ.pop("AWR_TUNE_CACHE")
    del net
    gc.collect()
    torch.cuda.empty_cache()
    best = min(fixed.values())
    return {"workload": name, "search_ms": {k: round(v, 3) for k, v in timings.items()}, "choice": mode, "source": source,
            "n_winograd": nw, "fixed_ms_per_step": {k: round(v, 3) for k, v in fixed.items()}, "auto_ms_per_step": round(ms_auto, 3),
            "auto_ms_per_step_warm": round(ms_auto_warm, 3), "best_fixed": min(fixed, key=fixed.get),
            "auto_vs_best": round(ms_auto / best, 4), "auto_vs_direct": round(ms_auto / fixed["direct"], 4),
            "within_1pct_of_best": ms_auto <= 1.01 * best, "not_slower_than_direct": ms_auto <= fixed["direct"],
            "setup_s": {"auto_cold": round(cold, 2), "fixed_cold": round(fixed_setup[mode], 2), "auto_warm": round(warm, 2), "fixed_warm": round(fixed_warm, 2)},
            "overhead_s": {"cold": round(cold - fixed_setup[mode], 2), "warm": round(warm - fixed_warm, 2)}, "warm_source": warm_source}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", nargs="*", default=None, help="workload names (default: all but config 5)")
    ap.add_argument("--config5", action="store_true", help="also Hourglass-2, 256 x 256, J = 21, batch 128 (152 GB plans; 5 steps, 3 warm-up)")
    args = ap.parse_args()
    import awr_amd
    dev = torch.device("cuda:0")
    todo = [w for w in WORKLOADS if args.only is None or w[0] in args.only]
    if args.config5 or (args.only and CONFIG5[0] in args.only):
        todo.append(CONFIG5)
    rows = []
    for w in todo:
        steps, warmup = (5, 3) if w is CONFIG5 else (args.steps, args.warmup)
        r = workload(awr_amd, w, steps, warmup, dev)
        print(json.dumps(r), flush=True)
        rows.append(r)
    print("\n%-22s %-14s %-48s %9s %9s %9s %14s %14s" % ("workload", "choice", "search ms/step", "auto ms", "best ms", "direct ms", "overhead cold", "overhead warm"))
    for r in rows:
        print("%-22s %-14s %-48s %9.3f %9.3f %9.3f %13.2fs %13.2fs" % (
            r["workload"], r["choice"], " ".join("%s=%.2f" % kv for kv in r["search_ms"].items()), r["auto_ms_per_step"],
            r["fixed_ms_per_step"][r["best_fixed"]], r["fixed_ms_per_step"]["direct"], r["overhead_s"]["cold"], r["overhead_s"]["warm"]))


if __name__ == "__main__":
    main()
