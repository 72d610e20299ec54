#!/usr/bin/env python3
"""bench.py -- the AWR hot path on MI355X: depth-images/sec of the full train step.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--net resnet_18|hourglass_1] [--graph] [--dp-selftest]
                    [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the headline line; nothing else.  `--full` adds everything else the
benchmark measures or checks: the live roofline blocks, the joint error against the oracle, the CPU baseline, the batch-256 shape,
the inference / Hourglass / data-path / Winograd / parity-mode / split-operand sub-records and, for N > 1, the replica check, the
bucket timeline and the transport A/B (each still switched off by its own --no-* option).  `--dump-outputs DIR` writes what the
timed path computes as DIR/<name>.npy: after the timed steps, the train step is run once more from the seeded starting state
(weights, optimiser state and batch are the same in every run), so two runs, or two builds, can be compared output for output.  The
last of the timed steps would not serve: split-K weight gradients are summed with atomics in the default mode, and Adam, stepping on
one batch again and again, amplifies their last-bit differences about tenfold per step.  With --deterministic the dumps are bitwise
identical.

`--gpus N` with N > 1 works both ways: under torchrun (RANK / LOCAL_RANK / WORLD_SIZE in the environment) this process is one rank;
started plainly (`python bench.py --gpus 8`) it spawns the N rank processes itself, one per GPU, and relays rank 0's JSON line.

Workload (BASELINE.json configs[1]): ResNet18-deconv, 128x128 depth crops, J=14, batch 64 per GPU, one full
reference iteration per step (GT map + forward + head + dense/joint Huber + backward + Adam; train.py:107-131)
on synthetic crops with reference-initialised weights.  N > 1 = one process per GPU, each
stepping its own batch-64 shard (weak scaling) with an RCCL all-reduce of the flat gradient arena.

Prints ONE JSON line (rank 0).  With --full, `roofline` is measured live with HIP events around every launch of the
implicit-GEMM conv kernels in serialised passes of the plan after the timed steps; `cpu_baseline` times the oracle (the CPU
restatement of the reference step, proven bit-identical to the reference in tools/gen_golden.py) on the host cores.
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

PEAK_FP32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CUs @ 2.4 GHz
PEAK_BF16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 (v_mfma_f32_32x32x16_bf16); the split-operand mode runs on this pipe


def _host_cpu():
    """(physical cores, model string) of the box bench.py runs on."""
    model, cores = "unknown", None
    try:
        pairs = set()
        phys = core = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                phys = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                core = line.split(":", 1)[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    pairs.add((phys, core))
                phys = core = None
        cores = len(pairs) or None
    except OSError:
        pass
    if not cores:
        try:
            import psutil
            cores = psutil.cpu_count(logical=False)
        except Exception:
            cores = None
    return int(cores or os.cpu_count() or 1), model


def cpu_baseline():
    """the CPU restatement of the path (oracle, kind 'port') on the host cores of the GPU box --
    (i) config 1: ResNet18-deconv, B=4, eval under no_grad, head included; (ii) the same net, B=4, one full train step
    (coord_weight 0, dense_weight 1, Adam lr 1e-3, kernel_size 1).  Synthetic inputs seed 1234, all physical cores,
    3 warm-up iterations, median of 10.  `value` is the train step (the unit of BASELINE.json's metric).  A batch of 4 images cannot
    feed 128 threads (the all-cores number is SLOWER than the survey's 8-vCPU container): `best_value` / `best_threads` report the
    host's best over a {8, 16, 32, 64, all} thread sweep of the same two workloads, so the stated baseline is not a handicapped one."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import awr_oracle as O
    cores, model = _host_cpu()
    prev = torch.get_num_threads()
    net, ks, b = "resnet_18", 1.0, 4
    img, jt = O.synth_batch(b, 128, 14, seed=1234)
    sd = O.reference_init_state(net, 14, seed=0)

    def med(fn, warm, reps):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        return 0.5 * (ts[reps // 2 - 1] + ts[reps // 2]) if reps % 2 == 0 else ts[reps // 2]

    def infer():
        with torch.no_grad():
            O.offset2joint_softmax(O.resnet18_forward(sd, img, False), img, ks)
    ost = {"step": 0, "m": {}, "v": {}}

    def train():
        O.train_step(net, sd, ost, img, jt, ks, 0.0, 1.0)
    sweep = {}
    try:
        torch.set_num_threads(cores)
        t_eval = med(infer, 3, 10)
        t_train = med(train, 3, 10)
        sweep[cores] = (t_eval, t_train)
        for n in (8, 16, 32, 64):
            if n >= cores:
                continue
            torch.set_num_threads(n)
            sweep[n] = (med(infer, 1, 3), med(train, 1, 3))
    finally:
        torch.set_num_threads(prev)
    bt = min(sweep, key=lambda n: sweep[n][1])
    be = min(sweep, key=lambda n: sweep[n][0])
    return {"value": round(b / t_train, 2), "unit": "images/s", "cores": cores, "cpu_model": model, "kind": "port",
            "eval_value": round(b / t_eval, 2), "eval_ms": round(1e3 * t_eval, 2), "train_ms": round(1e3 * t_train, 2),
            "best_value": round(b / sweep[bt][1], 2), "best_threads": bt, "best_eval_value": round(b / sweep[be][0], 2), "best_eval_threads": be,
            "thread_sweep_train_images_per_s": {str(n): round(b / sweep[n][1], 2) for n in sorted(sweep)},
            "sample": "BASELINE.md section 4: ResNet18-deconv B=4, (i) eval forward + head under no_grad [eval_value], (ii) one full train step "
                      "GT-map+fwd+head+Huber+bwd+Adam, coord_weight 0 [value]; torch-CPU fp32 restatement (oracle/awr_oracle.py, pinned bit-exact to "
                      "the reference), %d threads = physical cores, 3 warm-up, median of 10 -- NOTE: 4 images over-subscribe %d threads; best_value "
                      "is the same step at the best thread count of a {8,16,32,64,all} sweep (1 warm-up, median of 3)" % (cores, cores)}


def synth_nyu(n_frames, n_samples, seed=77):
    """Synthetic NYU-layout data for the data-path record: uint16 480 x 640 depth frames (far wall, a tilted hand-sized disc around the
    refined centre, 5 % sensor holes), camera-space joints around the centre, refined centres; sample i uses frame i % n_frames."""
    import numpy as np
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:480, 0:640]
    frames, fc = np.empty((n_frames, 480, 640), np.uint16), []
    for k in range(n_frames):
        c = np.array([rng.uniform(-120, 120), rng.uniform(-80, 80), rng.uniform(600, 950)])
        u, v = 588.03 * c[0] / c[2] + 320.0, -587.07 * c[1] / c[2] + 240.0
        d = np.full((480, 640), 1500.0 + rng.uniform(-200, 200))
        hand = (xx - u) ** 2 + (yy - v) ** 2 < (70 * 750.0 / c[2]) ** 2
        d[hand] = c[2] + 0.3 * (xx[hand] - u) - 0.2 * (yy[hand] - v) + rng.uniform(-3, 3, int(hand.sum()))
        d[rng.rand(480, 640) < 0.05] = 0
        frames[k] = np.round(d).astype(np.uint16)
        fc.append(c)
    frame_of = np.arange(n_samples) % n_frames
    centers = np.array(fc)[frame_of]
    raw = centers[:, None, :] + rng.uniform(-70, 70, (n_samples, 36, 3))        # joint_data.mat layout: 36 joints, nyu_loader.py:9-11 selects 14
    return frames, raw, centers, frame_of


def measure_data_path(awr_amd, O, dev, headline_ms, steps, warmup, batch=64, workers=8):
    """SURVEY 8f-2 / VERDICT r5 item 1: what feeds the engine.  (i) the host loader (awr_amd.nyu_data: the reference's per-sample numpy
    pipeline, dataloader/loader.py:19-179, PNG decode excluded) on ONE core; (ii) the device path's host half (parameter blocks + labels)
    on one core and its kernel alone; (iii) the BASELINE configs[1] train step fed by the device path: a DataLoader of `workers` processes
    yields parameter blocks (the reference's num_workers = 8, config.py:37), ONE awr_nyu_batch launch renders the batch from the frames
    resident in HBM, the engine steps on it -- images and labels differ every step."""
    import numpy as np
    from awr_amd import nyu_data as ND, nyu_device as DV
    from awr_amd.trainer import TrainEngine
    n_frames, n_samples = 256, batch * (steps + warmup + 4)
    frames, raw, centers, frame_of = synth_nyu(n_frames, n_samples)
    labels = raw[:, ND.JOINT][:, ND.EVAL]
    kw = dict(frame_of=frame_of, img_size=128, aug_para=[10, 0.1, 180])
    host = ND.NYU.from_arrays(frames, labels, centers, "train", **kw)
    devd = DV.DeviceNYU.from_arrays(frames.shape, labels, centers, "train", **kw)
    prev = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < 3.0:
            host[n % n_samples]
            n += 1
        cpu_rate = n / (time.perf_counter() - t0)
        t0, m = time.perf_counter(), 0
        while time.perf_counter() - t0 < 1.5:
            devd[m % n_samples]
            m += 1
        param_rate = m / (time.perf_counter() - t0)
    finally:
        torch.set_num_threads(prev)
    store = DV.FrameStore(frames)
    render = DV.Renderer(store, 128, batch)
    blocks = torch.stack([devd[i][0] for i in range(batch)])
    out = torch.empty((batch, 1, 128, 128), device=dev)
    for _ in range(5):
        render(blocks, out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(50):
        render(blocks, out)
    e1.record()
    torch.cuda.synchronize()
    render_us = e0.elapsed_time(e1) * 1e3 / 50          # includes the 12.8 KB block upload of each call
    render.check(batch)
    # bit-exactness spot check against the host loader inside the record (fresh datasets: the two random streams start together)
    h2 = ND.NYU.from_arrays(frames, labels, centers, "train", **kw)
    d2 = DV.DeviceNYU.from_arrays(frames.shape, labels, centers, "train", **kw)
    same = all(torch.equal(render(d2[i][0][None]).cpu()[0], h2[i][0]) for i in range(16))
    # (iii) the fed train step
    torch.manual_seed(0)
    net = _make_net(awr_amd, "resnet_18").cuda()
    eng = TrainEngine(net, batch, 128, 1.0, coord_weight=0.0, dense_weight=1.0, lr=1e-3, use_graph=False)
    img0, jt0 = O.synth_batch(batch, 128, 14, seed=1234)
    eng.compile(img0.to(dev), jt0.to(dev))
    loader = torch.utils.data.DataLoader(devd, batch_size=batch, shuffle=False, num_workers=workers, drop_last=True, pin_memory=True,
                                         persistent_workers=False, prefetch_factor=4 if workers else None)
    it = iter(loader)
    t_start = None
    for k in range(warmup + steps):
        if k == warmup:
            torch.cuda.synchronize()
            t_start = time.perf_counter()
        blk, _, jt_uvd, _, _, _ = next(it)
        eng.step(render(blk), jt_uvd.to(dev, non_blocking=True))
    torch.cuda.synchronize()
    fed_ms = (time.perf_counter() - t_start) / steps * 1e3
    loss = float(eng.losses[2])
    del it, loader, eng, net
    torch.cuda.empty_cache()
    cores, model = _host_cpu()
    return {"frames": "synthetic uint16 480x640, %d frames resident in HBM (%.0f MB)" % (n_frames, store.nbytes / 1e6),
            "cpu_loader": {"samples_per_s_per_worker": round(cpu_rate, 1), "cores_used": 1, "cpu_model": model, "host_cores": cores,
                           "what": "awr_amd.nyu_data.NYU.__getitem__ (crop + one of trans/scale/rot/none + normalise + labels), PNG decode excluded, 3 s sample"},
            "device_loader": {"host_param_blocks_per_s_per_worker": round(param_rate, 1),
                              "render_us_per_batch": round(render_us, 2), "render_samples_per_s": round(batch / render_us * 1e6, 0),
                              "render_gbps_out": round(batch * 128 * 128 * 4 / render_us / 1e3, 1), "batch": batch,
                              "bit_identical_to_host_loader": bool(same), "checked_samples": 16},
            "train_fed": {"workload": "resnet_18 train step, batch %d, every batch rendered by awr_nyu_batch from HBM-resident frames, parameter blocks + labels from "
                                      "a DataLoader with %d worker processes" % (batch, workers), "steps": steps, "warmup": warmup,
                          "ms_per_step": round(fed_ms, 3), "value": round(batch / fed_ms * 1e3, 2), "unit": "images/s",
                          "vs_synthetic_headline": round(headline_ms / fed_ms, 4), "final_loss": loss},
            "speedup_per_worker_vs_cpu_loader": round(param_rate / cpu_rate, 1)}


def _make_net(awr_amd, name, J=14):
    """'resnet_<18|50|101|152>' | 'hourglass_<n>' (train.py:51-57)"""
    return awr_amd.get_deconv_net(int(name.split("_")[1]), J, 2) if name.startswith("resnet") else awr_amd.PoseNet(name, J)


def parity_mm(net_name, ks, dev, parity=False):
    """mean / max 3D joint difference (mm, 300 mm cube => x150) between the HIP path and the oracle, eval mode (parity=True: the engine's
    blocked-accumulation plan, the mode Trainer.test scores with)."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import awr_oracle as O
    import awr_amd
    from awr_amd.trainer import InferEngine
    img, _ = O.synth_batch(4, 128, 14, seed=99)
    sd = O.procedural_state(O.manifest_for(net_name, 14), seed=0)
    m = _make_net(awr_amd, net_name)
    m.load_state_dict(sd)
    m = m.cuda()
    jt = InferEngine(m, 4, 128, ks, use_graph=False, parity=parity)(img.to(dev)).cpu()
    with torch.no_grad():
        ref = O.offset2joint_softmax(O.backbone_forward(net_name, sd, img)[-1], img, ks)
    d = (jt - ref).norm(dim=-1) * 150.0
    return float(d.mean()), float(d.max())


def _pool_info(L):
    """How many of the library's streams sit on a hardware queue of their own (awr_stream_pool_info)."""
    import ctypes as C
    n, k = C.c_int(), C.c_int()
    L.call("awr_stream_pool_info", C.byref(n), C.byref(k))
    return k.value


def measure_inference(awr_amd, O, net_name, batch, dev, rank, steps, warmup, graph, peak_tf, flop_mult, per_layer="", net=None, parity=False, winograd=None,
                      dump=""):
    """test.py:67-86 path: eval-mode BatchNorm folded into the GEMM epilogues, img -> dense map -> joints.  Returns images/s, ms per
    batch and the fraction of the MFMA roofline (algorithmic conv FLOPs of the forward / time / peak).  dump: directory that receives
    the joints of the last timed call."""
    from awr_amd.trainer import InferEngine
    ks = 1.0 if net_name.startswith("resnet") else 0.4
    if net is None:
        torch.manual_seed(0)
        net = _make_net(awr_amd, net_name).cuda()
    inf = InferEngine(net, batch, 128, ks, use_graph=graph, parity=parity, winograd=winograd)
    imgs, _ = O.synth_batch(batch, 128, 14, seed=1234 + rank)
    imgs = imgs.to(dev)
    for _ in range(warmup):
        inf(imgs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        jt = inf(imgs)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if dump:
        _dump_outputs(dump, {"jt_uvd_pred": jt})
    macs = sum(v for k, v in inf.plan.macs.items())
    if per_layer:
        per = {}
        for _ in range(5):
            for n, sec in inf.plan.timed("fwd", True).items():
                d = per.setdefault(n, [0.0, 0])
                d[0] += sec
                d[1] += 1
        with open(per_layer, "w") as f:
            f.write("%-52s %10s %10s %8s\n" % ("launch", "avg_us", "GFLOP", "TFLOP/s"))
            for n, (sec, c) in sorted(per.items(), key=lambda kv: -kv[1][0]):
                mc = inf.plan.macs.get(n, 0)
                cnt = inf.plan.timed_counts.get(n, 1)      # (element-wise launches share a name: total per forward, launches per forward)
                f.write("%-52s %10.1f %10.2f %8.1f%s\n" % (n, 1e6 * sec / c, 2e-9 * mc, 2e-12 * mc * c / max(sec, 1e-12), "" if cnt == 1 else "   x%d" % cnt))
    return {"workload": "%s eval forward + head (img -> joints), batch %d" % (net_name, batch), "value": round(batch * steps / el, 2), "unit": "images/s",
            "ms_per_step": round(1e3 * el / steps, 3), "steps": steps, "hipgraph": bool(graph),
            "algorithmic_gflop_per_image": round(2e-9 * macs / batch, 3),
            "mfma_frac": round(flop_mult * 2 * macs / (el / steps) / 1e12 / peak_tf, 4)}


def measure_train(awr_amd, O, net_name, J, H, batch, ks, dev, steps, warmup, peak_tf, workload, accum="auto", winograd=None):
    """Sub-record for one more single-GPU BASELINE training shape (same protocol as the headline: inputs resident in HBM, `warmup` untimed
    steps, `steps` steps between two synchronisations, the FULL fused step -- GT map, forward, head, Huber, backward, Adam)."""
    import time as _t
    from awr_amd.trainer import TrainEngine
    torch.manual_seed(0)
    net = (awr_amd.get_deconv_net(18, J, 2) if net_name.startswith("resnet") else awr_amd.PoseNet(net_name, J)).cuda()
    eng = TrainEngine(net, batch, H, ks, coord_weight=0.0, dense_weight=1.0, lr=1e-3, use_graph=False, accum=accum, winograd=winograd)
    img, jt = O.synth_batch(batch, H, J, seed=977)
    img, jt = img.to(dev), jt.to(dev)
    eng.compile(img, jt)
    for _ in range(warmup):
        eng.step(img, jt)
    torch.cuda.synchronize()
    t0 = _t.perf_counter()
    for _ in range(steps):
        eng.step(img, jt)
    torch.cuda.synchronize()
    dt = (_t.perf_counter() - t0) / steps
    macs = float(sum(eng.plan.macs.values()))
    loss = float(eng.losses[2])
    rec = {"workload": workload, "value": round(batch / dt, 2), "unit": "images/s", "ms_per_step": round(1e3 * dt, 3), "steps": steps, "warmup": warmup,
           "plan_gb": round(eng.plan.bytes / 1e9, 1), "algorithmic_gflop_per_image": round(2e-9 * macs / batch, 3),
           "step_mfma_frac": round(2.0 * macs / dt / 1e12 / peak_tf, 4), "final_loss": loss, "loss_finite": bool(loss == loss and abs(loss) < 1e30)}
    if eng.plan.n_winograd:
        # Winograd F(2x2, 3x3) forward launches execute 16 / 36 of their algorithmic multiplies: BOTH fractions are stated -- step_mfma_frac above is
        # algorithmic FLOPs over the FP32-MFMA peak (it may legitimately exceed what the pipe executed), step_mfma_frac_executed what the matrix pipe ran
        executed = macs - eng.plan.winograd_macs * (1.0 - 16.0 / 36.0)
        rec.update({"winograd_launches": int(eng.plan.n_winograd), "winograd_algorithmic_gflop_per_image": round(2e-9 * eng.plan.winograd_macs / batch, 3),
                    "mfma_flops_per_algorithmic_flop": round(executed / macs, 4), "step_mfma_frac_executed": round(2.0 * executed / dt / 1e12 / peak_tf, 4)})
    del eng, net
    import gc
    gc.collect()                 # (plans are freed by their finalisers: a 152 GB config-5 plan must be gone before the next one is built)
    torch.cuda.empty_cache()
    return rec


def _spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N rank processes ourselves (one per GPU, RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* in their environment, exactly what torch.distributed.run would set), let rank 0 write the JSON line to our stdout, wait for all
    of them and return the worst exit code."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), AWR_LAUNCHER="bench.py (self-spawned ranks)")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    try:
        while procs:
            for p in list(procs):
                c = p.poll()
                if c is None:
                    continue
                procs.remove(p)
                if c != 0:              # a dead rank leaves the others hanging in a collective: take them down
                    rc = rc or c
                    for q in procs:
                        q.terminate()
            time.sleep(0.05)
    finally:
        for q in procs:
            q.kill()
    return rc


def _cpulist(text):
    cpus = set()
    for part in text.strip().split(","):
        if part:
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
    return cpus


def _pin_cpu_affinity(dev, local, nlocal):
    """N > 1: keep the rank process (its launch thread issues ~190 launches per step) on the CPUs of its GPU's NUMA node -- the node the PCI
    device reports under /sys; when the platform reports none (-1), an equal contiguous share of the allowed CPUs per local rank.  Returns
    what was done (it goes into the line's `ranks_seen`)."""
    try:
        allowed = os.sched_getaffinity(0)
        pr = torch.cuda.get_device_properties(dev)
        node, src = -1, None
        bus, devid, dom = getattr(pr, "pci_bus_id", None), getattr(pr, "pci_device_id", None), getattr(pr, "pci_domain_id", 0)
        if bus is not None and devid is not None:
            src = "/sys/bus/pci/devices/%04x:%02x:%02x.0/numa_node" % (int(dom), int(bus), int(devid))
            if os.path.exists(src):
                node = int(open(src).read().strip())
        cpus = set()
        if node >= 0:
            cpus = _cpulist(open("/sys/devices/system/node/node%d/cpulist" % node).read()) & allowed
        if not cpus:          # no NUMA information: contiguous shares of what the launcher allowed
            al = sorted(allowed)
            per = max(1, len(al) // max(nlocal, 1))
            cpus, src = set(al[local * per:(local + 1) * per]) or allowed, "equal share of the %d allowed CPUs" % len(al)
        os.sched_setaffinity(0, cpus)
        return {"numa_node": node if node >= 0 else None, "n_cpus": len(cpus), "first_cpu": min(cpus), "source": src}
    except Exception as e:          # never fatal: an unpinned rank is slower, not wrong
        return {"numa_node": None, "error": "%s: %s" % (type(e).__name__, e)}


def _ranks_seen(pg, dev, extra=None):
    """What actually ran: every rank's (rank, device index, device name, uuid / PCI bus id, pid), all-gathered."""
    pr = torch.cuda.get_device_properties(dev)
    me = {"rank": int(os.environ.get("RANK", "0")), "device": dev.index, "name": pr.name, "pid": os.getpid()}
    for k in ("uuid", "pci_bus_id", "pci_device_id", "gcnArchName"):
        v = getattr(pr, k, None)
        if v is not None:
            me[k] = str(v)
    if extra:
        me.update(extra)
    if pg is None:
        return [me]
    out = [None] * torch.distributed.get_world_size(pg)
    torch.distributed.all_gather_object(out, me, group=pg)
    return out


def _replicas_equal(net):
    """Data parallel: True when every rank holds bitwise-identical active parameters (max == min over the ranks, element-wise)."""
    flat = net.flat_params()[:net.n_active]
    mx, mn = flat.clone(), flat.clone()
    torch.distributed.all_reduce(mx, op=torch.distributed.ReduceOp.MAX)
    torch.distributed.all_reduce(mn, op=torch.distributed.ReduceOp.MIN)
    return bool(torch.equal(mx, mn))


def _rccl_version():
    try:
        v = torch.cuda.nccl.version()
        return ".".join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)
    except Exception:
        return None


DUMP_LIMIT_BYTES = 64 << 20
PARAM_SAMPLE = 1 << 20          # parameters dumped per run: a fixed, seeded sample (a ResNet18-deconv arena alone is ~60 MB)


def _sample_index(n, k, seed=0):
    """Fixed, seeded choice of min(n, k) of n positions, ascending (the same positions in every run and every build)."""
    if n <= k:
        return torch.arange(n)
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(n, generator=g)[:k].sort().values


def _engine_state(eng, net):
    """Copies of everything a train step reads and updates: parameters, gradients, BatchNorm running statistics and counters, the
    optimiser's moments and its step count."""
    return [t.clone() for t in _state_tensors(eng, net)], eng.step_count


def _state_tensors(eng, net):
    return [t for t in (net.flat_params(), net.flat_grads(), net._barena, net._counters, eng.m, eng.v) if t is not None]


def _set_engine_state(eng, net, state):
    """Put a state taken by _engine_state back, in place (plans and captured graphs keep their pointers)."""
    saved, count = state
    for dst, src in zip(_state_tensors(eng, net), saved):
        dst.copy_(src)
    eng.step_count = count
    net.weights_changed()


def _train_outputs(eng, net):
    """What a caller of the train step holds after it: the losses [coord, dense, total] and the predicted joints the step returns,
    and the parameters (seeded sample) and BatchNorm running statistics it updated in place."""
    params = net.flat_params()[:net.n_active]
    idx = _sample_index(params.numel(), PARAM_SAMPLE).to(params.device)
    return {"losses": eng.losses, "jt_uvd_pred": eng.jt_pred, "params_sample": params[idx], "bn_running_stats": net._barena}


def _dump_outputs(dirname, arrays):
    """Write {name: tensor} as dirname/<name>.npy: float64 stays float64, everything else becomes float32.  Fails when the total
    would exceed DUMP_LIMIT_BYTES."""
    import numpy as np
    host = {}
    for name, t in arrays.items():
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        host[name] = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("--dump-outputs: %d bytes exceed the %d-byte limit" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(dirname, exist_ok=True)
    for name, a in host.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    return sorted(host)


def _roofline_blocks(args, eng, net, elapsed, nprod, peak_tf, flop_mult, rank):
    """--full / --per-layer: the per-kernel MFMA roofline of the conv launches and the HBM roofline of the head / loss / optimiser launches,
    both from serialised event passes after the timed steps.  -> (roofline, roofline_hbm, conv FLOPs of the passes, passes)."""
    # per-kernel HIP events only make sense when kernels do not share the GPU: the timed region runs untouched (side streams /
    # graph replay) and the per-kernel roofline comes from serialised passes of the same plan right after it
    per = {}
    for _ in range(3):
        for n, sec in eng.timed_core(every=bool(args.per_layer)).items():
            d = per.setdefault(n, [0.0, 0])
            d[0] += sec
            d[1] += 1
    torch.cuda.synchronize()
    macs = eng.plan.macs
    fam = {"conv_gemm_kernel(fwd+dgrad)": ("awr_conv_gemm:", "awr_conv_dgrad:"), "conv_wgrad_kernel": ("awr_conv_wgrad:",),
           "stem kernels (fused direct 5x5 conv+BN+ReLU+pool, fwd+bwd incl. recomputation)": ("awr_stem_",)}
    per_all = dict(per)
    per = {n: v for n, v in per.items() if n in macs}
    kern = {}
    for label, prefixes in fam.items():
        fl = sum(2.0 * macs[n] * c for n, (sec, c) in per.items() if n.startswith(prefixes))
        sec = sum(s for n, (s, c) in per.items() if n.startswith(prefixes))
        cnt = sum(c for n, (s, c) in per.items() if n.startswith(prefixes))
        kern[label] = {"tflops": fl / sec / 1e12 if sec else 0.0, "seconds": sec, "launches": cnt, "avg_us": 1e6 * sec / max(cnt, 1), "flops": fl}
    if args.per_layer and rank == 0:
        with open(args.per_layer, "w") as f:
            f.write("%-52s %10s %10s %8s\n" % ("launch", "avg_us", "GFLOP", "TFLOP/s"))
            for n, (sec, c) in sorted(per.items(), key=lambda kv: -kv[1][0]):
                f.write("%-52s %10.1f %10.2f %8.1f\n" % (n, 1e6 * sec / c, 2e-9 * macs[n], 2e-12 * macs[n] * c / sec))
            f.write("\nall other launches of the plan (serial replay, same event pass): total us per step, launches per step\n")
            tot_other = 0.0
            for n, (sec, c) in sorted(per_all.items(), key=lambda kv: -kv[1][0]):
                if n not in macs:
                    f.write("%-52s %10.1f %6d\n" % (n, 1e6 * sec / c, eng.plan.timed_counts.get(n, 1)))
                    tot_other += 1e6 * sec / c
            f.write("%-52s %10.1f\n" % ("sum", tot_other))
    dom = max(kern, key=lambda k: kern[k]["seconds"])
    tot_fl = sum(k["flops"] for k in kern.values())
    tot_sec = sum(k["seconds"] for k in kern.values())
    nsteps_timed = next(iter(per.values()))[1] if per else 1
    # HBM bytes per launch of the dominant kernel family: PMC passes (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE,
    # separate rocprofv3 --pmc runs of this same command: tools/gpu_pmc.sh) cannot be collected from inside the
    # process, so the committed summary of the last PMC run is reported (null when absent).
    traffic, traffic_src = None, None
    tfiles = sorted(f for f in os.listdir(os.path.join(REPO, "profiles")) if f.endswith("_hbm_traffic_pmc.json"))
    tpath = os.path.join(REPO, "profiles", tfiles[-1]) if tfiles else ""
    if tpath and args.net == "resnet_18" and args.batch == 64 and nprod == 1:      # the PMC passes profile exactly this command
        tj = json.load(open(tpath))
        keys = ("conv_gemm_kernel", "conv_gemm_dma_kernel") if dom.startswith("conv_gemm") else ("conv_wgrad_kernel", "conv_wgrad_dma_kernel", "conv_wgrad_row_kernel")
        ent = [v for k, v in tj.items() if any(key in k for key in keys)]
        nl = sum(v["launches"] for v in ent)
        if nl:
            traffic = round(sum(v["launches"] * (v["fetch_MB_per_launch_x2"] + v["write_MB_per_launch"]) for v in ent) / nl * 1e6)
            traffic_src = "profiles/%s (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, FETCH x2 per the gfx950 note, bytes per launch)" % os.path.basename(tpath)
    roofline = {
        "bound": "mfma", "kernel": dom, "event_pass": "serialised replay of the same plan right after the timed region (awr_plan_run_timed: a HIP-event pair around every launch; in the timed region kernels overlap on side streams)",
        "achieved": round(flop_mult * kern[dom]["tflops"], 2), "peak": peak_tf, "unit": "TFLOP/s", "mfma_flops_per_algorithmic_flop": flop_mult,
        "frac": round(flop_mult * kern[dom]["tflops"] / peak_tf, 4), "traffic": traffic, "traffic_source": traffic_src,
        "algorithmic_flop_per_launch": round(kern[dom]["flops"] / max(kern[dom]["launches"], 1)),
        "avg_launch_us": round(kern[dom]["avg_us"], 2), "launches_per_step": kern[dom]["launches"] // max(nsteps_timed, 1),
        # HBM rate of the dominant kernel: PMC bytes per launch over the live average launch time, against the 8 TB/s HBM3E figure
        "hbm_gbps": round(traffic / (kern[dom]["avg_us"] * 1e-6) / 1e9, 1) if traffic and kern[dom]["avg_us"] else None, "hbm_peak_gbps": 8000.0,
        "all_gemm_tflops": round(tot_fl / tot_sec / 1e12, 2) if tot_sec else 0.0,
        "gemm_seconds_per_step": round(tot_sec / max(nsteps_timed, 1), 6),
        "algorithmic_gflop_per_image": round(tot_fl / max(nsteps_timed, 1) / args.batch / 1e9, 3),
        "other_kernels": {k: {"tflops": round(v["tflops"], 2), "avg_us": round(v["avg_us"], 2)} for k, v in kern.items() if k != dom},
        "step_mfma_frac": round(flop_mult * (tot_fl / max(nsteps_timed, 1)) / (elapsed / args.steps) / 1e12 / peak_tf, 4),
    }

    # HBM-bound kernels of the step that live outside the plan: serial event passes, algorithmic bytes per launch
    hb = eng.timed_hbm()
    B_, J_, P_ = args.batch, 14, 64 * 64
    pred_b, depth_b = 4 * J_ * P_ * 4, P_ * 4
    alg = {"head_forward_nhwc": ("a4 offset2joint_softmax", B_ * (pred_b + depth_b + J_ * 12)),
           "head_forward": ("a4 offset2joint_softmax", B_ * (pred_b + depth_b + J_ * 12)),
           "head_backward": ("a5 head backward", B_ * (2 * pred_b + depth_b)),
           "dense_loss": ("a6+a7 GT map + dense Huber fwd+bwd", B_ * (2 * pred_b + depth_b)),
           # one pass does a4's partials AND a6+a7 (coord_weight 0) -- priced at the bytes that pass has to move (map in, gradient out);
           # with a coordinate loss the map is read twice (partials, then dense loss + head backward)
           "head_loss_step_nhwc": ("a4 + a6+a7 (+ a5 when coord_weight != 0) in one call", B_ * ((2 if args.coord_weight == 0.0 else 3) * pred_b + depth_b)),
           "adam_step": ("a8 Adam, 28 B / parameter", 28 * int(net.n_active))}
    roofline_hbm = {k: {"covers": alg[k][0], "bytes_algorithmic": alg[k][1], "avg_us": round(1e6 * v, 2), "gbps": round(alg[k][1] / v / 1e9, 1),
                        "frac_of_8TBps": round(alg[k][1] / v / 8e12, 4)} for k, v in hb.items() if k in alg}
    return roofline, roofline_hbm, tot_fl, nsteps_timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="images per GPU per step (BASELINE configs[1]: 64)")
    ap.add_argument("--net", default="resnet_18")
    ap.add_argument("--graph", action="store_true",
                    help="replay the step as ONE hipGraph (weight-gradient side streams forked / joined inside the capture) instead of issuing every launch "
                         "eagerly.  Measured slower on this stack (15.80 vs 14.93 ms / step, profiles/r02_summary.md): the eager two-stream issue stays the default")
    ap.add_argument("--no-extras", action="store_true", help="skip the inference / config-3 measurements reported under 'forward' and 'config3'")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the small HIP-vs-oracle joint check (keeps profiler traces to the timed workload)")
    ap.add_argument("--coord-weight", type=float, default=0.0, help="reference default config.py:41")
    ap.add_argument("--mode", default="train", choices=["train", "infer"], help="infer = test.py:67-86 path (eval BN, img -> joints); not the headline metric")
    ap.add_argument("--wgrad-streams", type=int, default=2, help="extra HIP streams for the weight-gradient GEMMs (0 = fully serial step)")
    ap.add_argument("--gemm-products", type=int, default=1, choices=[1, 6],
                    help="1 = FP32 MFMA (default, the headline); 6 = split-operand mode (fp32 operands as 3 exact bf16 pieces, 6 bf16 MFMA products)")
    ap.add_argument("--no-split-mode", action="store_true", help="skip the extra split-operand measurement reported under 'split_mode'")
    ap.add_argument("--per-layer", default="", help="write a per-GEMM-launch table (TFLOP/s per layer) to this file")
    ap.add_argument("--dp-selftest", action="store_true", help="data parallel: fail unless all replicas hold bitwise-identical parameters after the timed steps; "
                                                               "the per-bucket all-reduce timeline is reported either way when N > 1")
    ap.add_argument("--no-hourglass-train", action="store_true", help="skip the Hourglass training sub-records 'hg1_train_b64' and 'config5'")
    ap.add_argument("--no-b256", action="store_true", help="skip the config-4 per-GPU shape (batch 256) sub-record")
    ap.add_argument("--no-data-path", action="store_true", help="skip the 'data_path' sub-record (host loader vs device loader, train step fed by the device path)")
    ap.add_argument("--no-winograd", action="store_true", help="skip the 'winograd_mode' sub-record (Winograd F(2x2, 3x3) forward of the 3x3 convolutions)")
    ap.add_argument("--no-accurate-mode", action="store_true", help="skip the blocked-accumulation (parity mode) sub-record 'accurate_mode'")
    ap.add_argument("--no-native-rccl", action="store_true", help="N > 1: skip the 'native_rccl' sub-record (same steps, gradient buckets exchanged by the "
                                                                  "library's own RCCL communicator instead of torch.distributed work objects)")
    ap.add_argument("--deterministic", action="store_true", help="awr_amd.set_deterministic(True): bitwise-reproducible steps (no atomics on shared "
                                                                  "accumulators, no autotuning); reports what that costs")
    ap.add_argument("--full", action="store_true", help="after the headline, run every other measurement and check of the benchmark (roofline blocks, "
                                                        "oracle parity, CPU baseline, sub-records; N > 1: replica check, bucket timeline, transport A/B)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write what the timed path computes from the seeded starting state (train: "
                                                                      "its step, run once more after the timing; infer: the last timed call) to "
                                                                      "DIR/<name>.npy (float32 / float64, at most 64 MB in all)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(_spawn_ranks(args.gpus))          # plain `python bench.py --gpus N`: be our own launcher
    # stdout carries exactly ONE line, the JSON record: libraries that print banners on file descriptor 1 (RCCL's version block at
    # communicator creation) are sent to stderr for the duration of the run
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    def emit(line):
        os.write(real_stdout, (line + "\n").encode())
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("AWR_FORCE_DEVICE", os.environ.get("LOCAL_RANK", "0")))     # AWR_FORCE_DEVICE: test hook (several ranks on one GPU)
    if args.gpus != world and not (world == 1 and os.environ.get("AWR_FORCE_DP") == "1"):
        raise SystemExit("--gpus %d but the launcher started %d rank(s)" % (args.gpus, world))
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    affinity = None
    if world > 1 and os.environ.get("AWR_NO_AFFINITY") != "1":
        affinity = _pin_cpu_affinity(dev, int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("LOCAL_WORLD_SIZE", str(world))))
    pg, backend = None, None
    if world > 1 or os.environ.get("AWR_FORCE_DP") == "1":      # AWR_FORCE_DP: exercise the data-parallel path on a 1-rank group (tests)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("AWR_DIST_BACKEND", "nccl")        # "nccl" is RCCL on ROCm; tests run the same path over gloo on one GPU
        torch.distributed.init_process_group(backend, rank=rank, world_size=world, **({"device_id": dev} if backend == "nccl" else {}))
        pg = torch.distributed.group.WORLD

    import awr_amd
    from awr_amd import _lib as L
    from awr_amd.trainer import TrainEngine
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import awr_oracle as O          # synthetic-input generator + cpu_baseline only; never on the measured path

    ks = 1.0 if args.net.startswith("resnet") else 0.4          # config.py:42
    awr_amd.set_gemm_products(args.gemm_products)
    awr_amd.set_deterministic(args.deterministic)
    nprod = args.gemm_products
    dtype = "f32" if nprod == 1 else "f32 (operands as 3 exact bf16 pieces, 6 bf16 MFMA products per f32 product, f32 accumulate)"
    # MFMA roofline of the mode: FP32 MFMA peak, or the bf16 dense peak against 6 MFMA flops per algorithmic flop
    peak_tf, flop_mult = (PEAK_FP32_MFMA_TFLOPS, 1) if nprod == 1 else (PEAK_BF16_MFMA_TFLOPS, 6)
    torch.manual_seed(0)
    net = _make_net(awr_amd, args.net).cuda()
    if args.mode == "infer":
        res = measure_inference(awr_amd, O, args.net, args.batch, dev, rank, args.steps, max(args.warmup, 3), args.graph, peak_tf, flop_mult,
                                per_layer=args.per_layer, net=net, dump=args.dump_outputs if rank == 0 else "")
        emit(json.dumps({"metric": "depth-images/sec (inference, img -> joints)", "value": res["value"], "unit": "images/s",
                          "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": res["ms_per_step"],
                          "dtype": dtype, "data": "synthetic", "config": {"workload": res["workload"], "hipgraph": bool(args.graph), "gemm_products": nprod},
                          "mfma_frac": res["mfma_frac"]}))
        return
    def sync():
        torch.cuda.synchronize()
        if pg is not None:
            torch.distributed.barrier()

    def timed_steps(engine, im, jg, steps, warm):
        """W untimed steps, then EXACTLY `steps` steps between barrier + synchronize on both sides; the MAX over ranks."""
        for _ in range(warm):
            engine.step(im, jg)
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            engine.step(im, jg)
        sync()
        el = time.perf_counter() - t0
        if pg is not None:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            el = float(t[0])
        return el

    eng = TrainEngine(net, args.batch, 128, ks, coord_weight=args.coord_weight, dense_weight=1.0, lr=1e-3, process_group=pg,
                      use_graph=args.graph, wgrad_streams=args.wgrad_streams)
    img, jt = O.synth_batch(args.batch, 128, 14, seed=1234 + rank)
    img, jt = img.to(dev), jt.to(dev)           # inputs resident in HBM before the timed region
    graph = bool(eng.use_graph)          # the engine falls back to eager issue in data-parallel mode (RCCL calls inside the backward)
    eng.compile(img, jt)                 # set-up, not a step: kernel warm-up run (rolled back), GEMM tile autotune, hipGraph capture
    start = _engine_state(eng, net) if args.dump_outputs else None
    warm = args.warmup
    elapsed = timed_steps(eng, img, jt, args.steps, warm)
    loss = float(eng.losses[2])
    if start is not None:
        # The timed steps train on one batch over and over, and the default mode sums split-K weight gradients with atomics: their last-bit
        # differences grow about tenfold per Adam step, and after 25 steps two runs disagree on the joints by ~5 %.  So the dump is the timed
        # path's step taken from the seeded starting state (same engine, plan and inputs), run once more after the timing; every rank takes
        # part (the all-reduce is part of the step), and the state after the timed steps is put back before anything else runs.
        end = _engine_state(eng, net)
        _set_engine_state(eng, net, start)
        eng.step(img, jt)
        if rank == 0:
            _dump_outputs(args.dump_outputs, _train_outputs(eng, net))
        _set_engine_state(eng, net, end)
        del start, end
    ranks_seen = _ranks_seen(pg, dev, {"cpu_affinity": affinity} if affinity is not None else None)
    full = args.full

    # data-parallel self-test (after the timed region): replicas must hold bitwise-identical parameters after all those steps (every rank
    # stepped its own images; the all-reduced gradients and the optimiser are what keeps them together), and one traced step shows where
    # each bucket's exchange sat relative to the backward
    selftest = None
    if pg is not None and (args.dp_selftest or (full and world > 1)):
        same = _replicas_equal(net)
        eng.trace_buckets = True
        eng.step(img, jt)
        tl = eng.bucket_timeline()
        eng.trace_buckets = False
        selftest = {"replicas_bitwise_equal_after_steps": same, "steps_checked": warm + args.steps, "n_params": int(net.n_active),
                    "bucket_timeline_rank0": tl, "note": "timeline of one extra traced step: ms from the start of the step on the stream each bucket was handed to; "
                                                         "tracing makes that stream wait for its collective"}
        if args.dp_selftest and not same:
            raise SystemExit("dp-selftest: parameters differ across ranks after %d steps" % (warm + args.steps))

    roofline = roofline_hbm = None
    tot_fl, nsteps_timed = 0.0, 1
    if full or args.per_layer:
        roofline, roofline_hbm, tot_fl, nsteps_timed = _roofline_blocks(args, eng, net, elapsed, nprod, peak_tf, flop_mult, rank)

    if rank == 0:
        n_cu, mhz = L.C.c_int(0), L.C.c_int(0)
        L.lib.awr_device_info(L.C.byref(n_cu), L.C.byref(mhz), None, 0)
        out = {
            "metric": "depth-images/sec (train step)", "value": round(world * args.batch * args.steps / elapsed, 2), "unit": "images/s",
            "n_gpus": world, "steps": args.steps, "warmup": warm, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
            "config": {"workload": "%s-deconv NYU-shape 128x128 J=14 train step (GT-map+fwd+head+Huber+bwd+Adam), batch %d/GPU%s" % (
                           args.net, args.batch, {64: " = BASELINE configs[1]", 256: " = BASELINE configs[3] per-GPU shape"}.get(args.batch, "") if args.net == "resnet_18" else "")
                       if args.net.startswith("resnet") else "%s NYU-shape 128x128 J=14 train step, batch %d/GPU" % (args.net, args.batch),
                       "global_batch": world * args.batch, "img_size": 128, "joints": 14, "parallelism": "dp%d" % world,
                       "kernel_size": ks, "coord_weight": args.coord_weight, "dense_weight": 1.0, "hipgraph": graph, "wgrad_streams": args.wgrad_streams, "independent_hw_queues_for_side_streams": _pool_info(L),
                       "gemm_products": nprod, "deterministic": bool(args.deterministic), "device_cus": n_cu.value, "final_loss": loss,
                       "nhwc_head_loss": bool(eng.nhwc), "launcher": os.environ.get("AWR_LAUNCHER", "torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ else "direct")},
            "dist_backend": backend, "rccl_version": _rccl_version() if backend == "nccl" else None, "ranks_seen": ranks_seen,
        }
        if roofline is not None:
            out["roofline"], out["roofline_hbm"] = roofline, roofline_hbm
        if selftest is not None:
            out["dp_selftest"] = selftest
        if full and world == 1 and not args.no_parity:
            mean_mm, max_mm = parity_mm(args.net, ks, dev)
            out["joint_err_mm_vs_oracle"] = {"mean": round(mean_mm, 6), "max": round(max_mm, 6)}
            if not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline()
    # config 4's per-GPU shape (batch 256 / GPU: north_star states its scaling target there) beside the batch-64 headline, same protocol,
    # every rank takes part (the all-reduce is part of the step)
    b256 = None
    if full and args.batch != 256 and args.net == "resnet_18" and nprod == 1 and not args.no_b256 and not args.deterministic:
        del eng
        torch.cuda.empty_cache()
        eng2 = TrainEngine(net, 256, 128, ks, coord_weight=args.coord_weight, dense_weight=1.0, lr=1e-3, process_group=pg, use_graph=args.graph,
                           wgrad_streams=args.wgrad_streams)
        im2, jt2 = O.synth_batch(256, 128, 14, seed=4321 + rank)
        im2, jt2 = im2.to(dev), jt2.to(dev)
        eng2.compile(im2, jt2)
        k2 = max(4, min(args.steps, 10))
        el2 = timed_steps(eng2, im2, jt2, k2, 3)
        b256 = {"workload": "resnet_18-deconv train step, batch 256/GPU = BASELINE configs[3] per-GPU shape", "value": round(world * 256 * k2 / el2, 2), "unit": "images/s",
                "n_gpus": world, "steps": k2, "warmup": 3, "ms_per_step": round(1e3 * el2 / k2, 3), "plan_gb": round(eng2.plan.bytes / 1e9, 1),
                "step_mfma_frac": round(flop_mult * (tot_fl / max(nsteps_timed, 1)) * (256 / args.batch) / (el2 / k2) / 1e12 / peak_tf, 4)}
        # the HBM-bound head / loss launches at the batch where they have work (batch 64 moves 118 MB in 35 us: launch-ramp-bound)
        hb2 = eng2.timed_hbm()
        pb2, db2 = 4 * 14 * 64 * 64 * 4, 64 * 64 * 4
        alg2 = {"head_forward_nhwc": 256 * (pb2 + db2 + 14 * 12), "head_forward": 256 * (pb2 + db2 + 14 * 12), "head_backward": 256 * (2 * pb2 + db2),
                "dense_loss": 256 * (2 * pb2 + db2), "head_loss_step_nhwc": 256 * ((2 if args.coord_weight == 0.0 else 3) * pb2 + db2)}
        b256["roofline_hbm"] = {k: {"bytes_algorithmic": alg2[k], "avg_us": round(1e6 * v, 2), "gbps": round(alg2[k] / v / 1e9, 1), "frac_of_8TBps": round(alg2[k] / v / 8e12, 4)}
                                for k, v in hb2.items() if k in alg2}
        if pg is not None:          # north_star's scaling target is stated at this shape: the replicas must still agree bit for bit after its steps
            b256["dp_selftest"] = {"replicas_bitwise_equal_after_steps": _replicas_equal(net), "steps_checked": k2 + 3}
        del eng2
        eng = None
        torch.cuda.empty_cache()
    # N > 1: the same K steps with the gradient buckets exchanged by the library's own RCCL communicator (awr_dp_*: ncclAllReduce issued from
    # inside the native backward replay, no Python callback per bucket) -- the A/B of the two transports in ONE run of the 8-GPU node
    native = None
    if full and pg is not None and nprod == 1 and not args.no_native_rccl and not args.deterministic:
        if backend != "nccl":
            native = {"skipped": "dist backend %r: the library's communicator is RCCL (one GPU per rank)" % backend}
        else:
            # This block runs code no multi-rank RCCL job has executed before (ncclCommInitRank from the library, collectives issued from the
            # native replay): the measured headline must not be lost to a hang in it.  A watchdog emits the line without the A/B and ends the
            # process when the block overruns its allowance (every rank arms one; rank 0 writes).
            import threading

            def _overrun():
                if rank == 0:
                    out["native_rccl"] = {"error": "did not finish within %d s: abandoned by the watchdog, headline unaffected" % native_allowance}
                    if b256 is not None:
                        out["b256"] = b256
                    emit(json.dumps(out))
                os._exit(0)
            native_allowance = int(os.environ.get("AWR_NATIVE_RCCL_ALLOWANCE_S", "180"))
            dog = threading.Timer(native_allowance, _overrun)
            dog.daemon = True
            dog.start()
            try:
                eng = None
                torch.cuda.empty_cache()
                eng3 = TrainEngine(net, args.batch, 128, ks, coord_weight=args.coord_weight, dense_weight=1.0, lr=1e-3, process_group=pg,
                                   use_graph=False, wgrad_streams=args.wgrad_streams, native_rccl=True)
                eng3.compile(img, jt)
                el3 = timed_steps(eng3, img, jt, args.steps, warm)
                native = {"transport": "library-owned RCCL communicator (awr_dp_*, csrc/awr_dp.hip); the headline value uses torch.distributed work objects",
                          "value": round(world * args.batch * args.steps / el3, 2), "unit": "images/s", "n_gpus": world, "steps": args.steps,
                          "warmup": warm, "ms_per_step": round(1e3 * el3 / args.steps, 3), "vs_headline": round(elapsed / el3, 4),
                          "dp_selftest": {"replicas_bitwise_equal_after_steps": _replicas_equal(net), "steps_checked": warm + args.steps}}
                del eng3
            except Exception as e:          # (the headline has been measured: report, do not lose the line)
                native = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
            dog.cancel()
            torch.cuda.empty_cache()
    if rank == 0:
        if b256 is not None:
            out["b256"] = b256
        if native is not None:
            out["native_rccl"] = native
        if full and world == 1 and not args.no_extras:
            # north_star's forward target (>= 40 % MFMA utilisation on the ResNet18-deconv forward) and BASELINE config 3, each ~1 s,
            # outside the timed train region
            eng = None
            torch.cuda.empty_cache()
            out["forward"] = {"b%d" % b: measure_inference(awr_amd, O, "resnet_18", b, dev, rank, 30, 5, args.graph, peak_tf, flop_mult) for b in (64, 128)}
            out["config3"] = measure_inference(awr_amd, O, "hourglass_1", 128, dev, rank, 20, 5, args.graph, peak_tf, flop_mult)
            if nprod == 1 and not args.no_hourglass_train:
                # the two Hourglass TRAINING shapes: Hourglass-1 at the headline batch, and BASELINE configs[4]'s per-GPU
                # shape (Hourglass-2, 256x256, 21 joints, 128 images: ~150 GB of plan buffers on one MI355X, ~0.3 s per step)
                out["hg1_train_b64"] = measure_train(awr_amd, O, "hourglass_1", 14, 128, 64, 0.4, dev, 10, 3, peak_tf,
                                                     "hourglass_1 NYU-shape 128x128 J=14 train step, batch 64")
                try:
                    out["config5"] = measure_train(awr_amd, O, "hourglass_2", 21, 256, 128, 0.4, dev, 5, 3, peak_tf,
                                                   "hourglass_2 256x256 J=21 train step, batch 128/GPU = BASELINE configs[4] per-GPU shape")
                except Exception as e:      # (a 152 GB plan: if another process holds memory on this GPU, keep the line)
                    out["config5_error"] = "%s: %s" % (type(e).__name__, str(e)[:200])
                    import gc
                    gc.collect()
                    torch.cuda.empty_cache()
        if full and world == 1 and nprod == 1 and not args.no_data_path and args.net == "resnet_18" and args.batch == 64 and not args.deterministic:
            eng = None
            torch.cuda.empty_cache()
            try:
                out["data_path"] = measure_data_path(awr_amd, O, dev, out["ms_per_step"], max(args.steps, 20), 5)
            except Exception as e:          # (the headline has been measured: report, do not lose the line)
                out["data_path"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        if full and world == 1 and nprod == 1 and not args.no_winograd and not args.deterministic:
            # Winograd F(2x2, 3x3) modes of the stride-1 3x3 convolutions (awr_amd.set_conv_winograd, opt-in): the headline's step, the Hourglass-1 step and
            # config 5, same protocol
            eng = None
            torch.cuda.empty_cache()
            try:
                wm = {"mode": "eligible stride-1 3x3 convolutions as Winograd F(2x2, 3x3) on v_mfma_f32_32x32x2_f32 (csrc/awr_wino.hip): 'forward' = their forward "
                              "launches, 'forward+wgrad' = forward and weight gradients (the Winograd-domain weight gradient awr_wino_wgrad), 'full' = the data gradients "
                              "too (a Winograd data gradient leaves less room for the weight gradients that run beside it: level with 'forward+wgrad' or a little "
                              "behind); NOT the headline (value above is the direct path)"}
                for k, mode in (("train", True), ("train_fw", "forward+wgrad"), ("train_full", "full")):
                    wm[k] = measure_train(awr_amd, O, args.net, 14, 128, args.batch, ks, dev, args.steps, warm, peak_tf,
                                          "%s train step, batch %d, TrainEngine(winograd=%r)" % (args.net, args.batch, mode), winograd=mode)
                    wm[k]["vs_headline"] = round(wm[k]["value"] / out["value"], 4)
                if args.net == "resnet_18" and not args.no_hourglass_train and "hg1_train_b64" in out:
                    for k, mode in (("hg1_train_b64_fw", "forward+wgrad"), ("hg1_train_b64_full", "full")):
                        wm[k] = measure_train(awr_amd, O, "hourglass_1", 14, 128, 64, 0.4, dev, 10, 3, peak_tf,
                                              "hourglass_1 train step, batch 64, TrainEngine(winograd=%r)" % (mode,), winograd=mode)
                        wm[k]["vs_direct"] = round(wm[k]["value"] / out["hg1_train_b64"]["value"], 4)
                    if args.batch == 64 and not args.no_b256:      # BASELINE configs[3]'s per-GPU shape (layer4's 8 x 8 maps fill the chip from batch 128 on)
                        wm["b256_full"] = measure_train(awr_amd, O, "resnet_18", 14, 128, 256, 1.0, dev, 8, 3, peak_tf,
                                                        "resnet_18 train step, batch 256/GPU, TrainEngine(winograd='full')", winograd="full")
                        if isinstance(out.get("b256"), dict) and out["b256"].get("value"):
                            wm["b256_full"]["vs_direct"] = round(wm["b256_full"]["value"] / out["b256"]["value"], 4)
                    if "config3" in out:      # inference: the folded BatchNorm / residual add in the Winograd epilogue; Hourglass conv2 instead of the fused conv2 + conv3 launch
                        wm["config3"] = measure_inference(awr_amd, O, "hourglass_1", 128, dev, rank, 20, 5, args.graph, peak_tf, flop_mult, winograd=True)
                        wm["config3"]["vs_direct"] = round(wm["config3"]["value"] / out["config3"]["value"], 4)
                        wm["forward_b128"] = measure_inference(awr_amd, O, "resnet_18", 128, dev, rank, 30, 5, args.graph, peak_tf, flop_mult, winograd=True)
                        wm["forward_b128"]["vs_direct"] = round(wm["forward_b128"]["value"] / out["forward"]["b128"]["value"], 4)
                    if "config5" in out:
                        try:
                            wm["config5_fw"] = measure_train(awr_amd, O, "hourglass_2", 21, 256, 128, 0.4, dev, 5, 3, peak_tf,
                                                             "hourglass_2 256x256 J=21 train step, batch 128/GPU, TrainEngine(winograd='forward+wgrad')",
                                                             winograd="forward+wgrad")
                            wm["config5_fw"]["vs_direct"] = round(wm["config5_fw"]["value"] / out["config5"]["value"], 4)
                        except Exception as e:      # (a 152 GB plan: keep the rest of the record if it does not fit)
                            wm["config5_fw"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
            except Exception as e:          # (the headline has been measured: report, do not lose the line)
                wm = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
            out["winograd_mode"] = wm
        if full and world == 1 and nprod == 1 and not args.no_accurate_mode and not args.deterministic:
            # the parity mode (blocked accumulation: awr_conv_args.accum = 1, what Trainer.test scores with and TrainEngine(accum="blocked") trains
            # with): the headline's step at the same batch, the scoring pass at batch 128, and the joint error against the oracle in that mode
            eng = None
            torch.cuda.empty_cache()
            am = {"accum": "blocked (a K extent restarts its rounding chain every 128 terms; DESIGN.md section 5)",
                  "train": measure_train(awr_amd, O, args.net, 14, 128, args.batch, ks, dev, args.steps, warm, peak_tf,
                                         "%s train step, batch %d, TrainEngine(accum='blocked')" % (args.net, args.batch), accum="blocked"),
                  "infer_b128": measure_inference(awr_amd, O, args.net, 128, dev, rank, 20, 5, False, peak_tf, flop_mult, parity=True)}
            am["train"]["vs_headline"] = round(am["train"]["value"] / out["value"], 4)
            if not args.no_parity:
                mean_a, max_a = parity_mm(args.net, ks, dev, parity=True)
                am["joint_err_mm_vs_oracle"] = {"mean": round(mean_a, 6), "max": round(max_a, 6)}
            out["accurate_mode"] = am
        if full and world == 1 and nprod == 1 and not args.no_split_mode:
            # the same K steps in the opt-in split-operand mode (not the headline: `value` above is the FP32-MFMA path)
            awr_amd.set_gemm_products(6)
            torch.manual_seed(0)
            net6 = _make_net(awr_amd, args.net).cuda()
            eng6 = TrainEngine(net6, args.batch, 128, ks, coord_weight=args.coord_weight, dense_weight=1.0, lr=1e-3, use_graph=args.graph,
                               wgrad_streams=args.wgrad_streams)
            eng6.compile(img, jt)
            for _ in range(warm):
                eng6.step(img, jt)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                eng6.step(img, jt)
            torch.cuda.synchronize()
            el6 = time.perf_counter() - t0
            sm = {"gemm_products": 6, "dtype": "f32 operands cut exactly into 3 bf16 pieces, 6 bf16 MFMA partial products per f32 product, f32 accumulate",
                  "value": round(args.batch * args.steps / el6, 2), "unit": "images/s", "ms_per_step": round(1e3 * el6 / args.steps, 3),
                  "final_loss": float(eng6.losses[2]),
                  "step_mfma_frac_of_bf16_peak": round(6 * (tot_fl / max(nsteps_timed, 1)) / (el6 / args.steps) / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4)}
            if not args.no_parity:
                mean6, max6 = parity_mm(args.net, ks, dev)
                sm["joint_err_mm_vs_oracle"] = {"mean": round(mean6, 6), "max": round(max6, 6)}
            awr_amd.set_gemm_products(1)
            out["split_mode"] = sm
        emit(json.dumps(out))
    if pg is not None:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
