#!/usr/bin/env python3
"""Record what the plan engine builds and what a deterministic training step computes (GPU):

    tools/plan_snapshot.py OUT.json
    tools/plan_snapshot.py --wide OUT.json

One record per covered plan -- the forward and backward op names in order with `flags & 3` of awr_plan_op (bit 0 side_ok, bit 1 gemm),
the gradient buckets, n_gemm, n_bn, n_winograd and the plan's bytes -- and one per covered deterministic training run: the bit patterns
of the losses of three steps and the SHA-256 of the parameter arena after the third.  tests/test_plan_schedule_gpu.py compares the
plans and steps of the current build with tests/golden/plan_snapshot.json, which this tool wrote on the commit BEFORE the plan engine's
scheduling moved from op names to op flags; a change that is meant to alter a plan re-records the file and says so.

--wide writes the second record, tests/golden/plan_snapshot_wide.json (tests/test_plan_wide_gpu.py): the launch forms the first one's shape and
networks never reach (WIDE_PLAN_CASES), and per plan everything the introspection entry points list -- the ops with all four flag bits of
awr_plan_op and their MACs, the awr_plan_gemm listing, the buckets, the awr_plan_tensor listing and the counts.  In the file the four lists of a
plan stand as their length and SHA-256 (in full, 27 plans are half a megabyte); wide_plan_records() returns them in full, which is how two builds
are compared entry by entry.  It was written on the commit
BEFORE the plan builder was split into translation units and is never regenerated from a later builder.  Both modes use the public API only.
"""
import ctypes as C
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

B, H, J = 2, 128, 14      # the smallest shape at which both networks fork in the forward and the Hourglass forks in the backward

# (record name, network, training, n_buckets, winograd, split_k, deterministic)
PLAN_CASES = []
for _net in ("resnet_18", "hourglass_1"):
    for _w in ("direct", "force"):
        for _nb in (1, 4):
            PLAN_CASES.append(("%s/train/b%d/%s" % (_net, _nb, _w), _net, True, _nb, _w, None, False))
        PLAN_CASES.append(("%s/eval/%s" % (_net, _w), _net, False, 1, _w, None, False))
PLAN_CASES.append(("resnet_18/train/b1/direct/split_k", "resnet_18", True, 1, "direct", True, False))
PLAN_CASES.append(("resnet_18/train/b1/direct/det", "resnet_18", True, 1, "direct", None, True))

STEP_CASES = [("%s/%s" % (n, m), n, m == "dp") for n in ("resnet_18", "hourglass_1") for m in ("single", "dp")]


def make_net(name, sd=None):
    import awr_amd
    m = awr_amd.get_deconv_net(int(name.split("_")[1]), J, 2) if name.startswith("resnet") else awr_amd.PoseNet(name, J)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.cuda()


def op_flags(plan, which):
    """Raw awr_plan_op flags of every op of list `which` (0 forward, 1 backward)."""
    from awr_amd import _lib as L
    name, macs, flags = C.c_char_p(), C.c_double(), C.c_int()
    out = []
    for i in range(plan.n_ops[which]):
        L.call("awr_plan_op", plan.h, which, i, C.byref(name), C.byref(macs), C.byref(flags))
        out.append((name.value.decode(), flags.value))
    return out


def plan_record(plan):
    return {"fwd": [[n, f & 3] for n, f in op_flags(plan, 0)], "bwd": [[n, f & 3] for n, f in op_flags(plan, 1)],
            "buckets": [list(b) for b in plan.buckets], "n_gemm": plan.n_gemm, "n_bn": plan.n_bn, "n_winograd": plan.n_winograd, "bytes": plan.bytes}


def build_plan(net, case):
    """The plan of PLAN_CASES entry `case` on `net` (a deterministic case switches the process-wide mode for the build only)."""
    import awr_amd
    _, _, training, n_buckets, wino, split_k, det = case
    net.train(training)
    was = awr_amd.get_deterministic()
    try:
        awr_amd.set_deterministic(det)
        return net.get_plan(B, H, training, supervised=(net.nstage - 1,), bn_repeat=net.nstage, n_buckets=n_buckets, winograd=wino, split_k=split_k)
    finally:
        awr_amd.set_deterministic(was)


def plan_records():
    out = {}
    nets = {}
    for case in PLAN_CASES:
        net = nets.get(case[1])
        if net is None:
            net = nets[case[1]] = make_net(case[1])
        plan = build_plan(net, case)
        out[case[0]] = plan_record(plan)
        net.release_plan(plan)
    return out


def step_record(name, dp_group):
    """Three deterministic TrainEngine steps from a procedural start: loss bit patterns and the SHA-256 of the parameters.  The caller has
    the deterministic mode on; dp_group: a one-rank process group (with AWR_FORCE_DP=1 in the environment) or None."""
    import awr_oracle as O
    import numpy as np
    import torch
    from awr_amd.trainer import TrainEngine
    img, jt = O.synth_batch(B, H, J, seed=71)
    net = make_net(name, O.procedural_state(O.manifest_for(name, J), seed=7))
    eng = TrainEngine(net, B, H, 1.0, coord_weight=1.0, dense_weight=1.0, use_graph=False, autotune=False, wgrad_streams=2, process_group=dp_group,
                      n_buckets=4, native_rccl=True if dp_group is not None else None)
    assert len(eng.plan.buckets) == (4 if dp_group is not None else 1) and eng.plan.det
    dev = net.device
    bits = []
    for _ in range(3):
        losses = eng.step(img.to(dev), jt.to(dev))[0]
        bits += [int(v) for v in losses.detach().cpu().numpy().astype(np.float32).view(np.uint32)]
    torch.cuda.synchronize()
    sha = hashlib.sha256(net.flat_params().detach().cpu().numpy().tobytes()).hexdigest()
    return {"loss_bits": bits, "params_sha256": sha}


def step_records(cases=None):
    import awr_amd
    import torch
    import torch.distributed as dist
    out = {}
    was = awr_amd.get_deterministic()
    saved = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT", "AWR_FORCE_DP")}
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", AWR_FORCE_DP="1")
    try:
        awr_amd.set_deterministic(True)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
        try:
            for rec, name, dp in (STEP_CASES if cases is None else cases):
                out[rec] = step_record(name, dist.group.WORLD if dp else None)
        finally:
            dist.destroy_process_group()
    finally:
        awr_amd.set_deterministic(was)
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


# ---- the wide record ------------------------------------------------------------------------------------------------------------------------
def wide_case(name, net, training, n_buckets=1, winograd="direct", split_k=None, det=False, accum=None, downsample=2, env=None):
    return {"name": name, "net": net, "training": training, "n_buckets": n_buckets, "winograd": winograd, "split_k": split_k, "det": det,
            "accum": accum, "downsample": downsample, "env": env or {}}


def _wide_plan_cases():
    c = []
    for net in ("resnet_50", "hourglass_2"):                   # the bottleneck blocks; the second stack (a head gradient with a second producer)
        c += [wide_case("%s/train/b%d" % (net, nb), net, True, nb) for nb in (1, 4)] + [wide_case("%s/eval" % net, net, False)]
    for ds in (1, 4):                                          # the other downsample rates
        c += [wide_case("resnet_18/ds%d/%s" % (ds, "train" if t else "eval"), "resnet_18", t, downsample=ds) for t in (True, False)]
    for net in ("resnet_18", "hourglass_1"):                   # Winograd gradients
        c += [wide_case("%s/train/%s" % (net, w), net, True, winograd=w) for w in ("full", "forward+wgrad")]
    c.append(wide_case("resnet_18/eval/forward", "resnet_18", False, winograd="forward"))
    for net in ("hourglass_1", "hourglass_2"):                 # pairs and duals; pairs without duals; no pooling inside the GEMM launch
        c.append(wide_case("%s/eval/fuse2" % net, net, False, env={"AWR_FUSE2_MIN_WGS": "1"}))
        c.append(wide_case("%s/eval/fuse2/no_dual" % net, net, False, env={"AWR_FUSE2_MIN_WGS": "1", "AWR_NO_FUSE2_DUAL": "1"}))
        c.append(wide_case("%s/eval/no_gemm_pool" % net, net, False, env={"AWR_GEMM_POOL": "0"}))
    c += [wide_case("%s/train/det" % net, net, True, det=True) for net in ("hourglass_1", "resnet_50")]      # per-split copies of conv_bwd
    for t in (True, False):
        c.append(wide_case("resnet_18/%s/split_k" % ("train" if t else "eval"), "resnet_18", t, split_k=True))
        c.append(wide_case("resnet_18/%s/blocked" % ("train" if t else "eval"), "resnet_18", t, accum="blocked"))
    return c


WIDE_PLAN_CASES = _wide_plan_cases()
WIDE_STEP_CASES = [("%s/%s" % (n, m), n, m == "dp") for n in ("resnet_50", "hourglass_2") for m in ("single", "dp")]
WIDE_LISTS = ("fwd", "bwd", "gemms", "tensors")


def wide_record(plan):
    """Everything awr_plan_op / _gemm / _gemm_algo / _bucket / _tensor / _info / _winograd list of one plan, as JSON values."""
    from awr_amd import _lib as L
    rec = {"buckets": [list(b) for b in plan.buckets], "n_gemm": plan.n_gemm, "n_bn": plan.n_bn, "n_winograd": plan.n_winograd,
           "winograd_macs": float(plan.winograd_macs).hex(), "bytes": plan.bytes}
    name, macs, flags = C.c_char_p(), C.c_double(), C.c_int()
    for which, key in ((0, "fwd"), (1, "bwd")):
        rec[key] = []
        for i in range(plan.n_ops[which]):
            L.call("awr_plan_op", plan.h, which, i, C.byref(name), C.byref(macs), C.byref(flags))
            rec[key].append([name.value.decode(), flags.value, float(macs.value).hex()])
    tm, tn, tb, us, tuned, algo = C.c_int(), C.c_int(), C.c_int(), C.c_float(), C.c_int(), C.c_int()
    rec["gemms"] = []
    for i in range(plan.n_gemm):
        L.call("awr_plan_gemm", plan.h, i, C.byref(name), C.byref(tm), C.byref(tn), C.byref(tb), C.byref(us), C.byref(tuned))
        L.call("awr_plan_gemm_algo", plan.h, i, C.byref(algo))
        rec["gemms"].append([name.value.decode(), tm.value, tn.value, tb.value, tuned.value, algo.value])
    dims, lz = (C.c_int * 4)(), C.c_int()
    buf, grad, sc, sh = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    rec["tensors"], i = [], 0
    while L.lib.awr_plan_tensor(plan.h, i, C.byref(name), dims, C.byref(buf), C.byref(grad), C.byref(lz), C.byref(sc), C.byref(sh)) == 0:
        rec["tensors"].append([name.value.decode(), list(dims), lz.value, 1 if grad.value else 0])
        i += 1
    return rec


def wide_net(case):
    import awr_amd
    if case["net"].startswith("resnet"):
        return awr_amd.get_deconv_net(int(case["net"].split("_")[1]), J, case["downsample"]).cuda()
    return make_net(case["net"])


def wide_plan_records():
    """{record name: wide_record, or {"refused": text} where the library refuses the case}; one network per (name, downsample), one plan alive
    at a time; a case's environment (read by the builder per plan) and the deterministic mode hold for its build only."""
    import awr_amd
    from awr_amd import _lib as L
    out, nets = {}, {}
    for case in WIDE_PLAN_CASES:
        key = (case["net"], case["downsample"])
        if key not in nets:
            nets[key] = wide_net(case)
        net = nets[key]
        net.train(case["training"])
        was = awr_amd.get_deterministic()
        saved = {k: os.environ.get(k) for k in case["env"]}
        os.environ.update(case["env"])
        try:
            awr_amd.set_deterministic(case["det"])
            plan = net.get_plan(B, H, case["training"], supervised=(net.nstage - 1,), bn_repeat=net.nstage, n_buckets=case["n_buckets"],
                                accum=case["accum"], winograd=case["winograd"], split_k=case["split_k"])
            out[case["name"]] = wide_record(plan)
            net.release_plan(plan)
        except L.AwrError as e:
            out[case["name"]] = {"refused": str(e)}
        finally:
            awr_amd.set_deterministic(was)
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return out


def list_digest(items):
    """What stands for a list of the wide record in the file: its length and the SHA-256 of its compact JSON text."""
    return {"n": len(items), "sha256": hashlib.sha256(json.dumps(items, separators=(",", ":")).encode()).hexdigest()}


MAX_FILE_BYTES = 1 << 20      # committed files stay below 1 MiB


def ops_digest(ops):
    """What stands for an op list where the lists themselves would make the file too large."""
    return {"n": len(ops), "sha256": hashlib.sha256(json.dumps([[n, int(f)] for n, f in ops], separators=(",", ":")).encode()).hexdigest()}


def same_ops(recorded, ops):
    """Does the op list `ops` equal its record (a list, or an ops_digest)?"""
    if isinstance(recorded, dict):
        return recorded == ops_digest(ops)
    return recorded == [[n, int(f)] for n, f in ops]


def main():
    args = [a for a in sys.argv[1:] if a != "--wide"]
    wide = len(args) != len(sys.argv) - 1
    out = args[0] if args else os.path.join(REPO, "tests", "golden", "plan_snapshot_wide.json" if wide else "plan_snapshot.json")
    if wide:
        rec = {"shape": {"B": B, "H": H, "J": J}, "plans": wide_plan_records(), "steps": step_records(WIDE_STEP_CASES)}
    else:
        rec = {"shape": {"B": B, "H": H, "J": J}, "plans": plan_records(), "steps": step_records()}

    def text():
        return json.dumps(rec, separators=(",", ":"), sort_keys=True) + "\n"
    if wide:
        for r in rec["plans"].values():
            for k in WIDE_LISTS:
                if k in r:      # (a refused case has no lists)
                    r[k] = list_digest(r[k])
    elif len(text()) > MAX_FILE_BYTES:
        for r in rec["plans"].values():
            r["fwd"], r["bwd"] = ops_digest(r["fwd"]), ops_digest(r["bwd"])
    with open(out, "w") as f:
        f.write(text())
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
