#!/usr/bin/env python3
"""Record what the plan engine builds and what a deterministic training step computes (GPU):

    tools/plan_snapshot.py OUT.json

One record per covered plan -- the forward and backward op names in order with `flags & 3` of awr_plan_op (bit 0 side_ok, bit 1 gemm),
the gradient buckets, n_gemm, n_bn, n_winograd and the plan's bytes -- and one per covered deterministic training run: the bit patterns
of the losses of three steps and the SHA-256 of the parameter arena after the third.  tests/test_plan_schedule_gpu.py compares the
plans and steps of the current build with tests/golden/plan_snapshot.json, which this tool wrote on the commit BEFORE the plan engine's
scheduling moved from op names to op flags; a change that is meant to alter a plan re-records the file and says so.
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


def step_records():
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
            for rec, name, dp in STEP_CASES:
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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "plan_snapshot.json")
    rec = {"shape": {"B": B, "H": H, "J": J}, "plans": plan_records(), "steps": step_records()}

    def text():
        return json.dumps(rec, separators=(",", ":"), sort_keys=True) + "\n"
    if len(text()) > MAX_FILE_BYTES:
        for r in rec["plans"].values():
            r["fwd"], r["bwd"] = ops_digest(r["fwd"]), ops_digest(r["bwd"])
    with open(out, "w") as f:
        f.write(text())
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
