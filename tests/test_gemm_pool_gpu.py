"""The 2x2 / stride-2 max-pool of a plain or two-tensor 1x1 launch's output, written by that launch (awr_conv_args.pool_out without w2; DESIGN.md
4.14): operator level bit for bit against the same launch without pool_out and against awr_maxpool_fwd, the refusals, and the inference plans
that carry their pools in the producing launch (Winograd plans, plans whose conv pairs do not form) against the plans with the separate passes
and the golden bars of tests/test_nets_gpu.py (imported, not copied)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import awr_oracle as O
from test_nets_gpu import amd, assert_joints, make_net, oracle_fp64_joint_gap, report  # noqa: F401  (fixture + helpers of the golden tests)
from test_ops_gpu import L, dev, ops, rnd  # noqa: F401

pytestmark = pytest.mark.gpu


def launch(ops, L, dev, x, w, N, tm, tn, res=None, bias=None, x2=None, pool=True, **kw):
    """one 1x1 launch over x (B, H, W, C1) [| x2 (B, H, W, C2)] with the packed weights w -> (out, pooled or None); NaN-filled outputs"""
    B, H, W, c1 = x.shape
    cin = c1 + (x2.shape[3] if x2 is not None else 0)
    spec = ops.ConvSpec("conv", cin, N, 1, 1, 0)
    out = torch.full((B, H, W, N), float("nan"), device=dev)
    a = ops.make_conv_args(spec.fwd_problem(H, W), B, x, w, out, bias=bias, res=res, T=spec.T, **kw)
    a.tile_m, a.tile_n = tm, tn
    if x2 is not None:
        a.in2, a.Cin1 = L.ptr(x2), c1
    pooled = None
    if pool:
        pooled = torch.full((B, H // 2, W // 2, N), float("nan"), device=dev)
        a.pool_out = L.ptr(pooled)
    L.call("awr_conv_gemm", C.byref(a), L.stream())
    torch.cuda.synchronize()
    return out, pooled


def maxpool(L, dev, t):
    B, H, W, N = t.shape
    p = torch.full((B, H // 2, W // 2, N), float("nan"), device=dev)
    L.call("awr_maxpool_fwd", L.ptr(t), None, None, 0, B, H, W, N, 2, 2, 0, L.ptr(p), None, L.stream())
    torch.cuda.synchronize()
    return p


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(32, 32), (64, 64), (128, 64)])
def test_pooled_launch_is_bit_identical_to_launch_plus_maxpool(ops, L, dev, H, W, B):
    """Every tile x {no residual, residual} x {one tensor, two tensors (Cin1 < Cin)} x N in {56 (ragged N tile), 128, 256}: `out` equals the launch
    without pool_out and the pooled tensor equals awr_maxpool_fwd(out), bit for bit.  A 32-wide map admits tile_m = 1 only (the 2D patch of
    tile_m = 2 is 64 columns wide): that combination must be refused, not run."""
    cin, cin1 = 128, 32
    x = rnd(B, H, W, cin, seed=1).to(dev)
    xa, xb = x[..., :cin1].contiguous(), x[..., cin1:].contiguous()
    ran = 0
    for N in (56, 128, 256):
        w = ops.pack_weight(rnd(N, cin, 1, 1, seed=2 + N, scale=0.1).to(dev), ops.ConvSpec("conv", cin, N, 1, 1, 0).fwd_pack())
        bias = rnd(N, seed=3).to(dev)
        res = rnd(B, H, W, N, seed=4).to(dev)
        for tm in (1, 2):
            for tn in (1, 2):
                for r in (None, res):
                    for two in (False, True):
                        xs = dict(x=xa, x2=xb) if two else dict(x=x)
                        if W % (32 * tm) != 0:
                            with pytest.raises(L.AwrError, match="multiple of 64"):
                                launch(ops, L, dev, w=w, N=N, tm=tm, tn=tn, res=r, bias=bias, **xs)
                            continue
                        out0, _ = launch(ops, L, dev, w=w, N=N, tm=tm, tn=tn, res=r, bias=bias, pool=False, **xs)
                        out1, p1 = launch(ops, L, dev, w=w, N=N, tm=tm, tn=tn, res=r, bias=bias, **xs)
                        case = (B, H, W, N, tm, tn, r is not None, two)
                        assert not torch.isnan(out0).any() and not torch.isnan(p1).any(), case
                        assert torch.equal(out0, out1), case
                        assert torch.equal(maxpool(L, dev, out0), p1), case
                        ran += 1
    assert ran == (24 if W == 32 else 48)


@pytest.mark.parametrize("tm,tn", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_ties_and_signed_zeros_take_the_first_maximum(ops, L, dev, tm, tn):
    """The producer's weights are a 0/1 selection matrix and the inputs come from a handful of values (-0.0 and +0.0 among them), so the outputs are
    the chosen inputs exactly and most windows hold ties: the pooled tensor must equal awr_maxpool_fwd's bit for bit -- sign bits included (compared
    as integers) -- which pins the comparison order (0,0) (0,1) (1,0) (1,1) with `>`.  (The accumulators start at +0.0, so a -0.0 input leaves the GEMM
    as +0.0; the residual operand brings signed zeros and ties to the epilogue's own arithmetic.)"""
    B, H, W, cin, N = 2, 64, 64, 64, 128
    vals = torch.tensor([-1.0, -0.0, 0.0, 0.5, 2.0])
    g = torch.Generator().manual_seed(11)
    x = vals[torch.randint(0, 5, (B, H, W, cin), generator=g)].to(dev)
    sel = torch.randint(0, cin, (N,), generator=g)
    wsel = torch.zeros(N, cin, 1, 1)
    wsel[torch.arange(N), sel] = 1.0
    w = ops.pack_weight(wsel.to(dev), ops.ConvSpec("conv", cin, N, 1, 1, 0).fwd_pack())
    res = vals[torch.randint(0, 5, (B, H, W, N), generator=g)].to(dev)
    for r in (None, res):
        out0, _ = launch(ops, L, dev, x, w, N, tm, tn, res=r, pool=False)
        out1, p1 = launch(ops, L, dev, x, w, N, tm, tn, res=r)
        assert torch.equal(out0, x[..., sel.to(dev)] + (r if r is not None else 0.0))          # the chosen inputs, exactly
        assert torch.equal(out0.view(torch.int32), out1.view(torch.int32))
        p0 = maxpool(L, dev, out0)
        assert torch.equal(p0.view(torch.int32), p1.view(torch.int32))
        win = out0.view(B, H // 2, 2, W // 2, 2, N)
        ties = (win == p0.view(B, H // 2, 1, W // 2, 1, N)).sum(dim=(2, 4)) > 1
        # the fixture does what it is for: four draws from {-1: .2, 0: .4, .5: .2, 2: .2} tie at their maximum with probability 0.405 (with the
        # residual the values are sums of two draws: fewer ties, still thousands of windows)
        assert float(ties.float().mean()) > (0.3 if r is None else 0.0)


def test_refusals_leave_the_pooled_buffer_untouched(ops, L, dev):
    """pool_out on a launch that has no pooled form is an error that names the condition, and nothing is launched."""
    cin, N = 128, 128

    def attempt(match, H=32, W=32, k=1, tm=1, **kw):
        spec = ops.ConvSpec("conv", cin, N, k, 1, k // 2)
        B = 2
        x = torch.zeros(B, H, W, cin, device=dev)
        w = ops.pack_weight(rnd(N, cin, k, k, seed=1, scale=0.1).to(dev), spec.fwd_pack())
        out = torch.full((B, H, W, N), float("nan"), device=dev)
        pooled = torch.full((B, H // 2, W // 2, N), 7.25, device=dev)
        a = ops.make_conv_args(spec.fwd_problem(H, W), B, x, w, out, T=spec.T, **kw)
        a.tile_m, a.tile_n, a.pool_out = tm, 1, L.ptr(pooled)
        with pytest.raises(L.AwrError, match=match):
            L.call("awr_conv_gemm", C.byref(a), L.stream())
        torch.cuda.synchronize()
        assert bool((pooled == 7.25).all()) and bool(torch.isnan(out).all()), match

    attempt("even map height", H=33)
    attempt("multiple of 64", W=48, tm=2)
    attempt("plain epilogue", stats=torch.zeros(64, 2, N, device=dev, dtype=torch.float64))
    attempt("1x1 convolution", k=3)
    attempt("split-K", partial=torch.full((2, 2, 32, 32, N), float("nan"), device=dev), split_k=2)


def build_infer(amd, net, img, ks, monkeypatch, env, autotune=False):
    from awr_amd.trainer import InferEngine
    for k in ("AWR_GEMM_POOL", "AWR_PAIR_POOL", "AWR_NO_FUSE2", "AWR_FUSE2_MIN_WGS", "AWR_TUNE_CACHE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    J = 14
    m = make_net(amd, net, J, O.procedural_state(O.manifest_for(net, J), seed=0))
    m.eval()
    inf = InferEngine(m, img.shape[0], 128, ks, autotune=autotune)
    return m, inf


def pool_counts(names):
    return sum(1 for n in names if n == "awr_maxpool_fwd"), sum(1 for n in names if n.endswith("+pool"))


def run_pair_of_plans(amd, dev, net, img, ks, monkeypatch, env):
    """plan A as built under `env`, plan B under env + AWR_GEMM_POOL=0 -> (names A, names B, outputs A, outputs B)"""
    res = []
    for extra in ({}, {"AWR_GEMM_POOL": "0"}):
        m, inf = build_infer(amd, net, img, ks, monkeypatch, dict(env, **extra))
        jt = inf(img.to(dev)).cpu()
        res.append((inf.plan.op_names("fwd"), jt, inf.plan.dense_map(m.nstage - 1).cpu()))
    return res


def test_winograd_inference_plan_carries_its_pools(amd, dev, golden_dir, monkeypatch):
    """Hourglass-1 inference in the Winograd mode (conv2 is a Winograd launch, conv3 (+ skip) a plain 1x1 GEMM): the pools of the 128-, 64- and
    32-wide maps ride in the launch that produces their input; same bits as the plan with the separate passes, same golden bar."""
    g = np.load(os.path.join(golden_dir, "hourglass_1_fwd.npz"))
    img, ks = torch.from_numpy(g["img"]), float(g["ks"])
    amd.set_conv_winograd("force")
    try:
        (na, ja, da), (nb, jb, db) = run_pair_of_plans(amd, dev, "hourglass_1", img, ks, monkeypatch, {})
    finally:
        amd.set_conv_winograd(False)
    (pass_a, pool_a), (pass_b, pool_b) = pool_counts(na), pool_counts(nb)
    assert pool_b == 0 and pass_a < pass_b and pool_a == pass_b - pass_a, (na, nb)
    assert [n.replace("+pool", "") for n in na if n != "awr_maxpool_fwd"] == [n for n in nb if n != "awr_maxpool_fwd"]
    assert torch.equal(ja, jb) and torch.equal(da, db)
    sd = O.procedural_state(O.manifest_for("hourglass_1", 14), seed=0)
    gaps = oracle_fp64_joint_gap("hourglass_1", sd, img, ks, False)
    assert_joints("hourglass_1/eval@pool/stage0", ja.numpy(), g["eval_s0_jt"], gaps[0])


@pytest.mark.parametrize("net", ["hourglass_1", "hourglass_2"])
def test_direct_plans_without_pairs_carry_their_pools(amd, dev, golden_dir, net, monkeypatch):
    """Direct mode, batch 2, AWR_NO_FUSE2=1 (no pair forms): default against AWR_GEMM_POOL=0 -- fewer passes, the same bits; and under
    AWR_PAIR_POOL=0 no pool rides in any GEMM launch."""
    g = np.load(os.path.join(golden_dir, "%s_fwd.npz" % net))
    img, ks = torch.from_numpy(g["img"]), float(g["ks"])
    if img.shape[0] != 2:      # (the Hourglass-2 fixture holds one image)
        img = O.synth_batch(2, 128, 14, seed=3)[0]
    (na, ja, da), (nb, jb, db) = run_pair_of_plans(amd, dev, net, img, ks, monkeypatch, {"AWR_NO_FUSE2": "1"})
    (pass_a, pool_a), (pass_b, pool_b) = pool_counts(na), pool_counts(nb)
    assert pool_b == 0 and pass_a < pass_b and pool_a == pass_b - pass_a, (na, nb)
    assert torch.equal(ja, jb) and torch.equal(da, db)
    _, inf = build_infer(amd, net, img, ks, monkeypatch, {"AWR_NO_FUSE2": "1", "AWR_PAIR_POOL": "0"})
    assert pool_counts(inf.plan.op_names("fwd")) == (pass_b, 0)


# width of the map a residual of Hourglass-1 at 128x128 writes, by the layer prefix in its launch name: the three maps wide enough for the 2D tiles
POOLED_MAP_WIDTH = {"pre.1.": 128, "pre.4.": 64, "hgs.0.0.low1.": 32}


def test_tuned_plan_keeps_the_width_rule(amd, dev, monkeypatch):
    """autotune=True at batch 8: every +pool launch runs a tile whose 2D patch (32 tile_m columns) divides its map's width.  Outputs equal the
    AWR_GEMM_POOL=0 engine's bit for bit when both tuners chose the same tiles; otherwise within the 2e-5 relative bound
    test_inference_fused_conv_pairs uses between plan forms (a different tile or split-K depth changes a launch's summation order)."""
    img, _ = O.synth_batch(8, 128, 14, seed=5)
    ks = 0.4
    outs, tiles = [], []
    for env in ({}, {"AWR_GEMM_POOL": "0"}):
        m, inf = build_infer(amd, "hourglass_1", img, ks, monkeypatch, env, autotune=True)
        jt = inf(img.to(dev)).cpu()
        outs.append((jt, inf.plan.dense_map(0).cpu()))
        tiles.append({n.replace("+pool", ""): tuple(t[0][:3]) for n, t in inf.plan.tuned.items()})
        if not env:
            names = inf.plan.op_names("fwd")
            pooled = {n: t[0] for n, t in inf.plan.tuned.items() if n.endswith("+pool") and "conv2+" not in n}
            assert len(pooled) >= 1 and set(pooled) <= set(names), (pooled, names)
            for n, (tm, tn, *_) in pooled.items():
                wmap = [w for k, w in POOLED_MAP_WIDTH.items() if (":" + k) in n]
                assert len(wmap) == 1, n
                assert tm in (1, 2) and tn in (1, 2) and wmap[0] % (32 * tm) == 0, (n, tm, tn, wmap)
    scale = max(1.0, float(outs[1][1].abs().max()))
    report("hourglass_1/tuned@pool/same_tiles", float(tiles[0] == tiles[1]))
    report("hourglass_1/tuned@pool/dense_map_rel_diff", float((outs[0][1] - outs[1][1]).abs().max()) / scale)
    if tiles[0] == tiles[1]:
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    else:
        assert float((outs[0][1] - outs[1][1]).abs().max()) / scale <= 2e-5


def test_training_and_resnet_plans_are_unchanged(amd, dev, monkeypatch):
    """A ResNet18 inference plan (its pool is the stem's 3x3 / 2) and a Hourglass-1 TRAINING plan (a training pool also writes the argmax and the
    pooled tensor's statistics) are op for op the same with and without AWR_GEMM_POOL=0, and carry no +pool launch."""
    names = {}
    for env in ("1", "0"):
        monkeypatch.setenv("AWR_GEMM_POOL", env)
        m = make_net(amd, "resnet_18", 14, O.procedural_state(O.manifest_for("resnet_18", 14), seed=0))
        m.eval()
        pr = m.get_plan(2, 128, False)
        h = make_net(amd, "hourglass_1", 14, O.procedural_state(O.manifest_for("hourglass_1", 14), seed=0))
        ph = h.get_plan(2, 128, True)
        names[env] = (pr.op_names("fwd"), ph.op_names("fwd"), ph.op_names("bwd"))
    assert names["1"] == names["0"]
    assert not any("+pool" in n for part in names["1"] for n in part)
