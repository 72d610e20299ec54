"""Training split-K (awr_set_train_split_k): awr_conv_gemm splits launches that carry a BatchNorm statistics epilogue or the
fused BatchNorm-backward reductions, and the reduce kernel produces everything the unsplit epilogue would have -- operator level against
float64 and the single-pass launch, plan level against the golden bars of tests/test_nets_gpu.py (imported, not copied)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import awr_oracle as O
import test_nets_gpu as TN
from test_nets_gpu import amd, make_net  # noqa: F401  (fixture + helper of the golden tests)
from test_ops_gpu import L, _torch_fwd, dev, ops, rel_err, rnd  # noqa: F401

pytestmark = pytest.mark.gpu

SPLIT_CASES = [("conv", 512, 512, 3, 1, 2, 8), ("conv", 256, 512, 3, 2, 1, 16), ("deconv", 512, 256, 4, 2, 1, 8), ("conv", 96, 160, 1, 1, 3, 8),
               ("conv", 128, 128, 3, 1, 64, 4), ("conv", 512, 512, 3, 1, 16, 8)]


def reduce_grid(t):
    """workgroups of the reduce kernel for an NHWC output: one per 64 pixels x 64 channels (include/awr_hip.h: awr_conv_args.partial)"""
    npix = t.numel() // t.shape[-1]
    return ((npix + 63) // 64) * ((t.shape[-1] + 63) // 64)


def split_depth(ops, spec, x, wp, out, part, sk, st):
    """the depth awr_conv_gemm runs this forward launch with (awr_conv_split_depth)"""
    from awr_amd import _lib
    a = ops.make_conv_args(spec.fwd_problem(x.shape[1], x.shape[2]), x.shape[0], x, wp, out, stats=st, T=spec.T, partial=part, split_k=sk)
    d = C.c_int(0)
    _lib.call("awr_conv_split_depth", C.byref(a), C.byref(d))
    return d.value


def stat_err(got, ref):
    """largest per-channel error of a statistic relative to the largest channel's magnitude"""
    return float((got - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("kind,cin,cout,k,stride,B,H", SPLIT_CASES)
def test_forward_with_statistics_from_the_reduce_kernel(ops, dev, kind, cin, cout, k, stride, B, H):
    """Fused input affine + ReLU, bias, residual, ReLU and `stats` on a split launch (NaN-filled scratch): output within 5e-6 of float64 and
    2e-5 * max|y| of the single-pass launch (the bars of test_conv_split_k); the statistics, summed over the slots, equal the float64 sum and
    sum of squares of the value the launch returns before its ReLU to 1e-9 (fp64 accumulation of < 1e6 fp32 terms: a dropped row shows) --
    wherever the reduce kernel produced them: every explicit depth, and split_k=0 where the heuristic splits.  split_k=0 on the 1x1 case (three
    K slices) runs unsplit; its statistics are the unsplit epilogue's, compared with that launch's own."""
    pad = 1 if k > 1 else 0
    spec = ops.ConvSpec(kind, cin, cout, k, stride, pad)
    wshape = (cout, cin, k, k) if kind == "conv" else (cin, cout, k, k)
    w = rnd(*wshape, seed=1, scale=(cin * k * k) ** -0.5)
    x = rnd(B, cin, H, H, seed=2)
    bias = rnd(cout, seed=3)
    isc, ish = rnd(cin, seed=6) + 0.5, rnd(cin, seed=7) * 0.3
    a_in = TF.relu(x.double() * isc.double().view(1, -1, 1, 1) + ish.double().view(1, -1, 1, 1))
    y0 = _torch_fwd(kind, a_in, w.double(), bias.double(), stride, pad)
    res = rnd(*y0.shape, seed=8)
    y_ref = TF.relu(y0 + res.double())
    wp = ops.pack_weight(w.to(dev), spec.fwd_pack())
    kw = dict(bias=bias.to(dev), res=ops.nhwc(res).to(dev), in_scale=isc.to(dev), in_shift=ish.to(dev), relu_in=True)
    xg = ops.nhwc(x).to(dev)
    y1 = ops.conv_forward(spec, xg, wp, relu_out=True, **kw)
    assert rel_err(ops.nchw(y1).cpu(), y_ref) < 5e-6
    slots = reduce_grid(y1)
    for sk in (0, 2, 4, 8):
        part = torch.full((8,) + tuple(y1.shape), float("nan"), device=dev)      # every copy the launch reads must have been written
        st = torch.zeros(slots, 2, y1.shape[-1], device=dev, dtype=torch.float64)
        y2 = ops.conv_forward(spec, xg, wp, partial=part, split_k=sk, stats=st, relu_out=True, **kw)
        depth = split_depth(ops, spec, xg, wp, y2, part, sk, st)
        e64, e1 = rel_err(ops.nchw(y2).cpu(), y_ref), float((y2 - y1).abs().max()) / float(y1.abs().max())
        print("split_k=%d: rel. error vs float64 %.2e, vs single pass %.2e of max|y|" % (sk, e64, e1))
        assert e64 < 5e-6, sk
        assert e1 <= 2e-5, sk
        # the statistics describe the value BEFORE the ReLU: the same launch without it returns that value
        st0 = torch.zeros_like(st)
        v = ops.conv_forward(spec, xg, wp, partial=part, split_k=sk, stats=st0, relu_out=False, **kw)
        assert torch.equal(torch.relu(v), y2) and torch.equal(st0, st), sk
        vd = v.double().reshape(-1, v.shape[-1])
        got = st.sum(0).cpu()
        es, eq = stat_err(got[0], vd.sum(0).cpu()), stat_err(got[1], (vd * vd).sum(0).cpu())
        print("split_k=%d (runs at depth %d): statistics vs float64 sums of the stored value: sum %.2e, sum of squares %.2e" % (sk, depth, es, eq))
        if depth > 1:
            assert es < 1e-9 and eq < 1e-9, (sk, es, eq)
        else:
            # split_k=0 on a launch the heuristic leaves unsplit (the 1x1 case: three K slices): no reduce kernel runs, the statistics are the
            # unsplit epilogue's own (shifted fp32 sums per tile, measured 2.6e-8 / 5.6e-8 here) -- they must be exactly that launch's
            st1 = torch.zeros_like(st)
            ops.conv_forward(spec, xg, wp, stats=st1, relu_out=True, **kw)
            assert sk == 0 and stat_err(got, st1.sum(0).cpu()) < 1e-12, (sk, depth)


def _dgrad_case(ops, L, dev, form, split_k, part, tile=None):
    """One data-gradient launch of a 3x3 conv (256 -> 128 channels' gradient, 2 x 8 x 8) with the fused BatchNorm-backward reduction in `form`."""
    B, H, cin, cout = 2, 8, 128, 256
    spec = ops.ConvSpec("conv", cin, cout, 3, 1, 1)
    dp = spec.dgrad_problem(H, H)
    N = dp["N"]
    w = rnd(cout, cin, 3, 3, seed=43, scale=0.03)
    gy = ops.nhwc(rnd(B, cout, H, H, seed=41)).to(dev)
    y = ops.nhwc(rnd(B, N, H, H, seed=42) * 2.0 + 0.3).to(dev)
    coef4 = torch.stack([rnd(N, seed=44) + 1.2, rnd(N, seed=45) * 0.3, rnd(N, seed=46) * 0.2, rnd(N, seed=47) + 1.5]).to(dev).contiguous()
    wp = ops.pack_weight(w.to(dev), spec.dgrad_pack())
    g = torch.full((B, H, H, N), float("nan"), device=dev)
    slots = reduce_grid(g)
    sums = torch.zeros(slots, 2, N, device=dev, dtype=torch.float64)
    keep = [gy, y, coef4, wp, g, sums, part]
    d = ops.make_conv_args(dp, B, gy, wp, g, stats=sums, T=spec.T, partial=part, split_k=split_k)
    d.bnr_y, d.bnr_coef, d.stat_slots = L.ptr(y), L.ptr(coef4), slots
    act = y2 = coef2 = sums2 = None
    if form in ("act", "inplace", "bnr2"):
        act = ops.nhwc(rnd(B, N, H, H, seed=48)).to(dev)
        d.bnr_act = L.ptr(act)
    if form in ("inplace", "bnr2"):
        g.copy_(ops.nhwc(rnd(B, N, H, H, seed=49)).to(dev))
        d.res = L.ptr(g)
    if form == "bnr2":
        y2 = ops.nhwc(rnd(B, N, H, H, seed=50) * 1.5 - 0.2).to(dev)
        coef2 = torch.stack([rnd(N, seed=51) + 1.2, rnd(N, seed=52) * 0.3, rnd(N, seed=53) * 0.2, rnd(N, seed=54) + 1.5]).to(dev).contiguous()
        sums2 = torch.zeros(slots, 2, N, device=dev, dtype=torch.float64)
        d.bnr2_y, d.bnr2_coef, d.stats2 = L.ptr(y2), L.ptr(coef2), L.ptr(sums2)
    if tile:
        d.tile_m, d.tile_n = tile
    keep += [act, y2, coef2, sums2]
    L.call("awr_conv_gemm", C.byref(d), L.stream())
    torch.cuda.synchronize()
    return dict(g=g, sums=sums, sums2=sums2, y=y, coef4=coef4, y2=y2, coef2=coef2, act=act, keep=keep)


@pytest.mark.parametrize("form", ["plain", "act", "inplace", "bnr2"])
def test_data_gradient_reductions_from_the_reduce_kernel(ops, L, dev, form):
    """bnr_y in each of its forms -- plain, with bnr_act, in-place accumulating (res == out), with the second reduction bnr2_y: the stored masked
    gradient matches the unsplit launch within 2e-5 * max, both reduction sums match float64 sums formed from the stored gradient to 1e-9, and
    the ReLU mask is the unsplit launch's wherever |y * scale + shift| exceeds 1e-6."""
    ref = _dgrad_case(ops, L, dev, form, 0, None)
    g1 = ref["g"]
    assert torch.isfinite(g1).all()
    pre = ref["y"].double() * ref["coef4"][0].double() + ref["coef4"][1].double()
    guarded = pre.abs() <= 1e-6
    frac = float(guarded.double().mean())
    print("%s: the 1e-6 guard on |y * scale + shift| excludes %d of %d elements (%.4f %%)" % (form, int(guarded.sum()), guarded.numel(), 100 * frac))
    assert frac < 1e-3          # (a condition on the inputs, not on the code under test)
    for sk in (2, 4, 8):
        part = torch.full((8,) + tuple(g1.shape), float("nan"), device=dev)
        out = _dgrad_case(ops, L, dev, form, sk, part)
        g2 = out["g"]
        e = float((g2 - g1).abs().max()) / float(g1.abs().max())
        print("%s split_k=%d: masked gradient vs the unsplit launch %.2e of max" % (form, sk, e))
        assert e <= 2e-5, (form, sk, e)
        assert torch.equal((g2 != 0) | guarded, (g1 != 0) | guarded), (form, sk)
        gd, c = g2.double().reshape(-1, g2.shape[-1]), out["coef4"].double()
        yd = out["y"].double().reshape(-1, g2.shape[-1])
        got = out["sums"].sum(0)
        e1, e2 = stat_err(got[0], gd.sum(0)), stat_err(got[1], (gd * ((yd - c[2]) * c[3])).sum(0))
        print("%s split_k=%d: sum g %.2e, sum g * xhat %.2e vs float64 sums of the stored gradient" % (form, sk, e1, e2))
        assert e1 < 1e-9 and e2 < 1e-9, (form, sk, e1, e2)
        if form == "bnr2":
            c2, y2d = out["coef2"].double(), out["y2"].double().reshape(-1, g2.shape[-1])
            got2 = out["sums2"].sum(0)
            e3, e4 = stat_err(got2[0], gd.sum(0)), stat_err(got2[1], (gd * ((y2d - c2[2]) * c2[3])).sum(0))
            print("%s split_k=%d: second reduction %.2e, %.2e" % (form, sk, e3, e4))
            assert e3 < 1e-9 and e4 < 1e-9, (form, sk, e3, e4)


def test_same_depth_is_bitwise_reproducible(ops, L, dev):
    """Two launches with the same explicit depth agree bit for bit in outputs AND statistics when stat_slots >= the reduce grid (every address
    receives exactly one add onto zero) -- forward and data gradient."""
    spec = ops.ConvSpec("conv", 256, 512, 3, 2, 1)
    w, x = rnd(512, 256, 3, 3, seed=1, scale=0.02), rnd(2, 256, 16, 16, seed=2)
    wp, xg = ops.pack_weight(w.to(dev), spec.fwd_pack()), ops.nhwc(x).to(dev)
    runs = []
    for _ in range(2):
        part = torch.full((4, 2, 8, 8, 512), float("nan"), device=dev)
        st = torch.zeros(reduce_grid(part[0]), 2, 512, device=dev, dtype=torch.float64)
        a_out = torch.empty(2, 8, 8, 512, device=dev)
        a = ops.make_conv_args(spec.fwd_problem(16, 16), 2, xg, wp, a_out, stats=st, T=spec.T, partial=part, split_k=4)
        a.stat_slots = st.shape[0]
        L.call("awr_conv_gemm", C.byref(a), L.stream())
        torch.cuda.synchronize()
        runs.append((a_out, st))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][1].abs().sum()) > 0
    for form in ("plain", "bnr2"):
        outs = [_dgrad_case(ops, L, dev, form, 4, torch.full((4, 2, 8, 8, 128), float("nan"), device=dev)) for _ in range(2)]
        assert torch.equal(outs[0]["g"], outs[1]["g"]) and torch.equal(outs[0]["sums"], outs[1]["sums"])
        if form == "bnr2":
            assert torch.equal(outs[0]["sums2"], outs[1]["sums2"])


def test_blocked_split_launch_matches_the_blocked_launch(ops, L, dev):
    """accum = 1 on a split launch: every K range is accumulated blocked, the ordered sum over the copies is the outer fold -- the result stays
    within the split-K bar of the unsplit blocked launch and of float64, and awr_conv_split_depth reports the depth the launch runs with."""
    spec = ops.ConvSpec("conv", 512, 512, 3, 1, 1)
    w, x = rnd(512, 512, 3, 3, seed=1, scale=4608 ** -0.5), rnd(2, 512, 8, 8, seed=2)
    y_ref = TF.conv2d(x.double(), w.double(), None, 1, 1)
    wp, xg = ops.pack_weight(w.to(dev), spec.fwd_pack()), ops.nhwc(x).to(dev)
    prob = spec.fwd_problem(8, 8)
    outs = {}
    for sk in (1, 4):
        part = torch.full((8, 2, 8, 8, 512), float("nan"), device=dev)
        st = torch.zeros(16, 2, 512, device=dev, dtype=torch.float64)
        out = torch.full((2, 8, 8, 512), float("nan"), device=dev)
        a = ops.make_conv_args(prob, 2, xg, wp, out, stats=st, T=spec.T, partial=part, split_k=sk)
        a.accum = 1
        depth = C.c_int(0)
        L.call("awr_conv_split_depth", C.byref(a), C.byref(depth))
        assert depth.value == sk
        L.call("awr_conv_gemm", C.byref(a), L.stream())
        torch.cuda.synchronize()
        outs[sk] = out
        assert rel_err(ops.nchw(out).cpu(), y_ref) < 5e-6, sk
    assert float((outs[4] - outs[1]).abs().max()) <= 2e-5 * float(outs[1].abs().max())


def test_requests_the_rule_rejects_fail_by_name_and_launch_nothing(ops, L, dev):
    """in2, the fused pair, in_bnb_y, the split-operand product mode and a blocked launch whose K ranges would be shorter than one 128-k block:
    an error that names the reason, and the output buffer is untouched."""
    def attempt(spec, H, match, setup, cin_x=None, accum=0, split_k=2):
        B = 2
        prob = spec.fwd_problem(H, H)
        x = ops.nhwc(rnd(B, cin_x or prob["Cin"], H, H, seed=3)).to(dev)
        wshape = (spec.cout, spec.cin, spec.k, spec.k)
        wp = ops.pack_weight(rnd(*wshape, seed=4, scale=0.05).to(dev), spec.fwd_pack())
        out = torch.full((B, prob["Hout"], prob["Wout"], prob["N"]), float("nan"), device=dev)
        part = torch.full((8,) + tuple(out.shape), float("nan"), device=dev)
        st = torch.zeros(reduce_grid(out), 2, prob["N"], device=dev, dtype=torch.float64)
        a = ops.make_conv_args(prob, B, x, wp, out, stats=st, T=spec.T, partial=part, split_k=split_k)
        a.accum = accum
        keep = setup(a, prob, x, out)
        with pytest.raises(L.AwrError, match=match):
            L.call("awr_conv_gemm", C.byref(a), L.stream())
        torch.cuda.synchronize()
        assert torch.isnan(out).all() and torch.isnan(part).all() and float(st.abs().sum()) == 0.0, match
        return keep

    one = ops.ConvSpec("conv", 128, 128, 1, 1, 0)

    def with_in2(a, prob, x, out):
        x2 = torch.zeros(2, 8, 8, 64, device=dev)
        a.in2, a.Cin1 = L.ptr(x2), 64
        return x2
    attempt(one, 8, "second input tensor", with_in2, cin_x=64)

    def with_pair(a, prob, x, out):
        w2 = torch.zeros(256, 128, device=dev)
        a.w2, a.N1, a.N = L.ptr(w2), 128, 256
        return w2
    attempt(ops.ConvSpec("conv", 128, 128, 3, 1, 1), 8, "fused pair", with_pair)

    def with_bnb(a, prob, x, out):
        yb, c4 = torch.zeros_like(x), torch.zeros(4, 128, device=dev)
        a.in_bnb_y, a.in_bnb_coef, a.stats = L.ptr(yb), L.ptr(c4), None
        return yb, c4
    attempt(one, 8, "in_bnb_y", with_bnb)

    L.call("awr_set_gemm_products", 6)
    try:
        attempt(ops.ConvSpec("conv", 128, 128, 3, 1, 1), 8, "split-operand product mode", lambda a, prob, x, out: None)
    finally:
        L.call("awr_set_gemm_products", 1)
    # K = 576 = 18 slices: a nominal range of ceil(18 / 8) = 3 slices (96 k) is shorter than one 128-k block; split_k=4 (5 slices nominal) is admitted
    attempt(ops.ConvSpec("conv", 64, 64, 3, 1, 1), 8, "holds a whole 128-k block", lambda a, prob, x, out: None, accum=1, split_k=8)


# ---- plan level ---------------------------------------------------------------------------------------------------------------------------

def _depths(plan):
    """{launch name: split-K depth} of the plan's forward / data-gradient launches that have split-K scratch (awr_plan_gemm's target_blocks)"""
    out = {}
    for i in range(plan.n_gemm):
        name, (tm, tn, tb, algo), us, tuned = plan._gemm(i)
        if not name.startswith("awr_conv_wgrad") and tb:
            out[name] = tb
    return out


def _split_kinds(plan):
    """(forward launches, data-gradient launches) of `plan` that run at a depth > 1"""
    d = _depths(plan)
    return ({k: v for k, v in d.items() if k.startswith("awr_conv_gemm:") and v > 1},
            {k: v for k, v in d.items() if k.startswith("awr_conv_dgrad:") and v > 1})


@pytest.fixture
def split_mode(amd):
    assert not amd.get_train_split_k()
    amd.set_train_split_k(True)
    try:
        yield amd
    finally:
        amd.set_train_split_k(False)


@pytest.fixture
def engines(monkeypatch):
    """Every TrainEngine built while the fixture is active (the golden bodies build their own, and tune it: depth 1 is among the tuner's
    candidates) -- so that a test can assert that the plan whose bars were checked really ran split launches."""
    import awr_amd.trainer as T
    made = []

    class Recorded(T.TrainEngine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(T, "TrainEngine", Recorded)
    return made


def assert_ran_split(made):
    assert made
    for eng in made:
        fwd, dg = _split_kinds(eng.plan)
        print("checked engine (batch %d, tuned %s): %d forward and %d data-gradient launches at depth > 1" % (eng.B, bool(eng.plan.tuned), len(fwd), len(dg)))
        assert eng.plan.train_split_k == 1 and fwd and dg, (eng.B, _depths(eng.plan))


@pytest.mark.parametrize("mode", ["auto", "ordered"])
def test_resnet18_batch8_meets_the_golden_bars_split(split_mode, engines, dev, golden_dir, mode):
    """tests/golden/resnet_18_train_b8.npz with the process-wide mode on, through the golden test's own body: forward and data-gradient launches
    report a depth > 1 (under "auto" the blocked forward launches among them), and every bar of the default mode holds."""
    amd = split_mode
    m = make_net(amd, "resnet_18", 14, O.reference_init_state("resnet_18", 14, seed=3))
    plan = m.get_plan(8, 128, True, accum=mode)
    assert plan.train_split_k == 1
    d = _depths(plan)
    fwd = {k: v for k, v in d.items() if k.startswith("awr_conv_gemm:") and v > 1}
    dg = {k: v for k, v in d.items() if k.startswith("awr_conv_dgrad:") and v > 1}
    print("split forward launches %s\nsplit data-gradient launches %s" % (fwd, dg))
    assert fwd and dg
    m.release_plan(plan)
    TN.test_well_conditioned_training_fixture_meets_the_plain_bar_in_every_mode(amd, dev, golden_dir, mode)
    assert_ran_split(engines)          # the TUNED plans whose bars were just checked


@pytest.mark.parametrize("net", ["resnet_18", "hourglass_1"])
def test_training_fixtures_meet_the_golden_bars_split(split_mode, engines, dev, golden_dir, net):
    """The two-image training fixtures (ResNet18, Hourglass-1) under the mode, through test_fused_train_step_golden itself (accum = "auto", the
    engine's default): losses, joints, gradient norms, two Adam steps."""
    amd = split_mode
    m = make_net(amd, net, 14, O.procedural_state(O.manifest_for(net, 14), seed=1))
    plan = m.get_plan(2, 128, True)
    d = _depths(plan)
    assert any(k.startswith("awr_conv_gemm:") and v > 1 for k, v in d.items()) and any(k.startswith("awr_conv_dgrad:") and v > 1 for k, v in d.items()), d
    m.release_plan(plan)
    TN.test_fused_train_step_golden(amd, dev, golden_dir, net, "c1", 1.0)
    assert_ran_split(engines)


@pytest.mark.parametrize("autotune", [False, True])
def test_hourglass_fixture_meets_the_golden_bars_split_ordered(amd, dev, golden_dir, autotune):
    """tests/golden/hourglass_1_train.npz under accum="ordered" with split_k=True: the Hourglass launches (1x1 layers, in-place accumulating data
    gradients, the deep levels) then take the ordered split kernel, not the blocked one.  The bars and constants of test_fused_train_step_golden
    through its own helpers (loss 2e-4, joints within 2x the oracle's gap, gradient norms 5e-3, sampled parameters after one and two Adam steps);
    with the heuristic depths and with the tuned ones."""
    from awr_amd.trainer import TrainEngine
    net, tag, cw = "hourglass_1", "c1", 1.0
    g = np.load(os.path.join(golden_dir, "%s_train.npz" % net))
    img, jt_gt = torch.from_numpy(g["img"]), torch.from_numpy(g["jt_gt"])
    J, ks = int(g["J"]), float(g["ks"])
    man = O.manifest_for(net, J)
    pkeys = [str(k) for k in g["pkeys"]]
    m = make_net(amd, net, J, O.procedural_state(man, seed=1))
    eng = TrainEngine(m, img.shape[0], 128, ks, coord_weight=cw, dense_weight=1.0, lr=1e-3, use_graph=False, accum="ordered", split_k=True,
                      autotune=autotune)
    assert eng.plan.accum == 0 and eng.plan.train_split_k == 1
    losses, jt = eng.step(img.to(dev), jt_gt.to(dev))
    fwd, dg = _split_kinds(eng.plan)
    print("hourglass_1 ordered (autotune %s): %d forward, %d data-gradient launches at depth > 1" % (autotune, len(fwd), len(dg)))
    assert fwd and dg, _depths(eng.plan)
    l0, ref0 = float(losses[2]), float(g[tag + "_loss0"])
    assert abs(l0 - ref0) <= 2e-4 * abs(ref0), (l0, ref0)
    assert abs(float(losses[0]) - float(g[tag + "_lcoord0"])) <= 2e-4 * max(1e-6, abs(float(g[tag + "_lcoord0"]))) + 1e-9
    gap = TN.oracle_fp64_joint_gap(net, O.procedural_state(man, seed=1), img, ks, True)[-1]
    TN.assert_joints("%s/%s/train/split_k_ordered" % (net, tag), jt.cpu().numpy(), g[tag + "_jt0"], gap, factor=2.0, yardstick=None)
    TN.check_grad_norms(m, pkeys, g[tag + "_grad_l2"], g[tag + "_grad_smp"], tol=5e-3)
    assert all(int(v) == 1 for k, v in m.state_dict().items() if k.endswith("num_batches_tracked"))
    sd1 = m.state_dict()
    p1 = np.array([float(sd1[k].reshape(-1)[TN.smp_index(sd1[k].numel(), i)]) for i, k in enumerate(pkeys)], np.float32)
    d1 = np.abs(p1 - g[tag + "_param_smp1"])
    assert np.quantile(d1, 0.9) <= 1e-4 and d1.max() <= 2.1e-3, (np.quantile(d1, 0.9), d1.max())
    losses, _ = eng.step(img.to(dev), jt_gt.to(dev))
    ref1 = float(g[tag + "_loss1"])
    assert abs(float(losses[2]) - ref1) <= 2e-2 * abs(ref1)
    sd2 = m.state_dict()
    p2 = np.array([float(sd2[k].reshape(-1)[TN.smp_index(sd2[k].numel(), i)]) for i, k in enumerate(pkeys)], np.float32)
    d2 = np.abs(p2 - g[tag + "_param_smp2"])
    assert np.quantile(d2, 0.9) <= 3e-4 and d2.max() <= 2.1e-3, (np.quantile(d2, 0.9), d2.max())


def test_default_is_off_and_the_plan_is_what_it_was(amd, dev):
    """split_k=False is the default: no training launch has scratch, and the plan's bytes are those of a plan built while the mode is off.  (In a
    whole-suite run earlier tests of this file have switched the mode on and off again, so "before the mode was ever touched in the process" is
    approximated: the mode is asserted off at entry, and the bytes of plans built before and after an on-plan are equal.)"""
    from awr_amd.trainer import TrainEngine
    assert not amd.get_train_split_k()
    sd = O.reference_init_state("resnet_18", 14, seed=3)
    before = make_net(amd, "resnet_18", 14, sd).get_plan(8, 128, True)
    assert before.train_split_k == 0 and not _depths(before)
    on = make_net(amd, "resnet_18", 14, sd).get_plan(8, 128, True, split_k=True)
    assert on.train_split_k == 1 and _depths(on) and on.bytes > before.bytes
    print("plan bytes: %d without, %d with the mode (+%.1f MB of split-K scratch)" % (before.bytes, on.bytes, (on.bytes - before.bytes) / 2 ** 20))
    assert not amd.get_train_split_k()          # get_plan restored the process-wide mode
    m = make_net(amd, "resnet_18", 14, sd)
    eng = TrainEngine(m, 8, 128, 1.0, use_graph=False, autotune=False)
    assert eng.plan.train_split_k == 0 and not _depths(eng.plan)
    after = make_net(amd, "resnet_18", 14, sd).get_plan(8, 128, True)
    assert after.bytes == before.bytes and after.n_ops == before.n_ops and after.n_gemm == before.n_gemm
    eng2 = TrainEngine(make_net(amd, "resnet_18", 14, sd), 8, 128, 1.0, use_graph=False, autotune=False, split_k=True)
    assert eng2.plan.train_split_k == 1 and _depths(eng2.plan)
    # evaluation plans are not touched by the mode (they split on their own rule)
    ev0 = make_net(amd, "resnet_18", 14, sd).get_plan(8, 128, False)
    ev1 = make_net(amd, "resnet_18", 14, sd).get_plan(8, 128, False, split_k=True)
    assert ev0.bytes == ev1.bytes


@pytest.mark.parametrize("net", ["resnet_18", "hourglass_1"])
def test_deterministic_mode_with_split_k_is_bitwise_reproducible(amd, dev, net):
    """Deterministic plans take the heuristic depth (a pure function of the shapes) and size the statistics slots for the unsplit launch's
    workgroup count, which the reduce grid never exceeds: two engines from the same seed end three steps bit-equal in every parameter, the
    gradients, the BatchNorm buffers and the losses."""
    from awr_amd.trainer import TrainEngine
    J, B = 14, 4
    ks = 1.0 if net.startswith("resnet") else 0.4
    img, jt_gt = O.synth_batch(B, 128, J, seed=83)
    man = O.manifest_for(net, J)
    amd.set_deterministic(True)
    try:
        runs = []
        for streams in (0, 2):
            m = make_net(amd, net, J, O.procedural_state(man, seed=8))
            eng = TrainEngine(m, B, 128, ks, coord_weight=1.0, use_graph=False, wgrad_streams=streams, split_k=True)
            assert eng.plan.det and not eng.plan.tuned and any(v > 1 for v in _depths(eng.plan).values())
            ls = []
            for it in range(3):
                losses, jt = eng.step(img.to(dev), jt_gt.to(dev))
                ls.append(losses.clone())
            torch.cuda.synchronize()
            runs.append((torch.stack(ls), m.flat_grads()[:m.n_active].clone(), m.flat_params().clone(), m._barena.clone()))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        assert torch.isfinite(runs[0][0]).all()
    finally:
        amd.set_deterministic(False)


def test_split_k_composes_with_winograd_full(amd, engines, dev, golden_dir):
    """split_k=True with winograd="full": launches a Winograd form has taken keep it (same Winograd launch count), the rest may split, and the
    batch-8 fixture's bars hold."""
    sd = O.reference_init_state("resnet_18", 14, seed=3)
    n0 = make_net(amd, "resnet_18", 14, sd).get_plan(64, 128, True, winograd="full").n_winograd
    n1 = make_net(amd, "resnet_18", 14, sd).get_plan(64, 128, True, winograd="full", split_k=True).n_winograd
    assert n0 == n1 and n0 > 0, (n0, n1)
    amd.set_train_split_k(True)
    amd.set_conv_winograd("full")
    try:
        TN.test_well_conditioned_training_fixture_meets_the_plain_bar_in_every_mode(amd, dev, golden_dir, "auto")
    finally:
        amd.set_conv_winograd(False)
        amd.set_train_split_k(False)
    assert_ran_split(engines)


def test_gradients_against_the_fp64_yardstick_split_batch8(amd, dev):
    """The float64 gradient yardstick of tests/yardstick.py on ResNet18 at BATCH 8 with split_k=True (heuristic depths: autotune off): whole
    gradient tensors against float64 evaluated with the plan's own ReLU / max-pool decisions, within the ratio the default-mode test
    (test_nets_gpu.test_gradients_elementwise_against_the_fp64_yardstick) allows -- e_hip <= 3.0 * e_f32 + allow + 2e-5, decisions differing
    from float64's only within 1e-4 of a kink -- and the plan runs forward and data-gradient launches at depth > 1."""
    import yardstick as Y
    from awr_amd.trainer import TrainEngine
    net, cw, J, B, ks = "resnet_18", 1.0, 14, 8, 1.0
    img, jt_gt = O.synth_batch(B, 128, J, seed=23)
    sd = O.reference_init_state(net, J, seed=9)
    ref = Y.trace(net, sd, img, jt_gt, ks, cw, True)
    f32 = Y.trace(net, sd, img, jt_gt, ks, cw, False)
    fl32, pl32 = Y.decisions_from_trace(ref, f32)
    ref_f32 = Y.trace(net, sd, img, jt_gt, ks, cw, True, flips=fl32, pools=pl32)
    m = make_net(amd, net, J, sd)
    eng = TrainEngine(m, B, 128, ks, coord_weight=cw, dense_weight=1.0, lr=1e-3, autotune=False, split_k=True)
    fwd, dg = _split_kinds(eng.plan)
    print("batch-8 yardstick plan: forward depths %s, data-gradient depths %s" % (fwd, dg))
    assert fwd and dg
    eng.step(img.to(dev), jt_gt.to(dev))
    torch.cuda.synchronize()
    flips, pools, rep = Y.decisions_from_plan(ref, eng.plan.tensors(lazy=True))
    for tag, n, mx in rep:
        assert mx < 1e-4, ("ReLU / max-pool decision differs from float64 away from a kink", tag, n, mx)
    ref_hip = Y.trace(net, sd, img, jt_gt, ks, cw, True, flips=flips, pools=pools)
    stem_kink = Y.stem_allowance(ref)
    pkeys = O.params_of(sd, O.manifest_for(net, J))
    gmax = max(float(ref["grads"][k].norm()) for k in pkeys if ref["grads"][k] is not None)
    rows, bad = [], []
    for k in pkeys:
        if ref["grads"][k] is None:
            assert k in m._unused
            continue
        floor = 1e-3 * gmax
        e_hip = Y.rel_l2(m.grad_view(k).cpu(), ref_hip["grads"][k], floor)
        e_f32 = Y.rel_l2(f32["grads"][k], ref_f32["grads"][k], floor)
        rows.append((e_hip / max(e_f32, 1e-7), k, e_hip, e_f32))
        allow = 1.5 * stem_kink if k.startswith("pre.") else 0.0
        if not e_hip <= 3.0 * e_f32 + allow + 2e-5:
            bad.append((k, e_hip, e_f32, stem_kink))
    print("batch 8, split mode: median error ratio HIP / fp32 oracle %.2f, max rel. L2 error HIP %.2e / fp32 oracle %.2e; decisions flipped: %s" %
          (float(np.median([r[0] for r in rows])), max(r[2] for r in rows), max(r[3] for r in rows), rep))
    for r in sorted(rows, reverse=True)[:4]:
        print("  %6.2f  %-40s hip %.2e  fp32 oracle %.2e" % r)
    assert not bad, bad[:8]


def test_gradients_against_the_fp64_yardstick_split(split_mode, dev):
    """The same yardstick through the default-mode test itself under the process-wide mode: its own fixture (two images) and its own ratio."""
    TN.test_gradients_elementwise_against_the_fp64_yardstick(split_mode, dev, "resnet_18", 1.0)
