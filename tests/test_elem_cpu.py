"""No GPU needed: what keeps tests/test_elem_gpu.py honest.  The reduction shapes reach every launch class of col_reduce_launch /
col_reduce_kernel (read from elem_cases.reduce_launch, not from the table's comments), the `exact` inputs really are exact in fp32 in any
order of summation, and every float64 reference of elem_cases agrees with torch's own operator -- ties of the max-pool included."""
import pytest
import torch
import torch.nn.functional as TF

import elem_cases as EC

ids = EC.case_id


def test_the_launch_values_of_the_table():
    """the figures the shapes were chosen by, recomputed"""
    expect = {  # (npix, C): rpp, idle, rows, grid, chunks, per-thread rows in a full slab, in the last slab
        (1, 4): (256, 0, 256, 1, 1, set(), {0, 1}), (63, 8): (128, 0, 128, 1, 1, set(), {0, 1}), (65, 96): (10, 16, 70, 1, 1, set(), {6, 7}),
        (257, 4): (256, 0, 256, 2, 1, {1}, {0, 1}), (4099, 64): (16, 0, 64, 65, 1, {4}, {0, 1}), (66001, 64): (16, 0, 80, 826, 1, {5}, {0, 1}),
        (70001, 256): (4, 0, 72, 973, 1, {18}, {4, 5}), (577, 1024): (1, 0, 64, 10, 1, {64}, {1}), (131, 2048): (1, 0, 64, 3, 2, {64}, {3}),
        (97, 3072): (1, 0, 64, 2, 3, {64}, {33}), (1030, 516): (1, 127, 64, 17, 1, {64}, {6}), (351, 128): (8, 0, 64, 6, 1, {8}, {3, 4}),
    }
    assert set(expect) == set(EC.REDUCE_SHAPES)
    for shape, (rpp, idle, rows, grid, chunks, full, last) in expect.items():
        la = EC.reduce_launch(*shape)
        assert (la["rpp"], la["idle"], la["rows"], la["grid"], la["chunks"], set(la["full"]), set(la["last"])) == (rpp, idle, rows, grid, chunks, full, last), shape
        assert la["grid"] <= EC.MAX_BLOCKS and la["rows"] % la["rpp"] == 0 and (la["grid"] - 1) * la["rows"] < shape[0] <= la["grid"] * la["rows"]


def test_reduce_shapes_reach_every_launch_class():
    seen = set()
    for shape in EC.REDUCE_SHAPES:
        seen |= EC.launch_classes(*shape)
    assert seen == EC.ALL_CLASSES, EC.ALL_CLASSES ^ seen
    # the shapes of the BatchNorm-backward tests are reduction shapes, and the 3 x 9 x 13 map is the output of a pool case and an up-sampling case
    assert (351, 128) in EC.REDUCE_SHAPES and (2, 2, 0, 3, 18, 26, 128) in EC.POOL_CASES and (3, 9, 13, 128) in EC.UPSAMPLE_CASES
    assert any(c[:3] == (2, 2, 0) for c in EC.POOL_CASES) and any(c[:3] != (2, 2, 0) for c in EC.POOL_CASES)      # the fast path and the general one


def _three_orders(v, g):
    """float32 column sums of v (n, C) in three orders: forward (cumsum), reversed (cumsum), a seeded permutation summed in chunks of 7 rows"""
    n = v.shape[0]
    fwd = torch.cumsum(v, 0)[-1]
    rev = torch.cumsum(v.flip(0), 0)[-1]
    pv = v[torch.randperm(n, generator=g)]
    pad = (-n) % 7
    pv = torch.cat([pv, torch.zeros(pad, v.shape[1])]) if pad else pv
    chunked = torch.cumsum(pv.view(-1, 7, v.shape[1]).sum(1), 0)[-1]
    return fwd, rev, chunked


@pytest.mark.parametrize("shape", EC.REDUCE_SHAPES, ids=ids)
def test_exact_inputs_are_exact_in_fp32_in_any_order(shape):
    npix, C = shape
    assert EC.exact_bound_holds(npix)
    Cs = min(C, 64)                                                  # (the bound does not depend on the channel: a slice keeps the test quick)
    g = torch.Generator().manual_seed(npix)
    x = EC.exact_inputs("stats", npix, C)["x"]
    assert x.dtype == torch.float32 and torch.equal(x, x.round()) and float(x.abs().max()) <= 4
    x = x[:, :Cs]
    shifted = x - x[0]                                               # what the kernels sum: shifted by a first row
    terms = {"sum": x, "shifted": shifted, "shifted squares": shifted * shifted}
    d = EC.exact_inputs("bnbwd", npix, C)
    assert float(d["dout"].abs().max()) <= 4 and float(d["y"].abs().max()) <= 8 and float(d["mean"].abs().max()) <= 3
    assert set(d["invstd"].tolist()) <= {0.5, 1.0, 2.0} and set(d["mask_scale"].tolist()) <= {-1.0, 1.0, 2.0} and set(d["mask_shift"].tolist()) <= {-2.0, 0.0, 1.0}
    if npix * C >= 1000:
        assert float((d["act"] <= 0).float().mean()) > 0.4 and float((d["act"] == 0).float().mean()) > 0.1 and float((d["mask_scale"] < 0).float().mean()) > 0.1
    for mask in EC.MASKS:
        gm = d["dout"]
        if mask == "act":
            gm = gm * (d["act"] > 0)
        elif mask == "affine":
            gm = gm * (d["y"] * d["mask_scale"] + d["mask_shift"] > 0)
        xhat = (d["y"] - d["mean"]) * d["invstd"]
        assert float((gm * xhat).abs().max()) <= 88 and torch.equal(gm * xhat * 2, (gm * xhat * 2).round())
        terms["g " + mask], terms["g xhat " + mask] = gm[:, :Cs], (gm * xhat)[:, :Cs]
    for name, v in terms.items():
        ref = v.double().sum(0)
        for got in _three_orders(v, g):
            assert got.dtype == torch.float32 and torch.equal(got.double(), ref), (name, shape)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("case", EC.POOL_CASES, ids=ids)
@pytest.mark.parametrize("data", ["real", "exact", "exact affine"])
def test_maxpool_references_agree_with_torch_on_every_tie(case, data):
    k, s, p, B, H, W, C = case
    if data == "real":
        x = EC.pool_data(case)
        assert float((x == 0).float().mean()) > 0.3                                 # ties are present
    else:
        x, sc, sh = EC.exact_pool_inputs(case, data == "exact affine")
        if sc is not None:
            x = (x * sc + sh).clamp(min=0)
        assert torch.equal(x, x.round()) and float(x.abs().max()) <= 4
    out, arg = EC.maxpool_ref(x, k, s, p)
    Ho, Wo = EC.pool_out(k, s, p, H, W)
    assert out.shape == (B, Ho, Wo, C) and arg.dtype == torch.uint8
    xd = _nchw(x).double().requires_grad_(True)
    ref, idx = TF.max_pool2d(xd, k, s, p, return_indices=True)
    assert torch.equal(out, _nhwc(ref.detach()))
    iy, ix = idx // W, idx % W                                                       # flat index into the H x W map -> window code
    oy, ox = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    code = (iy - (oy * s - p)) * k + (ix - (ox * s - p))
    assert int(code.min()) >= 0 and int(code.max()) < k * k
    assert torch.equal(arg.long(), _nhwc(code))                                      # every tie resolved the same way
    dout = EC.rnd(torch.Generator().manual_seed(11), B, Ho, Wo, C)
    (gx,) = torch.autograd.grad(ref, xd, _nchw(dout).double())
    dx = EC.maxpool_bwd_ref(dout, arg, k, s, p, H, W)
    assert dx.shape == (B, H, W, C) and float((dx - _nhwc(gx)).abs().max()) < 1e-12
    if (k, s, p, H, W) == (2, 2, 0, 9, 7):                                           # the uncovered last row and column get no gradient
        assert float(dx[:, 8].abs().max()) == 0.0 and float(dx[:, :, 6].abs().max()) == 0.0 and float(dx[:, :8, :6].abs().max()) > 0


@pytest.mark.parametrize("case", EC.UPSAMPLE_CASES, ids=ids)
def test_upsample_references_agree_with_torch(case):
    B, Hl, Wl, C = case
    g = torch.Generator().manual_seed(12)
    up1, low = EC.rnd(g, B, 2 * Hl, 2 * Wl, C), EC.rnd(g, B, Hl, Wl, C)
    lowd = _nchw(low).double().requires_grad_(True)
    ref = _nchw(up1).double() + TF.interpolate(lowd, scale_factor=2, mode="nearest")
    assert torch.equal(EC.upsample2_add_ref(up1, low), _nhwc(ref.detach()))
    dout = EC.rnd(g, B, 2 * Hl, 2 * Wl, C)
    (gl,) = torch.autograd.grad(ref, lowd, _nchw(dout).double())
    assert float((EC.upsample2_bwd_ref(dout) - _nhwc(gl)).abs().max()) < 1e-12
    e1, e2 = EC.exact_upsample_inputs(case)
    s = EC.upsample2_add_ref(e1, e2)
    assert torch.equal(s, s.round()) and float(s.abs().max()) <= 4


@pytest.mark.parametrize("shape", [(65, 96), (351, 128)], ids=ids)
@pytest.mark.parametrize("residual", [False, True])
def test_batchnorm_references_agree_with_autograd(shape, residual):
    """y -> relu(batch_norm(y) [+ res]) in float64: the backward reference (act mask; without a residual also the affine mask) against autograd,
    lin4 against the same dy, bn_finalize_ref against F.batch_norm's values and running-statistic update"""
    npix, C = shape
    eps, mom = 1e-5, 0.1
    d = EC.real_inputs("bnbwd", npix, C)
    g = torch.Generator().manual_seed(13)
    beta, res = EC.rnd(g, C), EC.rnd(g, npix, C)
    rm, rv = EC.rnd(g, C), EC.rnd(g, C) + 1.5
    yd, gd, bd = d["y"].double().requires_grad_(True), d["gamma"].double().requires_grad_(True), beta.double().requires_grad_(True)
    rm_t, rv_t = rm.double().clone(), rv.double().clone()
    z = TF.batch_norm(yd.t().reshape(1, C, npix), rm_t, rv_t, gd, bd, True, mom, eps).reshape(C, npix).t()      # (1, C, npix): statistics over npix
    a = TF.relu(z + res.double() if residual else z)
    dout = d["dout"]
    gy, gg, gb = torch.autograd.grad(a, [yd, gd, bd], dout.double())
    s1, s2 = EC.stats_ref(d["y"])
    scale, shift, mean, invstd, rm_r, rv_r = EC.bn_finalize_ref(s1, s2, npix, d["gamma"], beta, rm, rv, mom, eps)
    assert float((yd.detach() * scale + shift - z.detach()).abs().max()) < 1e-12
    assert float((rm_r - rm_t).abs().max()) < 1e-13 and float((rv_r - rv_t).abs().max()) < 1e-12
    assert float((mean - yd.detach().mean(0)).abs().max()) < 1e-13 and float((invstd - 1 / torch.sqrt(yd.detach().var(0, unbiased=False) + eps)).abs().max()) < 1e-11
    r = EC.bn_bwd_ref(dout, d["y"], mean, invstd, d["gamma"], act=a.detach())
    assert float((r["dy"] - gy).abs().max()) < 1e-11 and float((r["dgamma"] - gg).abs().max()) < 1e-10 and float((r["dbeta"] - gb).abs().max()) < 1e-11
    assert torch.equal(r["g"], dout.double() * (a.detach() > 0))
    extra = EC.rnd(g, npix, C)
    r2 = EC.bn_bwd_ref(dout, d["y"], mean, invstd, d["gamma"], act=a.detach(), dy_add=extra)
    assert float((r2["dy"] - (r["dy"] + extra.double())).abs().max()) < 1e-12
    if not residual:        # the mask re-derived from y with the forward's scale / shift
        assert float((yd.detach() * scale + shift).abs().min()) > 1e-9
        r3 = EC.bn_bwd_ref(dout, d["y"], mean, invstd, d["gamma"], mask_scale=scale, mask_shift=shift)
        assert torch.equal(r3["g"], r["g"]) and float((r3["dy"] - r["dy"]).abs().max()) < 1e-12
    lin = EC.lin4_ref(r["s1"], r["s2"], npix, d["gamma"], mean, invstd)
    assert float((lin[0] * r["g"] + lin[1] * (yd.detach() - lin[3]) + lin[2] - r["dy"]).abs().max()) < 1e-11
    # no ReLU at all, gamma = None
    yd2 = d["y"].double().requires_grad_(True)
    z2 = TF.batch_norm(yd2.t().reshape(1, C, npix), None, None, None, None, True, mom, eps).reshape(C, npix).t()
    (gy2,) = torch.autograd.grad(z2, yd2, dout.double())
    assert float((EC.bn_bwd_ref(dout, d["y"], mean, invstd)["dy"] - gy2).abs().max()) < 1e-11


def test_bn_finalize_reference_edges():
    """a constant channel (variance clamped at exactly 0), count == 1 (the running variance takes the biased value), absent parameters"""
    C, eps = 4, 1e-5
    x = torch.full((7, C), 5.0)
    s1, s2 = EC.stats_ref(x)
    scale, shift, mean, invstd, rm, rv = EC.bn_finalize_ref(s1, s2, 7, None, None, None, torch.ones(C), 0.1, eps)
    assert rm is None and torch.equal(mean, torch.full((C,), 5.0, dtype=torch.float64)) and torch.equal(rv, torch.full((C,), 0.9, dtype=torch.float64))
    assert torch.equal(invstd, torch.full((C,), eps, dtype=torch.float64).rsqrt()) and torch.equal(scale, invstd) and torch.equal(shift, -5 * invstd)
    x1 = torch.tensor([[1.0, -2.0, 0.5, 3.0]])
    s1, s2 = EC.stats_ref(x1)
    _, _, mean, invstd, rm, rv = EC.bn_finalize_ref(s1, s2, 1, None, None, torch.zeros(C), torch.ones(C), 0.5, eps)
    assert torch.equal(mean, x1[0].double()) and torch.equal(rm, 0.5 * x1[0].double()) and torch.equal(rv, torch.full((C,), 0.5, dtype=torch.float64))


def test_real_inputs_are_seeded_and_in_the_stated_range():
    for shape in [(351, 128), (65, 96), (131, 2048), (4099, 64)]:
        a, b = EC.real_inputs("bnbwd", *shape), EC.real_inputs("bnbwd", *shape)
        assert all(torch.equal(a[k], b[k]) for k in a)
        assert float((a["gamma"] < 0).float().mean()) > 0 and float((a["act"] == 0).float().mean()) > 0.2
    x = EC.real_inputs("stats", 4099, 64)["x"]
    assert abs(float(x.mean()) - 3.0) < 0.05 and abs(float(x.std()) - 0.5) < 0.05
