"""Bodies of the operator checks of the implicit-GEMM convolution family (awr_conv_gemm, awr_conv_wgrad) on an H x W feature map, shared by
tests/test_ops_gpu.py (square maps, W = H) and tests/test_conv_rect_gpu.py (rectangular maps).  A plain helper module, not a conftest: every
function takes the `ops` / `_lib` modules and the device, asserts what the test of its name asserts, and returns the errors it measured
({name: relative error}) so a caller can print or tabulate them.  References: float64 torch conv2d / conv_transpose2d and autograd on the CPU,
or the second launch form of the same operator (algo 1, the two-launch pair, the materialised d(y), register staging)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as TF

_KEEP = []


def DP(L, t, dev):
    """device pointer of a host tensor; the device copy is kept alive until the module is torn down
    (a temporary freed right after data_ptr() would be recycled by the caching allocator)."""
    d = t.to(dev)
    _KEEP.append(d)
    return L.ptr(d)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def rel_err(a, ref):
    ref = ref.double()
    return float((a.double() - ref).abs().max() / (ref.abs().max() + 1e-30))


def torch_fwd(kind, x, w, b, stride, pad):
    return (TF.conv2d if kind == "conv" else TF.conv_transpose2d)(x, w, b, stride, pad)


def wshape_of(kind, cin, cout, k):
    return (cout, cin, k, k) if kind == "conv" else (cin, cout, k, k)


def input_hw(kind, stride, H, W):
    """Input size of the layer whose GEMM row map (Hq x Wq forward and data gradient, Hd x Wd weight gradient) is H x W: a stride-2 conv
    reads a map twice that size; a stride-1 conv and a transposed conv (which writes twice it) read H x W."""
    return (2 * H, 2 * W) if kind == "conv" and stride == 2 else (H, W)


# ---- forward, data gradient, weight gradient, bias gradient, the two accumulate forms -------------------------------------------------------
@functools.lru_cache(maxsize=4)      # the tile / product / staging cases of one geometry run back to back: a few entries share every reference
def _layer_reference(kind, cin, cout, k, stride, pad, B, H, W):
    """Inputs and float64 results of one layer: computed once per geometry, shared by every tile / product mode / staging that checks it
    (read-only: nothing below writes into these tensors)."""
    w = rnd(*wshape_of(kind, cin, cout, k), seed=1, scale=(cin * k * k) ** -0.5)
    x = rnd(B, cin, H, W, seed=2)
    bias = rnd(cout, seed=3)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y_ref = torch_fwd(kind, xd, wd, bias.double(), stride, pad)
    gy = rnd(*y_ref.shape, seed=4)
    gx_ref, gw_ref = torch.autograd.grad(y_ref, [xd, wd], gy.double())
    base = rnd(B, cin, H, W, seed=5)
    return w, x, bias, y_ref.detach(), gy, gx_ref, gw_ref, base


def conv_forward_dgrad_wgrad(ops, dev, kind, cin, cout, k, stride, pad, B, H, W=None):
    W = H if W is None else W
    spec = ops.ConvSpec(kind, cin, cout, k, stride, pad)
    w, x, bias, y_ref, gy, gx_ref, gw_ref, base = _layer_reference(kind, cin, cout, k, stride, pad, B, H, W)
    errs = {}

    wg = w.to(dev)
    wp = ops.pack_weight(wg, spec.fwd_pack())
    y = ops.conv_forward(spec, ops.nhwc(x).to(dev), wp, bias=bias.to(dev))
    # fp32 MFMA == k-ordered fmaf chain: rounding error grows ~ sqrt(K) * 2^-24 relative to the row scale
    tol = 5e-6
    errs["fwd"] = rel_err(ops.nchw(y).cpu(), y_ref)
    assert errs["fwd"] < tol
    wpd = ops.pack_weight(wg, spec.dgrad_pack())
    gx = ops.conv_dgrad(spec, ops.nhwc(gy).to(dev), wpd, H, W)
    errs["dgrad"] = rel_err(ops.nchw(gx).cpu(), gx_ref)
    assert errs["dgrad"] < tol
    bg = torch.empty(cout, device=dev) if kind == "conv" else None
    gw = ops.conv_wgrad(spec, ops.nhwc(x).to(dev), ops.nhwc(gy).to(dev), bias_grad=bg)
    errs["wgrad"] = rel_err(gw.cpu(), gw_ref)
    assert errs["wgrad"] < 1e-5
    if bg is not None:       # the bias gradient falls out of the same kernel (column sums of dY)
        errs["bgrad"] = rel_err(bg.cpu(), gy.double().sum((0, 2, 3)))
        assert errs["bgrad"] < 1e-5
    # accumulate paths: dgrad onto an existing gradient, wgrad onto an existing gradient
    acc = ops.nhwc(base).to(dev)
    ops.conv_dgrad(spec, ops.nhwc(gy).to(dev), wpd, H, W, out=acc, res=acc)
    errs["dgrad_acc"] = rel_err(ops.nchw(acc).cpu(), gx_ref + base.double())
    assert errs["dgrad_acc"] < tol
    gw2 = ops.conv_wgrad(spec, ops.nhwc(x).to(dev), ops.nhwc(gy).to(dev), grad=gw.clone(), accumulate=True)
    errs["wgrad_acc"] = rel_err(gw2.cpu(), 2 * gw_ref)
    assert errs["wgrad_acc"] < 1e-5
    return errs


def conv_every_tile_shape(ops, L, dev, products, staging, tm, tn, kind, cin, cout, k, stride, pad, B, H, W=None):
    """One forced workgroup tile, product mode and operand staging around conv_forward_dgrad_wgrad; the process-wide modes are restored."""
    L.call("awr_debug_force_tile", tm, tn)
    L.call("awr_set_gemm_products", products)
    L.call("awr_set_gemm_staging", staging)
    try:
        return conv_forward_dgrad_wgrad(ops, dev, kind, cin, cout, k, stride, pad, B, H, W)
    finally:
        L.call("awr_debug_force_tile", 0, 0)
        L.call("awr_set_gemm_products", 1)
        L.call("awr_set_gemm_staging", 2)


# ---- split-operand mode with a pre-cut activation image (study builds) ---------------------------------------------------------------------
def split_mode_with_precut_activations(ops, L, dev, tm, tn, kind, cin, cout, k, stride, pad, B, H, W=None):
    W = H if W is None else W
    spec = ops.ConvSpec(kind, cin, cout, k, stride, pad)
    x = rnd(B, cin, H, W, seed=1)
    w = rnd(*wshape_of(kind, cin, cout, k), seed=2, scale=0.05)
    prob = spec.fwd_problem(H, W)
    xin = ops.nhwc(x).to(dev)
    if prob["Cin"] != cin:
        xin = torch.nn.functional.pad(xin, (0, prob["Cin"] - cin))
    xin = xin.contiguous()
    errs = {}
    L.call("awr_set_gemm_products", 6)
    try:
        wp = ops.pack_weight(w.to(dev), spec.fwd_pack())
        ops.split_packed(wp)
        bias = rnd(prob["N"], seed=3).to(dev)
        res = rnd(B, prob["Hout"], prob["Wout"], prob["N"], seed=4).to(dev)
        sc, sh = (rnd(prob["Cin"], seed=5) + 1.5).to(dev), rnd(prob["Cin"], seed=6).to(dev)
        for form in ("plain", "epilogue", "stats", "bn_input"):
            outs = []
            for pre in (False, True):
                out = torch.full((B, prob["Hout"], prob["Wout"], prob["N"]), float("nan"), device=dev)
                kw = {}
                if form in ("epilogue", "stats"):
                    kw = dict(bias=bias, res=res, relu_out=True)
                st = torch.zeros(16, 2, prob["N"], device=dev, dtype=torch.float64) if form == "stats" else None
                if form == "bn_input":
                    if pre:
                        kw["in_split"] = ops.split_act(xin, sc, sh, True)
                    else:
                        kw.update(in_scale=sc, in_shift=sh, relu_in=True)
                elif pre:
                    kw["in_split"] = ops.split_act(xin)
                a = ops.make_conv_args(prob, B, xin, wp, out, stats=st, T=spec.T, **kw)
                a.tile_m, a.tile_n = tm, tn
                L.call("awr_conv_gemm", C.byref(a), L.stream())
                torch.cuda.synchronize()
                outs.append((out.clone(), None if st is None else st.sum(0).float()))
            (o0, s0), (o1, s1) = outs
            assert not torch.isnan(o1).any(), form
            assert torch.equal(o0, o1), (form, float((o0 - o1).abs().max()))
            if s0 is not None:
                assert rel_err(s1.cpu(), s0.cpu()) < 1e-6
        # and against float64
        ref = TF.conv2d(x.double(), w.double(), None, stride, pad) if kind == "conv" else TF.conv_transpose2d(x.double(), w.double(), None, stride, pad)
        out = torch.empty(B, prob["Hout"], prob["Wout"], prob["N"], device=dev)
        a = ops.make_conv_args(prob, B, xin, wp, out, T=spec.T, in_split=ops.split_act(xin))
        a.tile_m, a.tile_n = tm, tn
        L.call("awr_conv_gemm", C.byref(a), L.stream())
        errs["fwd"] = rel_err(ops.nchw(out)[:, :cout].cpu(), ref)
        assert errs["fwd"] < 2e-6
    finally:
        L.call("awr_set_gemm_products", 1)
    return errs


# ---- LDS-DMA staging against register staging ----------------------------------------------------------------------------------------------
# input maps of the sub-cases of lds_dma_staging_vs_register_staging, as the square test has always run them
SQUARE_STAGING_MAPS = dict(a=(18, 18), b=((20, 20), (10, 10), (12, 12)), c=(12, 12), d=(10, 10), e=(14, 14))


def staging_maps(H, W):
    """The same sub-cases with H x W as every GEMM's row map (the strided 3x3 of (b) reads twice that).  Sub-cases (c) (two-tensor K) and (d)
    (short K) are 1x1 stride-1 convs: pointwise, so a non-square map shows them ragged M and the row count, not a swapped row stride."""
    return dict(a=(H, W), b=((2 * H, 2 * W), (H, W), (H, W)), c=(H, W), d=(H, W), e=(H, W))


def lds_dma_staging_vs_register_staging(ops, L, dev, tm, tn, maps=None):
    maps = SQUARE_STAGING_MAPS if maps is None else maps
    outs, keep, errs = {}, [], {}

    def D(t):      # device copy kept alive until the test ends (make_conv_args only stores raw pointers)
        keep.append(t.to(dev).contiguous())
        return keep[-1]
    # 0 = register staging; 2 = LDS-DMA: these small launches take the deep pipeline (four stage buffers, round 5); "2s" = LDS-DMA with the
    # deep pipeline switched off (two stage buffers, what the chip-filling launches run)
    for staging in (0, 2, "2s"):
        L.call("awr_set_gemm_staging", 2 if staging == "2s" else staging)
        L.call("awr_debug_set_knob", b"deep", 0 if staging == "2s" else 1)
        try:
            got = []
            # (a) fused prologue + full epilogue, ragged N
            (H, W), B, cin, cout = maps["a"], 3, 64, 96
            spec = ops.ConvSpec("conv", cin, cout, 3, 1, 1)
            x, w = rnd(B, cin, H, W, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.05)
            s_, t_ = rnd(cin, seed=3) + 1.5, rnd(cin, seed=4)
            so, to, bias, res = rnd(cout, seed=5) + 1.5, rnd(cout, seed=6), rnd(cout, seed=7), rnd(B, cout, H, W, seed=8)
            wp = ops.pack_weight(D(w), spec.fwd_pack())
            stats = torch.zeros(16, 2, cout, device=dev, dtype=torch.float64)
            prob = spec.fwd_problem(H, W)
            out = torch.full((B, H, W, prob["N"]), float("nan"), device=dev)
            a = ops.make_conv_args(prob, B, D(ops.nhwc(x)), wp, out, in_scale=D(s_), in_shift=D(t_), relu_in=True, bias=D(bias),
                                   out_scale=D(so), out_shift=D(to), res=D(ops.nhwc(res)), relu_out=True, stats=stats, T=spec.T)
            a.tile_m, a.tile_n = tm, tn
            L.call("awr_conv_gemm", C.byref(a), L.stream())
            got += [out.clone(), stats.sum(0).float()]
            # (a2) the same without the statistics: the reduction-free epilogue (bias, folded BatchNorm, residual, ReLU)
            out2 = torch.full((B, H, W, prob["N"]), float("nan"), device=dev)
            a2 = ops.make_conv_args(prob, B, D(ops.nhwc(x)), wp, out2, in_scale=D(s_), in_shift=D(t_), relu_in=True, bias=D(bias),
                                    out_scale=D(so), out_shift=D(to), res=D(ops.nhwc(res)), relu_out=True, T=spec.T)
            a2.tile_m, a2.tile_n = tm, tn
            L.call("awr_conv_gemm", C.byref(a2), L.stream())
            got.append(out2.clone())
            # (b) strided conv, transposed conv, plain activations (both operands by DMA), ragged M
            for (kind, ci, co, k, st, p), (hh, ww_) in zip((("conv", 128, 160, 3, 2, 1), ("deconv", 64, 96, 4, 2, 1), ("conv", 96, 64, 1, 1, 0)), maps["b"]):
                sp = ops.ConvSpec(kind, ci, co, k, st, p)
                xx = rnd(2, ci, hh, ww_, seed=11)
                ww = rnd(*wshape_of(kind, ci, co, k), seed=12, scale=0.05)
                pr = sp.fwd_problem(hh, ww_)
                xin = ops.nhwc(xx)
                if pr["Cin"] != ci:
                    xin = torch.nn.functional.pad(xin, (0, pr["Cin"] - ci))
                oo = torch.full((2, pr["Hout"], pr["Wout"], pr["N"]), float("nan"), device=dev)
                aa = ops.make_conv_args(pr, 2, D(xin), D(ops.pack_weight(D(ww), sp.fwd_pack())), oo, T=sp.T)
                aa.tile_m, aa.tile_n = tm, tn
                L.call("awr_conv_gemm", C.byref(aa), L.stream())
                got.append(oo.clone())
            # (c) two input tensors (K = [in | in2]) with the affine on the first
            (H, W), c1, c2, co = maps["c"], 64, 128, 160
            xa, xb = rnd(2, c1, H, W, seed=21), rnd(2, c2, H, W, seed=22)
            wab = rnd(co, c1 + c2, 1, 1, seed=23, scale=0.1)
            sp = ops.ConvSpec("conv", c1 + c2, co, 1, 1, 0)
            pr = sp.fwd_problem(H, W)
            oo = torch.full((2, H, W, pr["N"]), float("nan"), device=dev)
            st2 = torch.zeros(16, 2, pr["N"], device=dev, dtype=torch.float64)
            sa, ta = rnd(c1, seed=24) + 1.2, rnd(c1, seed=25)
            aa = ops.make_conv_args(pr, 2, D(ops.nhwc(xa)), D(ops.pack_weight(D(wab), sp.fwd_pack())), oo, in_scale=D(sa), in_shift=D(ta),
                                    relu_in=True, stats=st2, T=sp.T)
            xb_d = D(ops.nhwc(xb))
            aa.in2, aa.Cin1, aa.tile_m, aa.tile_n = L.ptr(xb_d), c1, tm, tn
            L.call("awr_conv_gemm", C.byref(aa), L.stream())
            got += [oo.clone(), st2.sum(0).float()]
            ref_c = TF.conv2d(torch.cat([TF.relu(xa.double() * sa.double().view(1, -1, 1, 1) + ta.double().view(1, -1, 1, 1)), xb.double()], 1), wab.double())
            errs["two_tensor_k"] = max(errs.get("two_tensor_k", 0.0), rel_err(ops.nchw(oo)[:, :co].cpu(), ref_c))
            assert rel_err(ops.nchw(oo)[:, :co].cpu(), ref_c) < 2e-6
            # (d) short K + one epilogue operand (prefetch form) and (e) BatchNorm-backward reduction, plain and accumulating with a stored mask
            (H, W), cin, cout, B = maps["d"], 128, 160, 3
            sp = ops.ConvSpec("conv", cin, cout, 1, 1, 0)
            x, w, res = rnd(B, cin, H, W, seed=31), rnd(cout, cin, 1, 1, seed=32, scale=0.1), rnd(B, cout, H, W, seed=33)
            pr = sp.fwd_problem(H, W)
            oo = torch.full((B, H, W, pr["N"]), float("nan"), device=dev)
            aa = ops.make_conv_args(pr, B, D(ops.nhwc(x)), D(ops.pack_weight(D(w), sp.fwd_pack())), oo, res=D(ops.nhwc(res)), T=sp.T)
            aa.tile_m, aa.tile_n = tm, tn
            L.call("awr_conv_gemm", C.byref(aa), L.stream())
            got.append(oo.clone())
            H, W = maps["e"]
            sp3 = ops.ConvSpec("conv", 64, 96, 3, 1, 1)
            gy, y, w3 = rnd(2, 96, H, W, seed=41), rnd(2, 64, H, W, seed=42), rnd(96, 64, 3, 3, seed=43, scale=0.05)
            dp = sp3.dgrad_problem(H, W)
            coef4 = torch.zeros(4, dp["N"], device=dev)
            coef4[:, :64] = torch.stack([rnd(64, seed=44) + 1.2, rnd(64, seed=45) * 0.3, rnd(64, seed=46) * 0.2, rnd(64, seed=47) + 1.5]).to(dev)
            yg = torch.zeros(2, H, W, dp["N"], device=dev)
            yg[..., :64] = D(ops.nhwc(y))
            gin = ops.nhwc(gy)
            if dp["Cin"] != 96:
                gin = torch.nn.functional.pad(gin, (0, dp["Cin"] - 96))
            for accumulate in (False, True):
                g = torch.full((2, H, W, dp["N"]), float("nan"), device=dev)
                sums = torch.zeros(16, 2, dp["N"], device=dev, dtype=torch.float64)
                d = ops.make_conv_args(dp, 2, D(gin), D(ops.pack_weight(D(w3), sp3.dgrad_pack())), g, stats=sums, T=sp3.T)
                d.bnr_y, d.bnr_coef, d.tile_m, d.tile_n = L.ptr(yg), L.ptr(coef4), tm, tn
                if accumulate:
                    act = D(ops.nhwc(rnd(2, dp["N"], H, W, seed=48)))
                    g.copy_(ops.nhwc(rnd(2, dp["N"], H, W, seed=49)).to(dev))
                    d.bnr_act, d.res = L.ptr(act), L.ptr(g)
                L.call("awr_conv_gemm", C.byref(d), L.stream())
                torch.cuda.synchronize()
                got += [g.clone(), sums.sum(0).float()]
            outs[staging] = got
        finally:
            L.call("awr_set_gemm_staging", 2)
            L.call("awr_debug_set_knob", b"deep", 1)
    for other in (2, "2s"):
        assert len(outs[0]) == len(outs[other])
        for i, (p, q) in enumerate(zip(outs[0], outs[other])):
            if p.dtype == torch.float32 and p.dim() == 2:        # statistics: fp64 atomics in launch order, compared after rounding to fp32
                assert rel_err(q.cpu(), p.cpu()) < 1e-6, (other, i)
            else:
                assert torch.equal(torch.nan_to_num(p, nan=-1234.0), torch.nan_to_num(q, nan=-1234.0)), (other, i)
    return errs


# ---- data gradient that applies the BatchNorm backward to its operand -----------------------------------------------------------------------
def dgrad_with_unmaterialised_batchnorm_backward(ops, L, dev, accum, tm, tn, kind, cin, cout, k, stride, pad, B, H, W=None):
    W = H if W is None else W
    spec = ops.ConvSpec(kind, cin, cout, k, stride, pad)
    ho, wo = spec.out_hw(H, W)
    w = rnd(*wshape_of(kind, cin, cout, k), seed=2, scale=0.05)
    g, y = rnd(B, cout, ho, wo, seed=3), rnd(B, cout, ho, wo, seed=4) * 2.0 + 0.7
    gamma = rnd(cout, seed=5) + 1.5
    # reduction sums as the fused epilogue leaves them: sum g and sum g * xhat per channel (one slot)
    mean = y.double().mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(y.double().var((0, 2, 3), unbiased=False) + 1e-5)
    xhat = (y.double() - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    npix = B * ho * wo
    dp = spec.dgrad_problem(H, W)
    Cp = dp["Cin"]
    sums = torch.zeros(16, 2, Cp, dtype=torch.float64)
    sums[0, 0, :cout] = g.double().sum((0, 2, 3))
    sums[0, 1, :cout] = (g.double() * xhat).sum((0, 2, 3))
    dy_ref = (gamma.double() * invstd).view(1, -1, 1, 1) * (g.double() - (sums[0, 0, :cout] / npix).view(1, -1, 1, 1) - xhat * (sums[0, 1, :cout] / npix).view(1, -1, 1, 1))
    gx_ref = (TF.conv_transpose2d(dy_ref, w.double(), None, stride, pad, output_padding=((H + 2 * pad - k) % stride, (W + 2 * pad - k) % stride)) if kind == "conv"
              else TF.conv2d(dy_ref, w.double(), None, stride, pad))

    def padc(t, fill=0.0):      # NHWC with the channel padding of the GEMM's K extent
        t = ops.nhwc(t)
        return (torch.nn.functional.pad(t, (0, Cp - cout), value=fill) if Cp != cout else t).contiguous().to(dev)
    g_d, y_d = padc(g), padc(y)
    vec = lambda v, fill: torch.nn.functional.pad(v.float(), (0, Cp - cout), value=fill).to(dev)
    mean_d, invstd_d, gamma_d = vec(mean, 0.0), vec(invstd, 1.0), vec(gamma, 1.0)
    sums_d, coef, lin4 = sums.to(dev), torch.zeros(3, Cp, device=dev), torch.zeros(4, Cp, device=dev)
    dgam, dbet = torch.zeros(Cp, device=dev), torch.zeros(Cp, device=dev)
    L.call("awr_bn_bwd_finalize_lin", L.ptr(sums_d), Cp, npix, L.ptr(gamma_d), L.ptr(mean_d), L.ptr(invstd_d), L.ptr(coef), L.ptr(lin4), L.ptr(dgam), L.ptr(dbet), 0, 16, L.stream())
    assert rel_err(dgam[:cout].cpu(), (g.double() * xhat).sum((0, 2, 3))) < 1e-5 and rel_err(dbet[:cout].cpu(), g.double().sum((0, 2, 3))) < 1e-5
    assert float(sums_d.abs().max()) == 0.0          # the accumulator is re-armed
    dy_mat = torch.empty_like(g_d)
    L.call("awr_bn_bwd_apply_only", L.ptr(g_d), None, L.ptr(y_d), L.ptr(mean_d), L.ptr(invstd_d), None, None, L.ptr(coef), npix, Cp, L.ptr(dy_mat), None, None, L.stream())
    assert rel_err(ops.nchw(dy_mat)[:, :cout].cpu(), dy_ref) < 2e-6
    wd = ops.pack_weight(w.to(dev), spec.dgrad_pack())
    outs, errs = [], {}
    for lazy in (False, True):
        out = torch.full((B, H, W, dp["N"]), float("nan"), device=dev)
        if not dp["full"]:
            out.zero_()
        a = ops.make_conv_args(dp, B, g_d if lazy else dy_mat, wd, out, res=None if dp["full"] else out, T=spec.T)
        a.tile_m, a.tile_n, a.accum = tm, tn, accum
        if lazy:
            a.in_bnb_y, a.in_bnb_coef = L.ptr(y_d), L.ptr(lin4)
        L.call("awr_conv_gemm", C.byref(a), L.stream())
        torch.cuda.synchronize()
        outs.append(ops.nchw(out)[:, :cin].cpu())
        errs["lazy" if lazy else "materialised"] = rel_err(outs[-1], gx_ref)
        assert rel_err(outs[-1], gx_ref) < 3e-6, lazy
    errs["lazy_vs_materialised"] = rel_err(outs[1], outs[0])
    assert rel_err(outs[1], outs[0]) < 2e-6
    return errs


# ---- fused prologue / epilogue / statistics -------------------------------------------------------------------------------------------------
def conv_fused_prologue_epilogue_stats(ops, dev, B=2, H=16, cin=64, cout=96, W=None):
    W = H if W is None else W
    spec = ops.ConvSpec("conv", cin, cout, 3, 1, 1)
    x, w = rnd(B, cin, H, W, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.05)
    s, t = rnd(cin, seed=3) + 1.5, rnd(cin, seed=4)
    so, to, bias = rnd(cout, seed=5) + 1.5, rnd(cout, seed=6), rnd(cout, seed=7)
    res = rnd(B, cout, H, W, seed=8)
    a = TF.relu(x.double() * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1))
    pre = (TF.conv2d(a, w.double(), bias.double(), 1, 1)) * so.double().view(1, -1, 1, 1) + to.double().view(1, -1, 1, 1) + res.double()
    ref = TF.relu(pre)
    stats = torch.zeros(16, 2, cout, device=dev, dtype=torch.float64)
    wp = ops.pack_weight(w.to(dev), spec.fwd_pack())
    y = ops.conv_forward(spec, ops.nhwc(x).to(dev), wp, in_scale=s.to(dev), in_shift=t.to(dev), relu_in=True, bias=bias.to(dev),
                         out_scale=so.to(dev), out_shift=to.to(dev), res=ops.nhwc(res).to(dev), relu_out=True, stats=stats)
    errs = dict(fwd=rel_err(ops.nchw(y).cpu(), ref), sum=rel_err(stats.sum(0)[0].cpu(), pre.sum((0, 2, 3))),
                sumsq=rel_err(stats.sum(0)[1].cpu(), (pre * pre).sum((0, 2, 3))))
    assert errs["fwd"] < 2e-6
    assert errs["sum"] < 1e-5          # [AWR_STAT_SLOTS][2][N]
    assert errs["sumsq"] < 1e-5
    return errs


def stem_im2col_gemm(ops, L, dev, B=2, H=32, W=None):
    W = H if W is None else W
    img, w = rnd(B, 1, H, W, seed=1), rnd(64, 1, 5, 5, seed=2, scale=0.2)
    wd = w.double().requires_grad_(True)
    ref = TF.conv2d(img.double(), wd, None, 1, 2)
    gy = rnd(*ref.shape, seed=3)
    (gw_ref,) = torch.autograd.grad(ref, wd, gy.double())
    cols = torch.empty(B, H, W, 32, device=dev)
    L.call("awr_stem_im2col", DP(L, img, dev), B, H, W, L.ptr(cols), L.stream())
    spec = ops.ConvSpec("conv", 25, 64, 1, 1, 0, cin_pad=32)
    wp = ops.pack_weight(w.to(dev).view(64, 25, 1, 1), spec.fwd_pack())
    y = ops.conv_forward(spec, cols, wp)
    errs = dict(fwd=rel_err(ops.nchw(y).cpu(), ref.detach()))
    assert errs["fwd"] < 2e-6
    gw = ops.conv_wgrad(spec, cols, ops.nhwc(gy).to(dev))
    errs["wgrad"] = rel_err(gw.cpu().view(64, 1, 5, 5), gw_ref)
    assert errs["wgrad"] < 5e-6
    return errs


# ---- split-K ----------------------------------------------------------------------------------------------------------------------------------
def conv_split_k(ops, dev, kind, cin, cout, k, stride, B, H, W=None):
    W = H if W is None else W
    pad = 1 if k > 1 else 0
    spec = ops.ConvSpec(kind, cin, cout, k, stride, pad)
    w = rnd(*wshape_of(kind, cin, cout, k), seed=1, scale=(cin * k * k) ** -0.5)
    x = rnd(B, cin, H, W, seed=2)
    bias, osc, osh = rnd(cout, seed=3), rnd(cout, seed=4) + 1.5, rnd(cout, seed=5)
    isc, ish = rnd(cin, seed=6) + 0.5, rnd(cin, seed=7) * 0.3
    a_in = TF.relu(x.double() * isc.double().view(1, -1, 1, 1) + ish.double().view(1, -1, 1, 1))
    y0 = torch_fwd(kind, a_in, w.double(), bias.double(), stride, pad)
    res = rnd(*y0.shape, seed=8)
    y_ref = TF.relu(y0 * osc.double().view(1, -1, 1, 1) + osh.double().view(1, -1, 1, 1) + res.double())
    wp = ops.pack_weight(w.to(dev), spec.fwd_pack())
    kw = dict(bias=bias.to(dev), out_scale=osc.to(dev), out_shift=osh.to(dev), res=ops.nhwc(res).to(dev), relu_out=True,
              in_scale=isc.to(dev), in_shift=ish.to(dev), relu_in=True)
    xg = ops.nhwc(x).to(dev)
    y1 = ops.conv_forward(spec, xg, wp, **kw)
    errs = dict(single_pass=rel_err(ops.nchw(y1).cpu(), y_ref))
    assert errs["single_pass"] < 5e-6
    for sk in (0, 2, 4, 8):
        part = torch.full((8,) + tuple(y1.shape), float("nan"), device=dev)      # every copy the launch reads must have been written
        y2 = ops.conv_forward(spec, xg, wp, partial=part, split_k=sk, **kw)
        errs["split_k"] = max(errs.get("split_k", 0.0), rel_err(ops.nchw(y2).cpu(), y_ref))
        assert rel_err(ops.nchw(y2).cpu(), y_ref) < 5e-6, sk
        assert float((y2 - y1).abs().max()) <= 2e-5 * float(y1.abs().max()), sk
    y3 = ops.conv_forward(spec, xg, wp, partial=part, split_k=4, **kw)
    assert torch.equal(ops.conv_forward(spec, xg, wp, partial=part, split_k=4, **kw), y3)      # fixed summation order
    return errs


# ---- weight-gradient algorithms -------------------------------------------------------------------------------------------------------------
def wgrad_one_wave_per_tap(ops, L, dev, kind, cin, cout, k, stride, B, H, W=None):
    W = H if W is None else W
    spec = ops.ConvSpec(kind, cin, cout, k, stride, 1)
    wshape = wshape_of(kind, cin, cout, k)
    x = rnd(B, cin, H, W, seed=2)
    s_, t_ = rnd(cin, seed=5) + 0.3, rnd(cin, seed=6) * 0.5
    a = TF.relu(x * s_.view(1, -1, 1, 1) + t_.view(1, -1, 1, 1))
    wd = torch.zeros(*wshape, dtype=torch.float64, requires_grad=True)
    y_ref = torch_fwd(kind, a.double(), wd, None, stride, 1)
    gy = rnd(*y_ref.shape, seed=4)
    (gw_ref,) = torch.autograd.grad(y_ref, [wd], gy.double())
    xg, gyg = ops.nhwc(x).to(dev), ops.nhwc(gy).to(dev)
    aff = (s_.to(dev), t_.to(dev), True)
    bg = torch.empty(cout, device=dev) if kind == "conv" else None
    gw = ops.conv_wgrad(spec, xg, gyg, x_affine=aff, bias_grad=bg, algo=2)
    errs = dict(wgrad=rel_err(gw.cpu(), gw_ref))
    assert errs["wgrad"] < 1e-5
    if bg is not None:
        errs["bgrad"] = rel_err(bg.cpu(), gy.double().sum((0, 2, 3)))
        assert errs["bgrad"] < 1e-5
    old = ops.conv_wgrad(spec, xg, gyg, x_affine=aff, algo=1)
    errs["vs_algo1"] = rel_err(gw.cpu(), old.cpu())
    assert errs["vs_algo1"] < 2e-6
    # split-K depths that leave a ragged last chunk / a single chunk
    prob = spec.wgrad_problem(H, W)
    D, G = (gyg, xg) if prob["D"] == "dy" else (xg, gyg)
    for blocks in (1, 7, 100000):
        R = torch.zeros(prob["Cd"], len(prob["taps"]), prob["Cg"], device=dev)
        wa = ops.make_wgrad_args(prob, B, D, G, R, prob["Cg"], algo=2, **{"g_affine" if prob["D"] == "dy" else "d_affine": aff})
        wa.target_blocks = blocks
        L.call("awr_conv_wgrad", C.byref(wa), L.stream())
        out = torch.empty(*wshape, device=dev)
        L.call("awr_unpack_wgrad", L.ptr(R), prob["d0"], prob["d1"], spec.T, prob["Cg"], L.ptr(out), 0, L.stream())
        errs["wgrad"] = max(errs["wgrad"], rel_err(out.cpu(), gw_ref))
        assert rel_err(out.cpu(), gw_ref) < 1e-5, blocks
    return errs


def wgrad_one_workgroup_per_kernel_row(ops, L, dev, cin, cout, B, H, affine, W=None):
    W = H if W is None else W
    spec = ops.ConvSpec("conv", cin, cout, 3, 1, 1)
    x = rnd(B, cin, H, W, seed=2)
    s_, t_ = rnd(cin, seed=5) + 0.3, rnd(cin, seed=6) * 0.5
    a = TF.relu(x * s_.view(1, -1, 1, 1) + t_.view(1, -1, 1, 1)) if affine else x
    wd = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    y_ref = TF.conv2d(a.double(), wd, None, 1, 1)
    gy = rnd(*y_ref.shape, seed=4)
    (gw_ref,) = torch.autograd.grad(y_ref, [wd], gy.double())
    xg, gyg = ops.nhwc(x).to(dev), ops.nhwc(gy).to(dev)
    aff = (s_.to(dev), t_.to(dev), True) if affine else None
    bg = torch.empty(cout, device=dev)
    gw = ops.conv_wgrad(spec, xg, gyg, x_affine=aff, bias_grad=bg, algo=3)
    errs = dict(wgrad=rel_err(gw.cpu(), gw_ref), bgrad=rel_err(bg.cpu(), gy.double().sum((0, 2, 3))))
    assert errs["wgrad"] < 1e-5
    assert errs["bgrad"] < 1e-5
    old = ops.conv_wgrad(spec, xg, gyg, x_affine=aff, algo=1)
    errs["vs_algo1"] = rel_err(gw.cpu(), old.cpu())
    assert errs["vs_algo1"] < 2e-6
    prob = spec.wgrad_problem(H, W)
    for blocks in (1, 7, 100000):
        R = torch.zeros(prob["Cd"], 9, prob["Cg"], device=dev)
        wa = ops.make_wgrad_args(prob, B, gyg, xg, R, prob["Cg"], algo=3, **({"g_affine": aff} if aff else {}))
        wa.target_blocks = blocks
        L.call("awr_conv_wgrad", C.byref(wa), L.stream())
        out = torch.empty(cout, cin, 3, 3, device=dev)
        L.call("awr_unpack_wgrad", L.ptr(R), prob["d0"], prob["d1"], 9, prob["Cg"], L.ptr(out), 0, L.stream())
        errs["wgrad"] = max(errs["wgrad"], rel_err(out.cpu(), gw_ref))
        assert rel_err(out.cpu(), gw_ref) < 1e-5, blocks
    # geometries the kernel does not serve are refused, not mis-computed
    bad = ops.ConvSpec("conv", cin, cout, 3, 2, 1)
    pb = bad.wgrad_problem(H, W)
    Rb = torch.zeros(pb["Cd"], 9, pb["Cg"], device=dev)
    wb = ops.make_wgrad_args(pb, B, ops.nhwc(rnd(B, cout, pb["Hd"], pb["Wd"], seed=7)).to(dev), xg, Rb, pb["Cg"], algo=3)
    with pytest.raises(Exception):
        L.call("awr_conv_wgrad", C.byref(wb), L.stream())
    return errs


# ---- fused conv pair --------------------------------------------------------------------------------------------------------------------------
def fused_conv_pair(ops, L, dev, B, H, cin, k, n1, cx, tm, W=None):
    W = H if W is None else W
    n2 = 2 * n1
    s1 = ops.ConvSpec("conv", cin, n1, k, 1, k // 2)
    s2 = ops.ConvSpec("conv", n1 + cx, n2, 1, 1, 0)
    x = rnd(B, cin, H, W, seed=1)
    w1, b1 = rnd(n1, cin, k, k, seed=2, scale=0.05), rnd(n1, seed=3)
    w2, b2 = rnd(n2, n1 + cx, 1, 1, seed=4, scale=0.1), rnd(n2, seed=5)
    isc, ish = rnd(cin, seed=6) + 1.5, rnd(cin, seed=7)
    sc, sh = rnd(n1, seed=8) + 1.5, rnd(n1, seed=9)
    res = rnd(B, n2, H, W, seed=10) if not cx else None
    x2 = rnd(B, cx, H, W, seed=11) if cx else None
    a0 = TF.relu(x.double() * isc.double().view(1, -1, 1, 1) + ish.double().view(1, -1, 1, 1))
    mid = TF.relu((TF.conv2d(a0, w1.double(), b1.double(), 1, k // 2)) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
    ref = TF.conv2d(torch.cat([mid, x2.double()], 1) if cx else mid, w2.double(), b2.double()) + (res.double() if res is not None else 0.0)
    wp1, wp2 = ops.pack_weight(w1.to(dev), s1.fwd_pack()), ops.pack_weight(w2.to(dev), s2.fwd_pack())
    xg = ops.nhwc(x).to(dev)
    rg = ops.nhwc(res).to(dev) if res is not None else None
    x2g = ops.nhwc(x2).to(dev) if cx else None
    d = lambda t: t.to(dev)
    iscg, ishg, scg, shg, b1g, b2g = d(isc), d(ish), d(sc), d(sh), d(b1), d(b2)
    # two launches
    m2 = ops.conv_forward(s1, xg, wp1, in_scale=iscg, in_shift=ishg, relu_in=True, bias=b1g, out_scale=scg, out_shift=shg, relu_out=True)
    y2 = ops.conv_forward(s2, torch.cat([m2, x2g], 3).contiguous() if cx else m2, wp2, bias=b2g, res=rg)
    # one launch
    prob = s1.fwd_problem(H, W)
    y1 = torch.full((B, H, W, n2), float("nan"), device=dev)
    a = ops.make_conv_args(prob, B, xg, wp1, y1, in_scale=iscg, in_shift=ishg, relu_in=True, bias=b1g, out_scale=scg, out_shift=shg, relu_out=True, res=rg, T=s1.T)
    a.w2, a.bias2, a.N1, a.N, a.tile_m, a.tile_n = L.ptr(wp2), L.ptr(b2g), n1, n2, tm, (2 if n1 == 128 else 1)
    if cx:
        a.in2, a.N1x = L.ptr(x2g), cx
    L.call("awr_conv_gemm", C.byref(a), L.stream())
    torch.cuda.synchronize()
    errs = dict(one_launch=rel_err(ops.nchw(y1).cpu(), ref), two_launches=rel_err(ops.nchw(y2).cpu(), ref), one_vs_two=rel_err(y1.cpu(), y2.cpu()))
    assert errs["one_launch"] < 3e-6 and errs["two_launches"] < 3e-6
    assert errs["one_vs_two"] < 2e-6
    # refusals: other channel counts have no fused form
    a.N1 = 32
    with pytest.raises(Exception):
        L.call("awr_conv_gemm", C.byref(a), L.stream())
    a.N1, a.N = n1, n1
    with pytest.raises(Exception):
        L.call("awr_conv_gemm", C.byref(a), L.stream())
    return errs


# ---- short-K operand prefetch -----------------------------------------------------------------------------------------------------------------
def short_k_epilogue_operand_prefetch(ops, L, dev, tm, tn, cin, cout, B, H, W=None):
    W = H if W is None else W
    spec = ops.ConvSpec("conv", cin, cout, 1, 1, 0)
    x, w, bias = rnd(B, cin, H, W, seed=1), rnd(cout, cin, 1, 1, seed=2, scale=0.1), rnd(cout, seed=3)
    res = rnd(B, cout, H, W, seed=4)
    pre = TF.conv2d(x.double(), w.double(), bias.double()) + res.double()
    wp = ops.pack_weight(w.to(dev), spec.fwd_pack())
    stats = torch.zeros(16, 2, cout, device=dev, dtype=torch.float64)
    prob = spec.fwd_problem(H, W)
    out = torch.full((B, H, W, prob["N"]), float("nan"), device=dev)
    a = ops.make_conv_args(prob, B, ops.nhwc(x).to(dev), wp, out, bias=bias.to(dev), res=ops.nhwc(res).to(dev), stats=stats, T=spec.T)
    a.tile_m, a.tile_n = tm, tn
    L.call("awr_conv_gemm", C.byref(a), L.stream())
    errs = dict(fwd=rel_err(ops.nchw(out)[:, :cout].cpu(), pre))
    assert errs["fwd"] < 2e-6
    assert rel_err(stats.sum(0)[0][:cout].cpu(), pre.sum((0, 2, 3))) < 1e-5 and rel_err(stats.sum(0)[1][:cout].cpu(), (pre * pre).sum((0, 2, 3))) < 1e-5
    # data gradient (cout -> cin channels) masked by relu(bn(y)) and reduced for the BatchNorm backward in the same launch
    gy = rnd(B, cout, H, W, seed=5)
    y = rnd(B, cin, H, W, seed=6)
    coef4 = torch.stack([rnd(cin, seed=7) + 1.2, rnd(cin, seed=8) * 0.3, rnd(cin, seed=9) * 0.2, rnd(cin, seed=10) + 1.5])      # scale, shift, mean, invstd
    v = TF.conv_transpose2d(gy.double(), w.double())
    mask = (y.double() * coef4[0].double().view(1, -1, 1, 1) + coef4[1].double().view(1, -1, 1, 1)) > 0
    g_ref = v * mask
    xhat = (y.double() - coef4[2].double().view(1, -1, 1, 1)) * coef4[3].double().view(1, -1, 1, 1)
    wd = ops.pack_weight(w.to(dev), spec.dgrad_pack())
    dprob = spec.dgrad_problem(H, W)
    g = torch.full((B, H, W, dprob["N"]), float("nan"), device=dev)
    sums = torch.zeros(16, 2, dprob["N"], device=dev, dtype=torch.float64)
    yg = torch.zeros(B, H, W, dprob["N"], device=dev)
    yg[..., :cin] = ops.nhwc(y).to(dev)
    c4 = torch.zeros(4, dprob["N"], device=dev)
    c4[:, :cin] = coef4.to(dev)
    d = ops.make_conv_args(dprob, B, ops.nhwc(gy).to(dev) if cout == dprob["Cin"] else torch.nn.functional.pad(ops.nhwc(gy), (0, dprob["Cin"] - cout)).to(dev),
                           wd, g, stats=sums, T=spec.T)
    d.bnr_y, d.bnr_coef, d.tile_m, d.tile_n = L.ptr(yg), L.ptr(c4), tm, tn
    L.call("awr_conv_gemm", C.byref(d), L.stream())
    torch.cuda.synchronize()
    errs["dgrad"] = rel_err(ops.nchw(g)[:, :cin].cpu(), g_ref)
    assert errs["dgrad"] < 3e-6
    assert rel_err(sums.sum(0)[0][:cin].cpu(), g_ref.sum((0, 2, 3))) < 1e-5 and rel_err(sums.sum(0)[1][:cin].cpu(), (g_ref * xhat).sum((0, 2, 3))) < 2e-5
    return errs


# ---- statistics from the accumulators ---------------------------------------------------------------------------------------------------------
def statistics_from_the_accumulators(ops, L, dev, tile, B=2, H=16, W=None, cin=64, cout=96):
    W = H if W is None else W
    spec = ops.ConvSpec("conv", cin, cout, 3, 1, 1)
    x, w = rnd(B, cin, H, W, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.05)
    bias = (rnd(cout, seed=3) + 100.0).to(dev)
    prob = spec.fwd_problem(H, W)
    xin = ops.nhwc(x).to(dev).contiguous()
    wp = ops.pack_weight(w.to(dev), spec.fwd_pack())
    got = {}
    L.call("awr_debug_force_tile", *tile)
    try:
        for fast in ("0", "1"):
            L.call("awr_debug_set_knob", b"fast_stats", int(fast))
            out = torch.full((B, H, W, prob["N"]), float("nan"), device=dev)
            st = torch.zeros(16, 2, prob["N"], device=dev, dtype=torch.float64)
            a = ops.make_conv_args(prob, B, xin, wp, out, bias=bias, stats=st, T=spec.T)
            L.call("awr_conv_gemm", C.byref(a), L.stream())
            torch.cuda.synchronize()
            got[fast] = (out.clone(), st.sum(0).clone())
    finally:
        L.call("awr_debug_set_knob", b"fast_stats", 1)
        L.call("awr_debug_force_tile", 0, 0)
    assert torch.equal(got["0"][0], got["1"][0])
    ref = got["1"][0].double().reshape(-1, prob["N"])
    n = ref.shape[0]
    errs = {}
    for k in ("0", "1"):
        s1, s2 = got[k][1][0], got[k][1][1]
        assert float((s1 - ref.sum(0)).abs().max()) < 1e-7 * float(ref.abs().sum(0).max())
        var, var_ref = s2 / n - (s1 / n) ** 2, ref.var(0, unbiased=False)
        errs["var_fast" if k == "1" else "var_rows"] = float(((var - var_ref).abs() / var_ref).max())
        assert float(((var - var_ref).abs() / var_ref).max()) < 1e-4      # mean ~ 100, std ~ 1: the shifted sums keep five digits of the variance
    # the values themselves, against float64 (the square test never needed it: its geometry cannot be transposed)
    ref64 = TF.conv2d(x.double(), w.double(), bias.cpu().double(), 1, 1)
    errs["fwd"] = rel_err(ops.nchw(got["1"][0]).cpu(), ref64)
    return errs
