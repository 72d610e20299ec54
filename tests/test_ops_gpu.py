"""GPU parity of the backbone building blocks (implicit-GEMM conv family, BatchNorm pieces, pooling,
layout bridges) through the C ABI, against float64 torch-CPU evaluations of the same operators."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import conv_cases as CC
from conv_cases import DP, rel_err, rnd
from conv_cases import torch_fwd as _torch_fwd  # noqa: F401  (tests/test_train_split_k_gpu.py takes it from here)

pytestmark = pytest.mark.gpu


def _has_study():
    import awr_amd  # noqa: F401
    from awr_amd import _lib
    return _lib.HAS_STUDY


# measured-and-rejected forms of earlier rounds live in study builds only (AWR_BUILD_STUDY=1 python -m awr_amd.build --force): their tests run there
study_only = pytest.mark.skipif(not _has_study(), reason="study form: needs libawr_hip.so built with -DAWR_STUDY")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    import awr_amd  # noqa: F401
    from awr_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    import awr_amd  # noqa: F401
    from awr_amd import _lib
    return _lib


# kind, cin, cout, k, stride, pad, B, H
CONV_CASES = [
    ("conv", 64, 64, 3, 1, 1, 2, 32),
    ("conv", 64, 128, 3, 2, 1, 3, 20),      # ragged M (not a tile multiple)
    ("conv", 128, 256, 3, 2, 1, 2, 16),
    ("conv", 512, 512, 3, 1, 1, 2, 8),      # K = 4608
    ("conv", 64, 128, 1, 2, 0, 2, 16),      # downsample 1x1 s2
    ("conv", 256, 64, 1, 1, 0, 2, 16),
    ("conv", 128, 128, 3, 1, 1, 5, 4),      # tiny spatial (hourglass bottom)
    ("deconv", 128, 64, 4, 2, 1, 2, 8),
    ("deconv", 512, 256, 4, 2, 1, 1, 8),
]


@pytest.mark.parametrize("kind,cin,cout,k,stride,pad,B,H", CONV_CASES)
def test_conv_forward_dgrad_wgrad(ops, dev, kind, cin, cout, k, stride, pad, B, H):
    CC.conv_forward_dgrad_wgrad(ops, dev, kind, cin, cout, k, stride, pad, B, H)


@pytest.mark.parametrize("products,staging", [(1, 2), (1, 0), (6, 2)])
@pytest.mark.parametrize("tm,tn", [(1, 1), (1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("kind,cin,cout,k,stride,pad,B,H", [("conv", 64, 96, 3, 1, 1, 3, 18), ("conv", 128, 160, 3, 2, 1, 2, 20),
                                                              ("deconv", 64, 96, 4, 2, 1, 3, 10), ("conv", 32, 64, 1, 1, 0, 2, 12)])
def test_conv_every_tile_shape(ops, L, dev, products, staging, tm, tn, kind, cin, cout, k, stride, pad, B, H):
    """All four workgroup tiles (64/128 x 64/128) in both product modes (f32 MFMA, 6-product bf16 split) and, for the f32 mode, both
    operand staging paths (2 = LDS-DMA, the default; 0 = through registers) on ragged M and N (not multiples of any tile), incl. a
    single-K-slice problem."""
    CC.conv_every_tile_shape(ops, L, dev, products, staging, tm, tn, kind, cin, cout, k, stride, pad, B, H)


@study_only
def test_split_act_image_is_the_exact_three_way_cut(ops, L, dev):
    """awr_split_act: every element of [relu](x * scale + shift) as three bf16 pieces whose sum is the fp32 value EXACTLY, in the layout of the
    weights' split image (element idx -> shorts (idx / 32) * 96 + idx % 32 + {0, 32, 64})."""
    x = rnd(3, 5, 7, 96, seed=5).to(dev) * 3.0
    sc, sh = (rnd(96, seed=6) + 1.5).to(dev), rnd(96, seed=7).to(dev)
    for affine, relu in ((False, False), (True, True), (True, False)):
        img = ops.split_act(x, sc if affine else None, sh if affine else None, relu)
        ref = x * sc + sh if affine else x
        if relu:
            ref = torch.relu(ref)
        pl = img.view(-1, 3, 32)                                             # [slice][plane][32]
        pieces = (pl.to(torch.int32) << 16).view(torch.float32)              # bf16 bits -> fp32
        h, m, l = pieces[:, 0].reshape(-1), pieces[:, 1].reshape(-1), pieces[:, 2].reshape(-1)
        tot = (h.double() + m.double() + l.double()).float()                 # (three 8-bit pieces: the double sum is exact)
        assert torch.equal(tot.double(), h.double() + m.double() + l.double())
        if affine:      # the kernel's multiply-add is fused (one rounding): compared with the float64 expression, within one ulp of the larger term
            r64 = x.double() * sc.double() + sh.double()
            r64 = torch.relu(r64) if relu else r64
            bound = ((x.double() * sc.double()).abs() + sh.double().abs()).reshape(-1) * 2.0 ** -23
            assert bool(((tot.double() - r64.reshape(-1)).abs() <= bound).all()), (affine, relu)
        else:
            assert torch.equal(tot, ref.reshape(-1)), (affine, relu)
        assert torch.equal(h, (tot.view(torch.int32) & -65536).view(torch.float32))     # h = the top 16 bits of the value (truncation)
        r1 = tot - h
        assert torch.equal(m, (r1.view(torch.int32) & -65536).view(torch.float32)) and torch.equal(l, r1 - m)


@pytest.mark.parametrize("tm,tn", [(1, 1), (1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("kind,cin,cout,k,stride,pad,B,H", [("conv", 64, 96, 3, 1, 1, 3, 18), ("conv", 128, 160, 3, 2, 1, 2, 20),
                                                              ("deconv", 64, 96, 4, 2, 1, 3, 10), ("conv", 96, 64, 1, 1, 0, 2, 12)])
@study_only
def test_split_mode_with_precut_activations_is_bit_identical(ops, L, dev, tm, tn, kind, cin, cout, k, stride, pad, B, H):
    """Split-operand mode, both operands by LDS-DMA (awr_conv_args.in_split: the activation image cut ONCE by awr_split_act) against the
    kernel that cuts every staged row itself: same pieces, same six products per 16 k, same order -> the SAME BITS, on ragged M / N, padding
    taps (out-of-range DMA sources land zero pieces), strided and transposed phases; with bias / residual / ReLU / statistics epilogues.
    And a BatchNorm + ReLU input: cut after the affine by the producer vs applied by the consumer's loader."""
    CC.split_mode_with_precut_activations(ops, L, dev, tm, tn, kind, cin, cout, k, stride, pad, B, H)


@pytest.mark.parametrize("tm,tn", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_lds_dma_staging_is_bit_identical_to_register_staging(ops, L, dev, tm, tn):
    """The LDS-DMA kernel (buffer_load ... lds into swizzled unpadded rows, 16-float stages) walks K in the same order as the register-staged
    one, so every fused form must give the SAME BITS: 3x3 with the fused input affine + ReLU (activation rows through registers, weights by
    DMA) + bias / affine / residual / ReLU / statistics epilogue; a strided 3x3 and a transposed conv (padding taps = out-of-range DMA
    sources that must land zeros); the two-tensor K extent of conv3 + skip_layer (hourglass.py:44-59); the short-K operand-prefetch form;
    a data gradient with the fused BatchNorm-backward reduction, plain and accumulating onto an earlier contribution with the mask from a
    stored activation."""
    CC.lds_dma_staging_vs_register_staging(ops, L, dev, tm, tn)


@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("tm,tn", [(1, 1), (1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("kind,cin,cout,k,stride,pad,B,H", [("conv", 64, 96, 3, 1, 1, 3, 18), ("conv", 128, 160, 3, 2, 1, 2, 20),
                                                              ("deconv", 64, 96, 4, 2, 1, 3, 10), ("conv", 96, 64, 1, 1, 0, 2, 12)])
def test_dgrad_with_unmaterialised_batchnorm_backward(ops, L, dev, accum, tm, tn, kind, cin, cout, k, stride, pad, B, H):
    """awr_conv_args.in_bnb_y / in_bnb_coef: the data gradient of a conv whose output y feeds a BatchNorm takes g = d(loss)/d(bn(y)) and y
    and forms d(y) = a1 g + a2 (y - mean) + a3 per channel on the operand's way to the matrix pipe (padding taps stay zero), instead of
    reading a d(y) that a separate pass wrote.  Against float64 (conv_transpose / conv of the float64 d(y)), and against the same GEMM fed
    with d(y) materialised by awr_bn_bwd_apply_only from the coefficients awr_bn_bwd_finalize_lin derives from reduction sums.
    accum = 1: the blocked-accumulation instantiation of the same launches."""
    CC.dgrad_with_unmaterialised_batchnorm_backward(ops, L, dev, accum, tm, tn, kind, cin, cout, k, stride, pad, B, H)


def test_conv_fused_prologue_epilogue_stats(ops, dev):
    """conv( relu(x*s+t) ) * so + to + res -> relu, with per-channel statistics of the pre-ReLU value."""
    CC.conv_fused_prologue_epilogue_stats(ops, dev, B=2, H=16, cin=64, cout=96)           # N = 96: not a multiple of the 64/128 tile


def test_stem_im2col_gemm(ops, L, dev):
    """5x5 stem (Cin=1) as im2col + the same MFMA GEMM; forward and weight gradient."""
    CC.stem_im2col_gemm(ops, L, dev, B=2, H=32)


def test_batch_statistics_of_nearly_constant_channels(ops, L, dev):
    """sum x / sum x^2 of channels whose spread is tiny next to their mean (dead or saturated channels, a constant image
    background): a plain one-pass fp32 accumulation loses the variance (|mean| = 5, std = 1e-3: x^2 carries the spread in its last
    two bits).  All three producers -- GEMM epilogue, stand-alone channel statistics, fused stem -- accumulate shifted sums and must
    give the float64 variance to 1e-4 relative."""
    B, H, cin, cout = 2, 16, 64, 64
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, cin, H, H, generator=g)
    w = torch.randn(cout, cin, 1, 1, generator=g) * cin ** -0.5
    w[:16] *= 1e-3                                     # channels 0..15: conv output = bias + 1e-3 * noise
    bias = torch.randn(cout, generator=g)
    bias[:16] = torch.linspace(-8, 8, 16)
    spec = ops.ConvSpec("conv", cin, cout, 1, 1, 0)
    wp = ops.pack_weight(w.to(dev), spec.fwd_pack())
    stats = torch.zeros(16, 2, cout, device=dev, dtype=torch.float64)
    y = ops.conv_forward(spec, ops.nhwc(x).to(dev), wp, bias=bias.to(dev), stats=stats)
    n = B * H * H

    def var_of(st):
        st = st.sum(0).cpu()
        return st[0] / n, st[1] / n - (st[0] / n) ** 2

    yd = ops.nchw(y).cpu().double()                    # statistics of the values the kernel stored (fp32), evaluated in float64
    mean_ref, var_ref = yd.mean((0, 2, 3)), yd.var((0, 2, 3), unbiased=False)
    assert float(var_ref[:16].max()) < 1e-5 and float(var_ref[16:].min()) > 0.1
    mean, var = var_of(stats)
    assert float(((mean - mean_ref).abs() / (mean_ref.abs() + 1e-3)).max()) < 1e-6
    assert float(((var - var_ref).abs() / var_ref).max()) < 1e-4, ((var - var_ref).abs() / var_ref)[:16]
    stats2 = torch.zeros(16, 2, cout, device=dev, dtype=torch.float64)
    L.call("awr_channel_stats", L.ptr(y), n, cout, L.ptr(stats2), 0, L.stream())
    mean2, var2 = var_of(stats2)
    assert float(((var2 - var_ref).abs() / var_ref).max()) < 1e-4
    # fused stem: a constant image -> every interior conv pixel of a channel has the same value (bias + sum of taps)
    Hs = 64
    img = torch.full((B, 1, Hs, Hs), 1.0)
    img[:, :, 20:30, 20:30] += torch.randn(B, 1, 10, 10, generator=g) * 1e-3
    ws = torch.randn(64, 1, 5, 5, generator=g) * 0.2
    bs = torch.randn(64, generator=g) * 3
    ys = TF.conv2d(img.double(), ws.double(), bs.double(), 1, 2)
    stats3 = torch.zeros(16, 2, 64, device=dev, dtype=torch.float64)
    imgd, wsd, bsd = img.to(dev), ws.to(dev).contiguous(), bs.to(dev)      # (named: the launch is asynchronous, temporaries would be recycled)
    L.call("awr_stem_stats", L.ptr(imgd), L.ptr(wsd), L.ptr(bsd), B, Hs, Hs, L.ptr(stats3), 0, L.stream())
    st = stats3.sum(0).cpu()
    ns = B * Hs * Hs
    var3 = st[1] / ns - (st[0] / ns) ** 2
    assert float(((var3 - ys.var((0, 2, 3), unbiased=False)).abs() / ys.var((0, 2, 3), unbiased=False)).max()) < 1e-4


@pytest.mark.parametrize("B,H,C", [(2, 16, 64), (3, 10, 96), (2, 8, 512), (4, 32, 128), (2, 4, 2048)])      # 2048: the Bottleneck ResNets' layer4 (channel chunks)
def test_batchnorm_train_forward_backward(L, dev, B, H, C):
    x = rnd(B, C, H, H, seed=1) * 2 + 0.3
    gamma, beta = rnd(C, seed=2) + 1.5, rnd(C, seed=3)
    res = rnd(B, C, H, H, seed=4)
    rm, rv = rnd(C, seed=5), rnd(C, seed=6) + 1.5
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm_ref, rv_ref = rm.double().clone(), rv.double().clone()
    y_ref = TF.relu(TF.batch_norm(xd, rm_ref, rv_ref, gd, bd, True, 0.1, 1e-5) + res.double())
    gout = rnd(B, C, H, H, seed=7)
    gx_ref, gg_ref, gb_ref = torch.autograd.grad(y_ref, [xd, gd, bd], gout.double())

    from awr_amd import ops
    npix = B * H * H
    xg = ops.nhwc(x).to(dev)
    stats = torch.zeros(16, 2, C, device=dev, dtype=torch.float64)
    L.call("awr_channel_stats", L.ptr(xg), npix, C, L.ptr(stats), 0, L.stream())
    scale, shift, mean, invstd = (torch.empty(C, device=dev) for _ in range(4))
    rmg, rvg = rm.to(dev), rv.to(dev)
    L.call("awr_bn_finalize", L.ptr(stats), C, npix, DP(L, gamma, dev), DP(L, beta, dev), L.ptr(rmg), L.ptr(rvg), 0.1, 1e-5,
           L.ptr(scale), L.ptr(shift), L.ptr(mean), L.ptr(invstd), 0, L.stream())
    assert float(stats.abs().max()) == 0.0          # finalize re-arms the accumulator
    out = torch.empty_like(xg)
    resg = ops.nhwc(res).to(dev)
    L.call("awr_bn_apply", L.ptr(xg), L.ptr(scale), L.ptr(shift), L.ptr(resg), 1, L.ptr(out), npix, C, L.stream())
    assert rel_err(ops.nchw(out).cpu(), y_ref.detach()) < 3e-6
    assert rel_err(rmg.cpu(), rm_ref) < 1e-6 and rel_err(rvg.cpu(), rv_ref) < 1e-6
    # backward
    sums = torch.zeros(16, 2, C, device=dev, dtype=torch.float64)
    coef = torch.empty(3, C, device=dev)
    goutg = ops.nhwc(gout).to(dev)
    L.call("awr_bn_bwd_reduce", L.ptr(goutg), L.ptr(out), L.ptr(xg), L.ptr(mean), L.ptr(invstd), None, None, npix, C, L.ptr(sums), 0, L.stream())
    dy, g = torch.empty_like(xg), torch.empty_like(xg)
    dgam, dbet = torch.empty(C, device=dev), torch.empty(C, device=dev)
    L.call("awr_bn_bwd_apply", L.ptr(goutg), L.ptr(out), L.ptr(xg), L.ptr(mean), L.ptr(invstd), DP(L, gamma, dev), None, None, L.ptr(sums), L.ptr(coef), npix, C,
           L.ptr(dy), None, L.ptr(g), L.ptr(dgam), L.ptr(dbet), 0, 0, L.stream())
    assert rel_err(ops.nchw(dy).cpu(), gx_ref) < 2e-5
    assert rel_err(dgam.cpu(), gg_ref) < 2e-5 and rel_err(dbet.cpu(), gb_ref) < 2e-5
    assert rel_err(ops.nchw(g).cpu(), gout.double() * (y_ref.detach() > 0)) < 1e-6
    assert float(sums.abs().max()) == 0.0
    # no-residual variant: the ReLU mask is re-derived from y with the forward scale/shift instead of reading the activation
    out2 = torch.empty_like(xg)
    L.call("awr_bn_apply", L.ptr(xg), L.ptr(scale), L.ptr(shift), None, 1, L.ptr(out2), npix, C, L.stream())
    sa, sb = torch.zeros(16, 2, C, device=dev, dtype=torch.float64), torch.zeros(16, 2, C, device=dev, dtype=torch.float64)
    L.call("awr_bn_bwd_reduce", L.ptr(goutg), L.ptr(out2), L.ptr(xg), L.ptr(mean), L.ptr(invstd), None, None, npix, C, L.ptr(sa), 0, L.stream())
    L.call("awr_bn_bwd_reduce", L.ptr(goutg), None, L.ptr(xg), L.ptr(mean), L.ptr(invstd), L.ptr(scale), L.ptr(shift), npix, C, L.ptr(sb), 0, L.stream())
    assert rel_err(sb.sum(0).cpu(), sa.sum(0).cpu()) < 1e-9
    dya, dyb = torch.empty_like(xg), torch.empty_like(xg)
    gam = DP(L, gamma, dev)
    L.call("awr_bn_bwd_apply", L.ptr(goutg), L.ptr(out2), L.ptr(xg), L.ptr(mean), L.ptr(invstd), gam, None, None, L.ptr(sa), L.ptr(coef), npix, C,
           L.ptr(dya), None, None, L.ptr(dgam), L.ptr(dbet), 0, 0, L.stream())
    L.call("awr_bn_bwd_apply", L.ptr(goutg), None, L.ptr(xg), L.ptr(mean), L.ptr(invstd), gam, L.ptr(scale), L.ptr(shift), L.ptr(sb), L.ptr(coef), npix, C,
           L.ptr(dyb), None, None, L.ptr(dgam), L.ptr(dbet), 0, 0, L.stream())
    assert torch.equal(dya, dyb)


def test_bn_fold_eval(L, dev):
    C = 64
    g, b, m, v = rnd(C, seed=1) + 1.5, rnd(C, seed=2), rnd(C, seed=3), rnd(C, seed=4) + 1.5
    sc, sh = torch.empty(C, device=dev), torch.empty(C, device=dev)
    L.call("awr_bn_fold_eval", C, DP(L, g, dev), DP(L, b, dev), DP(L, m, dev), DP(L, v, dev), 1e-5, L.ptr(sc), L.ptr(sh), L.stream())
    x = rnd(2, C, 4, 4, seed=5)
    ref = TF.batch_norm(x.double(), m.double(), v.double(), g.double(), b.double(), False, 0.1, 1e-5)
    got = x.to(dev) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    assert rel_err(got.cpu(), ref) < 2e-6


@pytest.mark.parametrize("k,s,p,B,H,C", [(3, 2, 1, 2, 16, 64), (2, 2, 0, 3, 8, 128), (3, 2, 1, 1, 128, 64)])
def test_maxpool(L, dev, k, s, p, B, H, C):
    from awr_amd import ops
    x = rnd(B, C, H, H, seed=1)
    x[:, :, ::3, ::3] = 0.0
    x = TF.relu(x)            # many exact ties at 0, like the post-ReLU stem output
    xd = x.double().requires_grad_(True)
    ref = TF.max_pool2d(xd, k, s, p)
    gout = rnd(*ref.shape, seed=2)
    (gx_ref,) = torch.autograd.grad(ref, xd, gout.double())
    Ho = ref.shape[-1]
    xg = ops.nhwc(x).to(dev)
    out = torch.empty(B, Ho, Ho, C, device=dev)
    arg = torch.empty(B, Ho, Ho, C, device=dev, dtype=torch.uint8)
    L.call("awr_maxpool_fwd", L.ptr(xg), None, None, 0, B, H, H, C, k, s, p, L.ptr(out), L.ptr(arg), L.stream())
    assert rel_err(ops.nchw(out).cpu(), ref.detach()) == 0.0
    dx = torch.empty_like(xg)
    L.call("awr_maxpool_bwd", DP(L, ops.nhwc(gout), dev), L.ptr(arg), B, H, H, C, k, s, p, L.ptr(dx), 0, L.stream())
    got = ops.nchw(dx).cpu().double()
    # ties: ATen and this kernel both route to the first maximum in scan order
    assert rel_err(got, gx_ref) < 1e-6
    L.call("awr_maxpool_bwd", DP(L, ops.nhwc(gout), dev), L.ptr(arg), B, H, H, C, k, s, p, L.ptr(dx), 1, L.stream())
    assert rel_err(ops.nchw(dx).cpu(), 2 * gx_ref) < 1e-6


def test_fused_affine_loaders(ops, L, dev):
    """Un-materialised BatchNorm+ReLU inputs: wgrad (conv: gathered operand, deconv: dense operand) and max-pool
    apply relu(x*s+t) while loading and must equal the same op on the materialised tensor."""
    B, H, cin, cout = 2, 16, 64, 96
    x = rnd(B, cin, H, H, seed=1)
    s_, t_ = rnd(cin, seed=2) + 0.2, rnd(cin, seed=3) * 0.5          # some negative scales too
    a = TF.relu(x * s_.view(1, -1, 1, 1) + t_.view(1, -1, 1, 1))
    xg, ag, sg, tg = ops.nhwc(x).to(dev), ops.nhwc(a).to(dev), s_.to(dev), t_.to(dev)
    for kind, k, st, p in (("conv", 3, 1, 1), ("conv", 3, 2, 1), ("deconv", 4, 2, 1)):
        spec = ops.ConvSpec(kind, cin, cout, k, st, p)
        ho = spec.out_hw(H, H)[0]
        gy = ops.nhwc(rnd(B, cout, ho, ho, seed=4)).to(dev)
        ref = ops.conv_wgrad(spec, ag, gy)
        got = ops.conv_wgrad(spec, xg, gy, x_affine=(sg, tg, True))
        assert rel_err(got.cpu(), ref.cpu()) < 2e-5, kind
    out_a, out_x = torch.empty(B, 8, 8, cin, device=dev), torch.empty(B, 8, 8, cin, device=dev)
    arg_a, arg_x = torch.empty(B, 8, 8, cin, device=dev, dtype=torch.uint8), torch.empty(B, 8, 8, cin, device=dev, dtype=torch.uint8)
    L.call("awr_maxpool_fwd", L.ptr(ag), None, None, 0, B, H, H, cin, 3, 2, 1, L.ptr(out_a), L.ptr(arg_a), L.stream())
    L.call("awr_maxpool_fwd", L.ptr(xg), L.ptr(sg), L.ptr(tg), 1, B, H, H, cin, 3, 2, 1, L.ptr(out_x), L.ptr(arg_x), L.stream())
    assert rel_err(out_x.cpu(), out_a.cpu()) < 1e-6 and float((arg_a != arg_x).float().mean()) < 1e-3


def test_upsample_add_and_misc(L, dev):
    from awr_amd import ops
    B, Hl, C = 2, 8, 64
    up1, low = rnd(B, C, 2 * Hl, 2 * Hl, seed=1), rnd(B, C, Hl, Hl, seed=2)
    ref = up1 + TF.interpolate(low, scale_factor=2, mode="nearest")
    out = torch.empty(B, 2 * Hl, 2 * Hl, C, device=dev)
    L.call("awr_upsample2_add", DP(L, ops.nhwc(up1), dev), DP(L, ops.nhwc(low), dev), B, Hl, Hl, C, L.ptr(out), L.stream())
    assert rel_err(ops.nchw(out).cpu(), ref) < 1e-7
    gout = rnd(B, C, 2 * Hl, 2 * Hl, seed=3)
    dlow = torch.empty(B, Hl, Hl, C, device=dev)
    L.call("awr_upsample2_bwd", DP(L, ops.nhwc(gout), dev), B, Hl, Hl, C, L.ptr(dlow), 0, L.stream())
    ref_d = gout.view(B, C, Hl, 2, Hl, 2).sum((3, 5))
    assert rel_err(ops.nchw(dlow).cpu(), ref_d) < 1e-6
    # relu_bwd / add / bias_grad
    a, d = rnd(B, Hl, Hl, C, seed=4), rnd(B, Hl, Hl, C, seed=5)
    g = torch.empty(B, Hl, Hl, C, device=dev)
    L.call("awr_relu_bwd", DP(L, d, dev), DP(L, a, dev), L.ptr(g), a.numel(), L.stream())
    assert rel_err(g.cpu(), d * (a > 0)) == 0.0
    L.call("awr_add", DP(L, d, dev), DP(L, a, dev), L.ptr(g), a.numel(), L.stream())
    assert rel_err(g.cpu(), d + a) == 0.0
    db = torch.empty(C, device=dev)
    L.call("awr_bias_grad", DP(L, d, dev), B * Hl * Hl, C, L.ptr(db), 0, L.stream())
    assert rel_err(db.cpu(), d.double().sum((0, 1, 2))) < 1e-5


@pytest.mark.parametrize("B,P,C,Cp", [(2, 4096, 56, 64), (1, 16384, 84, 96), (3, 100, 56, 64)])
def test_layout_bridges(L, dev, B, P, C, Cp):
    x = rnd(B, P, Cp, seed=1)
    out = torch.empty(B, C, P, device=dev)
    L.call("awr_nhwc_to_nchw", DP(L, x, dev), B, P, Cp, C, L.ptr(out), L.stream())
    assert torch.equal(out.cpu(), x[:, :, :C].permute(0, 2, 1).contiguous())
    back = torch.full((B, P, Cp), 7.0, device=dev)
    L.call("awr_nchw_to_nhwc", L.ptr(out), B, P, Cp, C, L.ptr(back), L.stream())
    exp = x.clone()
    exp[:, :, C:] = 0.0
    assert torch.equal(back.cpu(), exp)


def test_pack_unpack_roundtrip(ops, L, dev):
    w = rnd(96, 64, 3, 3, seed=1)
    spec = ops.ConvSpec("conv", 64, 96, 3, 1, 1)
    wp = ops.pack_weight(w.to(dev), spec.fwd_pack())
    assert wp.shape == (128, 9, 64)
    assert torch.equal(wp[:96].cpu(), w.view(96, 64, 9).permute(0, 2, 1).contiguous())
    assert float(wp[96:].abs().max()) == 0.0
    g = torch.empty(96, 64, 3, 3, device=dev)
    L.call("awr_unpack_wgrad", L.ptr(wp), 96, 64, 9, 64, L.ptr(g), 0, L.stream())
    assert torch.equal(g.cpu(), w)
    wpt = ops.pack_weight(w.to(dev), spec.dgrad_pack())
    assert torch.equal(wpt[:64, :, :96].cpu(), w.view(96, 64, 9).permute(1, 2, 0).contiguous())


def test_batch_chunking_above_4gb(ops, dev):
    """Tensors >= 4 GiB (Hourglass 128-channel maps at 256x256, batch 128: BASELINE config 5) exceed the kernels' 32-bit
    buffer offsets; the entry points split the batch.  Property: the chunked call equals per-half calls bit for bit,
    for the forward GEMM (4 GiB input) and, to rounding, for the weight gradient (4 GiB gathered operand)."""
    B, H, cin, cout = 128, 256, 128, 64
    spec = ops.ConvSpec("conv", cin, cout, 1, 1, 0)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(B, H, H, cin, device=dev, generator=g) - 0.5
    assert x.numel() * 4 >= (1 << 32)
    w = (torch.rand(cout, cin, 1, 1, device=dev, generator=g) - 0.5) * 0.2
    wp = ops.pack_weight(w, spec.fwd_pack())
    y = ops.conv_forward(spec, x, wp)
    for lo, hi in ((0, 64), (64, 128)):
        assert torch.equal(y[lo:hi], ops.conv_forward(spec, x[lo:hi].contiguous(), wp))
    ref = torch.einsum("bhwc,oc->bhwo", x[100, 17:19].unsqueeze(0).double(), w.view(cout, cin).double())
    assert rel_err(y[100, 17:19].unsqueeze(0).cpu(), ref.cpu()) < 2e-6
    gw = ops.conv_wgrad(spec, x, y)
    gw2 = ops.conv_wgrad(spec, x[:64].contiguous(), y[:64].contiguous()) + ops.conv_wgrad(spec, x[64:].contiguous(), y[64:].contiguous())
    assert rel_err(gw.cpu(), gw2.cpu()) < 1e-4


def test_split_mode_accuracy_matches_fp32_mfma(ops, L, dev):
    """The 6-product split mode (awr_set_gemm_products(6)) against the FP32-MFMA mode, both measured against an fp64
    reference on a long contraction (K = 9*256 forward / dgrad, K = 2*24*24 pixels for the weight gradient) with wide
    dynamic range.  Dropping the m*l, l*m, l*l partial products costs <= 2^-23 per product -- below the rounding of the
    fp32 accumulation both modes share -- so the two errors must be of the same size."""
    spec = ops.ConvSpec("conv", 256, 256, 3, 1, 1)
    B, H = 2, 24
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 256, H, H, generator=g) * torch.exp(2.0 * torch.randn(B, 256, H, H, generator=g))     # heavy-tailed
    w = torch.randn(256, 256, 3, 3, generator=g) * (256 * 9) ** -0.5
    gy = torch.randn(B, 256, H, H, generator=g) * torch.exp(1.5 * torch.randn(B, 256, H, H, generator=g))
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y_ref = TF.conv2d(xd, wd, None, 1, 1)
    gx_ref, gw_ref = torch.autograd.grad(y_ref, [xd, wd], gy.double())
    errs = {}
    try:
        for n in (1, 6):
            L.call("awr_set_gemm_products", n)
            wg = w.to(dev)
            y = ops.conv_forward(spec, ops.nhwc(x).to(dev), ops.pack_weight(wg, spec.fwd_pack()))
            gx = ops.conv_dgrad(spec, ops.nhwc(gy).to(dev), ops.pack_weight(wg, spec.dgrad_pack()), H, H)
            gw = ops.conv_wgrad(spec, ops.nhwc(x).to(dev), ops.nhwc(gy).to(dev))
            errs[n] = (rel_err(ops.nchw(y).cpu(), y_ref.detach()), rel_err(ops.nchw(gx).cpu(), gx_ref), rel_err(gw.cpu(), gw_ref))
    finally:
        L.call("awr_set_gemm_products", 1)
    print("rel. error vs fp64 (fwd, dgrad, wgrad): f32 MFMA %s | 6-product split %s" % (errs[1], errs[6]))
    for e1, e6 in zip(errs[1], errs[6]):
        assert e6 <= 2.0 * e1 + 1e-7, (errs[1], errs[6])
        assert e6 < 5e-6


@pytest.mark.parametrize("B,H,W", [(2, 32, 48), (3, 128, 128), (1, 16, 16)])
def test_fused_stem_matches_conv_bn_relu_maxpool(L, dev, B, H, W):
    """csrc/awr_stem.hip: conv 5x5 (1 -> 64, pad 2, no bias) -> BatchNorm (batch statistics) -> ReLU -> MaxPool(3,2,1) without
    ever writing the full-resolution map, and its backward (BN parameter gradients, conv weight gradient) by recomputation --
    against float64 torch autograd of the four separate operators (resnet_deconv.py:31-36, :118-121)."""
    from awr_amd import ops
    g = torch.Generator().manual_seed(5 + H)
    img = (torch.rand(B, 1, H, W, generator=g) * 2 - 1)
    img[:, :, : H // 3] = 1.0                                    # constant background like the real crops
    w = torch.randn(64, 1, 5, 5, generator=g) * 0.2
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3
    # ---- float64 reference ----
    wd, gd, bd = w.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = TF.conv2d(img.double(), wd, None, 1, 2)
    a = TF.relu(TF.batch_norm(y, None, None, gd, bd, True, 0.1, 1e-5))
    p_ref = TF.max_pool2d(a, 3, 2, 1)
    gout = rnd(*p_ref.shape, seed=3)
    gw_ref, gg_ref, gb_ref = torch.autograd.grad(p_ref, (wd, gd, bd), gout.double())
    mean_ref, var_ref = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    # ---- HIP ----
    s = L.stream()
    imgd, wdv = img.to(dev), w.to(dev).contiguous()
    stats = torch.zeros(16, 2, 64, device=dev, dtype=torch.float64)
    L.call("awr_stem_stats", L.ptr(imgd), L.ptr(wdv), None, B, H, W, L.ptr(stats), 0, s)
    n = B * H * W
    st = stats.sum(0).cpu()
    assert rel_err(st[0] / n, mean_ref) < 2e-6 and rel_err(st[1] / n - (st[0] / n) ** 2, var_ref) < 2e-5
    coef4 = torch.zeros(4, 64, device=dev)
    rm, rv = torch.zeros(64, device=dev), torch.ones(64, device=dev)
    gam, bet = gamma.to(dev), beta.to(dev)
    L.call("awr_bn_finalize", L.ptr(stats), 64, n, L.ptr(gam), L.ptr(bet), L.ptr(rm), L.ptr(rv), 0.1, 1e-5, L.ptr(coef4[0]), L.ptr(coef4[1]),
           L.ptr(coef4[2]), L.ptr(coef4[3]), 0, s)
    assert float(stats.abs().max()) == 0.0                       # re-armed
    pooled = torch.empty(B, H // 2, W // 2, 64, device=dev)
    arg = torch.empty(B, H // 2, W // 2, 64, device=dev, dtype=torch.uint8)
    L.call("awr_stem_pool", L.ptr(imgd), L.ptr(wdv), L.ptr(coef4[0]), L.ptr(coef4[1]), B, H, W, L.ptr(pooled), L.ptr(arg), s)
    assert rel_err(ops.nchw(pooled).cpu(), p_ref.detach()) < 5e-6
    assert int(arg.max()) <= 8
    # eval-mode use: same kernel, folded coefficients, no argmax
    pooled2 = torch.empty_like(pooled)
    L.call("awr_stem_pool", L.ptr(imgd), L.ptr(wdv), L.ptr(coef4[0]), L.ptr(coef4[1]), B, H, W, L.ptr(pooled2), None, s)
    assert torch.equal(pooled, pooled2)
    # ---- backward ----
    dpool = ops.nhwc(gout).to(dev)
    sums = torch.zeros(16, 2, 64, device=dev, dtype=torch.float64)
    L.call("awr_stem_bwd_reduce", L.ptr(imgd), L.ptr(wdv), None, L.ptr(coef4), L.ptr(dpool), L.ptr(arg), B, H, W, L.ptr(sums), 0, s)
    coef = torch.zeros(3, 64, device=dev)
    dgam, dbet = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    L.call("awr_bn_bwd_finalize", L.ptr(sums), 64, n, L.ptr(gam), L.ptr(coef4[3]), L.ptr(coef), L.ptr(dgam), L.ptr(dbet), 0, 0, s)
    assert rel_err(dgam.cpu(), gg_ref) < 2e-5 and rel_err(dbet.cpu(), gb_ref) < 2e-5
    slots = torch.zeros(16 * 64 * 26, device=dev)
    gw = torch.empty(64, 1, 5, 5, device=dev)
    for _ in range(2):                                           # second call: the slot accumulator was re-armed by the first
        L.call("awr_stem_bwd_wgrad", L.ptr(imgd), L.ptr(wdv), None, L.ptr(coef4), L.ptr(coef), L.ptr(dpool), L.ptr(arg), B, H, W, L.ptr(slots), L.ptr(gw), None, 0, s)
        assert rel_err(gw.cpu(), gw_ref) < 5e-5
    assert float(slots.abs().max()) == 0.0


@pytest.mark.parametrize("kind,cin,cout,k,stride,B,H", [("conv", 512, 512, 3, 1, 2, 8), ("conv", 256, 512, 3, 2, 1, 16), ("deconv", 512, 256, 4, 2, 1, 8),
                                                       ("conv", 96, 160, 1, 1, 3, 8)])
def test_conv_split_k(ops, dev, kind, cin, cout, k, stride, B, H):
    """awr_conv_args.partial / split_k: blockIdx.z walks a range of the K slices, the reduce kernel sums the copies in order and applies
    bias, folded-BN affine, residual and ReLU -- against float64 and against the single-pass kernel (low-batch inference path)."""
    CC.conv_split_k(ops, dev, kind, cin, cout, k, stride, B, H)


@pytest.mark.parametrize("B,H,W", [(2, 32, 48), (2, 128, 128), (1, 16, 16)])
def test_fused_stem_dense_matches_conv_bias_bn_relu(L, dev, B, H, W):
    """Hourglass stem (hourglass.py:112): conv 5x5 (1 -> 64, pad 2, WITH bias) -> BatchNorm (batch statistics) -> ReLU at full
    resolution, and its backward from the dense gradient of that activation (BN parameter gradients, conv weight and bias
    gradients) by recomputing the conv -- against float64 torch autograd of the three operators."""
    from awr_amd import ops
    g = torch.Generator().manual_seed(11 + H)
    img = (torch.rand(B, 1, H, W, generator=g) * 2 - 1)
    img[:, :, : H // 3] = 1.0
    w = torch.randn(64, 1, 5, 5, generator=g) * 0.2
    bias = torch.randn(64, generator=g) * 0.5
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3
    wd, bsd = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = TF.conv2d(img.double(), wd, bsd, 1, 2)
    a_ref = TF.relu(TF.batch_norm(y, None, None, gd, bd, True, 0.1, 1e-5))
    gout = rnd(*a_ref.shape, seed=4)
    gw_ref, gg_ref, gb_ref = torch.autograd.grad(a_ref, (wd, gd, bd), gout.double())
    mean_ref, var_ref = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    s = L.stream()
    imgd, wdv, bsv = img.to(dev), w.to(dev).contiguous(), bias.to(dev)
    stats = torch.zeros(16, 2, 64, device=dev, dtype=torch.float64)
    L.call("awr_stem_stats", L.ptr(imgd), L.ptr(wdv), L.ptr(bsv), B, H, W, L.ptr(stats), 0, s)
    n = B * H * W
    st = stats.sum(0).cpu()
    assert rel_err(st[0] / n, mean_ref) < 2e-6 and rel_err(st[1] / n - (st[0] / n) ** 2, var_ref) < 2e-5
    coef4 = torch.zeros(4, 64, device=dev)
    rm, rv = torch.zeros(64, device=dev), torch.ones(64, device=dev)
    gam, bet = gamma.to(dev), beta.to(dev)
    L.call("awr_bn_finalize", L.ptr(stats), 64, n, L.ptr(gam), L.ptr(bet), L.ptr(rm), L.ptr(rv), 0.1, 1e-5, L.ptr(coef4[0]), L.ptr(coef4[1]),
           L.ptr(coef4[2]), L.ptr(coef4[3]), 0, s)
    assert rel_err(rm.cpu(), 0.1 * mean_ref) < 2e-6
    act = torch.empty(B, H, W, 64, device=dev)
    L.call("awr_stem_conv", L.ptr(imgd), L.ptr(wdv), L.ptr(bsv), L.ptr(coef4[0]), L.ptr(coef4[1]), 1, B, H, W, L.ptr(act), s)
    assert rel_err(ops.nchw(act).cpu(), a_ref.detach()) < 5e-6
    pre = torch.empty_like(act)                               # relu = 0: the plain normalised map
    L.call("awr_stem_conv", L.ptr(imgd), L.ptr(wdv), L.ptr(bsv), L.ptr(coef4[0]), L.ptr(coef4[1]), 0, B, H, W, L.ptr(pre), s)
    assert rel_err(ops.nchw(pre).cpu(), TF.batch_norm(y, None, None, gd, bd, True, 0.1, 1e-5).detach()) < 5e-6
    # ---- backward from the dense gradient ----
    dg = ops.nhwc(gout).to(dev)
    sums = torch.zeros(16, 2, 64, device=dev, dtype=torch.float64)
    L.call("awr_stem_bwd_reduce", L.ptr(imgd), L.ptr(wdv), L.ptr(bsv), L.ptr(coef4), L.ptr(dg), None, B, H, W, L.ptr(sums), 0, s)
    coef = torch.zeros(3, 64, device=dev)
    dgam, dbet = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    L.call("awr_bn_bwd_finalize", L.ptr(sums), 64, n, L.ptr(gam), L.ptr(coef4[3]), L.ptr(coef), L.ptr(dgam), L.ptr(dbet), 0, 0, s)
    assert rel_err(dgam.cpu(), gg_ref) < 2e-5 and rel_err(dbet.cpu(), gb_ref) < 2e-5
    slots = torch.zeros(16 * 64 * 26, device=dev)
    gw, gbias = torch.empty(64, 1, 5, 5, device=dev), torch.full((64,), 7.0, device=dev)
    for _ in range(2):
        L.call("awr_stem_bwd_wgrad", L.ptr(imgd), L.ptr(wdv), L.ptr(bsv), L.ptr(coef4), L.ptr(coef), L.ptr(dg), None, B, H, W, L.ptr(slots), L.ptr(gw),
               L.ptr(gbias), 0, s)
        assert rel_err(gw.cpu(), gw_ref) < 5e-5
        # a bias in front of a BatchNorm has a zero gradient in exact arithmetic: what is left is rounding noise of a sum of n terms
        assert float(gbias.abs().max()) < 1e-6 * n * float(gout.abs().mean())
    assert float(slots.abs().max()) == 0.0
    # the bias column proper: with the identity as "BatchNorm backward" (k1 = k2 = 0, gamma*invstd = 1) it is sum of relu' * g
    ident = torch.zeros(3, 64, device=dev)
    ident[2] = 1.0
    L.call("awr_stem_bwd_wgrad", L.ptr(imgd), L.ptr(wdv), L.ptr(bsv), L.ptr(coef4), L.ptr(ident), L.ptr(dg), None, B, H, W, L.ptr(slots), L.ptr(gw),
           L.ptr(gbias), 0, s)
    assert rel_err(gbias.cpu(), (gout.double() * (a_ref.detach() > 0)).sum((0, 2, 3))) < 2e-5


@pytest.mark.parametrize("kind,cin,cout,k,stride,B,H", [
    ("conv", 64, 64, 3, 1, 2, 32), ("conv", 96, 160, 3, 1, 3, 16),        # ragged channel tiles, odd batch
    ("conv", 64, 128, 3, 2, 2, 32), ("conv", 128, 256, 3, 2, 3, 16),      # strided: D map 16x16 / 8x8
    ("deconv", 128, 64, 4, 2, 2, 8), ("deconv", 512, 256, 4, 2, 1, 8), ("deconv", 96, 96, 4, 2, 3, 16),
    ("conv", 256, 256, 3, 1, 1, 8),                                        # 8x8 map: two patches per image
])
def test_wgrad_one_wave_per_tap(ops, L, dev, kind, cin, cout, k, stride, B, H):
    """awr_conv_wgrad algo 2 (a workgroup owns a 64x64 channel tile for all taps, wave t contracts tap t from one staged D patch
    + halo'd G patch) against float64 autograd and against algo 1, with the fused BatchNorm+ReLU loader and the bias-gradient
    by-product, and with split-K chunk counts that do not divide the patch count."""
    CC.wgrad_one_wave_per_tap(ops, L, dev, kind, cin, cout, k, stride, B, H)


@pytest.mark.parametrize("cin,cout,B,H,affine", [(64, 64, 2, 32, True), (64, 96, 3, 16, False), (128, 160, 2, 8, True), (96, 64, 1, 64, True), (64, 64, 5, 8, False)])
def test_wgrad_one_workgroup_per_kernel_row(ops, L, dev, cin, cout, B, H, affine):
    """awr_conv_wgrad algo 3 (3x3 stride 1: a workgroup contracts 16 staged D pixels against the three taps of one kernel row from one halo'd
    G row segment, three accumulators per wave, operands by LDS-DMA) against float64 autograd and against algo 1: maps of 64 / 32 / 16 pixels
    (one-row stages) and 8 pixels (two-row stages), ragged channel tiles, the fused BatchNorm + ReLU loader on the gathered operand (halo and
    padding pixels must stay zero through it), the bias gradient from the A fragments, and split-K depths with a ragged last chunk."""
    CC.wgrad_one_workgroup_per_kernel_row(ops, L, dev, cin, cout, B, H, affine)


@pytest.mark.parametrize("B,H,cin,k,n1,cx,tm", [(2, 16, 128, 3, 128, 0, 1), (3, 10, 128, 3, 128, 0, 1), (1, 8, 64, 1, 128, 0, 1),      # ragged M (300 pixels), a 1x1 first conv
                                                (2, 16, 128, 3, 128, 128, 1), (3, 10, 64, 3, 64, 64, 2), (3, 10, 64, 3, 64, 64, 1), (2, 16, 64, 3, 64, 0, 2)])
def test_fused_conv_pair(ops, L, dev, B, H, cin, k, n1, cx, tm):
    """awr_conv_args.w2: conv (cin -> n1) -> bias -> folded BatchNorm -> ReLU -> conv 1x1 (n1 [+ cx channels of a second tensor] -> 2 n1) ->
    bias2 [-> + residual] in ONE launch (the hourglass residual's conv2 / bn3 / conv3 / skip at inference, hourglass.py:44-59: identity skip =
    residual, skip conv = extra K of the second GEMM), against float64 and against the two-launch form; 64x128, 128x64 and 64x64 tiles."""
    CC.fused_conv_pair(ops, L, dev, B, H, cin, k, n1, cx, tm)


@pytest.mark.parametrize("tm,tn", [(1, 1), (1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("cin,cout,B,H", [(128, 160, 3, 10), (256, 128, 2, 16), (64, 96, 2, 12)])      # ragged M and N; 4 / 8 / 2 K-slices
def test_short_k_epilogue_operand_prefetch(ops, L, dev, tm, tn, cin, cout, B, H):
    """1x1 convs with at most eight K-slices whose epilogue reads ONE operand tensor run the instantiation that requests that tensor's
    rows ahead of their use (tile (0, 0) before the K loop): residual + statistics forward (hourglass.py:44-59 conv3 + identity skip), and
    the data gradient with the fused BatchNorm-backward reduction (mask re-derived from y), every tile, against float64 and against the
    plain instantiation (AWR_NO_EPRE is read once per process: the comparison is with the 3x3 / two-operand paths' arithmetic, i.e. float64)."""
    CC.short_k_epilogue_operand_prefetch(ops, L, dev, tm, tn, cin, cout, B, H)


@pytest.mark.parametrize("staging_at_launch", [2, 0])
def test_deterministic_wgrad_copies_survive_a_mode_switch(ops, L, dev, staging_at_launch):
    """a deterministic plan sizes its K-chunk copies of a weight gradient when it is built; the kernel a launch picks follows the
    process-wide staging mode AT LAUNCH TIME and may write fewer copies -- the batched scatter sums ALL of them.  awr_conv_wgrad zero-fills the
    copies it leaves unwritten: poisoned scratch, copies sized in one mode, launched in the other, and the sum of all copies is the gradient."""
    import ctypes as C
    spec = ops.ConvSpec("conv", 64, 64, 3, 1, 1)
    B, H = 4, 16
    x, gy = rnd(B, 64, H, H, seed=1), rnd(B, 64, H, H, seed=2)
    prob = spec.wgrad_problem(H, H)
    D, G = (ops.nhwc(gy).to(dev), ops.nhwc(x).to(dev)) if prob["D"] == "dy" else (ops.nhwc(x).to(dev), ops.nhwc(gy).to(dev))
    ld = prob["Cg"]
    rsize = prob["Cd"] * len(prob["taps"]) * ld
    ref = TF.conv2d(x.double().transpose(0, 1), gy.double().transpose(0, 1), padding=1).transpose(0, 1)      # (cout, cin, 3, 3)
    sizes = {}
    try:
        for mode in (2, 0):          # how many copies each mode's kernel writes
            L.call("awr_set_gemm_staging", mode)
            a = ops.make_wgrad_args(prob, B, D, G, D, ld)
            a.split_stride, a.max_split = rsize, 64
            n = C.c_int()
            L.call("awr_conv_wgrad_splits", C.byref(a), C.byref(n))
            sizes[mode] = n.value
        built = max(sizes.values()) + 2                      # what a plan built in the "larger" mode (and then some) would have allocated
        R = torch.full((built, rsize), float("nan"), device=dev)
        L.call("awr_set_gemm_staging", staging_at_launch)
        a = ops.make_wgrad_args(prob, B, D, G, R, ld)
        a.split_stride, a.max_split = rsize, built
        L.call("awr_conv_wgrad", C.byref(a), L.stream())
        torch.cuda.synchronize()
        assert not torch.isnan(R).any()
        assert bool((R[sizes[staging_at_launch]:] == 0).all())              # the unwritten copies were cleared, not left stale
        grad = torch.empty(prob["d0"], prob["d1"], 3, 3, device=dev)
        Rs = R.sum(0).contiguous()
        L.call("awr_unpack_wgrad", L.ptr(Rs), prob["d0"], prob["d1"], spec.T, ld, L.ptr(grad), 0, L.stream())
        assert rel_err(grad.cpu(), ref) < 2e-6
    finally:
        L.call("awr_set_gemm_staging", 2)


@pytest.mark.parametrize("k,s,p,B,H,C,lazy", [(2, 2, 0, 3, 16, 128, False), (2, 2, 0, 2, 8, 256, True), (3, 2, 1, 2, 14, 64, True), (2, 2, 0, 5, 12, 2048, False)])
def test_maxpool_and_upsample_add_with_fused_statistics(L, dev, k, s, p, B, H, C, lazy):
    """Round 5: awr_maxpool_fwd_stats / awr_upsample2_add_stats write exactly what awr_maxpool_fwd / awr_upsample2_add write (values and argmax bit for
    bit) and leave, in the slot layout of awr_channel_stats, the per-channel sum and sum of squares of that tensor -- the statistics pass the next
    BatchNorm would otherwise run over it (hourglass.py:62-88).  Incl. the un-materialised BatchNorm + ReLU on the pool's input, a padded 3x3 / 2
    window, ragged row slabs and the 2048-channel chunking; nearly constant channels keep their variance (shifted sums)."""
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(B, H, H, C, generator=g) * 0.5 + 3.0).to(dev)                 # |mean| >> std on purpose
    sc, sh = ((torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)) if lazy else (None, None)
    Ho = (H + 2 * p - k) // s + 1
    out0, out1 = torch.full((B, Ho, Ho, C), float("nan"), device=dev), torch.full((B, Ho, Ho, C), float("nan"), device=dev)
    arg0, arg1 = torch.zeros(B, Ho, Ho, C, dtype=torch.uint8, device=dev), torch.zeros(B, Ho, Ho, C, dtype=torch.uint8, device=dev)
    st_f, st_r = torch.zeros(16, 2, C, dtype=torch.float64, device=dev), torch.zeros(16, 2, C, dtype=torch.float64, device=dev)
    L.call("awr_maxpool_fwd", L.ptr(x), L.ptr(sc), L.ptr(sh), int(lazy), B, H, H, C, k, s, p, L.ptr(out0), L.ptr(arg0), L.stream())
    L.call("awr_maxpool_fwd_stats", L.ptr(x), L.ptr(sc), L.ptr(sh), int(lazy), B, H, H, C, k, s, p, L.ptr(out1), L.ptr(arg1), L.ptr(st_f), 0, L.stream())
    L.call("awr_channel_stats", L.ptr(out0), B * Ho * Ho, C, L.ptr(st_r), 0, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(out0, out1) and torch.equal(arg0, arg1)
    ref = out0.double().reshape(-1, C)
    for name, got in (("fused", st_f.sum(0)), ("separate", st_r.sum(0))):
        assert float(((got[0] - ref.sum(0)).abs() / ref.sum(0).abs().clamp_min(1e-9)).max()) < 1e-6, name
        assert float(((got[1] - (ref * ref).sum(0)).abs() / (ref * ref).sum(0)).max()) < 1e-6, name
    # variance of a nearly constant channel: computed from the fused sums to 1e-4 relative
    n = ref.shape[0]
    var = st_f.sum(0)[1] / n - (st_f.sum(0)[0] / n) ** 2
    assert float(((var - ref.var(0, unbiased=False)).abs() / ref.var(0, unbiased=False)).max()) < 1e-4
    if k == 2 and not lazy and C <= 1024:      # up-sampling add at the same sizes: out = up1 + up(low)
        up1, low = torch.randn(B, 2 * Ho, 2 * Ho, C, generator=g).to(dev), out0
        o0, o1 = torch.empty_like(up1), torch.empty_like(up1)
        s_f, s_r = torch.zeros(16, 2, C, dtype=torch.float64, device=dev), torch.zeros(16, 2, C, dtype=torch.float64, device=dev)
        L.call("awr_upsample2_add", L.ptr(up1), L.ptr(low), B, Ho, Ho, C, L.ptr(o0), L.stream())
        L.call("awr_upsample2_add_stats", L.ptr(up1), L.ptr(low), B, Ho, Ho, C, L.ptr(o1), L.ptr(s_f), 0, L.stream())
        L.call("awr_channel_stats", L.ptr(o0), B * 4 * Ho * Ho, C, L.ptr(s_r), 0, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(o0, o1)
        r2 = o0.double().reshape(-1, C)
        assert float(((s_f.sum(0)[0] - r2.sum(0)).abs()).max()) < 1e-6 * float(r2.abs().sum(0).max())
        assert float(((s_f.sum(0)[1] - (r2 * r2).sum(0)).abs() / (r2 * r2).sum(0)).max()) < 1e-6


@study_only
@pytest.mark.parametrize("kind,cin,cout,k,stride,pad,B,H", [("conv", 64, 96, 3, 1, 1, 4, 18), ("deconv", 64, 96, 4, 2, 1, 6, 10), ("conv", 96, 64, 1, 1, 0, 2, 12)])
def test_conv_gemm_in_batch_parts_equals_the_whole_launch(ops, L, dev, kind, cin, cout, k, stride, pad, B, H):
    """awr_conv_gemm_part: images are independent rows of the GEMM, so the launch issued as 2 (or B) equal batch parts writes the SAME BITS as the
    whole launch -- input, output, residual and the fused-reduction operands all advance with the part; the statistics of the parts add up."""
    import ctypes as C
    spec = ops.ConvSpec(kind, cin, cout, k, stride, pad)
    x = rnd(B, cin, H, H, seed=1)
    w = rnd(*((cout, cin, k, k) if kind == "conv" else (cin, cout, k, k)), seed=2, scale=0.05)
    prob = spec.fwd_problem(H, H)
    xin = ops.nhwc(x).to(dev)
    if prob["Cin"] != cin:
        xin = torch.nn.functional.pad(xin, (0, prob["Cin"] - cin))
    xin = xin.contiguous()
    wp = ops.pack_weight(w.to(dev), spec.fwd_pack())
    res = rnd(B, prob["Hout"], prob["Wout"], prob["N"], seed=3).to(dev)
    bias = rnd(prob["N"], seed=4).to(dev)
    outs = []
    for nparts in (1, 2, B):
        out = torch.full((B, prob["Hout"], prob["Wout"], prob["N"]), float("nan"), device=dev)
        st = torch.zeros(16, 2, prob["N"], device=dev, dtype=torch.float64)
        a = ops.make_conv_args(prob, B, xin, wp, out, bias=bias, res=res, relu_out=True, stats=st, T=spec.T)
        for part in range(nparts):
            L.call("awr_conv_gemm_part", C.byref(a), nparts, part, L.stream())
        torch.cuda.synchronize()
        outs.append((out.clone(), st.sum(0).float()))
    for o, s_ in outs[1:]:
        assert torch.equal(outs[0][0], o)
        assert rel_err(s_.cpu(), outs[0][1].cpu()) < 1e-6
    with pytest.raises(L.AwrError):
        L.call("awr_conv_gemm_part", C.byref(a), 3 if B % 3 else 5, 0, L.stream())      # the batch is not divisible by the part count


@pytest.mark.parametrize("kind,cin,cout,k,stride,pad,B,H", [("conv", 64, 96, 3, 1, 1, 4, 18), ("deconv", 64, 96, 4, 2, 1, 6, 10), ("conv", 96, 64, 1, 1, 0, 2, 12),
                                                             ("conv", 128, 256, 1, 1, 0, 3, 16)])
def test_streaming_output_stores_write_the_same_bits(ops, L, dev, kind, cin, cout, k, stride, pad, B, H):
    """awr_conv_args.out_nt: 1 = cached, 2 = streaming (`buffer_store ... nt`, the epilogue's residual loads `nt` too), 0 = the library's size / K-extent rule.
    A cache policy: every form writes the SAME BITS and the same statistics, with the residual + ReLU + statistics epilogue and on the short-K
    operand-prefetch form (the two 1x1 shapes); an unknown policy is refused."""
    import ctypes as C
    spec = ops.ConvSpec(kind, cin, cout, k, stride, pad)
    x = rnd(B, cin, H, H, seed=1)
    w = rnd(*((cout, cin, k, k) if kind == "conv" else (cin, cout, k, k)), seed=2, scale=0.05)
    prob = spec.fwd_problem(H, H)
    xin = ops.nhwc(x).to(dev).contiguous()
    wp = ops.pack_weight(w.to(dev), spec.fwd_pack())
    res = rnd(B, prob["Hout"], prob["Wout"], prob["N"], seed=3).to(dev)
    bias = rnd(prob["N"], seed=4).to(dev)
    outs = []
    for policy in (1, 2, 0):
        out = torch.full((B, prob["Hout"], prob["Wout"], prob["N"]), float("nan"), device=dev)
        st = torch.zeros(16, 2, prob["N"], device=dev, dtype=torch.float64)
        a = ops.make_conv_args(prob, B, xin, wp, out, bias=bias, res=res, relu_out=True, stats=st, T=spec.T)
        a.out_nt = policy
        L.call("awr_conv_gemm", C.byref(a), L.stream())
        torch.cuda.synchronize()
        outs.append((out.clone(), st.sum(0).float()))
    assert not torch.isnan(outs[0][0]).any()
    for o, s_ in outs[1:]:
        assert torch.equal(outs[0][0], o)
        assert rel_err(s_.cpu(), outs[0][1].cpu()) < 1e-6
    a.out_nt = 3
    with pytest.raises(L.AwrError):
        L.call("awr_conv_gemm", C.byref(a), L.stream())


@pytest.mark.parametrize("tile", [(1, 1), (2, 1), (1, 2)])
@pytest.mark.parametrize("affine", [False, True])
def test_blocked_accumulation_in_the_deep_pipeline_is_bit_identical(ops, L, dev, tile, affine):
    """Round 6: launches that cannot fill the chip (<= 384 workgroups: layer4 at batch 64, the two-image fixtures) take the deep pipeline (four stage
    buffers) in the BLOCKED accumulation mode too -- same k order, same fold points every 128 k, so the same bits as the two-buffer blocked kernel;
    and blocked differs from ordered (otherwise the flag did nothing).  3x3, K = 1152, statistics epilogue, with / without the fused input affine."""
    import ctypes as C
    B, H, cin, cout = 2, 8, 128, 128
    spec = ops.ConvSpec("conv", cin, cout, 3, 1, 1)
    x, w = rnd(B, cin, H, H, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.05)
    prob = spec.fwd_problem(H, H)
    xin = ops.nhwc(x).to(dev).contiguous()
    wp = ops.pack_weight(w.to(dev), spec.fwd_pack())
    sc, sh = (rnd(cin, seed=5).abs().to(dev) + 0.5, rnd(cin, seed=6).to(dev)) if affine else (None, None)
    got = {}
    L.call("awr_debug_force_tile", *tile)
    try:
        for accum, deep in ((1, 1), (1, 0), (0, 1)):
            L.call("awr_debug_set_knob", b"deep", deep)
            out = torch.full((B, H, H, prob["N"]), float("nan"), device=dev)
            st = torch.zeros(16, 2, prob["N"], device=dev, dtype=torch.float64)
            a = ops.make_conv_args(prob, B, xin, wp, out, in_scale=sc, in_shift=sh, relu_in=affine, stats=st, T=spec.T)
            a.accum = accum
            L.call("awr_conv_gemm", C.byref(a), L.stream())
            torch.cuda.synchronize()
            got[(accum, deep)] = (out.clone(), st.sum(0).clone())
    finally:
        L.call("awr_debug_set_knob", b"deep", 1)
        L.call("awr_debug_force_tile", 0, 0)
    assert not torch.isnan(got[(1, 1)][0]).any()
    assert torch.equal(got[(1, 1)][0], got[(1, 0)][0]) and torch.equal(got[(1, 1)][1], got[(1, 0)][1])
    assert not torch.equal(got[(1, 1)][0], got[(0, 1)][0])
    assert rel_err(got[(1, 1)][0].cpu(), got[(0, 1)][0].cpu()) < 1e-5


@pytest.mark.parametrize("tile", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_statistics_from_the_accumulators_match_the_row_layout_form(ops, L, dev, tile):
    """EM 5 (round 5): a statistics launch whose stored value is accumulator + bias on tiles wholly inside M sums x - c and (x - c)^2 in the ACCUMULATOR
    layout (a lane owns one channel, its registers 16 rows) instead of behind the LDS bounce.  Same output bits; sum and sum of squares agree with the
    row-layout form (awr_debug_set_knob fast_stats = 0) and with float64 sums of the stored tensor -- on a ragged N (96 of a 128-column tile), with a bias that puts the
    mean 100 standard deviations from zero (the shift is what keeps the variance)."""
    CC.statistics_from_the_accumulators(ops, L, dev, tile)
