"""GPU parity of the implicit-GEMM convolution family (awr_conv_gemm, awr_conv_wgrad and every launch form of theirs) on NON-SQUARE feature
maps, through the checks of tests/conv_cases.py that tests/test_ops_gpu.py runs on square ones -- same references (float64 torch on the CPU,
or the second launch form of the operator), same tolerances.  On a square map a kernel that strides a row by H instead of W, shifts by
log2 H instead of log2 W or tiles patches the wrong way round computes the right answer; tests/test_host_cpu.py shows that on these maps
such a swap is off by more than 100 % of the result's scale.

Shapes are the GEMM's ROW map (Hq x Wq forward / data gradient, Hd x Wd weight gradient): a stride-2 conv reads twice that, a transposed conv
reads it and writes twice it.  (4, 16) / (16, 4): both sides powers of two with different shifts; (6, 8) / (8, 6): exactly one side a power of
two -- decode_row and the weight-gradient launcher must take the division path; (10, 14): neither.  Batch 3: M is ragged against the 64- and
128-row tiles at (6, 8), (8, 6), (10, 14).  Channels 64 -> 96 and 128 -> 160: ragged N, 2 and 4 K-slices.

What a non-square map can and cannot show.  A 1x1 stride-1 conv is pointwise: its result does not depend on how the pixels are arranged in rows
(tests/test_host_cpu.py), so the forms that exist only as such layers -- the two-tensor K extent without w2 and the short-K operand prefetch --
see ragged M and the row count here, not a swapped row stride; `in2` next to a 3x3 first conv is covered by the fused pair.  Which weight-gradient
kernel a case of the automatic path reaches is fixed by the launcher's rules (awr_wgrad.hip: wgrad_plan, conv_wgrad_one), not asserted.

Every case prints its measured errors as a `conv_rect <family> <H>x<W> name=value ...` line (pytest -s).  The 8 x 8 map runs with the same
layers and batch as the square map of the same K: profiles/conv_rect_errors.txt is the per-family maximum of those lines, non-square maps
next to 8 x 8 (32 x 32 for the stem)."""
import ctypes as C

import pytest
import torch

import conv_cases as CC
from conv_cases import rel_err, rnd

pytestmark = pytest.mark.gpu

B = 3
SQUARE = (8, 8)                                            # the comparison map of the same K (see the module docstring)
RECT_SHAPES = [(4, 16), (16, 4), (6, 8), (8, 6), (10, 14)]
SHAPES = RECT_SHAPES + [SQUARE]
POW2_AND_MIXED = [(4, 16), (6, 8), SQUARE]                 # one non-square shape of each class for the launch forms of section (b)
WGRAD_ALGO_SHAPES = [(2, 32), (16, 8), (4, 32), (4, 16), SQUARE]      # Hd >= patch rows, Wd >= 8: one-row and two-row stages, 8- and 16-pixel row segments
REFUSED_SHAPES = [(16, 4), (6, 8)]                         # Wd < 8; a side that is no power of two
# kind, cin, cout, k, stride, pad
KINDS = [("conv", 64, 96, 3, 1, 1), ("conv", 128, 160, 3, 2, 1), ("conv", 64, 96, 1, 2, 0), ("conv", 128, 160, 1, 1, 0), ("deconv", 128, 160, 4, 2, 1)]
TILES = [(1, 1), (1, 2), (2, 1), (2, 2)]


def _id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) and all(isinstance(i, int) for i in v) else "-".join(str(i) for i in v)


def _study():
    import awr_amd  # noqa: F401
    from awr_amd import _lib
    return _lib.HAS_STUDY


study_only = pytest.mark.skipif(not _study(), reason="study form: needs libawr_hip.so built with -DAWR_STUDY")


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


def report(family, shape, errs):
    print("conv_rect %s %dx%d %s" % (family, shape[0], shape[1], " ".join("%s=%.3g" % kv for kv in sorted(errs.items()))))


# ---- (a) forward, data gradient, weight gradient, bias gradient, both accumulate forms: every tile, product mode and staging -----------------
@pytest.mark.parametrize("products,staging", [(1, 2), (1, 0), (6, 2)])
@pytest.mark.parametrize("tile", TILES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("layer", KINDS, ids=_id)
def test_rect_forward_dgrad_wgrad_every_tile(ops, L, dev, layer, shape, tile, products, staging):
    kind, cin, cout, k, stride, pad = layer
    H, W = CC.input_hw(kind, stride, *shape)
    report("layer_%s_k%d_s%d_p%d_st%d" % (kind, k, stride, products, staging), shape,
           CC.conv_every_tile_shape(ops, L, dev, products, staging, tile[0], tile[1], kind, cin, cout, k, stride, pad, B, H, W))


# ---- (b) the remaining launch forms, each against the reference its square test uses -----------------------------------------------------------
LAYERS_B = [("conv", 64, 96, 3, 1, 1), ("conv", 128, 160, 3, 2, 1), ("deconv", 64, 96, 4, 2, 1), ("conv", 96, 64, 1, 1, 0)]


@pytest.mark.parametrize("shape", POW2_AND_MIXED, ids=_id)
@pytest.mark.parametrize("layer", [("conv", 128, 160, 3, 1), ("conv", 128, 160, 3, 2), ("deconv", 128, 160, 4, 2), ("conv", 96, 160, 1, 1)], ids=_id)
def test_rect_split_k(ops, dev, layer, shape):
    """Split-K depths 0 / 2 / 4 / 8 with NaN-filled scratch: the copies' strides are B * Hout * Wout * N."""
    kind, cin, cout, k, stride = layer
    H, W = CC.input_hw(kind, stride, *shape)
    report("split_k_%s_k%d_s%d" % (kind, k, stride), shape, CC.conv_split_k(ops, dev, kind, cin, cout, k, stride, B, H, W))


@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("tile", TILES, ids=_id)
@pytest.mark.parametrize("shape", POW2_AND_MIXED, ids=_id)
@pytest.mark.parametrize("layer", LAYERS_B, ids=_id)
def test_rect_dgrad_with_unmaterialised_batchnorm_backward(ops, L, dev, layer, shape, tile, accum):
    kind, cin, cout, k, stride, pad = layer
    H, W = CC.input_hw(kind, stride, *shape)
    report("dgrad_bnb_%s_k%d_s%d" % (kind, k, stride), shape,
           CC.dgrad_with_unmaterialised_batchnorm_backward(ops, L, dev, accum, tile[0], tile[1], kind, cin, cout, k, stride, pad, B, H, W))


@pytest.mark.parametrize("shape", POW2_AND_MIXED, ids=_id)
@pytest.mark.parametrize("cin,k,n1,cx,tm", [(128, 3, 128, 0, 1), (64, 1, 128, 0, 1), (128, 3, 128, 128, 1), (64, 3, 64, 64, 2), (64, 3, 64, 64, 1), (64, 3, 64, 0, 2)])
def test_rect_fused_conv_pair(ops, L, dev, cin, k, n1, cx, tm, shape):
    """awr_conv_args.w2 with and without the second tensor (in2 / N1x), against float64 and the two-launch form."""
    report("pair_k%d_cx%d" % (k, cx), shape, CC.fused_conv_pair(ops, L, dev, B, shape[0], cin, k, n1, cx, tm, W=shape[1]))


@pytest.mark.parametrize("tile", TILES, ids=_id)
@pytest.mark.parametrize("shape", POW2_AND_MIXED, ids=_id)
@pytest.mark.parametrize("cin,cout", [(128, 160), (64, 96)])
def test_rect_short_k_epilogue_operand_prefetch(ops, L, dev, cin, cout, shape, tile):
    report("short_k", shape, CC.short_k_epilogue_operand_prefetch(ops, L, dev, tile[0], tile[1], cin, cout, B, shape[0], W=shape[1]))


@study_only
@pytest.mark.parametrize("tile", TILES, ids=_id)
@pytest.mark.parametrize("shape", POW2_AND_MIXED, ids=_id)
@pytest.mark.parametrize("layer", LAYERS_B, ids=_id)
def test_rect_split_mode_with_precut_activations_is_bit_identical(ops, L, dev, layer, shape, tile):
    kind, cin, cout, k, stride, pad = layer
    H, W = CC.input_hw(kind, stride, *shape)
    report("precut_%s_k%d_s%d" % (kind, k, stride), shape,
           CC.split_mode_with_precut_activations(ops, L, dev, tile[0], tile[1], kind, cin, cout, k, stride, pad, B, H, W))


@pytest.mark.parametrize("tile", TILES, ids=_id)
@pytest.mark.parametrize("shape", POW2_AND_MIXED, ids=_id)
def test_rect_lds_dma_staging_is_bit_identical_to_register_staging(ops, L, dev, shape, tile):
    """Every fused form of the square test, including the two-tensor K extent (in2 without w2, against float64), with H x W as each GEMM's
    row map: same bits from register staging, LDS-DMA with the deep pipeline and LDS-DMA without it.  (The two-tensor and short-K sub-cases
    are pointwise layers: see the module docstring.)"""
    report("staging", shape, CC.lds_dma_staging_vs_register_staging(ops, L, dev, tile[0], tile[1], maps=CC.staging_maps(*shape)))


@pytest.mark.parametrize("shape", POW2_AND_MIXED, ids=_id)
def test_rect_conv_fused_prologue_epilogue_stats(ops, dev, shape):
    report("prologue_epilogue_stats", shape, CC.conv_fused_prologue_epilogue_stats(ops, dev, B=B, H=shape[0], cin=64, cout=96, W=shape[1]))


@pytest.mark.parametrize("tile", TILES, ids=_id)
@pytest.mark.parametrize("shape", POW2_AND_MIXED, ids=_id)
def test_rect_statistics_from_the_accumulators_match_the_row_layout_form(ops, L, dev, shape, tile):
    """M = 192 / 144: whole tiles (accumulator-layout sums) and a ragged last one (row-layout sums) in the same launch.  The stored values are
    checked against float64 as well: the two statistics forms share one output, so their bit-identity says nothing about its addressing."""
    errs = CC.statistics_from_the_accumulators(ops, L, dev, tile, B=B, H=shape[0], W=shape[1])
    report("stats_accumulators", shape, errs)
    assert errs["fwd"] < 5e-6


@pytest.mark.parametrize("shape", [(16, 48), (32, 32)], ids=_id)
def test_rect_stem_im2col_gemm(ops, L, dev, shape):
    report("stem_im2col", shape, CC.stem_im2col_gemm(ops, L, dev, B=B, H=shape[0], W=shape[1]))


# ---- (c) weight-gradient algorithms ---------------------------------------------------------------------------------------------------------------
def _wgrad_args(ops, L, dev, kind, cin, cout, k, stride, pad, H, W, algo):
    """A plain weight-gradient launch of the layer at input H x W: (args, its tensors), for the refusal checks."""
    spec = ops.ConvSpec(kind, cin, cout, k, stride, pad)
    prob = spec.wgrad_problem(H, W)
    ho, wo = spec.out_hw(H, W)
    x, gy = torch.zeros(B, H, W, cin, device=dev), torch.zeros(B, ho, wo, cout, device=dev)
    D, G = (gy, x) if prob["D"] == "dy" else (x, gy)
    R = torch.zeros(prob["Cd"], len(prob["taps"]), prob["Cg"], device=dev)
    return ops.make_wgrad_args(prob, B, D, G, R, prob["Cg"], algo=algo), (x, gy, R)


def _algo_ok(L, a, algo):
    return int(L.lib.awr_conv_wgrad_algo_ok(C.byref(a), algo))


@pytest.mark.parametrize("shape", WGRAD_ALGO_SHAPES, ids=_id)
@pytest.mark.parametrize("layer", [("conv", 64, 96, 3, 1), ("conv", 128, 160, 3, 2), ("deconv", 64, 96, 4, 2)], ids=_id)
def test_rect_wgrad_one_wave_per_tap(ops, L, dev, layer, shape):
    """algo 2 at Hd != Wd (pc_log != pr_log), and Hg != Wg for the strided kinds, with target_blocks 1 / 7 / 100000, the fused BatchNorm + ReLU
    loader and the bias by-product; against float64 and algo 1.  The 3x3 stride-1 form has 4-row patches: a 2 x 32 map is refused -- and
    awr_conv_wgrad_algo_ok says so."""
    kind, cin, cout, k, stride = layer
    H, W = CC.input_hw(kind, stride, *shape)
    a, keep = _wgrad_args(ops, L, dev, kind, cin, cout, k, stride, 1, H, W, 2)
    serves = shape[0] >= (4 if stride == 1 else 2)
    assert _algo_ok(L, a, 2) == int(serves)
    if serves:
        report("wgrad_taps_%s_k%d_s%d" % (kind, k, stride), shape, CC.wgrad_one_wave_per_tap(ops, L, dev, kind, cin, cout, k, stride, B, H, W))
    else:
        with pytest.raises(L.AwrError):
            L.call("awr_conv_wgrad", C.byref(a), L.stream())


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("shape", WGRAD_ALGO_SHAPES, ids=_id)
@pytest.mark.parametrize("cin,cout", [(64, 96), (128, 160)])
def test_rect_wgrad_one_workgroup_per_kernel_row(ops, L, dev, cin, cout, shape, affine):
    """algo 3 at wlog != hlog: one-row stages of 16-pixel segments (2 x 32, 4 x 32, 4 x 16) and two-row stages (16 x 8)."""
    a, keep = _wgrad_args(ops, L, dev, "conv", cin, cout, 3, 1, 1, shape[0], shape[1], 3)
    assert _algo_ok(L, a, 3) == 1
    report("wgrad_row", shape, CC.wgrad_one_workgroup_per_kernel_row(ops, L, dev, cin, cout, B, shape[0], affine, W=shape[1]))


@pytest.mark.parametrize("algo", [2, 3])
@pytest.mark.parametrize("shape", REFUSED_SHAPES, ids=_id)
@pytest.mark.parametrize("layer", [("conv", 64, 96, 3, 1), ("conv", 128, 160, 3, 2), ("deconv", 64, 96, 4, 2)], ids=_id)
def test_rect_wgrad_algorithms_refuse_what_they_do_not_serve(ops, L, dev, layer, shape, algo):
    """A 16 x 4 map (Wd < 8) and a 6 x 8 map (one side no power of two) are refused by algo 2 and algo 3, not mis-computed, and
    awr_conv_wgrad_algo_ok agrees with the launch; algo 0 and 1 serve them (section (a) and the automatic path below)."""
    kind, cin, cout, k, stride = layer
    H, W = CC.input_hw(kind, stride, *shape)
    a, keep = _wgrad_args(ops, L, dev, kind, cin, cout, k, stride, 1, H, W, algo)
    assert _algo_ok(L, a, algo) == 0 and _algo_ok(L, a, 0) == 1 and _algo_ok(L, a, 1) == 1
    with pytest.raises(L.AwrError):
        L.call("awr_conv_wgrad", C.byref(a), L.stream())


@pytest.mark.parametrize("products", [1, 6])
@pytest.mark.parametrize("affine,bias", [(False, False), (True, True)])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("layer", [("conv", 64, 96, 3, 1, 1), ("conv", 128, 160, 3, 2, 1), ("conv", 128, 160, 1, 1, 0), ("deconv", 64, 96, 4, 2, 1)], ids=_id)
def test_rect_wgrad_automatic_path(ops, L, dev, layer, shape, affine, bias, products):
    """algo 0 as a plan launches it, against float64.  By the launcher's rules (not asserted here) the parameters reach, in FP32-MFMA mode: the
    LDS-DMA kernel for plain operands on power-of-two maps (the kernel-row one for 3x3 stride 1 from 8 pixels wide); the multiply-free
    conv_wgrad_kernel<.., true> for an operand through registers (fused BatchNorm + ReLU loader, bias by-product); the generic kernel
    (wshift = hshift = -1) for both when a side is no power of two; in split mode the split kernel.  Each with Hd != Wd and, for the strided
    kinds, Hg != Wg.  The comparison with algo 1 says something only where algo 0 picks the kernel-row kernel: everywhere else algo 0 IS algo 1
    (the same launch twice), and float64 is the check."""
    kind, cin, cout, k, stride, pad = layer
    H, W = CC.input_hw(kind, stride, *shape)
    spec = ops.ConvSpec(kind, cin, cout, k, stride, pad)
    x = rnd(B, cin, H, W, seed=2)
    s_, t_ = rnd(cin, seed=5) + 0.3, rnd(cin, seed=6) * 0.5
    act = torch.relu(x * s_.view(1, -1, 1, 1) + t_.view(1, -1, 1, 1)) if affine else x
    wd = torch.zeros(*CC.wshape_of(kind, cin, cout, k), dtype=torch.float64, requires_grad=True)
    y_ref = CC.torch_fwd(kind, act.double(), wd, None, stride, pad)
    gy = rnd(*y_ref.shape, seed=4)
    (gw_ref,) = torch.autograd.grad(y_ref, [wd], gy.double())
    xg, gyg = ops.nhwc(x).to(dev), ops.nhwc(gy).to(dev)
    aff = (s_.to(dev), t_.to(dev), True) if affine else None
    bg = torch.empty(cout, device=dev) if bias and kind == "conv" else None
    L.call("awr_set_gemm_products", products)
    try:
        gw = ops.conv_wgrad(spec, xg, gyg, x_affine=aff, bias_grad=bg, algo=0)
        old = ops.conv_wgrad(spec, xg, gyg, x_affine=aff, algo=1)
    finally:
        L.call("awr_set_gemm_products", 1)
    errs = dict(wgrad=rel_err(gw.cpu(), gw_ref), vs_algo1=rel_err(gw.cpu(), old.cpu()))
    if bg is not None:
        errs["bgrad"] = rel_err(bg.cpu(), gy.double().sum((0, 2, 3)))
    report("wgrad_auto_%s_k%d_s%d_p%d_aff%d" % (kind, k, stride, products, affine), shape, errs)
    assert errs["wgrad"] < 1e-5
    assert errs["vs_algo1"] < 2e-6
    assert errs.get("bgrad", 0.0) < 1e-5
