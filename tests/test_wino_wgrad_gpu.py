"""GPU: the Winograd-domain weight gradient (awr_wino_wgrad, csrc/awr_wino.hip: wino_wgrad_kernel + wino_wgrad_reduce_kernel) as an operator,
at the loop depths plans really run.  tests/test_wino_gpu.py::test_winograd_weight_gradient_matches_float64 runs one pair of stages per split;
the shapes here (tests/wino_wgrad_cases.py; what each one reaches is asserted without a GPU in tests/test_wino_wgrad_cpu.py) run 2 to 18
stages per split, ranges of different length inside one launch, and every part of the reduce kernel's split-copy sum.

Two kinds of inputs.  `exact`: small integers, for which every intermediate of the kernels is exactly representable in fp32
(wino_wgrad_cases.exact_bound_holds), so the kernels must return the float64 autograd result BIT FOR BIT -- a stage dropped, doubled or read
from a buffer that was already overwritten changes an integer.  `random`: normal inputs against the project's bar for this kernel, a relative
error max|diff| / max|ref| below 2e-5.

Measured worst relative error of the random-input test per shape (weight gradient, bias gradient; MI355X):
    1x8x8x64x64        1.66e-07  9.96e-08        5x16x32x256x256    2.22e-07  1.34e-07
    2x8x8x256x512      1.85e-07  8.42e-08        5x8x16x512x512     2.46e-07  1.15e-07
    2x16x16x64x192     1.76e-07  1.65e-07        3x32x32x256x256    2.37e-07  2.08e-07
    3x32x32x192x128    2.00e-07  1.72e-07        4x16x16x512x512    2.37e-07  8.73e-08
    5x64x64x64x64      2.18e-07  4.78e-07        16x32x32x128x128   2.41e-07  2.44e-07
    6x8x8x512x512      2.73e-07  8.14e-08        9x16x16x512x512    3.53e-07  1.01e-07
The deepest sums (5120 patches) stay a factor of 40 below the bar; no shape needed a bar of its own.

What the module was checked against (scratch builds of the library with one line of the kernels changed; none of them is in the repository):
the refill request `min(g_lo + i + 3, g_last)` made `min(g_lo + i + 2, g_last)` fails the exact and the random test on every shape with 4 or
more stages per split and passes on the three shapes with 2; the bias sum without its `live` condition fails both on every shape; the reduce
kernel's tail loop skipping its first copy fails both on every shape whose groups have a tail.  Starting that tail loop at accumulator 1
instead of 0 adds the same copies in another order: by design no exact-input test can tell, and the random one stays far below the bar.
"""
import pytest
import torch

import wino_wgrad_cases as WC

pytestmark = pytest.mark.gpu

GUARD = 4096
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    import awr_amd  # noqa: F401
    from awr_amd import _lib as L
    return L, torch.device("cuda:0")


def run(env, shape, form, x, dy, sc, sh, bias=True, ld_extra=64, scratch=None):
    """One launch on NaN-filled outputs -> (R (N, 9, ld), bias gradient (N) or None, scratch with its guard).  Every buffer the kernels write
    starts as NaN: an element they skip stays NaN, one they should not touch has to."""
    L, dev = env
    B, H, W, C, N = shape
    affine, relu = form
    n = int(L.lib.awr_wino_wgrad_scratch(B, H, W, C, N))
    if scratch is None:
        scratch = torch.full((n + GUARD,), NAN, device=dev)
    assert scratch.numel() == n + GUARD
    ld = C + ld_extra
    R = torch.full((N, 9, ld), NAN, device=dev)
    bg = torch.full((N,), NAN, device=dev) if bias else None
    xd, dyd = x.permute(0, 2, 3, 1).contiguous().to(dev), dy.permute(0, 2, 3, 1).contiguous().to(dev)
    scd, shd = (sc.to(dev), sh.to(dev)) if affine else (None, None)
    L.call("awr_wino_wgrad", L.ptr(xd), L.ptr(dyd), L.ptr(scd), L.ptr(shd), int(relu), B, H, W, C, N, L.ptr(scratch), L.ptr(R), ld, L.ptr(bg), L.stream())
    torch.cuda.synchronize()
    assert torch.isnan(scratch[n:]).all()                   # nothing behind the split copies is touched
    assert torch.isnan(R[:, :, C:]).all()                   # nothing beyond the C columns of a packed row is touched
    return R, bg, scratch


def weight_gradient(R, shape):
    """packed R (N, 9, ld) -> (N, C, 3, 3) on the host"""
    C, N = shape[3], shape[4]
    return R[:, :, :C].cpu().permute(0, 2, 1).reshape(N, C, 3, 3)


def forms_of(shape):
    return WC.FORMS if shape[3] >= 128 else [(True, True), (False, False)]


EXACT_CASES = [pytest.param(s, f, id="%s-affine%d-relu%d" % (WC.shape_id(s), f[0], f[1])) for s in WC.SHAPES for f in forms_of(s)]


def shapes(*which):
    assert set(which) <= set(WC.SHAPES)
    return pytest.mark.parametrize("shape", which, ids=WC.shape_id)


@pytest.mark.parametrize("shape,form", EXACT_CASES)
def test_exact_inputs_give_the_float64_gradient_bit_for_bit(env, shape, form):
    x, dy, sc, sh = WC.inputs(shape, form, "exact")
    gw, gb = WC.reference(shape, form, "exact")
    R, bg, _ = run(env, shape, form, x, dy, sc, sh)
    got, gotb = weight_gradient(R, shape).double(), bg.cpu().double()
    print("%s affine=%d relu=%d: weight gradient differs in %d of %d elements (max %g), bias gradient in %d of %d (max %g)" % (
        WC.shape_id(shape), form[0], form[1], int((got != gw).sum()), gw.numel(), float((got - gw).abs().nan_to_num(nan=float("inf")).max()),
        int((gotb != gb).sum()), gb.numel(), float((gotb - gb).abs().nan_to_num(nan=float("inf")).max())))
    assert torch.equal(got, gw)
    assert torch.equal(gotb, gb)


@pytest.mark.parametrize("shape", WC.SHAPES, ids=WC.shape_id)
def test_random_inputs_meet_the_projects_bar(env, shape):
    form = (True, True)
    x, dy, sc, sh = WC.inputs(shape, form, "random")
    gw, gb = WC.reference(shape, form, "random")
    R, bg, _ = run(env, shape, form, x, dy, sc, sh)
    got = weight_gradient(R, shape)
    assert torch.isfinite(got).all() and torch.isfinite(bg).all()
    err = float((got.double() - gw).abs().max()) / float(gw.abs().max())
    eb = float((bg.cpu().double() - gb).abs().max()) / float(gb.abs().max())
    print("%s: relative error of the weight gradient %.3g, of the bias gradient %.3g" % (WC.shape_id(shape), err, eb))
    assert err < 2e-5, err
    assert eb < 2e-5, eb


@shapes((3, 32, 32, 192, 128), (1, 8, 8, 64, 64))
def test_without_bias_nothing_is_written_for_it(env, shape):
    L, dev = env
    B, H, W, C, N = shape
    form = (True, True)
    x, dy, sc, sh = WC.inputs(shape, form, "random")
    R, _, _ = run(env, shape, form, x, dy, sc, sh, bias=True)
    R0, none, scratch = run(env, shape, form, x, dy, sc, sh, bias=False)
    assert none is None
    assert torch.equal(R0[:, :, :C], R[:, :, :C])
    S = WC.launch_shape(L.lib, *shape)["S"]
    assert not torch.isnan(scratch[:S * 16 * C * N]).any()
    assert torch.isnan(scratch[S * 16 * C * N:S * 16 * C * N + S * N]).all()        # the bias column sums' part of the scratch


@shapes((2, 16, 16, 64, 192), (5, 16, 32, 256, 256))
def test_packed_row_length_equal_to_c(env, shape):
    C = shape[3]
    form = (True, True)
    x, dy, sc, sh = WC.inputs(shape, form, "random")
    R, bg, _ = run(env, shape, form, x, dy, sc, sh)
    Rc, bgc, _ = run(env, shape, form, x, dy, sc, sh, ld_extra=0)
    assert Rc.shape[2] == C and not torch.isnan(Rc).any()
    assert torch.equal(Rc, R[:, :, :C]) and torch.equal(bgc, bg)


@shapes(*(WC.ELIGIBLE + [(3, 32, 32, 192, 128)]))
def test_two_launches_write_the_same_bits(env, shape):
    """ordered sums over the split copies, no atomics: a second launch into the scratch the first one left behind gives the same bits"""
    C = shape[3]
    form = (True, True)
    x, dy, sc, sh = WC.inputs(shape, form, "random")
    R, bg, scratch = run(env, shape, form, x, dy, sc, sh)
    assert not torch.isnan(R[:, :, :C]).any() and not torch.isnan(bg).any()
    R2, bg2, _ = run(env, shape, form, x, dy, sc, sh, scratch=scratch)
    assert torch.equal(R2[:, :, :C], R[:, :, :C]) and torch.equal(bg2, bg)


@shapes((5, 16, 32, 256, 256), (9, 16, 16, 512, 512))
def test_each_image_counts_once(env, shape):
    """dy zeroed everywhere but image b: the launch must return image b's own gradient exactly, and the B of them must add up to the full
    reference -- a stage that is dropped or counted twice shows up at its place in the split ranges, not only as "wrong" """
    B = shape[0]
    form = (True, True)
    x, dy, sc, sh = WC.inputs(shape, form, "exact")
    gw, gb = WC.reference(shape, form, "exact")
    total, totalb = torch.zeros_like(gw), torch.zeros_like(gb)
    wrong = []
    for b in range(B):
        dyb = torch.zeros_like(dy)
        dyb[b] = dy[b]
        R, bg, _ = run(env, shape, form, x, dyb, sc, sh)
        got, gotb = weight_gradient(R, shape).double(), bg.cpu().double()
        own, ownb = WC.float64_gradient(x[b:b + 1], dy[b:b + 1], sc, sh, form[1])      # the other images' terms are exact zeros
        if not (torch.equal(got, own) and torch.equal(gotb, ownb)):
            wrong.append(b)
        total += got
        totalb += gotb
    assert not wrong, "images whose own gradient is wrong: %s" % wrong
    assert torch.equal(total, gw) and torch.equal(totalb, gb)
