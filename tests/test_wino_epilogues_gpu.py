"""GPU: every epilogue form of awr_wino_conv (csrc/awr_wino.hip) at every tile geometry, at operator level, against float64 torch on the CPU.

The kernel has three instantiations (32-channel tile with 2 or 3 raw-tile requests per thread, the 64-channel 1024-thread form) and multi-image
tiles (2, 4, 8, 16 images of 16x8 ... 4x4 maps) whose last tile is ragged when B % nimg != 0.  GEOMS reaches each of them with tiny shapes;
every form that can take the 64-channel tile runs with the process-wide code 4 (wide whenever N % 64 == 0) and 12 (never wide).

What every launch here is held to:
  * guard images -- every image-shaped tensor has at least B + 1 images (the whole of a ragged last tile) and the kernel is told B; the input
    images from B on are NaN, the output images from B on are NaN before the launch and must be NaN after it, and the statistics must be finite: a slot b >= B of a ragged tile that is stored, or that reaches a
    reduction, fails;
  * elementwise bar, no element exempt -- |got - ref| <= 2e-5 max|c| max(1, max|out_scale|) + 4 * 2^-24 max|ref| with c the float64 convolution
    (bias included); ReLU masks of the data-gradient forms are built away from zero (|argument| >= 1e-2, float32 evaluation with and without a
    fused multiply-add checked against the float64 sign before the launch), so the float32 and float64 masks are the same everywhere;
  * reduced sums against the values the kernel itself STORED, per slot copy -- copy s holds the tiles with tile % nslots == s (tile = the
    64-patch tile of a workgroup, all its channel tiles in one copy), to 1e-12 sum|term| (double sums, only the order differs); the
    BatchNorm-backward product sum g * xhat to 2^-22 sum|term| against float64 and to 1e-12 against the same three float32 roundings
    on the host; a NaN copy behind the last one stays NaN.
Further: both tile forms give the same bits; awr_wino_dgrad_or_direct is bit-identical to the hand-written awr_wino_args block or, for a block
the kernel does not implement, to awr_conv_gemm; awr_wino_dgrad_supported's truth table; awr_wino_weights writes its padding as zeros.

Every check prints its figure before it asserts (`wino-epi ratio <family> <check> <error / bar>`, `wino-epi forms ...`; run with -s).
"""
import ctypes as C
import fractions
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, H, W, C, N) in the KERNEL's terms (C = reduction channels, N = output channels)
GEOMS = [(18, 4, 4, 16, 64),      # nimg 16, three raw-tile requests per thread; ragged last tile of 2 images
         (5, 8, 8, 64, 64),       # nimg 4; ragged last tile of 1 image
         (3, 16, 8, 32, 96),      # nimg 2, ragged; three 32-channel tiles, never the 64 form; 6 workgroups: not a multiple of 8 (XCD remap)
         (3, 4, 8, 24, 64),       # nimg 8, ragged; 3 K stages
         (3, 8, 4, 24, 64),       # nimg 8, the other orientation
         (2, 16, 16, 64, 128),    # one image per tile
         (1, 16, 32, 8, 64),      # two tile rows per image; one K stage: no prefetch iteration
         (1, 4, 128, 16, 32)]     # 32 patch columns per tile, two tile columns
GEOM_IDS = ["%dx%dx%d_%dto%d" % g for g in GEOMS]
CODES = (4, 12)                   # awr_set_conv_winograd: 4 = the 64-channel form whenever N % 64 == 0, 12 = never
SLOTS = (1, 3, 16)
NAN = float("nan")
EPS24 = 2.0 ** -24


@pytest.fixture(scope="module")
def env():
    import awr_amd  # noqa: F401
    from awr_amd import _lib as L, ops
    return L, ops, torch.device("cuda:0")


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def pc(v):
    """per-channel vector -> broadcastable over (B, C, H, W)"""
    return v.view(1, -1, 1, 1)


def images_per_tile(H, W):
    PH, PW = H // 2, W // 2
    PCt = min(PW, 32)
    PRt = min(PH, 64 // PCt)
    return 64 // (PRt * PCt)


def guarded(B, H, W):
    """images to allocate for a batch of B: at least B + 1, and the whole of a ragged last tile -- a kernel that ignored b < B would still stay in bounds"""
    nimg = images_per_tile(H, W)
    return max(B + 1, (B + nimg - 1) // nimg * nimg)


def guard(t, dev):
    """(B, H, W, .) -> (guarded(B, H, W), H, W, .) on the device, the images behind the batch NaN"""
    B, H, W = t.shape[:3]
    return torch.cat([t, torch.full((guarded(B, H, W) - B,) + tuple(t.shape[1:]), NAN, dtype=t.dtype)]).contiguous().to(dev)


def away_from_zero(shape, g, margin):
    z = torch.randn(*shape, generator=g)
    return torch.where(z >= 0, z + margin, z - margin)


def tile_of_pixel(B, H, W):
    """(B, H, W) -> the 64-patch tile that owns each pixel: nimg images x PRt x PCt patches (awr_wino_conv's host code)"""
    PH, PW = H // 2, W // 2
    PCt = min(PW, 32)
    PRt = min(PH, 64 // PCt)
    nimg = 64 // (PRt * PCt)
    tiles_x, tiles_y = PW // PCt, PH // PRt
    b, y, x = torch.arange(B).view(B, 1, 1), torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    return ((b // nimg) * tiles_y + (y // 2) // PRt) * tiles_x + (x // 2) // PCt


def transform(L, dev, w, N, Cc, mirror):
    U = torch.full((16, Cc, N), NAN, device=dev)
    L.call("awr_wino_weights", L.ptr(w.to(dev).contiguous()), N, Cc, N, Cc, int(mirror), L.ptr(U), L.stream())
    return U


def run_wino(L, dev, code, x, U, N, bias=None, in_affine=None, relu_in=False, relu=False, out_affine=None, res=None, acc=None, bnr=None, nslots=0):
    """one awr_wino_conv launch; x, res, acc, bnr tensors: NHWC float32 on the CPU, B images (the guard images are added here).  acc: the initial
    content of `out` with res == out.  -> rc, out (with its guard images), stats (nslots + 1 copies) or None, res after the launch or None"""
    B, H, W, Cc = x.shape
    held = []

    def put(t):
        held.append(t.to(dev).contiguous())
        return L.ptr(held[-1])
    a = L.WinoArgs()
    xin = guard(x, dev)
    out = guard(acc, dev) if acc is not None else torch.full((guarded(B, H, W), H, W, N), NAN, device=dev)
    a.in_, a.U, a.out = L.ptr(xin), L.ptr(U), L.ptr(out)
    a.B, a.H, a.W, a.C, a.N, a.relu, a.relu_in = B, H, W, Cc, N, int(relu), int(relu_in)
    if bias is not None:
        a.bias = put(bias)
    if in_affine is not None:
        a.in_scale, a.in_shift = put(in_affine[0]), put(in_affine[1])
    if out_affine is not None:
        a.out_scale = put(out_affine[0])
        if out_affine[1] is not None:
            a.out_shift = put(out_affine[1])
    resd = st = None
    if res is not None:
        resd = guard(res, dev)
        a.res = L.ptr(resd)
    if acc is not None:
        a.res = L.ptr(out)
    if nslots:
        st = torch.zeros(nslots + 1, 2, N, device=dev, dtype=torch.float64)
        st[nslots] = NAN
        a.stats, a.nslots = L.ptr(st), nslots
    if bnr is not None:
        yd = guard(bnr[0], dev)
        a.bnr_y, a.bnr_coef = L.ptr(yd), put(bnr[1])
        if bnr[2] is not None:
            ad = guard(bnr[2], dev)
            a.bnr_act = L.ptr(ad)
    L.call("awr_set_conv_winograd", code)
    try:
        rc = L.lib.awr_wino_conv(C.byref(a), L.stream())
        torch.cuda.synchronize()
    finally:
        L.call("awr_set_conv_winograd", 0)
    return rc, out.cpu(), None if st is None else st.cpu(), None if resd is None else resd.cpu()


def check_guard(out, B, st=None, nslots=0):
    assert torch.isnan(out[B:]).all(), "an image behind the batch was stored"
    assert torch.isfinite(out[:B]).all()
    if st is not None:
        assert torch.isfinite(st[:nslots]).all(), "a slot outside the batch reached the reduction"
        assert torch.isnan(st[nslots]).all(), "the copy behind the last slot was touched"


def check_elementwise(family, got_nhwc, ref_nchw, c_nchw, osc_max=1.0):
    bar = 2e-5 * float(c_nchw.abs().max()) * max(1.0, osc_max) + 4 * EPS24 * float(ref_nchw.abs().max())
    err = float((nchw(got_nhwc).double() - ref_nchw).abs().max())
    print("wino-epi ratio %s elementwise %.4f" % (family, err / bar))
    assert err <= bar, (err, bar)


def check_sums(family, st, nslots, B, H, W, terms, rels):
    """st[s][k][n] against the float64 sums of terms[k] (B, H, W, N) over the tiles of copy s, and the sum over the copies against the whole sum"""
    N = terms[0].shape[-1]
    slot = (tile_of_pixel(B, H, W) % nslots).flatten()
    worst = 0.0
    for k, (t, rel) in enumerate(zip(terms, rels)):
        flat = t.reshape(-1, N)
        exp = torch.zeros(nslots, N, dtype=torch.float64).index_add_(0, slot, flat)
        mag = torch.zeros(nslots, N, dtype=torch.float64).index_add_(0, slot, flat.abs())
        d = (st[:nslots, k] - exp).abs()
        assert bool((d <= rel * mag).all()), ("slot copy", k, float((d - rel * mag).max()))
        dt = (st[:nslots, k].sum(0) - flat.sum(0)).abs()
        assert bool((dt <= rel * mag.sum(0)).all()), ("sum over the copies", k)
        worst = max(worst, float((dt / (rel * mag.sum(0)).clamp(min=1e-300)).max()))
    print("wino-epi ratio %s sums %.4f" % (family, worst))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. inference epilogue: out = [relu]((conv([relu](in * in_scale + in_shift)) + bias) * out_scale + out_shift [+ res]), res a separate tensor
# ---------------------------------------------------------------------------------------------------------------------------------------
INFER_FORMS = ["affine_relu",            # hourglass conv2 -> bn3 -> ReLU (model/hourglass.py:44-59)
               "affine_res_relu",        # BasicBlock (model/resnet_deconv.py:74-78)
               "affine_bias_res",
               "inaffine_affine"]


@functools.lru_cache(maxsize=None)
def infer_case(gi, fi):
    B, H, W, Cc, N = GEOMS[gi]
    form = INFER_FORMS[fi]
    g = torch.Generator().manual_seed(1000 + 10 * gi + fi)
    x = torch.randn(B, Cc, H, W, generator=g)
    w = torch.randn(N, Cc, 3, 3, generator=g) * (2.0 / (9 * Cc)) ** 0.5
    bias = torch.randn(N, generator=g) if form == "affine_bias_res" else None
    isc, ish = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    osc = (torch.rand(N, generator=g) + 0.5) * torch.where(torch.rand(N, generator=g) < 0.3, -1.0, 1.0)
    osc[0], osc[1] = -abs(osc[0]), abs(osc[1])
    osh = torch.randn(N, generator=g) * 0.3
    res = torch.randn(B, N, H, W, generator=g) if "res" in form else None
    relu = "relu" in form
    inaff = form == "inaffine_affine"
    xin = x.double()
    if inaff:
        xin = (xin * pc(isc.double()) + pc(ish.double())).clamp(min=0)
    c = torch.nn.functional.conv2d(xin, w.double(), None if bias is None else bias.double(), padding=1)
    ref = c * pc(osc.double()) + pc(osh.double())
    if res is not None:
        ref = ref + res.double()
    if relu:
        ref = ref.clamp(min=0)
    return dict(x=nhwc(x), w=w, bias=bias, in_affine=(isc, ish) if inaff else None, relu_in=inaff, relu=relu, out_affine=(osc, osh),
                res=None if res is None else nhwc(res), c=c, ref=ref, osc_max=float(osc.abs().max()))


_OUT = {}


def infer_run(env, gi, fi, code):
    key = ("infer", gi, fi, code)
    if key not in _OUT:
        L, ops, dev = env
        k = infer_case(gi, fi)
        N = GEOMS[gi][4]
        U = transform(L, dev, k["w"], N, GEOMS[gi][3], 0)
        rc, out, _, res = run_wino(L, dev, code, k["x"], U, N, bias=k["bias"], in_affine=k["in_affine"], relu_in=k["relu_in"], relu=k["relu"],
                                   out_affine=k["out_affine"], res=k["res"])
        assert rc == 0, L.last_error()
        _OUT[key] = (out, res)
    return _OUT[key]


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("fi", range(len(INFER_FORMS)), ids=INFER_FORMS)
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=GEOM_IDS)
def test_inference_epilogue(env, gi, fi, code):
    B = GEOMS[gi][0]
    k = infer_case(gi, fi)
    out, res = infer_run(env, gi, fi, code)
    check_guard(out, B)
    check_elementwise("infer", out[:B], k["ref"], k["c"], k["osc_max"])
    if k["res"] is not None:
        assert torch.equal(res[:B], k["res"]) and torch.isnan(res[B:]).all(), "res was written"


def test_inference_epilogue_exclusions_are_errors(env):
    """out_scale together with stats, and out_scale without out_shift: a negative code, `out` untouched"""
    L, ops, dev = env
    k = infer_case(1, 0)
    B, H, W, Cc, N = GEOMS[1]
    U = transform(L, dev, k["w"], N, Cc, 0)
    rc, out, st, _ = run_wino(L, dev, 12, k["x"], U, N, out_affine=k["out_affine"], nslots=3)
    assert rc < 0 and torch.isnan(out).all() and bool((st[:3] == 0).all())
    rc, out, _, _ = run_wino(L, dev, 12, k["x"], U, N, out_affine=(k["out_affine"][0], None))
    assert rc < 0 and torch.isnan(out).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. data-gradient epilogues: mirrored weights, the kernel's C = the layer's Cout, its N = the layer's Cin
# ---------------------------------------------------------------------------------------------------------------------------------------
DGRAD_FORMS = ["plain", "acc", "bnr", "acc_bnr", "acc_bnr_act"]


@functools.lru_cache(maxsize=None)
def dgrad_tensors(seed, B, H, W, Cc, N):
    """everything a data-gradient launch can take, and the float64 gradient.  The CPU-side mask conditions are asserted here, before any launch."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Cc, N, 3, 3, generator=g) * (2.0 / (9 * Cc)) ** 0.5          # the layer's weight: (Cout, Cin, 3, 3)
    dy = torch.randn(B, Cc, H, W, generator=g)
    x = torch.zeros(B, N, H, W, dtype=torch.float64, requires_grad=True)
    (dx,) = torch.autograd.grad((torch.nn.functional.conv2d(x, w.double(), padding=1) * dy.double()).sum(), x)
    r = torch.randn(B, N, H, W, generator=g)
    sc, sh = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.3
    mu, istd = torch.randn(N, generator=g) * 0.2, torch.rand(N, generator=g) + 0.5
    # re-derived mask: y * sc + sh = t with |t| >= 1.1e-2 before y is rounded to float32, >= 1e-2 after (asserted)
    t = away_from_zero((B, N, H, W), g, 1.1e-2)
    y = ((t.double() - pc(sh.double())) / pc(sc.double())).float()
    act = away_from_zero((B, N, H, W), g, 1e-2)
    m64 = y.double() * pc(sc.double()) + pc(sh.double())
    assert float(m64.abs().min()) >= 1e-2 and float(act.abs().min()) >= 1e-2
    m32 = y * pc(sc) + pc(sh)                    # two float32 roundings
    m32f = m64.float()                           # the product of two floats is exact in double: one rounding, a fused multiply-add's
    assert torch.equal(m32 > 0, m64 > 0) and torch.equal(m32f > 0, m64 > 0)
    return dict(w=w, dy=nhwc(dy), dx=dx, r=r, y=y, act=act, coef=torch.cat([sc, sh, mu, istd]).contiguous(), mu=mu, istd=istd, mask_y=m64 > 0, mask_act=act > 0)


def dgrad_expect(k, form):
    """-> (float64 reference (B, N, H, W), the mask or None)"""
    v = k["dx"] + (k["r"].double() if "acc" in form else 0)
    mask = None
    if "bnr" in form:
        mask = k["mask_act"] if "act" in form else k["mask_y"]
        v = v * mask
    return v, mask


def dgrad_args(k, form, nslots):
    return dict(acc=nhwc(k["r"]) if "acc" in form else None, bnr=(nhwc(k["y"]), k["coef"], nhwc(k["act"]) if "act" in form else None) if "bnr" in form else None,
                nslots=nslots if "bnr" in form else 0)


def check_dgrad(family, k, form, out, st, nslots, B, H, W):
    """the stored gradient and the two BatchNorm-backward sums of one data-gradient launch"""
    check_guard(out, B, st, nslots)
    v, mask = dgrad_expect(k, form)
    check_elementwise(family, out[:B], v, k["dx"])
    if mask is None:
        assert st is None
        return
    got = out[:B]
    assert bool((got[~nhwc(mask)] == 0).all()), "a masked-out element is not stored as exactly 0"
    y, mu, istd = nhwc(k["y"]), k["mu"], k["istd"]
    xhat64 = (y.double() - mu.double()) * istd.double()
    check_sums(family, st, nslots, B, H, W, (got.double(), got.double() * xhat64), (1e-12, 2.0 ** -22))
    # the same three float32 roundings on the host: xhat = (y - mean) * invstd, g * xhat -- then only the order of the double sums differs
    t32 = (got * ((y - mu) * istd)).double()
    assert bool((t32[~nhwc(mask)] == 0).all())
    check_sums(family + "-f32terms", st, nslots, B, H, W, (got.double(), t32), (1e-12, 1e-12))


def dgrad_run(env, gi, fi, code):
    key = ("dgrad", gi, fi, code)
    if key not in _OUT:
        L, ops, dev = env
        B, H, W, Cc, N = GEOMS[gi]
        k = dgrad_tensors(2000 + gi, B, H, W, Cc, N)
        nslots = SLOTS[(gi + fi + CODES.index(code)) % 3]
        U = transform(L, dev, k["w"], N, Cc, 1)
        rc, out, st, _ = run_wino(L, dev, code, k["dy"], U, N, **dgrad_args(k, DGRAD_FORMS[fi], nslots))
        assert rc == 0, L.last_error()
        _OUT[key] = (k, out, st, nslots)
    return _OUT[key]


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("fi", range(len(DGRAD_FORMS)), ids=DGRAD_FORMS)
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=GEOM_IDS)
def test_data_gradient_epilogues(env, gi, fi, code):
    B, H, W, Cc, N = GEOMS[gi]
    k, out, st, nslots = dgrad_run(env, gi, fi, code)
    check_dgrad("dgrad", k, DGRAD_FORMS[fi], out, st, nslots, B, H, W)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. forward statistics against the stored output
# ---------------------------------------------------------------------------------------------------------------------------------------
def forward_case(gi, relu, constant_channel=False):
    B, H, W, Cc, N = GEOMS[gi]
    g = torch.Generator().manual_seed(3000 + 10 * gi + int(relu))
    x = torch.randn(B, Cc, H, W, generator=g)
    w = torch.randn(N, Cc, 3, 3, generator=g) * (2.0 / (9 * Cc)) ** 0.5
    bias = torch.randn(N, generator=g)
    isc, ish = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    if constant_channel:      # channel 0: mean 100 (the bias), standard deviation about 1e-3 (the weights)
        xin = (x.double() * pc(isc.double()) + pc(ish.double())).clamp(min=0)
        w[0] *= 1e-3 / float(torch.nn.functional.conv2d(xin, w[:1].double(), padding=1).std())
        bias[0] = 100.0
    xin = (x.double() * pc(isc.double()) + pc(ish.double())).clamp(min=0)
    c = torch.nn.functional.conv2d(xin, w.double(), bias.double(), padding=1)
    return dict(x=nhwc(x), w=w, bias=bias, in_affine=(isc, ish), c=c, ref=c.clamp(min=0) if relu else c)


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=GEOM_IDS)
def test_forward_statistics_are_the_sums_of_the_stored_output(env, gi, relu, code):
    L, ops, dev = env
    B, H, W, Cc, N = GEOMS[gi]
    k = forward_case(gi, relu)
    nslots = SLOTS[(gi + int(relu) + CODES.index(code)) % 3]
    U = transform(L, dev, k["w"], N, Cc, 0)
    rc, out, st, _ = run_wino(L, dev, code, k["x"], U, N, bias=k["bias"], in_affine=k["in_affine"], relu_in=True, relu=relu, nslots=nslots)
    assert rc == 0, L.last_error()
    check_guard(out, B, st, nslots)
    check_elementwise("fwdstats", out[:B], k["ref"], k["c"])
    o = out[:B].double()
    check_sums("fwdstats", st, nslots, B, H, W, (o, o * o), (1e-12, 1e-12))


@pytest.mark.parametrize("code", CODES)
def test_forward_statistics_keep_the_variance_of_a_nearly_constant_channel(env, code):
    """Channel 0 has mean 100 and standard deviation 1e-3: (std / mean)^2 = 1e-10, so sum x^2 taken in float32 has no variance left; the kernel
    squares and adds in double.  The variance recovered from the two sums equals that of the stored values to 1e-6 relative.  1e-6 * 1e-10 is
    float64's own resolution, so both variances are evaluated in exact rational arithmetic (from the float64 sums as they are / from the
    float32 values) -- what is compared is the kernel's sums, not this test's arithmetic.  Shape: the one of GEOMS with the fewest pixels per
    channel (96).  Stored values near 100 are multiples of 2^-17, their squares of 2^-34: a double holds such a sum exactly up to 2^19, i.e.
    52 values; with 96 the last additions of the kernel drop one bit (at most 2^-34 each, about 6e-7 of the variance per pixel count)."""
    L, ops, dev = env
    gi = 3
    B, H, W, Cc, N = GEOMS[gi]
    k = forward_case(gi, False, constant_channel=True)
    U = transform(L, dev, k["w"], N, Cc, 0)
    rc, out, st, _ = run_wino(L, dev, code, k["x"], U, N, bias=k["bias"], in_affine=k["in_affine"], relu_in=True, nslots=3)
    assert rc == 0, L.last_error()
    check_guard(out, B, st, 3)
    check_elementwise("fwdstats-const", out[:B], k["ref"], k["c"])
    o = out[:B].double()
    check_sums("fwdstats-const", st, 3, B, H, W, (o, o * o), (1e-12, 1e-12))
    vals = [fractions.Fraction(float(v)) for v in out[:B, :, :, 0].flatten()]
    n = len(vals)
    var_stored = sum(v * v for v in vals) / n - (sum(vals) / n) ** 2
    assert 0.25e-6 < float(var_stored) < 4e-6 and abs(float(sum(vals) / n) - 100) < 1e-2
    s1 = sum(fractions.Fraction(float(st[s, 0, 0])) for s in range(3))
    s2 = sum(fractions.Fraction(float(st[s, 1, 0])) for s in range(3))
    var_sums = s2 / n - (s1 / n) ** 2
    rel = float(abs(var_sums - var_stored) / var_stored)
    print("wino-epi ratio fwdstats-const variance %.4f" % (rel / 1e-6))
    assert rel <= 1e-6, rel


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. both tile forms agree
# ---------------------------------------------------------------------------------------------------------------------------------------
WIDE = [gi for gi, g in enumerate(GEOMS) if g[4] % 64 == 0]


@pytest.mark.parametrize("family,fi", [("infer", i) for i in range(len(INFER_FORMS))] + [("dgrad", i) for i in range(len(DGRAD_FORMS))],
                         ids=["infer-" + f for f in INFER_FORMS] + ["dgrad-" + f for f in DGRAD_FORMS])
@pytest.mark.parametrize("gi", WIDE, ids=[GEOM_IDS[i] for i in WIDE])
def test_both_tile_forms_agree(env, gi, family, fi):
    """The 64-channel form and the 32-channel form run the same k order per output element and the same epilogue arithmetic: BIT_IDENTICAL"""
    if family == "infer":
        a, b = infer_run(env, gi, fi, 4)[0], infer_run(env, gi, fi, 12)[0]
    else:
        a, b = dgrad_run(env, gi, fi, 4)[1], dgrad_run(env, gi, fi, 12)[1]
    B = GEOMS[gi][0]
    d = float((a[:B].double() - b[:B].double()).abs().max())
    print("wino-epi forms %s max difference %.3e" % (family, d))
    assert torch.equal(a[:B], b[:B]), d


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. awr_wino_dgrad_or_direct / awr_wino_dgrad_supported
# ---------------------------------------------------------------------------------------------------------------------------------------
DISPATCH_SHAPES = [(5, 8, 8, 64, 64), (3, 16, 8, 96, 32)]             # (B, H, W, layer Cin, layer Cout)
DISPATCH_IDS = ["%dx%dx%d_%dto%d" % s for s in DISPATCH_SHAPES]
SUPPORTED = ["plain", "acc", "bnr", "bnr_act"]
UNSUPPORTED = ["relu_out", "bias", "in_affine", "res_other", "stats_only"]


class Dispatch:
    """the data-gradient problem of one 3x3 stride-1 pad-1 layer on the device: fresh argument blocks (and fresh output / statistics buffers) on demand"""

    def __init__(self, env, shape, seed):
        L, ops, dev = env
        self.L, self.ops, self.dev = L, ops, dev
        self.B, self.H, self.W, self.cin, self.cout = shape
        B, H, W, cin, cout = shape
        self.k = k = dgrad_tensors(seed, B, H, W, cout, cin)
        self.spec = ops.ConvSpec("conv", cin, cout, 3, 1, 1)
        self.prob = self.spec.dgrad_problem(H, W)
        wd = k["w"].to(dev).contiguous()
        self.wp = ops.pack_weight(wd, self.spec.dgrad_pack())
        self.U = transform(L, dev, k["w"], cin, cout, 1)
        g = torch.Generator().manual_seed(seed + 1)
        self.din = guard(k["dy"], dev)
        self.y, self.act, self.coef = guard(nhwc(k["y"]), dev), guard(nhwc(k["act"]), dev), k["coef"].to(dev)
        self.other = guard(nhwc(torch.randn(B, cin, H, W, generator=g)), dev)
        self.bias = torch.randn(cin, generator=g).to(dev)
        self.isc, self.ish = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.randn(cout, generator=g) * 0.3).to(dev)

    def buffers(self, form, nslots):
        out = guard(nhwc(self.k["r"]), self.dev) if form == "acc" else torch.full((guarded(self.B, self.H, self.W), self.H, self.W, self.cin), NAN, device=self.dev)
        st = None
        if form in ("bnr", "bnr_act", "stats_only"):
            st = torch.zeros(nslots + 1, 2, self.cin, device=self.dev, dtype=torch.float64)
            st[nslots] = NAN
        return out, st

    def conv_args(self, form, out, st, stat_slots=0):
        kw = {}
        if form == "acc":
            kw["res"] = out
        if form == "res_other":
            kw["res"] = self.other
        if form == "bias":
            kw["bias"] = self.bias
        if form == "in_affine":
            kw["in_scale"], kw["in_shift"] = self.isc, self.ish
        a = self.ops.make_conv_args(self.prob, self.B, self.din, self.wp, out, T=self.spec.T, stats=st, relu_out=form == "relu_out", **kw)
        a.stat_slots = stat_slots
        if form in ("bnr", "bnr_act"):
            a.bnr_y, a.bnr_coef = self.L.ptr(self.y), self.L.ptr(self.coef)
        if form == "bnr_act":
            a.bnr_act = self.L.ptr(self.act)
        return a

    def wino_args(self, form, out, st, nslots):
        L = self.L
        a = L.WinoArgs()
        a.in_, a.U, a.out = L.ptr(self.din), L.ptr(self.U), L.ptr(out)
        a.B, a.H, a.W, a.C, a.N = self.B, self.H, self.W, self.cout, self.cin
        if form == "acc":
            a.res = L.ptr(out)
        if form in ("bnr", "bnr_act"):
            a.bnr_y, a.bnr_coef, a.stats, a.nslots = L.ptr(self.y), L.ptr(self.coef), L.ptr(st), nslots
        if form == "bnr_act":
            a.bnr_act = L.ptr(self.act)
        return a

    def dispatch(self, form, stat_slots=0):
        nslots = stat_slots or 16
        out, st = self.buffers(form, nslots)
        a = self.conv_args(form, out, st, stat_slots)
        self.L.call("awr_wino_dgrad_or_direct", C.byref(a), self.L.ptr(self.U), self.L.stream())
        torch.cuda.synchronize()
        return a, out.cpu(), None if st is None else st.cpu()

    def same(self, got, want, nslots):
        (out, st), (out2, st2) = got, want
        assert torch.equal(out[:self.B], out2[:self.B]) and torch.isnan(out[self.B:]).all() and torch.isnan(out2[self.B:]).all()
        assert (st is None) == (st2 is None)
        if st is not None:
            assert torch.equal(st[:nslots], st2[:nslots]) and torch.isnan(st[nslots]).all() and torch.isnan(st2[nslots]).all()


@functools.lru_cache(maxsize=None)
def _dispatch(env, si):
    shapes = DISPATCH_SHAPES + [(17, 16, 16, 32, 32)]      # the last: 17 one-image tiles -- more tiles than AWR_STAT_SLOTS copies
    return Dispatch(env, shapes[si], 5000 + si)


@pytest.mark.parametrize("form", SUPPORTED)
@pytest.mark.parametrize("si", range(len(DISPATCH_SHAPES)), ids=DISPATCH_IDS)
def test_dispatcher_runs_supported_blocks_as_winograd(env, si, form):
    """bit-identical to awr_wino_conv with the hand-written awr_wino_args block, and within the elementwise bar of float64"""
    L, ops, dev = env
    D = _dispatch(env, si)
    a, out, st = D.dispatch(form)
    assert L.lib.awr_wino_dgrad_supported(C.byref(a)) == 1
    out2, st2 = D.buffers(form, 16)
    L.call("awr_wino_conv", C.byref(D.wino_args(form, out2, st2, 16)), L.stream())
    torch.cuda.synchronize()
    D.same((out, st), (out2.cpu(), None if st2 is None else st2.cpu()), 16)
    check_dgrad("dispatch", D.k, form, out, st, 16, D.B, D.H, D.W)


@pytest.mark.parametrize("stat_slots", [0, 3])
@pytest.mark.parametrize("si", range(len(DISPATCH_SHAPES) + 1), ids=DISPATCH_IDS + ["17x16x16_32to32"])
def test_dispatcher_stat_slots(env, si, stat_slots):
    """stat_slots = 0: exactly AWR_STAT_SLOTS = 16 copies (copy 16, NaN, survives; with 17 tiles copy 0 holds tiles 0 and 16); 3: three"""
    L, ops, dev = env
    D = _dispatch(env, si)
    nslots = stat_slots or 16
    a, out, st = D.dispatch("bnr", stat_slots)
    out2, st2 = D.buffers("bnr", nslots)
    L.call("awr_wino_conv", C.byref(D.wino_args("bnr", out2, st2, nslots)), L.stream())
    torch.cuda.synchronize()
    D.same((out, st), (out2.cpu(), st2.cpu()), nslots)
    check_dgrad("dispatch", D.k, "bnr", out, st, nslots, D.B, D.H, D.W)


@pytest.mark.parametrize("form", UNSUPPORTED)
@pytest.mark.parametrize("si", range(len(DISPATCH_SHAPES)), ids=DISPATCH_IDS)
def test_dispatcher_falls_back_to_the_direct_kernel(env, si, form):
    """a block the Winograd kernel does not implement: bit for bit what awr_conv_gemm gives for the same block"""
    L, ops, dev = env
    D = _dispatch(env, si)
    a, out, st = D.dispatch(form)
    assert L.lib.awr_wino_dgrad_supported(C.byref(a)) == 0
    out2, st2 = D.buffers(form, 16)
    L.call("awr_conv_gemm", C.byref(D.conv_args(form, out2, st2)), L.stream())
    torch.cuda.synchronize()
    D.same((out, st), (out2.cpu(), None if st2 is None else st2.cpu()), 16)
    assert torch.isfinite(out[:D.B]).all()


def test_dgrad_supported_truth_table(env):
    L, ops, dev = env
    P, Q = 0x1000, 0x2000      # never dereferenced: a pure host function
    sup = L.lib.awr_wino_dgrad_supported

    def block(**kw):
        a = L.ConvArgs()
        a.in_, a.w, a.out = P, P, P
        for f, v in kw.items():
            setattr(a, f, v)
        return sup(C.byref(a))
    assert sup(None) == 0
    assert block() == 1
    assert block(res=P) == 1
    assert block(bnr_y=Q, bnr_coef=Q, stats=Q) == 1
    assert block(bnr_y=Q, bnr_coef=Q, stats=Q, bnr_act=Q) == 1
    assert block(res=P, bnr_y=Q, bnr_coef=Q, stats=Q, bnr_act=Q) == 1
    for f in ("in_scale", "bias", "out_scale", "in2", "w2", "partial", "in_bnb_y", "bnr2_y", "in_split", "pool_out"):
        assert block(**{f: Q}) == 0, f
        assert block(bnr_y=Q, bnr_coef=Q, stats=Q, **{f: Q}) == 0, f
    for f in ("relu_in", "relu_out"):
        assert block(**{f: 1}) == 0, f
    assert block(res=Q) == 0
    assert block(bnr_y=Q, stats=Q) == 0
    assert block(bnr_y=Q, bnr_coef=Q) == 0
    assert block(stats=Q) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. awr_wino_weights: padding rows and columns are written as zeros
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", [0, 1])
def test_weight_transform_writes_its_padding(env, mirror):
    L, ops, dev = env
    N, Npad, Cc, Cpad = 40, 64, 20, 24
    g = torch.Generator().manual_seed(60 + mirror)
    w = torch.randn(*((Cc, N) if mirror else (N, Cc)), 3, 3, generator=g) * (2.0 / (9 * Cc)) ** 0.5
    U = torch.full((16, Cpad, Npad), NAN, device=dev)
    L.call("awr_wino_weights", L.ptr(w.to(dev).contiguous()), N, Cc, Npad, Cpad, mirror, L.ptr(U), L.stream())
    torch.cuda.synchronize()
    got = U.cpu()
    assert torch.isfinite(got).all(), "an entry of U was not written"
    assert bool((got[:, Cc:, :] == 0).all()) and bool((got[:, :, N:] == 0).all())
    gk = (w.flip(2, 3).permute(1, 0, 2, 3) if mirror else w).double()             # (N, C, 3, 3): the taps the forward form of the launch sees
    G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)
    ref = torch.einsum("ia,ncab,jb->ijcn", G, gk, G).reshape(16, Cc, N)
    err = float((got[:, :Cc, :N].double() - ref).abs().max())
    bar = 4 * EPS24 * float(w.abs().max())
    print("wino-epi ratio weights transform %.4f" % (err / bar))
    assert err <= bar, (err, bar)
    # a forward through this U: finite garbage in the input's padding channels meets zero rows, the padding output channels are exact zeros
    B, H, W = 3, 8, 8
    x = torch.randn(B, Cc, H, W, generator=g)
    c = torch.nn.functional.conv2d(x.double(), gk, padding=1)
    xp = torch.cat([nhwc(x), away_from_zero((B, H, W, Cpad - Cc), g, 1.0) * 1e3], dim=3).contiguous()
    for code in CODES:
        rc, out, _, _ = run_wino(L, dev, code, xp, U, Npad, bias=torch.zeros(Npad))
        assert rc == 0, L.last_error()
        check_guard(out, B)
        check_elementwise("weights", out[:B, :, :, :N], c, c)
        assert bool((out[:B, :, :, N:] == 0).all())
