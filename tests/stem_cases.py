"""Inputs, float64 references and check bodies of the fused stem kernels (csrc/awr_stem.hip), shared by tests/test_stem_cases_cpu.py (the
references themselves) and tests/test_stem_gpu.py (the kernels).  A plain helper module like conv_cases.py, not a conftest: a check body takes
the `_lib` module and the device, runs the kernels through the C ABI and returns the figures it measured ({name: value}); the caller prints
them and asserts them (`assert_figures`).

The stem never stores the tensor it computes, so every reference here is the chain of separate operators in float64 torch on the CPU:
conv2d (5x5, pad 2, 1 -> 64) -> batch_norm (batch statistics) -> relu -> [max_pool2d(3, 2, 1)], and autograd through it.

Shapes (B, H, W), their 16x16-tile counts and the tiles a workgroup walks (stats and BN-backward sums: the largest power of two <= 4 that
divides the count; weight gradient: <= 8):

    (1, 16, 48)  3 tiles  1 / 1   one tile high          (2, 16, 32)  2 tiles  2 / 2   one tile high
    (2, 48, 16)  3 tiles  1 / 1   one tile wide, tall    (5, 32, 32)  4 tiles  4 / 4   odd batch
    (1, 48, 48)  9 tiles  1 / 1   odd count > 1          (2, 64, 64) 16 tiles  4 / 8
    (3, 48, 32)  6 tiles  2 / 2   tall

The deterministic slot counts tiles * B (3, 6, 9, 18, 4, 20, 32) lie on both sides of the default 16.
"""
import functools
import types

import torch
import torch.nn.functional as TF

from conv_cases import rel_err, rnd

SHAPES = [(1, 16, 48), (2, 48, 16), (1, 48, 48), (3, 48, 32), (2, 16, 32), (5, 32, 32), (2, 64, 64)]
TILE_COUNTS = [3, 3, 9, 6, 2, 4, 16]
# No shape above launches more than 9 workgroups per channel half (slot index = group + image * groups), so `slot % 16` never wraps there and
# a kernel that took the slot modulo the default 16 instead of nslots would fill deterministic slots just as well.  The slot tests add this
# one: 9 tiles, one per workgroup, 45 workgroups.
WRAP_SHAPE = (5, 48, 48)
SLOT_SHAPES = SHAPES + [WRAP_SHAPE]
DEFAULT_SLOTS = 16          # AWR_STAT_SLOTS: what nslots = 0 means
GUARD_SLOTS = 16            # copies behind the ones a launch may use: must come back untouched
SENTINEL = -3.5             # their fill (finite: a stray atomic add onto it shows)
WG_TILES = (1, 2, 4, 8)     # tiles one workgroup may walk

# the bounds of test_fused_stem_matches_conv_bn_relu_maxpool / test_fused_stem_dense_matches_conv_bias_bn_relu (tests/test_ops_gpu.py)
BOUNDS = dict(mean=2e-6, var=2e-5, map=5e-6, pre=5e-6, dgamma=2e-5, dbeta=2e-5, dW=5e-5, dW_again=5e-5, dbias=2e-5)
# figures that must be exactly zero: max |accumulator| after its finalize (re-armed), 1 - (guard copies untouched), argmax bytes above 8, ...
EXACT = ("stats_rearmed", "sums_rearmed", "dw_rearmed", "guard", "argmax_range", "eval_differs")


def shape_id(s):
    return "x".join(str(i) for i in s)


def tiles_of(H, W):
    return (H // 16) * (W // 16)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def make_inputs(pooled, B, H, W, kind="random"):
    """img with a constant top third (the background of the real crops: exact ties in every window there), the 64 filters, a conv bias for the
    dense (Hourglass) form, BatchNorm gamma / beta and the gradient of the stem's output.
    kind "random": gamma in [0.5, 1.5] (the existing tests' inputs); "alt": the same with another seed;
    "ties": gamma = [0, -g, g, 0, ...] and beta = [+, ., ., -, ...]: channels 0 mod 4 are the constant beta > 0 (every window is an exact tie and
    the gradient passes the ReLU), channels 3 mod 4 the constant beta < 0 (tie, masked), channels 1 mod 4 have a negative scale."""
    g = torch.Generator().manual_seed((5 if pooled else 11) + 7 * H + 3 * W + B + (100 if kind == "alt" else 0))
    img = torch.rand(B, 1, H, W, generator=g) * 2 - 1
    img[:, :, : H // 3] = 1.0
    w = torch.randn(64, 1, 5, 5, generator=g) * 0.2
    bias = None if pooled else torch.randn(64, generator=g) * 0.5
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3
    if kind == "ties":
        c = torch.arange(64) % 4
        gamma = torch.where((c == 0) | (c == 3), torch.zeros(64), torch.where(c == 1, -gamma, gamma))
        beta = torch.where(c == 0, beta.abs() + 0.1, torch.where(c == 3, -beta.abs() - 0.1, beta))
    Ho, Wo = (H // 2, W // 2) if pooled else (H, W)
    gout = rnd(B, 64, Ho, Wo, seed=3 if pooled else 4)
    return types.SimpleNamespace(pooled=pooled, B=B, H=H, W=W, kind=kind, img=img, w=w, bias=bias, gamma=gamma, beta=beta, gout=gout)


def evaluate(inp, dtype):
    """The separate operators and autograd in `dtype` on the CPU.  gz is the gradient that reaches the BatchNorm output (routed by the pooling,
    masked by the ReLU): its sum over the pixels is the bias column of the weight gradient under identity coefficients."""
    img = inp.img.to(dtype)
    w = inp.w.to(dtype).clone().requires_grad_(True)            # (clone: .to() of a float32 tensor is the tensor itself)
    gamma, beta = inp.gamma.to(dtype).clone().requires_grad_(True), inp.beta.to(dtype).clone().requires_grad_(True)
    bias = None if inp.bias is None else inp.bias.to(dtype)
    y = TF.conv2d(img, w, bias, 1, 2)
    z = TF.batch_norm(y, None, None, gamma, beta, True, 0.1, 1e-5)
    a = TF.relu(z)
    idx = None
    if inp.pooled:
        out, idx = TF.max_pool2d(a, 3, 2, 1, return_indices=True)
    else:
        out = a
    gw, gg, gb, gz = torch.autograd.grad(out, (w, gamma, beta, z), inp.gout.to(dtype))
    mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    return types.SimpleNamespace(y=y.detach(), pre=z.detach(), map=out.detach(), idx=idx, mean=mean.detach(), var=var.detach(), dW=gw, dgamma=gg,
                                 dbeta=gb, gz=gz, dbias=gz.sum((0, 2, 3)))


F32_FIGURES = ("mean", "var", "map", "pre", "dgamma", "dbeta", "dW", "dbias")


@functools.lru_cache(maxsize=None)
def reference(pooled, B, H, W, kind="random"):
    """Inputs, their float64 results and the error of float32 torch against those (the yardstick of a bound that has to be measured): computed
    once per case and shared by every test that needs it (read-only: nothing writes into these tensors)."""
    inp = make_inputs(pooled, B, H, W, kind)
    inp.r64 = evaluate(inp, torch.float64)
    r32 = evaluate(inp, torch.float32)
    inp.e32 = {k: rel_err(getattr(r32, k), getattr(inp.r64, k)) for k in F32_FIGURES}
    return inp


# ---- the argmax code of the pooling kernel -----------------------------------------------------------------------------------------------------
def window_code(idx, H, W):
    """Flat indices of max_pool2d(3, 2, 1, return_indices=True) on an H x W map (any leading dimensions, the last two the pooled map) -> the
    kernel's code dy * 3 + dx of the winning element inside its window, whose top-left element is (2 oy - 1, 2 ox - 1)."""
    Ho, Wo = idx.shape[-2:]
    oy = torch.arange(Ho, dtype=idx.dtype).view(Ho, 1)
    ox = torch.arange(Wo, dtype=idx.dtype).view(1, Wo)
    dy = torch.div(idx, W, rounding_mode="floor") - (2 * oy - 1)
    dx = idx % W - (2 * ox - 1)
    assert bool(((dy >= 0) & (dy < 3) & (dx >= 0) & (dx < 3)).all()), "index outside its window"
    return (dy * 3 + dx).to(torch.uint8)


def constant_map_codes(Ho, Wo):
    """The codes of a map whose every window is an exact tie: the first element in scan order that lies inside the map."""
    code = torch.zeros(Ho, Wo, dtype=torch.uint8)
    code[0, :] = 3
    code[:, 0] = 1
    code[0, 0] = 4
    return code


# ---- per-tile sums ------------------------------------------------------------------------------------------------------------------------------
def tile_sums(x):
    """(B, C, H, W) -> (B, tiles, C): the sum over each 16x16 tile, tiles in row-major order (the order the workgroups walk them)."""
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 16, 16, W // 16, 16).sum((3, 5)).reshape(B, C, -1).permute(0, 2, 1).contiguous()


def group_tiles(ts, t):
    """(B, tiles, C) -> (B * tiles / t, C): sums over t consecutive tiles of one image, in slot order (image-major)."""
    B, tiles, C = ts.shape
    return ts.reshape(B, tiles // t, t, C).sum(2).reshape(B * (tiles // t), C)


def used_prefix(raw):
    """raw[slot][2][64] -> n if exactly the slots [0, n) hold a non-zero entry, else -1."""
    used = (raw != 0).flatten(1).any(1)
    n = int(used.sum())
    return n if bool(used[:n].all()) else -1


# ---- device side --------------------------------------------------------------------------------------------------------------------------------
class Device:
    """The inputs of one case on the device, and the stem launches on them."""

    def __init__(self, L, dev, inp):
        self.L, self.dev, self.inp = L, dev, inp
        self.B, self.H, self.W = inp.B, inp.H, inp.W
        self.n = inp.B * inp.H * inp.W
        self.img, self.w = inp.img.to(dev).contiguous(), inp.w.to(dev).contiguous()
        self.bias = None if inp.bias is None else inp.bias.to(dev)
        self.gamma, self.beta = inp.gamma.to(dev), inp.beta.to(dev)
        self.dg = nhwc(inp.gout).to(dev)
        self.ident = torch.zeros(3, 64, device=dev)
        self.ident[2] = 1.0

    def slots(self):
        import ctypes as C
        ss, ws = C.c_int(-1), C.c_int(-1)
        self.L.call("awr_stem_slots", self.B, self.H, self.W, C.byref(ss), C.byref(ws))
        return ss.value, ws.value

    def buffer(self, nslots, per, dtype):
        """nslots (0 = the default 16) zeroed copies of `per` elements and GUARD_SLOTS sentinel copies behind them"""
        n = nslots or DEFAULT_SLOTS
        buf = torch.full(((n + GUARD_SLOTS) * per,), SENTINEL, dtype=dtype, device=self.dev)
        buf[: n * per] = 0
        return buf

    @staticmethod
    def used(buf, nslots, per):
        return buf[: (nslots or DEFAULT_SLOTS) * per]

    @staticmethod
    def guard_touched(buf, nslots, per):
        return float((buf[(nslots or DEFAULT_SLOTS) * per:] != SENTINEL).any())

    def stats(self, buf, nslots):
        L = self.L
        L.call("awr_stem_stats", L.ptr(self.img), L.ptr(self.w), L.ptr(self.bias), self.B, self.H, self.W, L.ptr(buf), nslots, L.stream())

    def bn_finalize(self, buf, nslots):
        """coef4 = scale, shift, mean, invstd; re-arms the slots it read"""
        L = self.L
        coef4 = torch.zeros(4, 64, device=self.dev)
        rm, rv = torch.zeros(64, device=self.dev), torch.ones(64, device=self.dev)
        L.call("awr_bn_finalize", L.ptr(buf), 64, self.n, L.ptr(self.gamma), L.ptr(self.beta), L.ptr(rm), L.ptr(rv), 0.1, 1e-5, L.ptr(coef4[0]),
               L.ptr(coef4[1]), L.ptr(coef4[2]), L.ptr(coef4[3]), nslots, L.stream())
        return coef4

    def pool(self, scale, shift, with_argmax=True):
        L = self.L
        pooled = torch.empty(self.B, self.H // 2, self.W // 2, 64, device=self.dev)
        arg = torch.full((self.B, self.H // 2, self.W // 2, 64), 255, device=self.dev, dtype=torch.uint8) if with_argmax else None
        L.call("awr_stem_pool", L.ptr(self.img), L.ptr(self.w), L.ptr(scale), L.ptr(shift), self.B, self.H, self.W, L.ptr(pooled), L.ptr(arg), L.stream())
        return pooled, arg

    def conv(self, scale, shift, relu, bias="own"):
        L = self.L
        out = torch.empty(self.B, self.H, self.W, 64, device=self.dev)
        L.call("awr_stem_conv", L.ptr(self.img), L.ptr(self.w), L.ptr(self.bias if bias == "own" else bias), L.ptr(scale), L.ptr(shift), relu, self.B,
               self.H, self.W, L.ptr(out), L.stream())
        return out

    def bwd_reduce(self, coef4, arg, buf, nslots):
        L = self.L
        L.call("awr_stem_bwd_reduce", L.ptr(self.img), L.ptr(self.w), L.ptr(self.bias), L.ptr(coef4), L.ptr(self.dg), L.ptr(arg), self.B, self.H, self.W,
               L.ptr(buf), nslots, L.stream())

    def bn_bwd_finalize(self, buf, coef4, nslots):
        L = self.L
        coef = torch.zeros(3, 64, device=self.dev)
        dgam, dbet = torch.zeros(64, device=self.dev), torch.zeros(64, device=self.dev)
        L.call("awr_bn_bwd_finalize", L.ptr(buf), 64, self.n, L.ptr(self.gamma), L.ptr(coef4[3]), L.ptr(coef), L.ptr(dgam), L.ptr(dbet), 0, nslots, L.stream())
        return coef, dgam, dbet

    def bwd_wgrad(self, coef4, coef, arg, buf, nslots):
        L = self.L
        gw, gbias = torch.full((64, 1, 5, 5), 7.0, device=self.dev), torch.full((64,), 7.0, device=self.dev)
        L.call("awr_stem_bwd_wgrad", L.ptr(self.img), L.ptr(self.w), L.ptr(self.bias), L.ptr(coef4), L.ptr(coef), L.ptr(self.dg), L.ptr(arg), self.B,
               self.H, self.W, L.ptr(buf), L.ptr(gw), L.ptr(gbias), nslots, L.stream())
        return gw, gbias


# ---- check bodies -------------------------------------------------------------------------------------------------------------------------------
def stem_chain(L, dev, inp, nslots=0):
    """Test 1 / 3 / 4: statistics -> BatchNorm coefficients -> pooled or dense map -> BN-backward sums -> weight gradient (twice: the first call
    re-arms the slots) -> bias column under identity coefficients, every accumulator with exactly `nslots` copies (0: the default 16) and a
    guard behind them.  Relative errors against float64; what must be exactly zero is a figure too (EXACT)."""
    d, r = Device(L, dev, inp), inp.r64
    f = {}
    stats = d.buffer(nslots, 128, torch.float64)
    d.stats(stats, nslots)
    st = d.used(stats, nslots, 128).view(-1, 2, 64).sum(0).cpu()
    f["mean"] = rel_err(st[0] / d.n, r.mean)
    f["var"] = rel_err(st[1] / d.n - (st[0] / d.n) ** 2, r.var)
    coef4 = d.bn_finalize(stats, nslots)
    f["stats_rearmed"] = float(d.used(stats, nslots, 128).abs().max())
    guard = d.guard_touched(stats, nslots, 128)
    arg = None
    if inp.pooled:
        pooled, arg = d.pool(coef4[0], coef4[1])
        f["map"] = rel_err(nchw(pooled).cpu(), r.map)
        f["argmax_range"] = float(int(arg.max()) > 8)
        pooled2, _ = d.pool(coef4[0], coef4[1], with_argmax=False)        # eval-mode use: no argmax
        f["eval_differs"] = float(not torch.equal(pooled, pooled2))
    else:
        f["map"] = rel_err(nchw(d.conv(coef4[0], coef4[1], 1)).cpu(), r.map)
        f["pre"] = rel_err(nchw(d.conv(coef4[0], coef4[1], 0)).cpu(), r.pre)
    sums = d.buffer(nslots, 128, torch.float64)
    d.bwd_reduce(coef4, arg, sums, nslots)
    coef, dgam, dbet = d.bn_bwd_finalize(sums, coef4, nslots)
    f["dgamma"], f["dbeta"] = rel_err(dgam.cpu(), r.dgamma), rel_err(dbet.cpu(), r.dbeta)
    f["sums_rearmed"] = float(d.used(sums, nslots, 128).abs().max())
    guard += d.guard_touched(sums, nslots, 128)
    dw = d.buffer(nslots, 64 * 26, torch.float32)
    gw, gbias = d.bwd_wgrad(coef4, coef, arg, dw, nslots)
    f["dW"] = rel_err(gw.cpu(), r.dW)
    gw, gbias = d.bwd_wgrad(coef4, coef, arg, dw, nslots)
    f["dW_again"] = rel_err(gw.cpu(), r.dW)
    # a bias in front of a BatchNorm has a zero gradient in exact arithmetic: what is left is the rounding noise of a sum of n terms
    f["dbias_bn_noise"] = float(gbias.abs().max()) / (1e-6 * d.n * float(inp.gout.abs().mean()))
    gw, gbias = d.bwd_wgrad(coef4, d.ident, arg, dw, nslots)             # identity as "BatchNorm backward": column 25 = sum of relu' * g
    f["dbias"] = rel_err(gbias.cpu(), r.dbias)
    f["dw_rearmed"] = float(d.used(dw, nslots, 64 * 26).abs().max())
    f["guard"] = guard + d.guard_touched(dw, nslots, 64 * 26)
    return f


def assert_figures(f, bounds=BOUNDS):
    for k, v in f.items():
        if k in EXACT:
            assert v == 0.0, (k, v)
        elif k in bounds:
            assert v < bounds[k], (k, v, bounds[k])
    if "dbias_bn_noise" in f:
        assert f["dbias_bn_noise"] < 1.0, f["dbias_bn_noise"]


def pool_scale_shift(B, H, W):
    """Test 2: folded coefficients of both signs; channels 0-7 scale = 0, shift > 0 (the whole window ties above the ReLU), channels 8-15
    scale = 0, shift < 0 (ties at the ReLU's zero)."""
    g = torch.Generator().manual_seed(31 + H + 2 * W + B)
    scale = (torch.rand(64, generator=g) + 0.5) * (torch.randint(0, 2, (64,), generator=g) * 2 - 1)
    shift = torch.randn(64, generator=g) * 0.5
    scale[:16] = 0.0
    shift[:8] = shift[:8].abs() + 0.1
    shift[8:16] = -shift[8:16].abs() - 0.1
    return scale, shift


def pool_is_maxpool_of_dense(L, dev, inp):
    """Test 2: stem_pool_kernel against max_pool2d (float32, CPU) of what stem_conv_kernel (relu = 1, no bias) writes with the same filters and
    scale / shift: the pooled map bit for bit, the argmax bytes equal to the codes of torch's indices (first maximum in scan order)."""
    d = Device(L, dev, inp)
    scale, shift = pool_scale_shift(inp.B, inp.H, inp.W)
    sc, sh = scale.to(dev), shift.to(dev)
    dense = nchw(d.conv(sc, sh, 1, bias=None)).cpu()
    pooled, arg = d.pool(sc, sh)
    pooled, arg = nchw(pooled).cpu(), nchw(arg).cpu()
    p_ref, idx = TF.max_pool2d(dense, 3, 2, 1, return_indices=True)
    code = window_code(idx, inp.H, inp.W)
    tie = constant_map_codes(inp.H // 2, inp.W // 2)
    y = TF.conv2d(inp.img.double(), inp.w.double(), None, 1, 2)
    ref64 = TF.relu(y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    return dict(map_differs=float((pooled != p_ref).sum()), argmax_differs=float((arg != code).sum()),
                tie_channels_differ=float((arg[:, :16] != tie).sum()), windows=float(arg.numel()),
                dense=rel_err(dense, ref64), tie_values=float((pooled[:, :8] != shift[:8].view(1, 8, 1, 1)).sum() + (pooled[:, 8:16] != 0).sum()))


def deterministic_slots(L, dev, inp):
    """Test 5: with awr_stem_slots() copies every workgroup owns its slot.  The raw [slot][2][64] arrays of the statistics and of the
    BN-backward sums, read before any finalize: the used slots are a prefix [0, n), n = B * tiles / t for one t of WG_TILES that divides the
    tile count (found from n, not assumed), slot k holds the sums over tiles [t j, t j + t) of image b, k = b * tiles / t + j; two runs give
    the same bits.  The weight gradient with wgrad_slots copies is bit-identical across two runs."""
    d, r = Device(L, dev, inp), inp.r64
    ss, ws = d.slots()
    tiles = tiles_of(inp.H, inp.W)
    f = dict(stats_slots=float(ss), wgrad_slots=float(ws))

    def groups(raw, name):
        n = used_prefix(raw)
        f[name + "_used"] = float(n)
        assert n > 0, (name, "the non-zero slots are no prefix")
        t, rem = divmod(inp.B * tiles, n)
        f[name + "_t"] = float(t)
        assert rem == 0 and t in WG_TILES and tiles % t == 0, (name, n, t)
        return n, t

    def raw_of(launch):
        out = []
        for _ in range(2):
            buf = d.buffer(ss, 128, torch.float64)
            launch(buf)
            out.append(d.used(buf, ss, 128).view(ss, 2, 64).cpu())
            f["guard"] = f.get("guard", 0.0) + d.guard_touched(buf, ss, 128)
        return out + [buf]

    a, b, stats = raw_of(lambda buf: d.stats(buf, ss))
    f["stats_runs_differ"] = float(not torch.equal(a, b))
    n, t = groups(a, "stats")
    f["slot_sum"] = rel_err(a[:n, 0], group_tiles(tile_sums(r.y), t))
    f["slot_sumsq"] = rel_err(a[:n, 1], group_tiles(tile_sums(r.y * r.y), t))
    coef4 = d.bn_finalize(stats, ss)
    arg = d.pool(coef4[0], coef4[1])[1] if inp.pooled else None
    a, b, sums = raw_of(lambda buf: d.bwd_reduce(coef4, arg, buf, ss))
    f["sums_runs_differ"] = float(not torch.equal(a, b))
    n, t = groups(a, "sums")
    xhat = (r.y - r.mean.view(1, -1, 1, 1)) / torch.sqrt(r.var.view(1, -1, 1, 1) + 1e-5)
    f["slot_g"] = rel_err(a[:n, 0], group_tiles(tile_sums(r.gz), t))
    f["slot_gxhat"] = rel_err(a[:n, 1], group_tiles(tile_sums(r.gz * xhat), t))
    coef, _, _ = d.bn_bwd_finalize(sums, coef4, ss)
    dw = d.buffer(ws, 64 * 26, torch.float32)
    gw1, gb1 = d.bwd_wgrad(coef4, coef, arg, dw, ws)
    gw2, gb2 = d.bwd_wgrad(coef4, coef, arg, dw, ws)
    f["wgrad_runs_differ"] = float(not (torch.equal(gw1, gw2) and torch.equal(gb1, gb2)))
    f["dW"] = rel_err(gw1.cpu(), r.dW)
    f["guard"] += d.guard_touched(dw, ws, 64 * 26)
    return f


# every raw slot sum at the bound of the mean check (the mean is such a sum divided by a constant; the BN-backward sums are float32 sums of
# as many terms); the sums of squares, which the variance check reads, at the variance's
SLOT_BOUNDS = dict(slot_sum=2e-6, slot_sumsq=2e-5, slot_g=2e-6, slot_gxhat=2e-6, dW=5e-5)
SLOT_EXACT = ("stats_runs_differ", "sums_runs_differ", "wgrad_runs_differ", "guard")


def accumulate(L, dev, inp, other):
    """Test 6: the statistics and BN-backward sums ADD to what the accumulator holds.  In deterministic-slot mode every slot takes one float64
    add per launch, so launching `inp` and then `other` (same shape) onto one array gives exactly the float64 sum of their separate arrays,
    and a launch onto a pre-filled array exactly pre-fill + its own array."""
    da, db = Device(L, dev, inp), Device(L, dev, other)
    ss, _ = da.slots()
    g = torch.Generator().manual_seed(9)
    prefill = torch.randn(ss * 128, generator=g, dtype=torch.float64).to(dev)
    f = {}

    def check(name, la, lb):
        sa, sb, both, pre = (da.buffer(ss, 128, torch.float64) for _ in range(4))
        la(sa)
        lb(sb)
        la(both)
        lb(both)
        da.used(pre, ss, 128).copy_(prefill)
        la(pre)
        f[name + "_two_launches"] = float((da.used(both, ss, 128) != da.used(sa, ss, 128) + da.used(sb, ss, 128)).sum())
        f[name + "_prefilled"] = float((da.used(pre, ss, 128) != prefill + da.used(sa, ss, 128)).sum())
        f[name + "_empty"] = float(not bool(da.used(sa, ss, 128).any() and da.used(sb, ss, 128).any()))
        f["guard"] = f.get("guard", 0.0) + sum(da.guard_touched(x, ss, 128) for x in (sa, sb, both, pre))
        return sa

    sa = check("stats", lambda buf: da.stats(buf, ss), lambda buf: db.stats(buf, ss))
    coef4 = da.bn_finalize(sa, ss)
    arg_a = da.pool(coef4[0], coef4[1])[1] if inp.pooled else None
    arg_b = db.pool(coef4[0], coef4[1])[1] if other.pooled else None
    check("sums", lambda buf: da.bwd_reduce(coef4, arg_a, buf, ss), lambda buf: db.bwd_reduce(coef4, arg_b, buf, ss))
    return f
