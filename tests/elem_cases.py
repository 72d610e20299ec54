"""The shapes, launch arithmetic, inputs and float64 references the operator tests of the streaming kernels share (csrc/awr_elem.hip: the
channel reductions of col_reduce_kernel, the BatchNorm pieces, relu_bwd / add, max-pool and the 2x up-sampling add; tests/test_elem_cpu.py,
tests/test_elem_gpu.py).

reduce_launch() restates ONLY the arithmetic of col_reduce_launch / col_reduce_kernel, so the CPU test can say which launch class each shape
of REDUCE_SHAPES is in.  The references are plain float64 loops / tensor expressions of the definitions in include/awr_hip.h; none of them calls
the library, and tests/test_elem_cpu.py holds each of them against torch's own operators."""
import torch

STAT_SLOTS = 16             # AWR_STAT_SLOTS: what nslots = 0 stands for
MAX_BLOCKS = 1024           # AWR_REDUCE_MAX_BLOCKS: workgroup cap of a reduction launch = slot copies of a deterministic plan

# (npix, C): what each is in the table for -- the classes tests/test_elem_cpu.py asserts from reduce_launch()
REDUCE_SHAPES = [
    (1, 4),             # one row, 256 row groups, 255 threads without a row
    (63, 8),            # fewer rows than row groups
    (65, 96),           # 16 idle threads, one slab, unrolled trip plus tail (6 / 7 rows per thread)
    (257, 4),           # second slab of one row
    (4099, 64),         # the unrolled trip only (4 rows per thread); last slab of 3 rows
    (66001, 64),        # slabs longer than 64 rows
    (70001, 256),       # slabs longer than 64 rows, 973 workgroups (near the cap), 4 trips + 2 tail rows
    (577, 1024),        # the widest single chunk
    (131, 2048),        # two channel chunks (Bottleneck layer4)
    (97, 3072),         # three channel chunks
    (1030, 516),        # 129 float4 columns: 127 idle threads in every one of 17 slabs
    (351, 128),         # 3 x 9 x 13 pixels: the non-square map of the pool cases
]

# (k, s, p, B, H, W, C)
POOL_CASES = [
    (3, 2, 1, 2, 14, 10, 8),
    (2, 2, 0, 3, 9, 7, 4),          # odd extents: the last row and column lie in no window
    (2, 2, 0, 3, 18, 26, 128),      # output 3 x 9 x 13 = 351 pixels
    (3, 1, 1, 2, 6, 5, 12),         # overlapping windows: up to 9 per input pixel
    (5, 3, 2, 1, 11, 17, 4),
    (3, 2, 0, 2, 7, 9, 64),
    (2, 2, 0, 2, 4, 4, 2048),       # two channel chunks in the fused-statistics form
]
# (B, Hl, Wl, C)
UPSAMPLE_CASES = [(1, 1, 1, 4), (2, 3, 5, 12), (3, 9, 13, 128), (1, 2, 2, 2048)]

MASKS = ["none", "act", "affine"]       # BatchNorm backward: no ReLU mask / (act > 0) / (y * mask_scale + mask_shift > 0)


def case_id(case):
    return "x".join(str(v) for v in case)


def pool_out(k, s, p, H, W):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _cdiv(a, b):
    return -(-a // b)


def reduce_launch(npix, C):
    """What col_reduce_launch starts for an (npix, C) matrix and what each thread of col_reduce_kernel walks: chunks of Cw <= 1024 channels
    (blockIdx.y), 256 threads = rpp row groups x C4 float4 columns (the rest idle), slabs of `rows` rows (>= 64, at most MAX_BLOCKS slabs,
    rounded up to rpp), and the number of rows one thread reads in a full slab / in the last slab (row group rg reads rg, rg + rpp, ...)."""
    assert C % 4 == 0 and C >= 4 and (C <= 1024 or C % 1024 == 0) and npix > 0
    Cw = min(C, 1024)
    C4 = Cw // 4
    rpp = 256 // C4
    rows = max(64, _cdiv(npix, MAX_BLOCKS))
    rows = _cdiv(rows, rpp) * rpp
    grid = _cdiv(npix, rows)
    last = npix - (grid - 1) * rows

    def per_thread(n):
        return frozenset(len(range(rg, n, rpp)) for rg in range(rpp))
    return {"Cw": Cw, "chunks": C // Cw, "C4": C4, "rpp": rpp, "idle": 256 - rpp * C4, "rows": rows, "grid": grid, "last_rows": last,
            "full": per_thread(rows) if grid > 1 else frozenset(), "last": per_thread(last)}


def launch_classes(npix, C):
    """The names of the launch classes an (npix, C) reduction is in (tests/test_elem_cpu.py requires REDUCE_SHAPES to cover ALL_CLASSES)"""
    la = reduce_launch(npix, C)
    cls = set()
    cls.add("single slab" if la["grid"] == 1 else "many slabs")
    if la["grid"] > 1 and la["last_rows"] < la["rows"]:
        cls.add("ragged last slab")
    if la["rows"] > 64:
        cls.add("rows > 64")
    if la["grid"] > 900:
        cls.add("grid > 900")
    if la["idle"]:
        cls.add("idle threads, one slab" if la["grid"] == 1 else "idle threads, many slabs")
    if la["rpp"] in (1, 256):
        cls.add("rpp == %d" % la["rpp"])
    if la["chunks"] in (2, 3):
        cls.add("%d chunks" % la["chunks"])
    for n in la["full"] | la["last"]:
        cls.add("no row" if n == 0 else "below 4 rows" if n < 4 else "4n rows" if n % 4 == 0 else "4n + r rows")
    return cls


ALL_CLASSES = {"single slab", "many slabs", "ragged last slab", "rows > 64", "grid > 900", "idle threads, one slab", "idle threads, many slabs",
               "rpp == 1", "rpp == 256", "2 chunks", "3 chunks", "no row", "below 4 rows", "4n rows", "4n + r rows"}


def exact_bound_holds(npix):
    """With exact_inputs() fp32 returns the float64 sums bit for bit, in any order of summation.  Statistics: the values are integers of
    magnitude <= 4; the kernels sum them shifted by a first row, |x - x0| <= 8, so every square is an integer <= 64 and every partial sum is an
    integer below 64 * npix.  BatchNorm backward: |g| <= 4, xhat = (y - mean) * invstd is a multiple of 1/2 of magnitude <= (8 + 3) * 2 = 22, so
    every term g * xhat is a multiple of 1/2 of magnitude <= 88 and every partial sum, counted in halves, stays below 2 * 88 * npix."""
    return 64 * npix < 2 ** 24 and 2 * 88 * npix < 2 ** 24


def _gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _choice(g, values, n):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), (n,), generator=g)]


def exact_inputs(kind, npix, C):
    """Integer-valued float32 inputs of one reduction, seeded by (kind, shape).  kind "stats" / "bias": {"x"} in [-4, 4].  kind "bnbwd": dout
    in [-4, 4], y in [-8, 8], mean in [-3, 3], invstd in {1/2, 1, 2}, mask_scale in {-1, 1, 2}, mask_shift in {-2, 0, 1}, act in [-2, 2] with
    three of five values at exactly zero or below."""
    assert exact_bound_holds(npix), npix
    g = _gen({"stats": 1, "bias": 2, "bnbwd": 3}[kind], npix, C)
    if kind in ("stats", "bias"):
        return {"x": _ints(g, -4, 4, npix, C)}
    return {"dout": _ints(g, -4, 4, npix, C), "y": _ints(g, -8, 8, npix, C), "mean": _ints(g, -3, 3, C), "invstd": _choice(g, [0.5, 1.0, 2.0], C),
            "mask_scale": _choice(g, [-1.0, 1.0, 2.0], C), "mask_shift": _choice(g, [-2.0, 0.0, 1.0], C), "act": _ints(g, -2, 2, npix, C)}


def exact_pool_inputs(case, affine):
    """x (B, H, W, C), scale (C), shift (C) or None: integers, so that the pooled tensor -- of x, or of relu(x * scale + shift) -- is an integer
    tensor of magnitude <= 4 with many ties, and fp32 evaluates x * scale + shift exactly with or without contraction"""
    k, s, p, B, H, W, C = case
    g = _gen(4, *case, int(affine))
    if not affine:
        return _ints(g, -4, 4, B, H, W, C), None, None
    return _ints(g, -1, 1, B, H, W, C), _choice(g, [-1.0, 1.0, 2.0], C), _ints(g, -2, 2, C)


def exact_upsample_inputs(case):
    """up1 (B, 2 Hl, 2 Wl, C), low (B, Hl, Wl, C): integers in [-2, 2], so the sum the kernel writes is an integer in [-4, 4]"""
    B, Hl, Wl, C = case
    g = _gen(5, *case)
    return _ints(g, -2, 2, B, 2 * Hl, 2 * Wl, C), _ints(g, -2, 2, B, Hl, Wl, C)


def rnd(g, *shape):
    """uniform in (-1, 1), the style of rnd() in tests/test_ops_gpu.py"""
    return torch.rand(*shape, generator=g) * 2 - 1


MASK_MARGIN = 1e-5


def real_inputs(kind, npix, C):
    """Seeded real-valued float32 inputs.  kind "stats": {"x"} with mean about 3 and spread about 0.5.  kind "bias": {"x"} in (-1, 1).
    kind "bnbwd": a BatchNorm input y, its batch mean / invstd, gamma, the forward's scale / shift as mask_scale / mask_shift (some negative
    gammas), dout, a residual, act = relu(y * scale + shift + res), and dy_add.  No element of y * mask_scale + mask_shift lies within
    MASK_MARGIN of zero (the few that did are moved; asserted), so the affine mask is the same in float64 and in fp32 with or without contraction."""
    g = _gen({"stats": 6, "bias": 7, "bnbwd": 8}[kind], npix, C)
    if kind == "stats":
        return {"x": 3.0 + 0.5 * torch.randn(npix, C, generator=g)}
    if kind == "bias":
        return {"x": rnd(g, npix, C)}
    y = rnd(g, npix, C) * 2 + 0.3
    yd = y.double()
    mean = yd.mean(0)
    invstd = 1.0 / torch.sqrt(yd.var(0, unbiased=False) + 1e-5) if npix > 1 else torch.ones(C, dtype=torch.float64)
    gamma = rnd(g, C) + 0.7
    beta = rnd(g, C) * 0.5
    scale = (gamma.double() * invstd).float()
    shift = (beta.double() - mean * scale.double()).float()
    t = yd * scale.double() + shift.double()
    for _ in range(8):          # (mean / invstd are operands of the kernels: they stay as they are)
        if float(t.abs().min()) > 10 * MASK_MARGIN:
            break
        y = torch.where(t.abs() < 10 * MASK_MARGIN, y + 0.25, y)
        yd = y.double()
        t = yd * scale.double() + shift.double()
    assert float(t.abs().min()) > MASK_MARGIN, (npix, C, float(t.abs().min()))
    res = rnd(g, npix, C)
    act = (t + res.double()).clamp(min=0).float()
    return {"dout": rnd(g, npix, C), "y": y, "mean": mean.float(), "invstd": invstd.float(), "gamma": gamma, "mask_scale": scale,
            "mask_shift": shift, "act": act, "dy_add": rnd(g, npix, C)}


def pool_data(case):
    """post-ReLU real data with many exact zeros (ties), as test_maxpool uses: (B, H, W, C) float32"""
    k, s, p, B, H, W, C = case
    x = rnd(_gen(9, *case), B, H, W, C)
    x[:, ::3, ::3, :] = 0.0
    return x.clamp(min=0)


# ------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------
def stats_ref(x):
    """(sum x, sum x^2) per channel of an (..., C) tensor, float64"""
    xd = x.double().reshape(-1, x.shape[-1])
    return xd.sum(0), (xd * xd).sum(0)


def _taps(k, s, p, n_in, n_out):
    """per tap offset kk: (output indices whose tap kk lies inside the map, the input indices it reads)"""
    o = torch.arange(n_out)
    out = []
    for kk in range(k):
        i = o * s - p + kk
        ok = (i >= 0) & (i < n_in)
        out.append((o[ok], i[ok]))
    return out


def maxpool_ref(x, k, s, p):
    """x (B, H, W, C) -> (out (B, Ho, Wo, C) float64, argmax uint8): the taps are scanned in ky, kx order, taps outside the map are skipped,
    the first maximum wins (strict >), the code is ky * k + kx"""
    B, H, W, C = x.shape
    Ho, Wo = pool_out(k, s, p, H, W)
    xd = x.double()
    m = torch.full((B, Ho, Wo, C), float("-inf"), dtype=torch.float64)
    arg = torch.zeros((B, Ho, Wo, C), dtype=torch.uint8)
    ty, tx = _taps(k, s, p, H, Ho), _taps(k, s, p, W, Wo)
    for ky in range(k):
        oy, iy = ty[ky]
        for kx in range(k):
            ox, ix = tx[kx]
            if not len(oy) or not len(ox):
                continue
            cand = torch.full_like(m, float("-inf"))
            cand[:, oy[:, None], ox[None, :]] = xd[:, iy[:, None], ix[None, :]]
            upd = cand > m
            m = torch.where(upd, cand, m)
            arg = torch.where(upd, torch.tensor(ky * k + kx, dtype=torch.uint8), arg)
    return m, arg


def maxpool_bwd_ref(dout, arg, k, s, p, H, W):
    """dx (B, H, W, C) float64: every output pixel's gradient goes to the tap its argmax code names"""
    B, Ho, Wo, C = dout.shape
    dx = torch.zeros((B, H, W, C), dtype=torch.float64)
    ty, tx = _taps(k, s, p, H, Ho), _taps(k, s, p, W, Wo)
    dd = dout.double()
    for ky in range(k):
        oy, iy = ty[ky]
        for kx in range(k):
            ox, ix = tx[kx]
            if not len(oy) or not len(ox):
                continue
            part = torch.where(arg == ky * k + kx, dd, torch.zeros_like(dd))
            dx[:, iy[:, None], ix[None, :]] += part[:, oy[:, None], ox[None, :]]      # one tap: every input pixel at most once
    return dx


def upsample2_add_ref(up1, low):
    """up1 (B, 2 Hl, 2 Wl, C) + nearest-neighbour x2 of low (B, Hl, Wl, C), float64"""
    B, Hl, Wl, C = low.shape
    out = up1.double().clone().view(B, Hl, 2, Wl, 2, C)
    out += low.double().view(B, Hl, 1, Wl, 1, C)
    return out.view(B, 2 * Hl, 2 * Wl, C)


def upsample2_bwd_ref(dout):
    """dlow (B, Hl, Wl, C) = the sum of dout over each 2x2 block, float64"""
    B, H, W, C = dout.shape
    return dout.double().view(B, H // 2, 2, W // 2, 2, C).sum((2, 4))


def bn_bwd_sums_ref(dout, y, mean, invstd, act=None, mask_scale=None, mask_shift=None):
    """(g, xhat, sum g, sum g * xhat) on (npix, C) matrices, float64: g = dout * mask with mask = (act > 0) if act is given,
    (y * mask_scale + mask_shift > 0) if those are, else 1; xhat = (y - mean) * invstd"""
    g, yd = dout.double(), y.double()
    if act is not None:
        g = torch.where(act.double() > 0, g, torch.zeros_like(g))
    elif mask_scale is not None:
        g = torch.where(yd * mask_scale.double() + mask_shift.double() > 0, g, torch.zeros_like(g))
    xhat = (yd - mean.double()) * invstd.double()
    return g, xhat, g.sum(0), (g * xhat).sum(0)


def bn_bwd_ref(dout, y, mean, invstd, gamma=None, act=None, mask_scale=None, mask_shift=None, dy_add=None):
    """BatchNorm backward, float64: with (g, xhat, s1, s2) of bn_bwd_sums_ref, dy = gamma * invstd * (g - s1 / n - xhat * s2 / n) [+ dy_add],
    dgamma = s2, dbeta = s1"""
    n = dout.shape[0]
    g, xhat, s1, s2 = bn_bwd_sums_ref(dout, y, mean, invstd, act, mask_scale, mask_shift)
    gi = (gamma.double() if gamma is not None else 1.0) * invstd.double()
    dy = gi * (g - s1 / n - xhat * (s2 / n))
    if dy_add is not None:
        dy = dy + dy_add.double()
    return {"g": g, "s1": s1, "s2": s2, "dy": dy, "dgamma": s2, "dbeta": s1}


def lin4_ref(s1, s2, n, gamma, mean, invstd):
    """[a1 | a2 | a3 | mean] with dy = a1 g + a2 (y - mean) + a3: a1 = gamma invstd, a2 = -a1 invstd s2 / n, a3 = -a1 s1 / n"""
    a1 = (gamma.double() if gamma is not None else 1.0) * invstd.double()
    return torch.stack([a1, -a1 * invstd.double() * (s2 / n), -a1 * (s1 / n), mean.double()])


def bn_finalize_ref(s1, s2, count, gamma, beta, rmean, rvar, momentum, eps):
    """nn.BatchNorm2d's training forward from the channel sums, float64: (scale, shift, mean, invstd, running mean, running var); the biased
    variance (clamped at 0) normalises, the running variance is the unbiased one where count > 1"""
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp(min=0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = (gamma.double() if gamma is not None else 1.0) * invstd
    shift = (beta.double() if beta is not None else 0.0) - mean * scale
    unb = var * count / (count - 1) if count > 1 else var
    rm = (1 - momentum) * rmean.double() + momentum * mean if rmean is not None else None
    rv = (1 - momentum) * rvar.double() + momentum * unb if rvar is not None else None
    return scale, shift, mean, invstd, rm, rv
