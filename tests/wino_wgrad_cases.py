"""The shapes, launch arithmetic, inputs and float64 reference the tests of the Winograd-domain weight gradient share (awr_wino_wgrad,
csrc/awr_wino.hip: wino_wgrad_kernel + wino_wgrad_reduce_kernel; tests/test_wino_wgrad_cpu.py, tests/test_wino_wgrad_gpu.py).

The kernel's main loop runs two stages (2 x 4 patch blocks) per iteration over the range [g_lo, g_hi) of its split; what a launch exercises --
how often the loop runs, whether the ranges of one launch differ in length, which parts of the reduce kernel's split-copy sum run -- follows from
the split count S the host picks.  launch_shape() reads S back from the library and restates ONLY the kernels' range arithmetic, so the CPU test
can say which of those classes each shape of the table is in, whatever the host rule becomes."""
import torch

# (B, H, W, C, N): what each is in the table for -- the classes tests/test_wino_wgrad_cpu.py asserts from launch_shape()
SHAPES = [
    (1, 8, 8, 64, 64),          # one split, three empty reduce groups, a grid of fewer than 8 workgroups
    (2, 8, 8, 256, 512),        # C != N, empty reduce groups between full ones
    (2, 16, 16, 64, 192),       # N > C, three N tiles
    (3, 32, 32, 192, 128),      # ranges of 2 and 4 stages; reduce groups of 10 and 11 (unrolled part + tail); grid % 8 = 2; 3 x 2 tiles
    (5, 64, 64, 64, 64),        # ranges of 2 and 4 stages at the largest S, eight blocks per image row
    (6, 8, 8, 512, 512),        # ranges of 2 and 4 stages, one block per image row
    (5, 16, 32, 256, 256),      # ranges of 4 and 6 stages: every split in the steady state
    (5, 8, 16, 512, 512),       # the same on 64 tiles
    (3, 32, 32, 256, 256),      # three loop iterations
    (4, 16, 16, 512, 512),      # eight stages: where plans start to take the kernel
    (16, 32, 32, 128, 128),     # eight stages, reduce groups of 16 (the unrolled part twice, no tail)
    (9, 16, 16, 512, 512),      # nine loop iterations
]
ELIGIBLE = [(4, 16, 16, 512, 512), (16, 32, 32, 128, 128), (9, 16, 16, 512, 512)]      # awr_wino_wgrad_eligible under the default code
FORMS = [(False, False), (False, True), (True, False), (True, True)]                    # (fused input affine, fused input ReLU)


def shape_id(shape):
    return "x".join(str(v) for v in shape)


def launch_shape(lib, B, H, W, C, N):
    """What the host launches for this shape: S from the library's scratch size, the rest the kernels' own arithmetic (wino_wgrad_kernel:
    g_lo / g_hi; wino_wgrad_reduce_kernel: s_lo / s_hi)"""
    n = int(lib.awr_wino_wgrad_scratch(B, H, W, C, N))
    per_split = 16 * C * N + N
    assert n > 0 and n % per_split == 0, (n, per_split)
    S = n // per_split
    nblocks = B * (H // 4) * (W // 8)
    npairs = nblocks // 2
    nst = [2 * (npairs * (s + 1) // S) - 2 * (npairs * s // S) for s in range(S)]
    assert sum(nst) == nblocks and min(nst) >= 2, (nst, nblocks)
    return {"S": S, "nblocks": nblocks, "nst": nst, "stages": frozenset(nst), "groups": tuple(S * (g + 1) // 4 - S * g // 4 for g in range(4)),
            "grid": S * (C // 64) * (N // 64), "scratch": n}


def exact_bound_holds(B, H, W):
    """With the `exact` inputs fp32 returns the float64 result bit for bit, in any order of summation: |d| <= 3 behind the affine, so
    |B^T d B| <= 12 and |A dY A^T| <= 4 are integers, and so is every partial sum over the K = B*H*W/4 patches, |dU| <= 48 K.  G^T . G (rows of
    absolute sum <= 2, entries 1, 1/2, 0) makes multiples of 1/4 of magnitude <= 4 * 48 K: exact in fp32 while 16 * 48 K < 2^24.  The bound
    asked for is four times stricter (64 * K * 12 * 4 < 2^24)."""
    return 64 * (B * H * W // 4) * 12 * 4 < 2 ** 24


def inputs(shape, form, kind):
    """x (B, C, H, W), dy (B, N, H, W), scale (C) / shift (C) or None, float32, seeded by the shape"""
    B, H, W, C, N = shape
    affine, _ = form
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + C + (7 if kind == "exact" else 0))
    if kind == "random":
        x = torch.randn(B, C, H, W, generator=g)
        dy = torch.randn(B, N, H, W, generator=g)
        sc = (torch.rand(C, generator=g) + 0.5) if affine else None
        sh = (torch.randn(C, generator=g) * 0.3) if affine else None
    else:
        assert kind == "exact", kind
        assert exact_bound_holds(B, H, W), shape
        x = torch.randint(-1, 2, (B, C, H, W), generator=g).float()
        dy = torch.randint(-1, 2, (B, N, H, W), generator=g).float()
        sc = torch.randint(1, 3, (C,), generator=g).float() if affine else None
        sh = torch.randint(-1, 2, (C,), generator=g).float() if affine else None
    return x, dy, sc, sh


def float64_gradient(x, dy, sc, sh, relu):
    """(dw (N, C, 3, 3), dbias (N)) in float64: autograd of conv2d(affine / ReLU(x), w, padding=1) at w = 0, dy summed over the pixels"""
    a = x.double()
    if sc is not None:
        a = a * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    if relu:
        a = a.clamp(min=0)
    w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad((torch.nn.functional.conv2d(a, w, padding=1) * dy.double()).sum(), w)
    return gw, dy.double().sum(dim=(0, 2, 3))


_REF = {}


def reference(shape, form, kind):
    """float64_gradient of inputs(shape, form, kind), computed once per (shape, form, kind).  The `exact` results are kept in float32: they
    have to fit it without loss for the bit-for-bit comparison to mean anything, which is asserted here."""
    key = (tuple(shape), tuple(form), kind)
    if key not in _REF:
        x, dy, sc, sh = inputs(shape, form, kind)
        gw, gb = float64_gradient(x, dy, sc, sh, form[1])
        if kind == "exact":
            assert torch.equal(gw.float().double(), gw) and torch.equal(gb.float().double(), gb), shape
            gw, gb = gw.float(), gb.float()
        _REF[key] = (gw, gb)
    gw, gb = _REF[key]
    return gw.double(), gb.double()
