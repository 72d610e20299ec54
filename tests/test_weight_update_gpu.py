"""The weight-update path link by link, through the C ABI: the batched unpack of the weight-gradient copies (awr_unpack_wgrads_batched), the
optimiser kernels (awr_adam_step / awr_sgd_step) and the batched repack with its split image (awr_pack_weights_batched).

Pack, unpack and the split image are data movement or fp32 additions in a fixed order: those tests compare BITS (torch.equal of the int32 / int16
views, so that -0.0 and the NaN fill count too) with plain CPU references and have no tolerance.  The optimiser tests bound the kernels' error
against the update rule in float64 by the error that the float32 torch rule makes on the same inputs, measured in the test itself."""
import math

import numpy as np
import pytest
import torch

import awr_oracle as O

pytestmark = pytest.mark.gpu

_KEEP = []
GUARD = 64      # guard elements in front of and behind every target (a multiple of 4 floats: the optimiser arenas stay 16-byte aligned)
NAN16 = 0x7FC0  # bf16 NaN: the fill of the split images


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    import awr_amd  # noqa: F401
    from awr_amd import _lib
    return _lib


def nan_arena(dev, n, host=None):
    """(whole, target): n floats (NaN, or `host`) between two NaN guard bands; kept alive until the module is torn down"""
    whole = torch.full((n + 2 * GUARD,), float("nan"))
    if host is not None:
        whole[GUARD:GUARD + n] = host.reshape(-1)
    whole = whole.to(dev)
    _KEEP.append(whole)
    return whole, whole[GUARD:GUARD + n]


def nan_image(dev, n):
    """(whole, image): the split image of n packed floats (3 n int16), filled with bf16 NaN, between two guard bands"""
    whole = torch.full((3 * n + 2 * GUARD,), NAN16, dtype=torch.int16, device=dev)
    _KEEP.append(whole)
    return whole, whole[GUARD:GUARD + 3 * n]


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def guards_are_nan(whole):
    w = whole.cpu()
    if w.dtype == torch.int16:
        return bool((w[:GUARD] == NAN16).all() and (w[-GUARD:] == NAN16).all())
    return bool(torch.isnan(w[:GUARD]).all() and torch.isnan(w[-GUARD:]).all())


# ------------------------------------------------------------------------------------------
# 1. awr_pack_weights_batched
# ------------------------------------------------------------------------------------------
def _pj(name, d0, d1, T, tr, rows, ld, cols=0, buf=None, off=0):
    return dict(name=name, d0=d0, d1=d1, T=T, tr=tr, rows=rows, ld=ld, cols=cols, buf=buf or name, off=off)


# one table: the one-row jobs (g1, g2) sit between larger ones and g2 is last
PACK_JOBS = [
    _pj("a0", 96, 64, 9, 0, 128, 64),          # the two recipes of test_pack_unpack_roundtrip; 32 zero rows
    _pj("g1", 1, 32, 1, 0, 1, 32),             # find_job: a one-row job between large ones
    _pj("b", 5, 928, 9, 0, 8, 928),            # two column chunks at T = 9 (896 + 32)
    _pj("c", 3, 512, 16, 0, 4, 512),           # two chunks at T = 16 (480 + 32)
    _pj("a1", 96, 64, 9, 1, 64, 96),
    _pj("d", 512, 3, 16, 1, 4, 512),           # transposed and chunked: the first deconvolution of the Bottleneck ResNets
    _pj("e", 2, 200, 25, 0, 2, 224),           # odd T, inner < ld (ONE chunk: at T = 25 a chunk holds 320 columns, more than ld)
    _pj("e2", 2, 340, 25, 0, 2, 352),          # odd T with a ragged second chunk (320 + 32 columns, of which 20 hold weights)
    _pj("f", 42, 250, 1, 0, 64, 256),          # T = 1, inner < ld, padded rows
    _pj("hA", 40, 120, 1, 0, 64, 192, cols=128, buf="h", off=0),      # two jobs fill one buffer side by side (dual layers)
    _pj("hB", 40, 64, 1, 0, 64, 192, cols=64, buf="h", off=128),
    _pj("g2", 1, 32, 1, 0, 1, 32),             # find_job: the last job has one row
]
SPLIT_JOBS = ("a0", "a1", "b", "c", "d", "f")  # rows * T * ld is a multiple of 32 in each


def _weights(jobs, seed):
    g = torch.Generator().manual_seed(seed)
    return {j["name"]: torch.randn(j["d0"], j["d1"], j["T"], generator=g) for j in jobs}


def pack_ref(w, j, fill=0.0):
    """the packed image of one cols == 0 job: zero-filled (rows, T, ld)"""
    p = torch.full((j["rows"], j["T"], j["ld"]), fill)
    if not j["tr"]:
        p[:j["d0"], :, :j["d1"]] = w.permute(0, 2, 1)
    else:
        p[:j["d1"], :, :j["d0"]] = w.permute(1, 2, 0)
    return p


def buffer_ref(jobs, ws, buf):
    """what one destination holds after the launch: NaN where no job writes, zeros in every job's rows x T x cols window, then the weights"""
    mine = [j for j in jobs if j["buf"] == buf]
    ref = torch.full((mine[0]["rows"], mine[0]["T"], mine[0]["ld"]), float("nan"))
    for j in mine:
        cols = j["cols"] or j["ld"]
        win = dict(j, ld=cols)
        ref[:, :, j["off"]:j["off"] + cols] = pack_ref(ws[j["name"]], win)
    return ref


def launch_pack(L, dev, jobs, ws, split=False):
    """ONE awr_pack_weights_batched launch over `jobs`; returns {buf: (whole, target)} and, with split, {buf: (whole, image)}"""
    bufs, imgs, table, first = {}, {}, [], 0
    for j in jobs:
        n = j["rows"] * j["T"] * j["ld"]
        if j["buf"] not in bufs:
            bufs[j["buf"]] = nan_arena(dev, n)
            if split:
                imgs[j["buf"]] = nan_image(dev, n)
        src = ws[j["name"]].contiguous().to(dev)
        _KEEP.append(src)
        table.append(L.PackJob(src=L.ptr(src), dst=bufs[j["buf"]][1].data_ptr() + 4 * j["off"],
                               split=imgs[j["buf"]][1].data_ptr() if split else None, d0=j["d0"], d1=j["d1"], T=j["T"], transpose=j["tr"],
                               rows=j["rows"], ld=j["ld"], first=first, cols=j["cols"], reserved=0))
        first += j["rows"]
    tab = L.job_table(table, dev)
    _KEEP.append(tab)
    L.call("awr_pack_weights_batched", L.ptr(tab), len(table), first, L.stream())
    torch.cuda.synchronize()
    return bufs, imgs


@pytest.fixture(scope="module")
def pack_run(L, dev):
    ws = _weights(PACK_JOBS, seed=11)
    bufs, _ = launch_pack(L, dev, PACK_JOBS, ws)
    return ws, bufs


def test_pack_batched_one_launch_equals_the_reference(pack_run):
    ws, bufs = pack_run
    for buf, (whole, got) in bufs.items():
        assert guards_are_nan(whole), buf
        assert same_bits(got, buffer_ref(PACK_JOBS, ws, buf).reshape(-1)), buf
    # the side-by-side pair, spelled out: A in columns [0, 120), zeros in [120, 128), B in [128, 192), zero rows from 40 on
    h = bufs["h"][1].cpu().view(64, 192)
    assert torch.equal(h[:40, :120], ws["hA"][:, :, 0]) and torch.equal(h[:40, 128:], ws["hB"][:, :, 0])
    assert same_bits(h[:40, 120:128], torch.zeros(40, 8)) and same_bits(h[40:], torch.zeros(24, 192))


@pytest.mark.parametrize("name", [j["name"] for j in PACK_JOBS if not j["cols"]])
def test_pack_batched_job_alone_and_single_kernel_write_the_same_bits(L, dev, pack_run, name):
    ws, bufs = pack_run
    j = next(x for x in PACK_JOBS if x["name"] == name)
    alone, _ = launch_pack(L, dev, [j], ws)                      # njobs = 1, first = 0
    assert same_bits(alone[name][0], bufs[name][0]), name        # guard bands included
    whole, dst = nan_arena(dev, j["rows"] * j["T"] * j["ld"])
    src = ws[name].to(dev)
    L.call("awr_pack_weight", L.ptr(src), j["d0"], j["d1"], j["T"], j["tr"], j["rows"], j["ld"], L.ptr(dst), L.stream())
    torch.cuda.synchronize()
    assert same_bits(whole, bufs[name][0]), name


# ------------------------------------------------------------------------------------------
# 2. the split image written by the pack pass
# ------------------------------------------------------------------------------------------
def _f32_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


DENORM_MIN, DENORM_MAX = 0x00000001, 0x007FFFFF
SPECIALS = [
    0x00000000, 0x80000000,        # 0.0, -0.0
    DENORM_MIN, DENORM_MAX,        # the smallest and the largest denormal: OUTSIDE the exact domain of the cut (see the test)
    0x00800000,                    # FLT_MIN
    0x7F7FFFFF, 0xFF7FFFFF,        # +-FLT_MAX
    0x3F800001, 0x3F7FFFFF,        # 1 + 2^-23, 1 - 2^-24
    0x3FFFFFFF,                    # an all-ones significand
    _f32_bits(1e-30),
    0x03802000,                    # 2^-120 + 2^-130: the residual x - h is an fp32 denormal that bf16 still holds (a multiple of 2^-133)
]
PLANTED = 2                        # copies of every special per weight tensor


def _plant_specials(w, seed):
    flat = w.view(-1).numpy().view(np.uint32)
    pos = torch.randperm(flat.size, generator=torch.Generator().manual_seed(seed))[:PLANTED * len(SPECIALS)].numpy()
    flat[pos] = np.array(SPECIALS * PLANTED, np.uint32)


def test_split_image_from_the_pack_pass(L, dev):
    """The image that pack_batched_kernel writes beside the packed weights is the image awr_split_weight makes of them, and it decodes to the cut
    the header promises: per 32 elements 96 int16 [h | m | l], each the bf16 bits of one piece, h = the top 16 bits of x, m = the top 16 bits of
    x - h, and h + m + l == x.

    FINDING (pinned here, stated in awr_hip.h): the sum is exact only where x is a multiple of 2^-133, the smallest bf16 denormal -- zero and every
    |x| >= 2^-110.  Below that a residual is an fp32 denormal whose low bits no bf16 holds, and the pieces sum to x truncated toward zero to a
    multiple of 2^-133: the smallest denormal decodes to 0, the largest (0x007FFFFF) to 0x007F0000.  The test asserts that truncated value for
    EVERY element and that the only elements it differs from x at are those two planted denormals.  Weights never get there (7.7e-34)."""
    jobs = [j for j in PACK_JOBS if j["name"] in SPLIT_JOBS]
    ws = _weights(jobs, seed=12)
    for i, j in enumerate(jobs):
        _plant_specials(ws[j["name"]], seed=100 + i)
    bufs, imgs = launch_pack(L, dev, jobs, ws, split=True)
    for j in jobs:
        name, n = j["name"], j["rows"] * j["T"] * j["ld"]
        ref = pack_ref(ws[name], j)
        assert guards_are_nan(bufs[name][0]) and same_bits(bufs[name][1], ref.reshape(-1)), name
        # bit for bit what awr_split_weight writes for the reference-packed buffer
        packed = ref.to(dev)
        whole2, img2 = nan_image(dev, n)
        L.call("awr_split_weight", L.ptr(packed), L.ptr(img2), n, L.stream())
        torch.cuda.synchronize()
        assert guards_are_nan(imgs[name][0]) and torch.equal(imgs[name][0].cpu(), whole2.cpu()), name
        # decoded on the CPU
        x = ref.reshape(-1).numpy()
        xb = x.view(np.uint32)
        img = imgs[name][1].cpu().numpy().view(np.uint16).reshape(-1, 3, 32)
        pieces = (img.astype(np.uint32) << 16).view(np.float32)
        h, m, l = (np.ascontiguousarray(pieces[:, k]).reshape(-1) for k in range(3))
        assert np.array_equal(h.view(np.uint32), xb & 0xFFFF0000), name
        r1 = x - h                                                                   # exact in fp32 (the low 16 bits of the significand)
        assert np.array_equal(m.view(np.uint32), r1.view(np.uint32) & 0xFFFF0000), name
        x64 = x.astype(np.float64)
        total = h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64)   # three 8-bit pieces within 24 bits: exact in fp64
        cut = np.trunc(x64 * 2.0 ** 133) * 2.0 ** -133                               # x toward zero to a multiple of 2^-133 (exact in fp64)
        assert np.array_equal(total, cut), name
        off = cut != x64
        assert int(off.sum()) == 2 * PLANTED and set(xb[off].tolist()) == {DENORM_MIN, DENORM_MAX}, name
        assert np.array_equal(total[~off], x64[~off]), name                          # h + m + l == x EXACTLY everywhere else
        pad = pack_ref(torch.ones(j["d0"], j["d1"], j["T"]), j).reshape(-1).numpy() == 0
        assert bool(pad.any()) == (n > ws[name].numel()), name
        assert not img.transpose(0, 2, 1).reshape(-1, 3)[pad].any(), name            # zero padding -> three zero pieces


# ------------------------------------------------------------------------------------------
# 3. awr_unpack_wgrads_batched
# ------------------------------------------------------------------------------------------
def _uj(name, d0, d1, T, ld, slots, stride, buf=None, off=0):
    return dict(name=name, d0=d0, d1=d1, T=T, ld=ld, slots=slots, stride=stride, buf=buf or name, off=off)


HEAD_STRIDE = 64 * 256 + 96      # the head's copies: 64 padded rows of 256 floats, and a stride larger than the copy
UNPACK_JOBS = [
    _uj("a", 96, 64, 9, 64, 1, 0),                                   # the baseline
    _uj("c1", 1, 42, 1, 42, 3, 64, buf="c"),                         # the two bias jobs of a head over one buffer: d0 = 1, d1 not a multiple of 4
    _uj("d1", 42, 256, 1, 256, 4, HEAD_STRIDE, buf="d"),             # the head's two weight jobs over one buffer
    _uj("b", 14, 120, 1, 128, 1, 0),                                 # ld > d1
    _uj("d2", 14, 256, 1, 256, 4, HEAD_STRIDE, buf="d", off=42 * 256),
    _uj("e1", 3, 928, 9, 928, 2, 3 * 9 * 928 + 32),                  # the column-chunk loop (896 + 32), which no network reaches
    _uj("f", 7, 21, 9, 32, 2, 7 * 9 * 32 + 32),                      # d1 odd
    _uj("e2", 2, 512, 16, 512, 5, 2 * 16 * 512 + 160),               # chunks at T = 16 (480 + 32), five copies
    _uj("e3", 3, 928, 9, 960, 3, 3 * 9 * 960 + 64),                  # the chunk loop with ld > d1; three copies, so their order counts here too
    _uj("c2", 1, 14, 1, 14, 3, 64, buf="c", off=42),                 # a one-row job last
]


def _spread(shape, g):
    """values whose exponents are spread over 2^+-12: the order of an fp32 sum of them changes its bits"""
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return sign * torch.exp2(torch.rand(shape, generator=g) * 24 - 12) * (1 + torch.rand(shape, generator=g))


def sum_ref(copies, order):
    """fp32, one add at a time, in the given slot order; returned in checkpoint layout grad[a][b][t] = packed[a][t][b]"""
    acc = copies[order[0]].clone()
    for k in order[1:]:
        acc = acc + copies[k]
    return acc.permute(0, 2, 1).contiguous()


def _unpack_inputs(dev, jobs, seed):
    """the copies of every job, laid into NaN arenas (one per packed buffer) so that a wrong stride, row pitch or column reads NaN"""
    g = torch.Generator().manual_seed(seed)
    copies = {j["name"]: [_spread((j["d0"], j["T"], j["d1"]), g) for _ in range(j["slots"])] for j in jobs}
    size = {}
    for j in jobs:
        size[j["buf"]] = max(size.get(j["buf"], 0), j["off"] + (j["slots"] - 1) * j["stride"] + j["d0"] * j["T"] * j["ld"])
    host = {b: torch.full((n,), float("nan")) for b, n in size.items()}
    for j in jobs:
        for k, c in enumerate(copies[j["name"]]):
            o = j["off"] + k * j["stride"]
            host[j["buf"]][o:o + j["d0"] * j["T"] * j["ld"]].view(j["d0"], j["T"], j["ld"])[:, :, :j["d1"]] = c
    arenas = {b: nan_arena(dev, size[b], host[b]) for b in size}
    return copies, arenas


def launch_unpack(L, dev, jobs, packed_ptr):
    """ONE awr_unpack_wgrads_batched launch; packed_ptr(job) -> device address of slot 0.  Returns {name: (whole, grad)}."""
    grads, table, first = {}, [], 0
    for j in jobs:
        grads[j["name"]] = nan_arena(dev, j["d0"] * j["d1"] * j["T"])
        table.append(L.UnpackJob(packed=packed_ptr(j), grad=L.ptr(grads[j["name"]][1]), d0=j["d0"], d1=j["d1"], T=j["T"], ld=j["ld"], first=first,
                                 slots=j["slots"], slot_stride=j["stride"]))
        first += j["d0"]
    tab = L.job_table(table, dev)
    _KEEP.append(tab)
    L.call("awr_unpack_wgrads_batched", L.ptr(tab), len(table), first, L.stream())
    torch.cuda.synchronize()
    return grads


@pytest.fixture(scope="module")
def unpack_run(L, dev):
    copies, arenas = _unpack_inputs(dev, UNPACK_JOBS, seed=21)
    addr = lambda j: arenas[j["buf"]][1].data_ptr() + 4 * j["off"]      # noqa: E731
    return copies, addr, launch_unpack(L, dev, UNPACK_JOBS, addr)


def test_unpack_inputs_tell_the_order_of_summation(unpack_run):
    """The reference summed in REVERSE slot order must differ from the forward one, or the inputs would not notice a kernel that sums in another
    order.  This can hold from three copies on only: with two, b + a and a + b are the same fp32 sum (IEEE addition commutes), so the two-copy jobs
    (e1, f) check the stride, the pitch and the chunk loop but cannot check the order; c, d, e2 and e3 do, the last two inside the chunk loop."""
    copies = unpack_run[0]
    for j in UNPACK_JOBS:
        fwd = sum_ref(copies[j["name"]], list(range(j["slots"])))
        rev = sum_ref(copies[j["name"]], list(range(j["slots"]))[::-1])
        if j["slots"] >= 3:
            assert not same_bits(fwd, rev), j["name"]
        else:
            assert same_bits(fwd, rev), j["name"]
    assert sum(j["slots"] >= 3 for j in UNPACK_JOBS) == 6


def test_unpack_batched_one_launch_equals_the_ordered_sum(unpack_run):
    copies, _, grads = unpack_run
    for j in UNPACK_JOBS:
        whole, got = grads[j["name"]]
        assert guards_are_nan(whole), j["name"]
        assert same_bits(got, sum_ref(copies[j["name"]], list(range(j["slots"]))).reshape(-1)), j["name"]


@pytest.mark.parametrize("name", [j["name"] for j in UNPACK_JOBS])
def test_unpack_batched_job_alone_and_single_kernel_write_the_same_bits(L, dev, unpack_run, name):
    _, addr, grads = unpack_run
    j = next(x for x in UNPACK_JOBS if x["name"] == name)
    alone = launch_unpack(L, dev, [j], addr)                     # njobs = 1, first = 0
    assert same_bits(alone[name][0], grads[name][0]), name
    if j["slots"] == 1:
        whole, g = nan_arena(dev, j["d0"] * j["d1"] * j["T"])
        L.call("awr_unpack_wgrad", addr(j), j["d0"], j["d1"], j["T"], j["ld"], L.ptr(g), 0, L.stream())
        torch.cuda.synchronize()
        assert same_bits(whole, grads[name][0]), name


def test_unpack_of_pack_returns_the_weights(L, dev, pack_run):
    """every transpose == 0 recipe of the pack table, unpacked with the pack's own ld in one launch"""
    ws, bufs = pack_run
    jobs = [_uj(j["name"], j["d0"], j["d1"], j["T"], j["ld"], 1, 0) for j in PACK_JOBS if not j["tr"] and not j["cols"]]
    assert len(jobs) == 8
    grads = launch_unpack(L, dev, jobs, lambda j: L.ptr(bufs[j["name"]][1]))
    for j in jobs:
        assert guards_are_nan(grads[j["name"]][0]) and same_bits(grads[j["name"]][1], ws[j["name"]].reshape(-1)), j["name"]


# ------------------------------------------------------------------------------------------
# 4. optimiser kernels at their edges
# ------------------------------------------------------------------------------------------
def f32(x):
    """the fp32-rounded scalar the ABI receives, widened to a Python double"""
    return float(np.float32(x))


OPT_N = [3, 7, 4 * 256 * 2, 4 * 256 * 2 + 3, 1000003]      # tail alone in one workgroup; full last workgroups; tail in workgroup 0 among others
E_SAMPLE = 4096      # the fp32 rule's own error E is taken over at least this many elements, so that at n = 3 it is not a matter of luck


def ulp32(a):
    """the fp32 unit in the last place at magnitude a (float64 array), not below the smallest denormal"""
    _, e = np.frexp(a)
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def _opt_inputs(n, seed):
    """parameters of which half lie in [0.5, 2) and half are spread down to 1e-6 (there the update is larger than the parameter and its own
    error shows); a gradient per step comes from grad()."""
    N = max(n, E_SAMPLE)
    g = torch.Generator().manual_seed(seed)
    mag = torch.where(torch.rand(N, generator=g) < 0.5, 0.5 + 1.5 * torch.rand(N, generator=g), torch.pow(10.0, -6 * torch.rand(N, generator=g)))
    p = mag * (torch.randint(0, 2, (N,), generator=g).float() * 2 - 1)

    def grad():
        x = torch.randn(N, generator=g) * 0.03
        x[::7] = 0.0      # every seventh gradient element is zero
        return x
    return N, g, p, grad


class _Arenas:
    """device arenas of n floats between NaN guard bands, and the host-side state of N >= n elements: [:n] follows the kernel, the rest the fp32 rule"""

    def __init__(self, dev, n, **host):
        self.n, self.host = n, {k: v.clone() for k, v in host.items()}
        self.dev = {k: nan_arena(dev, n, v[:n]) for k, v in host.items()}

    def ptr(self, L, k):
        return L.ptr(self.dev[k][1])

    def set(self, k, v):      # a read-only input of the next step (the gradient)
        self.host[k] = v
        self.dev[k][1].copy_(v[:self.n])

    def after_step(self, rule32):
        """the kernel's results; the host state becomes the kernel's in [:n] and the fp32 rule's beyond"""
        out = {}
        for k, v in rule32.items():
            out[k] = self.dev[k][1].cpu()
            self.host[k] = torch.cat([out[k], v[self.n:]])
        return out

    def guards_intact(self):
        return all(guards_are_nan(w) for w, _ in self.dev.values())


# THE UNIT of the optimiser errors.  Each error is divided, element by element, by the first-order scale of the rounding error an fp32 evaluation
# of that quantity makes (adam_ref64 / sgd_ref64 compute it in fp64): for a parameter far larger than its update that is the ulp of |p|; where
# terms cancel (g * grad_scale against weight_decay * p, m against the gradient, a parameter smaller than its update) the ulps of the TERMS
# are added, carried through the rule's derivatives.  With the plain ulp of the result the worst element would be whichever cancels most (the
# fp32 rule itself is then thousands of "ulp" off on a few elements of a million) and the bound 2 E + 1 would let a kernel be wrong everywhere.
# In this unit the fp32 torch rule comes out between 0.45 and 1.3 on the CPU for every case below.
def _worst(x, ref64, unit, n=None):
    k = x.numel() if n is None else n
    return float((np.abs(x.double().numpy()[:k] - ref64[:k]) / unit[:k]).max())


def _check(tag, names, rule32, kern, ref64, unit, n, report):
    for k in names:
        E, K = _worst(rule32[k], ref64[k], unit[k]), _worst(kern[k], ref64[k], unit[k], n)
        report.append("%s %s: E=%.3f ulp kernel=%.3f ulp" % (tag, k, E, K))
        # The kernel against fp64 may be at most twice as wrong as the fp32 torch rule is, plus one ulp: it receives lr / bc1 and sqrt(bc2) rounded
        # to fp32 on the host, two roundings the torch rule does not make.  What both measured on the MI355X: MEASURED below.
        assert K <= 2 * E + 1, (tag, k, E, K)


# MEASURED (MI355X, worst over every n, setting, schedule and step of the two tests below; E is the fp32 CPU rule, K the kernel):
#   Adam: E_p 0.46 .. 0.86, K_p <= 0.80;  E_m <= 0.70, K_m <= 0.80;  E_v <= 1.13, K_v <= 1.22
#   SGD:  E_p 0.50 .. 1.30, K_p <= 1.30;  E_buf <= 1.88, K_buf <= 1.88      (in most cases the kernel and the fp32 rule agree to the digit)
ADAM_SETTINGS = [(1e-2, f32(1.0 / 3.0)), (0.0, 0.125), (1e-2, 1.0)]      # (weight_decay, grad_scale)


def adam_ref64(p, g, m, v, step, lr, b1, b2, eps, wd, gs):
    P, G, M, V = (t.double().numpy() for t in (p, g, m, v))
    gr = G * gs + wd * P
    M2 = M + (gr - M) * (1.0 - b1)
    V2 = V * b2 + (1.0 - b2) * gr * gr
    D = np.sqrt(V2) / math.sqrt(1.0 - b2 ** step) + eps
    s = lr / (1.0 - b1 ** step)
    upd = s * (M2 / D)
    ref = dict(p=P - upd, m=M2, v=V2)
    # the error scales (THE UNIT above), with c = sqrt(bc2):
    #   gr = g * gs + wd * p          is rounded at the size of its larger term A:             u(gr) = ulp(A)
    #   m' = m + (gr - m) * (1 - b1)  is linear with weights <= 1:                             u(m') = ulp(max(|m|, |m'|, A))
    #   v' = v * b2 + (1 - b2) * gr^2 is rounded at its own size and carries d(gr^2) = 2 |gr| u(gr):
    #                                                                                          u(v') = ulp(v') + (1 - b2) * 2 |gr| * ulp(A)
    #   D  = sqrt(v') / c + eps       dD/dv' = 1 / (2 sqrt(v') c)  (v' == 0 only with u(v') == 0): u(D) = ulp(D) + u(v') / (2 sqrt(v') c)
    #   p' = p - s * m' / D           d(m'/D) = u(m') / D + |m'| u(D) / D^2:    u(p') = ulp(max(|p|, |p'|)) + ulp(upd) + s * (u(m') / D + |m'| u(D) / D^2)
    A = np.maximum(np.maximum(np.abs(G * gs), np.abs(wd * P)), np.abs(gr))
    um = ulp32(np.maximum(np.maximum(np.abs(M), np.abs(M2)), A))
    uv = ulp32(V2) + (1.0 - b2) * 2.0 * np.abs(gr) * ulp32(A)
    uD = ulp32(D) + np.where(V2 > 0, uv / (2.0 * np.sqrt(np.where(V2 > 0, V2, 1.0)) * math.sqrt(1.0 - b2 ** step)), 0.0)
    up = ulp32(np.maximum(np.abs(P), np.abs(ref["p"]))) + ulp32(upd) + s * (um / D + np.abs(M2) * uD / (D * D))
    unit = dict(p=up, m=um, v=uv)
    return ref, unit


@pytest.mark.parametrize("wd,gs", ADAM_SETTINGS)
@pytest.mark.parametrize("n", OPT_N)
def test_adam_step_edges(L, dev, n, wd, gs):
    lr, b1, b2, eps, wd = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(wd)
    report = []
    for steps in ((1, 2, 3), (1000, 1001)):
        N, gen, p0, grad = _opt_inputs(n, seed=n + steps[0])
        if steps[0] == 1:
            m0, v0 = torch.zeros(N), torch.zeros(N)
        else:
            m0, v0 = torch.randn(N, generator=gen) * 0.01, (torch.randn(N, generator=gen) * 0.01) ** 2
        A = _Arenas(dev, n, p=p0, m=m0, v=v0, g=torch.zeros(N))
        for step in steps:
            A.set("g", grad())
            h = A.host
            ref64, unit = adam_ref64(h["p"], h["g"], h["m"], h["v"], step, lr, b1, b2, eps, wd, gs)
            r32 = dict(p=h["p"].clone(), m=h["m"].clone(), v=h["v"].clone())
            O.adam_update(r32["p"], h["g"] * gs, r32["m"], r32["v"], step, lr=lr, b1=b1, b2=b2, eps=eps, wd=wd)
            L.call("awr_adam_step", A.ptr(L, "p"), A.ptr(L, "g"), A.ptr(L, "m"), A.ptr(L, "v"), n, lr, b1, b2, eps, wd, step, gs, L.stream())
            torch.cuda.synchronize()
            before = h["p"][:n].clone()
            kern = A.after_step(r32)
            _check("adam n=%d wd=%g gs=%g step=%d" % (n, wd, gs, step), ("p", "m", "v"), r32, kern, ref64, unit, n, report)
            if step == 1:      # from zero state |update| is about lr: every element with a gradient, the tail's too, visibly moved
                live = (A.host["g"][:n] != 0) if wd == 0 else torch.ones(n, dtype=torch.bool)
                assert bool((kern["p"] != before)[live].all()) and bool((kern["m"] != 0)[live].all()) and bool((kern["v"] != 0)[live].all())
            assert A.guards_intact()
        if steps[0] == 1 and wd == 0:      # zero state, zero gradient, no decay: 0 / (0 + eps) -- not one bit of those parameters may change
            assert same_bits(A.host["p"][:n][::7], p0[:n][::7])
            assert not bool(A.host["m"][:n][::7].any()) and not bool(A.host["v"][:n][::7].any())
    print("\n".join(report))


SGD_SETTINGS = [(0.9, 0.0, 0.125), (0.9, 1e-2, f32(1.0 / 3.0)), (0.0, 1e-2, 1.0)]      # (momentum, weight_decay, grad_scale)


def sgd_ref64(p, g, buf, first, lr, mom, wd, gs):
    P, G = p.double().numpy(), g.double().numpy()
    old = np.zeros_like(P) if first else buf.double().numpy() * mom
    gr = G * gs + wd * P
    B2 = old + gr
    ref = dict(p=P - lr * B2, buf=B2)
    # the error scales (THE UNIT above):  buf' = mom * buf + gr is a sum, rounded at the size of its largest term (A = the larger term of gr):
    #   u(buf') = ulp(max(|mom * buf|, |buf'|, A));   p' = p - lr * buf':  u(p') = ulp(max(|p|, |p'|)) + ulp(lr * buf') + lr * u(buf')
    A = np.maximum(np.maximum(np.abs(G * gs), np.abs(wd * P)), np.abs(gr))
    ub = ulp32(np.maximum(np.maximum(np.abs(old), np.abs(B2)), A))
    unit = dict(p=ulp32(np.maximum(np.abs(P), np.abs(ref["p"]))) + ulp32(lr * B2) + lr * ub, buf=ub)
    return ref, unit


def sgd_rule32(p, g, buf, first, lr, mom, wd):
    """torch.optim.SGD's single-tensor rule in fp32 on the CPU; in place"""
    if wd != 0.0:
        g = g + wd * p
    if first:
        buf.copy_(g)
    else:
        buf.mul_(mom).add_(g)
    p.add_(buf, alpha=-lr)


@pytest.mark.parametrize("mom,wd,gs", SGD_SETTINGS)
@pytest.mark.parametrize("n", OPT_N)
def test_sgd_step_edges(L, dev, n, mom, wd, gs):
    lr, mom, wd = f32(0.01), f32(mom), f32(wd)
    report = []
    N, gen, p0, grad = _opt_inputs(n, seed=n + 5)
    A = _Arenas(dev, n, p=p0, buf=torch.full((N,), float("nan")), g=torch.zeros(N))      # step 1 must ignore the NaN momentum buffer and overwrite it
    for step in (1, 2, 3):
        A.set("g", grad())
        h = A.host
        ref64, unit = sgd_ref64(h["p"], h["g"], h["buf"], step == 1, lr, mom, wd, gs)
        r32 = dict(p=h["p"].clone(), buf=h["buf"].clone())
        sgd_rule32(r32["p"], h["g"] * gs, r32["buf"], step == 1, lr, mom, wd)
        L.call("awr_sgd_step", A.ptr(L, "p"), A.ptr(L, "g"), A.ptr(L, "buf"), n, lr, mom, wd, step, gs, L.stream())
        torch.cuda.synchronize()
        kern = A.after_step(r32)
        assert not bool(torch.isnan(kern["buf"]).any()) and not bool(torch.isnan(kern["p"]).any())
        _check("sgd n=%d mom=%g wd=%g gs=%g step=%d" % (n, mom, wd, gs, step), ("p", "buf"), r32, kern, ref64, unit, n, report)
        assert A.guards_intact()
    print("\n".join(report))


# ------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------
def test_batched_entry_points_refuse_empty_tables(L, dev):
    w = torch.randn(4, 32, 1)
    src = w.to(dev)
    wp, dst = nan_arena(dev, 4 * 32)
    ptab = L.job_table([L.PackJob(src=L.ptr(src), dst=L.ptr(dst), split=None, d0=4, d1=32, T=1, transpose=0, rows=4, ld=32, first=0, cols=0,
                                  reserved=0)], dev)
    wg, grad = nan_arena(dev, 4 * 32)
    utab = L.job_table([L.UnpackJob(packed=L.ptr(src), grad=L.ptr(grad), d0=4, d1=32, T=1, ld=32, first=0, slots=1, slot_stride=0)], dev)
    for entry, tab in (("awr_pack_weights_batched", ptab), ("awr_unpack_wgrads_batched", utab)):
        for args in ((None, 1, 4), (L.ptr(tab), 0, 4), (L.ptr(tab), 1, 0)):
            assert getattr(L.lib, entry)(args[0], args[1], args[2], L.stream()) != 0, (entry, args[1:])
            assert "batched" in L.last_error(), (entry, args[1:])
            with pytest.raises(L.AwrError):
                L.call(entry, args[0], args[1], args[2], L.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(wp.cpu()).all()) and bool(torch.isnan(wg.cpu()).all())
