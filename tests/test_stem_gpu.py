"""GPU checks of the fused stem kernels (csrc/awr_stem.hip: stem_stats_kernel, stem_conv_kernel, stem_pool_kernel, stem_bwd_kernel<0|1, dense|
pooled>, stem_dw_finalize_kernel) through the C ABI, against float64 torch on the CPU -- the bodies and references of tests/stem_cases.py
(checked themselves by tests/test_stem_cases_cpu.py).  Next to test_fused_stem_* of tests/test_ops_gpu.py (tile counts 6, 64, 1) these run odd
tile counts above 1, tall, one-tile-wide and one-tile-high maps, every slot-count form, the argmax bytes exactly, ties that reach the
gradients, and the refusals.

Every case prints its figures as a `stem <test> <B>x<H>x<W> name=value ...` line (pytest -s), tests 1 and 3 with the error of float32 torch
against float64 behind each figure (`name=kernel/float32`); profiles/stem_errors.txt is the table of those lines."""
import ctypes as C

import pytest
import torch

import stem_cases as SC
from stem_cases import SHAPES, SLOT_SHAPES, shape_id

pytestmark = pytest.mark.gpu

IDS = [shape_id(s) for s in SHAPES]
FORMS = [True, False]
FORM_IDS = ["pooled", "dense"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    import awr_amd  # noqa: F401
    from awr_amd import _lib
    return _lib


def report(test, inp, f, e32=None):
    e32 = e32 or {}
    print("stem %s %s %s" % (test, shape_id((inp.B, inp.H, inp.W)),
                             " ".join("%s=%.3g" % (k, v) + ("/%.3g" % e32[k] if k in e32 else "") for k, v in sorted(f.items()))))


# ---- 1. the whole chain at every shape ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooled", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_stem_chain_matches_float64(L, dev, shape, pooled):
    """Mean, variance, pooled or dense map, dgamma, dbeta, dW (twice), dbias under identity coefficients and the re-armed accumulators, at the
    bounds of the existing stem tests."""
    inp = SC.reference(pooled, *shape)
    f = SC.stem_chain(L, dev, inp)
    report("chain_%s" % ("pooled" if pooled else "dense"), inp, f, inp.e32)
    SC.assert_figures(f)


# ---- 2. the pooling kernel is exactly a max-pool of what the dense kernel writes ---------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_stem_pool_is_exactly_maxpool_of_stem_conv(L, dev, shape):
    """Same filters, scale and shift: stem_pool_kernel's map is torch.equal to max_pool2d (float32, CPU) of stem_conv_kernel's map, and its
    argmax bytes are the codes of torch's indices -- the first maximum in scan order, from the right start on the top and left border.  Scales
    of both signs; eight channels tie the whole window above the ReLU (scale 0, shift > 0), eight at its zero (scale 0, shift < 0); the
    constant top third of the image ties whole windows in every other channel."""
    inp = SC.reference(True, *shape)
    f = SC.pool_is_maxpool_of_dense(L, dev, inp)
    report("pool_exact", inp, f)
    assert f["dense"] < SC.BOUNDS["map"]
    assert f["map_differs"] == 0 and f["tie_values"] == 0
    assert f["argmax_differs"] == 0 and f["tie_channels_differ"] == 0


# ---- 3. ties are routed like torch routes them, down to the gradients --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_stem_tie_routing_reaches_the_gradients(L, dev, shape):
    """gamma = [0, -g, g, 0, ...], beta of both signs: a gamma = 0, beta > 0 channel is an exact tie in every window for float64 torch and for
    the kernel alike, and its dgamma = sum g * xhat depends on which element the gradient is routed to (tests/test_stem_cases_cpu.py: last
    instead of first moves it by more than 1e-2 of the largest dgamma)."""
    inp = SC.reference(True, *shape, "ties")
    f = SC.stem_chain(L, dev, inp)
    report("ties", inp, f, inp.e32)
    SC.assert_figures(f)


# ---- 4. slot counts ----------------------------------------------------------------------------------------------------------------------------
def _slots(L, B, H, W):
    ss, ws = C.c_int(-1), C.c_int(-1)
    L.call("awr_stem_slots", B, H, W, C.byref(ss), C.byref(ws))
    return ss.value, ws.value


@pytest.mark.parametrize("shape", SLOT_SHAPES, ids=shape_id)
def test_stem_slots_counts(L, shape):
    B, H, W = shape
    ss, ws = _slots(L, B, H, W)
    tiles = SC.tiles_of(H, W)
    assert ss == tiles * B
    assert ws > 0 and ss % ws == 0 and ss // ws in SC.WG_TILES and tiles % (ss // ws) == 0


@pytest.mark.parametrize("pooled", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", SLOT_SHAPES, ids=shape_id)
def test_stem_chain_with_every_slot_count(L, dev, shape, pooled):
    """nslots = 1, 3, 16 and the two counts of awr_stem_slots, each accumulator with exactly that many copies: same results, same bounds, the
    copies behind them untouched, the ones used re-armed."""
    inp = SC.reference(pooled, *shape)
    for nslots in sorted({1, 3, 16} | set(_slots(L, *shape))):
        f = SC.stem_chain(L, dev, inp, nslots)
        report("slots%d_%s" % (nslots, "pooled" if pooled else "dense"), inp, f)
        SC.assert_figures(f)


# ---- 5. deterministic slots: one copy per workgroup --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooled", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", SLOT_SHAPES, ids=shape_id)
def test_stem_deterministic_slots_hold_one_workgroup_each(L, dev, shape, pooled):
    """nslots = awr_stem_slots: the raw slot arrays of the statistics and of the BN-backward sums, before any finalize, are a prefix of
    per-workgroup sums over t consecutive tiles of one image (t found from the number of used slots) and bitwise the same in two runs; the
    weight gradient with wgrad_slots copies is bitwise the same in two runs."""
    inp = SC.reference(pooled, *shape)
    f = SC.deterministic_slots(L, dev, inp)
    report("det_%s" % ("pooled" if pooled else "dense"), inp, f)
    for k in SC.SLOT_EXACT:
        assert f[k] == 0.0, (k, f[k])
    for k, bound in SC.SLOT_BOUNDS.items():
        assert f[k] < bound, (k, f[k], bound)


# ---- 6. the accumulators accumulate ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooled", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", [(2, 48, 16), (3, 48, 32), (2, 64, 64)], ids=shape_id)
def test_stem_sums_add_to_what_the_accumulator_holds(L, dev, shape, pooled):
    """Deterministic-slot mode: two launches (different images, weights and gradients) onto one array give exactly the float64 sum of their
    separate arrays; a launch onto a pre-filled array exactly pre-fill + its own array.  Statistics and BN-backward sums."""
    f = SC.accumulate(L, dev, SC.reference(pooled, *shape), SC.reference(pooled, *shape, "alt"))
    report("accumulate_%s" % ("pooled" if pooled else "dense"), SC.reference(pooled, *shape), f)
    for k, v in f.items():
        assert v == 0.0, (k, v)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
class _Refusals:
    """Buffers for a (2, 48, 48) call, outputs and accumulators filled with NaN; every entry point as a function of (B, H, W) and of the name
    of one pointer to pass as NULL."""

    B, H, W = 2, 48, 48

    def __init__(self, L, dev):
        self.L = L
        B, H, W = self.B, self.H, self.W
        nan32 = lambda *s: torch.full(s, float("nan"), device=dev)                                # noqa: E731
        self.inputs = dict(img=torch.ones(B, 1, H, W, device=dev), w=torch.ones(64, 25, device=dev), bias=torch.zeros(64, device=dev),
                           scale=torch.ones(64, device=dev), shift=torch.zeros(64, device=dev), coef4=torch.ones(4, 64, device=dev),
                           coef=torch.ones(3, 64, device=dev), dg=torch.ones(B, H, W, 64, device=dev),
                           arg=torch.zeros(B, H // 2, W // 2, 64, device=dev, dtype=torch.uint8))
        self.outputs = dict(stats=torch.full((B * 9 * 128,), float("nan"), device=dev, dtype=torch.float64),
                            sums=torch.full((B * 9 * 128,), float("nan"), device=dev, dtype=torch.float64),
                            out=nan32(B, H, W, 64), pooled=nan32(B, H // 2, W // 2, 64), dw=nan32(B * 9 * 64 * 26), grad=nan32(64, 25), gbias=nan32(64))
        self.argmax_out = torch.full((B, H // 2, W // 2, 64), 255, device=dev, dtype=torch.uint8)
        self.ss, self.ws = C.c_int(-7), C.c_int(-7)

    def p(self, name, null):
        if name == null:
            return None
        t = self.inputs.get(name, self.outputs.get(name))
        return self.L.ptr(self.argmax_out if name == "argmax_out" else t)

    def entries(self):
        L, s = self.L, self.L.stream()

        def slots(B, H, W, null=None):
            L.call("awr_stem_slots", B, H, W, None if null == "stats_slots" else C.byref(self.ss), None if null == "wgrad_slots" else C.byref(self.ws))

        def stats(B, H, W, null=None, nslots=0):
            p = lambda n: self.p(n, null)                                                            # noqa: E731
            L.call("awr_stem_stats", p("img"), p("w"), p("bias"), B, H, W, p("stats"), nslots, s)

        def conv(B, H, W, null=None):
            p = lambda n: self.p(n, null)                                                            # noqa: E731
            L.call("awr_stem_conv", p("img"), p("w"), p("bias"), p("scale"), p("shift"), 1, B, H, W, p("out"), s)

        def pool(B, H, W, null=None):
            p = lambda n: self.p(n, null)                                                            # noqa: E731
            L.call("awr_stem_pool", p("img"), p("w"), p("scale"), p("shift"), B, H, W, p("pooled"), p("argmax_out"), s)

        def reduce(B, H, W, null=None, nslots=0):
            p = lambda n: self.p(n, null)                                                            # noqa: E731
            L.call("awr_stem_bwd_reduce", p("img"), p("w"), p("bias"), p("coef4"), p("dg"), p("arg"), B, H, W, p("sums"), nslots, s)

        def wgrad(B, H, W, null=None, nslots=0):
            p = lambda n: self.p(n, null)                                                            # noqa: E731
            L.call("awr_stem_bwd_wgrad", p("img"), p("w"), p("bias"), p("coef4"), p("coef"), p("dg"), p("arg"), B, H, W, p("dw"), p("grad"), p("gbias"), nslots, s)

        # entry: (call, its required pointers, takes nslots, the output a served call fills)
        return dict(slots=(slots, ["stats_slots", "wgrad_slots"], False, None), stats=(stats, ["img", "w", "stats"], True, "stats"),
                    conv=(conv, ["img", "w", "scale", "shift", "out"], False, "out"), pool=(pool, ["img", "w", "scale", "shift", "pooled"], False, "pooled"),
                    reduce=(reduce, ["img", "w", "coef4", "dg", "sums"], True, "sums"),
                    wgrad=(wgrad, ["img", "w", "coef4", "coef", "dg", "dw", "grad"], True, "grad"))

    def untouched(self):
        torch.cuda.synchronize()
        return (all(bool(torch.isnan(t).all()) for t in self.outputs.values()) and bool((self.argmax_out == 255).all())
                and self.ss.value == -7 and self.ws.value == -7)

    def served(self, call, written):
        """the call with nothing wrong, onto zeroed accumulators: its output is finite and not all zero"""
        for name in ("stats", "sums", "dw"):
            self.outputs[name].zero_()
        call(self.B, self.H, self.W)
        torch.cuda.synchronize()
        if written is None:
            return (self.ss.value, self.ws.value) == (self.B * 9, self.B * 9)
        t = self.outputs[written]
        return bool(torch.isfinite(t).all()) and bool((t != 0).any())


@pytest.fixture
def refusals(L, dev):
    return _Refusals(L, dev)


@pytest.mark.parametrize("entry", ["slots", "stats", "conv", "pool", "reduce", "wgrad"])
def test_stem_refusals_come_before_any_launch(L, refusals, entry):
    """H or W of 0, 8, 24, 40 (no positive multiple of 16), B = 0, a negative B or slot count, each required pointer NULL: AwrError, and neither
    an output nor an accumulator (all NaN) has been written.  The same call with nothing wrong is served and writes its output."""
    R = refusals
    call, required, has_nslots, written = R.entries()[entry]
    for bad in (0, 8, 24, 40):
        for B, H, W in ((R.B, bad, R.W), (R.B, R.H, bad), (R.B, bad, bad)):
            with pytest.raises(L.AwrError):
                call(B, H, W)
    for B in (0, -1):
        with pytest.raises(L.AwrError):
            call(B, R.H, R.W)
    for name in required:
        with pytest.raises(L.AwrError):
            call(R.B, R.H, R.W, null=name)
    if has_nslots:
        with pytest.raises(L.AwrError):
            call(R.B, R.H, R.W, nslots=-1)
    assert R.untouched()
    assert R.served(call, written)
