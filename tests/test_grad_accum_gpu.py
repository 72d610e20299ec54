"""Gradient accumulation and global-norm clipping on the device, through the C ABI and through TrainEngine.

Operator level: awr_grad_norm against numpy in float64 (bar 1e-9 relative, derived below), its determinism and its clip coefficient;
awr_grad_accumulate and the *_dev optimiser entries BIT for bit against the existing entry points.  Every device buffer a kernel writes sits
between NaN guard bands.  Engine level (deterministic mode): an accumulation window lands on the bits of one hand-built awr_adam_step over the
micro-batch gradients added in order, ragged windows and flush() included; clipping lands on the bits of awr_adam_step with the coefficient
the device computed."""
import math

import numpy as np
import pytest
import torch

import awr_oracle as O

pytestmark = pytest.mark.gpu

_KEEP = []
GUARD = 64      # guard elements in front of and behind every target (a multiple of 4 floats: the arenas stay 16-byte aligned)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    import awr_amd  # noqa: F401
    from awr_amd import _lib
    return _lib


def nan_arena(dev, n, host=None, dtype=torch.float32):
    """(whole, target): n elements (NaN, or `host`) between two NaN guard bands; kept alive until the module is torn down"""
    whole = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype)
    if host is not None:
        whole[GUARD:GUARD + n] = host.reshape(-1)
    whole = whole.to(dev)
    _KEEP.append(whole)
    return whole, whole[GUARD:GUARD + n]


def guards_are_nan(whole):
    w = whole.cpu()
    return bool(torch.isnan(w[:GUARD]).all() and torch.isnan(w[-GUARD:]).all())


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def f32(x):
    """the fp32-rounded scalar the ABI receives, widened to a Python double"""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------
# 1. awr_grad_norm
# ------------------------------------------------------------------------------------------
# tail only; exactly one float4; a float4 and a tail; one workgroup; one workgroup and a tail; several workgroups; 1024 workgroups that each loop twice
NORM_N = [1, 3, 4, 5, 255, 1024, 1027, 65537, (1 << 21) + 3]
# THE BAR (derived, not measured): float64 products of float32 values are exact, and a sum of at most 2^21 + 3 non-negative float64 terms is off by
# at most n * 2^-53 ~ 2.3e-10 relative in any order -- the kernel's and numpy's alike.  The square root and the product with grad_scale add a few 2^-53.
NORM_REL = 1e-9


def _norm_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda: torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 8 - 6)      # noqa: E731  randn * 10^U(-6, 2)
    return mk(), mk()


class _Norm:
    """one set of device buffers for awr_grad_norm over n elements, all between guard bands"""

    def __init__(self, L, dev, n, g, g2):
        self.L, self.n = L, n
        self.g = nan_arena(dev, n, g)
        self.g2 = nan_arena(dev, n, g2) if g2 is not None else None
        nscr = int(L.lib.awr_grad_norm_scratch(n))
        assert 0 < nscr <= 8192 and nscr % 8 == 0
        self.scratch = nan_arena(dev, nscr // 8, dtype=torch.float64)
        self.norm = nan_arena(dev, 1, dtype=torch.float64)
        self.scale = nan_arena(dev, 1)

    def __call__(self, gs, max_norm):
        L = self.L
        L.call("awr_grad_norm", L.ptr(self.g[1]), L.ptr(self.g2[1]) if self.g2 else None, self.n, gs, max_norm, L.ptr(self.scratch[1]),
               L.ptr(self.norm[1]), L.ptr(self.scale[1]), L.stream())
        torch.cuda.synchronize()
        return self.norm[1].cpu().clone(), self.scale[1].cpu().clone()

    def guards_intact(self):
        return all(guards_are_nan(a[0]) for a in (self.g, self.g2, self.scratch, self.norm, self.scale) if a is not None)


def clip_formula(norm, max_norm):
    """section 1 of the design on the host, from the device's own float64 norm -> the float32 coefficient"""
    if not math.isfinite(norm):
        return np.float32("nan")
    if max_norm <= 0 or max_norm == float("inf"):
        return np.float32(1.0)
    c = max_norm / (norm + 1e-6)
    return np.float32(c) if c < 1.0 else np.float32(1.0)


@pytest.mark.parametrize("gs", [1.0, f32(1.0 / 3.0)])
@pytest.mark.parametrize("with_g2", [False, True])
@pytest.mark.parametrize("n", NORM_N)
def test_grad_norm_against_float64_numpy(L, dev, n, with_g2, gs):
    g, g2 = _norm_inputs(n, seed=n + 17)
    if not with_g2:
        g2 = None
    run = _Norm(L, dev, n, g, g2)
    e = g.numpy() if g2 is None else (g.numpy() + g2.numpy())          # the float32 add the optimiser kernel makes
    assert e.dtype == np.float32
    ref = np.float64(gs) * np.sqrt(np.sum(e.astype(np.float64) ** 2))
    norm, scale = run(gs, 0.0)
    N = float(norm)
    rel = abs(N - ref) / ref
    print("n=%d g2=%s gs=%g: norm %.17g ref %.17g rel %.3e" % (n, with_g2, gs, N, ref, rel))
    assert rel <= NORM_REL
    assert same_bits(scale, torch.tensor([1.0]))                          # max_norm = 0: no clipping
    norm2, _ = run(gs, 0.0)
    assert same_bits(norm, norm2)                                         # two calls: bitwise equal
    for max_norm in (0.5 * N, 2.0 * N, 0.0, float("inf")):
        nrm, sc = run(gs, max_norm)
        assert same_bits(nrm, norm)
        want = clip_formula(N, max_norm)
        assert same_bits(sc, torch.tensor([float(want)], dtype=torch.float32)), (max_norm, float(sc), float(want))
        if max_norm == 0.5 * N:
            assert 0.0 < float(sc) < 1.0
        if max_norm == 2.0 * N and N >= 1e-6:                             # 2 N / (N + 1e-6) >= 1: exactly 1.0f
            assert float(sc) == 1.0
    assert run.guards_intact()


@pytest.mark.parametrize("with_g2", [False, True])
@pytest.mark.parametrize("n", NORM_N)
def test_grad_norm_keeps_a_nan_visible(L, dev, n, with_g2):
    g, g2 = _norm_inputs(n, seed=n + 18)
    g[n // 2] = float("nan")
    run = _Norm(L, dev, n, g, g2 if with_g2 else None)
    for max_norm in (1.0, 0.0, float("inf")):
        norm, scale = run(1.0, max_norm)
        assert math.isnan(float(norm)) and math.isnan(float(scale)), max_norm
    assert run.guards_intact()


# ------------------------------------------------------------------------------------------
# 2. awr_grad_accumulate
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 1027])
def test_grad_accumulate(L, dev, n):
    gen = torch.Generator().manual_seed(n)
    g1, g2 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    wa, acc = nan_arena(dev, n)                       # NaN: first = 1 must overwrite it without reading it
    wg, g = nan_arena(dev, n, g1)
    L.call("awr_grad_accumulate", L.ptr(acc), L.ptr(g), n, 1, L.stream())
    torch.cuda.synchronize()
    assert same_bits(acc, g1) and same_bits(g, g1)
    g.copy_(g2)
    want = acc + g                                    # the device's own float32 add
    L.call("awr_grad_accumulate", L.ptr(acc), L.ptr(g), n, 0, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(acc, want) and same_bits(acc, g1 + g2) and same_bits(g, g2)
    assert guards_are_nan(wa) and guards_are_nan(wg)


# ------------------------------------------------------------------------------------------
# 3. awr_adam_step_dev / awr_sgd_step_dev
# ------------------------------------------------------------------------------------------
GS, DS = f32(1.0 / 3.0), f32(0.37)
GS_TIMES_DS = float(np.float32(GS) * np.float32(DS))      # the float32 product the kernel makes


def _dev_inputs(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    grads = [(torch.randn(n, generator=gen) * 0.03, torch.randn(n, generator=gen) * 0.03) for _ in range(2)]
    return p, grads


# (g2 given, dev_scale given): the four instantiations of the one kernel body
FORMS = [(False, False), (True, True), (True, False), (False, True)]


@pytest.mark.parametrize("has_g2,has_ds", FORMS)
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("n", [5, 1027])
def test_adam_step_dev_equals_the_existing_entry_point(L, dev, n, wd, has_g2, has_ds):
    """(a) g2 = NULL, dev_scale = NULL: the bits of awr_adam_step.  (b) with g2 and dev_scale = d: the bits of awr_adam_step fed the device
    float32 sum g + g2 and grad_scale = float32(gs) * float32(d); and each option alone.  Steps 1 and 2, each arm on its own state."""
    lr, b1, b2, eps, wd = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(wd)
    p0, grads = _dev_inputs(n, seed=3 * n + 1)
    (wp, p), (wm, m), (wv, v) = nan_arena(dev, n, p0), nan_arena(dev, n, torch.zeros(n)), nan_arena(dev, n, torch.zeros(n))
    (wg, g), (wh, h) = nan_arena(dev, n), nan_arena(dev, n)
    wd_, d = nan_arena(dev, 1, torch.tensor([DS]))
    rp, rm, rv = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for step, (ga, gb) in enumerate(grads, 1):
        g.copy_(ga)
        h.copy_(gb)
        L.call("awr_adam_step_dev", L.ptr(p), L.ptr(g), L.ptr(h) if has_g2 else None, L.ptr(d) if has_ds else None, L.ptr(m), L.ptr(v), n,
               lr, b1, b2, eps, wd, step, GS, L.stream())
        rg = (g + h) if has_g2 else g.clone()
        L.call("awr_adam_step", L.ptr(rp), L.ptr(rg), L.ptr(rm), L.ptr(rv), n, lr, b1, b2, eps, wd, step, GS_TIMES_DS if has_ds else GS, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(p, rp) and torch.equal(m, rm) and torch.equal(v, rv), step
        assert not same_bits(p, p0) and same_bits(g, ga) and same_bits(h, gb)
        assert all(guards_are_nan(w) for w in (wp, wm, wv, wg, wh, wd_))


@pytest.mark.parametrize("has_g2,has_ds", FORMS)
@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("n", [5, 1027])
def test_sgd_step_dev_equals_the_existing_entry_point(L, dev, n, mom, has_g2, has_ds):
    lr, mom, wd = f32(0.01), f32(mom), f32(1e-2)
    p0, grads = _dev_inputs(n, seed=3 * n + 2)
    (wp, p), (wb, buf) = nan_arena(dev, n, p0), nan_arena(dev, n)          # step 1 must ignore the NaN momentum buffer and overwrite it
    (wg, g), (wh, h) = nan_arena(dev, n), nan_arena(dev, n)
    wd_, d = nan_arena(dev, 1, torch.tensor([DS]))
    rp, rbuf = p0.to(dev), torch.full((n,), float("nan"), device=dev)
    for step, (ga, gb) in enumerate(grads, 1):
        g.copy_(ga)
        h.copy_(gb)
        L.call("awr_sgd_step_dev", L.ptr(p), L.ptr(g), L.ptr(h) if has_g2 else None, L.ptr(d) if has_ds else None, L.ptr(buf), n, lr, mom, wd,
               step, GS, L.stream())
        rg = (g + h) if has_g2 else g.clone()
        L.call("awr_sgd_step", L.ptr(rp), L.ptr(rg), L.ptr(rbuf), n, lr, mom, wd, step, GS_TIMES_DS if has_ds else GS, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(p, rp) and torch.equal(buf, rbuf), step
        assert not bool(torch.isnan(p).any()) and not bool(torch.isnan(buf).any()) and not same_bits(p, p0)
        assert all(guards_are_nan(w) for w in (wp, wb, wg, wh, wd_))


# ------------------------------------------------------------------------------------------
# 4. TrainEngine: accumulation windows, flush(), clipping
# ------------------------------------------------------------------------------------------
SEED, B, S, J = 1234, 2, 128, 14


@pytest.fixture(scope="module")
def det():
    """deterministic mode for every engine test of the module: two nets built from the same seed run the same bits"""
    import awr_amd
    awr_amd.set_deterministic(True)
    try:
        yield awr_amd
    finally:
        awr_amd.set_deterministic(False)


def _net(awr_amd):
    torch.manual_seed(SEED)
    return awr_amd.get_deconv_net(18, J, 2).cuda()


def _engine(net, **kw):
    from awr_amd.trainer import TrainEngine
    kw.setdefault("lr", 1e-3)
    return TrainEngine(net, B, S, 1.0, coord_weight=1.0, use_graph=False, autotune=False, **kw)


def _batch(seed, b=B):
    img, jt = O.synth_batch(b, S, J, seed=seed)
    return img.cuda(), jt.cuda()


def _state(net, eng):
    n = net.n_active
    return net.flat_params()[:n].clone(), eng.m[:n].clone(), eng.v[:n].clone()


class _Twin:
    """Net B of the design: the same seed, a plain engine with SGD at lr = 0 -- its parameters never move, so the gradient arena after each
    of its steps is that micro-batch's gradient at the parameters it holds."""

    def __init__(self, awr_amd):
        self.net = _net(awr_amd)
        self.eng = _engine(self.net, optimizer="sgd", lr=0.0, momentum=0.0, weight_decay=0.0)
        self.n = self.net.n_active

    def follow(self, net):
        """take over another net's parameters (BatchNorm buffers must already agree)"""
        self.net.flat_params().copy_(net.flat_params())
        self.net.weights_changed()

    def grad(self, seed, b=B):
        before = self.net.flat_params()[:self.n].clone()
        self.eng.step(*_batch(seed, b))
        assert torch.equal(self.net.flat_params()[:self.n], before)
        return self.net.flat_grads()[:self.n].clone()


def _adam(L, state, g, step, gs):
    """awr_adam_step, the engine's constants, on clones -> the next (p, m, v)"""
    p, m, v = (t.clone() for t in state)
    L.call("awr_adam_step", L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), 1e-3, 0.9, 0.999, 1e-8, 0.0, step, gs, L.stream())
    torch.cuda.synchronize()
    return p, m, v


def _ordered_sum(grads):
    acc = grads[0]
    for g in grads[1:]:
        acc = acc + g          # ((g1 + g2) + g3): the order the window adds them in
    return acc


def _assert_state(net, eng, want):
    for got, exp, name in zip(_state(net, eng), want, ("params", "m", "v")):
        assert torch.equal(got, exp), name


@pytest.mark.parametrize("k", [2, 3])
def test_accumulation_window_equals_one_hand_built_step(L, det, k):
    net = _net(det)
    eng = _engine(net, accum_steps=k)
    twin = _Twin(det)
    want = _state(net, eng)
    assert torch.equal(want[0], twin.net.flat_params()[:twin.n])
    seed = 70
    for window in (1, 2):          # the second window applies step 2 of Adam's bias correction
        start, grads = _state(net, eng), []
        for micro in range(1, k + 1):
            assert eng.micro_step == micro - 1
            eng.step(*_batch(seed))
            grads.append(twin.grad(seed))
            seed += 1
            if micro < k:          # nothing but the accumulator moved
                _assert_state(net, eng, start)
                assert eng.step_count == window - 1
        want = _adam(L, want, _ordered_sum(grads), window, 1.0 / k)
        _assert_state(net, eng, want)
        assert not torch.equal(want[0], start[0])
        assert eng.step_count == window and eng.micro_step == 0
        assert torch.equal(net._barena, twin.net._barena)          # every micro-step ran its BatchNorm update
        twin.follow(net)


def test_ragged_micro_batch_shares_the_window(L, det):
    """two images, then one: the child plan adds to the parent's accumulator, and each micro-step weighs 1/2 whatever its batch size"""
    net = _net(det)
    eng = _engine(net, accum_steps=2)
    twin = _Twin(det)
    start = _state(net, eng)
    eng.step(*_batch(80))
    assert eng.micro_step == 1 and eng.step_count == 0
    eng.step(*_batch(81, b=1))
    assert eng.micro_step == 0 and eng.step_count == 1
    grads = [twin.grad(80), twin.grad(81, b=1)]
    _assert_state(net, eng, _adam(L, start, _ordered_sum(grads), 1, 1.0 / 2))
    assert torch.equal(net._barena, twin.net._barena)


def test_flush_applies_a_partly_filled_window(L, det):
    net = _net(det)
    eng = _engine(net, accum_steps=3)
    twin = _Twin(det)
    start = _state(net, eng)
    eng.flush()                                      # nothing pending: nothing happens
    assert eng.step_count == 0
    _assert_state(net, eng, start)
    grads = []
    for seed in (90, 91):
        eng.step(*_batch(seed))
        grads.append(twin.grad(seed))
    assert eng.micro_step == 2 and eng.step_count == 0
    eng.flush()
    want = _adam(L, start, _ordered_sum(grads), 1, 1.0 / 2)
    _assert_state(net, eng, want)
    assert eng.micro_step == 0 and eng.step_count == 1
    eng.flush()                                      # a second flush changes no bit
    _assert_state(net, eng, want)
    assert eng.step_count == 1


def test_optimizer_state_dict_refuses_a_pending_window(L, det):
    net = _net(det)
    eng = _engine(net, accum_steps=2)
    eng.step(*_batch(70))
    with pytest.raises(L.AwrError, match="1 micro-step"):
        eng.optimizer_state_dict()
    eng.flush()
    assert len(eng.optimizer_state_dict()["state"]) > 0


@pytest.fixture(scope="module")
def plain_step(L, det):
    """one step of a plain engine on batch 70 and the gradient it applied: (initial state, state after, gradient, its norm from the operator)"""
    net = _net(det)
    eng = _engine(net)
    start = _state(net, eng)
    eng.step(*_batch(70))
    after = _state(net, eng)
    g = _Twin(det).grad(70)
    assert all(torch.equal(a, b) for a, b in zip(after, _adam(L, start, g, 1, 1.0)))
    dev = g.device
    scr = torch.zeros(int(L.lib.awr_grad_norm_scratch(g.numel())) // 8, dtype=torch.float64, device=dev)
    norm, scale = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, device=dev)
    L.call("awr_grad_norm", L.ptr(g), None, g.numel(), 1.0, 0.0, L.ptr(scr), L.ptr(norm), L.ptr(scale), L.stream())
    torch.cuda.synchronize()
    assert math.isfinite(float(norm)) and float(norm) > 0
    return start, after, g, norm.cpu()


def test_grad_norm_alone_changes_no_bit_and_reports_the_norm(L, det, plain_step):
    _, after, _, norm = plain_step
    net = _net(det)
    eng = _engine(net, grad_norm=True)
    assert math.isnan(float(eng.grad_norm))          # no applying step yet
    eng.step(*_batch(70))
    _assert_state(net, eng, after)
    assert same_bits(eng.grad_norm, norm) and float(eng.clip_scale) == 1.0
    assert eng.grad_norm.dtype == torch.float64 and eng.grad_norm.is_cuda and eng.clip_scale.dtype == torch.float32 and eng.clip_scale.is_cuda


def test_clipping_below_the_norm_scales_the_step(L, det, plain_step):
    start, after, g, norm = plain_step
    net = _net(det)
    eng = _engine(net, clip_grad_norm=0.5 * float(norm))
    eng.step(*_batch(70))
    assert same_bits(eng.grad_norm, norm)
    cs = eng.clip_scale.cpu()
    assert same_bits(cs, torch.tensor([float(clip_formula(float(norm), 0.5 * float(norm)))], dtype=torch.float32)) and 0.0 < float(cs) < 1.0
    want = _adam(L, start, g, 1, float(np.float32(1.0) * np.float32(float(cs))))
    _assert_state(net, eng, want)
    assert not torch.equal(want[2], after[2])        # the clipped step differs from the plain one (v scales with the gradient squared)


def test_clipping_far_above_the_norm_is_the_plain_step(L, det, plain_step):
    _, after, _, norm = plain_step
    net = _net(det)
    eng = _engine(net, clip_grad_norm=1e30)
    eng.step(*_batch(70))
    _assert_state(net, eng, after)
    assert same_bits(eng.grad_norm, norm) and float(eng.clip_scale) == 1.0


def test_defaults_spelled_out_are_the_plain_engine(L, det, plain_step):
    _, after, _, _ = plain_step
    net = _net(det)
    eng = _engine(net, accum_steps=1, clip_grad_norm=None, grad_norm=False)
    eng.step(*_batch(70))
    _assert_state(net, eng, after)
    assert eng.micro_step == 0 and eng.step_count == 1
    eng.flush()
    _assert_state(net, eng, after)
    with pytest.raises(L.AwrError, match="not measured"):
        eng.grad_norm


# ------------------------------------------------------------------------------------------
# 5. Trainer: the config keys reach the engine, the epoch's last window is flushed, the log line
# ------------------------------------------------------------------------------------------
def test_trainer_flushes_the_epochs_last_window_and_logs_the_norm(tmp_path):
    import os
    import re
    from awr_amd.config import Config
    from awr_amd.trainer import SyntheticHands, Trainer

    class Cfg(Config):
        net, kernel_size, batch_size, num_workers, max_epoch, output_dir, load_model, exp_id, use_hipgraph, vis_freq, print_freq = \
            "resnet_18", 1.0, 4, 0, 1, str(tmp_path), "", "accum", False, 0, 1
    tr = Trainer(Cfg(accum_steps=2, clip_grad_norm=1.0), SyntheticHands(10, seed=3), None)
    eng = tr.engine
    assert eng.accum_steps == 2 and eng._max_norm == 1.0
    tr.train()          # batches of 4, 4 and 2 images: one full window, then one micro-step that the end of the epoch flushes
    assert eng.step_count == 2 and eng.micro_step == 0
    assert os.path.exists(os.path.join(tr.work_dir, "epoch_1.pth"))          # (optimizer_state_dict() refuses a pending window)
    log = open(os.path.join(tr.work_dir, "resnet_18_dense.log")).read()
    lines = [l for l in log.splitlines() if l.startswith("[epoch: 01][train loss")]
    assert len(lines) == 3
    norms = [re.search(r"\[coord_loss: [^\]]+\]\[grad norm: ([^\]]+)\]$", l).group(1) for l in lines]
    assert norms[0] == "nan" and all(float(x) > 0 for x in norms[1:])          # no applying step before the first line
    assert "accum_steps:2" in log and "clip_grad_norm:1.0" in log
