"""Weight EMA on the device, through the C ABI, TrainEngine and Trainer.

Operator level: awr_ema_update BIT for bit against numpy float32 `e + (p - e) * w` (three operations, each rounded on its own: with contraction
off no rounding differs), every size at which the kernel takes another path, the arenas between NaN guard bands.  Engine level: the shadow
network follows a host recurrence over the downloaded parameters and buffers bit for bit, with the warm-up schedule, accumulation windows,
flush() and ragged batches; the training state keeps the bits of a run without the EMA; an InferEngine scores the shadow.  Trainer: the
checkpoint keys, the log lines, resuming and load_ema."""
import os

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


def nan_arena(dev, host):
    """(whole, target): `host` between two NaN guard bands on the device; kept alive until the module is torn down"""
    n = host.numel()
    whole = torch.full((n + 2 * GUARD,), float("nan"))
    whole[GUARD:GUARD + n] = host.reshape(-1)
    whole = whole.to(dev)
    _KEEP.append(whole)
    return whole, whole[GUARD:GUARD + n]


def guards_are_nan(whole):
    w = whole.cpu()
    return bool(torch.isnan(w[:GUARD]).all() and torch.isnan(w[-GUARD:]).all())


def bits(t):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------
# 1. awr_ema_update
# ------------------------------------------------------------------------------------------
# tail only; a tail of three; one float4; a float4 and a tail; under one workgroup; exactly one workgroup (of float4s: 1024 floats); one workgroup
# and a tail; many workgroups and a tail.  (The grid is ceil(n / 1024) workgroups, one float4 per thread: no workgroup loops.)
EMA_N = [1, 3, 4, 5, 255, 1024, 1027, 65537]
EMA_W = [float(np.float32(0.9)), float(np.float32(1e-3)), 1.0]


def _inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda: torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 8 - 6)      # noqa: E731  randn * 10^U(-6, 2)
    return mk(), mk()


def _host_ema(e, p, w):
    """numpy float32: a subtract, a multiply and an add, each rounded to float32"""
    e, p, w = np.asarray(e, np.float32), np.asarray(p, np.float32), np.float32(w)
    with np.errstate(invalid="ignore", over="ignore"):
        d = p - e
        d = d * w
        out = e + d
    assert out.dtype == np.float32
    return out


def _device_ema(L, dev, e, p, w):
    (we, de), (wp, dp) = nan_arena(dev, e), nan_arena(dev, p)
    L.call("awr_ema_update", L.ptr(de), L.ptr(dp), e.numel(), w, L.stream())
    torch.cuda.synchronize()
    assert guards_are_nan(we) and guards_are_nan(wp)
    assert same_bits(dp, p)                                   # src is only read
    return de.cpu()


@pytest.mark.parametrize("w", EMA_W)
@pytest.mark.parametrize("n", EMA_N)
def test_ema_update_equals_numpy_float32_bitwise(L, dev, n, w):
    e, p = _inputs(n, seed=n + 31)
    equal = torch.arange(n) % 3 == 0 if n > 1 else torch.zeros(1, dtype=torch.bool)
    p[equal] = e[equal]                                       # elements the average has already reached
    got = _device_ema(L, dev, e, p, w)
    want = _host_ema(e.numpy(), p.numpy(), w)
    assert np.isfinite(want).all()
    assert same_bits(got, want)
    assert same_bits(got[equal], e[equal])                    # p == e: e + 0 * w keeps e's bits
    if w == 1.0 and n > 1:
        assert not same_bits(got, e)
    if n > 1:
        assert not same_bits(got[~equal], e[~equal])


@pytest.mark.parametrize("n", [3, 5, 1027])
def test_ema_update_propagates_non_finite_values_like_numpy(L, dev, n):
    """no guard: NaN and +-Inf in either arena go where numpy float32 puts them (Inf - Inf and 0 * Inf included)"""
    e, p = _inputs(n, seed=n + 32)
    specials = [float("nan"), float("inf"), -float("inf")]
    k = 0
    for i in range(n):                                        # every third element of src, every third (shifted) of ema, some of both
        if i % 3 == 0:
            p[i] = specials[k % 3]
            k += 1
        if i % 3 == 1 or i % 9 == 0:
            e[i] = specials[(k + i) % 3]
    for w in EMA_W:
        got = _device_ema(L, dev, e, p, w).numpy()
        want = _host_ema(e.numpy(), p.numpy(), w)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any()
        fin = ~np.isnan(want)
        assert same_bits(got[fin], want[fin])                 # (+-Inf and the finite elements by bits; a NaN's payload is not compared)
        assert np.isnan(got[np.isnan(p.numpy())]).all()       # a NaN parameter makes its EMA element NaN


# ------------------------------------------------------------------------------------------
# 2. TrainEngine
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
    return TrainEngine(net, B, S, 1.0, coord_weight=1.0, lr=1e-3, use_graph=False, autotune=False, **kw)


def _batch(seed, b=B):
    img, jt = O.synth_batch(b, S, J, seed=seed)
    return img.cuda(), jt.cuda()


class _HostEma:
    """the recurrence on the host: numpy float32 over the downloaded parameter and buffer arenas"""

    def __init__(self, net, decay, warmup):
        self.decay, self.warmup, self.updates = decay, warmup, 0
        self.p, self.b = net.flat_params().cpu().numpy().copy(), net._barena.cpu().numpy().copy()

    def advance(self, net):
        from awr_amd.trainer import ema_decay_at
        w = np.float32(1.0 - ema_decay_at(self.decay, self.updates, self.warmup))
        self.p = _host_ema(self.p, net.flat_params().cpu().numpy(), w)
        self.b = _host_ema(self.b, net._barena.cpu().numpy(), w)
        self.updates += 1

    def check(self, eng):
        sh = eng.ema_net
        assert same_bits(sh.flat_params(), self.p), "EMA parameters"
        assert same_bits(sh._barena, self.b), "EMA buffers"
        assert eng.ema_updates == self.updates
        assert torch.equal(sh._counters, eng.net._counters)


@pytest.mark.parametrize("decay,warmup", [(0.999, True), (0.5, False)])
def test_shadow_follows_the_host_recurrence(det, decay, warmup):
    net = _net(det)
    eng = _engine(net, ema_decay=decay, ema_warmup=warmup)
    sh = eng.ema_net
    assert type(sh) is type(net) and sh is not net and not sh.training and net.training and sh.device == net.device
    assert sh.flat_params().data_ptr() != net.flat_params().data_ptr() and not sh._plans
    assert same_bits(sh.flat_params(), net.flat_params()) and same_bits(sh._barena, net._barena)      # initialisation: a copy
    host = _HostEma(net, decay, warmup)
    host.check(eng)
    for step in range(1, 5):
        before = sh.flat_params().clone()
        eng.step(*_batch(40 + step))
        host.advance(net)
        host.check(eng)
        assert eng.ema_updates == eng.step_count == step
        assert not torch.equal(sh.flat_params(), before) and not torch.equal(sh.flat_params(), net.flat_params())
    assert int(sh._counters[0]) == 4


def test_accumulation_micro_steps_leave_the_shadow_alone(det):
    net = _net(det)
    eng = _engine(net, ema_decay=0.5, accum_steps=2)
    sh = eng.ema_net
    host = _HostEma(net, 0.5, True)
    eng.step(*_batch(50))                            # micro-step: the BatchNorm statistics move, the shadow and its counter do not
    assert eng.micro_step == 1 and eng.ema_updates == 0
    assert same_bits(sh.flat_params(), host.p) and same_bits(sh._barena, host.b)
    assert not torch.equal(sh._barena, net._barena)
    eng.step(*_batch(51))                            # applying step: one update
    host.advance(net)
    host.check(eng)
    assert eng.ema_updates == 1 and eng.step_count == 1
    eng.step(*_batch(52))
    assert eng.micro_step == 1 and eng.ema_updates == 1
    assert same_bits(sh.flat_params(), host.p) and same_bits(sh._barena, host.b)
    eng.flush()                                      # the partly filled window is applied: one more update
    host.advance(net)
    host.check(eng)
    assert eng.ema_updates == 2 and eng.step_count == 2
    eng.flush()                                      # nothing pending: nothing happens
    host.check(eng)


def test_ragged_batch_updates_the_same_shadow(det):
    net = _net(det)
    eng = _engine(net, ema_decay=0.5)
    host = _HostEma(net, 0.5, True)
    eng.step(*_batch(60))
    host.advance(net)
    host.check(eng)
    eng.step(*_batch(61, b=1))                       # one image through the B = 2 engine: the child plan, the parent's shadow and counter
    host.advance(net)
    host.check(eng)
    assert eng.ema_updates == 2 and eng.step_count == 2
    assert eng._children[1]._ema is eng._ema and eng._children[1].ema_net is eng.ema_net


def test_ema_only_reads_the_training_state(det):
    """parameters, m, v, BatchNorm buffers and counters of a run with ema_decay are bit for bit those of the same run without it"""
    runs = []
    for kw in ({}, dict(ema_decay=0.9)):
        net = _net(det)
        eng = _engine(net, **kw)
        for step in range(3):
            eng.step(*_batch(70 + step))
        torch.cuda.synchronize()
        runs.append((net.flat_params().clone(), eng.m.clone(), eng.v.clone(), net._barena.clone(), net._counters.clone()))
    for a, b, name in zip(runs[0], runs[1], ("params", "m", "v", "buffers", "counters")):
        assert torch.equal(a, b), name


def _fresh_from(awr_amd, sd):
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(sd)
    return net.cuda()


def test_infer_engine_scores_the_shadow(det):
    from awr_amd.trainer import InferEngine
    net = _net(det)
    eng = _engine(net, ema_decay=0.5, ema_warmup=False)
    for step in range(2):
        eng.step(*_batch(80 + step))
    img = _batch(90)[0]
    inf = InferEngine(eng.ema_net, B, S, 1.0, use_graph=False, autotune=False)
    jt1 = inf(img).clone()
    ref1 = InferEngine(_fresh_from(det, eng.ema_state_dict()), B, S, 1.0, use_graph=False, autotune=False)(img).clone()
    assert torch.isfinite(jt1).all() and same_bits(jt1, ref1)
    eng.step(*_batch(82))                            # the update marks the shadow's weights changed: the same engine repacks them
    jt2 = inf(img).clone()
    ref2 = InferEngine(_fresh_from(det, eng.ema_state_dict()), B, S, 1.0, use_graph=False, autotune=False)(img).clone()
    assert same_bits(jt2, ref2) and not same_bits(jt2, jt1)
    raw = InferEngine(net, B, S, 1.0, use_graph=False, autotune=False)(img).clone()
    net.train()
    assert not same_bits(raw, jt2)
    assert not eng.ema_net.training


def test_hourglass_clone_on_the_device(det):
    net = det.PoseNet("hourglass_1", J).cuda()
    net._counters.fill_(3)
    twin = net.clone()
    assert type(twin) is type(net) and twin.device == net.device and twin.flat_params().is_cuda and twin.training
    assert (twin.nstack, twin.J, twin.n_params, twin.n_active) == (net.nstack, net.J, net.n_params, net.n_active) and net.n_active < net.n_params
    assert same_bits(twin.flat_params(), net.flat_params()) and same_bits(twin._barena, net._barena) and torch.equal(twin._counters, net._counters)
    assert twin.flat_params().data_ptr() != net.flat_params().data_ptr() and not twin._plans


def test_ema_state_dict_round_trip(L, det):
    net = _net(det)
    eng = _engine(net, ema_decay=0.5)
    for step in range(2):
        eng.step(*_batch(95 + step))
    sd, ref = eng.ema_state_dict(), net.state_dict()
    assert list(sd) == list(ref)
    for k in ref:
        assert sd[k].shape == ref[k].shape and sd[k].dtype == ref[k].dtype, k
        assert sd[k].data_ptr() != eng.ema_net.state_dict()[k].data_ptr() and not sd[k].requires_grad, k
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(ref[k]) == 2, k
    assert any(k.endswith("num_batches_tracked") for k in ref)
    p, b = eng.ema_net.flat_params().clone(), eng.ema_net._barena.clone()
    assert not torch.equal(p, net.flat_params())
    eng.ema_reset()
    assert eng.ema_updates == 0
    assert torch.equal(eng.ema_net.flat_params(), net.flat_params()) and torch.equal(eng.ema_net._barena, net._barena)
    assert torch.equal(eng.ema_net._counters, net._counters)
    eng.load_ema_state_dict(sd, 2)
    assert eng.ema_updates == 2
    assert same_bits(eng.ema_net.flat_params()[:net.n_active], p[:net.n_active]) and same_bits(eng.ema_net._barena, b)
    assert torch.equal(eng.ema_net._counters, net._counters)
    for bad in (-1, True, 1.0):
        with pytest.raises(ValueError, match="updates"):
            eng.load_ema_state_dict(sd, bad)
    plain = _engine(_net(det))
    assert plain._ema is None
    for use in (lambda: plain.ema_net, lambda: plain.ema_updates, plain.ema_state_dict, plain.ema_reset, lambda: plain.load_ema_state_dict(sd, 0)):
        with pytest.raises(L.AwrError, match="ema_decay"):
            use()


# ------------------------------------------------------------------------------------------
# 3. Trainer: config keys, log lines, checkpoint keys, resuming, load_ema
# ------------------------------------------------------------------------------------------
def _cfg(tmp, exp_id, **over):
    from awr_amd.config import Config

    class Cfg(Config):
        net, kernel_size, batch_size, num_workers, max_epoch, output_dir, load_model, use_hipgraph, vis_freq, print_freq = \
            "resnet_18", 1.0, 4, 0, 1, str(tmp), "", False, 0, 1
    return Cfg(exp_id=exp_id, **over)


def _log_text(tr):
    tr.log.flush()          # (a Trainer that has not trained yet has only buffered its init lines)
    return open(os.path.join(tr.work_dir, "resnet_18_dense.log")).read()


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """one epoch over 10 synthetic hands in batches of 4, 4 and 2 with ema_decay = 0.9 -> (tmp dir, checkpoint path, trainer)"""
    from awr_amd.trainer import SyntheticHands, Trainer
    tmp = tmp_path_factory.mktemp("ema")
    tr = Trainer(_cfg(tmp, "ema", ema_decay=0.9, test_loss=True), SyntheticHands(10, seed=3), SyntheticHands(6, seed=4))
    tr.train()
    torch.cuda.synchronize()
    return tmp, os.path.join(tr.work_dir, "epoch_1.pth"), tr


def test_trainer_checkpoint_and_log(trained):
    tmp, path, tr = trained
    pth = torch.load(path, map_location="cpu", weights_only=False)
    assert set(pth) == {"model", "optimizer", "best_records", "model_ema", "ema_updates"}
    assert pth["ema_updates"] == 3 == tr.engine.ema_updates == tr.engine.step_count
    assert list(pth["model_ema"]) == list(pth["model"])
    assert any(not torch.equal(pth["model_ema"][k], pth["model"][k]) for k in pth["model"])
    log = _log_text(tr).splitlines()
    assert log.count("weight EMA: decay 0.9, warm-up on") == 1
    assert len([l for l in log if l.startswith("[epoch  1], [test mpe ema ")]) == 1
    assert len([l for l in log if l.startswith("[epoch  1], [test mpe ") and "ema" not in l and l.endswith("]") and "[lr " in l]) == 1
    assert len([l for l in log if l.startswith("[epoch  1], [test loss ema ")]) == 1 and len([l for l in log if l.startswith("[epoch  1], [test loss ")]) == 2
    assert "ema_decay:0.9" in log and "ema_warmup:True" in log and "load_ema:False" in log
    assert os.path.exists(os.path.join(tr.work_dir, "test_pck_epoch_1.png")) and os.path.exists(os.path.join(tr.work_dir, "test_pck_ema_epoch_1.png"))
    assert tr.last_test_mpe_ema == tr.last_test_mpe_ema and tr.net.training and not tr.engine.ema_net.training


def test_trainer_resumes_the_shadow_and_load_ema(trained):
    from awr_amd.trainer import Trainer
    tmp, path, _ = trained
    pth = torch.load(path, map_location="cpu", weights_only=False)
    tr = Trainer(_cfg(tmp, "resume", ema_decay=0.9, load_model=path), None, torch.utils.data.TensorDataset(torch.zeros(1)))
    assert tr.engine.ema_updates == 3
    sd, raw = tr.engine.ema_state_dict(), tr.net.state_dict()
    for k, v in pth["model_ema"].items():
        assert torch.equal(sd[k].cpu(), v), k
    for k, v in pth["model"].items():
        assert torch.equal(raw[k].cpu(), v), k
    assert "weight EMA: restored from the checkpoint after 3 updates" in _log_text(tr)
    # load_ema: the averaged weights become the network's (here without an EMA of its own)
    tr = Trainer(_cfg(tmp, "load_ema", load_ema=True, load_model=path), None, torch.utils.data.TensorDataset(torch.zeros(1)))
    raw = tr.net.state_dict()
    for k, v in pth["model_ema"].items():
        assert torch.equal(raw[k].cpu(), v), k
    assert tr.engine._ema is None


def test_trainer_without_the_key(trained, L):
    from awr_amd.trainer import Trainer
    tmp, path, _ = trained
    pth = torch.load(path, map_location="cpu", weights_only=False)
    plain = os.path.join(str(tmp), "plain.pth")
    torch.save({k: pth[k] for k in ("model", "optimizer", "best_records")}, plain)
    with pytest.raises(L.AwrError, match="model_ema") as ei:
        Trainer(_cfg(tmp, "nokey", load_ema=True, load_model=plain), None, torch.utils.data.TensorDataset(torch.zeros(1)))
    assert "model_ema" in str(ei.value) and plain in str(ei.value)
    # ema_decay on a checkpoint without the key: the shadow starts from the loaded weights
    tr = Trainer(_cfg(tmp, "restart", ema_decay=0.9, load_model=plain), None, torch.utils.data.TensorDataset(torch.zeros(1)))
    assert tr.engine.ema_updates == 0
    assert torch.equal(tr.engine.ema_net.flat_params(), tr.net.flat_params()) and torch.equal(tr.engine.ema_net._barena, tr.net._barena)
    assert "starting from its weights" in _log_text(tr)
