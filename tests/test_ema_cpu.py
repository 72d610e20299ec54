"""Weight EMA: the parts that need no GPU -- the config keys, the decay schedule, the validation of the engine's options
(before it looks at the network or the GPU) and the argument checks of awr_ema_update, which run before any HIP call."""
import ctypes as C

import pytest


def test_config_defaults_and_validation():
    from awr_amd.config import Config
    c = Config()
    assert c.ema_decay is None and c.ema_warmup is True and c.load_ema is False
    c = Config(ema_decay=0.999, ema_warmup=False, load_ema=True)
    assert c.ema_decay == 0.999 and c.ema_warmup is False and c.load_ema is True
    for bad in (0, 1, -0.1, True, "x", float("nan"), 0.0, 1.0, 1.5, float("inf"), False):
        with pytest.raises(ValueError, match="ema_decay"):
            Config(ema_decay=bad)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="ema_warmup"):
            Config(ema_warmup=bad)
        with pytest.raises(ValueError, match="load_ema"):
            Config(load_ema=bad)


def test_entry_point_overrides_reach_the_config():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from train import parse_overrides
    from awr_amd.config import Config
    over = parse_overrides(["ema_decay=0.999", "ema_warmup=False"])
    assert over == {"ema_decay": 0.999, "ema_warmup": False}
    c = Config(**over)
    assert c.ema_decay == 0.999 and c.ema_warmup is False and c.load_ema is False


def test_decay_schedule():
    from awr_amd.trainer import ema_decay_at
    assert ema_decay_at(0.999, 0, True) == 0.1 and ema_decay_at(0.999, 1, True) == 2 / 11
    seq = [ema_decay_at(0.999, t, True) for t in range(0, 9100)]
    assert all(b >= a for a, b in zip(seq, seq[1:]))                      # non-decreasing
    # (1 + t) / (10 + t) >= 0.999  <=>  t >= 8990
    assert seq[8989] < 0.999 and all(d == 0.999 for d in seq[8990:])
    assert ema_decay_at(0.999, 10 ** 9, True) == 0.999
    assert ema_decay_at(0.5, 0, True) == 0.1 and ema_decay_at(0.5, 8, True) == 0.5 and ema_decay_at(0.5, 7, True) == 8 / 17
    assert all(ema_decay_at(d, t, False) == d for d in (0.5, 0.999) for t in (0, 1, 10, 8990, 10 ** 6))      # warm-up off: constant


def test_engine_refuses_bad_values_before_it_looks_for_a_gpu():
    from awr_amd.trainer import TrainEngine
    for bad in (True, False, "0.9", [0.9]):
        with pytest.raises(TypeError, match="ema_decay"):
            TrainEngine(None, 2, 128, 1.0, ema_decay=bad)          # (net = None: nothing may touch the network first)
    for bad in (0, 1, 0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ema_decay"):
            TrainEngine(None, 2, 128, 1.0, ema_decay=bad)
    for bad in (1, 0, "yes", None):
        with pytest.raises(TypeError, match="ema_warmup"):
            TrainEngine(None, 2, 128, 1.0, ema_decay=0.9, ema_warmup=bad)


def test_argument_validation_without_gpu():
    """NULL pointers, n <= 0, misaligned or overlapping arenas and a weight outside (0, 1] are refused with an error code before any HIP call.
    The pointers are host addresses that nothing dereferences: every call here fails its checks."""
    from awr_amd import _lib as L
    buf = (C.c_double * 128)()
    a = (C.addressof(buf) + 15) & ~15          # 16-byte aligned; b = 64 floats further on
    b = a + 256
    f = lambda e, s, n, w=0.5: L.lib.awr_ema_update(e, s, n, w, None)      # noqa: E731

    def refused(rc, word=None):
        return rc == -1 and "ema_update" in L.last_error() and (word is None or word in L.last_error())
    assert refused(f(None, b, 8)) and refused(f(a, None, 8)) and refused(f(None, None, 8))
    for n in (0, -4):
        assert refused(f(a, b, n))
    for off in (4, 8, 12, 2):
        assert refused(f(a + off, b, 8), "aligned") and refused(f(a, b + off, 8), "aligned")
    # overlap: the same arena, src starting inside ema, ema starting inside src; 64 floats apart is fine up to n = 64 only
    assert refused(f(a, a, 8), "overlap") and refused(f(a, a + 16, 8), "overlap") and refused(f(a + 16, a, 8), "overlap")
    assert refused(f(a, b, 65), "overlap") and refused(f(b, a, 65), "overlap")
    for w in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf"), -float("inf")):
        assert refused(f(a, b, 8, w), "(0, 1]"), w


def test_clone_is_a_second_network_of_the_same_kind():
    """AwrBackbone.clone() on the host (the arenas are plain tensors until .cuda()): class, constructor arguments, arenas and counters"""
    import torch
    from awr_amd import get_deconv_net
    from awr_amd.hourglass import PoseNet
    from awr_amd.nets import ResNet18Deconv
    for make, attrs in ((lambda: get_deconv_net(18, 14, 4), ("J", "downsample", "depth")), (lambda: ResNet18Deconv(21, 2), ("J", "downsample", "depth")),
                        (lambda: PoseNet("hourglass_1", 14), ("J", "nstack", "f"))):
        net = make()
        net._barena.uniform_(0.5, 1.5)
        net._counters.fill_(7)
        net.eval()
        before = torch.random.get_rng_state()
        twin = net.clone()
        assert torch.equal(torch.random.get_rng_state(), before)          # the caller's random stream is where it was
        assert type(twin) is type(net) and twin is not net and not twin.training and twin.device == net.device
        assert all(getattr(twin, a) == getattr(net, a) for a in attrs + ("n_params", "n_active", "nstage"))
        assert torch.equal(twin.flat_params(), net.flat_params()) and torch.equal(twin._barena, net._barena) and torch.equal(twin._counters, net._counters)
        for a in ("_arena", "_garena", "_barena", "_counters"):
            assert getattr(twin, a).data_ptr() != getattr(net, a).data_ptr(), a
        assert twin._handle is not net._handle and not twin._plans
        sd, ref = twin.state_dict(), net.state_dict()
        assert list(sd) == list(ref) and all(torch.equal(sd[k], ref[k]) for k in ref)
        twin.flat_params().add_(1.0)                                      # nothing is shared: the original keeps its values
        assert not torch.equal(twin.flat_params(), net.flat_params())
        assert net.train().clone().training
