"""Gradient accumulation and global-norm clipping: the parts that need no GPU -- the config keys, the validation of the engine's
options (before it looks at the network or the GPU) and the argument checks of the four new entry points, which run before any HIP call."""
import ctypes as C

import pytest


def test_config_defaults_and_validation():
    from awr_amd.config import Config
    c = Config()
    assert c.accum_steps == 1 and c.clip_grad_norm is None and c.log_grad_norm is False
    c = Config(accum_steps=4, clip_grad_norm=1.0, log_grad_norm=True)
    assert c.accum_steps == 4 and c.clip_grad_norm == 1.0 and c.log_grad_norm is True
    assert Config(clip_grad_norm=2).clip_grad_norm == 2          # `--set clip_grad_norm=2` parses to an int
    for bad in (True, False, 0, -1, 2.0, "4", None):
        with pytest.raises(ValueError, match="accum_steps"):
            Config(accum_steps=bad)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), "1.0", True):
        with pytest.raises(ValueError, match="clip_grad_norm"):
            Config(clip_grad_norm=bad)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="log_grad_norm"):
            Config(log_grad_norm=bad)


def test_entry_point_overrides_reach_the_config():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from train import parse_overrides
    from awr_amd.config import Config
    c = Config(**parse_overrides(["accum_steps=4", "clip_grad_norm=1.0", "log_grad_norm=True"]))
    assert c.accum_steps == 4 and c.clip_grad_norm == 1.0 and c.log_grad_norm is True


def test_engine_refuses_bad_values_before_it_looks_for_a_gpu():
    from awr_amd.trainer import TrainEngine
    for bad in (True, False, 2.0, "2", None):
        with pytest.raises(TypeError, match="accum_steps"):
            TrainEngine(None, 2, 128, 1.0, accum_steps=bad)          # (net = None: nothing may touch the network first)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="accum_steps"):
            TrainEngine(None, 2, 128, 1.0, accum_steps=bad)
    for bad in ("1.0", True, [1.0]):
        with pytest.raises(TypeError, match="clip_grad_norm"):
            TrainEngine(None, 2, 128, 1.0, clip_grad_norm=bad)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="clip_grad_norm"):
            TrainEngine(None, 2, 128, 1.0, clip_grad_norm=bad)
    for bad in (1, 0, "yes", None):
        with pytest.raises(TypeError, match="grad_norm"):
            TrainEngine(None, 2, 128, 1.0, grad_norm=bad)


def test_scratch_size_is_host_arithmetic():
    from awr_amd import _lib as L
    f = L.lib.awr_grad_norm_scratch
    assert f(0) == 0 and f(-5) == 0
    assert f(1) == 8 and f(1027) == 8 and f(1028) == 16
    assert f(4 * 256 * 1024) == 8192 and f(1 << 40) == 8192      # never more than 1024 float64 partials
    assert all(0 < f(n) <= 8192 and f(n) % 8 == 0 for n in (3, 65537, (1 << 21) + 3, 11_000_000))


def test_argument_validation_without_gpu():
    """NULL pointers, n <= 0, step < 1 and misaligned arenas are refused with an error code before any HIP call.  The pointers are host addresses
    that nothing dereferences: every call here fails its checks."""
    from awr_amd import _lib as L
    buf = (C.c_double * 64)()
    a = (C.addressof(buf) + 15) & ~15          # 16-byte aligned
    lib = L.lib
    adam = lambda p, g, g2, ds, m, v, n, step: lib.awr_adam_step_dev(p, g, g2, ds, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, 1.0, None)      # noqa: E731
    sgd = lambda p, g, g2, ds, b, n, step: lib.awr_sgd_step_dev(p, g, g2, ds, b, n, 1e-2, 0.9, 0.0, step, 1.0, None)      # noqa: E731
    norm = lambda g, g2, n, sc, no, so, mx=1.0: lib.awr_grad_norm(g, g2, n, 1.0, mx, sc, no, so, None)      # noqa: E731
    # NULL
    assert adam(None, a, None, None, a, a, 8, 1) == -1 and "adam_step_dev" in L.last_error()
    assert adam(a, None, None, None, a, a, 8, 1) == -1 and adam(a, a, None, None, None, a, 8, 1) == -1 and adam(a, a, None, None, a, None, 8, 1) == -1
    assert sgd(None, a, None, None, a, 8, 1) == -1 and "sgd_step_dev" in L.last_error()
    assert sgd(a, None, None, None, a, 8, 1) == -1 and sgd(a, a, None, None, None, 8, 1) == -1
    assert lib.awr_grad_accumulate(None, a, 8, 1, None) == -1 and "grad_accumulate" in L.last_error()
    assert lib.awr_grad_accumulate(a, None, 8, 0, None) == -1
    assert norm(None, None, 8, a, a, a) == -1 and "grad_norm" in L.last_error()
    assert norm(a, None, 8, None, a, a) == -1 and norm(a, None, 8, a, None, a) == -1 and norm(a, None, 8, a, a, None) == -1
    # n <= 0, step < 1
    for n in (0, -4):
        assert adam(a, a, None, None, a, a, n, 1) == -1 and sgd(a, a, None, None, a, n, 1) == -1
        assert lib.awr_grad_accumulate(a, a, n, 1, None) == -1 and norm(a, None, n, a, a, a) == -1
    assert adam(a, a, None, None, a, a, 8, 0) == -1 and sgd(a, a, None, None, a, 8, 0) == -1
    # misaligned arenas: 4 bytes off for the float4 kernels (each arena in turn, g2 too), 2 bytes off for the scalar SGD kernel
    for k in range(5):
        ptrs = [a + 4 if i == k else a for i in range(5)]
        p, g, g2, m, v = ptrs
        assert adam(p, g, g2, None, m, v, 8, 1) == -1 and "aligned" in L.last_error(), k
    assert adam(a, a, None, a + 2, a, a, 8, 1) == -1 and "aligned" in L.last_error()
    for k in range(5):
        p, g, g2, ds, b = [a + 2 if i == k else a for i in range(5)]
        assert sgd(p, g, g2, ds, b, 8, 1) == -1 and "aligned" in L.last_error(), k
    assert lib.awr_grad_accumulate(a + 4, a, 8, 1, None) == -1 and "aligned" in L.last_error()
    assert lib.awr_grad_accumulate(a, a + 8, 8, 1, None) == -1 and "aligned" in L.last_error()
    assert norm(a + 4, None, 8, a, a, a) == -1 and "aligned" in L.last_error()
    assert norm(a, a + 8, 8, a, a, a) == -1 and "aligned" in L.last_error()
    assert norm(a, None, 8, a + 4, a, a) == -1 and norm(a, None, 8, a, a + 4, a) == -1 and norm(a, None, 8, a, a, a + 2) == -1
    assert norm(a, None, 8, a, a, a, float("nan")) == -1 and "NaN" in L.last_error()
