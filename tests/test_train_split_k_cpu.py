"""Training split-K (awr_set_train_split_k): the parts that need no GPU -- the exported symbols, the process-wide default and the
validation of the Python options (False / True only: an unknown value is never read as "on")."""
import ctypes as C
import os
import subprocess
import sys

import pytest


def test_library_exports_the_mode_and_the_depth_query():
    from awr_amd import _lib as L
    for sym in ("awr_set_train_split_k", "awr_get_train_split_k", "awr_conv_split_depth"):
        assert hasattr(L.lib, sym), sym
    assert L.lib.awr_get_train_split_k.restype is C.c_int


def test_mode_is_off_in_a_fresh_process():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "AWR_TRAIN_SPLIT_K"}
    code = "import sys; sys.path.insert(0, %r); import awr_amd; from awr_amd import _lib as L; print(int(L.lib.awr_get_train_split_k()))" % repo
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "0"
    env["AWR_TRAIN_SPLIT_K"] = "1"          # the precedent of $AWR_WINOGRAD: the unchanged benchmark can time the mode
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "1"


def test_setter_takes_zero_or_one_only():
    from awr_amd import _lib as L
    was = int(L.lib.awr_get_train_split_k())
    try:
        assert L.lib.awr_set_train_split_k(1) == 0 and L.lib.awr_get_train_split_k() == 1
        assert L.lib.awr_set_train_split_k(2) != 0 and L.lib.awr_get_train_split_k() == 1
        assert L.lib.awr_set_train_split_k(0) == 0 and L.lib.awr_get_train_split_k() == 0
    finally:
        L.lib.awr_set_train_split_k(was)


def test_config_default_and_validation():
    from awr_amd.config import Config
    assert Config().train_split_k is False
    assert Config(train_split_k=True).train_split_k is True
    for bad in ("yes", "auto", 1, None):
        with pytest.raises(ValueError):
            Config(train_split_k=bad)


def test_engine_and_setter_refuse_unknown_values():
    import awr_amd
    from awr_amd.trainer import TrainEngine
    for bad in ("auto", "yes", 1, None):
        with pytest.raises(ValueError):
            TrainEngine(None, 2, 128, 1.0, split_k=bad)      # (validated before anything touches the network or the GPU)
        with pytest.raises(ValueError):
            awr_amd.set_train_split_k(bad)


def test_tuning_cache_key_carries_the_mode():
    from awr_amd.engine import tile_cache_key
    off, on = tile_cache_key("train/x", 1, 2, 2, 0), tile_cache_key("train/x", 1, 2, 2, 0, 1)
    assert off != on and off == "train/x/x1/s2/a2/w0"      # plans without the mode keep the key they always had
