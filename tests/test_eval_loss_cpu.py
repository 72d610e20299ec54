"""CPU: the configuration keys of the validation loss, and the entry point's declaration / export / argument checks."""
import os
import re

import pytest

from test_abi import REPO, declared_symbols, lib  # noqa: F401  (fixture)


def test_config_keys_are_validated():
    from awr_amd.config import Config
    assert Config.test_loss is False and Config.test_loss_stages == "last"
    assert Config(test_loss=True).test_loss is True and Config(test_loss=False).test_loss is False
    assert Config(test_loss_stages="all").test_loss_stages == "all" and Config(test_loss_stages="last").test_loss_stages == "last"
    for bad in (1, 0, "True", None, 1.0):
        with pytest.raises(ValueError, match="test_loss"):
            Config(test_loss=bad)
    for bad in ("first", "", None, True, 1, ["all"]):
        with pytest.raises(ValueError, match="test_loss_stages"):
            Config(test_loss_stages=bad)


def test_header_declares_and_library_exports_the_entry_point(lib):
    assert "awr_head_eval_nhwc" in declared_symbols()
    assert hasattr(lib.lib, "awr_head_eval_nhwc") and "awr_head_eval_nhwc" in lib.EXPORTS and not lib.MISSING
    text = open(os.path.join(REPO, "include", "awr_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int awr_head_eval_nhwc\((.*?)\);", text, flags=re.S)
    assert m, "awr_head_eval_nhwc is not documented like its neighbours"
    assert "test.py:73-86" in m.group(1) and "n_valid" in m.group(1)
    args = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
    assert re.search(r"const float\*\s*pred", args) and re.search(r"int n_valid", args) and re.search(r"double\*\s*acc", args)


def test_argument_checks_run_before_any_launch(lib):
    import ctypes as C
    buf = (C.c_double * 4)()
    p = C.addressof(buf)
    call = lib.lib.awr_head_eval_nhwc
    assert call(None, 64, p, p, 2, 14, 8, 16, 2, 0.4, 0.01, 1.0, 1.0, p, p, None, p, None) == -1 and "null pointer" in lib.last_error()
    assert call(p, 64, p, p, 2, 14, 8, 16, 3, 0.4, 0.01, 1.0, 1.0, p, p, None, p, None) == -1 and "n_valid" in lib.last_error()
    assert call(p, 64, p, p, 2, 14, 8, 16, -1, 0.4, 0.01, 1.0, 1.0, p, p, None, p, None) == -1 and "n_valid" in lib.last_error()
    assert call(p, 48, p, p, 2, 14, 8, 16, 2, 0.4, 0.01, 1.0, 1.0, p, p, None, p, None) == -1 and "Cp" in lib.last_error()
    assert call(p, 256, p, p, 2, 60, 8, 16, 2, 0.4, 0.01, 1.0, 1.0, p, p, None, p, None) == -1 and "Cp" in lib.last_error()


def test_infer_engine_keywords_exist():
    import inspect
    from awr_amd.trainer import InferEngine
    sig = inspect.signature(InferEngine.__init__).parameters
    assert sig["loss_weights"].default is None and sig["loss_stages"].default == "last"
    call = inspect.signature(InferEngine.__call__).parameters
    assert list(call)[1:] == ["img", "jt_uvd_gt", "n_valid"] and call["jt_uvd_gt"].default is None and call["n_valid"].default is None
    assert all(hasattr(InferEngine, n) for n in ("loss_means", "reset_loss"))
