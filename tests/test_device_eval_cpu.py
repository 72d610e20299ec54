"""CPU: the device evaluator's ABI, config key and failure mode without a GPU (no compute calls -- there is no GPU here)."""
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import awr_amd  # noqa: F401
    from awr_amd import build
    if not os.path.exists(build.LIB):
        build.build_lib(verbose=False)
    from awr_amd import _lib
    return _lib


def test_header_declares_awr_eval_batch_and_the_library_exports_it(lib):
    import ctypes as C
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "awr_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+awr_eval_batch\s*\((.*?)\)\s*;", header, flags=re.S)
    assert m, "include/awr_hip.h does not declare awr_eval_batch"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const float* jt_pred", "const float* jt_xyz_gt", "const float* center_xyz", "const float* M", "const float* cube",
                    "int B", "int J", "int n_valid", "float img_size", "double fx", "double fy", "double u0", "double v0", "int flip",
                    "float* uvd_out", "float* err_out", "int64_t row", "int64_t capacity", "double* acc", "int* status", "void* stream"]
    for code, value in (("AWR_EVAL_OK", 0), ("AWR_EVAL_SINGULAR", 1), ("AWR_EVAL_NONFINITE", 2), ("AWR_EVAL_MAX_JOINTS", 256)):
        assert re.search(r"#define\s+%s\s+%d\b" % (code, value), header), code
    assert hasattr(lib.lib, "awr_eval_batch") and "awr_eval_batch" in lib.EXPORTS and not lib.MISSING
    # the binding passes what the header declares, type by type
    P, I, F, D, L64 = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_int64
    assert lib.lib.awr_eval_batch.argtypes == [P] * 5 + [I, I, I, F, D, D, D, D, I, P, P, L64, L64, P, P, P]


def test_awr_eval_batch_validates_its_arguments_before_any_hip_call(lib):
    f = lib.lib.awr_eval_batch
    ok = dict(B=4, J=14, n=4, S=128.0, flip=-1, row=0, cap=0)

    def call(ptrs=1, **kw):
        a = dict(ok, **kw)
        p = ptrs or None
        return f(p, p, p, p, p, a["B"], a["J"], a["n"], a["S"], 588.03, 587.07, 320.0, 240.0, a["flip"], None, None, a["row"], a["cap"], p, p, None)
    assert call(ptrs=0) == -1 and "NULL" in lib.last_error()
    assert call(J=0) == -1 and call(J=257) == -1 and "J" in lib.last_error()
    assert call(n=5) == -1 and "n_valid" in lib.last_error()
    assert call(flip=0) == -1 and call(S=0.0) == -1
    assert call(row=-1) == -1
    assert call(n=0) == 0            # an empty batch launches nothing
    # result rows that would not fit the caller's buffers are refused, not written
    assert f(1, 1, 1, 1, 1, 4, 14, 4, 128.0, 588.03, 587.07, 320.0, 240.0, -1, 1, 1, 6, 8, 1, 1, None) == -1 and "do not fit" in lib.last_error()


def test_config_key_defaults_to_the_host_evaluator(lib):
    from awr_amd.config import Config, opt
    from awr_amd.evaluator import EvalUtil
    from awr_amd.trainer import SyntheticHands, make_evaluator
    assert Config.device_eval is False and opt.device_eval is False and Config(device_eval=True).device_eval is True
    with pytest.raises(ValueError, match="device_eval"):
        Config(device_eval="yes")
    data = SyntheticHands(2, img_size=32)
    ev = make_evaluator(Config(), data)              # what Trainer.train / Trainer.test construct
    assert type(ev) is EvalUtil and (ev.img_size, ev.num_kp, ev.flip) == (32, 14, -1)


def test_trainer_sources_build_their_evaluators_through_the_config(lib):
    """Trainer needs a GPU to construct; its two loops take their evaluator from make_evaluator and nowhere else."""
    import inspect
    from awr_amd.trainer import Trainer
    for fn in (Trainer.train, Trainer._score):      # (Trainer.test's scoring pass)
        src = inspect.getsource(fn)
        assert "make_evaluator(cfg, " in src and "self.EvalUtil(" not in src and "DeviceEvalUtil(" not in src


def test_device_evaluator_without_a_gpu_is_an_awr_error(lib, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (so the test says the same on a GPU box)
    from awr_amd.config import Config
    from awr_amd.evaluator import DeviceEvalUtil
    from awr_amd.trainer import SyntheticHands, make_evaluator
    with pytest.raises(lib.AwrError, match="needs a GPU"):
        DeviceEvalUtil(128, (588.03, 587.07, 320.0, 240.0), -1, 14)
    with pytest.raises(lib.AwrError, match="needs a GPU"):
        make_evaluator(Config(device_eval=True), SyntheticHands(2, img_size=32))
