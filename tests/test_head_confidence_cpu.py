"""CPU: per-joint confidence and vote spread -- the library exports the entry points and the binding knows them, their
argument checks run before any HIP call, the host restatement (tests/confidence_ref.py) on cases with a closed form, and the argument
validation of the Python surface (no compute calls -- there is no GPU here)."""
import math
import os
import re
import subprocess

import pytest
import torch

import confidence_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"awr_head_confidence_nhwc": 13, "awr_head_confidence": 11, "awr_confidence_fields": 12}      # name: number of arguments


@pytest.fixture(scope="module")
def lib():
    import awr_amd  # noqa: F401
    from awr_amd import build
    if not os.path.exists(build.LIB):
        build.build_lib(verbose=False)
    from awr_amd import _lib
    return _lib


def test_entry_points_are_exported_declared_and_bound(lib):
    from awr_amd import build
    dyn = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(awr_\w+)$", dyn, flags=re.M))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "awr_hip.h")).read(), flags=re.S)
    for name, nargs in ENTRY.items():
        assert name in exported, "libawr_hip.so does not export %s" % name
        assert name in lib.EXPORTS and name not in lib.MISSING
        fn = getattr(lib.lib, name)
        assert len(fn.argtypes) == nargs and fn.restype is lib.C.c_int
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, header, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    # the float arguments sit where the header puts `ks`
    assert lib.lib.awr_head_confidence_nhwc.argtypes[9] is lib.C.c_float and lib.lib.awr_head_confidence.argtypes[8] is lib.C.c_float
    text = open(os.path.join(REPO, "include", "awr_hip.h")).read()
    assert "feature_tool.py:57-63" in text


def test_entry_points_check_their_arguments_without_a_gpu(lib):
    one = 16                                     # any non-null address: the checks come before the first dereference or launch
    f = lib.lib.awr_head_confidence_nhwc
    assert f(None, 64, one, one, one, 2, 14, 8, 16, 0.4, one, one, None) == -1 and "null pointer" in lib.last_error()
    assert f(one, 64, one, one, None, 2, 14, 8, 16, 0.4, one, one, None) == -1 and "null pointer" in lib.last_error()
    assert f(one, 64, one, one, one, 2, 14, 8, 16, 0.4, one, None, None) == -1 and "null pointer" in lib.last_error()
    assert f(one, 256, one, one, one, 2, 60, 8, 16, 0.4, one, one, None) == -1 and "Cp" in lib.last_error()          # more than 56 joints
    assert f(one, 64, one, one, one, 2, 14, 4, 16, 0.4, one, one, None) == -1 and "multiple of 64" in lib.last_error()
    assert f(one, 48, one, one, one, 2, 12, 8, 16, 0.4, one, one, None) == -1 and "Cp" in lib.last_error()
    g = lib.lib.awr_head_confidence
    assert g(one, one, one, None, 2, 14, 8, 16, 0.4, one, None) == -1 and "null pointer" in lib.last_error()
    assert g(one, one, one, one, 2, 14, 63, 128, 0.4, one, None) == -1 and "F % 4" in lib.last_error()
    assert g(one, one, one, one, 0, 14, 8, 16, 0.4, one, None) == -1 and "positive" in lib.last_error()
    k = lib.lib.awr_confidence_fields
    assert k(one, one, None, None, None, 2, 14, 2, one, one, one, None) == -1 and "null pointer" in lib.last_error()
    assert k(one, one, one, None, None, 2, 14, 3, one, one, one, None) == -1 and "n_valid" in lib.last_error()
    assert k(one, one, one, None, None, 2, 14, 0, one, one, one, None) == 0          # nothing to do: no launch


@pytest.mark.parametrize("F", [8, 24])
def test_zero_map_on_a_foreground_image_is_the_variance_of_the_grid(F):
    """h = 0 everywhere: uniform weights 1 / P and votes = pixel centres, so var_u = var_v = the variance of the F cell centres of [-1, 1],
    (F^2 - 1) / (3 F^2), and var_d the plain (population) variance of the sampled depths."""
    B, J, H = 2, 3, 2 * F
    g = torch.Generator().manual_seed(F)
    img = torch.rand(B, 1, H, H, generator=g) * 1.8 - 0.9              # all foreground
    out = R.confidence(torch.zeros(B, 4 * J, F, F), img, 0.4)
    d = img[:, 0, ::2, ::2].double().reshape(B, -1)
    want = (F * F - 1) / (3.0 * F * F)
    assert out.dtype == torch.float64 and out.shape == (B, J, 4)
    assert float(out[..., 0].abs().max()) == 0.0
    assert float((out[..., 1:3] - want).abs().max()) < 1e-14
    assert float((out[..., 3] - d.var(-1, unbiased=False).unsqueeze(1)).abs().max()) < 1e-14
    out32 = R.confidence(torch.zeros(B, 4 * J, F, F), img, 0.4, dtype=torch.float32)
    assert out32.dtype == torch.float32 and float((out32.double() - out).abs().max()) < 1e-5


def test_one_hot_pixel_takes_all_the_weight():
    """one foreground pixel with heat 1, every other heat 0, offsets zero: conf = w* = e^30 / (e^30 + P - 1), and every squared distance
    between two points of [-1, 1]^3 is at most 4 per coordinate, so the three variances together stay below (1 - w*) * 4 * 3"""
    B, J, F, H = 1, 2, 8, 16
    P = F * F
    g = torch.Generator().manual_seed(1)
    img = torch.rand(B, 1, H, H, generator=g) * 1.8 - 0.9
    img[0, 0, 0, 0] = 1.0                                                # one background pixel somewhere else
    off = torch.zeros(B, 4 * J, F, F)
    off[0, 3 * J + 0, 3, 5] = 1.0
    off[0, 3 * J + 1, 6, 2] = 1.0
    out = R.confidence(off, img, 1.0)
    w = R.E30 / (R.E30 + P - 1)
    assert float((out[..., 0] - w).abs().max()) < 1e-12
    assert float(out[..., 1:].sum(-1).max()) <= (1.0 - w) * 4 * 3
    assert float(out[..., 1:].min()) >= 0.0
    # and the joint is that pixel's centre
    jt = R.joints(off, img, 1.0)
    assert abs(float(jt[0, 0, 0]) - (2 * 5.5 / F - 1)) < 1e-10 and abs(float(jt[0, 0, 1]) - (2 * 3.5 / F - 1)) < 1e-10


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_heat_on_background_pixels_changes_nothing(dtype):
    off, img = R.bump_case(2, 5, 8, 16, seed=3)
    bg = (img[:, :, ::2, ::2] >= 0.99)
    assert bool(bg.any()) and bool((~bg).any())
    loud = off.clone()
    loud[:, 15:] += 5.0 * bg.float()                  # heat, and
    loud[:, :15] += 3.0 * bg.float()                  # offsets, on background pixels only
    assert torch.equal(R.confidence(off, img, 0.4, dtype=dtype), R.confidence(loud, img, 0.4, dtype=dtype))
    assert torch.equal(R.peak(off, img), R.peak(loud, img))


@pytest.mark.parametrize("ks", [0.4, 1.0])
def test_variances_are_never_negative(ks):
    for seed, (B, J, F, H) in enumerate([(2, 14, 8, 16), (2, 21, 16, 32), (1, 3, 24, 48)]):
        off, img = R.bump_case(B, J, F, H, seed=seed)
        for dtype in (torch.float64, torch.float32):
            out = R.confidence(off, img, ks, dtype=dtype)
            assert float(out[..., 1:].min()) >= 0.0 and bool(torch.isfinite(out).all())
            # a tight joint keeps its spread: the scatter about the joint, not E[v^2] - E[v]^2
            assert float(out[..., 0].min()) > 0.0 and float(out[..., 0].max()) < 1.3
    c = R.spread_mm(torch.tensor([[[0.5, 1e-4, 4e-4, 0.0]]]), (300.0, 300.0, 300.0))
    assert abs(float(c) - math.sqrt(5e-4) * 150.0) < 1e-3


def test_python_surface_validates_confidence_without_a_gpu(lib):
    import awr_amd
    from awr_amd.trainer import InferEngine
    import inspect
    for bad in ("yes", 1, None):
        with pytest.raises(TypeError, match="confidence"):
            InferEngine(None, 2, 128, 0.4, confidence=bad)
        with pytest.raises(TypeError, match="confidence"):
            awr_amd.Predictor(None, 128, 0.4, confidence=bad)
    if not torch.cuda.is_available():
        with pytest.raises(lib.AwrError, match="GPU"):          # a valid flag: on to the check it always made
            awr_amd.Predictor(None, 128, 0.4, confidence=True)
    assert inspect.signature(InferEngine.__init__).parameters["confidence"].default is False
    assert inspect.signature(awr_amd.Predictor.__init__).parameters["confidence"].default is False
    from awr_amd import predictor
    assert predictor.Prediction._fields == ("xyz", "uvd", "center_xyz", "M", "status")
    assert predictor.ConfidentPrediction._fields == predictor.Prediction._fields + ("conf", "peak", "spread_mm")
    with pytest.raises(lib.AwrError):          # no CPU fallback here either
        awr_amd.FeatureModule().joint_confidence(torch.zeros(1, 56, 64, 64), torch.zeros(1, 1, 128, 128), 0.4)


def test_predict_py_parses_the_confidence_flag():
    import predict
    a = predict.parse_args(["frames.npy", "--load-model", "x.pth"])
    assert a.confidence is False and a.out == "."
    b = predict.parse_args(["frames.npy", "--load-model", "x.pth", "--confidence", "--out", "o"])
    assert b.confidence is True and b.out == "o" and b.frames == "frames.npy"
