"""CPU: the hand detector's numpy restatement on a synthetic scene, the ABI of the prediction entry points, their argument validation
and the Predictor's failure mode without a GPU (no compute calls -- there is no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
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


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


def scene():
    """zeros, a background plane at 1500 mm, a 60 x 60 pixel square at 700 mm whose middle is (u_mid, v_mid) = (229.5, 189.5)"""
    f = np.zeros((480, 640), np.uint16)
    f[40:440, 60:600] = 1500
    f[160:220, 200:260] = 700
    return f, 229.5, 189.5


def test_restatement_finds_the_square_exactly(D):
    f, u_mid, v_mid = scene()
    c, st = D.detect(f, seed="nearest", slab=150, iters=2)
    # means of consecutive integers are exact in double; at 700 mm a 300 mm cube spans 252 pixels and 550 ... 850 mm: the window holds
    # the whole square and none of the plane, so the square is a fixed point of the refinement
    assert c == (u_mid, v_mid, 700.0) and st == D.OK
    assert D.detect(f, seed="nearest", slab=150, iters=0) == ((u_mid, v_mid, 700.0), D.OK)
    assert D.detect(f, seed="given", center=(u_mid + 20, v_mid - 15, 720.0), iters=1) == ((u_mid, v_mid, 700.0), D.OK)


def test_seed_mode_matters(D):
    f, u_mid, v_mid = scene()
    c, st = D.detect(f, seed="range", depth_range=(1, 2000), iters=0)
    assert st == D.OK and c != (u_mid, v_mid, 700.0)
    assert abs(c[2] - 1500.0) < 20.0          # the plane outweighs the square
    c2, _ = D.detect(f, seed="range", depth_range=(1, 2000), iters=2)
    assert c2 != (u_mid, v_mid, 700.0)


def test_centre_of_mass_is_int64_arithmetic(D):
    f = np.full((480, 640), 65535, np.uint16)
    c, n = D.center_of_mass(f, None, 1.0, 65535.0)
    assert n == 480 * 640 and c == (319.5, 239.5, 65535.0)          # sum of d ~ 2e10: a 32-bit sum would have wrapped
    c, n = D.center_of_mass(f, (600, 640, 470, 480), 0.0, 1e9)
    assert n == 400 and c == (619.5, 474.5, 65535.0)
    with pytest.raises(ValueError, match="uint16"):
        D.center_of_mass(f.astype(np.float32))


def test_empty_frame_and_window_outside(D):
    z = np.zeros((480, 640), np.uint16)
    for seed in ("nearest", "range"):
        c, st = D.detect(z, seed=seed, iters=2)
        assert st == D.EMPTY and all(np.isnan(c))
    f, _, _ = scene()
    c, st = D.detect(f, seed="given", center=(-5000.0, 100.0, 700.0), iters=2)          # window wholly outside the frame
    assert st == D.EMPTY and all(np.isnan(c))
    c, st = D.detect(f, seed="given", center=(float("nan"), 100.0, 700.0), iters=1)
    assert st == D.EMPTY and all(np.isnan(c))
    assert D.detect(f, seed="given", center=(10.0, 20.0, 0.0), iters=1)[1] == D.EMPTY      # depth 0: no window
    with pytest.raises(ValueError):
        D.detect(f, iters=9)
    with pytest.raises(ValueError):
        D.detect(f, seed="brightest")


def test_host_blocks_follow_set_crop(D, lib):
    from awr_amd import nyu_data as ND
    blocks, M, cxyz, cube, st = D.sample_blocks([(229.5, 189.5, 700.0), (-5000.0, 100.0, 700.0), (float("nan"),) * 3], (300, 300, 300), 128)
    assert st.tolist() == [D.OK, D.BAD_WINDOW, D.BAD_WINDOW] and blocks[1] is None and blocks[2] is None
    b = blocks[0]
    c = np.array([229.5, 189.5, 700.0])
    (us, ue, vs, ve, zs, ze), size, (ox, oy) = ND.crop_geometry(c, [300, 300, 300], (128, 128))
    assert (b.ustart, b.cw, b.vstart, b.ch) == (us, ue - us, vs, ve - vs) and (b.rw, b.rh, b.ox, b.oy) == (size[0], size[1], int(ox), int(oy))
    assert (b.zstart, b.zend, b.lo, b.far, b.center_z, b.half, b.op, b.norm32) == (550.0, 850.0, 550.0, 850.0, 700.0, 150.0, 0, 0)
    assert np.array_equal(M[0], ND.center2transmat(np.array([229.5, 189.5, 700.0]), [300, 300, 300], (128, 128)))
    assert np.isnan(M[1]).all() and cube.dtype == np.float32 and cxyz.dtype == np.float32


def _decl(header, name, ret="int"):
    m = re.search(r"\b%s\s+%s\s*\((.*?)\)\s*;" % (ret, name), header, flags=re.S)
    assert m, "include/awr_hip.h does not declare %s" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entry_points_and_the_library_exports_them(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "awr_hip.h")).read(), flags=re.S)
    assert _decl(header, "awr_detect_scratch", "int64_t") == ["int B"]
    assert _decl(header, "awr_detect") == [
        "const void* frames", "int frame_type", "int64_t n_frames", "int fh", "int fw", "const int64_t* frame", "int B", "int seed_mode",
        "const double* seed_uvd", "double zmin", "double zmax", "double slab", "const double* cube", "int cube_stride", "double fx", "double fy",
        "int iters", "int parts", "void* scratch", "double* center_uvd", "int* status", "void* stream"]
    assert _decl(header, "awr_detect_samples") == [
        "const double* center_uvd", "const double* cube", "int cube_stride", "int64_t n_frames", "const int64_t* frame", "int B", "int dsize",
        "int fh", "int fw", "double fx", "double fy", "double u0", "double v0", "int flip", "awr_nyu_sample* samples", "float* M",
        "float* center_xyz", "float* cube_out", "int* status", "void* stream"]
    assert _decl(header, "awr_joints_unproject") == [
        "const float* jt_pred", "const float* center_xyz", "const float* M", "const float* cube", "int B", "int J", "int n_valid",
        "float img_size", "double fx", "double fy", "double u0", "double v0", "int flip", "float* uvd_out", "float* xyz_out", "int* status",
        "void* stream"]
    for code, value in (("AWR_DET_OK", 0), ("AWR_DET_EMPTY", 1), ("AWR_DET_BAD_FRAME", 2), ("AWR_DET_BAD_WINDOW", 3), ("AWR_DET_SEED_GIVEN", 0),
                        ("AWR_DET_SEED_RANGE", 1), ("AWR_DET_SEED_NEAREST", 2), ("AWR_DET_MAX_ITERS", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (code, value), header), code
    P, I, D64, F, L64 = C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_int64
    for name in ("awr_detect_scratch", "awr_detect", "awr_detect_samples", "awr_joints_unproject"):
        assert hasattr(lib.lib, name) and name in lib.EXPORTS
    assert not lib.MISSING
    assert lib.lib.awr_detect_scratch.argtypes == [I] and lib.lib.awr_detect_scratch.restype == L64
    assert lib.lib.awr_detect.argtypes == [P, I, L64, I, I, P, I, I, P, D64, D64, D64, P, I, D64, D64, I, I, P, P, P, P]
    assert lib.lib.awr_detect_samples.argtypes == [P, P, I, L64, P, I, I, I, I, D64, D64, D64, D64, I, P, P, P, P, P, P]
    assert lib.lib.awr_joints_unproject.argtypes == [P, P, P, P, I, I, I, F, D64, D64, D64, D64, I, P, P, P, P]
    # the Python codes are the header's
    from awr_amd import detect as Dm
    assert (Dm.OK, Dm.EMPTY, Dm.BAD_FRAME, Dm.BAD_WINDOW) == (0, 1, 2, 3) and Dm.SEEDS == {"given": 0, "range": 1, "nearest": 2} and Dm.MAX_ITERS == 8


def test_scratch_query(lib):
    f = lib.lib.awr_detect_scratch
    assert f(1) > 0 and f(64) == 64 * f(1) and f(1) % 8 == 0
    assert f(0) == -1 and "B" in lib.last_error()


def test_awr_detect_validates_its_arguments_before_any_hip_call(lib):
    f = lib.lib.awr_detect
    ok = dict(p=1 << 12, ftype=0, n_frames=4, fh=480, fw=640, B=2, mode=2, zmin=1.0, zmax=2000.0, slab=150.0, stride=0, iters=2, parts=0)

    def call(**kw):
        a = dict(ok, **kw)
        p = a["p"] or None
        return f(p, a["ftype"], a["n_frames"], a["fh"], a["fw"], p, a["B"], a["mode"], a.get("seed", p), a["zmin"], a["zmax"], a["slab"], p,
                 a["stride"], 588.03, 587.07, a["iters"], a["parts"], p, p, p, None)
    assert call(p=0) == -1 and "NULL" in lib.last_error()
    assert call(n_frames=0) == -1 and "n_frames" in lib.last_error()
    assert call(iters=9) == -1 and "iters" in lib.last_error()
    assert call(iters=-1) == -1
    assert call(zmin=5.0, zmax=4.0) == -1 and "zmin" in lib.last_error()
    assert call(zmin=float("nan")) == -1
    assert call(ftype=1) == -1 and "uint16" in lib.last_error()
    assert call(B=0) == -1 and "B" in lib.last_error()
    assert call(mode=3) == -1 and "seed_mode" in lib.last_error()
    assert call(mode=0, seed=None) == -1 and "seed_uvd" in lib.last_error()
    assert call(fh=0) == -1 and call(fw=1 << 20) == -1 and call(stride=2) == -1 and call(parts=-1) == -1 and call(parts=4096) == -1


def test_samples_and_unproject_validate_their_arguments_before_any_hip_call(lib):
    s, u = lib.lib.awr_detect_samples, lib.lib.awr_joints_unproject
    p = 1 << 12

    def samples(ptr=p, stride=0, n_frames=4, B=2, dsize=128, fh=480, fw=640, flip=-1):
        return s(ptr, ptr, stride, n_frames, ptr, B, dsize, fh, fw, 588.03, 587.07, 320.0, 240.0, flip, ptr, ptr, ptr, ptr, ptr, None)
    assert samples(ptr=None) == -1 and "NULL" in lib.last_error()
    assert samples(B=0) == -1 and samples(n_frames=0) == -1 and samples(dsize=0) == -1 and samples(fh=0) == -1 and samples(flip=0) == -1
    assert samples(stride=1) == -1 and "cube_stride" in lib.last_error()

    def unproject(ptr=p, B=4, J=14, n=4, S=128.0, flip=-1):
        return u(ptr, ptr, ptr, ptr, B, J, n, S, 588.03, 587.07, 320.0, 240.0, flip, ptr, ptr, ptr, None)
    assert unproject(ptr=None) == -1 and "NULL" in lib.last_error()
    assert unproject(B=0) == -1 and unproject(J=0) == -1 and unproject(J=257) == -1 and unproject(S=0.0) == -1 and unproject(flip=2) == -1
    assert unproject(n=5) == -1 and "n_valid" in lib.last_error()
    assert unproject(n=0) == 0            # nothing to do launches nothing


def test_predictor_without_a_gpu_is_an_awr_error(lib, monkeypatch):
    import torch
    import awr_amd
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (so the test says the same on a GPU box)
    with pytest.raises(lib.AwrError, match=r"detect\.detect"):
        awr_amd.Predictor(None, 128, 0.4)
