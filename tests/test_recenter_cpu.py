"""CPU: re-centring on predicted joints and tracking -- the ABI of awr_joints_center / awr_centers_select, their argument
validation, their numpy statements (detect.joints_center, detect.select) on hand-made batches, and the validation of the Predictor's and
predict.py's new options (no compute calls -- there is no GPU here)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAS, FLIP = (147.0, 146.8, 80.0, 60.0), -1


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


def hand_made_batch():
    """B = 6, J = 14 around (-20, 10, 620) in a 300 mm cube: frame 1 has a NaN (joint 5), frame 2 is 2 m too deep, frame 3 is 200 mm off in
    x, frame 4 has a detector status; frames 0 and 5 are ordinary.  -> xyz, center_uvd, center_xyz, cube, status, ustatus"""
    from awr_amd.evaluator import xyz2uvd
    r = np.random.RandomState(3)
    B, J = 6, 14
    cxyz = np.tile(np.array([-20.0, 10.0, 620.0], np.float32), (B, 1))
    xyz = (cxyz[:, None, :] + r.uniform(-100, 100, (B, J, 3))).astype(np.float32)
    xyz[1, 5, 1] = np.nan
    xyz[2, :, 2] += 2000.0
    xyz[3, :, 0] += 200.0
    status, ustatus = np.zeros(B, np.int32), np.zeros(B, np.int32)
    status[4] = 1
    cuvd = xyz2uvd(cxyz.astype(np.float64), PARAS, FLIP).astype(np.float64) + r.uniform(-0.25, 0.25, (B, 3))      # (no round numbers)
    return xyz, cuvd, cxyz, np.full((B, 3), 300.0, np.float32), status, ustatus


def _decl(header, name, ret="int"):
    m = re.search(r"\b%s\s+%s\s*\((.*?)\)\s*;" % (ret, name), header, flags=re.S)
    assert m, "include/awr_hip.h does not declare %s" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entry_points_and_the_library_exports_them(lib, D):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "awr_hip.h")).read(), flags=re.S)
    assert _decl(header, "awr_joints_center") == [
        "const float* xyz", "const double* center_uvd", "const float* center_xyz", "const float* cube", "const int* status",
        "const int* ustatus", "int B", "int J", "int n_valid", "const int* joints", "int n_joints", "double fx", "double fy", "double u0",
        "double v0", "int flip", "double zmin", "double zmax", "double max_shift", "double* center_out", "double* next_out", "int* code",
        "void* stream"]
    assert _decl(header, "awr_centers_select") == [
        "const double* a_center", "const int* a_status", "const double* b_center", "const int* b_status", "int B", "double* out_center",
        "int* out_status", "int* which", "void* stream"]
    for code, value in (("AWR_RECENTER_KEPT_FRAME", 0), ("AWR_RECENTER_MOVED", 1), ("AWR_RECENTER_KEPT_NONFINITE", 2),
                        ("AWR_RECENTER_KEPT_DEPTH", 3), ("AWR_RECENTER_KEPT_SHIFT", 4), ("AWR_RECENTER_MAX_JOINTS", 256)):
        assert re.search(r"#define\s+%s\s+%d\b" % (code, value), header), code
    P, I, D64 = C.c_void_p, C.c_int, C.c_double
    for name in ("awr_joints_center", "awr_centers_select"):
        assert hasattr(lib.lib, name) and name in lib.EXPORTS
    assert not lib.MISSING
    assert lib.lib.awr_joints_center.argtypes == [P, P, P, P, P, P, I, I, I, P, I, D64, D64, D64, D64, I, D64, D64, D64, P, P, P, P]
    assert lib.lib.awr_centers_select.argtypes == [P, P, P, P, I, P, P, P, P]
    assert (D.KEPT_FRAME, D.MOVED, D.KEPT_NONFINITE, D.KEPT_DEPTH, D.KEPT_SHIFT, D.MAX_JOINTS) == (0, 1, 2, 3, 4, 256)


def test_entry_points_validate_their_arguments_before_any_hip_call(lib):
    f, g = lib.lib.awr_joints_center, lib.lib.awr_centers_select
    p = 1 << 12
    inf, nan = float("inf"), float("nan")

    def center(ptr=p, B=4, J=14, n=4, joints=p, nj=3, fx=588.03, fy=587.07, flip=-1, zmin=1.0, zmax=2000.0, shift=1.0, out=p, nxt=p, code=p):
        return f(ptr, ptr, ptr, ptr, ptr, ptr, B, J, n, joints, nj, fx, fy, 320.0, 240.0, flip, zmin, zmax, shift, out, nxt, code, None)
    assert center(ptr=None) == -1 and "NULL" in lib.last_error()
    assert center(out=None) == -1 and "NULL" in lib.last_error()
    assert center(code=None) == -1 and "NULL" in lib.last_error()
    assert center(B=0) == -1 and "B" in lib.last_error()
    assert center(B=65536) == -1
    assert center(J=257) == -1 and "J" in lib.last_error()
    assert center(J=0) == -1
    assert center(n=5) == -1 and "n_valid" in lib.last_error()
    assert center(n=-1) == -1
    assert center(nj=15) == -1 and "n_joints" in lib.last_error()
    assert center(nj=-1) == -1
    assert center(joints=None, nj=3) == -1 and "NULL" in lib.last_error()
    assert center(flip=0) == -1 and "flip" in lib.last_error()
    assert center(flip=2) == -1
    assert center(fx=0.0) == -1 and center(fy=inf) == -1 and center(fx=nan) == -1
    assert center(zmin=5.0, zmax=4.0) == -1 and "zmin" in lib.last_error()
    assert center(zmin=nan) == -1
    assert center(shift=-1.0) == -1 and "max_shift" in lib.last_error()
    assert center(shift=nan) == -1
    # what must pass the checks: nothing to do launches nothing (so it is testable here), with and without the optional arguments
    assert center(n=0) == 0 and center(n=0, shift=inf) == 0 and center(n=0, joints=None, nj=0, nxt=None) == 0 and center(n=0, J=256, nj=256) == 0

    def select(a=p, b=p, out=p, B=4, which=p):
        return g(a, a, b, b, B, out, out, which, None)
    assert select(a=None) == -1 and "NULL" in lib.last_error()
    assert select(b=None) == -1 and select(out=None) == -1
    assert select(B=0) == -1 and "B" in lib.last_error()
    assert select(B=65536) == -1


def test_joints_center_on_a_hand_made_batch(D):
    from awr_amd.evaluator import xyz2uvd
    xyz, cuvd, cxyz, cube, status, ustatus = hand_made_batch()
    keep = cuvd.copy()
    out, nxt, code = D.joints_center(xyz, cuvd, cxyz, cube, status, ustatus, PARAS, FLIP)
    assert code.dtype == np.int32 and code.tolist() == [1, 2, 3, 4, 0, 1]
    assert out.dtype == np.float64 and nxt.dtype == np.float64 and np.array_equal(cuvd, keep)          # the input is left alone
    sub = D.joints_center(xyz, cuvd, cxyz, cube, status, ustatus, PARAS, FLIP, joints=[0, 3, 13], max_shift=1e9, depth_range=(1, 65535))
    assert sub[2].tolist() == [1, 1, 1, 1, 0, 1]
    for (o, n, c), sel in (((out, nxt, code), list(range(14))), (sub, [0, 3, 13])):
        for b in range(6):
            if c[b] != D.MOVED:
                assert o[b].tobytes() == cuvd[b].tobytes() and np.isnan(n[b]).all(), b          # kept: the input centre bit for bit
                continue
            m = np.zeros(3, np.float64)
            for j in sel:
                m = m + xyz[b, j].astype(np.float64)
            m = m / float(len(sel))
            # evaluator.xyz2uvd works in the dtype it is given (float64 here) and stores float32: the statement keeps the doubles
            want = np.array([m[0] * PARAS[0] / m[2] + PARAS[2], (m[1] * FLIP) * PARAS[1] / m[2] + PARAS[3], m[2]])
            assert o[b].tobytes() == want.tobytes() and n[b].tobytes() == want.tobytes(), b
            assert np.array_equal(o[b].astype(np.float32), xyz2uvd(m, PARAS, FLIP)), b
    # the un-projection's code keeps a frame too; an index outside [0, J) is "not finite", never a read
    ustatus2 = ustatus.copy()
    ustatus2[0] = 2
    assert D.joints_center(xyz, cuvd, cxyz, cube, status, ustatus2, PARAS, FLIP)[2].tolist() == [0, 2, 3, 4, 0, 1]
    assert D.joints_center(xyz, cuvd, cxyz, cube, status, ustatus, PARAS, FLIP, joints=[0, 14])[2].tolist() == [2, 2, 2, 2, 0, 2]
    assert D.joints_center(xyz, cuvd, cxyz, cube, status, ustatus, PARAS, FLIP, joints=[-1])[2].tolist() == [2, 2, 2, 2, 0, 2]
    # the shift gate is inclusive and per axis; no gate at all with infinity; max_shift = 0 keeps everything that is not exactly there
    one = np.array([[[30.0, 10.0, 620.0]]], np.float32)
    args = (cuvd[:1], np.array([[-20.0, 10.0, 620.0]], np.float32), np.full((1, 3), 100.0, np.float32), [0], [0], PARAS, FLIP)
    assert D.joints_center(one, *args, max_shift=1.0)[2].tolist() == [D.MOVED]               # |dx| = 50 = 1.0 * 100 / 2
    assert D.joints_center(one, *args, max_shift=0.999)[2].tolist() == [D.KEPT_SHIFT]
    assert D.joints_center(one, *args, max_shift=0.0)[2].tolist() == [D.KEPT_SHIFT]
    assert D.joints_center(one, *args, max_shift=float("inf"))[2].tolist() == [D.MOVED]
    assert D.joints_center(one, *args, depth_range=(620.0, 620.0))[2].tolist() == [D.MOVED]   # the depth gate is inclusive too
    assert D.joints_center(one, *args, depth_range=(1.0, 619.9))[2].tolist() == [D.KEPT_DEPTH]
    with pytest.raises(ValueError):
        D.joints_center(one, *args, max_shift=-1.0)
    with pytest.raises(ValueError):
        D.joints_center(one, *args, depth_range=(5.0, 4.0))


def test_select(D):
    nan = float("nan")
    a = np.array([(1.0, 2.0, 3.0), (1.0, nan, 3.0), (4.0, 5.0, 6.0), (nan, nan, nan), (7.0, 8.0, float("inf"))])
    a_st = np.array([D.OK, D.OK, D.EMPTY, D.EMPTY, D.OK], np.int32)
    b = np.array([(10.0, 20.0, 30.0), (11.0, 21.0, 31.0), (12.0, 22.0, 32.0), (nan, nan, nan), (14.0, 24.0, 34.0)])
    b_st = np.array([D.OK, D.OK, D.BAD_WINDOW, D.EMPTY, D.OK], np.int32)
    out, st, which = D.select(a, a_st, b, b_st)
    assert which.tolist() == [0, 1, 1, 1, 1] and st.dtype == np.int32 and out.dtype == np.float64
    assert out[0].tolist() == [1.0, 2.0, 3.0] and st[0] == D.OK                       # OK + finite: a
    assert out[1].tolist() == [11.0, 21.0, 31.0] and st[1] == D.OK                    # OK + a NaN component: b
    assert out[2].tolist() == [12.0, 22.0, 32.0] and st[2] == D.BAD_WINDOW            # not OK: b, with b's status
    assert np.isnan(out[3]).all() and st[3] == D.EMPTY                                # both lost: b's NaN and b's code
    assert out[4].tolist() == [14.0, 24.0, 34.0]                                      # an infinite component is not a centre either


def test_predictor_options_are_validated_before_anything_is_built(lib, monkeypatch):
    import torch
    import awr_amd
    net = awr_amd.get_deconv_net(18, 14, 2)          # on the host: the option checks come before the GPU check and before any plan
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (so the test says the same on a GPU box)

    def make(**kw):
        return awr_amd.Predictor(net, 128, 0.4, **kw)
    for bad in (dict(recenter=5), dict(recenter=-1), dict(max_shift=-1), dict(max_shift=float("nan")), dict(center_joints=[0, 14]),
                dict(center_joints=[-1]), dict(center_joints=[])):
        with pytest.raises(ValueError):
            make(**bad)
    for bad in (dict(recenter="1"), dict(recenter=True), dict(recenter=1.0), dict(track="yes"), dict(track=1), dict(max_shift="1"),
                dict(center_joints="012"), dict(center_joints=[0.5])):
        with pytest.raises(TypeError):
            make(**bad)
    # valid options get as far as the GPU check
    with pytest.raises(lib.AwrError, match=r"detect\.detect"):
        make(recenter=4, track=True, center_joints=[0, 3, 13], max_shift=float("inf"))


def test_predict_py_accepts_the_new_flags():
    sys.path.insert(0, REPO)
    try:
        import predict
    finally:
        sys.path.remove(REPO)
    a = predict.parse_args(["frames.npy", "--load-model", "x.pth"])
    assert a.recenter == 0 and a.track is False
    a = predict.parse_args(["frames.npy", "--load-model", "x.pth", "--recenter", "2", "--track"])
    assert a.recenter == 2 and a.track is True
    with pytest.raises(SystemExit):
        predict.parse_args(["frames.npy", "--load-model", "x.pth", "--recenter", "two"])
