"""CPU: the scalar arithmetic of csrc/awr_frame.h -- the one device statement of nyu_data.center2bounds (bounds_window, palm_window) and of
evaluator.uvd2xyz / xyz2uvd that awr_detect.hip, awr_palm.hip, awr_hands.hip, awr_track.hip and awr_assign.hip share -- run on the host by
tests/native/frame_math_main.cpp and held to the numpy statements bit for bit.  The header's double arithmetic is numpy's only without
contraction, so the program is built with -ffp-contract=off, as build.SOURCES builds every translation unit that uses it."""
import os
import subprocess
import warnings

import numpy as np
import pytest

from test_host_cpu import _hipcc_clangxx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
FH, FW = 480, 640
CLAMP = 2 ** 30            # trunc_clamped's bound: a pixel bound beyond it stays there, far outside any frame (sides <= 16384)
DEPTHS = np.arange(1, 65536, dtype=np.float64)          # every raw depth that is a measurement


@pytest.fixture(scope="module")
def mods():
    from awr_amd import detect, evaluator, nyu_data
    return detect, evaluator, nyu_data


def _window_cases(paras):
    """[(name, centre, cube, (fx, fy), fh, fw)]: the named edges, then 300 random ones around PARAS and a 480 x 640 frame."""
    f = (paras[0], paras[1])
    c0, cube = (320.0, 240.0, 700.0), (300.0, 300.0, 300.0)
    cases = [("plain", c0, cube, f, FH, FW)]
    for a in range(3):
        for bad in (NAN, INF, -INF):
            c = list(c0)
            c[a] = bad
            cases.append(("centre[%d] = %r" % (a, bad), tuple(c), cube, f, FH, FW))
    cases += [("d = 0", (320.0, 240.0, 0.0), cube, f, FH, FW),
              ("d = 0, cube 0", (320.0, 240.0, 0.0), (0.0, 0.0, 0.0), f, FH, FW),
              ("1e300 pixels right", (1e300, 240.0, 700.0), cube, f, FH, FW),
              ("1e300 pixels left", (-1e300, 240.0, 700.0), cube, f, FH, FW),
              ("1e300 pixels below", (320.0, 1e300, 700.0), cube, f, FH, FW),
              ("1e300 pixels above", (320.0, -1e300, 700.0), cube, f, FH, FW),
              ("3e9 pixels right: outside int32, inside the clamp's reach", (3e9, 240.0, 700.0), cube, f, FH, FW),
              ("wholly left", (-400.0, 240.0, 700.0), cube, f, FH, FW),
              ("wholly right", (1100.0, 240.0, 700.0), cube, f, FH, FW),
              ("wholly above", (320.0, -300.0, 700.0), cube, f, FH, FW),
              ("wholly below", (320.0, 900.0, 700.0), cube, f, FH, FW),
              ("larger than the frame", (320.0, 240.0, 100.0), cube, f, FH, FW),
              ("fh = 1", (320.0, 0.0, 700.0), cube, f, 1, FW),
              ("fw = 1", (0.0, 240.0, 700.0), cube, f, FH, 1),
              ("fh = fw = 1", (0.2, 0.3, 700.0), cube, f, 1, 1),
              ("16384 x 16384", (9000.0, 16000.0, 400.0), cube, f, 16384, 16384),
              ("16384 x 16384, larger than the frame", (8000.0, 8000.0, 2.0), cube, f, 16384, 16384),
              ("zstart > zend: a negative cube depth", c0, (300.0, 300.0, -300.0), f, FH, FW),
              ("fractional zstart / zend", (320.0, 240.0, 700.25), (300.0, 300.0, 100.5), f, FH, FW),
              ("integral zstart / zend", (320.0, 240.0, 700.0), (300.0, 300.0, 100.0), f, FH, FW),
              ("zend = 65535", (320.0, 240.0, 65435.0), (300.0, 300.0, 200.0), f, FH, FW),
              ("zend = 65535.5", (320.0, 240.0, 65435.5), (300.0, 300.0, 200.0), f, FH, FW),
              ("zend = 1e9", (320.0, 240.0, 5e8), (300.0, 300.0, 1e9), f, FH, FW),
              ("negative zend", (320.0, 240.0, -500.0), cube, f, FH, FW),
              ("zstart below 0, zend inside", (320.0, 240.0, 100.0), cube, f, FH, FW),
              ("cube edge 0 in u", c0, (0.0, 300.0, 300.0), f, FH, FW),
              ("cube edge 0 in v", c0, (300.0, 0.0, 300.0), f, FH, FW),
              ("cube edge 0 in d", c0, (300.0, 300.0, 0.0), f, FH, FW),
              ("cube depth NaN", c0, (300.0, 300.0, NAN), f, FH, FW)]
    rng = np.random.default_rng(20)
    for i in range(300):
        c = (rng.uniform(-150.0, FW + 150.0), rng.uniform(-150.0, FH + 150.0), rng.uniform(150.0, 1800.0))
        cb = tuple(rng.uniform(100.0, 500.0, 3))
        fr = (paras[0] * rng.uniform(0.9, 1.1), paras[1] * rng.uniform(0.9, 1.1))
        cases.append(("random %d" % i, c, cb, fr, FH, FW))
    return cases


def _palm_cases(paras):
    """The window cases under search 1.0, 1.5 and 2.0 and a depth range, then the depth-range edges on the plain window."""
    cases = []
    for i, (name, c, cube, f, fh, fw) in enumerate(_window_cases(paras)):
        search = (1.0, 1.5, 2.0)[i % 3]
        zr = ((1.0, 2000.0), (650.5, 749.5), (0.0, 65535.0))[(i // 3) % 3]
        cases.append(("%s, search %g, range %r" % (name, search, zr), c, cube, f, search, zr, fh, fw))
    c0, cube, f = (320.0, 240.0, 700.0), (300.0, 300.0, 300.0), (paras[0], paras[1])
    for search in (1.0, 1.5):
        for zr in ((5.0, 1.0), (700.0, 700.0), (700.25, 700.75), (-50.0, -1.0), (0.0, 1e9), (65535.0, 65535.5), (1.0, 65536.0), (NAN, 2000.0),
                   (1.0, NAN), (-INF, INF)):
            cases.append(("search %g, range %r" % (search, zr), c0, cube, f, search, zr, FH, FW))
    return cases


def _camera_cases(paras):
    """[(point, paras, flip)] for both directions: NaN, infinities, zero depth, then 300 random points."""
    pts = [(320.0, 240.0, 700.0), (0.0, 0.0, 0.0), (100.5, 200.25, 0.0), (NAN, 1.0, 2.0), (1.0, NAN, 2.0), (1.0, 2.0, NAN), (INF, 1.0, 2.0),
           (1.0, -INF, 2.0), (1.0, 2.0, INF), (1e300, -1e300, 1e-300), (-0.0, 0.0, -0.0)]
    rng = np.random.default_rng(21)
    pts += [tuple(rng.uniform(-800.0, 800.0, 2)) + (rng.uniform(150.0, 1800.0),) for _ in range(300)]
    return [(p, paras, flip) for p in pts for flip in (1, -1)]


def _hex(*xs):
    return " ".join(float(x).hex() for x in xs)


def _bits(x):
    return [int(b) for b in np.asarray(x, np.float64).reshape(-1).view(np.uint64)]


def _depth_set(dlo, dhi):
    return (DEPTHS >= dlo) & (DEPTHS <= dhi)


def _empty(w):
    return w[0] >= w[1] or w[2] >= w[3] or w[4] > w[5]


@pytest.fixture(scope="module")
def native(mods, tmp_path_factory):
    """Builds the program and runs it once over every case: -> {"W" | "P" | "C" | "X": [(case, output tokens)]}."""
    paras = mods[2].PARAS
    tmp = tmp_path_factory.mktemp("frame_math")
    exe = str(tmp / "frame_math_main")
    # plain C++ by the clang++ of the library's hipcc; the sanitizers instrument this host program and nothing else
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([_hipcc_clangxx()] + flags + [os.path.join(REPO, "tests", "native", "frame_math_main.cpp"), "-o", exe], check=True)
    cases = {"W": _window_cases(paras), "P": _palm_cases(paras), "C": _camera_cases(paras), "X": _camera_cases(paras)}
    lines = []
    for name, c, cube, f, fh, fw in cases["W"]:
        lines.append("W %s %d %d" % (_hex(*c, *cube, *f), fh, fw))
    for name, c, cube, f, search, zr, fh, fw in cases["P"]:
        lines.append("P %s %d %d" % (_hex(*c, *cube, *f, search, *zr), fh, fw))
    for kind in "CX":
        for p, par, flip in cases[kind]:
            lines.append("%s %s" % (kind, _hex(*p, *par, flip)))
    inp = tmp / "cases.txt"
    inp.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(inp)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    out = [ln.split() for ln in run.stdout.splitlines()]
    assert len(out) == len(lines)
    got, at = {}, 0
    for kind in "WPCX":
        got[kind] = list(zip(cases[kind], out[at:at + len(cases[kind])]))
        at += len(cases[kind])
    return got


def _clipped(window):
    """detect._window's clipped tuple as the device holds it: a bound beyond trunc_clamped's +-2^30 stays there (a lower bound is at least 0
    and an upper one at most the frame's side, so a lower bound meets + 2^30 and an upper one - 2^30).  Such a window is empty either way."""
    u0, u1, v0, v1 = window
    if max(u0, v0) > CLAMP or min(u1, v1) < -CLAMP:
        assert u0 >= u1 or v0 >= v1
    return min(u0, CLAMP), max(u1, -CLAMP), min(v0, CLAMP), max(v1, -CLAMP)


def test_bounds_window_equals_center2bounds_and_window(mods, native):
    """center_bounds = the four doubles center2bounds truncates, bit for bit (recomputed here with its three expressions); bounds_window =
    detect._window exactly: empty where that has no window, its clipped tuple elsewhere (_clipped), and dlo <= d <= dhi admits the raw
    depths 1 .. 65535 that zstart <= d <= zend admits in float64."""
    D, _, ND = mods
    assert len(native["W"]) >= 330
    n_none = n_clamped = 0
    for (name, c, cube, f, fh, fw), tok in native["W"]:
        with np.errstate(all="ignore"):
            center, csize, ff = np.asarray(c, np.float64), np.asarray(cube, np.float64), np.asarray(f, np.float64)
            ustart, vstart = center[:2] - (csize[:2] / 2.0) / center[2] * ff + 0.5
            uend, vend = center[:2] + (csize[:2] / 2.0) / center[2] * ff + 0.5
        assert [int(t, 16) for t in tok[:4]] == _bits([ustart, uend, vstart, vend]), name
        got = tuple(int(t) for t in tok[4:])
        want = D._window(c, cube, f, fh, fw)
        if want is None:
            n_none += 1
            assert _empty(got), name
            continue
        window, zstart, zend = want
        n_clamped += max(window[0], window[2]) > CLAMP or min(window[1], window[3]) < -CLAMP
        assert got[:4] == _clipped(window), name
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert np.array_equal(_depth_set(got[4], got[5]), (DEPTHS >= zstart) & (DEPTHS <= zend)), name
    assert n_none >= 10 and n_clamped >= 5


def test_palm_window_equals_the_statement(mods, native):
    """palm_window = detect._window(c, search * cube, ...) with its depth range intersected with [zmin, zmax], as palm_center states it."""
    D, _, ND = mods
    n_none = 0
    for (name, c, cube, f, search, (zmin, zmax), fh, fw), tok in native["P"]:
        got = tuple(int(t) for t in tok)
        want = D._window(tuple(float(x) for x in c), tuple(search * float(x) for x in cube), f, fh, fw)
        if want is None:
            n_none += 1
            assert _empty(got), name
            continue
        window, zstart, zend = want
        assert got[:4] == _clipped(window), name
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mask = (DEPTHS >= zstart) & (DEPTHS <= zend) & (DEPTHS >= zmin) & (DEPTHS <= zmax)
        assert np.array_equal(_depth_set(got[4], got[5]), mask), name
    assert n_none >= 10


def test_camera_functions_equal_the_evaluator(mods, native):
    """(uvd2x, uvd2y, d) and (xyz2u, xyz2v(y * flip), z) = evaluator.uvd2xyz / xyz2uvd on float64 input before their float32 cast, bit for
    bit (their statements, recomputed here), and after it = the evaluator's own output."""
    _, E, _ = mods
    for kind, fn in (("C", E.uvd2xyz), ("X", E.xyz2uvd)):
        assert len(native[kind]) >= 600
        for (p, paras, flip), tok in native[kind]:
            with np.errstate(all="ignore"):
                q = np.array(p, np.float64).reshape(-1, 3).copy()
                par = np.asarray(paras, np.float64)
                if kind == "C":
                    q[:, :2] = (q[:, :2] - par[2:]) * q[:, 2:] / par[:2]
                    q[:, 1] *= flip
                else:
                    q[:, 1] *= flip
                    q[:, :2] = q[:, :2] * par[:2] / q[:, 2:] + par[2:]
                assert [int(t, 16) for t in tok] == _bits(q[0, :2]), (kind, p, flip)
                got32 = np.array([int(t, 16) for t in tok], np.uint64).view(np.float64).astype(np.float32)
                assert np.array_equal(got32, fn(np.array(p, np.float64), paras, flip)[:2], equal_nan=True), (kind, p, flip)
