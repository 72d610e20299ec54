"""CPU: the marshalling of awr_amd.detect_calls against the prototypes of _lib._SIGS (which tests/test_abi.py ties to include/awr_hip.h).
_lib.call is replaced by a recorder and _lib.stream by a stub, every function is called with plain integer addresses, and each recorded
call is checked slot by slot: how many arguments, what type each one has, what the None conventions send and which entry point is named."""
import ctypes as C
import math
import os
import types

import pytest

STREAM = 0x5000
SRC = (0x1000, 0, 6, 120, 160)                                       # a frame source: address, ftype, n_frames, fh, fw
PARAS, FLIP, RANGE = (147, 146.8, 80, 60.0), -1, (200, 1200.0)     # ints among them on purpose: the conversions are the module's


@pytest.fixture(scope="module")
def lib():
    import awr_amd  # noqa: F401
    from awr_amd import build
    if not os.path.exists(build.LIB):
        build.build_lib(verbose=False)
    from awr_amd import _lib
    return _lib


@pytest.fixture
def calls(lib, monkeypatch):
    recorded = []
    monkeypatch.setattr(lib, "call", lambda name, *args: recorded.append((name, args)))
    monkeypatch.setattr(lib, "stream", lambda: STREAM)
    return recorded


def cases():
    """name -> (entry point expected, function name, arguments); p(i) are distinct fake addresses"""
    from awr_amd import track as T
    p = lambda i: 0x10000 + 256 * i          # noqa: E731
    euro, ident = T.check_filter(True), T.check_identity(True)
    return {
        "denoise": ("awr_frames_denoise", "awr_frames_denoise", SRC + (p(0), 2, 1, 40, 0, 3, p(1), p(2))),
        "denoise_none": ("awr_frames_denoise", "awr_frames_denoise", SRC + (p(0), 2, 2, None, 2, None, p(1), p(2))),
        "detect": ("awr_detect", "awr_detect", SRC + (p(0), 2, "nearest", None, RANGE, 100, p(1), False, PARAS, 2, 0, p(2), p(3), p(4))),
        "detect_given": ("awr_detect", "awr_detect", SRC + (p(0), 2, "given", p(5), RANGE, 100.0, p(1), True, PARAS, 0, 4, p(2), p(3), p(4))),
        "palm": ("awr_detect_palm", "awr_detect_palm", SRC + (p(0), 2, p(1), p(2), RANGE, p(3), False, PARAS, 2, (1, 3), (25, 4), p(4), p(1), p(2), p(5))),
        "palm_no_info": ("awr_detect_palm", "awr_detect_palm", SRC + (p(0), 2, p(1), p(2), RANGE, p(3), True, PARAS, 2.0, (1, 3), (25, 4), p(4), p(6), p(7), None)),
        "hands": ("awr_detect_hands", "awr_detect_hands", SRC + (p(0), 2, 2, RANGE, 300, None, 100, 400, p(1), None, p(2), p(3), p(4), p(5))),
        "hands_edge": ("awr_detect_hands_edge", "awr_detect_hands", SRC + (p(0), 2, 2, RANGE, 300.0, 40, 100.0, 400, p(1), p(6), p(2), p(3), p(4), p(5))),
        "isolate": ("awr_hands_isolate", "awr_hands_isolate", SRC + (p(0), 2, 2, p(1), p(2), p(3), p(4))),
        "select": ("awr_centers_select", "awr_centers_select", (p(0), p(1), p(2), p(3), 2, p(4), p(5), p(6))),
        "select_no_which": ("awr_centers_select", "awr_centers_select", (p(0), p(1), p(2), p(3), 2, p(4), p(5), None)),
        "assign": ("awr_hands_assign", "awr_hands_assign", (p(0), p(1), p(2), p(3), p(4), p(5), p(6), p(7), 2, 2, 1, ident, PARAS, FLIP, p(8), p(9), 14,
                                                            p(10), p(11), p(12), p(13), p(14), p(15))),
        "assign_bare": ("awr_hands_assign", "awr_hands_assign", (p(0), p(1), p(2), p(3), p(4), p(5), None, None, 2, 2, 2, ident, PARAS, FLIP, None, None, 0,
                                                                 p(10), p(11), p(12), p(13), p(14), p(15))),
        "samples": ("awr_detect_samples", "awr_detect_samples", (p(0), p(1), False, 6, p(2), 2, 64, 120, 160, PARAS, FLIP, p(3), p(4), p(5), p(6), p(7))),
        "samples_rows": ("awr_detect_samples", "awr_detect_samples", (p(0), p(1), True, 6, p(2), 6, 64, 120, 160, PARAS, FLIP, p(3), p(4), p(5), p(6), p(7))),
        "unproject": ("awr_joints_unproject", "awr_joints_unproject", (p(0), p(1), p(2), p(3), 2, 14, 1, 64, PARAS, FLIP, p(4), p(5), p(6))),
        "view_centers": ("awr_view_centers", "awr_view_centers", (p(0), p(1), p(2), False, p(3), 3, 2, 2, PARAS, FLIP, p(4), p(5), p(6), p(7))),
        "view_rotate": ("awr_view_rotate", "awr_view_rotate", (p(0), p(1), p(2), p(3), 3, 2, 1)),
        "fuse": ("awr_views_fuse", "awr_views_fuse", (p(0), p(1), p(2), None, "median", 3, 2, 14, 2, PARAS, FLIP, p(3), p(4), p(5), p(6))),
        "fuse_conf": ("awr_views_fuse", "awr_views_fuse", (p(0), p(1), p(2), p(7), "conf", 3, 2, 14, 2, PARAS, FLIP, p(3), p(4), p(5), p(6))),
        "center": ("awr_joints_center", "awr_joints_center", (p(0), p(1), p(2), p(3), p(4), p(5), 2, 14, 2, None, PARAS, FLIP, RANGE, 1, p(6), None, p(7))),
        "center_joints": ("awr_joints_center", "awr_joints_center", (p(0), p(1), p(2), p(3), p(4), p(5), 2, 14, 1, (p(8), 5), PARAS, FLIP, RANGE, 0.5, p(6),
                                                                     p(9), p(7))),
        "filter": ("awr_joints_filter", "awr_joints_filter", (p(0), p(1), p(2), p(3), p(4), None, 2, 14, 2, 1, euro._replace(gate_mm=None), PARAS, FLIP,
                                                              p(5), p(6), p(7), p(8))),
        "filter_conf": ("awr_joints_filter", "awr_joints_filter", (p(0), p(1), p(2), p(3), p(4), p(9), 2, 14, 1, 1 / 30, euro._replace(gate_mm=80, weight="conf"),
                                                                   PARAS, FLIP, p(5), p(6), p(7), p(8))),
        "fields": ("awr_confidence_fields", "awr_confidence_fields", (p(0), p(1), p(2), p(3), p(4), 2, 14, 2, p(5), p(6), p(7))),
    }


def run(calls, case):
    from awr_amd import detect_calls as DC
    entry, fn, args = cases()[case]
    getattr(DC, fn)(*args)
    assert len(calls) == 1, "one L.call per function"
    name, sent = calls.pop()
    assert name == entry
    return sent


NAMES = ["denoise", "denoise_none", "detect", "detect_given", "palm", "palm_no_info", "hands", "hands_edge", "isolate", "select", "select_no_which",
         "assign", "assign_bare", "samples", "samples_rows", "unproject", "view_centers", "view_rotate", "fuse", "fuse_conf", "center", "center_joints",
         "filter", "filter_conf", "fields"]


def test_every_function_of_the_module_is_a_case():
    from awr_amd import detect_calls as DC
    public = {n for n, f in vars(DC).items() if isinstance(f, types.FunctionType) and not n.startswith("_")}
    assert sorted(cases()) == sorted(NAMES)
    assert public == {fn for _, fn, _ in cases().values()} and len(public) == 15
    assert len({entry for entry, _, _ in cases().values()}) == 16


@pytest.mark.parametrize("case", NAMES)
def test_count_and_type_of_every_slot(lib, calls, case):
    sent = run(calls, case)
    proto = lib._SIGS[cases()[case][0]][0]
    assert len(sent) == len(proto), (len(sent), len(proto))
    assert sent[-1] == STREAM
    for i, (x, t) in enumerate(zip(sent, proto)):
        if t is C.c_void_p:
            assert x is None or type(x) is int, (i, x)
        elif t in (C.c_int, C.c_int64):
            assert type(x) is int, (i, x)          # (type(True) is bool: a bool fails here)
        else:
            assert t in (C.c_double, C.c_float) and type(x) is float, (i, t, x)


def test_none_conventions(calls):
    d = run(calls, "denoise_none")
    assert d[8] == math.inf and d[10] == 0 and (d[7], d[9]) == (2, 2)
    d = run(calls, "denoise")
    assert d[8] == 40.0 and d[10] == 3
    f = run(calls, "filter")
    assert f[13] == -1.0 and f[15] == 0
    f = run(calls, "filter_conf")
    assert f[13] == 80.0 and f[15] == 1 and f[9] == 1 / 30
    c = run(calls, "center")
    assert c[9:11] == (None, 0) and c[11:16] == (147.0, 146.8, 80.0, 60.0, -1) and c[16:19] == (200.0, 1200.0, 1.0) and c[20] is None
    c = run(calls, "center_joints")
    assert c[9:11] == (0x10000 + 256 * 8, 5)
    assert run(calls, "palm_no_info")[23] is None and run(calls, "select_no_which")[7] is None
    a = run(calls, "assign_bare")
    assert a[6:8] == (None, None) and a[19:22] == (None, None, 0)


def test_edge_picks_the_entry_point(calls):
    plain, edge = run(calls, "hands"), run(calls, "hands_edge")          # (run asserts the names: awr_detect_hands, awr_detect_hands_edge)
    assert edge[11] == 40.0 and plain[:11] == edge[:11] and plain[11:13] == edge[12:14] == (100.0, 400)
    assert plain[14] is None and edge[15] == 0x10000 + 256 * 6           # labels: NULL, or the address


def test_strides_codes_and_the_camera(calls):
    assert run(calls, "samples")[2] == 0 and run(calls, "samples_rows")[2] == 3
    assert run(calls, "samples")[9:14] == (147.0, 146.8, 80.0, 60.0, -1)
    d, g = run(calls, "detect"), run(calls, "detect_given")
    assert (d[7], d[8], d[13]) == (2, None, 0) and (g[7], g[8], g[13]) == (0, 0x10000 + 256 * 5, 3)
    assert d[9:12] == (200.0, 1200.0, 100.0) and d[14:18] == (147.0, 146.8, 2, 0)
    assert run(calls, "palm")[12] == 0 and run(calls, "palm_no_info")[12] == 3 and run(calls, "palm")[15:20] == (2.0, 1, 3, 25, 4)
    assert run(calls, "view_centers")[3] == 0
    assert run(calls, "fuse")[4] == 2 and run(calls, "fuse_conf")[4] == 1
    assert run(calls, "unproject")[7:13] == (64.0, 147.0, 146.8, 80.0, 60.0, -1)
    assert run(calls, "assign")[14:19] == (147.0, 146.8, 80.0, 60.0, -1)
