"""CPU: the numpy statement of awr_frames_denoise (awr_amd.detect.denoise) against the per-pixel loop of
tests/denoise_cases.py on every case, the consequences of the rule, one 480 x 640 noisy two-hand composite on a band of rows, and the
argument checks -- in Python, in the entry point before it looks at a pointer, and in the Predictor's constructor before it looks for a
GPU."""
import numpy as np
import pytest

import denoise_cases as DC


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


@pytest.mark.parametrize("shape", list(DC.groups()), ids=lambda s: "%dx%d" % s)
def test_statement_equals_the_loop(D, shape):
    """every case at its options: the whole grid on the frames smaller than the window, a diagonal through it on the larger ones, and the
    threshold cases (steps, holes, speckles) at the options that make their count or their step the threshold"""
    for name in DC.groups()[shape]:
        frame = DC.cases()[name]
        for o in DC.options_for(name):
            got = D.denoise(frame, **o)
            assert got.dtype == np.uint16 and got.shape == frame.shape
            assert np.array_equal(got, DC.reference(name, o["radius"], o["edge"], o["support"], o["fill"])), (name, o)


def test_thresholds_decide_what_they_are_built_to_decide(D):
    """the cases bite: a step of exactly `edge` is smoothed across and a step of edge + 1 is not; a hole with `fill` valid neighbours is
    filled and one with fill - 1 is not; a speckle with `support` similar neighbours stays and one with support - 1 goes"""
    c = DC.cases()
    for where, (v, u) in (("row16", (16, 30)), ("col64", (10, 64)), ("inside_row", (5, 30)), ("inside_col", (10, 20))):
        for edge in (40, 12.5, 0):
            e = int(np.floor(edge))
            exact, plus1 = c["33x130_step_exact_%s_e%g" % (where, edge)], c["33x130_step_plus1_%s_e%g" % (where, edge)]
            # the first pixel behind the step: 3 of its 9 window values are in front of it
            a = D.denoise(exact, 1, edge)
            assert a[v, u] == DC.NEAR + e and np.array_equal(a, exact)          # 6 of 9 on its side: the median stays, also across the step
            assert np.array_equal(D.denoise(plus1, 1, edge), plus1)
            # with support 6 the pixel needs neighbours across the step: it has 8 within `edge` on the exact step, 5 on the other
            assert D.denoise(exact, 1, edge, support=6)[v, u] == DC.NEAR + e and D.denoise(plus1, 1, edge, support=6)[v, u] == 0
    for shape in DC.TILES:
        tag = "%dx%d_" % shape
        for r, k in ((1, 1), (1, 6), (2, 6), (2, 24)):
            v, u = DC.sites(shape)[0]
            full, short = c[tag + "holes_r%d_fill%d_n%d" % (r, k, k)], c[tag + "holes_r%d_fill%d_n%d" % (r, k, k - 1)]
            # the k valid neighbours are NEAR, NEAR + 3, ...: their lower median is element (k - 1) // 2
            assert full[v, u] == 0 and D.denoise(full, r, None, 0, k)[v, u] == DC.NEAR + 3 * ((k - 1) // 2)
            assert short[v, u] == 0 and D.denoise(short, r, None, 0, k)[v, u] == 0
        for r, k in ((1, 1), (1, 3), (2, 3), (2, 24)):
            for v, u in DC.sites(shape)[:1] + DC.sites(shape)[3:]:
                full, short = c[tag + "speckles_r%d_support%d_n%d" % (r, k, k)], c[tag + "speckles_r%d_support%d_n%d" % (r, k, k - 1)]
                assert D.denoise(full, r, 40, k)[v, u] != 0 and D.denoise(short, r, 40, k)[v, u] == 0 and short[v, u] == DC.NEAR


def test_even_counts_take_the_nearer_surface(D):
    for shape in DC.TILES + DC.ODD:
        f = DC.cases()["%dx%d_two_surfaces" % shape]
        for r in (1, 2):
            out = D.denoise(f, r, 30)
            assert (out[f > 0] == DC.NEAR).all() and not out[f == 0].any() and (f == DC.NEAR + 30).sum() == (f == DC.NEAR).sum() > 0
            assert np.array_equal(D.denoise(f, r, 29), f)          # the surfaces apart: each pixel with its row neighbour, the lower median of two equals


def test_consequences_of_the_rule(D):
    for name, f in DC.cases().items():
        if f.shape not in DC.TINY + DC.ODD and "random" not in name and "noise" not in name and "checker" not in name:
            continue
        for r in (1, 2):
            d = f.astype(np.int64)
            # support 0, no fill: zeros stay zero, the others stay non-zero
            for edge in (None, 12.5):
                out = D.denoise(f, r, edge)
                assert np.array_equal(out == 0, f == 0), name
            # with an edge no depth moves further than elim, whatever support and fill are
            for edge, support, fill in ((12.5, 0, None), (40, 3, 1), (0, 1, 6)):
                out = D.denoise(f, r, edge, support, fill).astype(np.int64)
                both = (out != 0) & (d != 0)
                assert (np.abs(out - d)[both] <= int(np.floor(edge))).all(), name
                # every non-zero output occurs in the pixel's window of the input
                pad = np.zeros((f.shape[0] + 2 * r, f.shape[1] + 2 * r), np.int64)
                pad[r:r + f.shape[0], r:r + f.shape[1]] = d
                occurs = np.zeros(f.shape, bool)
                for dv in range(2 * r + 1):
                    for du in range(2 * r + 1):
                        occurs |= pad[dv:dv + f.shape[0], du:du + f.shape[1]] == out
                assert occurs[out != 0].all(), name
    # a constant frame is a fixed point, at every option that removes nothing in the interior
    for shape in DC.SIZES:
        for value in (1, DC.NEAR, 65535):
            f = np.full(shape, value, np.uint16)
            for o in (dict(), dict(radius=2, edge=0), dict(radius=1, edge=40, fill=1), dict(radius=2, edge=None, fill=24)):
                assert np.array_equal(D.denoise(f, **o), f)


def test_no_edge_the_largest_edge_and_infinity_agree(D):
    for name in ("33x130_random_wide", "17x67_random_wide", "48x64_extremes", "5x3_random_wide"):
        f = DC.cases()[name]
        for r, support, fill in ((1, 0, None), (1, 3, 1), (2, 8, 6)):
            want = D.denoise(f, r, None, support, fill)
            for edge in (65535, 65535.5, float("inf"), 1e12):
                assert np.array_equal(D.denoise(f, r, edge, support, fill), want), (name, edge)
    # 1 next to 65535 is a step of 65534: the largest edge that still separates them is 65533
    f = DC.cases()["48x64_extremes"]
    # (an interior pixel has 5 neighbours on its own stripe and 3 on the other: support 6 needs the other stripe)
    assert np.array_equal(D.denoise(f, 1, 65534, 6)[1:-1, 1:-1], f[1:-1, 1:-1]) and not D.denoise(f, 1, 65533, 6).any()


def test_full_frame_band_against_the_loop(D):
    """480 x 640, two noisy hands: the statement on the whole frame equals the loop on a 64-row band through both hands (the band is cut
    with `radius` rows of context, which the loop's own frame edge then never sees)"""
    f = DC.noisy_host()[0]
    rows = np.flatnonzero((f > 0).any(1))
    lo = int(rows[len(rows) // 2]) - 32
    assert lo >= 2 and lo + 66 <= f.shape[0] and (f[lo:lo + 64] > 0).sum() > 2000
    for o in DC.FULL_OPTIONS:
        r = o["radius"]
        got = D.denoise(f, **o)
        band = DC.loop(f[lo - r:lo + 64 + r], **o)[r:-r]
        assert np.array_equal(got[lo:lo + 64], band), o
        assert not np.array_equal(got, f)                      # the noise is there and the filter moves it


def test_bad_values_raise(D):
    f = np.full((4, 4), 700, np.uint16)
    bad = [(dict(radius=0), ValueError, "radius"), (dict(radius=3), ValueError, "radius"), (dict(radius=True), TypeError, "radius"),
           (dict(radius=1.0), TypeError, "radius"), (dict(radius="1"), TypeError, "radius"),
           (dict(support=-1), ValueError, "support"), (dict(support=9), ValueError, "support"), (dict(radius=2, support=25), ValueError, "support"),
           (dict(support=True), TypeError, "support"), (dict(support=1.0), TypeError, "support"), (dict(support=None), TypeError, "support"),
           (dict(fill=0), ValueError, "fill"), (dict(fill=9), ValueError, "fill"), (dict(radius=2, fill=25), ValueError, "fill"),
           (dict(fill=False), TypeError, "fill"), (dict(fill=2.0), TypeError, "fill"),
           (dict(edge=-1), ValueError, "edge"), (dict(edge=float("nan")), ValueError, "edge"), (dict(edge=float("-inf")), ValueError, "edge"),
           (dict(edge="40"), TypeError, "edge"), (dict(edge=True), TypeError, "edge")]
    for kw, exc, word in bad:
        with pytest.raises(exc, match=word):
            D._check_denoise(**kw)
        with pytest.raises(exc, match=word):
            D.denoise(f, **kw)
    assert D._check_denoise(np.int64(2), np.float32(3), np.int32(24), np.int64(24)) == (2, 3.0, 24, 24)
    assert D._check_denoise() == (1, None, 0, None) and D._check_denoise(1, 40, 8, 8) == (1, 40.0, 8, 8)
    with pytest.raises(ValueError, match="uint16"):
        D.denoise(f.astype(np.int32))
    assert D.check_denoise_option(None) is None and D.check_denoise_option(True) == dict(radius=1, edge=40.0, support=0, fill=None)
    assert D.check_denoise_option(dict(radius=2, fill=6)) == dict(radius=2, edge=40.0, support=0, fill=6)
    assert D.check_denoise_option(dict(edge=None))["edge"] is None
    for opt, exc in ((False, TypeError), (1, TypeError), ("on", TypeError), (dict(window=3), ValueError)):
        with pytest.raises(exc, match="denoise"):
            D.check_denoise_option(opt)


def test_bad_values_raise_in_the_entry_point_and_the_predictor_without_a_gpu(D):
    """the entry point names itself and the value before it looks at a pointer or launches anything; the constructor reaches
    _check_denoise before it looks for a GPU"""
    import awr_amd
    from awr_amd import _lib as L
    inf = float("inf")
    entry = lambda radius=1, edge=inf, support=0, fill=0, ftype=0: L.lib.awr_frames_denoise(None, ftype, 1, 8, 8, None, 1, radius, edge, support,
                                                                                        fill, None, None, None)
    for kw, word in ((dict(radius=0), "radius = 0"), (dict(radius=3), "radius = 3"), (dict(edge=-1.0), "edge = -1"), (dict(edge=float("nan")), "edge = "),
                     (dict(edge=-inf), "edge = -inf"), (dict(support=-1), "support = -1"), (dict(support=9), "support = 9"),
                     (dict(radius=2, support=25), "support = 25"), (dict(fill=-1), "fill = -1"), (dict(fill=9), "fill = 9"),
                     (dict(radius=2, fill=25), "fill = 25"), (dict(ftype=1), "uint16")):
        assert entry(**kw) == -1 and "awr_frames_denoise: " in L.last_error() and word in L.last_error(), (kw, L.last_error())
    for kw in (dict(), dict(radius=2, support=24, fill=24), dict(edge=0.0), dict(edge=12.5, support=8, fill=8)):
        assert entry(**kw) == -1 and L.last_error() == "awr_frames_denoise: NULL pointer", (kw, L.last_error())
    for kw in (dict(radius=True), dict(support=1.5), dict(fill="1"), dict(edge="40")):
        with pytest.raises(TypeError, match=list(kw)[0]):
            D.denoise_device(None, [0], **kw)
    for opt, exc, word in ((dict(radius=3), ValueError, "radius"), (dict(edge=-1), ValueError, "edge"), (dict(support=9), ValueError, "support"),
                           (dict(fill=0), ValueError, "fill"), (dict(fill=True), TypeError, "fill"), (False, TypeError, "denoise"),
                           (dict(kernel=3), ValueError, "denoise")):
        with pytest.raises(exc, match=word):
            awr_amd.Predictor(None, 64, 1.0, denoise=opt)
        with pytest.raises(exc, match=word):
            awr_amd.Predictor(None, 64, 1.0, hands=2, isolate=True, edge_mm=40, denoise=opt)


def test_predict_py_takes_denoise():
    import predict
    base = ["frames.npy", "--load-model", "x.pth"]
    assert predict.denoise_config(predict.parse_args(base)) is None
    assert predict.denoise_config(predict.parse_args(base + ["--denoise"])) is True
    assert predict.denoise_config(predict.parse_args(base + ["--denoise", "2,40,6,18"])) == dict(radius=2, edge=40.0, support=6, fill=18)
    assert predict.denoise_config(predict.parse_args(base + ["--denoise", "1,none,0,None"])) == dict(radius=1, edge=None, support=0, fill=None)
    for bad in ("2,40,6", "a,b,c,d", "1,40,0.5,none"):
        with pytest.raises(SystemExit, match="--denoise"):
            predict.denoise_config(predict.parse_args(base + ["--denoise", bad]))
