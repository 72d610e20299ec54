"""CPU: the numpy statements of the background model (awr_amd.background.learn and foreground) against hand-written
expectations and against the per-pixel loops of tests/background_cases.py; the option checks; the exports; and the premise of the GPU
predictor tests: the detector ends OK on every masked frame they use."""
import numpy as np
import pytest

import background_cases as BC


@pytest.fixture(scope="module")
def BG():
    import awr_amd  # noqa: F401
    from awr_amd import background
    return background


def u16(*v):
    return np.array([v], np.uint16)


def test_the_margin_is_a_strict_integer_comparison(BG):
    d, m = u16(870, 869, 871, 870, 870), u16(900, 900, 900, 901, 899)
    out, new = BG.foreground(d, m, margin=30.0)
    assert out.tolist() == [[0, 869, 0, 870, 0]]          # d + margin == m is dropped, d + margin == m - 1 is kept
    assert np.array_equal(new, m) and new is not m
    assert BG.foreground(d, m, margin=30.9)[0].tolist() == [[0, 869, 0, 870, 0]]          # floor(margin)
    assert BG.foreground(d, m, margin=29.999)[0].tolist() == [[870, 869, 0, 870, 0]]


def test_no_sixteen_bit_wrap(BG):
    # d + margin = 131070: in 16 bits it would be 65534 < 65535 and the pixel would be kept
    out, _ = BG.foreground(u16(65535, 1, 65534), u16(65535, 65535, 65535), margin=65535)
    assert out.tolist() == [[0, 0, 0]]
    assert BG.foreground(u16(65535, 1, 65534), u16(65535, 65535, 65535), margin=65533)[0].tolist() == [[0, 1, 0]]


def test_unknown_zero_and_the_margins_ends(BG):
    d, m = u16(700, 0, 700, 0), u16(0, 0, 900, 900)
    assert BG.foreground(d, m, unknown="keep")[0].tolist() == [[700, 0, 700, 0]]
    assert BG.foreground(d, m, unknown="drop")[0].tolist() == [[0, 0, 700, 0]]
    # margin = 0: everything strictly nearer than the model; margin = inf: floor(min(inf, 65535)) = 65535, nothing in front of a known model
    assert BG.foreground(u16(899, 900, 901), u16(900, 900, 900), margin=0)[0].tolist() == [[899, 0, 0]]
    assert BG.foreground(u16(1, 899, 5), u16(65535, 900, 0), margin=float("inf"))[0].tolist() == [[0, 0, 5]]
    # an all-zero model with unknown="keep" passes a frame through
    f = BC.apply_cases()["37x53_wide"][0]
    assert np.array_equal(BG.foreground(f, np.zeros_like(f))[0], f)


def test_adapt_steps_towards_the_frame_and_only_at_background_pixels(BG):
    #          far behind  far in front (kept)  just in front (bg)  d == m  zero  unknown  one behind  within the step
    d = u16(1000, 700, 895, 900, 0, 700, 901, 903)
    m = u16(900, 900, 900, 900, 900, 0, 900, 900)
    out, new = BG.foreground(d, m, margin=30, adapt=5)
    assert out.tolist() == [[0, 700, 0, 0, 0, 700, 0, 0]]
    assert new.tolist() == [[905, 900, 895, 900, 900, 0, 901, 903]]
    assert BG.foreground(u16(891), u16(900), margin=10, adapt=5)[1].tolist() == [[895]]          # clamped in the other direction
    assert BG.foreground(d, m, margin=30, adapt=None)[1].tolist() == m.tolist()
    # the ends of the range: the model stays in [1, 65535]
    assert BG.foreground(u16(65535, 1), u16(65530, 1), margin=0, adapt=65535)[1].tolist() == [[65535, 1]]


def test_a_chain_of_six_steps(BG):
    d, m = u16(1000, 896, 700), u16(988, 900, 900)          # behind the model, 4 mm in front of it (inside the margin), a hand
    seen = []
    for _ in range(6):
        out, m = BG.foreground(d, m, margin=5, adapt=3)
        seen.append(m.tolist()[0])
        assert out.tolist() == [[0, 0, 700]]
    assert seen == [[991, 897, 900], [994, 896, 900], [997, 896, 900], [1000, 896, 900], [1000, 896, 900], [1000, 896, 900]]


@pytest.mark.parametrize("name", [n for n in BC.apply_cases() if not n.startswith("48x64")])
def test_foreground_equals_the_loop(BG, name):
    d, m = BC.apply_cases()[name]
    for o in BC.options():
        want, got = BC.loop_foreground(d, m, **o), BC.apply_reference(name, **o)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), o
        assert got[0].dtype == np.uint16 and got[1].dtype == np.uint16


def test_foreground_equals_the_loop_at_48x64(BG):
    for name in BC.apply_groups()[(48, 64)]:
        d, m = BC.apply_cases()[name]
        for o in BC.options(thin=True):
            want, got = BC.loop_foreground(d, m, **o), BC.apply_reference(name, **o)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, o)


def test_learning_by_hand(BG):
    f = np.array([[[5, 0, 7, 0]], [[3, 0, 7, 9]], [[4, 0, 0, 0]], [[9, 0, 7, 8]]], np.uint16)          # V: {3,4,5,9}, {}, {7,7,7}, {8,9}
    assert BG.learn(f, "min").tolist() == [[3, 0, 7, 8]]
    assert BG.learn(f, "median").tolist() == [[4, 0, 7, 8]]          # even |V|: the LOWER median
    assert BG.learn(f, "max").tolist() == [[9, 0, 7, 9]]
    assert BG.learn(f, "median", min_valid=3).tolist() == [[4, 0, 7, 0]]          # valid in min_valid - 1 = 2 frames: 0; in 3: a value
    assert BG.learn(f, "max", min_valid=4).tolist() == [[9, 0, 0, 0]]
    assert BG.learn(f[:1]).tolist() == [[5, 0, 7, 0]]
    assert BG.learn(f[:2], "median").tolist() == [[3, 0, 7, 9]]
    assert BG.learn(f).dtype == np.uint16


@pytest.mark.parametrize("n", BC.LEARN_N)
def test_learn_equals_the_loop(BG, n):
    for shape in ((16, 8), (37, 53)) if n <= 3 else ((16, 8),):
        f = BC.learn_frames(shape, n)
        for o in BC.learn_options(n):
            assert np.array_equal(BC.learn_reference(shape, n, o["rank"], o["min_valid"]), BC.loop_learn(f, **o)), (shape, o)
    # row 0, column 3 + u is valid in exactly u frames: 0 below min_valid, a value from it on
    f = BC.learn_frames((16, 8), n)
    for k in sorted({1, min(2, n), n}):
        got = BC.learn_reference((16, 8), n, "max", k)
        for u in range(min(5, n + 1)):
            assert (got[0, 3 + u] != 0) == (u >= k), (n, k, u)


def test_refusals(BG):
    d, m = u16(1, 2), u16(3, 4)
    for kw, err in ((dict(margin=-1.0), ValueError), (dict(margin=float("nan")), ValueError), (dict(margin="30"), TypeError), (dict(margin=True), TypeError),
                    (dict(unknown="maybe"), ValueError), (dict(adapt=0), ValueError), (dict(adapt=65536), ValueError), (dict(adapt=1.5), TypeError),
                    (dict(adapt=True), TypeError)):
        with pytest.raises(err):
            BG.foreground(d, m, **kw)
    with pytest.raises(ValueError):
        BG.foreground(d, u16(1, 2, 3))
    with pytest.raises(ValueError):
        BG.foreground(d.astype(np.int32), m)
    f = np.zeros((3, 2, 2), np.uint16)
    for kw, err in ((dict(rank="mean"), ValueError), (dict(min_valid=0), ValueError), (dict(min_valid=4), ValueError), (dict(min_valid=1.0), TypeError)):
        with pytest.raises(err):
            BG.learn(f, **kw)
    with pytest.raises(ValueError):
        BG.learn(np.zeros((65, 2, 2), np.uint16))
    with pytest.raises(ValueError):
        BG.learn(np.zeros((0, 2, 2), np.uint16))
    with pytest.raises(ValueError):
        BG.learn(f[0])


def test_the_option(BG):
    assert BG.check_background_option(None) is None
    assert BG.check_background_option(True) == dict(margin=30.0, unknown="keep", adapt=None, shared=True, rank="median", min_valid=1) == BG.BACKGROUND_DEFAULTS
    got = BG.check_background_option(dict(margin=10, adapt=2, shared=False, rank="min"))
    assert got == dict(margin=10.0, unknown="keep", adapt=2, shared=False, rank="min", min_valid=1) and isinstance(got["margin"], float)
    for bad, err in ((False, TypeError), ("on", TypeError), (dict(step=2), ValueError), (dict(shared=1), TypeError), (dict(margin=-2), ValueError),
                     (dict(rank="mean"), ValueError), (dict(min_valid=65), ValueError), (dict(adapt=0), ValueError), (dict(unknown=None), ValueError)):
        with pytest.raises(err):
            BG.check_background_option(bad)


def test_the_library_exports_the_entry_points_and_the_constants_agree(BG):
    import re
    from pathlib import Path
    from awr_amd import _lib as L
    for name in ("awr_background_learn", "awr_frames_foreground"):
        assert hasattr(L.lib, name) and name in L.EXPORTS and not L.MISSING
    header = (Path(__file__).resolve().parent.parent / "include" / "awr_hip.h").read_text()
    const = {k: int(v) for k, v in re.findall(r"#define (AWR_BG_\w+) (\d+)", header)}
    assert const == dict(AWR_BG_MAX_FRAMES=BG.MAX_FRAMES, AWR_BG_MIN=BG.RANKS["min"], AWR_BG_MEDIAN=BG.RANKS["median"], AWR_BG_MAX=BG.RANKS["max"])


def test_predict_py_parses_the_flags():
    import predict
    base = ["frames.npy", "--load-model", "m.pth"]
    assert predict.background_config(predict.parse_args(base)) is None
    assert predict.background_config(predict.parse_args(base + ["--background", "e.npy"])) is True
    args = predict.parse_args(base + ["--background", "e.npy", "--background-margin", "12.5", "--background-adapt", "2"])
    assert predict.background_config(args) == dict(margin=12.5, adapt=2)
    with pytest.raises(SystemExit):
        predict.background_config(predict.parse_args(base + ["--background-margin", "10"]))


def test_the_detector_ends_ok_on_every_masked_frame_of_the_predictor_tests(BG):
    """the premise of tests/test_background_gpu.py's predictor tests: on the cluttered frames the "nearest" seed lands on the bar, on the
    masked frames the detector finds the hand, and masking the composite equals masking the clutter-free frame"""
    from awr_amd import detect as D
    sc = BC.scene()
    assert sc.model.min() > 0 and np.array_equal(sc.model[200:204, 300:308], BC.loop_learn(sc.empty[:, 200:204, 300:308]))
    for i in range(BC.N_SCENE):
        c, st = D.detect(sc.frames[i])
        assert st == D.OK and c[1] > 400 and abs(c[2] - BC.BAR_MM) < 40          # the bar, not the hand
        c, st = D.detect(sc.masked[i])
        want, want_st = D.detect(BG.foreground(sc.hands[i], sc.model)[0])
        assert st == D.OK and want_st == D.OK and 600 < c[2] < 1000 and c[1] < 400
        assert np.array_equal(sc.masked[i], BG.foreground(sc.hands[i], sc.model)[0]) and c == want
        assert (sc.masked[i] != 0).sum() > 1000
