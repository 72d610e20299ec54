"""CPU: awr_amd.detect.palm_center, the numpy statement of awr_detect_palm -- its distance transform against the
definition, hand-made silhouettes with known answers against an independent plain-Python form, procedural hands against the detector as it
stands, and argument validation."""
import numpy as np
import pytest

import palm_cases as PC


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


def random_masks():
    r = np.random.RandomState(2024)
    for k in range(200):
        h, w = 12 + r.randint(-3, 4), 17 + r.randint(-3, 4)
        yield r.uniform(size=(h, w)) < (0.35, 0.7, 0.9, 0.97)[k % 4]


def test_distance_transform_equals_the_definition(D):
    n_fg = 0
    for mask in random_masks():
        got = D.distance_transform(mask)
        assert got.dtype == np.int64 and np.array_equal(got, PC.brute_d2(mask)), mask
        n_fg += int(mask.sum())
    assert n_fg > 20000
    for mask in (np.ones((9, 14), bool), np.zeros((5, 7), bool), np.ones((1, 1), bool), np.ones((1, 30), bool), np.ones((30, 1), bool)):
        assert np.array_equal(D.distance_transform(mask), PC.brute_d2(mask))


def test_distance_transform_equals_scipy(D):
    ndi = pytest.importorskip("scipy.ndimage")
    for mask in random_masks():
        ref = ndi.distance_transform_edt(np.pad(mask, 1)) ** 2
        assert np.array_equal(D.distance_transform(mask), np.rint(ref[1:-1, 1:-1]).astype(np.int64))
        assert np.abs(ref - np.rint(ref)).max() < 1e-6


def window_of(D, c):
    from awr_amd import nyu_data as ND
    fh, fw = c["frame"].shape
    u0, u1, v0, v1, zs, ze = ND.center2bounds(c["center"], (600, 600, 600), c["paras"])
    return (max(u0, 0), min(u1, fw), max(v0, 0), min(v1, fh)), int(np.ceil(max(zs, 1.0))), int(np.floor(min(ze, 2000.0)))


OK_CASES = [n for n, c in PC.hand_cases().items() if c["status"] == 0 and n not in
            ("empty_mask", "out_of_depth", "nan_centre", "inf_depth", "zero_depth", "window_off_frame")]


@pytest.mark.parametrize("name", OK_CASES)
def test_hand_made_frames(D, name):
    c = PC.hand_cases()[name]
    center, status, info = PC.hand_reference(name)
    assert status == D.OK
    window, dlo, dhi = window_of(D, c)
    ref_center, ref_info = PC.brute_palm(c["frame"], window, dlo, dhi)
    assert tuple(info) == ref_info and tuple(center) == ref_center
    if c["point"] is not None:
        assert tuple(info[:2]) == c["point"]
    if c["palm_box"] is not None:
        v_lo, v_hi, u_lo, u_hi = c["palm_box"]
        assert u_lo <= info[0] < u_hi and v_lo <= info[1] < v_hi, (info, c["palm_box"])
        assert info[2] == (PC.PALM // 2) ** 2


def test_known_answers(D):
    center, _, info = PC.hand_reference("disc")
    assert tuple(info[:3]) == (30, 22, 10 * 10 + 1 * 1)        # the nearest pixels outside x^2 + y^2 <= 100 are (+-10, +-1) and (+-1, +-10)
    assert abs(center[0] - 30.0) < 1e-9 and abs(center[1] - 22.0) < 1e-9 and center[2] == 500.0
    assert info[3] == int(PC._disc(PC.SMALL, 22, 30, 10).sum())                                    # the disc of 2.5 radii holds the whole shape
    center, _, info = PC.hand_reference("tie_rectangle")
    # the disc of radius^2 = 25 / 4 * 16 = 100 about (3, 3) of the 8 x 20 rectangle: 14 pixels of row 3 (u <= 13), 13 of each other row (u <= 12)
    assert tuple(info) == (25, 23, 16, 14 + 7 * 13)
    center, _, info = PC.hand_reference("single_pixel")
    assert tuple(info) == (41, 17, 1, 1) and tuple(center) == (41.0, 17.0, 500.0)
    # the ring alone: the window at 1000 mm is 36 x 36 inside the frame; its four middle pixels are 18 from the ring, the first one wins
    from awr_amd import nyu_data as ND
    c = PC.hand_cases()["full_window_inside"]
    u0, u1, v0, v1, _, _ = ND.center2bounds(c["center"], (600, 600, 600), c["paras"])
    assert 0 < u0 and u1 < 64 and 0 < v0 and v1 < 48 and (u1 - u0, v1 - v0) == (36, 36)
    center, _, info = PC.hand_reference("full_window_inside")
    assert tuple(info[:3]) == (u0 + 17, v0 + 17, 18 * 18)
    center, _, info = PC.hand_reference("full_window_clipped")
    assert info[2] == 24 * 24 and info[1] == 23                                                    # 48 rows: rows 23 and 24 are 24 from the ring


@pytest.mark.parametrize("name,status", [("empty_mask", 1), ("out_of_depth", 1), ("nan_centre", 1), ("inf_depth", 1), ("zero_depth", 1),
                                         ("window_off_frame", 1), ("status_empty", 1), ("status_bad_window", 3)])
def test_statuses(D, name, status):
    c = PC.hand_cases()[name]
    center, st, info = PC.hand_reference(name)
    assert st == status and tuple(info) == (-1, -1, 0, 0)
    if c["status"] != 0:
        assert PC.same(center, np.array(c["center"]))          # passed through, whatever it is
    else:
        assert np.isnan(center).all()


def test_procedural_hands_with_a_forearm(D):
    """The issue's bound: on sample_poses(24, 202) with the forearm, the mean centre error of palm_center (seeded by detect) is at most half
    of detect's, and no more frames lie beyond 100 mm."""
    from awr_amd.evaluator import uvd2xyz
    frames, labels, paras, flip = PC.synth_frames(24, 202, PC.FULL, 1.0)
    det_c, det_s, palm_c, palm_s, info = PC.synth_reference(24, 202, PC.FULL, 1.0)
    assert (det_s == 0).all() and (palm_s == 0).all()
    e_det = np.linalg.norm(uvd2xyz(det_c, paras, flip).astype(np.float64) - labels, axis=1)
    e_palm = np.linalg.norm(uvd2xyz(palm_c, paras, flip).astype(np.float64) - labels, axis=1)
    print("detect: mean %.1f max %.1f over100 %d; palm: mean %.1f max %.1f over100 %d"
          % (e_det.mean(), e_det.max(), (e_det > 100).sum(), e_palm.mean(), e_palm.max(), (e_palm > 100).sum()))
    assert e_palm.mean() <= 0.5 * e_det.mean()
    assert (e_palm > 100.0).sum() <= (e_det > 100.0).sum()


def test_small_procedural_hands_have_inner_windows(D):
    """what the GPU tests compare against: at 48 x 64 and 96 x 128 some windows lie inside the frame and some are clipped"""
    for shape, scale in ((PC.SMALL, 0.1), (PC.MID, 0.2)):
        _, _, palm_c, palm_s, info = PC.synth_reference(6, 77, shape, scale)
        assert (palm_s == 0).all() and (info[:, 3] > 0).all()


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """awr_detect_palm checks its arguments on the host before any HIP call, so the refusals are testable without a GPU: every call below
    is invalid, none dereferences the (fake, aligned) pointers"""
    from awr_amd import _lib as L
    p = 0x10000
    good = dict(frames=p, frame_type=0, n_frames=4, fh=48, fw=64, frame=p, B=2, center_in=p, status_in=p, zmin=1.0, zmax=2000.0, cube=p,
                cube_stride=0, fx=58.8, fy=58.7, search=2.0, tau_num=1, tau_den=3, rho2_num=25, rho2_den=4, scratch=p, center_out=p,
                status_out=p, info=None, stream=None)
    for bad, word in ((dict(frames=None), "NULL"), (dict(status_in=None), "NULL"), (dict(scratch=None), "NULL"), (dict(frame_type=1), "uint16"),
                      (dict(B=0), "B ="), (dict(B=65536), "B ="), (dict(n_frames=0), "n_frames"), (dict(fw=16385), "16384"), (dict(fh=0), "16384"),
                      (dict(zmin=3.0, zmax=2.0), "zmin"), (dict(zmin=float("nan")), "zmin"), (dict(cube_stride=1), "cube_stride"),
                      (dict(fx=0.0), "intrinsics"), (dict(search=0.0), "search"), (dict(search=float("inf")), "search"),
                      (dict(search=float("nan")), "search"), (dict(tau_num=0), "tau"), (dict(tau_num=4), "tau"), (dict(rho2_den=0), "rho2"),
                      (dict(rho2_num=3), "rho2"), (dict(scratch=p + 2), "misaligned"), (dict(frames=p + 1), "misaligned")):
        args = dict(good, **bad)
        assert L.lib.awr_detect_palm(*args.values()) == -1, bad
        assert word in L.last_error(), (bad, L.last_error())
    # one int32 word per pixel and frame and a few accumulator words per frame; the largest call does not overflow int64
    assert 3 * 48 * 64 * 4 <= int(L.lib.awr_detect_palm_scratch(3, 48, 64)) <= 3 * (48 * 64 * 4 + 4096)
    assert 65535 * 16384 * 16384 * 4 <= int(L.lib.awr_detect_palm_scratch(65535, 16384, 16384)) <= 65535 * (16384 * 16384 * 4 + 4096)
    for B, fh, fw in ((0, 48, 64), (65536, 48, 64), (1, 0, 64), (1, 48, 16385)):
        assert int(L.lib.awr_detect_palm_scratch(B, fh, fw)) == -1


def test_argument_validation(D):
    f = PC.hand_cases()["disc"]["frame"]
    c = (32.0, 24.0, 500.0)
    for kw in (dict(search=0.0), dict(search=-1.0), dict(search=float("inf")), dict(search=float("nan")), dict(tau=(0, 3)), dict(tau=(4, 3)),
               dict(tau=(-1, -3)), dict(rho2=(4, 25)), dict(rho2=(25, 0)), dict(rho2=(2 ** 31, 4)), dict(depth_range=(2.0, 1.0))):
        with pytest.raises(ValueError):
            D.palm_center(f, c, **kw)
    for kw in (dict(search="2"), dict(tau=(1.0, 3.0)), dict(tau=3), dict(rho2=(25, 4, 1)), dict(tau=(True, 3))):
        with pytest.raises(TypeError):
            D.palm_center(f, c, **kw)
    with pytest.raises(ValueError):
        D.palm_center(f.astype(np.float32), c)
    with pytest.raises(ValueError):
        D.palm_center(np.zeros((1, 16385), np.uint16), c)
    assert D.palm_center(f, c, tau=(1, 1), rho2=(1, 1), search=0.5)[1] in (D.OK, D.EMPTY)
