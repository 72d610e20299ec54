"""CPU: the tables of tests/head_cases.py cover every launch class of the head kernels, their inputs hold what the GPU tests rely on, the
references are finite and leave room under the fixed bars, and the references would notice a depth sample or a joint slot read one off."""
import pytest
import torch

import awr_oracle as O
import confidence_ref as R
import head_cases as HC

SMALL = [c for c in HC.NHWC_CASES if c[0] * c[1] * c[2] * c[2] <= 3 * 56 * 40 * 40]      # the float64 checks skip the three largest maps
IDS = [HC.case_id(c) for c in HC.NHWC_CASES]


def test_the_nhwc_table_covers_every_launch_class():
    got = set().union(*(HC.launch_classes(*c) for c in HC.NHWC_CASES))
    assert HC.ALL_CLASSES <= got, sorted(HC.ALL_CLASSES - got)
    assert set(HC.PEAKED_CASES) <= set(HC.NHWC_CASES) and {HC.nhwc_launch(*c)["JS"] for c in HC.PEAKED_CASES} == {16, 32, 64}


def test_dropping_a_case_is_noticed():
    """the coverage assertion has teeth: without the ragged case, the widest map or the 256-chunk case a class is missing"""
    for drop in [(256, 14, 24, 48, 64), (3, 56, 24, 48, 224), (3, 14, 128, 128, 64), (3, 1, 8, 8, 32)]:
        assert drop in HC.NHWC_CASES
        rest = set().union(*(HC.launch_classes(*c) for c in HC.NHWC_CASES if c != drop))
        assert not HC.ALL_CLASSES <= rest, drop


def test_the_nchw_table_covers_its_classes():
    got = set().union(*(HC.nchw_classes(*c) for c in HC.NCHW_CASES))
    assert HC.ALL_NCHW_CLASSES <= got, sorted(HC.ALL_NCHW_CLASSES - got)


def test_launch_restatement_on_known_shapes():
    la = HC.nhwc_launch(256, 14, 24, 48, 64)
    assert (la["JS"], la["POW2"], la["rs"], la["tiles"], la["tiles_per_wg"], la["chunks"], la["ragged"], la["last_tiles"]) == (16, False, 2, 9, 2, 5, True, 1)
    la = HC.nhwc_launch(64, 14, 64, 128, 64)          # the benchmarked step: 64 tiles, 4 per workgroup
    assert (la["tiles"], la["tiles_per_wg"], la["chunks"], la["ragged"], la["NL"], la["idle_lanes"]) == (64, 4, 16, False, 4, 32)
    la = HC.nhwc_launch(3, 56, 24, 48, 224)
    assert la["lds_bytes"] == 58624 < 65536 and la["JS"] == 64 and la["NL"] == 14 and la["NLMAX"] == 16
    assert HC.nhwc_launch(3, 14, 128, 128, 64)["chunks"] == 256
    for c, want in zip(HC.ENV_CASES, [(8, 2, 1), (16, 2, 9), (4, 1, 4)]):          # AWR_NHWC_WGS=1
        la = HC.nhwc_launch(*c, want_wgs=1)
        assert (la["tiles_per_wg"], la["chunks"], la["last_tiles"]) == want
    for bad in [(3, 57, 8, 8, 256), (3, 14, 8, 8, 96), (3, 14, 12, 12, 64), (3, 14, 8, 8, 48)]:
        with pytest.raises(AssertionError):
            HC.nhwc_launch(*bad)


@pytest.mark.parametrize("case", HC.NHWC_CASES + HC.ENV_CASES, ids=HC.case_id)
def test_partials_fit_the_documented_scratch(case):
    B, J, F, H, Cp = case
    for wgs in (HC.WANT_WGS, 1):
        la = HC.nhwc_launch(*case, want_wgs=wgs)
        assert la["partials"] <= HC.scratch_floats(B, J, F) and la["lds_bytes"] < 65536 and la["NL"] <= la["NLMAX"]
        assert la["NL"] * 256 * 4 == HC.TPX * Cp           # the float4 loads of a tile cover it exactly: no thread reads past the tile


def _all_cases():
    return [c[:4] for c in HC.NHWC_CASES] + HC.NCHW_CASES + [c[:4] for c in HC.ENV_CASES]


@pytest.mark.parametrize("case", sorted(set(_all_cases())), ids=HC.case_id)
def test_inputs_hold_what_the_gpu_tests_rely_on(case):
    B, J, F, H = case
    c = HC.inputs(*case)
    d = c["img"][:, 0, ::H // F, ::H // F]
    bg = (d >= 0.99).flatten(1).float().mean(1)
    assert float(bg[0]) == 1.0 and float(bg[1]) == 0.0 and bool(((bg[2:] > 0) & (bg[2:] < 1)).all())
    assert float(c["off"].abs().max()) <= 0.6 + 1e-7 and bool((c["off"][:, 3 * J:].abs() * 30 > 15).any())
    for ks in HC.KSS:
        gt = O.joint2offset(c["jt_gt"], c["img"], ks, F)
        ieee = torch.from_numpy(O.joint2offset_ieee(c["jt_gt"], c["img"], ks, F))
        assert torch.equal(gt != 0, ieee != 0)
        assert float((HC.gt_map64(c["jt_gt"], c["img"], ks, F) - ieee).abs().max()) <= 1e-5      # the same map (the offset of the joint 0.01 from a
        #                                                    pixel is a difference of coordinates near 1: 6e-8 absolute, 6e-6 of the unit vector)
        hit = (gt[:, 3 * J:] != 0).flatten(2).any(-1)
        assert bool(hit.any()) and bool((~hit).any()) and bool(hit[B - 1, J - 1])
        assert not bool(hit[:, 0].any()) or J == 1
        assert not bool(hit[0].any())                      # no hand pixel, no GT map
        z = (c["off"] - gt).abs()
        assert bool((z < HC.DELTA).any()) and bool((z > HC.DELTA).any())


@pytest.mark.parametrize("case", HC.NHWC_CASES, ids=IDS)
def test_references_are_finite(case):
    for ks in HC.KSS:
        for cw in (0.0, 1.0):
            r = HC.loss_refs(*case[:4], ks, cw)
            assert bool(torch.isfinite(r["jt"]).all()) and bool(torch.isfinite(r["grad"]).all()) and r["lc"] == r["lc"] and r["ld"] > 0


@pytest.mark.parametrize("case", SMALL, ids=HC.case_id)
def test_room_under_the_fixed_bars(case):
    """on the standard inputs the fp32 oracle sits within half of each fixed bar of float64 (joints: 3e-6; head gradient: 3e-6 max|g|)"""
    for ks in HC.KSS:
        jt, g = HC.head_refs(*case[:4], ks)
        jt64, g64 = HC.head_refs(*case[:4], ks, f64=True)
        dj, dg, gmax = float((jt - jt64).abs().max()), float((g - g64).abs().max()), float(g64.abs().max())
        print("%s ks %.1f: joints %.2e  head gradient %.2e max|g| (max|g| %.2e)" % (HC.case_id(case), ks, dj, dg / gmax, gmax))
        assert dj <= 1.5e-6 and dg <= 1.5e-6 * gmax
        assert float((R.joints(HC.inputs(*case[:4])["off"], HC.inputs(*case[:4])["img"], ks) - jt64).abs().max()) <= 1e-12      # two statements, one formula


@pytest.mark.parametrize("case", HC.PEAKED_CASES, ids=HC.case_id)
def test_peaked_inputs_are_peaked_and_finite(case):
    B, J, F, H, Cp = case
    c = HC.inputs(B, J, F, H, True)
    assert 80 < float(c["off"][:, 3 * J:].abs().max()) * 30 <= 90 and torch.equal(c["off"][:, :3 * J], HC.inputs(B, J, F, H)["off"][:, :3 * J])
    r, r64 = HC.loss_refs(B, J, F, H, 0.4, 1.0, 1.0, True), HC.loss_refs64(B, J, F, H, 0.4, 1.0, 1.0, True)
    assert bool(torch.isfinite(r["jt"]).all()) and bool(torch.isfinite(r["grad"]).all())
    assert float((r["gt"] - r64["gt"]).abs().max()) <= 1e-5    # the float64 GT map takes the float32 mask decisions: a flipped pixel would differ by O(1)
    print("%s peaked: fp32 oracle to float64: joints %.2e, gradient %.2e max|g|" % (HC.case_id(case), float((r["jt"] - r64["jt"]).abs().max()),
                                                                               float((r["grad"] - r64["grad"]).abs().max() / r64["grad"].abs().max())))


@pytest.mark.parametrize("case", [c for c in HC.NHWC_CASES + HC.ENV_CASES if c[0] <= 3], ids=HC.case_id)
def test_the_references_would_notice(case):
    """A depth sample taken one source pixel off (rs > 1), or a joint reading its neighbour's channels, moves the reference joints by more
    than 100 times the joint bar: the GPU comparison cannot pass by luck."""
    B, J, F, H, Cp = case
    c = HC.inputs(B, J, F, H)
    for ks in HC.KSS:
        ref = HC.loss_refs(B, J, F, H, ks, 0.0)["jt"]
        if H // F > 1:
            for dim in (-1, -2):
                off_by_one = O.offset2joint_softmax(c["off"], torch.roll(c["img"], -1, dim), ks)
                assert float((off_by_one - ref).abs().max()) > 3e-4
        if J > 1:
            perm = torch.cat([(3 * torch.arange(J).roll(-1)).repeat_interleave(3) + torch.arange(3).repeat(J), 3 * J + torch.arange(J)])
            assert float((O.offset2joint_softmax(c["off"][:, perm], c["img"], ks) - ref).abs().max()) > 3e-4        # vector channels of joint j + 1
            perm = torch.cat([torch.arange(3 * J), 3 * J + torch.arange(J).roll(-1)])
            assert float((O.offset2joint_softmax(c["off"][:, perm], c["img"], ks) - ref).abs().max()) > 3e-4        # heat channel of joint j + 1
