"""CPU: the shape table of the Winograd weight-gradient tests (tests/wino_wgrad_cases.py) really has the coverage it is chosen for.  The split
count of a launch is host arithmetic (awr_wino_wgrad_scratch runs without a GPU); from it launch_shape() restates the kernels' ranges, and
every class of loop depth, range evenness, reduce-group size and grid size the GPU module relies on is asserted here.  If the host rule
changes and a class disappears, re-choose the table: the class is not to be dropped."""
import os

import pytest

import wino_wgrad_cases as WC


@pytest.fixture(scope="module")
def lib():
    import awr_amd  # noqa: F401
    from awr_amd import build
    if not os.path.exists(build.LIB):
        build.build_lib(verbose=False)
    from awr_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def launches(lib):
    return {s: WC.launch_shape(lib.lib, *s) for s in WC.SHAPES}


def test_table_is_well_formed(launches):
    assert len(set(WC.SHAPES)) == len(WC.SHAPES) and set(WC.ELIGIBLE) <= set(WC.SHAPES)
    for (B, H, W, C, N), ls in launches.items():
        assert C % 64 == 0 and N % 64 == 0 and H >= 8 and W >= 8 and H & (H - 1) == 0 and W & (W - 1) == 0
        assert ls["scratch"] * 4 <= 68e6 and B * H * W * max(C, N) <= 2 * 2 ** 20      # a launch stays small: 68 MB of copies, 2 M floats
        assert sum(ls["groups"]) == ls["S"] and len(ls["nst"]) == ls["S"] and all(n % 2 == 0 for n in ls["nst"])


def test_launch_shape_of_every_row(launches):
    """the properties each row was chosen for, as the host rule gives them today"""
    want = {
        (1, 8, 8, 64, 64): (1, 1, {2}, (0, 0, 0, 1)),
        (2, 8, 8, 256, 512): (2, 64, {2}, (0, 1, 0, 1)),
        (2, 16, 16, 64, 192): (8, 24, {2}, (2, 2, 2, 2)),
        (3, 32, 32, 192, 128): (43, 258, {2, 4}, (10, 11, 11, 11)),
        (5, 64, 64, 64, 64): (256, 256, {2, 4}, (64, 64, 64, 64)),
        (6, 8, 8, 512, 512): (4, 256, {2, 4}, (1, 1, 1, 1)),
        (5, 16, 32, 256, 256): (16, 256, {4, 6}, (4, 4, 4, 4)),
        (5, 8, 16, 512, 512): (4, 256, {4, 6}, (1, 1, 1, 1)),
        (3, 32, 32, 256, 256): (16, 256, {6}, (4, 4, 4, 4)),
        (4, 16, 16, 512, 512): (4, 256, {8}, (1, 1, 1, 1)),
        (16, 32, 32, 128, 128): (64, 256, {8}, (16, 16, 16, 16)),
        (9, 16, 16, 512, 512): (4, 256, {18}, (1, 1, 1, 1)),
    }
    assert set(want) == set(WC.SHAPES)
    for s, (S, grid, stages, groups) in want.items():
        ls = launches[s]
        assert (ls["S"], ls["grid"], set(ls["stages"]), ls["groups"]) == (S, grid, stages, groups), (s, ls)


def test_every_loop_depth_class_is_in_the_table(launches):
    sets = [set(ls["stages"]) for ls in launches.values()]
    assert any(s == {2} for s in sets)                                  # one loop iteration, every request past the first pair clamped
    assert any(len(s) > 1 and 2 in s for s in sets)                     # ranges of different length, some of one iteration
    assert any(len(s) > 1 and 2 not in s for s in sets)                 # ranges of different length, every split in the steady state
    assert any(s == {6} for s in sets)                                  # three iterations
    assert any(min(s) >= 8 for s in sets)                               # what plans accept outside test mode
    assert any(min(s) >= 16 for s in sets)


def test_every_reduce_and_grid_class_is_in_the_table(launches):
    groups = [g for ls in launches.values() for g in ls["groups"]]
    assert any(ls["S"] == 1 for ls in launches.values())
    assert any(9 <= g <= 15 for g in groups)                            # the 8-wide unrolled part and the tail in one group
    assert any(g == 0 for g in groups)
    assert any(g >= 16 and g % 8 == 0 for g in groups)                  # the unrolled part more than once, no tail
    assert any(ls["grid"] % 8 != 0 for ls in launches.values())         # the workgroup renumbering's remainder branch
    assert any(ls["grid"] < 8 for ls in launches.values())
    assert any(W == 8 for (_, _, W, _, _) in launches)                  # one 2 x 4 patch block per image row (lg_bpr = 0)
    assert any(C > N for (_, _, _, C, N) in launches) and any(N > C for (_, _, _, C, N) in launches)


def test_eligible_rows_are_the_ones_plans_run(lib):
    """under the default Winograd code plans take the kernel at 8 or more stages per split ($AWR_WINOGRAD changes the code the library
    answers for: nothing is asserted then)"""
    if "AWR_WINOGRAD" in os.environ:
        return
    was = lib.lib.awr_get_conv_winograd()
    try:
        assert lib.lib.awr_set_conv_winograd(0) == 0
        for s in WC.SHAPES:
            assert lib.lib.awr_wino_wgrad_eligible(*s) == (1 if s in WC.ELIGIBLE else 0), s
    finally:
        lib.lib.awr_set_conv_winograd(was)


def test_exact_bound_holds_for_every_row():
    for B, H, W, _, _ in WC.SHAPES:
        assert WC.exact_bound_holds(B, H, W), (B, H, W)
    assert max(B * H * W // 4 for B, H, W, _, _ in WC.SHAPES) == 5120
    assert not WC.exact_bound_holds(6, 64, 64)                          # (the bound is a real one: the next batch size up misses it)


def test_exact_inputs_are_small_integers_and_the_reference_is_cached():
    s, form = (1, 8, 8, 64, 64), (True, True)
    x, dy, sc, sh = WC.inputs(s, form, "exact")
    assert set(x.unique().tolist()) == {-1.0, 0.0, 1.0} and set(dy.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert set(sc.unique().tolist()) == {1.0, 2.0} and set(sh.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert WC.inputs(s, (False, False), "exact")[2] is None
    gw, gb = WC.reference(s, form, "exact")
    assert gw.shape == (64, 64, 3, 3) and gb.shape == (64,) and gw.dtype == gb.dtype == WC.torch.float64
    assert WC.torch.equal(gw * 4, (gw * 4).round()) and gw.abs().max() > 0
    before = len(WC._REF)
    gw2, _ = WC.reference(s, form, "exact")
    assert len(WC._REF) == before and WC.torch.equal(gw, gw2)
