"""The references of tests/stem_cases.py checked on the CPU, so that tests/test_stem_gpu.py can lean on them: the argmax code of the pooling
kernel against a brute-force scan, the code pattern of an all-tie map, the per-tile sums, and that the tie case of the gradient test really
tells first-maximum routing from last-maximum routing."""
import pytest
import torch
import torch.nn.functional as TF

import stem_cases as SC


def brute_force_codes(x):
    """First maximum in scan order of every 3x3 / stride 2 / pad 1 window of x (C, H, W), as dy * 3 + dx from (2 oy - 1, 2 ox - 1)."""
    C, H, W = x.shape
    out = torch.zeros(C, H // 2, W // 2, dtype=torch.uint8)
    for c in range(C):
        for oy in range(H // 2):
            for ox in range(W // 2):
                best, code = None, -1
                for dy in range(3):
                    for dx in range(3):
                        iy, ix = 2 * oy - 1 + dy, 2 * ox - 1 + dx
                        if 0 <= iy < H and 0 <= ix < W and (best is None or float(x[c, iy, ix]) > best):
                            best, code = float(x[c, iy, ix]), dy * 3 + dx
                out[c, oy, ox] = code
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("H,W", [(16, 16), (8, 12), (12, 6)])
def test_window_code_matches_a_brute_force_scan(H, W, dtype):
    """Few distinct values (ties in most windows, also across the window's rows), a post-ReLU map (ties at 0), a map whose maxima sit on the
    four borders, and a strictly decreasing / increasing ramp (first / last element wins)."""
    g = torch.Generator().manual_seed(H * 100 + W)
    few = torch.randint(0, 3, (3, H, W), generator=g).to(dtype)
    relu = torch.relu(torch.randn(3, H, W, generator=g)).to(dtype)
    border = torch.rand(1, H, W, generator=g).to(dtype)
    border[:, 0, :] += 2
    border[:, -1, :] += 2
    border[:, :, 0] += 2
    border[:, :, -1] += 2
    ramp = torch.arange(H * W, dtype=dtype).view(1, H, W)
    x = torch.cat([few, relu, border, ramp, -ramp])
    _, idx = TF.max_pool2d(x[None], 3, 2, 1, return_indices=True)
    code = SC.window_code(idx[0], H, W)
    assert torch.equal(code, brute_force_codes(x))
    assert bool((code[-2] == 8).all())                                      # increasing ramp: the last element of every window
    assert torch.equal(code[-1], SC.constant_map_codes(H // 2, W // 2))     # decreasing ramp: the first one inside the map


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("value", [0.0, 0.37, -1.5])
def test_constant_map_codes(value, dtype):
    """corner 4, top row 3, left column 1, interior 0 -- from torch's own indices in both precisions"""
    H, W = 16, 32
    x = torch.full((1, 2, H, W), value, dtype=dtype)
    _, idx = TF.max_pool2d(x, 3, 2, 1, return_indices=True)
    code = SC.window_code(idx, H, W)
    want = SC.constant_map_codes(H // 2, W // 2)
    assert want[0, 0] == 4 and bool((want[0, 1:] == 3).all()) and bool((want[1:, 0] == 1).all()) and bool((want[1:, 1:] == 0).all())
    assert bool((code == want).all())


def test_window_code_refuses_an_index_outside_its_window():
    idx = torch.zeros(1, 1, 4, 4, dtype=torch.int64)        # element (0, 0) lies in the first window only
    with pytest.raises(AssertionError):
        SC.window_code(idx, 8, 8)


@pytest.mark.parametrize("B,H,W", SC.SHAPES, ids=[SC.shape_id(s) for s in SC.SHAPES])
def test_tile_sums_add_up_to_the_map(B, H, W):
    g = torch.Generator().manual_seed(H + W)
    x = torch.randn(B, 5, H, W, generator=g, dtype=torch.float64)
    ts = SC.tile_sums(x)
    tiles = SC.tiles_of(H, W)
    assert ts.shape == (B, tiles, 5)
    assert float((ts.sum(1) - x.sum((2, 3))).abs().max()) < 1e-10
    # tile k is row k // (W / 16), column k % (W / 16)
    k = tiles - 1
    ty, tx = divmod(k, W // 16)
    assert float((ts[:, k] - x[:, :, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].sum((2, 3))).abs().max()) < 1e-10
    for t in SC.WG_TILES:
        if tiles % t == 0:
            grouped = SC.group_tiles(ts, t)
            assert grouped.shape == (B * tiles // t, 5)
            assert float((grouped.view(B, -1, 5).sum(1) - x.sum((2, 3))).abs().max()) < 1e-10
            assert float((grouped[0] - ts[0, :t].sum(0)).abs().max()) < 1e-10


def test_shapes_cover_the_tile_counts_and_workgroup_walks():
    assert [SC.tiles_of(H, W) for _, H, W in SC.SHAPES] == SC.TILE_COUNTS

    def walk(tiles, want):
        while tiles % want:
            want //= 2
        return want
    assert {walk(t, 4) for t in SC.TILE_COUNTS} == {1, 2, 4}
    assert {walk(t, 8) for t in SC.TILE_COUNTS} == {1, 2, 4, 8}
    # deterministic slot counts (tiles * B) on both sides of the default 16; workgroups per channel half above it only at WRAP_SHAPE
    det = [B * SC.tiles_of(H, W) for B, H, W in SC.SHAPES]
    assert min(det) < SC.DEFAULT_SLOTS < max(det)
    groups = [B * SC.tiles_of(H, W) // walk(SC.tiles_of(H, W), 4) for B, H, W in SC.SLOT_SHAPES]
    assert max(groups[:-1]) < SC.DEFAULT_SLOTS < groups[-1]


def test_used_prefix():
    raw = torch.zeros(6, 2, 64, dtype=torch.float64)
    assert SC.used_prefix(raw) == 0
    raw[0, 1, 3] = raw[1, 0, 0] = raw[2, 1, 63] = 1.0
    assert SC.used_prefix(raw) == 3
    raw[4, 0, 0] = 1.0
    assert SC.used_prefix(raw) == -1


def test_tie_channels_tell_first_maximum_from_last():
    """gamma = 0, beta > 0: every window of the channel is an exact tie above the ReLU, in float64 and in float32.  torch routes the gradient
    to the first element in scan order; dgamma = sum g * xhat there.  Routing to the LAST element instead moves dgamma of these channels by
    far more than the bound the GPU test asserts (2e-5 of the largest dgamma)."""
    inp = SC.reference(True, 2, 16, 32, "ties")
    r = inp.r64
    H, W = inp.H, inp.W
    tie = torch.arange(64)[(inp.gamma == 0) & (inp.beta > 0)]
    assert len(tie) == 16
    want = SC.constant_map_codes(H // 2, W // 2)
    assert bool((SC.window_code(r.idx, H, W)[:, tie] == want).all())
    xhat = (r.y - r.mean.view(1, -1, 1, 1)) / torch.sqrt(r.var.view(1, -1, 1, 1) + 1e-5)
    oy, ox = torch.arange(H // 2), torch.arange(W // 2)
    first = xhat[:, :, (2 * oy - 1).clamp(min=0)][:, :, :, (2 * ox - 1).clamp(min=0)]
    last = xhat[:, :, 2 * oy + 1][:, :, :, 2 * ox + 1]
    g = inp.gout.double()
    dg_first, dg_last = (g * first).sum((0, 2, 3))[tie], (g * last).sum((0, 2, 3))[tie]
    scale = float(r.dgamma.abs().max())
    assert float((dg_first - r.dgamma[tie]).abs().max()) < 1e-9 * scale
    assert float((dg_last - r.dgamma[tie]).abs().max()) > 1e-2 * scale
    # the masked tie channels (beta < 0) carry no gradient at all
    dead = torch.arange(64)[(inp.gamma == 0) & (inp.beta < 0)]
    assert len(dead) == 16 and float(r.dgamma[dead].abs().max()) == 0.0 and float(r.dbeta[dead].abs().max()) == 0.0


def test_pool_inputs_of_the_exact_test():
    for B, H, W in SC.SHAPES:
        scale, shift = SC.pool_scale_shift(B, H, W)
        assert bool((scale[:16] == 0).all()) and bool((shift[:8] > 0).all()) and bool((shift[8:16] < 0).all())
        assert bool((scale[16:] > 0).any()) and bool((scale[16:] < 0).any()) and bool((scale[16:].abs() >= 0.5).all())
