"""CPU: what keeps tests/test_detect_gpu.py from passing for the wrong reason, checked on the numpy statements alone (awr_amd.detect.detect,
sample_blocks): the window sweep of detect_cases reaches every branch of detect_pass_kernel's row decomposition at every frame-origin offset,
few of its rows are EMPTY, four mutants of the decomposition would each change its centres, the sloping blob moves the centre on every
refinement pass, and the crop-block boundary centres are exact and flip the refusal tests.  Every figure checked is printed (pytest -s)."""
from fractions import Fraction

import numpy as np
import pytest

import detect_cases as DC


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


@pytest.fixture(scope="module")
def reach():
    """the decomposition of every sweep row on the odd-size store: per row a dict with mis and the sets of (align, branch, length) reached"""
    frame, _, _ = DC.sweep(DC.ODD)
    out = []
    for b, (bounds, window) in enumerate(DC.sweep_windows(DC.ODD)):
        mis = DC.origin_offset(DC.ODD, int(frame[b]))
        dc = DC.decompose(mis, DC.ODD[1], window)
        classes, last_group = set(), False
        if dc is not None:
            live = dc["live"]
            classes = set(zip(dc["align"][live].tolist(), dc["branch"][live].tolist(), (dc["hi"] - dc["lo"])[live].tolist()))
            last_group = bool(live[:, -1].any())
        out.append(dict(mis=mis, classes=classes, last_group=last_group, bounds=bounds, window=window, dc=dc))
    return out


def test_stores_hold_every_origin_offset():
    assert DC.ODD[0] * DC.ODD[1] % 8 == 3 and DC.EVEN[0] * DC.EVEN[1] % 8 == 0
    assert [DC.origin_offset(DC.ODD, f) for f in range(8)] == [0, 3, 6, 1, 4, 7, 2, 5]
    assert [DC.origin_offset(DC.EVEN, 5, s) for s in range(8)] == list(range(8))
    for shape in (DC.ODD, DC.EVEN):
        f = DC.dense_frames(shape)
        zeros = (f == 0).mean()
        assert f.shape == (8,) + shape and 0.07 < zeros < 0.13 and f[f > 0].min() >= 650 and f.max() <= 1050
        # every non-zero pixel lies inside the depth range of every sweep window
        _, centers, cubes = DC.sweep(shape)
        assert (centers[:, 2] - cubes[:, 2] / 2 <= f[f > 0].min()).all() and (centers[:, 2] + cubes[:, 2] / 2 >= f.max()).all()


def test_sweep_reaches_every_branch_at_every_offset(reach):
    frame, centers, cubes = DC.sweep(DC.ODD)
    assert len(frame) > 256 and DC.sweep(DC.EVEN)[0].shape == frame.shape
    vec = {(r["mis"], a) for r in reach for a, br, _ in r["classes"] if br == DC.VEC}
    assert vec == {(m, a) for m in range(8) for a in range(8)}
    classes = {(r["mis"], a, br) for r in reach for a, br, _ in r["classes"]}
    # a row that starts on a group boundary has no head: 8 of the 192 classes do not exist
    assert classes == {(m, a, br) for m in range(8) for a in range(8) for br in (DC.VEC, DC.HEAD, DC.TAIL) if not (a == 0 and br == DC.HEAD)}
    for br in (DC.HEAD, DC.TAIL):
        lengths = {(r["mis"], n) for r in reach for _, b2, n in r["classes"] if b2 == br}
        assert lengths == {(m, n) for m in range(8) for n in range(1, 8)}, br
    print("\nsweep: %d rows; 16-byte branch at %d of 64 (offset, alignment) pairs; %d of 192 (offset, alignment, branch) classes; head and tail "
          "loops at lengths 1 ... 7 at all 8 offsets" % (len(frame), len(vec), len(classes)))


def test_sweep_holds_every_clipping_class(reach):
    fh, fw = DC.ODD
    for shape in (DC.ODD, DC.EVEN):
        wins = DC.sweep_windows(shape)
        live = [(b, w) for b, w in wins if w[0] < w[1] and w[2] < w[3]]
        sides = {DC.clipped_sides(b, shape) for b, _ in live}
        want = [{"left"}, {"right"}, {"top"}, {"bottom"}, {"left", "right"}, {"top", "bottom"}, {"left", "top"}, {"right", "top"}, {"left", "bottom"},
                {"right", "bottom"}, {"left", "right", "top"}, {"left", "right", "bottom"}, {"left", "top", "bottom"}, {"right", "top", "bottom"},
                {"left", "right", "top", "bottom"}, set()]
        assert all(frozenset(s) in sides for s in want), [s for s in want if frozenset(s) not in sides]
        widths = {w[1] - w[0] for _, w in live}
        assert set(range(1, 9)) <= widths and shape[1] in widths
        # the narrow windows are unclipped ones: 1 ... 7 pixels by their cube, not by the frame's edge
        assert set(range(1, 8)) <= {b[1] - b[0] for b, w in live if not DC.clipped_sides(b, shape)}
    # a window that is, in one of its rows, exactly one aligned group and nothing else -- at every origin offset
    one_group = set()
    for r in reach:
        if r["dc"] is not None and r["window"][1] - r["window"][0] == 8:
            live, vec = r["dc"]["live"], r["dc"]["branch"] == DC.VEC
            if ((live.sum(1) == 1) & (live & vec).any(1)).any():
                one_group.add(r["mis"])
    assert one_group == set(range(8))
    # ... and on the even store whatever its shift: rows alternate between two alignments, the eight starts cover the rest
    frame = DC.sweep(DC.EVEN)[0]
    for shift in range(8):
        hit = False
        for b, (_, w) in enumerate(DC.sweep_windows(DC.EVEN)):
            if w[1] - w[0] == 8 and w[2] < w[3]:
                dc = DC.decompose(DC.origin_offset(DC.EVEN, int(frame[b]), shift), DC.EVEN[1], w)
                hit = hit or bool(((dc["live"].sum(1) == 1) & (dc["live"] & (dc["branch"] == DC.VEC)).any(1)).any())
        assert hit, shift


def test_few_rows_are_empty_and_each_has_an_empty_window():
    for shape in (DC.ODD, DC.EVEN):
        centers, status = DC.sweep_reference(shape)
        wins = DC.sweep_windows(shape)
        empty = np.flatnonzero(status == DC.EMPTY)
        assert set(status.tolist()) == {DC.OK, DC.EMPTY} and 0 < len(empty) <= 0.05 * len(status)
        assert np.isnan(centers[empty]).all() and not np.isnan(centers[status == DC.OK]).any()
        assert all(wins[b][1][0] >= wins[b][1][1] or wins[b][1][2] >= wins[b][1][3] for b in empty)
        print("\n%d x %d: %d of %d sweep rows are EMPTY (%.1f %%), each with an empty clipped window" % (shape + (len(empty), len(status), 100.0 * len(empty) / len(status))))


def test_the_model_equals_the_statement_and_every_mutant_bites(reach):
    """Mutants 1 and 2 drop `- mis`, which is nothing where mis == 0: their rows are those of frames with mis != 0 (that reach a 16-byte load,
    for mutant 1).  Mutant 3 loses a row's last group: its rows have a window row that needs all gpr groups.  Mutant 4: rows with a tail."""
    ref_c, ref_s = DC.sweep_reference(DC.ODD)
    got_c, got_s = DC.model_sweep(DC.ODD)
    assert same(got_c, ref_c) and np.array_equal(got_s, ref_s)
    for shift in (0, 5):
        c, s = DC.model_sweep(DC.EVEN, shift=shift)
        assert same(c, DC.sweep_reference(DC.EVEN)[0]) and np.array_equal(s, DC.sweep_reference(DC.EVEN)[1])
    has = lambda r, br: any(b2 == br for _, b2, _ in r["classes"])
    rows = {1: [b for b, r in enumerate(reach) if r["mis"] and has(r, DC.VEC)], 2: [b for b, r in enumerate(reach) if r["mis"] and r["classes"]],
            3: [b for b, r in enumerate(reach) if r["last_group"]], 4: [b for b, r in enumerate(reach) if has(r, DC.TAIL)]}
    for m in (1, 2, 3, 4):
        c, _ = DC.model_sweep(DC.ODD, mutant=m)
        differs = np.array([not same(c[b], ref_c[b]) for b in rows[m]])
        outside = [b for b in range(len(ref_c)) if b not in set(rows[m]) and not same(c[b], ref_c[b])]
        print("\nmutant %d (%s): %d of the %d rows that reach it differ (%.1f %%)" % (m, DC.MUTANTS[m], differs.sum(), len(rows[m]), 100.0 * differs.mean()))
        assert len(rows[m]) >= 50 and differs.mean() >= 0.10 and not outside, (m, outside)


def test_every_refinement_pass_moves_the_centre(D):
    ref = DC.slope_reference()
    assert len(ref) == D.MAX_ITERS + 1 == 9 and all(s == DC.OK for _, s in ref) and ref[0][0] == DC.SLOPE_START
    distinct = [all(ref[i][0] != ref[j][0] for j in range(i)) for i in range(9)]
    print("\nsloping blob: centres after 0 ... 8 passes:", [tuple(round(x, 3) for x in c) for c, _ in ref])
    assert all(distinct)
    # the blob's own pixels alone: the far plane is outside every window's depth range
    assert all(c[2] < 1200 for c, _ in ref)


def test_depth_cases_reach_the_edges_of_depth_bounds(D):
    f = DC.depth_frame()
    assert {1, 450, 451, 1499, 1500, DC.PIXEL, 65535} <= set(np.unique(f).tolist()) and (f == DC.PIXEL).sum() == 12 and (f == 0).any()
    cases = DC.depth_cases()
    assert len(set(cases)) == len(cases) == 18
    for seed, rng, slab in cases:
        c, s = DC.depth_reference(seed, rng, slab, 0)
        if rng == (0.25, 0.75):
            assert (s == DC.EMPTY).all() and np.isnan(c).all()
        else:
            assert (s == DC.OK).all()
    # a fractional bound admits neither 450 nor 1500; a bound equal to a pixel value admits that pixel; zmin == zmax is the patch alone
    n = lambda lo, hi: D.center_of_mass(f, None, lo, hi)[1]
    assert n(450.5, 1499.5) == n(451.0, 1499.0) == n(450.0, 1500.0) - 2 and n(DC.PIXEL, DC.PIXEL) == 12
    assert DC.depth_reference("range", (float(DC.PIXEL), float(DC.PIXEL)), 0.0, 0)[0][0].tolist() == [31.5, 13.0, float(DC.PIXEL)]
    assert DC.depth_reference("nearest", (1.0, 65535.0), 0.0, 0)[0][0].tolist() == [40.0, 30.0, 1.0]
    # the cut slabs: dmin + slab > zmax, and the seed is then the "range" seed
    for rng, slab in (((450.5, 1499.5), 2000.0), ((1.0, 65535.0), 70000.0)):
        dmin = float(f[(f >= rng[0]) & (f <= rng[1]) & (f != 0)].min())
        assert dmin + slab > rng[1] and same(DC.depth_reference("nearest", rng, slab, 0)[0], DC.depth_reference("range", rng, 0.0, 0)[0])
    assert all(cube[2] / 2.0 != int(cube[2] / 2.0) for cube in DC.DEPTH_CUBES)
    # the refinement's per-row cubes matter: the rows of a case differ
    c = DC.depth_reference("nearest", (450.5, 1499.5), 119.99, 2)[0]
    assert len({tuple(r) for r in c.tolist()}) == len(DC.DEPTH_CUBES)


def test_mixed_batch_is_mixed():
    frame, cubes = DC.mixed_batch()
    c, s = DC.mixed_reference()
    bad = (frame < 0) | (frame >= DC.N_FRAMES)
    assert len(frame) >= 300 and bad[:256].sum() == 3 and bad[256:].sum() == 3 and {-1, DC.N_FRAMES, DC.N_FRAMES + 5} == set(frame[bad].tolist())
    assert (s[bad] == DC.BAD_FRAME).all() and np.isnan(c[bad]).all() and (s[~bad] == DC.OK).all()
    assert len(np.unique(frame[~bad])) == DC.N_FRAMES and len({tuple(r) for r in c[~bad].tolist()}) > 100


def test_boundary_centres_are_exact_and_flip_the_refusal(D):
    import awr_amd  # noqa: F401
    from awr_amd import nyu_data as ND
    fh, fw = DC.ODD
    assert Fraction(DC.EXACT_CUBE[0]) / 2 / Fraction(DC.EXACT_D) * Fraction(DC.PARAS[0]) == Fraction(DC.EXACT_HU) == Fraction((DC.EXACT_CUBE[0] / 2.0) / DC.EXACT_D * DC.PARAS[0])
    assert Fraction(DC.EXACT_CUBE[1]) / 2 / Fraction(DC.EXACT_D) * Fraction(DC.PARAS[1]) == Fraction(DC.EXACT_HV) == Fraction((DC.EXACT_CUBE[1] / 2.0) / DC.EXACT_D * DC.PARAS[1])
    centers, cubes, frame, status_in, first = DC.sample_rows()
    pairs = DC.boundary_pairs()
    for k, (name, which, bad_value, bad, good_value, good) in enumerate(pairs):
        assert same(centers[first + 2 * k], bad) and same(centers[first + 2 * k + 1], good) and same(cubes[first + 2 * k], DC.EXACT_CUBE)
        for c, value in ((bad, bad_value), (good, good_value)):
            exact = DC.exact_bounds(c)
            # the double arithmetic of center2bounds is exact here: every intermediate equals the rational one, and the bound is the integer
            u, v, d = c
            hu, hv = (DC.EXACT_CUBE[0] / 2.0) / d * DC.PARAS[0], (DC.EXACT_CUBE[1] / 2.0) / d * DC.PARAS[1]
            doubles = dict(us=u - hu + 0.5, ue=u + hu + 0.5, vs=v - hv + 0.5, ve=v + hv + 0.5)
            assert all(Fraction(doubles[k2]) == exact[k2] for k2 in doubles) and exact[which] == value, (name, c)
            b = ND.center2bounds(c, DC.EXACT_CUBE, DC.PARAS)
            assert dict(us=b[0], ue=b[1], vs=b[2], ve=b[3])[which] == value
        st = D.sample_blocks(np.array([bad, good]), DC.EXACT_CUBE, DC.DSIZE, DC.PARAS, DC.FLIP, DC.ODD)[4]
        assert st.tolist() == [DC.BAD_WINDOW, DC.OK], name
    print("\n%d boundary pairs: every bound an exact integer in float64, sample_blocks refuses one centre of each pair and accepts the other" % len(pairs))


def test_sample_rows_cover_the_refusals(D):
    centers, cubes, frame, status_in, first = DC.sample_rows()
    blocks, M, cxyz, cube32, status = DC.sample_reference()
    B = len(centers)
    assert B > 256 and frame.shape == status_in.shape == (B,)
    bad = (frame < 0) | (frame >= DC.N_FRAMES)
    assert bad[:256].sum() >= 3 and bad[256:].sum() >= 2 and (status[bad] == DC.BAD_FRAME).all()
    assert sum(blk is None for blk in blocks) == np.isnan(M[:, 0, 0]).sum() > 40 and sum(blk is not None for blk in blocks) > 100
    assert all((blocks[b] is None) == (status[b] in (DC.BAD_WINDOW, DC.BAD_FRAME)) for b in range(B) if status_in[b] == 0)
    # incoming codes sit on windows that hold and on windows refused, and are kept
    kept = np.flatnonzero((status_in != 0) & ~bad)
    assert (status[kept] == status_in[kept]).all() and any(blocks[b] is None for b in kept) and any(blocks[b] is not None for b in kept)
    # windows larger than the frame, windows of one pixel and of none, and crops that resize to nothing in one direction only
    ok = [blk for blk in blocks if blk is not None]
    assert any(blk.cw > DC.ODD[1] and blk.ch > DC.ODD[0] for blk in ok) and any(blk.cw == 1 for blk in ok) and any(blk.ch == 1 for blk in ok)
    assert any(blk.ustart < 0 for blk in ok) and any(blk.ustart + blk.cw > DC.ODD[1] for blk in ok) and any(blk.vstart < 0 for blk in ok)
    assert any(blk.vstart + blk.ch > DC.ODD[0] for blk in ok) and any(blk.rw == 1 for blk in ok) and any(blk.rh == 1 for blk in ok)
    refused_resize = 0
    for c, cube in zip(centers, cubes):
        if np.isfinite(c).all() and np.isfinite(cube).all() and c[2] > 0:
            import awr_amd.nyu_data as ND
            b = ND.center2bounds(c, cube, DC.PARAS)
            cw, ch = b[1] - b[0], b[3] - b[2]
            if cw > 0 and ch > 0 and b[1] > 0 and b[3] > 0 and b[0] < DC.ODD[1] and b[2] < DC.ODD[0]:
                scale = min(DC.DSIZE / cw, DC.DSIZE / ch)
                refused_resize += int(cw * scale) == 0 or int(ch * scale) == 0
    assert refused_resize >= 2
    assert np.isnan(centers).any() and np.isinf(centers).any() and (centers[:, 2] == 0).any()
