"""CPU: awr_amd.track.assign_step, the numpy statement of awr_hands_assign -- against an independent
itertools.permutations restatement over random chains, and rule by rule on hand-written frames whose gate edges are exact integers; the
validation of the identity option; awr_hands_assign's argument checks, which come before any launch."""
import itertools
import math

import numpy as np
import pytest

import assign_cases as AC

OK, EMPTY = AC.OK, AC.EMPTY


@pytest.fixture(scope="module")
def T():
    import awr_amd  # noqa: F401
    from awr_amd import track
    return track


def step(T, state, rows, K=None, trk=None, cfg=AC.CFG, **kw):
    K = state["ids"].shape[0] if K is None else K
    c, s = AC.frame(K, rows)
    t, ts = (None, None) if trk is None else AC.frame(K, trk)
    return AC.run(T, state, c, s, t, ts, cfg, **kw)


def col(a):
    return a[:, 0].tolist()


@pytest.mark.parametrize("tracked", (False, True), ids=("detector", "tracked"))
@pytest.mark.parametrize("K", (1, 2, 3, 4))
def test_random_chains_equal_the_independent_solver(T, K, tracked):
    B = 6
    state, ref_state = AC.new_state(T, K, B), AC.new_state(T, K, B)
    seen = set()
    for t, (cand, cstat, trk, tstat) in enumerate(AC.chain(K, B, T=40, seed=3, tracked=tracked)):
        got = AC.run(T, state, cand, cstat, trk, tstat)
        want = AC.reference_step(ref_state, cand, cstat, trk, tstat)
        for n in AC.NAMES:
            assert AC.same(got[n], want[n]), (t, n, got[n], want[n])
        for n in AC.STATE:
            assert AC.same(state[n], ref_state[n]), (t, n, state[n], ref_state[n])
        seen |= set(np.unique(got["code"]).tolist())
        # identities are unique within a frame, and a slot is free exactly where its last centre is NaN
        for b in range(B):
            live = state["ids"][:, b][state["ids"][:, b] > 0]
            assert len(set(live.tolist())) == len(live) and (live < state["next_id"][b]).all()
        assert np.array_equal(state["ids"] == 0, np.isnan(state["last_uvd"]).all(-1))
    # what the comparison covered (a slot with a tracker is hardly ever without it and without a candidate three steps on end: ID_LOST is
    # asked of the chains without one; test_max_miss_edge has it rule by rule)
    want = {T.BORN, T.MATCHED, T.COASTING} | ({T.TRACKED} if tracked else {T.ID_LOST, T.FREE}) | ({T.FREE, T.MERGED} if K > 1 and tracked else set())
    assert seen >= want, (seen, want)


@pytest.mark.parametrize("K", (1, 2, 3, 4))
def test_conservation_without_a_tracker(T, K):
    """every usable candidate is reported exactly once, bit for bit, and none is dropped: K slots always have room for K candidates"""
    B = 5
    state = AC.new_state(T, K, B)
    for cand, cstat, _, _ in AC.chain(K, B, T=30, seed=7):
        got = AC.run(T, state, cand, cstat)
        assert not got["dropped"].any()
        for b in range(B):
            usable = sorted(tuple(cand[j, b]) for j in range(K) if cstat[j, b] == OK and np.isfinite(cand[j, b]).all())
            out = sorted(tuple(got["centers"][i, b]) for i in range(K) if got["status"][i, b] == OK)
            assert usable == out
            src = got["source"][:, b]
            assert sorted(src[src >= 0].tolist()) == [j for j in range(K) if cstat[j, b] == OK and np.isfinite(cand[j, b]).all()]
        assert np.array_equal(np.isnan(got["centers"]).all(-1), got["status"] == EMPTY) and set(np.unique(got["status"])) <= {OK, EMPTY}


def test_births_fill_slots_in_candidate_order_and_swapped_candidates_keep_their_ids(T):
    state = AC.new_state(T, 2, 1)
    a, b = (10, 10, 2), (30, 10, 2)
    got = step(T, state, [a, b])
    assert col(got["code"]) == [T.BORN] * 2 and col(got["reset"]) == [1, 1] and col(got["source"]) == [0, 1] and col(state["ids"]) == [1, 2]
    # the same hands, one unit on, in the OTHER candidate order: slot 0 is still hand a
    a2, b2 = (11, 10, 2), (29, 10, 2)
    got = step(T, state, [b2, a2])
    assert col(got["code"]) == [T.MATCHED] * 2 and col(got["source"]) == [1, 0] and col(got["reset"]) == [0, 0] and col(state["ids"]) == [1, 2]
    assert got["centers"][:, 0].tolist() == [list(map(float, a2)), list(map(float, b2))] and state["next_id"].tolist() == [3]
    assert AC.same(state["last_uvd"], got["centers"])


def test_gate_edge_is_inclusive(T):
    """gate 6: a move of exactly 6 mm matches; one unit more coasts and the candidate is born into the free slot"""
    for move, matched in ((6, True), (7, False)):
        state = AC.new_state(T, 2, 1)
        step(T, state, [(10, 10, 1)])
        got = step(T, state, [(10 + move, 10, 1)])
        if matched:
            assert col(got["code"]) == [T.MATCHED, T.FREE] and col(state["ids"]) == [1, 0] and col(state["miss"]) == [0, 0]
        else:
            assert col(got["code"]) == [T.COASTING, T.BORN] and col(state["ids"]) == [1, 2] and col(state["miss"]) == [1, 0]
            assert col(got["status"]) == [EMPTY, OK] and np.isnan(got["centers"][0]).all() and state["last_uvd"][0, 0].tolist() == [10.0, 10.0, 1.0]
    # on two axes: (3, 4, 1) -> (0, 0, 1) is exactly 5 mm; and in depth, where xyz = (u d, v d, d): (0, 0, 1) -> (0, 0, 6) is 5 mm, (0, 0, 7) is not
    state = AC.new_state(T, 2, 1)
    step(T, state, [(3, 4, 1)], cfg=dict(gate_mm=5.0))
    assert col(step(T, state, [(0, 0, 1)], cfg=dict(gate_mm=5.0))["code"]) == [T.MATCHED, T.FREE]
    assert col(step(T, state, [(0, 0, 6)], cfg=dict(gate_mm=5.0))["code"]) == [T.MATCHED, T.FREE]
    assert col(step(T, state, [(0, 0, 12)], cfg=dict(gate_mm=5.0))["code"]) == [T.COASTING, T.BORN]


def test_max_miss_edge(T):
    state = AC.new_state(T, 1, 1)
    step(T, state, [(5, 5, 1)])
    codes = [col(step(T, state, [None])["code"])[0] for _ in range(3)]
    assert codes == [T.COASTING, T.COASTING, T.ID_LOST]                     # max_miss = 2: two calls of waiting, the third releases
    assert col(state["ids"]) == [0] and col(state["miss"]) == [0] and np.isnan(state["last_uvd"]).all() and state["next_id"].tolist() == [2]
    # a candidate on the last allowed call is still this identity; max_miss = 0 releases at once
    state = AC.new_state(T, 1, 1)
    step(T, state, [(5, 5, 1)])
    step(T, state, [None])
    step(T, state, [None])
    assert col(step(T, state, [(6, 5, 1)])["code"]) == [T.MATCHED] and col(state["ids"]) == [1]
    assert col(step(T, state, [None], cfg=dict(AC.CFG, max_miss=0))["code"]) == [T.ID_LOST]
    # K = 1: a candidate outside the gate takes the coasting slot at once
    state = AC.new_state(T, 1, 1)
    step(T, state, [(5, 5, 1)])
    got = step(T, state, [(25, 5, 1)])
    assert col(got["code"]) == [T.BORN] and col(got["reset"]) == [1] and col(state["ids"]) == [2] and not got["dropped"].any()


def test_steal_order_and_its_ties(T):
    """no free slot: a birth takes the coasting slot with the largest miss, the lowest index on ties"""
    far = [(0, 0, 1), (20, 0, 1), (40, 0, 1)]
    state = AC.new_state(T, 3, 1)
    step(T, state, far)
    step(T, state, [far[0], None, far[2]])                                # slot 1 misses once
    got = step(T, state, [far[0], (60, 0, 1)])                            # slots 1 and 2 coast (miss 2 and 1); the stranger takes slot 1
    assert col(got["code"]) == [T.MATCHED, T.BORN, T.COASTING] and col(state["ids"]) == [1, 4, 3] and col(got["reset"]) == [0, 1, 0]
    assert col(state["miss"]) == [0, 0, 1] and not got["dropped"].any()
    # a tie: slots 0 and 2 have both missed once
    state = AC.new_state(T, 3, 1)
    step(T, state, far)
    got = step(T, state, [far[1], (60, 0, 1), (80, 0, 1)])
    assert col(got["code"]) == [T.BORN, T.MATCHED, T.BORN] and col(got["source"]) == [1, 0, 2] and col(state["ids"]) == [4, 2, 5]
    # neither a free nor a coasting slot: the candidate is dropped and counted (only a tracked slot can leave one over)
    state = AC.new_state(T, 2, 1)
    step(T, state, [(0, 0, 1), (20, 0, 1)])
    got = step(T, state, [(40, 0, 1), (60, 0, 1)], trk=[(0, 0, 1), (20, 0, 1)])
    assert col(got["code"]) == [T.TRACKED] * 2 and got["dropped"].tolist() == [2] and col(got["source"]) == [-2, -2] and state["next_id"].tolist() == [3]


def test_merge_releases_the_younger_identity(T):
    state = AC.new_state(T, 3, 1)
    step(T, state, [(0, 0, 1), (20, 0, 1), (40, 0, 1)])
    # the trackers of slots 0 and 1 end on one hand (2 mm apart: the edge is inclusive): identity 2 goes; slot 2 is 3 mm from slot 1 -- but
    # slot 1 is out of it by then, and 5 mm from slot 0 is no merge
    got = step(T, state, [None], trk=[(10, 0, 1), (12, 0, 1), (15, 0, 1)])
    assert col(got["code"]) == [T.TRACKED, T.MERGED, T.TRACKED] and col(state["ids"]) == [1, 0, 3] and np.isnan(state["last_uvd"][1]).all()
    assert col(got["status"]) == [OK, EMPTY, OK] and state["last_uvd"][0, 0].tolist() == [10.0, 0.0, 1.0]
    # chained pairs: 0-1 and 0-2 merge, so only the oldest survives; with the order of ids reversed the survivor is the last slot
    for ids, keep in (([1, 2, 3], 0), ([3, 2, 1], 2), ([2, 1, 3], 1)):
        state = AC.new_state(T, 3, 1)
        step(T, state, [(0, 0, 1), (20, 0, 1), (40, 0, 1)])
        state["ids"][:, 0] = ids
        got = step(T, state, [None], trk=[(10, 0, 1), (11, 0, 1), (12, 0, 1)])
        want = [T.MERGED] * 3
        want[keep] = T.TRACKED
        assert col(got["code"]) == want, (ids, col(got["code"]))
    # a released slot is free at once: a candidate is born into it in the same step, and the tracked slot's own candidate is a duplicate
    state = AC.new_state(T, 2, 1)
    step(T, state, [(0, 0, 1), (20, 0, 1)])
    got = step(T, state, [(10, 0, 1), (40, 0, 1)], trk=[(10, 0, 1), (11, 0, 1)])
    assert col(got["code"]) == [T.TRACKED, T.BORN] and col(got["source"]) == [-2, 1] and col(state["ids"]) == [1, 3] and not got["dropped"].any()
    # merge_mm = 0: only identical centres merge
    state = AC.new_state(T, 2, 1)
    step(T, state, [(0, 0, 1), (20, 0, 1)])
    cfg = dict(AC.CFG, merge_mm=0.0)
    assert col(step(T, state, [None], trk=[(10, 0, 1), (11, 0, 1)], cfg=cfg)["code"]) == [T.TRACKED] * 2
    assert col(step(T, state, [None], trk=[(10, 0, 1), (10, 0, 1)], cfg=cfg)["code"]) == [T.TRACKED, T.MERGED]


def test_a_tracked_slot_without_its_tracker_falls_back_to_the_candidates(T):
    state = AC.new_state(T, 2, 1)
    step(T, state, [(0, 0, 1), (20, 0, 1)])
    c, s = AC.frame(2, [(21, 0, 1), (1, 0, 1)])
    t, ts = AC.frame(2, [(2, 0, 1), (22, 0, 1)], status=[OK, EMPTY])
    got = AC.run(T, state, c, s, t, ts)
    assert col(got["code"]) == [T.TRACKED, T.MATCHED] and col(got["source"]) == [-2, 0]
    assert got["centers"][:, 0].tolist() == [[2.0, 0.0, 1.0], [21.0, 0.0, 1.0]] and not got["dropped"].any()      # candidate 1 was slot 0's own hand


def test_ids_are_never_reused(T):
    K, B = 3, 4
    state = AC.new_state(T, K, B)
    seen = [dict() for _ in range(B)]                       # id -> the step it was last live at
    for t, (cand, cstat, trk, tstat) in enumerate(AC.chain(K, B, T=60, seed=11, tracked=True)):
        before = state["next_id"].copy()
        got = AC.run(T, state, cand, cstat, trk, tstat)
        assert (state["next_id"] - before == got["reset"].sum(0)).all()
        for b in range(B):
            for i in state["ids"][:, b][state["ids"][:, b] > 0].tolist():
                assert seen[b].get(i, t - 1) == t - 1, "identity %d of frame %d came back" % (i, b)
                seen[b][i] = t
            born = state["ids"][:, b][got["reset"][:, b] == 1]
            assert sorted(born.tolist()) == list(range(before[b], state["next_id"][b]))


def test_candidates_that_are_not_usable(T):
    state = AC.new_state(T, 4, 1)
    c, s = AC.frame(4, [(0, 0, 1), (20, np.nan, 1), (40, 0, np.inf), (60, 0, 1)], status=[OK, OK, OK, AC.BAD_WINDOW])
    got = AC.run(T, state, c, s)
    assert col(got["code"]) == [T.BORN, T.FREE, T.FREE, T.FREE] and col(state["ids"]) == [1, 0, 0, 0] and not got["dropped"].any()
    # ... neither match nor are born: the identity at (0, 0, 1) coasts although a NaN row and a finite non-OK row are there
    c, s = AC.frame(4, [(np.nan, 0, 1), (0, 0, 1)], status=[OK, EMPTY])
    got = AC.run(T, state, c, s)
    assert col(got["code"]) == [T.COASTING, T.FREE, T.FREE, T.FREE] and state["next_id"].tolist() == [2]


def test_rows_past_n_valid_are_untouched(T):
    K, B, nv = 2, 3, 2
    state = AC.new_state(T, K, B)
    steps = AC.chain(K, B, T=6, seed=2, tracked=True)
    AC.run(T, state, *steps[0])
    kept = AC.copy_state(state)
    fs, fc = np.ones((K * B, 3, 6)), np.ones((K * B, 3, 2), np.int32)
    for cand, cstat, trk, tstat in steps[1:]:
        got = AC.run(T, state, cand, cstat, trk, tstat, n_valid=nv, filter_state=fs, filter_count=fc)
        for n in AC.STATE:
            past = (slice(None), slice(nv, None)) if state[n].ndim > 1 else slice(nv, None)
            assert AC.same(state[n][past], kept[n][past]), n
        assert np.isnan(got["centers"][:, nv:]).all() and (got["status"][:, nv:] == EMPTY).all() and not got["code"][:, nv:].any()
        assert not got["reset"][:, nv:].any() and (got["source"][:, nv:] == -1).all() and not got["dropped"][nv:].any()
    assert (state["ids"][:, :nv] != kept["ids"][:, :nv]).any()
    rows = fs.reshape(K, B, 3, 6)
    assert (rows[:, nv:] == 1).all() and (fc.reshape(K, B, 3, 2)[:, nv:] == 1).all() and (rows[:, :nv] == 0).any()


def test_filter_rows_are_zeroed_for_births_and_released_identities(T):
    K, B, nj = 3, 4, 3
    state = AC.new_state(T, K, B)
    for cand, cstat, trk, tstat in AC.chain(K, B, T=30, seed=5, tracked=True):
        fs, fc = np.full((K * B, nj, 6), 7.0), np.full((K * B, nj, 2), 7, np.int32)
        got = AC.run(T, state, cand, cstat, trk, tstat, filter_state=fs, filter_count=fc)
        cleared = (got["reset"] == 1) | (got["code"] == T.ID_LOST) | (got["code"] == T.MERGED)
        assert np.array_equal((fs == 0).all((1, 2)).reshape(K, B), cleared) and np.array_equal((fc == 0).all((1, 2)).reshape(K, B), cleared)
        assert np.array_equal((fs == 7).all((1, 2)).reshape(K, B), ~cleared)


def test_equal_cost_permutations_resolve_to_the_first(T):
    """slots at (0, 0) and (4, 0), candidates at (2, 3) and (2, -3): both pairings cost 13 + 13 -- the identity permutation wins; and the
    number of pairs beats the sum: one far pair and one near pair beat a single very near one"""
    state = AC.new_state(T, 2, 1)
    step(T, state, [(0, 0, 1), (4, 0, 1)])
    got = step(T, state, [(2, 3, 1), (2, -3, 1)])
    assert col(got["code"]) == [T.MATCHED] * 2 and col(got["source"]) == [0, 1]
    state = AC.new_state(T, 2, 1)
    step(T, state, [(0, 0, 1), (4, 0, 1)])
    got = step(T, state, [(2, -3, 1), (2, 3, 1)])
    assert col(got["source"]) == [0, 1]
    # K = 3 with all six pairings equal (an equilateral arrangement does not exist on integers: use three identical candidates' costs)
    state = AC.new_state(T, 3, 1)
    step(T, state, [(0, 0, 1), (0, 0, 2), (0, 0, 3)])
    state["last_uvd"][:, 0] = [(1, 1, 1)] * 3
    got = step(T, state, [(2, 1, 1), (1, 2, 1), (0, 1, 1)])
    assert col(got["source"]) == [0, 1, 2]
    # pairs before cost: slot 0 at 0, slot 1 at 6; candidates at 5 and 11: (0 -> 5, 1 -> 11) is 25 + 25, (1 -> 5) alone is 1
    state = AC.new_state(T, 2, 1)
    step(T, state, [(0, 0, 1), (6, 0, 1)])
    got = step(T, state, [(5, 0, 1), (11, 0, 1)])
    assert col(got["source"]) == [0, 1] and col(got["code"]) == [T.MATCHED] * 2
    # the permutations come in lexicographic order
    assert [T.permutation(p, 3) for p in range(6)] == [[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]]
    assert [T.permutation(p, 4) for p in range(24)] == [list(p) for p in itertools.permutations(range(4))]


def test_identity_option_validation(T):
    assert T.check_identity(True) == T.Identity(150.0, 60.0, 5) == T.Identity()
    assert T.check_identity(dict(gate_mm=80, max_miss=np.int64(2))) == T.Identity(80.0, 60.0, 2)
    assert T.check_identity(T.Identity(merge_mm=0)) == T.Identity(150.0, 0.0, 5)
    for bad, exc in ((dict(gate_mm=0.0), ValueError), (dict(gate_mm=-1.0), ValueError), (dict(gate_mm=math.inf), ValueError),
                     (dict(gate_mm=math.nan), ValueError), (dict(merge_mm=-1.0), ValueError), (dict(merge_mm=math.nan), ValueError),
                     (dict(max_miss=-1), ValueError), (dict(max_miss=1.5), TypeError), (dict(max_miss=True), TypeError),
                     (dict(gate_mm="far"), TypeError), (dict(gate=3.0), ValueError), (False, TypeError), (3, TypeError), (None, TypeError)):
        with pytest.raises(exc):
            T.check_identity(bad)
    with pytest.raises(AttributeError):
        T.Identity().gate_mm = 3.0
    with pytest.raises(ValueError):
        T.identity_state(5, 1)
    last, ids, miss, nxt = T.identity_state(2, 3)
    assert last.shape == (2, 3, 3) and np.isnan(last).all() and not ids.any() and not miss.any() and nxt.tolist() == [1, 1, 1]


def test_argument_errors_come_before_any_launch(T):
    """no GPU here: every refusal below returns before a HIP call"""
    import ctypes as C
    from awr_amd import _lib as L
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(K=2, B=1, nv=1, gate=150.0, merge=60.0, max_miss=5, fx=1.0, flip=1, last=p, trk=(None, None), filt=(None, None), nj=0, dropped=p):
        return L.lib.awr_hands_assign(last, p, p, p, p, p, trk[0], trk[1], K, B, nv, gate, merge, max_miss, fx, 1.0, 0.0, 0.0, flip, filt[0], filt[1],
                                      nj, p, p, p, p, p, dropped, None)
    for kw, word in ((dict(K=0), "K = 0"), (dict(K=5), "K = 5"), (dict(B=0), "B = 0"), (dict(nv=2), "n_valid"), (dict(nv=-1), "n_valid"),
                     (dict(flip=0), "flip"), (dict(flip=2), "flip"), (dict(last=None), "NULL"), (dict(dropped=None), "NULL"),
                     (dict(trk=(p, None)), "trk_"), (dict(filt=(None, p)), "filter_"), (dict(filt=(p, p), nj=0), "J = 0"),
                     (dict(filt=(p, p), nj=257), "J = 257"), (dict(gate=0.0), "gate_mm"), (dict(gate=math.nan), "gate_mm"),
                     (dict(merge=-1.0), "merge_mm"), (dict(max_miss=-1), "max_miss"), (dict(fx=0.0), "focal")):
        assert call(**kw) == -1 and word in L.last_error(), (kw, L.last_error())
    assert not any(buf)
