"""GPU: hand identities across calls -- awr_hands_assign against awr_amd.track.assign_step, np.array_equal (NaN positions
equal) on every output and on all state after every step of chains whose state never leaves the device, and
awr_amd.Predictor(hands=K, identity=...) against compositions of the plain hands predictor and the statements."""
import types

import numpy as np
import pytest
import torch

import assign_cases as AC
import hands_cases as HC

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 256, 0x5A
NJ = 3                                  # joints of the filter state the kernel zeroes
CAMERAS = {"exact": (AC.PARAS, AC.FLIP, AC.CFG, None),
           # NYU's camera: the integer walk scaled to pixels and millimetres, so every division rounds
           "nyu": ((588.03, 587.07, 320.0, 240.0), -1, dict(gate_mm=30.0, merge_mm=8.0, max_miss=2), ((4.0, 4.0, 40.0), (300.0, 200.0, 500.0)))}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T():
    import awr_amd  # noqa: F401
    from awr_amd import track
    return track


class Guarded:
    """a device tensor with GUARD bytes of a known pattern on either side"""

    def __init__(self, array, dev):
        array = np.ascontiguousarray(array)
        n = array.nbytes
        self.whole = torch.full((2 * GUARD + n,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        self.t = self.whole[GUARD:GUARD + n].view(getattr(torch, array.dtype.name)).view(array.shape)
        self.t.copy_(torch.from_numpy(array))
        self.n = n

    def intact(self):
        return bool((self.whole[:GUARD] == GUARD_BYTE).all()) and bool((self.whole[GUARD + self.n:] == GUARD_BYTE).all())

    def numpy(self):
        return self.t.cpu().numpy()


def camera_steps(K, B, camera, tracked, steps=12):
    paras, flip, cfg, affine = CAMERAS[camera]
    out = []
    for cand, cstat, trk, tstat in AC.chain(K, B, T=steps, seed=len(camera), tracked=tracked):
        if affine is not None:
            scale, offset = np.array(affine[0]), np.array(affine[1])
            cand = cand * scale + offset
            trk = None if trk is None else trk * scale + offset
        out.append((cand, cstat, trk, tstat))
    return paras, flip, cfg, out


def run_chain(T, dev, K, B, camera, tracked, filtered, n_valid=None, compare=True):
    """-> the list, per step, of every output and all state as numpy; with `compare` each is checked against the statement"""
    paras, flip, cfg, steps = camera_steps(K, B, camera, tracked)
    state = dict(zip(AC.STATE, T.identity_state(K, B)))
    fs = fc = None
    rs = np.random.RandomState(K + B)
    if n_valid is not None:             # the slots past n_valid hold identities of their own, which no step may touch
        state["ids"][:, n_valid:], state["miss"][:, n_valid:], state["next_id"][n_valid:] = 7, 1, 9
        state["last_uvd"][:, n_valid:] = rs.uniform(1, 30, state["last_uvd"][:, n_valid:].shape)
    if filtered:
        fs, fc = rs.uniform(-300, 300, (K * B, NJ, 6)), rs.randint(1, 9, (K * B, NJ, 2)).astype(np.int32)
    d_state = {n: Guarded(state[n], dev) for n in AC.STATE}                 # uploaded once, never again
    d_fs, d_fc = (Guarded(fs, dev), Guarded(fc, dev)) if filtered else (None, None)
    outs = [Guarded(np.full((K, B, 3), -7.0), dev)] + [Guarded(np.full((K, B), -7, np.int32), dev) for _ in range(4)] + [Guarded(np.full(B, -7, np.int32), dev)]
    record, seen = [], set()
    for t, (cand, cstat, trk, tstat) in enumerate(steps):
        ins = [Guarded(a, dev) if a is not None else None for a in (cand, cstat, trk, tstat)]
        got = T.assign_step_device(*(d_state[n].t for n in AC.STATE), ins[0].t, ins[1].t, None if trk is None else ins[2].t,
                                   None if trk is None else ins[3].t, cfg, n_valid, paras, flip, None if d_fs is None else d_fs.t,
                                   None if d_fc is None else d_fc.t, out=tuple(o.t for o in outs))
        assert all(g.data_ptr() == o.t.data_ptr() for g, o in zip(got, outs))
        now = [o.numpy() for o in outs] + [d_state[n].numpy() for n in AC.STATE] + ([d_fs.numpy(), d_fc.numpy()] if filtered else [])
        record.append(now)
        for g in outs + list(d_state.values()) + [i for i in ins if i is not None] + ([d_fs, d_fc] if filtered else []):
            assert g.intact(), (t, "a guard word was overwritten")
        for i, a in zip(ins, (cand, cstat, trk, tstat)):
            assert i is None or AC.same(i.numpy(), a), (t, "an input was written")
        if compare:
            want = T.assign_step(state["last_uvd"], state["ids"], state["miss"], state["next_id"], cand, cstat, trk, tstat, cfg, n_valid, paras, flip,
                                 fs, fc)
            names = AC.NAMES + AC.STATE + (("filter_state", "filter_count") if filtered else ())
            for g, w, name in zip(now, list(want) + [state[n] for n in AC.STATE] + ([fs, fc] if filtered else []), names):
                assert AC.same(g, w), (t, name, g, w)
            seen |= set(np.unique(want[2]).tolist())
    return record, seen


@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("B", (1, 4, 5, 9))
@pytest.mark.parametrize("K", (1, 2, 3, 4))
def test_kernel_equals_the_statement_after_every_step(T, dev, K, B, camera):
    """B = 5 and 9 cross the four-frames-per-workgroup boundary; tracked inputs on and off, filter pointers NULL and given"""
    seen = set()
    for tracked in (False, True):
        for filtered in (False, True):
            seen |= run_chain(T, dev, K, B, camera, tracked, filtered)[1]
    assert seen >= {T.BORN, T.MATCHED, T.TRACKED, T.COASTING}, seen


def test_kernel_leaves_rows_past_n_valid_alone(T, dev):
    for K, B, nv in ((2, 5, 3), (4, 9, 4), (3, 4, 0)):
        run_chain(T, dev, K, B, "exact", True, True, n_valid=nv)


def test_the_same_chain_twice_is_bitwise_equal(T, dev):
    a, _ = run_chain(T, dev, 4, 9, "nyu", True, True, compare=False)
    b, _ = run_chain(T, dev, 4, 9, "nyu", True, True, compare=False)
    assert len(a) == len(b) == 12
    for x, y in zip(a, b):
        assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(x, y))


def test_argument_errors_leave_the_outputs_untouched(T, dev):
    from awr_amd import _lib as L
    K, B = 2, 3
    state = [Guarded(a, dev) for a in T.identity_state(K, B)]
    cand, cstat = Guarded(np.ones((K, B, 3)), dev), Guarded(np.zeros((K, B), np.int32), dev)
    outs = [Guarded(np.full((K, B, 3), -7.0), dev)] + [Guarded(np.full((K, B), -7, np.int32), dev) for _ in range(4)] + [Guarded(np.full(B, -7, np.int32), dev)]
    before = [s.numpy() for s in state]

    def call(K=K, B=B, nv=B, gate=150.0, flip=-1, last=state[0].t, trk=(None, None), filt=(None, None), nj=0):
        return L.lib.awr_hands_assign(L.ptr(last), L.ptr(state[1].t), L.ptr(state[2].t), L.ptr(state[3].t), L.ptr(cand.t), L.ptr(cstat.t), L.ptr(trk[0]),
                                      L.ptr(trk[1]), K, B, nv, gate, 60.0, 5, 588.0, 587.0, 320.0, 240.0, flip, L.ptr(filt[0]), L.ptr(filt[1]), nj,
                                      *(L.ptr(o.t) for o in outs), L.stream())
    for kw, word in ((dict(K=0), "K = 0"), (dict(K=5), "K = 5"), (dict(B=0), "B = 0"), (dict(nv=B + 1), "n_valid"), (dict(flip=0), "flip"),
                     (dict(last=None), "NULL"), (dict(trk=(cand.t, None)), "trk_"), (dict(filt=(cand.t, None)), "filter_"),
                     (dict(filt=(cand.t, cstat.t), nj=0), "J = 0"), (dict(gate=-1.0), "gate_mm")):
        assert call(**kw) == -1 and word in L.last_error(), (kw, L.last_error())
    torch.cuda.synchronize()
    assert all((o.numpy() == -7).all() and o.intact() for o in outs) and all(AC.same(s.numpy(), w) for s, w in zip(state, before))
    with pytest.raises(L.AwrError, match="cand_uvd"):
        T.assign_step_device(*(s.t for s in state), cand.t[:, :2], cstat.t)
    with pytest.raises(L.AwrError, match="trk_"):
        T.assign_step_device(*(s.t for s in state), cand.t, cstat.t, trk_uvd=cand.t)
    # and the legal call does write them: K = 1 is legal at this level
    assert call() == 0
    one = T.assign_step_device(*(s.t[:1] for s in state[:3]), state[3].t, cand.t[:1], cstat.t[:1])
    torch.cuda.synchronize()
    assert (outs[2].numpy() == T.BORN).all() and one[2].tolist() == [[T.MATCHED] * B]


# ---- the Predictor ----------------------------------------------------------------------------------------------------------------------
# (the tiny network and the composites of tests/test_hands_gpu.py's fixtures, built here again: that file is not imported)
S, J, NB = 64, 14, 8
SHARED = ("xyz", "uvd", "center_xyz", "M", "status", "n_hands")
FLIP, CUBE = -1, (300.0, 300.0, 300.0)
EH, EW = 120, 160
E_PARAS = (147.0, 146.8, 80.0, 60.0)                # NYU's intrinsics scaled to a 160 x 120 frame
SMALL = dict(cube=CUBE, paras=E_PARAS, flip=FLIP, frame_shape=(EH, EW), depth_range=(200.0, 1200.0), slab=100.0, refine_iters=2)


def blobs(*hands):
    """one 120 x 160 frame: a far plane and, per (u, v, z), a hand-sized blob of 41 x 41 pixels at z ... z + 4 mm"""
    f = np.full((1, EH, EW), 1400, np.uint16)
    vv, uu = np.mgrid[0:EH, 0:EW]
    for cu, cv, z in hands:
        m = (np.abs(uu - cu) <= 20) & (np.abs(vv - cv) <= 20)
        f[0][m] = (z + (uu[m] + vv[m]) % 5).astype(np.uint16)
    return f


@pytest.fixture(scope="module")
def e2e(dev):
    import awr_amd
    import awr_oracle as O
    from awr_amd import synth as SY
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    net = net.cuda().eval()
    prims_a, bbox_a, prims_b, bbox_b = HC.two_hands()
    fa = torch.empty((NB,) + HC.FULL, dtype=torch.uint16, device=dev)
    fb = torch.empty_like(fa)
    SY.render_device(prims_a[:NB], bbox_a[:NB], fa)
    SY.render_device(prims_b[:NB], bbox_b[:NB], fb)
    frames = SY.compose(fa, fb)

    def make(max_batch=NB, **kw):
        return awr_amd.Predictor(net, S, 1.0, max_batch=max_batch, **kw)

    def small(**kw):
        return awr_amd.Predictor(net, S, 1.0, max_batch=1, hands=2, **SMALL, **kw)
    return types.SimpleNamespace(make=make, small=small, frames=frames)


def same_t(a, b):
    return AC.same(a.cpu().numpy(), b.cpu().numpy() if isinstance(b, torch.Tensor) else b)


def test_first_call_equals_the_plain_hands_predictor(T, e2e):
    """from a clean state every candidate is born, in candidate order: the rows are where Predictor(hands=2) has them, so the bits are"""
    from awr_amd import predictor as P
    plain, ident = e2e.make(hands=2, confidence=True), e2e.make(hands=2, identity=True, confidence=True)
    want, got = plain.predict(e2e.frames), ident.predict(e2e.frames)
    assert type(got) is P.ConfidentTrackedHandsPrediction and type(want) is P.ConfidentHandsPrediction
    assert got._fields == P.HandsPrediction._fields + ("ids", "conf", "peak", "spread_mm")
    for f in SHARED + ("conf", "peak", "spread_mm"):
        g, w = getattr(got, f), getattr(want, f)
        assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w) and not torch.isnan(g.float()).any(), f
    assert got.ids.dtype == torch.int32 and got.ids.tolist() == [[1, 2]] * NB and got.n_hands.tolist() == [2] * NB
    assert ident.hand_codes.tolist() == [[T.BORN] * 2] * NB and ident.hand_source.tolist() == [[0, 1]] * NB and ident.hands_dropped.tolist() == [0] * NB
    assert torch.equal(ident.hand_info, plain.hand_info)
    ident.check()
    # the same frames again: every hand is matched to itself, nothing moves, the bits stay
    again = ident.predict(e2e.frames)
    assert again.ids.tolist() == [[1, 2]] * NB and ident.hand_codes.tolist() == [[T.MATCHED] * 2] * NB
    assert all(torch.equal(getattr(again, f), getattr(want, f)) for f in SHARED)
    # explicit centres are the candidates: handed in the other order, the identities stay where they are
    swapped = ident._centers.view(2, NB, 3).transpose(0, 1).flip(1).clone()
    out = ident.predict(e2e.frames, centers_uvd=swapped)
    assert out.ids.tolist() == [[1, 2]] * NB and ident.hand_source.tolist() == [[1, 0]] * NB and ident.hand_info is None
    # n_valid: the slots past it keep their identities and report nothing
    part = ident.predict(e2e.frames[:3], n_valid=2)
    assert part.ids.tolist() == [[1, 2]] * 3 and part.status[2].tolist() == [1, 1] and part.n_hands.tolist() == [2, 2, 0]
    ident.reset_identity(slots=[1])
    out = ident.predict(e2e.frames)
    assert out.ids.tolist() == [[1, 2], [3, 4]] + [[1, 2]] * (NB - 2) and ident.hand_codes[1].tolist() == [T.BORN] * 2
    ident.reset_identity()
    assert not ident._id_ids.any() and torch.isnan(ident._id_last).all() and ident._id_next.tolist() == [3, 5] + [3] * (NB - 2)


def test_ids_follow_the_hands_when_they_swap_depth_order(T, e2e):
    plain, ident = e2e.small(), e2e.small(identity=True)
    a, b = (45, 60), (115, 60)
    first, second = blobs(a + (600,), b + (650,)), blobs(a + (670,), b + (620,))
    p1, i1 = plain.predict(first), ident.predict(first)
    assert i1.ids.tolist() == [[1, 2]] and all(torch.equal(getattr(p1, f), getattr(i1, f)) for f in SHARED)
    assert float(p1.center_xyz[0, 0, 0]) < 0 < float(p1.center_xyz[0, 1, 0])           # slot 0 is blob a, on the left
    p2, i2 = plain.predict(second), ident.predict(second)
    # the plain predictor's slots are depth ranks: they swap; the identities do not
    assert float(p2.center_xyz[0, 0, 0]) > 0 > float(p2.center_xyz[0, 1, 0])
    assert i2.ids.tolist() == [[1, 2]] and ident.hand_source.tolist() == [[1, 0]] and ident.hand_codes.tolist() == [[T.MATCHED] * 2]
    assert torch.equal(i2.center_xyz, p2.center_xyz.flip(1)) and torch.equal(i2.M, p2.M.flip(1)) and i2.status.tolist() == [[0, 0]]
    assert torch.equal(ident.hand_info, plain.hand_info)                                # (stays in candidate order)
    # blob a leaves: its slot waits, EMPTY with NaN rows -- and that is no error although it is slot 0
    i3 = ident.predict(blobs(b + (620,)))
    assert i3.ids.tolist() == [[1, 2]] and i3.status.tolist() == [[1, 0]] and i3.n_hands.tolist() == [1] and ident.hand_codes.tolist() == [[T.COASTING, T.MATCHED]]
    assert torch.isnan(i3.xyz[0, 0]).all() and not torch.isnan(i3.xyz[0, 1]).any()
    ident.check()
    plain.predict(blobs(b + (620,)))
    plain.check()                               # (the plain predictor's slot 0 is the nearest hand, whichever it is)
    # ... and comes back where it was: the same identity
    i4 = ident.predict(second)
    assert i4.ids.tolist() == [[1, 2]] and ident.hand_codes.tolist() == [[T.MATCHED] * 2]
    # no hand at all is an error
    from awr_amd import _lib as L
    ident.predict(np.zeros((1, EH, EW), np.uint16))
    with pytest.raises(L.AwrError, match="no hand slot is OK"):
        ident.check()


def hand_major(t):
    """a prediction's (nb, K, ...) field as the (K * nb, ...) rows of the hand-major buffers"""
    return t.transpose(0, 1).reshape((-1,) + tuple(t.shape[2:])).cpu().numpy()


def test_smooth_equals_the_filter_statement_on_the_slot_ordered_joints(T, e2e):
    """three hands come and go over two slots: the filter follows the SLOT, and a birth into a stolen slot starts its track again"""
    cfg = dict(gate_mm=500.0, max_coast=3)
    ident = e2e.small(identity=dict(max_miss=3), smooth=cfg)
    a, b, c = (45, 40), (115, 40), (115, 95)
    calls = [blobs(a + (600,), b + (650,)), blobs((46, 41, 604), (116, 41, 652)), blobs((47, 41, 606), c + (640,)), blobs((48, 42, 608), (116, 96, 642))]
    state, count = T.filter_state(2, J)
    want_codes = [[T.BORN, T.BORN], [T.MATCHED, T.MATCHED], [T.MATCHED, T.BORN], [T.MATCHED, T.MATCHED]]
    firsts = []
    for i, frame in enumerate(calls):
        out = ident.predict(frame, dt=0.04)
        assert type(out).__name__ == "TrackedHandsPrediction" and ident.hand_codes.tolist() == [want_codes[i]], (i, ident.hand_codes.tolist())
        assert ident.raw_xyz.shape == (1, 2, J, 3) and ident.filter_codes.shape == (1, 2, J) and ident.ahead_xyz.shape == (1, 2, J, 3)
        codes = ident.hand_codes[0].tolist()
        for k in range(2):                      # what awr_hands_assign does to the filter rows of a slot whose identity starts or ends
            if codes[k] in (T.BORN, T.ID_LOST, T.MERGED):
                state[k], count[k] = 0.0, 0
        want = T.filter_step(state, count, hand_major(ident.raw_xyz), hand_major(out.status), ident._last[1].reshape(-1).cpu().numpy(), None, cfg,
                             0.04, None, E_PARAS, FLIP)
        for g, w, name in ((out.xyz, want[0], "xyz"), (out.uvd, want[1], "uvd"), (ident.ahead_xyz, want[2], "ahead"), (ident.filter_codes, want[3], "codes")):
            assert AC.same(hand_major(g), w), (i, name)
        assert same_t(ident._filter_state, state) and same_t(ident._filter_count, count), i
        firsts.append(want[3][:, 0].tolist())
    # the third call's slot 1 is another hand (500 mm gate: the filter alone would have filtered it in): its track starts again
    assert out.ids.tolist() == [[1, 3]] and firsts == [[T.INIT, T.INIT], [T.UPDATED, T.UPDATED], [T.UPDATED, T.INIT], [T.UPDATED, T.UPDATED]], firsts
    assert not same_t(out.xyz, ident.raw_xyz)
    # reset_smooth / reset_identity take the hand axis: batch slot 0 is rows 0 and 1
    ident.reset_smooth(slots=[0])
    assert not ident._filter_state.any() and not ident._filter_count.any() and ident._id_ids.tolist() == [[1], [3]]
    ident.reset_identity()
    assert not ident._id_ids.any()


def test_track_equals_the_composition_of_the_statements(T, D, e2e):
    """detect over the components' seeds and over the slots' last centres, assign_step, joints_center: the centres the crops are made at"""
    ident = e2e.small(identity=True, track=True)
    last, ids, miss, nxt_id = T.identity_state(2, 1)
    a, b = (45, 60), (115, 60)
    calls = [blobs(a + (600,), b + (650,)), blobs((47, 61, 640), (113, 60, 620)), blobs((48, 62, 645), (112, 60, 615))]
    kw = dict(cube=CUBE, paras=E_PARAS, depth_range=SMALL["depth_range"], slab=SMALL["slab"], iters=SMALL["refine_iters"])
    seen = []
    for i, frame in enumerate(calls):
        if i == 1:
            # tracked centres from outside, (n, K, 3): on the blobs, so this call's slots are held by their trackers
            given = np.array([[[47.0, 61.0, 642.0], [113.0, 60.0, 622.0]]])
            ident.set_track(given)
            last[:, 0] = given[0]
            assert same_t(ident._id_last, last) and same_t(ident._id_ids, ids)
        out = ident.predict(frame)
        seeds, _, info, _ = D.hand_seeds(frame[0], 2, SMALL["depth_range"], D.REACH, SMALL["slab"], D.MIN_PIXELS)
        cand, cstat, trk, tstat = np.empty((2, 1, 3)), np.empty((2, 1), np.int32), np.empty((2, 1, 3)), np.empty((2, 1), np.int32)
        for k in range(2):
            cand[k, 0], cstat[k, 0] = D.detect(frame[0], "given", seeds[k], **kw)
            trk[k, 0], tstat[k, 0] = D.detect(frame[0], "given", last[k, 0], **kw)
        centers, status, code, _, source, dropped = T.assign_step(last, ids, miss, nxt_id, cand, cstat, trk, tstat, True, None, E_PARAS, FLIP)
        assert same_t(ident.centers_uvd, centers.transpose(1, 0, 2)) and same_t(out.status, status.T), (i, ident.centers_uvd, centers)
        assert same_t(ident.hand_codes, code.T) and same_t(ident.hand_source, source.T) and same_t(ident.hands_dropped, dropped) and same_t(out.ids, ids.T)
        moved = D.joints_center(hand_major(out.xyz), centers.reshape(2, 3), hand_major(out.center_xyz), np.tile(np.float32(CUBE), (2, 1)), status.reshape(2),
                                ident._last[1].reshape(-1).cpu().numpy(), E_PARAS, FLIP, depth_range=SMALL["depth_range"], max_shift=1.0)
        assert same_t(ident.next_centers_uvd, moved[1].reshape(2, 1, 3).transpose(1, 0, 2)) and ident.recenter_codes[-1].tolist() == moved[2].reshape(2, 1).T.tolist()
        finite = np.isfinite(moved[1]).all(-1).reshape(2, 1)
        last[finite] = moved[1].reshape(2, 1, 3)[finite]
        assert same_t(ident._id_last, last) and same_t(ident._id_miss, miss) and same_t(ident._id_next, nxt_id), i
        seen.append(code[:, 0].tolist())
    print("assignment codes per call:", seen, "recentre codes of the last call:", ident.recenter_codes.tolist())
    assert seen[0] == [T.BORN] * 2 and seen[1] == [T.TRACKED] * 2
    # a NaN row ends its slot's identity; reset_track forgets a batch slot's identities altogether
    ident.set_track(np.array([[[48.0, 62.0, 645.0], [np.nan] * 3]]), slots=[0])
    assert ident._id_ids.tolist() == [[int(ids[0, 0])], [0]] and torch.isnan(ident._id_last[1]).all() and not torch.isnan(ident._id_last[0]).any()
    ident.reset_track()
    assert not ident._id_ids.any()


@pytest.fixture(scope="module")
def D():
    import awr_amd  # noqa: F401
    from awr_amd import detect
    return detect


def test_identity_none_is_todays_path(e2e, monkeypatch):
    """the same launches, in the same order with the same sizes, and the same bits as no argument"""
    from awr_amd import _lib as L
    from awr_amd import predictor as P
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append((name,) + tuple(x for x in a if isinstance(x, (int, float)) and not isinstance(x, bool) and abs(x) < 1 << 20)), real(name, *a))[1])
    a, b = e2e.make(max_batch=2, hands=2), e2e.make(max_batch=2, hands=2, identity=None)
    a.predict(e2e.frames[:2])                       # (an engine's first call also uploads its weights: compare the calls after it)
    b.predict(e2e.frames[:2])
    calls.clear()
    out_a = a.predict(e2e.frames[:2])
    calls_a = list(calls)
    calls.clear()
    out_b = b.predict(e2e.frames[:2])
    assert calls == calls_a and len(calls) >= 4 and not any(c[0] == "awr_hands_assign" for c in calls)
    assert type(out_b) is P.HandsPrediction and all(torch.equal(getattr(out_a, f), getattr(out_b, f)) for f in SHARED)
    assert b.identity is None and not any(name.startswith("_id_") or name in ("_cand", "hand_codes") for name in vars(b))
    # with identity there is exactly one more launch, between the detector and the crop
    c = e2e.make(max_batch=2, hands=2, identity=True)
    c.predict(e2e.frames[:2])
    calls.clear()
    c.predict(e2e.frames[:2])
    names_a, names_c = [x[0] for x in calls_a], [x[0] for x in calls]
    at = names_c.index("awr_hands_assign")
    assert names_c[:at] + names_c[at + 1:] == names_a and names_c[at - 1] == "awr_detect" and names_c[at + 1] == "awr_detect_samples"


def test_identity_option_errors(D, e2e):
    from awr_amd import _lib as L
    with pytest.raises(ValueError, match="hands >= 2"):
        e2e.make(max_batch=1, identity=True)
    with pytest.raises(ValueError, match="not combined yet"):
        e2e.make(max_batch=1, hands=2, identity=True, views=D.make_views(rot=(10.0,)))
    for bad, exc in ((3, TypeError), (False, TypeError), (dict(gate_mm=0.0), ValueError), (dict(gate=1.0), ValueError), (dict(max_miss=1.5), TypeError)):
        with pytest.raises(exc):
            e2e.make(max_batch=1, hands=2, identity=bad)
    with pytest.raises(ValueError, match="track=True"):
        e2e.make(max_batch=1, hands=2, identity=True, smooth=dict(lead=True))
    plain = e2e.small(identity=True)
    with pytest.raises(L.AwrError, match="dt"):
        plain.predict(blobs((45, 60, 600)), dt=0.03)
    for name in ("set_track", "reset_track", "reset_smooth"):
        with pytest.raises(L.AwrError):
            getattr(plain, name)(np.zeros((1, 2, 3))) if name == "set_track" else getattr(plain, name)()
    with pytest.raises(L.AwrError, match="identity"):
        e2e.small().reset_identity()
    # track, smooth, lead and dt are accepted with identity
    full = e2e.small(identity=dict(max_miss=4), track=True, smooth=dict(lead=True), recenter=1, palm=True, confidence=True)
    for z in (600, 604):
        out = full.predict(blobs((45, 60, z), (115, 60, z + 50)), dt=0.03)
    assert bool((out.ids > 0).all()) and out.xyz.shape == (1, 2, J, 3) and full.recenter_codes.shape == (2, 1, 2) and full.palm_info.shape == (1, 2, 4)
    assert type(out).__name__ == "ConfidentTrackedHandsPrediction" and out.conf.shape == (1, 2, J) and full.ahead_xyz.shape == (1, 2, J, 3)
    assert full.identity == full.identity.__class__(150.0, 60.0, 4)
    with pytest.raises(L.AwrError, match="centers_uvd"):
        full.set_track(np.zeros((1, 3)))
    full.check()
