"""CPU: winograd="auto" (awr_amd/winograd_auto.py) -- the mode strings the engines and the library accept, the choice rule, the collapsing of
candidates that build the same plan, deterministic mode, the tile-cache key that carries the Winograd code, the decision cache, and two gloo
ranks that time differently and still choose the same mode."""
import json
import os
import socket
import types

import pytest
import torch
import torch.multiprocessing as mp


@pytest.fixture(scope="module")
def amd():
    import awr_amd
    from awr_amd import build
    if not os.path.exists(build.LIB):
        build.build_lib(verbose=False)
    return awr_amd


@pytest.fixture(scope="module")
def WA(amd):
    from awr_amd import winograd_auto
    return winograd_auto


# ---- mode strings ---------------------------------------------------------------------------------------------------
def test_auto_is_an_engine_mode_not_a_library_code(amd):
    assert amd._engine_winograd("auto") == "auto"
    assert amd._engine_winograd(None) is None
    assert [amd._engine_winograd(m) for m in (False, True, "forward", "full", "forward+wgrad")] == [0, 1, 1, 2, 3]
    with pytest.raises(ValueError, match="engine"):
        amd.set_conv_winograd("auto")
    with pytest.raises(ValueError):
        amd._winograd_code("auto")


@pytest.mark.parametrize("bad", ["atuo", "off", "Full", "on"])
def test_unknown_mode_strings_are_refused(amd, bad):
    with pytest.raises(ValueError, match="unknown Winograd mode"):
        amd._winograd_code(bad)
    with pytest.raises(ValueError):
        amd._engine_winograd(bad)
    with pytest.raises(ValueError):
        amd.set_conv_winograd(bad)


def test_existing_values_and_codes_keep_their_meaning(amd):
    assert [amd._winograd_code(m) for m in (None, False, True, "forward", "full", "forward+wgrad", "force", 3)] == [0, 0, 1, 1, 2, 3, 6, 3]
    assert [amd._winograd_code(c) for c in (0, 1, 2, 4, 6, 12)] == [0, 1, 2, 4, 6, 12]
    assert amd._winograd_code("direct") == 0


def test_mode_names_of_library_codes(WA):
    assert [WA.mode_name(c) for c in (0, 1, 2, 3, 6, 4, 12)] == ["direct", "forward", "full", "forward+wgrad", "full", "forward", "forward"]
    assert [WA.mode_name(c, training=False) for c in (0, 1, 2, 3)] == ["direct", "forward", "forward", "forward"]


# ---- the choice -----------------------------------------------------------------------------------------------------
N4 = {"direct": 0, "forward": 10, "forward+wgrad": 16, "full": 24}


def test_choose_picks_the_fastest(WA):
    assert WA.choose({"direct": 12.9, "forward": 12.6, "forward+wgrad": 12.4, "full": 12.19}, N4) == "full"
    assert WA.choose({"direct": 10.0, "forward": 10.5, "forward+wgrad": 11.0, "full": 12.0}, N4) == "direct"
    assert WA.choose({"direct": 283.0, "forward": 270.0, "forward+wgrad": 257.0, "full": 262.0}, N4) == "forward+wgrad"


def test_choose_breaks_ties_within_the_margin_towards_fewer_winograd_launches(WA):
    assert WA.MARGIN == 0.01
    # full is fastest by 0.5 %: a tie with forward+wgrad (fewer Winograd launches)
    assert WA.choose({"direct": 20.0, "forward": 19.0, "forward+wgrad": 18.09, "full": 18.0}, N4) == "forward+wgrad"
    # ... and with everything inside 1 %: the direct plan
    assert WA.choose({"direct": 10.09, "forward": 10.05, "forward+wgrad": 10.02, "full": 10.0}, N4) == "direct"
    # just outside the margin: the fastest stays
    assert WA.choose({"direct": 10.2, "forward": 10.2, "forward+wgrad": 10.2, "full": 10.0}, N4) == "full"
    assert WA.choose({"direct": 10.2, "forward": 10.2, "forward+wgrad": 10.2, "full": 10.0}, N4, margin=0.05) == "direct"


def test_search_does_not_time_collapsed_candidates(WA):
    built, timed = [], []
    n = {"direct": 0, "forward": 0, "forward+wgrad": 6, "full": 6}      # no forward launch eligible; no data gradient either

    def build(mode):
        built.append(mode)
        return n[mode]

    def time_ms(mode):
        timed.append(mode)
        return {"direct": 10.0, "forward+wgrad": 9.0}[mode]
    mode, timings, nw, collapsed = WA.search(WA.TRAIN_CANDIDATES, build, time_ms)
    assert built == list(WA.TRAIN_CANDIDATES)
    assert timed == ["direct", "forward+wgrad"]
    assert timings == {"direct": 10.0, "forward+wgrad": 9.0} and mode == "forward+wgrad"
    assert collapsed == {"forward": "direct", "full": "forward+wgrad"} and nw == n
    # a batch where nothing is eligible: one plan timed, the direct one
    timed.clear()
    mode, timings, _, collapsed = WA.search(WA.TRAIN_CANDIDATES, lambda m: 0, lambda m: timed.append(m) or 5.0)
    assert mode == "direct" and timed == ["direct"] and set(collapsed) == {"forward", "forward+wgrad", "full"}
    assert set(collapsed.values()) == {"direct"}
    # inference: two candidates only
    mode, timings, _, _ = WA.search(WA.INFER_CANDIDATES, lambda m: {"direct": 0, "forward": 9}[m], lambda m: {"direct": 3.0, "forward": 2.5}[m])
    assert mode == "forward" and set(timings) == {"direct", "forward"}


def test_deterministic_mode_resolves_to_direct_without_timing(amd, WA):
    from awr_amd.trainer import _WinogradAuto
    eng = types.SimpleNamespace(net=types.SimpleNamespace(nstage=1, device="cpu"), J=14, B=8, H=128, _wino_pending=False)
    amd.set_deterministic(True)
    try:
        mode = _WinogradAuto._wino_start(eng, True, 2, None)
    finally:
        amd.set_deterministic(False)
    assert mode == "direct" and eng.winograd_source == "deterministic" and not eng._wino_pending
    assert list(eng.winograd_timings) == ["skipped"] and "deterministic" in eng.winograd_timings["skipped"]


def test_without_a_cached_decision_the_search_is_pending(amd, WA, tmp_path, monkeypatch):
    from awr_amd.trainer import _WinogradAuto
    monkeypatch.setenv("AWR_TUNE_CACHE", str(tmp_path / "tune.json"))
    eng = types.SimpleNamespace(net=types.SimpleNamespace(nstage=1, device="cpu"), J=14, B=8, H=128, _wino_pending=False)
    assert _WinogradAuto._wino_start(eng, True, 2, None) == "direct" and eng._wino_pending
    # ... and with one stored for exactly this plan: resolved, timings from the cache
    WA.store_decision(eng._wino_key, "full", {"direct": 12.9, "full": 12.2}, N4, {})
    eng2 = types.SimpleNamespace(net=eng.net, J=14, B=8, H=128, _wino_pending=False)
    assert _WinogradAuto._wino_start(eng2, True, 2, None) == "full"
    assert not eng2._wino_pending and eng2.winograd_source == "cache" and eng2.winograd_timings == {"direct": 12.9, "full": 12.2}
    # an inference plan of the same shape has its own key
    eng3 = types.SimpleNamespace(net=eng.net, J=14, B=8, H=128, _wino_pending=False)
    assert _WinogradAuto._wino_start(eng3, False, 0, None) == "direct" and eng3._wino_pending


# ---- caches ---------------------------------------------------------------------------------------------------------
def test_tile_cache_key_carries_the_winograd_code(amd, tmp_path):
    from awr_amd.engine import cached_tiles, tile_cache_key
    base = "train/ResNet18Deconv1/J14/B64/H128"
    kd, kf = tile_cache_key(base, 1, 1, 2, 0), tile_cache_key(base, 1, 1, 2, 2)
    assert kd == base + "/x1/s1/a2/w0" and kf == base + "/x1/s1/a2/w2" and kd != kf
    names = ["awr_conv_gemm:layer1.0.conv1", "awr_conv_wgrad:layer1.0.conv1"]
    f = tmp_path / "tune.json"
    f.write_text(json.dumps({kd: {n: [[128, 64, 2, 1], 10.0] for n in names}}))
    assert cached_tiles(str(f), kd, names) is not None
    assert cached_tiles(str(f), kf, names) is None                # a direct plan's entry is never applied to a "full" plan
    assert cached_tiles(str(f), kd, names + ["awr_wino_wgrad:layer1.0.conv1"]) is None
    # a file written before the key carried the code misses once
    f.write_text(json.dumps({base + "/x1/s1/a2": {n: [[128, 64, 2, 1], 10.0] for n in names}}))
    assert cached_tiles(str(f), kd, names) is None


def test_decision_cache_round_trip(WA, tmp_path, monkeypatch):
    f = tmp_path / "tune.json"
    monkeypatch.setenv("AWR_TUNE_CACHE", str(f))
    f.write_text(json.dumps({"train/x/w0": {"a": [[1, 1, 1, 0], 1.0]}}))          # tile entries share the file
    k = WA.decision_key(True, "ResNet18Deconv1", 14, 64, 128, 1, 1, 2)
    assert k != WA.decision_key(False, "ResNet18Deconv1", 14, 64, 128, 1, 1, 2) != WA.decision_key(True, "ResNet18Deconv1", 14, 64, 128, 1, 1, 0)
    assert WA.load_decision(k, WA.TRAIN_CANDIDATES) is None
    WA.store_decision(k, "full", {"direct": 12.9, "full": 12.2}, N4, {"forward": "direct"})
    ent = WA.load_decision(k, WA.TRAIN_CANDIDATES)
    assert ent["mode"] == "full" and ent["timings"] == {"direct": 12.9, "full": 12.2} and ent["n_winograd"] == N4
    assert WA.load_decision(k, WA.INFER_CANDIDATES) is None                   # not a candidate there
    assert "train/x/w0" in json.load(open(f))
    monkeypatch.delenv("AWR_TUNE_CACHE")
    assert WA.load_decision(k, WA.TRAIN_CANDIDATES) is None


# ---- data parallel --------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import awr_amd  # noqa: F401
    from awr_amd import winograd_auto as WA
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pg = torch.distributed.group.WORLD
        # rank 0 alone would pick "full", rank 1 alone "forward": the slowest rank's time per candidate decides for both
        mine = [{"direct": 10.0, "forward": 9.0, "forward+wgrad": 9.5, "full": 8.0},
                {"direct": 10.5, "forward": 8.5, "forward+wgrad": 9.4, "full": 12.0}][rank]
        n = {"direct": 0, "forward": 8, "forward+wgrad": 12, "full": 20}
        alone = WA.search(WA.TRAIN_CANDIDATES, n.get, mine.get)[0]
        mode, timings, _, _ = WA.search(WA.TRAIN_CANDIDATES, n.get, mine.get, WA.allreduce_max_fn(pg, "cpu"))
        # a cached decision is used only where every rank read the same one
        same = WA.agree("full", WA.TRAIN_CANDIDATES, pg, "cpu")
        split = WA.agree("full" if rank == 0 else None, WA.TRAIN_CANDIDATES, pg, "cpu")
        q.put((rank, alone, mode, timings, same, split))
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_with_different_timings_choose_the_same_mode_gloo():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, a0, m0, t0, s0, x0), (_, a1, m1, t1, s1, x1) = res
    assert (a0, a1) == ("full", "forward")
    assert m0 == m1 == "forward"
    assert t0 == t1 == {"direct": 10.5, "forward": 9.0, "forward+wgrad": 9.5, "full": 12.0}
    assert s0 == s1 == "full" and x0 is None and x1 is None
