"""GPU: winograd="auto" -- the engines time their candidate plans (winograd_auto.py) and run the chosen one.  The search leaves no trace (parameters,
BatchNorm running statistics, optimiser state, inputs), frees every candidate it built, runs exactly the plan an explicit engine of the chosen mode
runs, meets the golden bars, and a second engine with the same AWR_TUNE_CACHE reuses the stored decision without building a candidate."""
import gc
import os

import numpy as np
import pytest
import torch

import awr_oracle as O
from test_nets_gpu import NORTH_STAR_MEAN_MM, assert_joints, check_grad_norms, make_net, oracle_fp64_joint_gap, smp_index_stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import awr_amd
    assert torch.cuda.is_available()
    return awr_amd


@pytest.fixture(autouse=True)
def no_cache(monkeypatch):
    monkeypatch.delenv("AWR_TUNE_CACHE", raising=False)


def _state(eng):
    m = eng.net
    return [m.flat_params().clone(), m._barena.clone(), eng.m.clone(), eng.v.clone(), eng.plan.img.clone(), eng.jt_gt.clone()]


def test_resnet18_auto_leaves_no_trace_and_meets_the_golden_bars(amd, golden_dir):
    """tests/golden/resnet_18_train_b8.npz (the bars of test_nets_gpu.test_well_conditioned_training_fixture_meets_the_plain_bar_in_every_mode)"""
    from awr_amd import winograd_auto as WA
    from awr_amd.trainer import TrainEngine
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(golden_dir, "resnet_18_train_b8.npz"))
    net, J, ks, B = "resnet_18", int(g["J"]), float(g["ks"]), int(g["B"])
    img, jt_gt = O.synth_batch(B, 128, J, seed=int(g["img_seed"]))
    pkeys = [str(k) for k in g["pkeys"]]
    for tag, cw in (("c0", 0.0), ("c1", 1.0)):
        m = make_net(amd, net, J, O.reference_init_state(net, J, seed=int(g["w_seed"])))
        eng = TrainEngine(m, B, 128, ks, coord_weight=cw, dense_weight=1.0, lr=1e-3, use_graph=False, winograd="auto")
        assert eng._wino_pending and eng.winograd_timings is None
        eng.plan.img.copy_(img.to(dev))
        eng.jt_gt.copy_(jt_gt.to(dev))
        before, count = _state(eng), eng.step_count
        eng.compile()
        torch.cuda.synchronize()
        after = _state(eng)
        for name, a, b in zip(("params", "bn buffers", "m", "v", "img", "jt_gt"), before, after):
            assert torch.equal(a, b), name
        assert eng.step_count == count
        assert eng.winograd_mode in WA.MODES and eng.winograd_source == "search"
        assert eng.winograd_mode in eng.winograd_timings and all(t > 0 for t in eng.winograd_timings.values())
        assert list(m._plans.values()) == [eng.plan]                    # every other candidate was freed
        m2 = make_net(amd, net, J, O.reference_init_state(net, J, seed=int(g["w_seed"])))
        assert eng.plan.n_winograd == m2.get_plan(B, 128, True, supervised=(0,), bn_repeat=1, accum="auto", winograd=eng.winograd_mode).n_winograd
        del m2
        losses, jt = eng.step(img.to(dev), jt_gt.to(dev))
        ref0 = float(g[tag + "_loss0"])
        assert abs(float(losses[2]) - ref0) <= 2e-4 * abs(ref0), (float(losses[2]), ref0)
        assert abs(float(losses[0]) - float(g[tag + "_lcoord0"])) <= 2e-4 * max(1e-6, abs(float(g[tag + "_lcoord0"]))) + 1e-9
        d = np.linalg.norm(jt.cpu().numpy().astype(np.float64) - g[tag + "_jt0"].astype(np.float64), axis=-1) * 150.0
        assert float(d.mean()) <= NORTH_STAR_MEAN_MM and float(d.max()) <= 5e-3, (tag, float(d.mean()), float(d.max()))
        pred = eng.plan.dense_map(0).cpu().reshape(-1).numpy()[g["pred_idx"]]
        ref = g[tag + "_pred_val"]
        assert float(np.abs(pred - ref).max()) <= 2e-4 * max(1.0, float(np.abs(ref).max()))
        check_grad_norms(m, pkeys, g[tag + "_grad_l2"], g[tag + "_grad_smp"], tol=5e-3)
    sd = m.state_dict()
    got = np.array([float(sd[str(k)].reshape(-1)[smp_index_stream(sd[str(k)].numel(), 90 + i)]) for i, k in enumerate(g["bn_keys"])], np.float32)
    np.testing.assert_allclose(got, g["bn_smp"], rtol=2e-4, atol=2e-6)


def test_forced_choice_runs_the_explicit_modes_plan(amd, monkeypatch):
    """An injected timer makes "full" win at batch 64 (where it has Winograd launches): the engine then runs the plan an explicit
    winograd="full" engine runs -- same launches, same step -- holds no candidate plan, and no more memory than that engine."""
    from awr_amd import winograd_auto as WA
    from awr_amd.trainer import TrainEngine
    dev = torch.device("cuda:0")
    J, B, ks = 14, 64, 1.0
    timed = []

    def fake_time_steps(fn, reps=5, per=3):
        code = fn.__self__.plan.winograd
        timed.append(code)
        return 1.0 if code == 2 else 10.0
    monkeypatch.setattr(WA, "time_steps", fake_time_steps)
    img, jt_gt = O.synth_batch(B, 128, J, seed=5)
    sd = O.reference_init_state("resnet_18", J, seed=4)
    ma, mf = make_net(amd, "resnet_18", J, sd), make_net(amd, "resnet_18", J, sd)
    gc.collect()        # engines of earlier tests that sit in reference cycles are freed now, not by a collection inside the windows measured below
    torch.cuda.synchronize()
    a0, f0 = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
    ea = TrainEngine(ma, B, 128, ks, coord_weight=1.0, use_graph=False, autotune=False, winograd="auto")
    ea.compile(img.to(dev), jt_gt.to(dev))
    torch.cuda.synchronize()
    a1, f1 = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
    assert ea.winograd_mode == "full" and 2 in timed and timed[0] == 0
    assert list(ma._plans.values()) == [ea.plan]
    ef = TrainEngine(mf, B, 128, ks, coord_weight=1.0, use_graph=False, autotune=False, winograd="full")
    ef.compile(img.to(dev), jt_gt.to(dev))
    torch.cuda.synchronize()
    a2, f2 = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
    assert ef.plan.n_winograd > 0 and ea.plan.n_winograd == ef.plan.n_winograd and ea.plan.winograd == ef.plan.winograd == 2
    assert ea.plan.op_names("fwd") == ef.plan.op_names("fwd") and ea.plan.op_names("bwd") == ef.plan.op_names("bwd")
    assert abs((a1 - a0) - (a2 - a1)) <= 1 << 20, (a1 - a0, a2 - a1)
    # the native buffers (not torch allocations): the candidates' are returned, not only dropped from the table
    assert abs((f0 - f1) - (f1 - f2)) <= max(256 << 20, ef.plan.bytes // 4), (f0 - f1, f1 - f2, ef.plan.bytes)
    la, ja = (t.clone() for t in ea.step(img.to(dev), jt_gt.to(dev)))
    lf, jf = (t.clone() for t in ef.step(img.to(dev), jt_gt.to(dev)))
    ga, gf = ma.flat_grads()[:ma.n_active], mf.flat_grads()[:mf.n_active]
    # (the default mode combines some partial sums with atomics, so two replays of one plan may differ in the last bits; deterministic mode,
    # which would make them bitwise equal, turns Winograd off)
    same = torch.equal(la, lf) and torch.equal(ja, jf) and torch.equal(ga, gf)
    print("auto vs explicit 'full' step bit-identical:", same)
    assert float((la - lf).abs().max()) <= 1e-5 * float(lf.abs().max())
    assert float((ja - jf).abs().max()) <= 1e-5
    assert float((ga - gf).abs().max()) <= 1e-4 * float(gf.abs().max())


def test_inference_engine_auto_on_hourglass(amd, golden_dir):
    from awr_amd.trainer import InferEngine
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(golden_dir, "hourglass_1_fwd.npz"))
    img = torch.from_numpy(g["img"])
    J, ks = int(g["J"]), float(g["ks"])
    man = O.manifest_for("hourglass_1", J)
    m = make_net(amd, "hourglass_1", J, O.procedural_state(man, seed=0))
    m.eval()
    inf = InferEngine(m, img.shape[0], 128, ks, autotune=False, winograd="auto")
    jt = inf(img.to(dev)).cpu()
    assert inf.winograd_mode in ("direct", "forward") and set(inf.winograd_timings) <= {"direct", "forward"}
    assert list(m._plans.values()) == [inf.plan]
    gaps = oracle_fp64_joint_gap("hourglass_1", O.procedural_state(man, seed=0), img, ks, False)
    assert_joints("hourglass_1/eval_auto/stage0", jt.numpy(), g["eval_s0_jt"], gaps[0])


def test_second_engine_reuses_the_cached_decision(amd, tmp_path, monkeypatch):
    from awr_amd import nets
    from awr_amd.trainer import TrainEngine
    dev = torch.device("cuda:0")
    monkeypatch.setenv("AWR_TUNE_CACHE", str(tmp_path / "tune.json"))
    J, B, ks = 14, 4, 1.0
    img, jt_gt = O.synth_batch(B, 128, J, seed=9)
    sd = O.reference_init_state("resnet_18", J, seed=2)
    built = []

    class CountingPlan(nets.Plan):
        def __init__(self, *a, **k):
            built.append(1)
            super().__init__(*a, **k)
    monkeypatch.setattr(nets, "Plan", CountingPlan)
    e1 = TrainEngine(make_net(amd, "resnet_18", J, sd), B, 128, ks, use_graph=False, autotune=False, winograd="auto")
    e1.step(img.to(dev), jt_gt.to(dev))
    assert e1.winograd_source == "search" and len(built) >= 1 + len(e1.winograd_timings) - 1
    n1 = len(built)
    e2 = TrainEngine(make_net(amd, "resnet_18", J, sd), B, 128, ks, use_graph=False, autotune=False, winograd="auto")
    losses, _ = e2.step(img.to(dev), jt_gt.to(dev))
    assert torch.isfinite(losses).all()
    assert e2.winograd_source == "cache" and not e2._wino_pending
    assert e2.winograd_mode == e1.winograd_mode and e2.winograd_timings == e1.winograd_timings
    assert len(built) == n1 + 1                                          # its own plan, nothing else
