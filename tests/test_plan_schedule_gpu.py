"""The plan engine's schedule, pinned to the commit before its scheduling moved from op names to op fields (csrc/awr_plan_run.hip: run_list).

tests/golden/plan_snapshot.json was written by tools/plan_snapshot.py on that commit: the op lists, buckets and counts of fourteen plans at
B = 2, H = 128 (the smallest shape at which both networks fork in the forward and the Hourglass forks in the backward), and the bit patterns
of three deterministic training steps of both networks, single-process and as a one-rank data-parallel engine with four buckets."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# run_list's rule before the op fields: a backward launch with one of these names (or name prefixes) was issued without first joining the
# side and branch streams; every other launch, and the __bucket__ marker, joined
NO_JOIN_PREFIXES = ("awr_conv_", "awr_stem_")
NO_JOIN_NAMES = ("awr_bn_bwd_reduce", "awr_bn_bwd_apply", "awr_bn_bwd_finalize", "awr_maxpool_bwd", "awr_upsample2_bwd", "awr_add")


def name_rule_joins(name):
    return not (name.startswith(NO_JOIN_PREFIXES) or name in NO_JOIN_NAMES)


@pytest.fixture(scope="module")
def snap():
    spec = importlib.util.spec_from_file_location("awr_plan_snapshot", os.path.join(REPO, "tools", "plan_snapshot.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "plan_snapshot.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def built(snap):
    """Every covered plan built once by the current library: {record name: (record, forward flags, backward flags)}."""
    out, nets = {}, {}
    for case in snap.PLAN_CASES:
        net = nets.get(case[1])
        if net is None:
            net = nets[case[1]] = snap.make_net(case[1])
        plan = snap.build_plan(net, case)
        out[case[0]] = (snap.plan_record(plan), snap.op_flags(plan, 0), snap.op_flags(plan, 1))
        net.release_plan(plan)
    return out


def test_plans_equal_the_snapshot(snap, golden, built):
    assert golden["shape"] == {"B": snap.B, "H": snap.H, "J": snap.J}
    assert sorted(golden["plans"]) == sorted(c[0] for c in snap.PLAN_CASES) and len(snap.PLAN_CASES) == 14
    for name, (rec, _, _) in built.items():
        want = golden["plans"][name]
        for lst in ("fwd", "bwd"):
            assert snap.same_ops(want[lst], [tuple(o) for o in rec[lst]]), (name, lst)
        for field in ("buckets", "n_gemm", "n_bn", "n_winograd", "bytes"):
            assert rec[field] == want[field], (name, field)
        assert set(rec) == set(want)


def test_schedule_flags_restate_the_name_rule(snap, built):
    n_train = n_scatter = 0
    for name, (_, _, bwd) in built.items():
        if "/train/" not in name:
            assert not bwd
            continue
        n_train += 1
        for op, flags in bwd:
            assert bool(flags & 8) == name_rule_joins(op), (name, op, flags)
            assert bool(flags & 4) == (op == "awr_unpack_wgrads_batched"), (name, op, flags)
            n_scatter += bool(flags & 4)
        assert name_rule_joins("__bucket__") and any(op == "__bucket__" for op, _ in bwd) == ("/b4/" in name)
    assert n_train == 10 and n_scatter == 4 * 1 + 4 * 4 + 2


def test_deterministic_steps_are_bitwise_the_snapshot(snap, golden):
    assert sorted(golden["steps"]) == sorted(c[0] for c in snap.STEP_CASES) and len(snap.STEP_CASES) == 4
    got = snap.step_records()       # (deterministic mode inside try / finally; a one-rank process group for the data-parallel runs)
    for name, want in golden["steps"].items():
        assert len(want["loss_bits"]) == 9
        assert got[name]["loss_bits"] == want["loss_bits"], name
        assert got[name]["params_sha256"] == want["params_sha256"], name
