"""What the plan builder builds, pinned to the commit before it was split into translation units (csrc/awr_plan_build.hip: Builder, NetBuilder).

tests/golden/plan_snapshot_wide.json was written by `tools/plan_snapshot.py --wide` on that commit and is never regenerated from a later builder:
27 plans at B = 2, H = 128, J = 14 that reach the launch forms tests/golden/plan_snapshot.json does not -- the ResNet-50 bottlenecks, the second
Hourglass stack, downsample 1 and 4, Winograd "full" / "forward+wgrad" / "forward", fused pairs and dual launches (with and without the dual form,
with and without the max-pool inside the GEMM launch), the deterministic per-split copies, training split-K and blocked accumulation -- each with
every op's name, all four flag bits of awr_plan_op and MACs, the awr_plan_gemm listing, the buckets, the awr_plan_tensor listing, the counts and
the bytes (each list as its length and SHA-256: to see where two builds part, compare their snap.wide_plan_records()); and the bit patterns of
three deterministic training steps of ResNet-50 and Hourglass-2, single-process and as a one-rank data-parallel engine with four buckets."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PLANS = 27


@pytest.fixture(scope="module")
def snap():
    spec = importlib.util.spec_from_file_location("awr_plan_snapshot", os.path.join(REPO, "tools", "plan_snapshot.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "plan_snapshot_wide.json")) as f:
        return json.load(f)


def test_wide_plans_equal_the_record(snap, golden):
    assert golden["shape"] == {"B": snap.B, "H": snap.H, "J": snap.J}
    assert sorted(golden["plans"]) == sorted(c["name"] for c in snap.WIDE_PLAN_CASES) and len(snap.WIDE_PLAN_CASES) == N_PLANS
    built = snap.wide_plan_records()      # (one plan alive at a time; environment and deterministic mode restored per case)
    for name, want in golden["plans"].items():
        got = built[name]
        assert set(got) == set(want), name
        for field in want:
            have = snap.list_digest(got[field]) if field in snap.WIDE_LISTS else got[field]      # (the file holds a list as its length and SHA-256)
            assert have == want[field], (name, field)


def test_wide_deterministic_steps_are_bitwise_the_record(snap, golden):
    assert sorted(golden["steps"]) == sorted(c[0] for c in snap.WIDE_STEP_CASES) and len(snap.WIDE_STEP_CASES) == 4
    got = snap.step_records(snap.WIDE_STEP_CASES)
    for name, want in golden["steps"].items():
        assert len(want["loss_bits"]) == 9
        assert got[name]["loss_bits"] == want["loss_bits"], name
        assert got[name]["params_sha256"] == want["params_sha256"], name
