"""GPU: what TrainEngine and InferEngine hand to the library, configuration by configuration, against tests/golden/engine_trace.json -- the
calls of the commit BEFORE the engines moved out of trainer.py onto one base class and one set of head launches, recorded
there by tools/engine_trace.py on an MI355X and never regenerated from a later engine.  Entry-point names, their order, and every bool,
small int, float (as hex) and NULL argument, from the engine's construction to its last step or call."""
import json
import os
import sys

import pytest
import torch

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import engine_trace as ET  # noqa: E402

pytestmark = pytest.mark.gpu
HEAD = ("awr_head_forward", "awr_head_forward_nhwc", "awr_head_loss_step_nhwc", "awr_dense_loss", "awr_huber", "awr_head_backward",
        "awr_head_eval_nhwc", "awr_head_confidence", "awr_head_confidence_nhwc")


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "engine_trace.json")) as f:
        return json.load(f)


def test_the_golden_has_every_configuration(golden):
    assert list(golden) == ET.CONFIGS
    named = {c[0] for calls in golden.values() for c in calls}
    assert named >= set(HEAD), sorted(set(HEAD) - named)


@pytest.mark.parametrize("name", ET.CONFIGS)
def test_calls_equal_the_recorded_ones(golden, name):
    assert torch.cuda.is_available()
    got, _ = ET.trace(name)
    want = golden[name]
    assert [c[0] for c in got] == [c[0] for c in want]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (name, "call %d" % i, a, b)
