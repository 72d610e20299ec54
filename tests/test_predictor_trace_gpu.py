"""GPU: what Predictor.predict launches, configuration by configuration, against tests/golden/predictor_trace.json -- the launches of the
commit BEFORE predict() became one pipeline of stage methods, recorded there by tools/predictor_trace.py on an MI355X and
never regenerated from a later predictor.  Names, order and every small int / float argument (row counts, strides, the camera, thresholds)
of the predictor's own entry points; the names alone of the engine's and the renderer's."""
import json
import os
import sys

import pytest
import torch

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import predictor_trace as PT  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net():
    assert torch.cuda.is_available()
    return PT.network()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "predictor_trace.json")) as f:
        return json.load(f)


def test_the_golden_has_every_configuration(golden):
    assert sorted(golden) == sorted(PT.CONFIGS) and all(len(calls) == 3 for calls in golden.values())
    named = {c[0] for calls in golden.values() for call in calls for c in call}
    assert named >= set(PT.STAGES), sorted(set(PT.STAGES) - named)


@pytest.mark.parametrize("name", list(PT.CONFIGS))
def test_launches_equal_the_recorded_ones(net, golden, name):
    got, _ = PT.trace(name, net)
    for i, (g, w) in enumerate(zip(got, golden[name])):
        assert len(g) == len(w), (name, i, [c[0] for c in g], [c[0] for c in w])
        for j, (a, b) in enumerate(zip(g, w)):
            assert a == b, (name, "call %d, launch %d" % (i, j), a, b)
    assert got == golden[name]
