"""GPU: what Predictor.predict launches, configuration by configuration, against tests/golden/predictor_trace.json -- the launches of the
commit BEFORE predict() became one pipeline of stage methods, recorded there by tools/predictor_trace.py on an MI355X and
never regenerated from a later predictor.  Names, order and every small int / float argument (row counts, strides, the camera, thresholds)
of the predictor's own entry points; the names alone of the engine's and the renderer's.  The options that came after it (isolate=,
edge_mm=, denoise=: PT.NEWER) are held to tests/golden/predictor_trace_newer.json in the same way, recorded at the commit before the
detector's launches moved into detect_calls.py."""
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


def _golden(golden_dir, table):
    with open(os.path.join(golden_dir, PT.TABLES[table][1])) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return _golden(golden_dir, "options")


@pytest.fixture(scope="module")
def golden_newer(golden_dir):
    return _golden(golden_dir, "newer")


def test_the_golden_has_every_configuration(golden, golden_newer):
    for g, configs in ((golden, PT.CONFIGS), (golden_newer, PT.NEWER)):
        assert sorted(g) == sorted(configs) and all(len(calls) == 3 for calls in g.values())
    assert not set(PT.CONFIGS) & set(PT.NEWER)
    named = {c[0] for g in (golden, golden_newer) for calls in g.values() for call in calls for c in call}
    assert named >= set(PT.STAGES), sorted(set(PT.STAGES) - named)


def _compare(name, net, want):
    got, _ = PT.trace(name, net)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (name, i, [c[0] for c in g], [c[0] for c in w])
        for j, (a, b) in enumerate(zip(g, w)):
            assert a == b, (name, "call %d, launch %d" % (i, j), a, b)
    assert got == want


@pytest.mark.parametrize("name", list(PT.CONFIGS))
def test_launches_equal_the_recorded_ones(net, golden, name):
    _compare(name, net, golden[name])


@pytest.mark.parametrize("name", list(PT.NEWER))
def test_newer_launches_equal_the_recorded_ones(net, golden_newer, name):
    _compare(name, net, golden_newer[name])
