"""CPU: awr_amd.surface.joints_surface, the numpy statement of awr_joints_surface -- against the hand-written expectations of
tests/surface_cases.py and against its point-by-point loop on every case, the option refusals, the entry point's refusals (they come before
any HIP call), and the rule's claim on 96 procedural hands: true joints are never OFF, joints moved 40 mm sideways are, joints pushed 60 mm
deeper are OCCLUDED."""
import inspect
import re

import numpy as np
import pytest

import surface_cases as SC


@pytest.fixture(scope="module")
def SF():
    import awr_amd  # noqa: F401
    from awr_amd import surface
    return surface


def statement(SF, c):
    o = c["options"]
    if c["raw_bones"] is not None:          # indices outside [0, J): the rule below the wrappers' check
        return SF._statement(c["frames"], c["frame_idx"], c["uvd"], c["status"], c["ustatus"], c["raw_bones"], o["samples"], o["radius"], o["in_mm"],
                             o["out_mm"], o["min_on"])
    return SF.joints_surface(c["frames"], c["frame_idx"], c["uvd"], c["status"], c["ustatus"], **o)


def test_the_cases_cover_what_they_should():
    names = list(SC.cases())
    assert len(names) == len(set(names)) >= 40
    js = {c["uvd"].shape[1] for c in SC.cases().values()}
    assert {1, 14, 21, 100, 256} <= js
    assert {c["frames"].shape[1:] for c in SC.cases().values()} == set(SC.SHAPES)
    assert {c["options"]["radius"] for c in SC.cases().values()} == {0, 1, 2, 3} and {c["options"]["samples"] for c in SC.cases().values()} >= {1, 3, 7}
    assert any(c["raw_bones"] is not None and ((c["raw_bones"] < 0) | (c["raw_bones"] >= c["uvd"].shape[1])).any() for c in SC.cases().values())
    assert any(c["n_valid"] < len(c["uvd"]) for c in SC.cases().values())


@pytest.mark.parametrize("name", list(SC.cases()))
def test_statement_on_every_case(SF, name):
    c = SC.cases()[name]
    codes, gap, counts, row_status = statement(SF, c)
    n, J = c["uvd"].shape[:2]
    assert codes.shape == (n, J) and codes.dtype == np.int32 and gap.shape == (n, J) and gap.dtype == np.float32
    assert counts.shape == (n, 8) and counts.dtype == np.int32 and row_status.shape == (n,) and row_status.dtype == np.int32
    e = c["expect"]
    for (r, j), code in e.get("codes", {}).items():
        assert codes[r, j] == code, (r, j, code, codes[r, j])
    for (r, j), g in e.get("gap", {}).items():
        want = np.float32(np.nan if g is None else g)
        assert SC.bits(gap[r, j]) == SC.bits(want), (r, j, g, gap[r, j])
    for r, row in e.get("counts", {}).items():
        assert counts[r].tolist() == row, (r, row, counts[r])
    if "row_status" in e:
        assert row_status.tolist() == e["row_status"]
    # the rule read off point by point
    want = SC.reference(name)
    assert np.array_equal(codes, want[0]) and np.array_equal(SC.bits(gap), SC.bits(want[1]))
    assert np.array_equal(counts, want[2]) and np.array_equal(row_status, want[3])
    # what always holds: the counts are the codes', a skipped row has neither, every NaN is the one quiet NaN
    live = row_status == 0
    assert (codes[~live] == SF.SKIPPED).all() and not counts[~live].any() and (codes[live] != SF.SKIPPED).all()
    for k in (SF.ON, SF.OCCLUDED, SF.OFF, SF.OUTSIDE):
        assert np.array_equal(counts[live, k], (codes[live] == k).sum(1))
    assert (SC.bits(gap)[np.isnan(gap)] == 0x7FC00000).all() and np.isnan(gap[codes >= SF.OUTSIDE]).all()


def test_default_bones_are_the_skeletons(SF):
    from awr_amd import vis_tool
    assert SF.default_bones(14) == SC.NYU_BONES == [b for _, bones in vis_tool._SKELETON["nyu"] for b in bones]
    assert SF.default_bones(21) == SC.default_bones(21) == [b for _, bones in vis_tool._SKELETON["hands"] for b in bones] and len(SF.default_bones(21)) == 20
    assert SF.default_bones(16) == [] and SF.bone_table(None, 5).shape == (0, 2) and SF.bone_table(None, 14).dtype == np.int32
    assert SF.SURFACE_DEFAULTS == SC.DEFAULTS == dict(radius=1, in_mm=40.0, out_mm=15.0, min_on=1, bones=None, samples=3)
    assert (SF.ON, SF.OCCLUDED, SF.OFF, SF.OUTSIDE, SF.SKIPPED) == (0, 1, 2, 3, 4)


def test_option_refusals(SF):
    ok = SF.check_surface_option
    assert ok(None) is None and ok(True) == SF.SURFACE_DEFAULTS and ok({}) == SF.SURFACE_DEFAULTS
    assert ok(dict(radius=3, min_on=49, in_mm=0, out_mm=2, samples=7, bones=[(0, 1), [2, 3]])) == dict(radius=3, in_mm=0.0, out_mm=2.0, min_on=49,
                                                                                                     bones=[(0, 1), (2, 3)], samples=7)
    assert ok(dict(radius=0, bones=[])) == dict(SF.SURFACE_DEFAULTS, radius=0, bones=[])
    for bad, exc, word in ((False, TypeError, "surface is None, True or a dict"), ("on", TypeError, "surface is"), (dict(window=3), ValueError, "unknown keys"),
                           (dict(radius=4), ValueError, "radius = 4"), (dict(radius=-1), ValueError, "radius = -1"), (dict(radius=1.0), TypeError, "radius is an int"),
                           (dict(radius=True), TypeError, "radius"), (dict(in_mm=-1), ValueError, "in_mm = -1"), (dict(in_mm=float("inf")), ValueError, "in_mm"),
                           (dict(out_mm=float("nan")), ValueError, "out_mm"), (dict(out_mm="15"), TypeError, "out_mm"), (dict(min_on=0), ValueError, "min_on = 0"),
                           (dict(min_on=10), ValueError, r"min_on = 10 is outside \[1, 9\]"), (dict(radius=0, min_on=2), ValueError, "min_on = 2"),
                           (dict(samples=0), ValueError, "samples = 0"), (dict(samples=8), ValueError, "samples = 8"), (dict(samples=2.0), TypeError, "samples"),
                           (dict(bones=[(0, 1)] * 65), ValueError, "65 pairs"), (dict(bones=[(0, 1, 2)]), TypeError, "pair"), (dict(bones=[(0, 1.5)]), TypeError, "index"),
                           (dict(bones="nyu"), TypeError, "bones is None or a sequence"), (dict(bones=3), TypeError, "bones")):
        with pytest.raises(exc, match=word):
            ok(bad)
    # an index outside [0, J) is refused where J is known
    for bones in ([(0, 14)], [(-1, 3)]):
        with pytest.raises(ValueError, match=r"outside \[0, J = 14\)"):
            SF.bone_table(bones, 14)
    c = SC.cases()["48x64_rounding"]
    with pytest.raises(ValueError, match="outside"):
        SF.joints_surface(c["frames"], c["frame_idx"], c["uvd"], c["status"], c["ustatus"], bones=[(0, 99)])
    with pytest.raises(ValueError, match="uint16"):
        SF.joints_surface(c["frames"].astype(np.int32), c["frame_idx"], c["uvd"], c["status"], c["ustatus"])
    with pytest.raises(ValueError, match="float32"):
        SF.joints_surface(c["frames"], c["frame_idx"], c["uvd"].astype(np.float64), c["status"], c["ustatus"])


def test_entry_point_refusals_come_before_any_launch(SF):
    """argument checks run before any HIP call, so a machine without a GPU sees them"""
    from awr_amd import _lib as L
    good = dict(ftype=0, n_frames=2, fh=48, fw=64, n=3, J=14, n_valid=3, n_bones=0, samples=3, radius=1, in_mm=40.0, out_mm=15.0, min_on=1)

    def call(**kw):
        a = dict(good, **kw)
        p = 16          # (never dereferenced: every call below is refused)
        return L.lib.awr_joints_surface(a.get("frames", p), a["ftype"], a["n_frames"], a["fh"], a["fw"], p, p, p, p, a["n"], a["J"], a["n_valid"], a.get("bones"),
                                        a["n_bones"], a["samples"], a["radius"], a["in_mm"], a["out_mm"], a["min_on"], p, p, p, a.get("row_status", p), None)
    for kw, word in ((dict(ftype=1), "uint16"), (dict(n=0), "B = 0"), (dict(n_frames=0), "n_frames = 0"), (dict(fw=0), "48 x 0"), (dict(fh=16385), "16385"),
                     (dict(J=0), "J = 0"), (dict(J=257), r"J = 257 is outside \[1, 256\]"), (dict(n_valid=4), "n_valid = 4"), (dict(n_valid=-1), "n_valid = -1"),
                     (dict(radius=4), "radius = 4"), (dict(radius=-1), "radius = -1"), (dict(in_mm=-0.5), "in_mm = -0.5"), (dict(in_mm=float("nan")), "in_mm"),
                     (dict(in_mm=float("inf")), "in_mm = inf"), (dict(out_mm=-1.0), "out_mm = -1"), (dict(out_mm=float("inf")), "out_mm"),
                     (dict(min_on=0), "min_on = 0"), (dict(min_on=10), r"min_on = 10 is outside \[1, 9\]"), (dict(radius=0, min_on=2), "min_on = 2"),
                     (dict(n_bones=65, bones=16), "n_bones = 65"), (dict(n_bones=-1), "n_bones = -1"), (dict(n_bones=2), "n_bones = 2 needs the bone table"),
                     (dict(samples=0), "samples = 0"), (dict(samples=8), "samples = 8"), (dict(frames=None), "NULL pointer"), (dict(row_status=None), "NULL pointer"),
                     (dict(frames=17), "misaligned")):
        assert call(**kw) == -1, kw
        assert re.search("awr_joints_surface.*" + word, L.last_error()), (kw, L.last_error())
    assert "awr_joints_surface" in L.EXPORTS and not L.MISSING


# ---- 96 procedural hands: the rule separates right from wrong ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hands():
    import awr_amd  # noqa: F401
    from awr_amd import evaluator, nyu_data, synth
    poses = synth.sample_poses(96, 7)
    joints21, prims, bbox = synth.forward_kinematics(poses)
    frames = synth.render(prims, bbox)
    lab = synth.labels(joints21, 14)[0]

    def uvd(moved):
        return evaluator.xyz2uvd((lab + np.asarray(moved, np.float64)).astype(np.float32), nyu_data.PARAS, -1)
    return frames, uvd


def test_true_and_displaced_joints_on_procedural_hands(SF, hands):
    frames, uvd = hands
    idx, zero = np.arange(96), np.zeros(96, np.int32)
    o = dict(radius=1, in_mm=40, out_mm=15, min_on=1)
    codes, gap, counts, row_status = SF.joints_surface(frames, idx, uvd((0, 0, 0)), zero, zero, **o)
    assert not row_status.any() and codes.shape == (96, 14)
    assert (counts[:, SF.OFF] == 0).all() and (counts[:, SF.OUTSIDE] == 0).all()                  # true joints: 0 OFF and 0 OUTSIDE
    assert (codes == SF.ON).mean() > 0.9 and np.isfinite(gap).all() and (gap[codes == SF.ON] >= -15).all() and (gap[codes == SF.ON] <= 40).all()
    counts = SF.joints_surface(frames, idx, uvd((40, 0, 0)), zero, zero, **o)[2]
    assert (counts[:, SF.OFF] >= 3).all(), counts[:, SF.OFF].min()                                # + 40 mm in x: at least 3 OFF joints in every frame
    codes = SF.joints_surface(frames, idx, uvd((0, 0, 60)), zero, zero, **o)[0]
    assert (codes == SF.OCCLUDED).sum() > (codes == SF.ON).sum()                                  # + 60 mm in z: more OCCLUDED than ON


def test_predictor_surface_defaults_to_none():
    import awr_amd
    from awr_amd import predictor
    p = inspect.signature(awr_amd.Predictor.__init__).parameters
    assert p["surface"].default is None and list(p)[-1] == "surface"
    assert predictor.Predictor.surface is None
