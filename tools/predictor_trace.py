"""What Predictor.predict launches, configuration by configuration -> tests/golden/predictor_trace.json (and, with --bits, what it returns)

    python tools/predictor_trace.py [--table options | newer | both] [--out FILE] [--bits FILE] [--config NAME ...]

The golden file is recorded ONCE, at the commit before predict() became one pipeline of stages, and never regenerated from a later
predictor: tests/test_predictor_trace_gpu.py asserts that every configuration still issues the same launches, in the same order, with the
same sizes.  The tool uses the public API only, so it runs unchanged in a checkout of any commit that has the options it names.

Two tables, two golden files (TABLES).  CONFIGS -> predictor_trace.json is the one above and stays as it was recorded.  NEWER ->
predictor_trace_newer.json holds the options that came after it (isolate=, edge_mm=, denoise=), recorded ONCE at the commit before the
detector's launches moved into detect_calls.py, and never regenerated either.  STAGES names the three entry points of those options too;
no configuration of the first table issues them, so its trace is what it was.

Recording (the trick of test_hands_1_is_todays_path): awr_amd._lib.call is replaced by a recorder.  For the predictor's own entry points
(STAGES) it keeps the name and those positional arguments that are int or float, not bool, with abs(x) < 2**20 -- row counts, strides,
the camera, thresholds; pointers fall out by their size.  For every other entry point (the engine's, the renderer's) it keeps the name
only, so that the golden does not depend on plan build modes.

Fixture: ResNet-18 with procedural weights, J = 14, img_size 64, 120 x 160 frames of two hand-sized blobs, max_batch = 2.  Per configuration
one predictor; one warm-up call (an engine's first call also uploads its weights), then three recorded calls: nb = 2; nb = 2 with
n_valid = 1 (the padding paths); explicit centers_uvd.

--bits FILE additionally writes, per configuration and call, the SHA-256 of the bytes (after one synchronise) of every field of the returned
tuple and of every documented after-call attribute.  Two commits compute the same bits when their files are identical.  Rows of the
batch axis at and past n_valid are documented as unspecified and are left out of the hashes of the n_valid call.  An engine's default plan
picks its GEMM tiles by TIMING them, so two processes of one commit may sum in different orders and differ in the last bits of the joints;
--bits therefore switches awr_amd.set_deterministic on before it builds anything (the predictor's own launches do not depend on it, the
engine's may: record the golden trace without --bits)."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (REPO, os.path.join(REPO, "oracle")) if p not in sys.path]

STAGES = ("awr_detect", "awr_detect_palm", "awr_detect_hands", "awr_detect_samples", "awr_joints_unproject", "awr_joints_center",
          "awr_joints_filter", "awr_confidence_fields", "awr_centers_select", "awr_hands_assign", "awr_view_centers", "awr_view_rotate",
          "awr_views_fuse", "awr_hands_isolate", "awr_detect_hands_edge", "awr_frames_denoise")
S, J, B = 64, 14, 2
EH, EW = 120, 160
SMALL = dict(cube=(300.0, 300.0, 300.0), paras=(147.0, 146.8, 80.0, 60.0), flip=-1, frame_shape=(EH, EW), depth_range=(200.0, 1200.0), slab=100.0,
             refine_iters=2)
VIEWS = [dict(rot=0.0), dict(rot=-15.0), dict(rot=15.0)]          # the identity and two rotations
CONFIGS = {
    "defaults": dict(),
    "confidence": dict(confidence=True),
    "recenter2": dict(recenter=2),
    "track": dict(track=True),
    "track_palm_recenter1": dict(track=True, palm=True, recenter=1),
    "smooth": dict(smooth=True),
    "smooth_lead_track": dict(smooth=dict(lead=True), track=True),
    "smooth_conf": dict(smooth=dict(weight="conf")),
    "views_mean": dict(views=VIEWS, fuse="mean"),
    "views_conf_confidence": dict(views=VIEWS, fuse="conf", confidence=True),
    "views_track_smooth": dict(views=VIEWS, track=True, smooth=True),
    "hands2": dict(hands=2),
    "hands2_palm_recenter1_confidence": dict(hands=2, palm=True, recenter=1, confidence=True),
    "hands2_identity": dict(hands=2, identity=True),
    "hands2_identity_full": dict(hands=2, identity=True, track=True, smooth=dict(lead=True), recenter=1, palm=True, confidence=True),
    "hands3_identity_smooth_conf": dict(hands=3, identity=True, smooth=dict(weight="conf")),
}
# the options behind the first golden file, over the same fixture
NEWER = {
    "isolate": dict(hands=2, isolate=True),
    "isolate_identity_track": dict(hands=2, isolate=True, identity=True, track=True),
    "edge": dict(hands=2, edge_mm=40.0),
    "edge_isolate_palm_recenter1": dict(hands=2, edge_mm=40.0, isolate=True, palm=True, recenter=1),
    "denoise": dict(denoise=True),
    "denoise_fill_views": dict(denoise=dict(radius=2, edge=None, support=2, fill=3), views=VIEWS),
    "denoise_identity_full": dict(denoise=True, hands=2, identity=True, track=True, smooth=dict(lead=True), recenter=1, palm=True, confidence=True),
    "denoise_edge_isolate": dict(denoise=dict(edge=25.0), hands=2, edge_mm=40.0, isolate=True),
}
TABLES = {"options": (CONFIGS, "predictor_trace.json"), "newer": (NEWER, "predictor_trace_newer.json")}
# the documented after-call attributes and the axis of each that is the batch
ATTRS = dict(centers_uvd=0, next_centers_uvd=0, recenter_codes=1, raw_xyz=0, raw_uvd=0, ahead_xyz=0, filter_codes=0, hand_info=0, hand_codes=0,
             hand_source=0, hands_dropped=0, palm_info=0, isolated=0, raw_frames=0, denoise_status=0)


def blobs(*hands):
    """one 120 x 160 frame: a far plane and, per (u, v, z), a hand-sized blob of 41 x 41 pixels at z ... z + 4 mm"""
    f = np.full((EH, EW), 1400, np.uint16)
    vv, uu = np.mgrid[0:EH, 0:EW]
    for cu, cv, z in hands:
        m = (np.abs(uu - cu) <= 20) & (np.abs(vv - cv) <= 20)
        f[m] = (z + (uu[m] + vv[m]) % 5).astype(np.uint16)
    return f


# the frames of the warm-up call, and of the recorded calls: the same two hands a few pixels and millimetres on
WARM = np.stack([blobs((45, 60, 600), (115, 60, 650)), blobs((50, 40, 700), (112, 85, 640))])
FRAMES = np.stack([blobs((47, 61, 604), (113, 60, 652)), blobs((51, 42, 698), (111, 84, 644))])
CENTERS = np.array([[[47.0, 61.0, 606.0], [113.0, 60.0, 654.0], [np.nan] * 3], [[51.0, 42.0, 700.0], [111.0, 84.0, 646.0], [np.nan] * 3]])


def network():
    import awr_amd
    import awr_oracle as O
    net = awr_amd.get_deconv_net(18, J, 2)
    net.load_state_dict(O.procedural_state(O.manifest_for("resnet_18", J), seed=5), strict=True)
    return net.cuda().eval()


def digest(t, nv, axis):
    """SHA-256 of the bytes of rows [0, nv) of t's batch axis"""
    t = t.narrow(axis, 0, nv).contiguous().cpu()
    return "%s %s %s" % (str(t.dtype), list(t.shape), hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest())


def bits_of(pred, out, nv):
    torch.cuda.synchronize()
    bits = {"type": type(out).__name__}
    for name, value in zip(out._fields, out):
        bits[name] = digest(value, nv, 0)
    for name, axis in ATTRS.items():
        value = getattr(pred, name, None)
        if value is not None:
            bits[name] = digest(value, nv, axis)
    if getattr(pred, "view_outputs", None) is not None:
        for name, value in sorted(vars(pred.view_outputs).items()):
            bits["view_outputs." + name] = digest(value, nv, 1)
    return bits


def trace(name, net, bits=False):
    """-> (the three recorded calls' launches, their bits or None) of configuration `name`"""
    import awr_amd
    from awr_amd import _lib as L
    kw = CONFIGS[name] if name in CONFIGS else NEWER[name]
    K = kw.get("hands", 1)
    pred = awr_amd.Predictor(net, S, 1.0, max_batch=B, **SMALL, **kw)
    centers = CENTERS[:, :K] if K > 1 else CENTERS[:, 0]
    pred.predict(WARM)
    calls, real, launches, hashes = [], L.call, [], []

    def recorder(entry, *args):
        if entry in STAGES:
            calls.append([entry] + [x for x in args if isinstance(x, (int, float)) and not isinstance(x, bool) and abs(x) < 1 << 20])
        else:
            calls.append([entry])
        return real(entry, *args)
    L.call = recorder
    try:
        for nv, extra in ((B, dict()), (1, dict(n_valid=1)), (B, dict(centers_uvd=centers))):
            del calls[:]
            out = pred.predict(FRAMES, **extra)
            launches.append(list(calls))
            if bits:
                hashes.append(bits_of(pred, out, nv))
    finally:
        L.call = real
    torch.cuda.synchronize()
    return launches, hashes if bits else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default="options", choices=list(TABLES) + ["both"], help="both: one file over both tables, for --bits (pass --out)")
    ap.add_argument("--out", default=None, help="default: the table's golden file under tests/golden/")
    ap.add_argument("--bits", default=None, help="also write the SHA-256 of every returned field and after-call attribute to this file")
    ap.add_argument("--config", nargs="*", default=None, help="default: every configuration of the table")
    a = ap.parse_args()
    if a.table == "both" and a.out is None:
        raise SystemExit("--table both writes no golden file: pass --out")
    if a.out is None:
        a.out = os.path.join(REPO, "tests", "golden", TABLES[a.table][1])
    if a.config is None:
        a.config = [name for t in (TABLES if a.table == "both" else [a.table]) for name in TABLES[t][0]]
    if not torch.cuda.is_available():
        raise SystemExit("tools/predictor_trace.py needs a GPU: nothing is launched without one")
    if a.bits is not None:
        import awr_amd
        awr_amd.set_deterministic(True)
    net = network()
    launches, hashes = {}, {}
    for name in a.config:
        launches[name], hashes[name] = trace(name, net, a.bits is not None)
        print("%-36s %s launches per call" % (name, [len(c) for c in launches[name]]), flush=True)
    for path, what in ((a.out, launches), (a.bits, hashes)):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in what.items()) + "\n}\n")
            print("%s  sha256 %s" % (path, hashlib.sha256(open(path, "rb").read()).hexdigest()))


if __name__ == "__main__":
    main()
