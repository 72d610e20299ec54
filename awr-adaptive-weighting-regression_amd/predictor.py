"""Predict hand joints from raw depth frames: no dataset index, no refined-centre file, no labels.

    pred = Predictor(net, img_size=128, kernel_size=0.4, max_batch=64)
    out = pred.predict(frames)              # (B, 480, 640) uint16 millimetres: numpy, host tensor or device tensor
    out.xyz, out.uvd                        # (B, J, 3) camera millimetres / original-image uvd, on the device
    pred.check()                            # synchronises; raises AwrError naming the first frame that could not be predicted
    Predictor(..., confidence=True)         # out additionally carries conf, peak, spread_mm (B, J): how sure each joint is
    Predictor(..., recenter=1)              # crop again around the predicted joints and predict again
    Predictor(..., track=True)              # start each call's crop at the previous call's joint centre of the same batch slot
    Predictor(..., views=make_views(rot=(-15, 15)), fuse="mean")      # the same hand under several views in ONE pass, fused
    Predictor(..., palm=True)               # move the detector's centre to the palm disc, away from the forearm
    Predictor(..., smooth=True)             # filter the joints over time: One-Euro per joint, gate, coasting, look-ahead
    Predictor(..., hands=2)                 # up to K hands per frame from connected components; the outputs gain a hand axis
    Predictor(..., hands=2, identity=True)  # slot k is the same hand from call to call; track, smooth and lead work per hand

Everything between the frames and the joints runs on the device, on the current stream, without a synchronisation: awr_detect (hand
centre by iterated centre of mass) -> awr_detect_samples (crop blocks, crop matrices) -> awr_nyu_batch (crop + normalise) -> the
inference plan and the single-pass head (InferEngine) -> awr_joints_unproject.  The host only issues launches.  There is no host
fallback in this class: without a GPU it raises; `awr_amd.detect.detect` is the numpy statement of the detector for such a machine.

Re-centring and tracking (both opt-in; with the defaults the launches and the bits are what they were).  The detector's centre is a centre
of mass of depth pixels, biased towards the forearm and whatever else lies in the slab, while the network was trained on refined centres.
The network's own joints are the better centre, and awr_joints_center turns them into one on the device: the float64 mean of the (selected)
joints, projected back to uvd, accepted only where the frame has no status code, the mean is finite, its depth lies in the detector's
depth_range and it is within max_shift half cubes of the present centre on every axis.  recenter=N appends N passes of awr_joints_center ->
awr_detect_samples -> render -> engine -> awr_joints_unproject on the same engine and buffers; a frame that is not moved keeps its centre
and so repeats its previous pass bit for bit.  track=True keeps one float64 centre per batch slot (NaN: lost) and runs the detector twice,
seeded with the tracked centres and as configured, and awr_centers_select takes the tracked result where it found the hand.  Nothing of this
synchronises.  Whether either improves accuracy on real frames is UNMEASURED: no NYU frames and no trained checkpoint exist where this was
written.

Views (opt-in; views=None issues the launches and gives the bits it always did).  Test-time ensembling over the three augmentations the
network was trained with (loader.py:75-86): in-plane rotations, cube scales and shifts of the crop centre.  The plan holds max_batch x V
images, view-major (view v of batch slot b is row v * max_batch + b, so view 0 sits where a plain predictor's rows do).  awr_view_centers
expands the centres, the unchanged awr_detect_samples builds V * max_batch blocks with a cube per row, awr_view_rotate turns the rotating
views' blocks into AWR_NYU_AFFINE ones and their crop matrices into M_v = R . M; the renderer, the engine and awr_joints_unproject then run
once over all rows -- un-projection inverts whatever matrix it is given, so a rotated view needs no arithmetic of its own -- and
awr_views_fuse fuses the views' camera-space joints per frame and joint.  Whether fusing views lowers the joint error on real frames is
UNMEASURED too, for the same reason.

Palm centre (opt-in; palm=False issues the launches and gives the bits it always did).  The detector's centre of mass is dragged up a
forearm that lies at the hand's depth, and no later pass repairs a first crop that misses the hand.  palm=True sends the configured
detector's centres through awr_detect_palm (nine small launches, a frame split over several workgroups: the exact integer distance transform of the silhouette in a
window of palm_search cubes, its medial set, the end of it with the fingers beyond, the palm disc's centre of mass) before
awr_detect_samples.  With track=True only the detector branch is refined, before awr_centers_select: a tracked centre is the joints' own.
With centers_uvd handed to predict() it does not apply.  Measured on procedural hands only (profiles/synth_accuracy.txt); behaviour on real
depth frames -- sleeves, a body within the search depth, NYU -- is UNMEASURED.

Temporal filter (opt-in; smooth=None issues the launches and gives the bits it always did).  smooth=True | dict | track.OneEuro puts ONE
awr_joints_filter launch behind the final pass (with views: behind awr_views_fuse): per batch slot, joint and axis a One-Euro low-pass
in camera millimetres whose state (six doubles and two ints per joint) lives on the device from call to call; a measurement outside
gate_mm, a frame that is not OK or a non-finite joint is answered with the held joint for up to max_coast calls, then the track restarts
at the measurement or is dropped.  predict() returns the filtered joints; raw_xyz / raw_uvd / ahead_xyz / filter_codes hold the rest.
lead=True hands the tracker the look-ahead joints x + d dt for the next call's crop.  The statement is awr_amd.track.filter_step; the
kernel equals it bit for bit.  Measured on procedural sequences only (profiles/track_accuracy.txt, profiles/predict_smooth.txt); the
defaults are engineering choices and accuracy on real frames is UNMEASURED.

Several hands (opt-in; hands=1 issues the launches and gives the bits it always did).  The "nearest" seed is the centre of mass of every
pixel within the slab of the nearest one: with two hands in view it lies between them, and one hand at most is reported.  hands=K >= 2
puts awr_detect_hands (nine small launches: the near foreground's 4-connected components by a union-find forest with integer atomicMin,
canonical labels, the K nearest components of at least min_pixels pixels seeded with their own slab's centre of mass) in front of the
unchanged awr_detect, which refines all K * max_batch hand-major seeds as given centres; the crop, the network, the un-projection, the
re-centring passes, the confidence fields and the palm pass then run per row, as the views' rows do.  Touching or overlapping hands are
ONE component and count as one hand; which hand of one call is which hand of the next is not decided here, so views, track and smooth
are refused with hands >= 2 (identity=..., below, decides it and lifts the refusal for track and smooth).  Measured on procedural two-hand composites only (profiles/detect_hands.txt); reach and min_pixels are
engineering defaults, UNMEASURED on real frames.

Hand identities (opt-in; identity=None issues the launches, gives the bits and raises the errors it always did).  With hands=K >= 2 and
identity=True | dict | track.Identity, ONE awr_hands_assign launch between the detector and the crop decides which of this call's
detected hands (the candidates) is which identity of the previous call: an exact assignment over the K! permutations in camera
millimetres, gated by gate_mm, per batch slot, with state (last centre, id, misses, next id) that stays on the device.  Slot k then is
the same hand from call to call -- a hand without a candidate waits for max_miss calls (status EMPTY, NaN rows) before its slot is given
up, a new hand takes the lowest free slot and a fresh id -- and so track=True (a second awr_detect seeded with every slot's last centre;
two trackers that end on one hand are merged), smooth=... (K launches of the unchanged awr_joints_filter over the hand-major filter
state, whose rows awr_hands_assign zeroes where an identity starts or ends) and lead=True are accepted.  predict() returns a
TrackedHandsPrediction with ids (nb, K).  The statement is awr_amd.track.assign_step; the kernel equals it bit for bit.  Measured on
procedural two-hand sequences only (profiles/hands_identity.txt); gate_mm, merge_mm and max_miss are engineering defaults, UNMEASURED on
real frames.
"""
import collections
import types

import numpy as np
import torch

from . import _lib as L
from . import detect as D
from . import nyu_data as ND
from . import track as T

Prediction = collections.namedtuple("Prediction", "xyz uvd center_xyz M status")
ConfidentPrediction = collections.namedtuple("ConfidentPrediction", Prediction._fields + ("conf", "peak", "spread_mm"))
ViewPrediction = collections.namedtuple("ViewPrediction", Prediction._fields + ("view_spread_mm", "views_used"))
ConfidentViewPrediction = collections.namedtuple("ConfidentViewPrediction", ConfidentPrediction._fields + ("view_spread_mm", "views_used"))
HandsPrediction = collections.namedtuple("HandsPrediction", Prediction._fields + ("n_hands",))
ConfidentHandsPrediction = collections.namedtuple("ConfidentHandsPrediction", HandsPrediction._fields + ("conf", "peak", "spread_mm"))
TrackedHandsPrediction = collections.namedtuple("TrackedHandsPrediction", HandsPrediction._fields + ("ids",))
ConfidentTrackedHandsPrediction = collections.namedtuple("ConfidentTrackedHandsPrediction", TrackedHandsPrediction._fields + ("conf", "peak", "spread_mm"))
MAX_RECENTER = 4
MAX_VIEWS = D.MAX_VIEWS


class Predictor:
    views, fuse, V = None, "mean", 1          # a predictor without views: one identity view, no view table, no per-view buffers
    smooth = None                             # a predictor without a temporal filter: no filter state, no launch, no extra attributes
    identity = None                           # a predictor without hand identities: no assignment state, no launch, no extra attributes

    def __init__(self, net, img_size, kernel_size, cube=(300, 300, 300), paras=ND.PARAS, flip=-1, max_batch=1, frame_shape=(480, 640),
                 seed="nearest", depth_range=D.DEPTH_RANGE, slab=D.SLAB, refine_iters=D.REFINE_ITERS, winograd=None, parity=False, confidence=False,
                 recenter=0, track=False, center_joints=None, max_shift=1.0, views=None, fuse="mean", palm=False, palm_search=D.PALM_SEARCH,
                 smooth=None, hands=1, reach=D.REACH, min_pixels=D.MIN_PIXELS, identity=None):
        """net: an awr_amd network on the GPU with its weights loaded.  cube: the crop cube in mm.  paras = (fx, fy, u0, v0), flip: the camera.
        max_batch: the static batch of the inference plan; smaller batches are padded, larger ones refused.  seed / depth_range / slab /
        refine_iters: the detector (awr_amd.detect); with `centers_uvd` handed to predict() the seed is the given centre and refine_iters
        still applies -- refine_iters=0 takes centres as they are, the dataset's behaviour.  winograd / parity: InferEngine's.
        confidence: False -- predict() returns the five-field Prediction | True -- a ConfidentPrediction, the same five fields and per joint
        conf (the expected closeness under the head's aggregation weights, in [0, 1] for a trained map), peak (the largest masked heat value)
        and spread_mm = sqrt(var_u (cube_x / 2)^2 + var_v (cube_y / 2)^2 + var_d (cube_z / 2)^2), the scatter of the per-pixel votes about the
        joint in NOMINAL millimetres: the crop maps the cube onto [-1, 1] by construction, so half a cube edge is one normalised unit (exact
        in depth, and in the image plane as far as the crop's pinhole scaling is).  One more pass over the dense map and one small launch.
        recenter: 0 ... 4 extra passes, each cropped around the joints of the pass before it (awr_joints_center's gate decides per frame).
        track: True -- a call without centers_uvd first tries the centre the previous call's joints left for the same batch slot (refined
        by refine_iters passes, which is also what validates it against the new frame: with refine_iters=0 a tracked centre is NEVER
        re-validated against the frame and is only dropped when the gate or a status code drops it) and falls back to the configured
        detector per slot; the second detector run is the price of never synchronising.  center_joints: indices into [0, J) whose mean is
        the centre (default: all joints), uploaded once.  max_shift: the gate, in half cubes per axis, of both modes; the gate's depth range
        is depth_range.  After a predict() with recenter > 0 or track on: centers_uvd (nb, 3) float64 the final crop centres,
        next_centers_uvd (nb, 3) the joint centre of the final pass (NaN where not moved), recenter_codes (recenter + 1, nb) int32
        awr_amd.detect's KEPT_* / MOVED, one row per awr_joints_center call -- device tensors, nothing synchronised.
        views: None | 2 ... 8 views (awr_amd.detect.make_views), each a dict or tuple of rot (degrees, in the image plane), scale (a factor
        on the cube's three edges, > 0) and shift (3 camera millimetres added to the crop centre); view 0 must be the identity.  The plan
        then holds max_batch * len(views) images; predict() still takes at most max_batch frames.  fuse: "mean" (every used view weighs 1) |
        "conf" (the weight is max(conf, 0) of DESIGN.md 4.18's conf per view and joint; the engine computes it whether or not confidence=True
        asks for the fields) | "median" (per axis).  predict() then returns a ViewPrediction / ConfidentViewPrediction: xyz and uvd are the
        FUSED joints, center_xyz / M / status (and conf / peak / spread_mm) are view 0's, and view_spread_mm (nb, J) float32 -- the weighted
        RMS distance of the used views' joints from the fused one -- and views_used (nb, J) int32 follow.  view_outputs holds the per-view
        device tensors of the last call: xyz, uvd (V, nb, J, 3), M (V, nb, 3, 3), center_xyz, cube (V, nb, 3), status, ustatus (V, nb) and,
        with an engine that has it, conf (V, nb, J) -- views into the call's buffers, nothing copied or synchronised.  With recenter / track
        the fused joints and view 0's centre and cube are what awr_joints_center reads, and each pass expands its views anew.
        palm: True -- the configured detector's centres go through awr_detect_palm (awr_amd.detect.palm_center) before the
        crop; not applied to centers_uvd handed to predict() nor to a tracked centre.  palm_search: the side of its window in cubes.  After
        such a predict(), palm_info (nb, 4) int32 holds awr_detect_palm's info rows (palm point u, v, its squared radius, pixels of the disc).
        smooth: None | True (the defaults) | a dict of awr_amd.track.OneEuro's fields | a OneEuro -- one awr_joints_filter launch (DESIGN.md
        4.25; statement: awr_amd.track.filter_step) behind the final pass (with views: behind awr_views_fuse): a One-Euro low-pass per batch
        slot, joint and axis with a gate (gate_mm), coasting (max_coast) and a constant-velocity look-ahead.  predict() then returns the
        FILTERED joints in xyz / uvd of the same named tuples; status, center_xyz, M and the confidence fields remain the measurement's.  A
        frame that is not OK yields the held joints instead of NaN rows while its track lives (check() still reports the frame).  After
        such a predict(): raw_xyz, raw_uvd (nb, J, 3) the unfiltered joints, ahead_xyz (nb, J, 3) the joints one dt ahead at the filtered
        velocity, filter_codes (nb, J) int32 awr_amd.track's NONE ... LOST -- device tensors, nothing synchronised.  Slot b of the filter is
        batch slot b, as the tracker's is; slots >= n_valid keep their state; reset_smooth() clears it.  weight="conf" scales each step by
        the joint's conf (view 0's) and switches the engine's confidence pass on whether or not confidence=True asks for the fields.
        lead=True needs track=True: the tracker's centre for the next call is the joint centre of ahead_xyz, not of the raw joints (the
        re-centring passes inside a call are unaffected).  The defaults are engineering choices; accuracy on real frames is UNMEASURED.
        hands: 1 | 2 ... 4 -- the hands looked for in every frame.  With K >= 2 the plan holds max_batch * K images,
        hand-major (slot k of batch slot b is row k * max_batch + b), awr_detect_hands seeds the K nearest connected components of the
        near foreground (reach: the depth of that foreground behind the nearest pixel, in millimetres; min_pixels: the smallest component
        that counts) and the configured refinement, the optional palm pass, the crop, the network and the re-centring passes run per row.
        predict() then returns a HandsPrediction / ConfidentHandsPrediction whose fields carry a hand axis behind the batch axis -- xyz, uvd
        (nb, K, J, 3), center_xyz (nb, K, 3), M (nb, K, 3, 3), status (nb, K), conf / peak / spread_mm (nb, K, J) -- and n_hands (nb,)
        int32; slot 0 is the nearest hand, an absent hand has status EMPTY and NaN rows.  hand_info (nb, K, 4) int32 holds
        awr_detect_hands' info rows (the component's first pixel u, v, its pixels, its nearest depth) after a call.  Not combined with
        views, track or smooth (track and smooth: unless identity is set, below); touching or overlapping hands are ONE component and count as one hand; reach and min_pixels are
        engineering defaults, UNMEASURED on real frames.
        identity: None | True (the defaults) | a dict of awr_amd.track.Identity's fields | an Identity -- with hands >= 2, keep every hand in
        ITS slot from call to call (statement: awr_amd.track.assign_step): one awr_hands_assign launch assigns this call's
        detected hands to the identities of the previous call of the same batch slot, exactly, within gate_mm camera millimetres; a hand
        that is not seen waits for max_miss calls (status EMPTY, NaN rows), a new hand takes the lowest free slot and the next id.  track,
        smooth (with lead) and predict(dt=...) are then accepted: the tracker seeds a second detector run with every slot's last centre and
        two tracked centres within merge_mm of each other are one hand; the filter state is (K * max_batch, J, ...) and a slot's rows are
        zeroed where an identity starts or ends.  predict() returns a TrackedHandsPrediction / ConfidentTrackedHandsPrediction:
        HandsPrediction's fields, where slot k is an identity and NOT the k-th nearest hand, n_hands the slots with status OK, and ids
        (nb, K) int32 (0: a free slot).  After such a call: hand_codes, hand_source (nb, K) int32 awr_amd.track's FREE ... MERGED and the
        candidate each slot took (-1 none, -2 its tracked centre), hands_dropped (nb,) int32 candidates that found no slot; hand_info and
        palm_info stay in CANDIDATE order (the nearest first); raw_xyz, raw_uvd, ahead_xyz, filter_codes carry the hand axis.  Explicit
        centers_uvd (nb, K, 3) are the candidates.  reset_identity() forgets the identities.  views stays refused.  The defaults are
        engineering choices, UNMEASURED on real frames."""
        if isinstance(hands, bool) or not isinstance(hands, int):
            raise TypeError("hands is an int in [1, %d], not %r" % (D.MAX_HANDS, hands))
        K, self.reach, _, self.min_pixels = D._check_hands(hands, reach, 0.0, min_pixels)
        self.hands, self.hand_info = K, None
        if identity is not None:
            self.identity = T.check_identity(identity)
            if K == 1:
                raise ValueError("identity decides which of SEVERAL hands is which: it needs hands >= 2 (hands=1 has one slot, and track=True follows it)")
        if K > 1:
            D._check_hands(K, reach, slab, min_pixels)
            for name, on in (("views", views is not None), ("track", track is not False), ("smooth", smooth is not None)):
                if on and (identity is None or name == "views"):
                    raise ValueError("hands = %d and %s are not combined yet: which hand of one call is which hand of the next is not decided "
                                     "here (hands=1 takes %s)" % (K, name, name))
        if not isinstance(palm, bool):
            raise TypeError("palm is True or False, not %r" % (palm,))
        self.palm, self.palm_search = palm, D.check_palm(palm_search)[0]
        self.palm_info = None
        if not isinstance(confidence, bool):
            raise TypeError("confidence is True or False, not %r" % (confidence,))
        self.confidence = confidence
        if isinstance(recenter, bool) or not isinstance(recenter, int):
            raise TypeError("recenter is an int in [0, %d], not %r" % (MAX_RECENTER, recenter))
        if not 0 <= recenter <= MAX_RECENTER:
            raise ValueError("recenter = %d is outside [0, %d]" % (recenter, MAX_RECENTER))
        if not isinstance(track, bool):
            raise TypeError("track is True or False, not %r" % (track,))
        if isinstance(max_shift, (bool, str)) or not isinstance(max_shift, (int, float)):
            raise TypeError("max_shift is a number >= 0, not %r" % (max_shift,))
        if not float(max_shift) >= 0.0:
            raise ValueError("max_shift = %r must be >= 0 (infinity: no shift gate)" % (max_shift,))
        if center_joints is not None:
            if isinstance(center_joints, (str, bytes)) or any(isinstance(j, bool) or not isinstance(j, (int, np.integer)) for j in center_joints):
                raise TypeError("center_joints is a list of joint indices, not %r" % (center_joints,))
            center_joints = [int(j) for j in center_joints]
            nj = int(net.J)
            if not 0 < len(center_joints) <= nj or any(not 0 <= j < nj for j in center_joints):
                raise ValueError("center_joints needs 1 ... %d indices in [0, %d), got %r" % (nj, nj, center_joints))
        if fuse not in D.FUSE_MODES:
            raise ValueError("fuse is one of %s, not %r" % (sorted(D.FUSE_MODES), fuse))
        if views is not None:
            self.views, self.fuse = D.check_views(views, fuse), fuse
            self.V = len(self.views)
        self.view_outputs = None
        if smooth is not None:
            self.smooth = T.check_filter(smooth)
            if self.smooth.lead and not track:
                raise ValueError("smooth lead=True moves the TRACKER's next centre to the look-ahead joints: it needs track=True")
        self.recenter, self.track, self.max_shift = recenter, track, float(max_shift)
        self.centers_uvd = self.next_centers_uvd = self.recenter_codes = None
        if not torch.cuda.is_available():
            raise L.AwrError("Predictor runs the detector, the crop, the network and the un-projection as HIP kernels and needs a GPU: none is "
                             "visible -- awr_amd.detect.detect is the host statement of the detector")
        from . import nyu_device as DV
        from .trainer import InferEngine
        if seed not in ("nearest", "range"):
            raise ValueError("seed is \"nearest\" or \"range\" (pass centers_uvd to predict() for given centres), not %r" % (seed,))
        if not 0 <= int(refine_iters) <= D.MAX_ITERS:
            raise ValueError("refine_iters = %r is outside [0, %d]" % (refine_iters, D.MAX_ITERS))
        if not float(depth_range[0]) <= float(depth_range[1]):
            raise ValueError("depth_range needs zmin <= zmax")
        self.S, self.B = int(img_size), int(max_batch)
        self.fh, self.fw = int(frame_shape[0]), int(frame_shape[1])
        self.paras, self.flip = tuple(float(p) for p in paras), int(flip)
        self.seed, self.depth_range, self.slab, self.iters = seed, (float(depth_range[0]), float(depth_range[1])), float(slab), int(refine_iters)
        dev = self.device = net.device
        B = self.B
        V = self.V
        P = B * V * K                            # rows of the plan: view-major, view 0 first; with hands hand-major, the nearest hand first
        self.engine = InferEngine(net, P, self.S, kernel_size, winograd=winograd, parity=parity,
                                  confidence=confidence or (V > 1 and fuse == "conf") or (smooth is not None and self.smooth.weight == "conf"))
        self.J = self.engine.J
        # the predictor's own small frame store: the FrameStore layout, one row per image of a batch
        self._frames = torch.empty((B, self.fh, self.fw), dtype=torch.uint16, device=dev)
        self._frames.view(torch.int16).zero_()
        self._stage = torch.empty((B, self.fh, self.fw), dtype=torch.uint16).pin_memory()
        self._stage_free = None                  # event: the last upload from the staging buffer has been issued and has finished
        self._store = types.SimpleNamespace(data=self._frames, ftype=0, fh=self.fh, fw=self.fw, n=B)
        self._render = DV.Renderer(self._store, self.S, P)
        self._idx = torch.arange(B, dtype=torch.int64, device=dev).repeat(K)          # (K > 1: the frame of every hand-major row)
        self._cube = torch.tensor([float(c) for c in cube], dtype=torch.float64, device=dev)
        self._scratch = torch.empty(int(L.lib.awr_detect_scratch(B * K)) // 8, dtype=torch.int64, device=dev)
        self._centers = torch.empty((B * K, 3), dtype=torch.float64, device=dev)
        self._seed = torch.empty((B * K, 3), dtype=torch.float64, device=dev)
        self._blocks = torch.empty((P, DV.BLOCK_BYTES), dtype=torch.uint8, device=dev)
        self._cube32 = torch.empty((P, 3), dtype=torch.float32, device=dev)
        self._img = torch.zeros((P, 1, self.S, self.S), dtype=torch.float32, device=dev)
        self._last = None
        if V > 1:
            self._vtable = torch.from_numpy(D.view_table(self.views, self.S)).to(dev)          # cos / sin are the host's: uploaded once
            self._vcenters = torch.full((P, 3), float("nan"), dtype=torch.float64, device=dev)
            self._vcubes = torch.ones((P, 3), dtype=torch.float64, device=dev)
            self._vframe = torch.zeros(P, dtype=torch.int64, device=dev)
        if recenter or track:
            self._joints = None if center_joints is None else torch.tensor(center_joints, dtype=torch.int32, device=dev)
            self._moved = torch.empty((B * K, 3), dtype=torch.float64, device=dev)      # center_out of the call that only asks for `next`
        if palm:
            nbytes = int(L.lib.awr_detect_palm_scratch(B * K, self.fh, self.fw))
            if nbytes < 0:
                raise L.AwrError(L.last_error())
            self._palm_scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
            self._palm_info = torch.empty((B * K, 4), dtype=torch.int32, device=dev)
        if K > 1:
            nbytes = int(L.lib.awr_detect_hands_scratch(B, self.fh, self.fw))
            if nbytes < 0:
                raise L.AwrError(L.last_error())
            self._hands_scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            self._hands_status = torch.empty((K, B), dtype=torch.int32, device=dev)
            self._hands_info = torch.empty((K, B, 4), dtype=torch.int32, device=dev)
            self._hands_count = torch.empty(B, dtype=torch.int32, device=dev)
        if smooth is not None:
            self._filter_state = torch.zeros((B * K, self.J, 6), dtype=torch.float64, device=dev)      # x0 x1 x2 d0 d1 d2 per slot (and hand) and joint
            self._filter_count = torch.zeros((B * K, self.J, 2), dtype=torch.int32, device=dev)        # age, coast
            self.raw_xyz = self.raw_uvd = self.ahead_xyz = self.filter_codes = None
        if self.identity is not None:
            # the assignment's state, hand-major (track.identity_state), and the candidates it chooses among
            self._id_last = torch.full((K, B, 3), float("nan"), dtype=torch.float64, device=dev)
            self._id_ids = torch.zeros((K, B), dtype=torch.int32, device=dev)
            self._id_miss = torch.zeros((K, B), dtype=torch.int32, device=dev)
            self._id_next = torch.ones(B, dtype=torch.int32, device=dev)
            self._cand = torch.empty((B * K, 3), dtype=torch.float64, device=dev)
            self._cand_status = torch.empty(B * K, dtype=torch.int32, device=dev)
            self.hand_codes = self.hand_source = self.hands_dropped = None
            if recenter or track:
                self._zero_status = torch.zeros(B * K, dtype=torch.int32, device=dev)
                self._sel = torch.empty((B * K, 3), dtype=torch.float64, device=dev)
                self._sel_status = torch.empty(B * K, dtype=torch.int32, device=dev)
        if track:
            # (with identities the tracked centres ARE the assignment's last centres, one per slot and hand)
            self._track = torch.full((B, 3), float("nan"), dtype=torch.float64, device=dev) if K == 1 else self._id_last.view(B * K, 3)
            self._tcenters = torch.empty((B * K, 3), dtype=torch.float64, device=dev)
            self._dcenters = torch.empty((B, 3), dtype=torch.float64, device=dev)
            self._tstatus = torch.empty(B * K, dtype=torch.int32, device=dev)
            self._dstatus = torch.empty(B, dtype=torch.int32, device=dev)

    def _slots(self, slots, n=None):
        if slots is None:
            return None
        if isinstance(slots, torch.Tensor):
            return slots.to(device=self.device, dtype=torch.int64, non_blocking=True)
        idx = [int(i) for i in slots]
        if any(not 0 <= i < self.B for i in idx) or (n is not None and len(idx) != n):
            raise L.AwrError("slots must be %sindices in [0, max_batch = %d), got %r" % ("" if n is None else "%d " % n, self.B, slots))
        return torch.tensor(idx, dtype=torch.int64).to(self.device, non_blocking=True)

    def set_track(self, centers_uvd, slots=None):
        """Set the tracked centres from outside: centers_uvd (n, 3), numpy or tensor, host or device, for batch slots `slots` (default:
        slots [0, n)).  A NaN row marks its slot as lost.  With identity: (n, K, 3), a centre per hand slot (see _set_track_hands).  Does not block."""
        if not self.track:
            raise L.AwrError("set_track needs a Predictor built with track=True")
        if self.identity is not None:
            return self._set_track_hands(centers_uvd, slots)
        c = centers_uvd if isinstance(centers_uvd, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(centers_uvd, dtype=np.float64))
        if c.dim() != 2 or c.shape[1] != 3 or not 0 < c.shape[0] <= self.B:
            raise L.AwrError("centers_uvd must be (n, 3) with n in [1, max_batch = %d], got %s" % (self.B, tuple(c.shape)))
        idx = self._slots(slots, int(c.shape[0]))
        if idx is None:
            self._track[:c.shape[0]].copy_(c, non_blocking=True)
        else:
            self._track.index_copy_(0, idx, c.to(device=self.device, dtype=torch.float64, non_blocking=True))

    def reset_track(self, slots=None):
        """Mark batch slots (default: all of them) as lost: their next call starts from the detector.  With identity this is reset_identity.
        Does not block."""
        if not self.track:
            raise L.AwrError("reset_track needs a Predictor built with track=True")
        if self.identity is not None:
            return self.reset_identity(slots)          # (a tracked centre is its identity's last centre: without one the identity ends)
        idx = self._slots(slots)
        if idx is None:
            self._track.fill_(float("nan"))
        else:
            self._track.index_fill_(0, idx, float("nan"))

    def reset_smooth(self, slots=None):
        """Drop the temporal filter's tracks of batch slots (default: all of them; with hands >= 2 every hand of each): their next usable
        frame starts a track.  Does not block."""
        if self.smooth is None:
            raise L.AwrError("reset_smooth needs a Predictor built with smooth=...")
        idx = self._slots(slots)
        if idx is None:
            self._filter_state.zero_()
            self._filter_count.zero_()
        elif self.hands > 1:                     # hand-major rows: batch slot b is row k * max_batch + b of every hand k
            self._filter_state.view(self.hands, self.B, self.J, 6).index_fill_(1, idx, 0.0)
            self._filter_count.view(self.hands, self.B, self.J, 2).index_fill_(1, idx, 0)
        else:
            self._filter_state.index_fill_(0, idx, 0.0)
            self._filter_count.index_fill_(0, idx, 0)

    def reset_identity(self, slots=None):
        """Forget the hand identities of batch slots (default: all of them), every hand of each: their next call starts new identities (ids are
        never used again) and, with smooth, new filter tracks.  Does not block."""
        if self.identity is None:
            raise L.AwrError("reset_identity needs a Predictor built with identity=...")
        idx = self._slots(slots)
        if idx is None:
            self._id_last.fill_(float("nan"))
            self._id_ids.zero_()
            self._id_miss.zero_()
        else:
            self._id_last.index_fill_(1, idx, float("nan"))
            self._id_ids.index_fill_(1, idx, 0)
            self._id_miss.index_fill_(1, idx, 0)
        if self.smooth is not None:
            self.reset_smooth(slots)

    def _set_track_hands(self, centers_uvd, slots):
        """set_track with identities: centers_uvd (n, K, 3); a finite row puts slot k of its batch slot there -- it keeps the identity it has, a
        free slot gets the next one -- and a NaN row ends the slot's identity.  Device arithmetic only; does not block."""
        K, B, nan = self.hands, self.B, float("nan")
        c = centers_uvd if isinstance(centers_uvd, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(centers_uvd, dtype=np.float64))
        if c.dim() != 3 or tuple(c.shape[1:]) != (K, 3) or not 0 < c.shape[0] <= B:
            raise L.AwrError("centers_uvd must be (n, %d, 3) with n in [1, max_batch = %d], got %s" % (K, B, tuple(c.shape)))
        n = int(c.shape[0])
        idx = self._slots(slots, n)
        if idx is None:
            idx = torch.arange(n, dtype=torch.int64, device=self.device)
        c = c.to(device=self.device, dtype=torch.float64, non_blocking=True).transpose(0, 1)          # (K, n, 3)
        ids, nxt = self._id_ids.index_select(1, idx), self._id_next.index_select(0, idx)
        finite = torch.isfinite(c).all(-1)
        new = finite & (ids == 0)
        fresh = (nxt[None] + new.cumsum(0) - 1).to(torch.int32)
        ended = ~finite & (ids > 0)
        self._id_ids.index_copy_(1, idx, torch.where(new, fresh, torch.where(finite, ids, torch.zeros_like(ids))))
        self._id_miss.index_fill_(1, idx, 0)
        self._id_next.index_copy_(0, idx, (nxt + new.sum(0)).to(torch.int32))
        self._id_last.index_copy_(1, idx, torch.where(finite[..., None], c, torch.full_like(c, nan)))
        if self.smooth is not None:
            fs, fc = self._filter_state.view(K, B, self.J, 6), self._filter_count.view(K, B, self.J, 2)
            fs.index_copy_(1, idx, torch.where(ended[..., None, None], torch.zeros_like(fs[:, :n]), fs.index_select(1, idx)))
            fc.index_copy_(1, idx, torch.where(ended[..., None, None], torch.zeros_like(fc[:, :n]), fc.index_select(1, idx)))

    def _joints_center(self, xyz, cxyz, status, ustatus, nv, center_out, next_out, code):
        fx, fy, u0, v0 = self.paras
        L.call("awr_joints_center", L.ptr(xyz), self._centers.data_ptr(), L.ptr(cxyz), L.ptr(self._cube32), status.data_ptr(), ustatus.data_ptr(),
               self.B, self.J, nv, L.ptr(self._joints), 0 if self._joints is None else int(self._joints.numel()), fx, fy, u0, v0, self.flip,
               self.depth_range[0], self.depth_range[1], self.max_shift, center_out.data_ptr(), L.ptr(next_out), code.data_ptr(), L.stream())

    def _smooth_step(self, xyz, status, ustatus, conf, nv, dt):
        """one awr_joints_filter launch over the call's output joints -> (xyz_f, uvd_f, ahead (B, J, 3), code (B, J)), fresh tensors"""
        cfg, B, J, dev = self.smooth, self.B, self.J, self.device
        fx, fy, u0, v0 = self.paras
        if cfg.weight == "conf" and conf is None:
            conf = self.engine.conf[:B, :, 0].contiguous()          # (B, J): view 0's rows come first
        out = [torch.empty((B, J, 3), dtype=torch.float32, device=dev) for _ in range(3)] + [torch.empty((B, J), dtype=torch.int32, device=dev)]
        L.call("awr_joints_filter", self._filter_state.data_ptr(), self._filter_count.data_ptr(), L.ptr(xyz), status.data_ptr(), ustatus.data_ptr(),
               L.ptr(conf) if cfg.weight == "conf" else None, B, J, nv, dt, cfg.min_cutoff, cfg.beta, cfg.d_cutoff,
               -1.0 if cfg.gate_mm is None else cfg.gate_mm, cfg.max_coast, T.WEIGHTS[cfg.weight], cfg.conf_floor, fx, fy, u0, v0, self.flip,
               L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]), L.stream())
        return out

    def _upload(self, frames):
        """(nb, fh, fw) uint16 -> rows [0, nb) of the frame store, without blocking"""
        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint16:
                raise L.AwrError("frames must be uint16 millimetres (the sensor format; it makes the detector's sums exact), not %s" % frames.dtype)
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint16:
            raise L.AwrError("frames must be a uint16 numpy array or tensor")
        if frames.dim() != 3 or tuple(frames.shape[1:]) != (self.fh, self.fw):
            raise L.AwrError("frames must be (B, %d, %d), got %s" % (self.fh, self.fw, tuple(frames.shape)))
        nb = int(frames.shape[0])
        if not 0 < nb <= self.B:
            raise L.AwrError("a batch of %d frames does not fit the predictor's max_batch %d" % (nb, self.B))
        if frames.is_cuda:
            self._frames[:nb].copy_(frames, non_blocking=True)
            return nb
        if not frames.is_pinned():
            # pageable memory -> the pinned staging buffer -> HBM.  The buffer is reused: wait for the previous upload FROM IT (a copy, not
            # the pipeline: the launches behind it stay queued)
            if self._stage_free is not None:
                self._stage_free.synchronize()
            self._stage[:nb].copy_(frames)
            frames = self._stage[:nb]
            self._frames[:nb].copy_(frames, non_blocking=True)
            self._stage_free = torch.cuda.Event()
            self._stage_free.record()
        else:
            self._frames[:nb].copy_(frames, non_blocking=True)
        return nb

    def predict(self, frames, centers_uvd=None, n_valid=None, dt=None):
        """-> Prediction(xyz (nb, J, 3), uvd (nb, J, 3), center_xyz (nb, 3), M (nb, 3, 3), status (nb,) int32), device tensors, nothing
        synchronised; with confidence=True a ConfidentPrediction: these and conf, peak, spread_mm (nb, J).  centers_uvd (nb, 3): hand centres in original-image uvd (numpy or tensor) instead of the detector's seed.  n_valid:
        frames of the batch that count (default: all of them); rows past it hold unspecified values.  status: awr_amd.detect's codes; a frame that is
        not OK has NaN rows (of conf / peak / spread_mm too).  With recenter > 0 every field is the FINAL pass's; with track=True a call
        without centers_uvd starts from the tracked centres (see __init__), an explicit centers_uvd overrides them for this call, and either
        way slots [0, n_valid) of the tracker take this call's next_centers_uvd.  dt: seconds since the previous call, for a predictor with
        smooth (default 1 / its fps); xyz and uvd are then the filtered joints (see __init__)."""
        if self.hands > 1:
            if self.identity is not None and self.smooth is not None:
                return self._predict_identity(frames, centers_uvd, n_valid, T.check_dt(1.0 / self.smooth.fps if dt is None else dt))
            if dt is not None:
                raise L.AwrError("predict(dt=...) is the temporal filter's time step: it needs a Predictor built with smooth=...")
            if self.identity is not None:
                return self._predict_identity(frames, centers_uvd, n_valid, None)
            return self._predict_hands(frames, centers_uvd, n_valid)
        if self.smooth is None:
            if dt is not None:
                raise L.AwrError("predict(dt=...) is the temporal filter's time step: it needs a Predictor built with smooth=...")
        else:
            dt = T.check_dt(1.0 / self.smooth.fps if dt is None else dt)
        nb = self._upload(frames)
        nv = nb if n_valid is None else int(n_valid)
        if not 0 < nv <= nb:
            raise L.AwrError("n_valid = %d is outside [1, %d]" % (nv, nb))
        dev, B, J, s = self.device, self.B, self.J, L.stream()
        fx, fy, u0, v0 = self.paras
        mode, seed = D.SEEDS[self.seed], None
        if centers_uvd is not None:
            c = centers_uvd if isinstance(centers_uvd, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(centers_uvd, dtype=np.float64))
            if tuple(c.shape) != (nb, 3):
                raise L.AwrError("centers_uvd must be (%d, 3), got %s" % (nb, tuple(c.shape)))
            self._seed[:nb].copy_(c, non_blocking=True)          # (converts to float64 on the way)
            mode, seed = D.SEED_GIVEN, self._seed
        V, P = self.V, self.B * self.V
        M = torch.empty((P, 3, 3), dtype=torch.float32, device=dev)
        cxyz = torch.empty((P, 3), dtype=torch.float32, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        ustatus = torch.zeros(P, dtype=torch.int32, device=dev)
        uvd = torch.empty((P, J, 3), dtype=torch.float32, device=dev)
        xyz = torch.empty((P, J, 3), dtype=torch.float32, device=dev)
        if V > 1:
            # status: the frames' (the detector's); vstatus: one per row, view 0's first -- what every later stage and check() read
            vstatus = torch.zeros(P, dtype=torch.int32, device=dev)
            fxyz = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
            fuvd = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
            vspread = torch.empty((B, J), dtype=torch.float32, device=dev)
            vused = torch.empty((B, J), dtype=torch.int32, device=dev)
            weights = [None]

        def detect(mode, seed, centers, status):
            L.call("awr_detect", self._frames.data_ptr(), 0, B, self.fh, self.fw, self._idx.data_ptr(), nv, mode, L.ptr(seed), self.depth_range[0],
                   self.depth_range[1], self.slab, self._cube.data_ptr(), 0, fx, fy, self.iters, 0, self._scratch.data_ptr(),
                   centers.data_ptr(), status.data_ptr(), s)

        def palm(centers, status):
            # in place: a frame that is not OK keeps its centre and status
            L.call("awr_detect_palm", self._frames.data_ptr(), 0, B, self.fh, self.fw, self._idx.data_ptr(), nv, centers.data_ptr(),
                   status.data_ptr(), self.depth_range[0], self.depth_range[1], self._cube.data_ptr(), 0, fx, fy, self.palm_search,
                   D.PALM_TAU[0], D.PALM_TAU[1], D.PALM_RHO2[0], D.PALM_RHO2[1], self._palm_scratch.data_ptr(), centers.data_ptr(),
                   status.data_ptr(), self._palm_info.data_ptr(), s)
            self.palm_info = self._palm_info[:nb]

        def crop_and_predict():
            L.call("awr_detect_samples", self._centers.data_ptr(), self._cube.data_ptr(), 0, B, self._idx.data_ptr(), nv, self.S, self.fh, self.fw,
                   fx, fy, u0, v0, self.flip, self._blocks.data_ptr(), L.ptr(M), L.ptr(cxyz), L.ptr(self._cube32), status.data_ptr(), s)
            self._render(self._blocks[:nv], out=self._img[:nv])
            if nv < B:
                self._img[nv:].zero_()          # padding rows of the static plan: constant input, and no later stage reads their output
            jt = self.engine(self._img)
            L.call("awr_joints_unproject", L.ptr(jt), L.ptr(cxyz), L.ptr(M), L.ptr(self._cube32), B, J, nv, float(self.S), fx, fy, u0, v0, self.flip,
                   L.ptr(uvd), L.ptr(xyz), ustatus.data_ptr(), s)

        def views_and_predict():
            # centres -> one centre, cube and frame row per view; the rows past n_valid of each view hold NaN centres: blocks without pixels
            if nv < B:
                self._vcenters.fill_(float("nan"))
            L.call("awr_view_centers", self._centers.data_ptr(), status.data_ptr(), self._cube.data_ptr(), 0, self._vtable.data_ptr(), V, B, nv,
                   fx, fy, u0, v0, self.flip, self._vcenters.data_ptr(), self._vcubes.data_ptr(), self._vframe.data_ptr(), vstatus.data_ptr(), s)
            L.call("awr_detect_samples", self._vcenters.data_ptr(), self._vcubes.data_ptr(), 3, B, self._vframe.data_ptr(), P, self.S, self.fh,
                   self.fw, fx, fy, u0, v0, self.flip, self._blocks.data_ptr(), L.ptr(M), L.ptr(cxyz), L.ptr(self._cube32), vstatus.data_ptr(), s)
            L.call("awr_view_rotate", self._blocks.data_ptr(), L.ptr(M), vstatus.data_ptr(), self._vtable.data_ptr(), V, B, nv, s)
            self._render(self._blocks, out=self._img)
            jt = self.engine(self._img)
            L.call("awr_joints_unproject", L.ptr(jt), L.ptr(cxyz), L.ptr(M), L.ptr(self._cube32), P, J, P, float(self.S), fx, fy, u0, v0, self.flip,
                   L.ptr(uvd), L.ptr(xyz), ustatus.data_ptr(), s)
            if self.fuse == "conf":
                weights[0] = self.engine.conf[..., 0].contiguous()          # (P, J): the head's conf of every row, packed
            L.call("awr_views_fuse", L.ptr(xyz), vstatus.data_ptr(), ustatus.data_ptr(), L.ptr(weights[0]), D.FUSE_MODES[self.fuse], V, B, J, nv,
                   fx, fy, u0, v0, self.flip, L.ptr(fxyz), L.ptr(fuvd), L.ptr(vspread), L.ptr(vused), s)

        smoothed = None
        if V > 1:
            crop_and_predict, out_xyz, out_uvd, out_status = views_and_predict, fxyz, fuvd, vstatus
        else:
            out_xyz, out_uvd, out_status = xyz, uvd, status
        if self.track and seed is None:
            # the tracked centres first (a lost slot's NaN seed finds nothing), the configured detector second, per slot whichever holds
            detect(D.SEED_GIVEN, self._track, self._tcenters, self._tstatus)
            detect(mode, None, self._dcenters, self._dstatus)
            if self.palm:
                palm(self._dcenters, self._dstatus)
            L.call("awr_centers_select", self._tcenters.data_ptr(), self._tstatus.data_ptr(), self._dcenters.data_ptr(), self._dstatus.data_ptr(),
                   nv, self._centers.data_ptr(), status.data_ptr(), None, s)
        else:
            detect(mode, seed, self._centers, status)
            if self.palm and seed is None:
                palm(self._centers, status)
        crop_and_predict()
        if self.recenter or self.track:
            codes = torch.zeros((self.recenter + 1, B), dtype=torch.int32, device=dev)
            for k in range(self.recenter):
                # moved frames get their new centre in place, the others keep theirs: their next pass repeats this one bit for bit
                self._joints_center(out_xyz, cxyz, out_status, ustatus, nv, self._centers, None, codes[k])
                crop_and_predict()
            nxt = torch.full((B, 3), float("nan"), dtype=torch.float64, device=dev)
            next_from = out_xyz
            if self.smooth is not None and self.smooth.lead:
                # the next call's crop starts where constant velocity says the hand will be: filter first, centre the look-ahead joints
                smoothed = self._smooth_step(out_xyz, out_status, ustatus, weights[0] if V > 1 else None, nv, dt)
                next_from = smoothed[2]
            self._joints_center(next_from, cxyz, out_status, ustatus, nv, self._moved, nxt, codes[self.recenter])
            self.centers_uvd, self.next_centers_uvd, self.recenter_codes = self._centers[:nb].clone(), nxt[:nb], codes[:, :nb]
            if self.track:
                self._track[:nv].copy_(nxt[:nv])
        self._last = (out_status, ustatus, nv)
        if self.smooth is not None:
            fxyz_t, fuvd_t, ahead, fcodes = smoothed or self._smooth_step(out_xyz, out_status, ustatus, weights[0] if V > 1 else None, nv, dt)
            self.raw_xyz, self.raw_uvd, self.ahead_xyz, self.filter_codes = out_xyz[:nb], out_uvd[:nb], ahead[:nb], fcodes[:nb]
            if V > 1:
                fxyz, fuvd = fxyz_t, fuvd_t
            else:
                xyz, uvd = fxyz_t, fuvd_t
        if self.confidence:
            # (with views: view 0's rows are the first B of every per-row buffer)
            fields = torch.empty((3, B, J), dtype=torch.float32, device=dev)
            L.call("awr_confidence_fields", L.ptr(self.engine.conf), L.ptr(self.engine.stat), L.ptr(self._cube32), out_status.data_ptr(),
                   ustatus.data_ptr(), B, J, nv, L.ptr(fields[0]), L.ptr(fields[1]), L.ptr(fields[2]), s)
        if V > 1:
            per_view = dict(xyz=xyz.view(V, B, J, 3)[:, :nb], uvd=uvd.view(V, B, J, 3)[:, :nb], M=M.view(V, B, 3, 3)[:, :nb],
                            center_xyz=cxyz.view(V, B, 3)[:, :nb], cube=self._cube32.view(V, B, 3)[:, :nb], status=vstatus.view(V, B)[:, :nb],
                            ustatus=ustatus.view(V, B)[:, :nb])
            if self.engine.conf is not None:
                per_view["conf"] = (self.engine.conf[..., 0] if weights[0] is None else weights[0]).view(V, B, J)[:, :nb]
            self.view_outputs = types.SimpleNamespace(**per_view)
            if self.confidence:
                return ConfidentViewPrediction(fxyz[:nb], fuvd[:nb], cxyz[:nb], M[:nb], vstatus[:nb], fields[0, :nb], fields[1, :nb], fields[2, :nb],
                                               vspread[:nb], vused[:nb])
            return ViewPrediction(fxyz[:nb], fuvd[:nb], cxyz[:nb], M[:nb], vstatus[:nb], vspread[:nb], vused[:nb])
        if self.confidence:
            return ConfidentPrediction(xyz[:nb], uvd[:nb], cxyz[:nb], M[:nb], status[:nb], fields[0, :nb], fields[1, :nb], fields[2, :nb])
        return Prediction(xyz[:nb], uvd[:nb], cxyz[:nb], M[:nb], status[:nb])

    def _predict_hands(self, frames, centers_uvd, n_valid):
        """predict() of a predictor with hands = K >= 2: every stage over the K * max_batch hand-major rows, row k * max_batch + b"""
        nb = self._upload(frames)
        nv = nb if n_valid is None else int(n_valid)
        if not 0 < nv <= nb:
            raise L.AwrError("n_valid = %d is outside [1, %d]" % (nv, nb))
        dev, B, K, J, s = self.device, self.B, self.hands, self.J, L.stream()
        P = B * K
        fx, fy, u0, v0 = self.paras
        nan = float("nan")
        seeds = self._seed.view(K, B, 3)
        if centers_uvd is not None:
            c = centers_uvd if isinstance(centers_uvd, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(centers_uvd, dtype=np.float64))
            if tuple(c.shape) != (nb, K, 3):
                raise L.AwrError("centers_uvd must be (%d, %d, 3): a centre per frame and hand, NaN rows for an absent hand, got %s" % (nb, K, tuple(c.shape)))
            seeds[:, :nb].copy_(c.transpose(0, 1), non_blocking=True)          # (converts to float64 on the way)
            self.hand_info = None
        else:
            L.call("awr_detect_hands", self._frames.data_ptr(), 0, B, self.fh, self.fw, self._idx.data_ptr(), B, K, self.depth_range[0],
                   self.depth_range[1], self.reach, self.slab, self.min_pixels, self._hands_scratch.data_ptr(), None, self._seed.data_ptr(),
                   self._hands_status.data_ptr(), self._hands_info.data_ptr(), self._hands_count.data_ptr(), s)
            self.hand_info = self._hands_info[:, :nb].transpose(0, 1)
        if nv < B:
            seeds[:, nv:].fill_(nan)                 # rows past n_valid of every block: NaN seeds, blocks without pixels
        M = torch.empty((P, 3, 3), dtype=torch.float32, device=dev)
        cxyz = torch.empty((P, 3), dtype=torch.float32, device=dev)
        status = torch.empty(P, dtype=torch.int32, device=dev)
        ustatus = torch.zeros(P, dtype=torch.int32, device=dev)
        uvd = torch.empty((P, J, 3), dtype=torch.float32, device=dev)
        xyz = torch.empty((P, J, 3), dtype=torch.float32, device=dev)
        # the unchanged detector refines every seed: a NaN seed (an absent hand) finds nothing and ends EMPTY
        L.call("awr_detect", self._frames.data_ptr(), 0, B, self.fh, self.fw, self._idx.data_ptr(), P, D.SEED_GIVEN, self._seed.data_ptr(),
               self.depth_range[0], self.depth_range[1], self.slab, self._cube.data_ptr(), 0, fx, fy, self.iters, 0, self._scratch.data_ptr(),
               self._centers.data_ptr(), status.data_ptr(), s)
        if self.palm and centers_uvd is None:
            L.call("awr_detect_palm", self._frames.data_ptr(), 0, B, self.fh, self.fw, self._idx.data_ptr(), P, self._centers.data_ptr(),
                   status.data_ptr(), self.depth_range[0], self.depth_range[1], self._cube.data_ptr(), 0, fx, fy, self.palm_search,
                   D.PALM_TAU[0], D.PALM_TAU[1], D.PALM_RHO2[0], D.PALM_RHO2[1], self._palm_scratch.data_ptr(), self._centers.data_ptr(),
                   status.data_ptr(), self._palm_info.data_ptr(), s)
            self.palm_info = self._palm_info.view(K, B, 4)[:, :nb].transpose(0, 1)

        def crop_and_predict():
            L.call("awr_detect_samples", self._centers.data_ptr(), self._cube.data_ptr(), 0, B, self._idx.data_ptr(), P, self.S, self.fh, self.fw,
                   fx, fy, u0, v0, self.flip, self._blocks.data_ptr(), L.ptr(M), L.ptr(cxyz), L.ptr(self._cube32), status.data_ptr(), s)
            self._render(self._blocks, out=self._img)
            jt = self.engine(self._img)
            L.call("awr_joints_unproject", L.ptr(jt), L.ptr(cxyz), L.ptr(M), L.ptr(self._cube32), P, J, P, float(self.S), fx, fy, u0, v0, self.flip,
                   L.ptr(uvd), L.ptr(xyz), ustatus.data_ptr(), s)

        def joints_center(center_out, next_out, code):
            L.call("awr_joints_center", L.ptr(xyz), self._centers.data_ptr(), L.ptr(cxyz), L.ptr(self._cube32), status.data_ptr(), ustatus.data_ptr(),
                   P, J, P, L.ptr(self._joints), 0 if self._joints is None else int(self._joints.numel()), fx, fy, u0, v0, self.flip,
                   self.depth_range[0], self.depth_range[1], self.max_shift, center_out.data_ptr(), L.ptr(next_out), code.data_ptr(), s)

        crop_and_predict()
        if self.recenter:
            codes = torch.zeros((self.recenter + 1, P), dtype=torch.int32, device=dev)
            for k in range(self.recenter):
                joints_center(self._centers, None, codes[k])
                crop_and_predict()
            nxt = torch.full((P, 3), nan, dtype=torch.float64, device=dev)
            joints_center(self._moved, nxt, codes[self.recenter])
            self.centers_uvd = self._centers.clone().view(K, B, 3)[:, :nb].transpose(0, 1)
            self.next_centers_uvd = nxt.view(K, B, 3)[:, :nb].transpose(0, 1)
            self.recenter_codes = codes.view(self.recenter + 1, K, B)[:, :, :nb].transpose(1, 2)
        self._last = (status.view(K, B), ustatus.view(K, B), nv)
        if centers_uvd is None:
            n_hands = self._hands_count[:nb].clamp(max=K)
        else:
            n_hands = (status.view(K, B)[:, :nb] == D.OK).sum(0, dtype=torch.int32)

        def rows(t):          # hand-major (K * B, ...) -> a (nb, K, ...) view
            return t.view((K, B) + tuple(t.shape[1:]))[:, :nb].transpose(0, 1)
        fields = (rows(xyz), rows(uvd), rows(cxyz), rows(M), rows(status), n_hands)
        if self.confidence:
            conf = torch.empty((3, P, J), dtype=torch.float32, device=dev)
            L.call("awr_confidence_fields", L.ptr(self.engine.conf), L.ptr(self.engine.stat), L.ptr(self._cube32), status.data_ptr(),
                   ustatus.data_ptr(), P, J, P, L.ptr(conf[0]), L.ptr(conf[1]), L.ptr(conf[2]), s)
            return ConfidentHandsPrediction(*fields, rows(conf[0]), rows(conf[1]), rows(conf[2]))
        return HandsPrediction(*fields)

    def _predict_identity(self, frames, centers_uvd, n_valid, dt):
        """predict() of a predictor with hands = K >= 2 and identity: _predict_hands with awr_hands_assign between the detector and the crop,
        the optional tracker in front of it and the optional temporal filter behind the final pass"""
        nb = self._upload(frames)
        nv = nb if n_valid is None else int(n_valid)
        if not 0 < nv <= nb:
            raise L.AwrError("n_valid = %d is outside [1, %d]" % (nv, nb))
        dev, B, K, J, s = self.device, self.B, self.hands, self.J, L.stream()
        P = B * K
        fx, fy, u0, v0 = self.paras
        nan, cfg = float("nan"), self.identity
        seeds = self._seed.view(K, B, 3)
        if centers_uvd is not None:
            c = centers_uvd if isinstance(centers_uvd, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(centers_uvd, dtype=np.float64))
            if tuple(c.shape) != (nb, K, 3):
                raise L.AwrError("centers_uvd must be (%d, %d, 3): a centre per frame and hand, NaN rows for an absent hand, got %s" % (nb, K, tuple(c.shape)))
            seeds[:, :nb].copy_(c.transpose(0, 1), non_blocking=True)          # (converts to float64 on the way)
            self.hand_info = None
        else:
            L.call("awr_detect_hands", self._frames.data_ptr(), 0, B, self.fh, self.fw, self._idx.data_ptr(), B, K, self.depth_range[0],
                   self.depth_range[1], self.reach, self.slab, self.min_pixels, self._hands_scratch.data_ptr(), None, self._seed.data_ptr(),
                   self._hands_status.data_ptr(), self._hands_info.data_ptr(), self._hands_count.data_ptr(), s)
            self.hand_info = self._hands_info[:, :nb].transpose(0, 1)
        if nv < B:
            seeds[:, nv:].fill_(nan)                 # rows past n_valid of every block: NaN seeds, candidates that are EMPTY
        M = torch.empty((P, 3, 3), dtype=torch.float32, device=dev)
        cxyz = torch.empty((P, 3), dtype=torch.float32, device=dev)
        status = torch.empty(P, dtype=torch.int32, device=dev)
        ustatus = torch.zeros(P, dtype=torch.int32, device=dev)
        uvd = torch.empty((P, J, 3), dtype=torch.float32, device=dev)
        xyz = torch.empty((P, J, 3), dtype=torch.float32, device=dev)
        assigned = torch.empty((3, K, B), dtype=torch.int32, device=dev)          # code, reset, source
        dropped = torch.empty(B, dtype=torch.int32, device=dev)

        def detect(seed, centers, dstatus):
            L.call("awr_detect", self._frames.data_ptr(), 0, B, self.fh, self.fw, self._idx.data_ptr(), P, D.SEED_GIVEN, seed.data_ptr(),
                   self.depth_range[0], self.depth_range[1], self.slab, self._cube.data_ptr(), 0, fx, fy, self.iters, 0, self._scratch.data_ptr(),
                   centers.data_ptr(), dstatus.data_ptr(), s)

        # the candidates: the detector over the K nearest components' seeds, in depth order
        detect(self._seed, self._cand, self._cand_status)
        if self.palm and centers_uvd is None:
            L.call("awr_detect_palm", self._frames.data_ptr(), 0, B, self.fh, self.fw, self._idx.data_ptr(), P, self._cand.data_ptr(),
                   self._cand_status.data_ptr(), self.depth_range[0], self.depth_range[1], self._cube.data_ptr(), 0, fx, fy, self.palm_search,
                   D.PALM_TAU[0], D.PALM_TAU[1], D.PALM_RHO2[0], D.PALM_RHO2[1], self._palm_scratch.data_ptr(), self._cand.data_ptr(),
                   self._cand_status.data_ptr(), self._palm_info.data_ptr(), s)
            self.palm_info = self._palm_info.view(K, B, 4)[:, :nb].transpose(0, 1)
        if self.track:
            # every slot's last centre as a given seed (a free slot's NaN seed finds nothing): where it still finds the hand the slot is held
            detect(self._track, self._tcenters, self._tstatus)
        smooth = self.smooth is not None
        L.call("awr_hands_assign", self._id_last.data_ptr(), self._id_ids.data_ptr(), self._id_miss.data_ptr(), self._id_next.data_ptr(),
               self._cand.data_ptr(), self._cand_status.data_ptr(), self._tcenters.data_ptr() if self.track else None,
               self._tstatus.data_ptr() if self.track else None, K, B, nv, cfg.gate_mm, cfg.merge_mm, cfg.max_miss, fx, fy, u0, v0, self.flip,
               self._filter_state.data_ptr() if smooth else None, self._filter_count.data_ptr() if smooth else None, J if smooth else 0,
               self._centers.data_ptr(), status.data_ptr(), L.ptr(assigned[0]), L.ptr(assigned[1]), L.ptr(assigned[2]), dropped.data_ptr(), s)

        def crop_and_predict():
            L.call("awr_detect_samples", self._centers.data_ptr(), self._cube.data_ptr(), 0, B, self._idx.data_ptr(), P, self.S, self.fh, self.fw,
                   fx, fy, u0, v0, self.flip, self._blocks.data_ptr(), L.ptr(M), L.ptr(cxyz), L.ptr(self._cube32), status.data_ptr(), s)
            self._render(self._blocks, out=self._img)
            jt = self.engine(self._img)
            L.call("awr_joints_unproject", L.ptr(jt), L.ptr(cxyz), L.ptr(M), L.ptr(self._cube32), P, J, P, float(self.S), fx, fy, u0, v0, self.flip,
                   L.ptr(uvd), L.ptr(xyz), ustatus.data_ptr(), s)

        def joints_center(joints, center_out, next_out, code):
            L.call("awr_joints_center", L.ptr(joints), self._centers.data_ptr(), L.ptr(cxyz), L.ptr(self._cube32), status.data_ptr(), ustatus.data_ptr(),
                   P, J, P, L.ptr(self._joints), 0 if self._joints is None else int(self._joints.numel()), fx, fy, u0, v0, self.flip,
                   self.depth_range[0], self.depth_range[1], self.max_shift, center_out.data_ptr(), L.ptr(next_out), code.data_ptr(), s)

        def smooth_step():
            """K launches of awr_joints_filter, one per hand block: the rows past n_valid of EVERY block keep their state"""
            scfg = self.smooth
            weighted = scfg.weight == "conf"
            conf = self.engine.conf[..., 0].contiguous() if weighted else None          # (P, J)
            out = [torch.empty((P, J, 3), dtype=torch.float32, device=dev) for _ in range(3)] + [torch.empty((P, J), dtype=torch.int32, device=dev)]
            for k in range(K):
                o = k * B
                L.call("awr_joints_filter", self._filter_state[o:].data_ptr(), self._filter_count[o:].data_ptr(), xyz[o:].data_ptr(),
                       status[o:].data_ptr(), ustatus[o:].data_ptr(), conf[o:].data_ptr() if weighted else None, B, J, nv, dt, scfg.min_cutoff,
                       scfg.beta, scfg.d_cutoff, -1.0 if scfg.gate_mm is None else scfg.gate_mm, scfg.max_coast, T.WEIGHTS[scfg.weight],
                       scfg.conf_floor, fx, fy, u0, v0, self.flip, out[0][o:].data_ptr(), out[1][o:].data_ptr(), out[2][o:].data_ptr(),
                       out[3][o:].data_ptr(), s)
            return out

        def rows(t):          # hand-major (K * B, ...) -> a (nb, K, ...) view
            return t.view((K, B) + tuple(t.shape[1:]))[:, :nb].transpose(0, 1)

        crop_and_predict()
        smoothed = None
        if self.recenter or self.track:
            codes = torch.zeros((self.recenter + 1, P), dtype=torch.int32, device=dev)
            for k in range(self.recenter):
                joints_center(xyz, self._centers, None, codes[k])
                crop_and_predict()
            nxt = torch.full((P, 3), nan, dtype=torch.float64, device=dev)
            next_from = xyz
            if smooth and self.smooth.lead:
                # the next call's crop starts where constant velocity says the hand will be: filter first, centre the look-ahead joints
                smoothed = smooth_step()
                next_from = smoothed[2]
            joints_center(next_from, self._moved, nxt, codes[self.recenter])
            # every slot's last centre becomes its joints' centre where there is one: `nxt` where finite, else what it was
            L.call("awr_centers_select", nxt.data_ptr(), self._zero_status.data_ptr(), self._id_last.data_ptr(), self._cand_status.data_ptr(), P,
                   self._sel.data_ptr(), self._sel_status.data_ptr(), None, s)
            self._id_last.view(P, 3).copy_(self._sel)
            self.centers_uvd = rows(self._centers.clone())
            self.next_centers_uvd = rows(nxt)
            self.recenter_codes = codes.view(self.recenter + 1, K, B)[:, :, :nb].transpose(1, 2)
        self._last = (status.view(K, B), ustatus.view(K, B), nv)
        n_hands = (status.view(K, B)[:, :nb] == D.OK).sum(0, dtype=torch.int32)
        self.hand_codes, self.hand_source, self.hands_dropped = rows(assigned[0].reshape(P)), rows(assigned[2].reshape(P)), dropped[:nb]
        out_xyz, out_uvd = xyz, uvd
        if smooth:
            out_xyz, out_uvd, ahead, fcodes = smoothed or smooth_step()
            self.raw_xyz, self.raw_uvd, self.ahead_xyz, self.filter_codes = rows(xyz), rows(uvd), rows(ahead), rows(fcodes)
        ids = self._id_ids[:, :nb].transpose(0, 1).clone()          # (the state moves on with the next call)
        fields = (rows(out_xyz), rows(out_uvd), rows(cxyz), rows(M), rows(status), n_hands, ids)
        if self.confidence:
            conf = torch.empty((3, P, J), dtype=torch.float32, device=dev)
            L.call("awr_confidence_fields", L.ptr(self.engine.conf), L.ptr(self.engine.stat), L.ptr(self._cube32), status.data_ptr(),
                   ustatus.data_ptr(), P, J, P, L.ptr(conf[0]), L.ptr(conf[1]), L.ptr(conf[2]), s)
            return ConfidentTrackedHandsPrediction(*fields, rows(conf[0]), rows(conf[1]), rows(conf[2]))
        return TrackedHandsPrediction(*fields)

    def check(self):
        """Synchronising: raise AwrError naming the first frame of the last batch that could not be predicted, and its status code.  With
        hands >= 2: the first frame whose slot 0 (the nearest hand) is not OK, or a found hand whose un-projection failed; an absent
        second hand is not an error.  With identity: the first frame without ANY slot that is OK; an EMPTY slot 0 is not an error."""
        if self._last is None:
            return
        status, ustatus, nv = self._last
        if self.hands > 1:
            st, ust = status[:, :nv].tolist(), ustatus[:, :nv].tolist()
            for b in range(nv):
                if self.identity is not None:      # a slot is an identity, not a depth rank: slot 0 may well be the one that is away
                    if all(st[k][b] != D.OK for k in range(self.hands)):
                        raise L.AwrError("predict: frame %d of the batch: no hand slot is OK (slot 0: %s, status %d); no hand was found and its "
                                         "joints are NaN" % (b, D.STATUS_NAMES.get(st[0][b], "invalid"), st[0][b]))
                elif st[0][b] != D.OK:
                    raise L.AwrError("predict: frame %d of the batch, hand slot 0: %s (status %d); no hand was found and its joints are NaN"
                                     % (b, D.STATUS_NAMES.get(st[0][b], "invalid"), st[0][b]))
                for k in range(self.hands):
                    if st[k][b] == D.OK and ust[k][b] != 0:
                        raise L.AwrError("predict: frame %d of the batch, hand slot %d: its crop matrix is %s (un-projection status %d); its "
                                         "joints are NaN" % (b, k, {1: "singular", 2: "not finite"}.get(ust[k][b], "invalid"), ust[k][b]))
            return
        st, ust = status[:nv].tolist(), ustatus[:nv].tolist()
        for b in range(nv):
            if st[b] != D.OK:
                raise L.AwrError("predict: frame %d of the batch: %s (status %d); its joints are NaN" % (b, D.STATUS_NAMES.get(st[b], "invalid"), st[b]))
            if ust[b] != 0:
                raise L.AwrError("predict: frame %d of the batch: its crop matrix is %s (un-projection status %d); its joints are NaN"
                                 % (b, {1: "singular", 2: "not finite"}.get(ust[b], "invalid"), ust[b]))
