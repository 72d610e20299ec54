"""Predict hand joints from raw depth frames: no dataset index, no refined-centre file, no labels.

    pred = Predictor(net, img_size=128, kernel_size=0.4, max_batch=64)
    out = pred.predict(frames)              # (B, 480, 640) uint16 millimetres: numpy, host tensor or device tensor
    out.xyz, out.uvd                        # (B, J, 3) camera millimetres / original-image uvd, on the device
    pred.check()                            # synchronises; raises AwrError naming the first frame that could not be predicted

Everything between the frames and the joints runs on the device, on the current stream, without a synchronisation; the host only issues
launches.  There is no host fallback in this class: without a GPU it raises; `awr_amd.detect.detect` is the numpy statement of the
detector for such a machine.  Every option is opt-in, and a predictor without it issues the launches and gives the bits it always did
(tests/test_predictor_trace_gpu.py holds every configuration's launches to the recorded ones).  The options, described in __init__:

    confidence=True                         conf, peak, spread_mm per joint                               DESIGN.md 4.18
    recenter=N, track=True                  crop again around the predicted joints; follow them from call to call      4.19
    views=make_views(...), fuse=            the same hand under several views in ONE batched pass, fused               4.22
    palm=True                               the detector's centre moved to the palm disc, away from the forearm        4.24
    smooth=True | dict | track.OneEuro      One-Euro filter per joint, gate, coasting, look-ahead (lead)               4.25
    hands=K                                 up to K hands per frame from connected components; a hand axis             4.26
    hands=K, identity=True | dict           slot k is the same hand from call to call; track, smooth, lead per hand    4.27
    hands=K, isolate=True                   every hand refined and cropped on a frame that holds only its component    4.28
    hands=K, edge_mm=E                      components join only within E mm of depth: a hand in front of another splits 4.29
    denoise=True | dict                     edge-preserving median, speckle removal, hole filling in front of every stage 4.30
    surface=True | dict                     per joint: on the surface the sensor saw, occluded, or off the silhouette; label-free 4.31
    background=True | dict                  a learnt static-scene model; only what is nearer than it reaches any other stage      4.32
    hands=K, edge_mm=E, link_mm=L           a rear hand's fragments rejoined across the hand in front of it            4.33

predict() is ONE pipeline over one stage method per entry point, and it reads top to bottom: upload the frames -> with background the
frames without their learnt background (awr_frames_foreground) -> with denoise the filtered
frames (awr_frames_denoise) -> the seeds (given centres | awr_detect_hands, with edge_mm awr_detect_hands_edge, with link_mm awr_detect_hands_link | the configured seed mode) -> with isolate a frame per hand (awr_hands_isolate) -> the
candidate centres (awr_detect, awr_detect_palm) -> the tracked detector (a second awr_detect) -> combine (awr_centers_select |
awr_hands_assign | nothing) -> crop and predict
(awr_detect_samples -> awr_nyu_batch -> the inference plan and the single-pass head -> awr_joints_unproject; with views awr_view_centers
and awr_view_rotate around the crop and awr_views_fuse behind it) -> the recenter passes (awr_joints_center, crop and predict) -> the next
centre, from the look-ahead joints with lead -> the tracker's state -> awr_joints_filter -> awr_confidence_fields -> with surface
awr_joints_surface -> the named tuple.
The plan's rows are group-major: G = V views or K hands, each a group of max_batch rows, group 0 first (_rows).

What is measured and what is not stands with each option in DESIGN.md: accuracy on real frames is UNMEASURED throughout (no NYU frames
and no trained checkpoint exist where this was written); the detector, the palm pass, the filter, the hands and the identities are
measured on procedural hands only (profiles/).
"""
import collections
import types

import numpy as np
import torch

from . import _lib as L
from . import background as BG
from . import detect as D
from . import detect_calls as DC
from . import nyu_data as ND
from . import surface as SF
from . import track as T

Prediction = collections.namedtuple("Prediction", "xyz uvd center_xyz M status")
ConfidentPrediction = collections.namedtuple("ConfidentPrediction", Prediction._fields + ("conf", "peak", "spread_mm"))
ViewPrediction = collections.namedtuple("ViewPrediction", Prediction._fields + ("view_spread_mm", "views_used"))
ConfidentViewPrediction = collections.namedtuple("ConfidentViewPrediction", ConfidentPrediction._fields + ("view_spread_mm", "views_used"))
HandsPrediction = collections.namedtuple("HandsPrediction", Prediction._fields + ("n_hands",))
ConfidentHandsPrediction = collections.namedtuple("ConfidentHandsPrediction", HandsPrediction._fields + ("conf", "peak", "spread_mm"))
TrackedHandsPrediction = collections.namedtuple("TrackedHandsPrediction", HandsPrediction._fields + ("ids",))
ConfidentTrackedHandsPrediction = collections.namedtuple("ConfidentTrackedHandsPrediction", TrackedHandsPrediction._fields + ("conf", "peak", "spread_mm"))
_CONFIDENT = {Prediction: ConfidentPrediction, ViewPrediction: ConfidentViewPrediction, HandsPrediction: ConfidentHandsPrediction,
              TrackedHandsPrediction: ConfidentTrackedHandsPrediction}
MAX_RECENTER = 4
MAX_VIEWS = D.MAX_VIEWS


class Predictor:
    views, fuse, V = None, "mean", 1          # a predictor without views: one identity view, no view table, no per-view buffers
    smooth = None                             # a predictor without a temporal filter: no filter state, no launch, no extra attributes
    identity = None                           # a predictor without hand identities: no assignment state, no launch, no extra attributes
    denoise = None                            # a predictor without the depth pre-filter: no raw buffer, no launch, no extra attributes
    surface = None                            # a predictor without the surface check: no bone table, no launch, no extra attributes
    background = None                         # a predictor without a background model: no model, no upload buffer, no launch, no extra attributes

    def __init__(self, net, img_size, kernel_size, cube=(300, 300, 300), paras=ND.PARAS, flip=-1, max_batch=1, frame_shape=(480, 640),
                 seed="nearest", depth_range=D.DEPTH_RANGE, slab=D.SLAB, refine_iters=D.REFINE_ITERS, winograd=None, parity=False, confidence=False,
                 recenter=0, track=False, center_joints=None, max_shift=1.0, views=None, fuse="mean", palm=False, palm_search=D.PALM_SEARCH,
                 smooth=None, hands=1, reach=D.REACH, min_pixels=D.MIN_PIXELS, identity=None, isolate=False, edge_mm=None, denoise=None,
                 background=None, link_mm=None, link_gap=D.LINK_GAP, surface=None):
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
        views, track or smooth (track and smooth: unless identity is set, below); without edge_mm touching or overlapping hands are ONE component and count as one hand; reach and min_pixels are
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
        engineering choices, UNMEASURED on real frames.
        isolate: True -- with hands >= 2, every hand gets a frame that holds only ITS component (statement:
        awr_amd.detect.isolate): awr_detect_hands writes its labels, one awr_hands_isolate launch writes K frames per frame behind the raw
        ones (the frame store grows to max_batch + K * max_batch rows), and the refinement, the palm pass, the crop and every recenter pass
        of slot k read row max_batch + k * max_batch + b instead of b -- two hands nearer than half a crop cube no longer stand in each
        other's window and crop.  With identity the candidates are refined on their isolated rows and a slot crops from the row of the
        candidate it took; a slot that follows its tracked centre, the tracker's own detector run and predict(centers_uvd=...) (which
        computes no labels) read the raw frames.  After a call `isolated` (nb, K) int32: 1 where the slot's row was an isolated frame, 0
        for a raw one and for a slot without a hand.  Refused with hands=1 and with views.  Without edge_mm touching or overlapping hands
        remain ONE component and ONE hand; UNMEASURED on real frames.
        edge_mm: None | a number of millimetres >= 0 -- with hands >= 2, the hands stage issues awr_detect_hands_edge (DESIGN.md 4.29;
        statement: awr_amd.detect.components(edge=)): two neighbouring pixels of the near foreground are joined only when their raw depths
        differ by at most edge_mm, so a hand held in front of another one is a component, a slot and (with isolate) a frame of its own.
        Everything behind the hands stage is untouched and reads its labels, seeds and info rows.  What it does not split: hands that
        touch in depth.  What it adds: an occluded hand cut into fragments by the front one gives several candidates (n_hands may be
        larger), and with isolate the fragments that are not the slot's root are removed from that hand's own frame
        (profiles/hands_overlap.txt).  No default is chosen: the right value depends on the sensor's noise, UNMEASURED on real frames.
        Refused with hands=1.
        link_mm, link_gap: None | a number of millimetres >= 0, and an int in [1, 64] (default 32) -- with hands >= 2 and edge_mm, the hands
        stage issues awr_detect_hands_link (statement: awr_amd.detect.components(edge=, link=, gap=)): a pixel with a
        run of 1 ... link_gap OCCLUDERS beside it in its row or column (non-zero pixels more than edge_mm nearer than itself) is joined
        with the first pixel behind them when that one is in the near foreground and within link_mm of its own depth, so the fragments
        the front hand cuts a rear hand into are ONE component, slot and (with isolate) frame again.  Both are handed to the hands stage
        only; everything behind it reads its labels.  Limits: a zero pixel (a sensor shadow) inside the gap breaks the link; hands that
        touch in depth stay merged; two DIFFERENT hands at similar depth with a nearer object of link_gap pixels or fewer between them
        are linked (profiles/hands_link.txt).  No default for link_mm; link_gap = 32 is an engineering choice; both UNMEASURED on real
        frames.  Refused with hands=1 and without edge_mm; link_mm=None is the predictor without it.
        denoise: None | True (awr_amd.detect.DENOISE_DEFAULTS: radius=1, edge=40.0, support=0, fill=None -- a pure edge-preserving 3 x 3
        median) | a dict with any of the keys radius (1 | 2), edge (None | millimetres >= 0), support (a pixel with fewer neighbours
        within `edge` becomes 0) and fill (None | a zero pixel with at least that many valid neighbours takes their lower median) over
        those defaults (statement: awr_amd.detect.denoise).  The frames are uploaded into a raw buffer of max_batch rows
        next to the frame store and ONE awr_frames_denoise launch writes the filtered frames into the store's rows [0, nb) before
        anything else runs: the seeds, given centres, the tracker, hands, isolate, palm, views and the crop all read the filtered
        frames, so the option combines with every other one and a prediction equals the plain predictor's on
        awr_amd.detect.denoise of each frame, bit for bit.  After a call raw_frames (nb, fh, fw) uint16 is a view of the raw buffer
        and denoise_status (nb,) int32 the launch's codes -- device tensors, nothing synchronised.  The defaults are engineering
        choices (40 mm is the edge 4.29 measured on procedural composites), UNMEASURED on real frames.
        surface: None | True (awr_amd.surface.SURFACE_DEFAULTS: radius=1, in_mm=40.0, out_mm=15.0, min_on=1, bones=None, samples=3) | a dict
        with any of the keys radius (0 ... 3), in_mm, out_mm (finite millimetres >= 0), min_on (1 ... (2 radius + 1)^2), bones (None: the
        pairs of vis_tool's skeleton for J = 14 and J = 21, none for another J | up to 64 (from, to) joint index pairs) and samples (1 ... 7)
        over those defaults (statement: awr_amd.surface.joints_surface) -- a label-free check of every joint against the
        depth frame, next to `confidence`, which is the network's opinion of itself.  A joint lies inside the hand, a few millimetres
        behind the surface the sensor sees at its pixel: it is ON (0) where at least min_on valid pixels of the (2 radius + 1)^2 window
        around its pixel lie at most in_mm in front of it and at most out_mm behind it, else OCCLUDED (1) where a pixel is more than in_mm
        in front of it -- the joint may be right, but it is unseen -- else OFF (2): only background or nothing is there, the joint floats
        off the silhouette; OUTSIDE (3) off the frame or not finite, SKIPPED (4) in a row without a prediction.  ONE awr_joints_surface
        launch behind the final pass over the joints predict() measured -- the fused ones with views, the MEASUREMENT and not the filtered
        joints with smooth -- and over the stored frames: the denoised ones with denoise, and never a hand's isolated frame, on which the
        other hand is zeroed and a joint behind it would read OFF where OCCLUDED is the truth.  After a call: surface_codes (nb, J) int32,
        surface_gap_mm (nb, J) float32 (the joint's depth minus the nearest-in-depth valid pixel of its window; NaN without one),
        surface_counts (nb, 8) int32 (joints ON / OCCLUDED / OFF / OUTSIDE, then `samples` points along every bone, linear in uvd, the
        same four) and surface_status (nb,) int32 (0, 1: the row was skipped, 2: its frame is outside the store), with the hand axis
        behind the batch axis where hands >= 2 -- device tensors, nothing synchronised.  The returned named tuples do not change and every
        other bit of a call is what it is without the option, which combines with every other one.  The defaults are engineering choices:
        on procedural hands true joints are ON or OCCLUDED and joints moved 40 mm sideways are OFF in two of three cases, but a skeleton
        laid over the wrong piece of a surface -- a crop that slid onto the forearm -- reads ON everywhere, so the counts do not rank a
        trained network's gross failures (profiles/surface_check.txt); UNMEASURED on real frames.
        background: None | True (awr_amd.background.BACKGROUND_DEFAULTS: margin=30.0, unknown="keep", adapt=None, shared=True,
        rank="median", min_valid=1) | a dict with any of those keys over the defaults (statements:
        awr_amd.background.learn and foreground) -- for a FIXED sensor with static things nearer than the hand (a table edge, a monitor,
        a knee, a torso), which every other stage would take for the hand.  The predictor keeps a model, one uint16 depth per pixel (0: no
        background known here), zeros at first; learn_background(frames) learns it from 1 ... 64 frames of the scene without a hand
        (rank: "median" the lower median of a pixel's valid depths | "min" | "max"; a pixel valid in fewer than min_valid frames stays
        0), set_background(model) takes one from outside, reset_background() zeroes it.  The frames are uploaded into a buffer of
        max_batch rows of their own and ONE awr_frames_foreground launch, in front of everything else, writes them without their
        background where every other stage reads (with denoise: its raw buffer, so the order is sensor -> foreground -> denoise): a pixel
        stays where it is at least margin millimetres nearer than the model (d + floor(margin) < m) or, with unknown="keep", where the
        model is 0, and becomes 0 otherwise.  The option combines with every other one, and a prediction equals the plain predictor's
        on awr_amd.background.foreground of each frame, bit for bit; with an all-zero model and unknown="keep" it equals the plain
        predictor's.  adapt: None | step 1 ... 65535 -- every call moves the model at most step millimetres towards the frame where the
        pixel is valid BACKGROUND (not kept, model known), in rows below n_valid: slow drift is followed, a hand is foreground and is
        never absorbed; furniture moved NEARER after learning stays foreground until the model is learnt again.  shared: True -- one
        model for every batch slot | False -- one per batch slot, where slot b is the same camera from call to call, as the tracker's
        and the filter's slots are; adapt with shared=True and max_batch > 1 is refused (several rows would step one model).  After a
        call sensor_frames (nb, fh, fw) uint16 is a view of the upload buffer and background_status (nb,) int32 the launch's codes --
        device tensors, nothing synchronised; raw_frames keeps its meaning (the frames denoise read).  The named tuples do not change.
        The defaults are engineering choices; what the option loses -- hand pixels within margin of the desk -- and what it leaves
        stand in profiles/background_accuracy.txt, procedural frames only; UNMEASURED on real frames."""
        if background is not None:
            self.background = BG.check_background_option(background)
            if self.background["adapt"] is not None and self.background["shared"] and int(max_batch) > 1:
                raise ValueError("background adapt = %d with shared=True and max_batch = %d: several rows of a batch would step ONE model "
                                 "(shared=False keeps a model per batch slot)" % (self.background["adapt"], int(max_batch)))
        if denoise is not None:
            self.denoise = D.check_denoise_option(denoise)
        if surface is not None:
            self.surface = SF.check_surface_option(surface)
            surface_bones = SF.bone_table(self.surface["bones"], int(net.J))          # (refused here, before anything is allocated)
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
        if not isinstance(isolate, bool):
            raise TypeError("isolate is True or False, not %r" % (isolate,))
        if isolate and (K == 1 or views is not None):
            raise ValueError("isolate gives each of SEVERAL hands a frame of its own component: it needs hands >= 2, and views are not combined with it")
        self.isolate, self.isolated = isolate, None
        self.edge_mm = D._check_edge(edge_mm)
        if self.edge_mm is not None and K == 1:
            raise ValueError("edge_mm is the depth test on the joins of the connected components of SEVERAL hands: it needs hands >= 2")
        if link_mm is not None and (K == 1 or self.edge_mm is None):
            D._check_link(link_mm, link_gap, 0.0)          # (a wrong type or value is named first)
            raise ValueError("link_mm rejoins a rear hand's fragments across an occluder, a pixel more than edge_mm nearer: it needs hands >= 2 and edge_mm")
        self.link_mm, self.link_gap = D._check_link(link_mm, link_gap, self.edge_mm)
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
        # (isolate: one buffer of B + K * B rows -- the raw frames, then every hand's isolated frames, hand-major)
        self._nframes = B + K * B if isolate else B
        self._all_frames = torch.empty((self._nframes, self.fh, self.fw), dtype=torch.uint16, device=dev)
        self._all_frames.view(torch.int16).zero_()
        self._frames = self._all_frames[:B]
        if self.denoise is not None:
            # the frames as they arrive; the store's rows [0, B) then hold the filtered ones
            self._raw = torch.empty((B, self.fh, self.fw), dtype=torch.uint16, device=dev)
            self._denoise_status = torch.empty(B, dtype=torch.int32, device=dev)
            self.raw_frames = self.denoise_status = None
        if self.background is not None:
            # the frames as the sensor gave them; the store's rows [0, B) (with denoise: the raw buffer) then hold them without their background
            self._sensor = torch.empty((B, self.fh, self.fw), dtype=torch.uint16, device=dev)
            self._bg_model = torch.empty((1 if self.background["shared"] else B, self.fh, self.fw), dtype=torch.uint16, device=dev)
            self._bg_model.view(torch.int16).zero_()
            self._bg_status = torch.empty(B, dtype=torch.int32, device=dev)
            self.sensor_frames = self.background_status = self.background_learn_status = None
        self._stage = torch.empty((B, self.fh, self.fw), dtype=torch.uint16).pin_memory()
        self._stage_free = None                  # event: the last upload from the staging buffer has been issued and has finished
        self._store = types.SimpleNamespace(data=self._all_frames, ftype=0, fh=self.fh, fw=self.fw, n=self._nframes)
        self._render = DV.Renderer(self._store, self.S, P)
        self._idx = torch.arange(B, dtype=torch.int64, device=dev).repeat(K)          # (K > 1: the frame of every hand-major row)
        self._cube = torch.tensor([float(c) for c in cube], dtype=torch.float64, device=dev)
        self._scratch = L.scratch("awr_detect_scratch", B * K, dtype=torch.int64, device=dev)
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
            self._palm_scratch = L.scratch("awr_detect_palm_scratch", B * K, self.fh, self.fw, dtype=torch.int32, device=dev)
            self._palm_info = torch.empty((B * K, 4), dtype=torch.int32, device=dev)
        if K > 1:
            self._hands_scratch = L.scratch("awr_detect_hands_scratch", B, self.fh, self.fw, dtype=torch.int64, device=dev)
            self._hands_status = torch.empty((K, B), dtype=torch.int32, device=dev)
            self._hands_info = torch.empty((K, B, 4), dtype=torch.int32, device=dev)
            self._hands_count = torch.empty(B, dtype=torch.int32, device=dev)
        if isolate:
            self._labels = torch.empty((B, self.fh, self.fw), dtype=torch.int32, device=dev)
            self._iso_status = torch.empty(B, dtype=torch.int32, device=dev)
            self._iso_idx = torch.arange(B, B + K * B, dtype=torch.int64, device=dev)          # the isolated frame of every hand-major row
        if smooth is not None:
            self._filter_state = torch.zeros((B * K, self.J, 6), dtype=torch.float64, device=dev)      # x0 x1 x2 d0 d1 d2 per slot (and hand) and joint
            self._filter_count = torch.zeros((B * K, self.J, 2), dtype=torch.int32, device=dev)        # age, coast
            self.raw_xyz = self.raw_uvd = self.ahead_xyz = self.filter_codes = None
        if self.surface is not None:
            self._surface_bones = torch.from_numpy(surface_bones).to(dev) if len(surface_bones) else None          # uploaded once
            self._surface_n_bones = len(surface_bones)
            self.surface_codes = self.surface_gap_mm = self.surface_counts = self.surface_status = None
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

    def _background_rows(self, slots):
        """the model rows a call names: every row for slots=None; with a shared model there is one row and slots must be None"""
        if self.background is None:
            raise L.AwrError("the background model needs a Predictor built with background=...")
        if slots is not None and self.background["shared"]:
            raise L.AwrError("slots name the models of batch slots: this predictor keeps ONE shared model (background shared=False keeps one per slot)")
        return self._slots(slots)

    def _put_background(self, model, idx):
        """a (fh, fw) device model -> the model rows idx (None: all of them)"""
        if idx is None:
            self._bg_model.copy_(model.expand_as(self._bg_model))
        else:                                    # (index operations take the bits as int16)
            self._bg_model.view(torch.int16).index_copy_(0, idx, model.view(torch.int16).expand(idx.shape[0], self.fh, self.fw))

    def learn_background(self, frames, slots=None):
        """Learn the background model from frames (n, fh, fw) uint16 of the scene WITHOUT a hand, 1 <= n <= 64, numpy or tensor, host or
        device: one awr_background_learn launch with the predictor's rank and min_valid (awr_amd.background.learn is its statement), and
        the model replaces what the predictor had.  With shared=False, slots names the batch slots that take the model (default: all of
        them).  background_learn_status (1,) int32 is the launch's status word, a device tensor.  Does not block."""
        idx = self._background_rows(slots)
        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint16:
                raise L.AwrError("frames must be uint16 millimetres, not %s" % frames.dtype)
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint16:
            raise L.AwrError("frames must be a uint16 numpy array or tensor")
        if frames.dim() != 3 or tuple(frames.shape[1:]) != (self.fh, self.fw) or not 1 <= frames.shape[0] <= BG.MAX_FRAMES:
            raise L.AwrError("frames must be (n, %d, %d) with n in [1, %d], got %s" % (self.fh, self.fw, BG.MAX_FRAMES, tuple(frames.shape)))
        o, n = self.background, int(frames.shape[0])
        if o["min_valid"] > n:
            raise L.AwrError("min_valid = %d needs at least that many frames to learn from, got %d" % (o["min_valid"], n))
        frames = frames.to(self.device, non_blocking=True).contiguous()
        model = torch.empty((self.fh, self.fw), dtype=torch.uint16, device=self.device)
        status = torch.empty(1, dtype=torch.int32, device=self.device)
        listed = torch.arange(n, dtype=torch.int64, device=self.device)
        BG.awr_background_learn(frames.data_ptr(), 0, n, self.fh, self.fw, listed.data_ptr(), n, o["rank"], o["min_valid"], model.data_ptr(),
                                status.data_ptr())
        self._put_background(model, idx)
        self.background_learn_status = status

    def set_background(self, model, slots=None):
        """Set the background model from outside: model (fh, fw) uint16, numpy or tensor, host or device (0: no background known at that
        pixel).  With shared=False, slots names the batch slots that take it (default: all of them).  Does not block."""
        idx = self._background_rows(slots)
        m = model if isinstance(model, torch.Tensor) else torch.from_numpy(np.array(model))          # (a copy: the caller's array may be read-only)
        if m.dtype != torch.uint16 or tuple(m.shape) != (self.fh, self.fw):
            raise L.AwrError("model must be (%d, %d) uint16, got %s %s" % (self.fh, self.fw, m.dtype, tuple(m.shape)))
        self._put_background(m.to(self.device, non_blocking=True), idx)

    def reset_background(self, slots=None):
        """Zero the background model (with shared=False: of batch slots `slots`, default all of them): everything is foreground again
        (with unknown="drop": nothing is).  Does not block."""
        idx = self._background_rows(slots)
        if idx is None:
            self._bg_model.view(torch.int16).zero_()
        else:
            self._bg_model.view(torch.int16).index_fill_(0, idx, 0)

    @property
    def background_model(self):
        """the model store, a device tensor: (1, fh, fw) uint16 with shared=True, else (max_batch, fh, fw), row b the model of batch slot b"""
        if self.background is None:
            raise L.AwrError("background_model needs a Predictor built with background=...")
        return self._bg_model

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

    # ---- one call: the row layout, the call's tensors, one stage per entry point, predict() -------------------------------
    # The plan has R = max_batch * V * K rows, group-major: G = V views or K hands, each a group of max_batch rows, group 0 first.  The
    # detector's buffers have F = max_batch * K rows (F == R unless there are views).  A stage takes the rows it is launched over, how many
    # of them are valid and the tensors it reads and writes; the camera, the depth range, the cube, the frame store and the stream are self's.

    def _rows(self, t, nb, axis=0, group_first=False):
        """What a result carries of a group-major (G * max_batch, ...) buffer whose rows lie along `axis`: with hands its (nb, K, ...) view,
        else the nb rows of group 0 (the only group, or view 0).  group_first: the (G, nb, ...) view."""
        if self.hands == 1 and not group_first:
            return t.narrow(axis, 0, nb)
        t = t.view(tuple(t.shape[:axis]) + (-1, self.B) + tuple(t.shape[axis + 1:])).narrow(axis + 1, 0, nb)
        return t if group_first else t.transpose(axis, axis + 1)

    def _tensors(self, nb, nv):
        """Everything one call allocates, and its row counts.  F, fv: the detector's rows and how many of them are valid -- hands = 1 launches
        over (max_batch, n_valid) and needs a zeroed status, hands >= 2 over (F, F): its rows past n_valid have NaN seeds and end EMPTY by
        themselves.  R, rv: the same for the plan's rows, (R, R) unless the plan is one group.  xyz_j / uvd_j / status_j are the joints and
        codes the stages behind the crop read: the fused ones with views."""
        dev, B, K, J = self.device, self.B, self.hands, self.J
        F, R = B * K, B * K * self.V
        c = types.SimpleNamespace(nb=nb, nv=nv, F=F, R=R, fv=nv if K == 1 else F, rv=nv if R == B else R, weights=None, filtered=None)
        c.M = torch.empty((R, 3, 3), dtype=torch.float32, device=dev)
        c.cxyz = torch.empty((R, 3), dtype=torch.float32, device=dev)
        c.status = torch.zeros(B, dtype=torch.int32, device=dev) if K == 1 else torch.empty(F, dtype=torch.int32, device=dev)
        c.ustatus = torch.zeros(R, dtype=torch.int32, device=dev)
        c.uvd = torch.empty((R, J, 3), dtype=torch.float32, device=dev)
        c.xyz = torch.empty((R, J, 3), dtype=torch.float32, device=dev)
        c.xyz_j, c.uvd_j, c.status_j = c.xyz, c.uvd, c.status
        if self.V > 1:
            # status: the frames' (the detector's); vstatus: one per row, view 0's first -- what every later stage and check() read
            c.vstatus = torch.zeros(R, dtype=torch.int32, device=dev)
            c.fxyz = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
            c.fuvd = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
            c.vspread = torch.empty((B, J), dtype=torch.float32, device=dev)
            c.vused = torch.empty((B, J), dtype=torch.int32, device=dev)
            c.xyz_j, c.uvd_j, c.status_j = c.fxyz, c.fuvd, c.vstatus
        if self.identity is not None:
            c.assigned = torch.empty((3, F), dtype=torch.int32, device=dev)          # code, reset, source
            c.dropped = torch.empty(B, dtype=torch.int32, device=dev)
        if self.recenter or self.track:
            c.codes = torch.zeros((self.recenter + 1, F), dtype=torch.int32, device=dev)
            c.nxt = torch.full((F, 3), float("nan"), dtype=torch.float64, device=dev)
        if self.confidence:
            c.fields = torch.empty((3, F, J), dtype=torch.float32, device=dev)
        if self.surface is not None:
            c.surface = (torch.empty((F, J), dtype=torch.int32, device=dev), torch.empty((F, J), dtype=torch.float32, device=dev),
                         torch.empty((F, 8), dtype=torch.int32, device=dev), torch.empty(F, dtype=torch.int32, device=dev))
        return c

    def _frames_foreground(self, nb, nv):
        """rows [0, nb) of the upload buffer -> rows [0, nb) of what the next stage reads, without their background; rows below nv adapt"""
        o = self.background
        out = self._frames if self.denoise is None else self._raw
        BG.awr_frames_foreground(self._sensor.data_ptr(), 0, self.B, self.fh, self.fw, self._idx.data_ptr(), nb, nv, self._bg_model.data_ptr(),
                                 self._bg_model.shape[0], not o["shared"], o["margin"], o["unknown"], o["adapt"], out.data_ptr(),
                                 self._bg_status.data_ptr())
        self.sensor_frames, self.background_status = self._sensor[:nb], self._bg_status[:nb]

    def _frames_denoise(self, nb):
        """rows [0, nb) of the raw buffer -> rows [0, nb) of the frame store, filtered"""
        o = self.denoise
        DC.awr_frames_denoise(self._raw.data_ptr(), 0, self.B, self.fh, self.fw, self._idx.data_ptr(), nb, o["radius"], o["edge"], o["support"],
                              o["fill"], self._frames.data_ptr(), self._denoise_status.data_ptr())
        self.raw_frames, self.denoise_status = self._raw[:nb], self._denoise_status[:nb]

    def _detect(self, n, seed, seed_centers, centers, status, frame):
        DC.awr_detect(self._frames.data_ptr(), 0, self._nframes, self.fh, self.fw, frame.data_ptr(), n, seed, L.ptr(seed_centers), self.depth_range,
                      self.slab, self._cube.data_ptr(), False, self.paras, self.iters, 0, self._scratch.data_ptr(), centers.data_ptr(), status.data_ptr())

    def _detect_palm(self, n, nb, centers, status, frame):
        """in place: a frame that is not OK keeps its centre and status"""
        DC.awr_detect_palm(self._frames.data_ptr(), 0, self._nframes, self.fh, self.fw, frame.data_ptr(), n, centers.data_ptr(), status.data_ptr(),
                           self.depth_range, self._cube.data_ptr(), False, self.paras, self.palm_search, D.PALM_TAU, D.PALM_RHO2,
                           self._palm_scratch.data_ptr(), centers.data_ptr(), status.data_ptr(), self._palm_info.data_ptr())
        self.palm_info = self._rows(self._palm_info, nb)

    def _detect_hands(self, nb):
        """the K nearest components' seeds of every frame -> self._seed, hand-major"""
        DC.awr_detect_hands(self._frames.data_ptr(), 0, self.B, self.fh, self.fw, self._idx.data_ptr(), self.B, self.hands, self.depth_range, self.reach,
                            self.edge_mm, self.slab, self.min_pixels, self._hands_scratch.data_ptr(), self._labels.data_ptr() if self.isolate else None,
                            self._seed.data_ptr(), self._hands_status.data_ptr(), self._hands_info.data_ptr(), self._hands_count.data_ptr(),
                            link=self.link_mm, gap=self.link_gap)
        self.hand_info = self._hands_info[:, :nb].transpose(0, 1)

    def _hands_isolate(self):
        """the raw frames, their labels and the slots' info rows -> rows [B, B + K * B) of the frame store: a frame per hand, hand-major"""
        DC.awr_hands_isolate(self._frames.data_ptr(), 0, self.B, self.fh, self.fw, self._idx.data_ptr(), self.B, self.hands, self._labels.data_ptr(),
                             self._hands_info.data_ptr(), self._all_frames[self.B:].data_ptr(), self._iso_status.data_ptr())

    def _centers_select(self, n, first, first_status, second, second_status, out, out_status):
        """per row `first` where its status is OK, else `second`"""
        DC.awr_centers_select(first.data_ptr(), first_status.data_ptr(), second.data_ptr(), second_status.data_ptr(), n, out.data_ptr(),
                              out_status.data_ptr(), None)

    def _hands_assign(self, c):
        """the candidates (and the tracked centres) -> every slot's centre and status, in self._centers / c.status; the state moves on"""
        smooth = self.smooth is not None
        DC.awr_hands_assign(self._id_last.data_ptr(), self._id_ids.data_ptr(), self._id_miss.data_ptr(), self._id_next.data_ptr(), self._cand.data_ptr(),
                            self._cand_status.data_ptr(), self._tcenters.data_ptr() if self.track else None,
                            self._tstatus.data_ptr() if self.track else None, self.hands, self.B, c.nv, self.identity, self.paras, self.flip,
                            self._filter_state.data_ptr() if smooth else None, self._filter_count.data_ptr() if smooth else None,
                            self.J if smooth else 0, self._centers.data_ptr(), c.status.data_ptr(), L.ptr(c.assigned[0]), L.ptr(c.assigned[1]),
                            L.ptr(c.assigned[2]), c.dropped.data_ptr())

    def _detect_samples(self, n, c, centers, cubes, cube_rows, frame, status):
        """centres -> crop blocks, crop matrices, centres in camera space, float cubes"""
        DC.awr_detect_samples(centers.data_ptr(), cubes.data_ptr(), cube_rows, self._nframes, frame.data_ptr(), n, self.S, self.fh, self.fw, self.paras,
                              self.flip, self._blocks.data_ptr(), L.ptr(c.M), L.ptr(c.cxyz), L.ptr(self._cube32), status.data_ptr())

    def _joints_unproject(self, n, nv, jt, c):
        DC.awr_joints_unproject(L.ptr(jt), L.ptr(c.cxyz), L.ptr(c.M), L.ptr(self._cube32), n, self.J, nv, self.S, self.paras, self.flip, L.ptr(c.uvd),
                                L.ptr(c.xyz), c.ustatus.data_ptr())

    def _view_centers(self, c):
        """the centres -> one centre, cube and frame row per view, and the rows' status"""
        DC.awr_view_centers(self._centers.data_ptr(), c.status.data_ptr(), self._cube.data_ptr(), False, self._vtable.data_ptr(), self.V, self.B, c.nv,
                            self.paras, self.flip, self._vcenters.data_ptr(), self._vcubes.data_ptr(), self._vframe.data_ptr(), c.vstatus.data_ptr())

    def _view_rotate(self, c):
        DC.awr_view_rotate(self._blocks.data_ptr(), L.ptr(c.M), c.vstatus.data_ptr(), self._vtable.data_ptr(), self.V, self.B, c.nv)

    def _views_fuse(self, c):
        DC.awr_views_fuse(L.ptr(c.xyz), c.vstatus.data_ptr(), c.ustatus.data_ptr(), L.ptr(c.weights), self.fuse, self.V, self.B, self.J, c.nv, self.paras,
                          self.flip, L.ptr(c.fxyz), L.ptr(c.fuvd), L.ptr(c.vspread), L.ptr(c.vused))

    def _joints_center(self, c, joints, center_out, next_out, code):
        """the joints' centre per frame row, gated (see __init__): moved rows into center_out, every row's into next_out (NaN: not moved)"""
        DC.awr_joints_center(L.ptr(joints), self._centers.data_ptr(), L.ptr(c.cxyz), L.ptr(self._cube32), c.status_j.data_ptr(), c.ustatus.data_ptr(),
                             c.F, self.J, c.fv, None if self._joints is None else (self._joints.data_ptr(), self._joints.numel()), self.paras, self.flip,
                             self.depth_range, self.max_shift, center_out.data_ptr(), L.ptr(next_out), code.data_ptr())

    def _joints_filter(self, c, dt):
        """awr_joints_filter over the call's joints, one launch per group of max_batch rows (the rows past n_valid of EVERY group keep their
        state) -> c.filtered = (xyz, uvd, ahead (F, J, 3), code (F, J)), fresh tensors"""
        cfg, B, J, dev = self.smooth, self.B, self.J, self.device
        conf = None
        if cfg.weight == "conf":          # (F, J): the views' weights where there are some, else the head's conf; view 0's rows come first
            conf = c.weights if c.weights is not None else self.engine.conf[:c.F, :, 0].contiguous()
        out = [torch.empty((c.F, J, 3), dtype=torch.float32, device=dev) for _ in range(3)] + [torch.empty((c.F, J), dtype=torch.int32, device=dev)]
        for o in range(0, c.F, B):
            DC.awr_joints_filter(self._filter_state[o:].data_ptr(), self._filter_count[o:].data_ptr(), c.xyz_j[o:].data_ptr(), c.status_j[o:].data_ptr(),
                                 c.ustatus[o:].data_ptr(), None if conf is None else conf[o:].data_ptr(), B, J, c.nv, dt, cfg, self.paras, self.flip,
                                 out[0][o:].data_ptr(), out[1][o:].data_ptr(), out[2][o:].data_ptr(), out[3][o:].data_ptr())
        c.filtered = out

    def _confidence_fields(self, c):
        """conf, peak, spread_mm of every frame row (with views: view 0's rows are the first of every per-row buffer) -> c.fields"""
        DC.awr_confidence_fields(L.ptr(self.engine.conf), L.ptr(self.engine.stat), L.ptr(self._cube32), c.status_j.data_ptr(), c.ustatus.data_ptr(),
                                 c.F, self.J, c.fv, L.ptr(c.fields[0]), L.ptr(c.fields[1]), L.ptr(c.fields[2]))

    def _joints_surface(self, c):
        """the call's joints (the measurement; with views the fused ones and view 0's codes) against the STORED frame of every frame row ->
        c.surface = (codes, gap_mm (F, J), counts (F, 8), row_status (F,)) and the after-call attributes"""
        o = self.surface
        SF.awr_joints_surface(self._frames.data_ptr(), 0, self.B, self.fh, self.fw, self._idx.data_ptr(), L.ptr(c.uvd_j), c.status_j.data_ptr(),
                              c.ustatus.data_ptr(), c.F, self.J, c.fv, L.ptr(self._surface_bones), self._surface_n_bones, o["samples"], o["radius"],
                              o["in_mm"], o["out_mm"], o["min_on"], *(L.ptr(t) for t in c.surface))
        self.surface_codes, self.surface_gap_mm, self.surface_counts, self.surface_status = (self._rows(t, c.nb) for t in c.surface)

    def _crop_and_predict(self, c):
        """self._centers -> c.xyz / c.uvd (with views: and the fused c.fxyz / c.fuvd): crop, render, the network, un-projection"""
        if self.V > 1:
            # one centre, cube and frame row per view; the rows past n_valid of each view hold NaN centres: blocks without pixels
            if c.nv < self.B:
                self._vcenters.fill_(float("nan"))
            self._view_centers(c)
            self._detect_samples(c.R, c, self._vcenters, self._vcubes, True, self._vframe, c.vstatus)
            self._view_rotate(c)
        else:
            self._detect_samples(c.fv, c, self._centers, self._cube, False, c.frame, c.status)
        if c.R == self.B:
            self._render(self._blocks[:c.nv], out=self._img[:c.nv])
            if c.nv < self.B:
                self._img[c.nv:].zero_()          # padding rows of the static plan: constant input, and no later stage reads their output
        else:
            self._render(self._blocks, out=self._img)
        self._joints_unproject(c.R, c.rv, self.engine(self._img), c)
        if self.V > 1:
            if self.fuse == "conf":
                c.weights = self.engine.conf[..., 0].contiguous()          # (R, J): the head's conf of every row, packed
            self._views_fuse(c)

    def _upload(self, frames):
        """(nb, fh, fw) uint16 -> rows [0, nb) of the frame store (with denoise: of the raw buffer; with background: of its upload buffer),
        without blocking"""
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
        staged = not frames.is_cuda and not frames.is_pinned()
        if staged:
            # pageable memory -> the pinned staging buffer -> HBM.  The buffer is reused: wait for the previous upload FROM IT (a copy, not
            # the pipeline: the launches behind it stay queued)
            if self._stage_free is not None:
                self._stage_free.synchronize()
            self._stage[:nb].copy_(frames)
            frames = self._stage[:nb]
        if self.background is not None:
            self._sensor[:nb].copy_(frames, non_blocking=True)
        else:
            (self._frames if self.denoise is None else self._raw)[:nb].copy_(frames, non_blocking=True)
        if staged:
            self._stage_free = torch.cuda.Event()
            self._stage_free.record()
        return nb

    def _given_centers(self, centers_uvd, nb):
        """centers_uvd (nb, 3), with hands (nb, K, 3) -> rows [0, nb) of every group of self._seed (converts to float64 on the way)"""
        K = self.hands
        c = centers_uvd if isinstance(centers_uvd, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(centers_uvd, dtype=np.float64))
        if K == 1 and tuple(c.shape) != (nb, 3):
            raise L.AwrError("centers_uvd must be (%d, 3), got %s" % (nb, tuple(c.shape)))
        if K > 1 and tuple(c.shape) != (nb, K, 3):
            raise L.AwrError("centers_uvd must be (%d, %d, 3): a centre per frame and hand, NaN rows for an absent hand, got %s" % (nb, K, tuple(c.shape)))
        self._rows(self._seed, nb, group_first=True).copy_(c if K == 1 else c.transpose(0, 1), non_blocking=True)

    def predict(self, frames, centers_uvd=None, n_valid=None, dt=None):
        """-> Prediction(xyz (nb, J, 3), uvd (nb, J, 3), center_xyz (nb, 3), M (nb, 3, 3), status (nb,) int32), device tensors, nothing
        synchronised; with confidence=True a ConfidentPrediction: these and conf, peak, spread_mm (nb, J); with views, hands or identity the
        named tuples __init__ describes.  centers_uvd (nb, 3), with hands (nb, K, 3): hand centres in original-image uvd (numpy or tensor)
        instead of the detector's seed.  n_valid: frames of the batch that count (default: all of them); rows past it hold unspecified values.
        status: awr_amd.detect's codes; a frame that is not OK has NaN rows (of conf / peak / spread_mm too).  With recenter > 0 every field
        is the FINAL pass's; with track=True a call without centers_uvd starts from the tracked centres (see __init__), an explicit
        centers_uvd overrides them for this call (with identity: it is the candidates), and either way slots [0, n_valid) of the tracker take
        this call's next_centers_uvd.  dt: seconds since the previous call, for a predictor with smooth (default 1 / its fps); xyz and uvd are
        then the filtered joints (see __init__)."""
        K, B, nan = self.hands, self.B, float("nan")
        if self.smooth is not None:
            dt = T.check_dt(1.0 / self.smooth.fps if dt is None else dt)
        elif dt is not None:
            raise L.AwrError("predict(dt=...) is the temporal filter's time step: it needs a Predictor built with smooth=...")
        nb = self._upload(frames)
        nv = nb if n_valid is None else int(n_valid)
        if not 0 < nv <= nb:
            raise L.AwrError("n_valid = %d is outside [1, %d]" % (nv, nb))
        if self.background is not None:
            self._frames_foreground(nb, nv)          # (in front of the filter: the sensor's frames -> foreground -> denoise -> every other stage)
        if self.denoise is not None:
            self._frames_denoise(nb)          # (in front of the seeds, given centres and the tracker alike: every stage reads the filtered frames)
        # the seeds: given centres, the K nearest components, or the configured seed mode
        given = centers_uvd is not None
        mode, seed = ("given", self._seed) if given or K > 1 else (self.seed, None)
        if given:
            self._given_centers(centers_uvd, nb)
            self.hand_info = None
        elif K > 1:
            self._detect_hands(nb)
        # the frame of every detector row: the raw one, or with isolate the hand's own (given centres come without labels: raw frames)
        isolated = self.isolate and not given
        frame = self._idx
        if isolated:
            self._hands_isolate()
            frame = self._iso_idx
        if K > 1 and nv < B:
            self._seed.view(K, B, 3)[:, nv:].fill_(nan)          # rows past n_valid of every group: NaN seeds, blocks without pixels
        c = self._tensors(nb, nv)
        c.frame = frame
        # the candidate centres, where configured through the palm pass, and the tracked detector: seeded with the centres the previous
        # call left (a lost slot's NaN seed finds nothing).  Hands without identities have nothing to combine: the candidates are the centres
        tracked = self.track and (K > 1 or not given)
        cand, cand_status = self._centers, c.status
        if tracked and K == 1:
            cand, cand_status = self._dcenters, self._dstatus
            self._detect(c.fv, "given", self._track, self._tcenters, self._tstatus, self._idx)          # (one slot: the tracker goes first)
        elif self.identity is not None:
            cand, cand_status = self._cand, self._cand_status
        self._detect(c.fv, mode, seed, cand, cand_status, frame)
        if self.palm and not given:
            self._detect_palm(c.fv, nb, cand, cand_status, frame)
        if tracked and K > 1:
            # (on the RAW frames, also with isolate: which component a tracked centre belongs to is not decided here)
            self._detect(c.fv, "given", self._track, self._tcenters, self._tstatus, self._idx)
        # combine them: per slot the tracked centre where it holds, else the detector's; with identities the assignment
        if tracked and K == 1:
            self._centers_select(nv, self._tcenters, self._tstatus, cand, cand_status, self._centers, c.status)
        elif self.identity is not None:
            self._hands_assign(c)
            if isolated:
                # a slot crops from the isolated frame of the candidate it took; one that follows its tracked centre, or has none, from the raw frame
                source = c.assigned[2].to(torch.int64)
                c.frame = torch.where(source >= 0, self._idx + B + source * B, self._idx)
        self._crop_and_predict(c)
        if self.recenter or self.track:
            for k in range(self.recenter):
                # moved frames get their new centre in place, the others keep theirs: their next pass repeats this one bit for bit
                self._joints_center(c, c.xyz_j, self._centers, None, c.codes[k])
                self._crop_and_predict(c)
            next_from = c.xyz_j
            if self.smooth is not None and self.smooth.lead:
                # the next call's crop starts where constant velocity says the hand will be: filter first, centre the look-ahead joints
                self._joints_filter(c, dt)
                next_from = c.filtered[2]
            self._joints_center(c, next_from, self._moved, c.nxt, c.codes[self.recenter])
            if self.identity is not None:
                # every slot's last centre becomes its joints' centre where there is one: `nxt` where finite, else what it was
                self._centers_select(c.F, c.nxt, self._zero_status, self._id_last, self._cand_status, self._sel, self._sel_status)
                self._id_last.view(c.F, 3).copy_(self._sel)
            self.centers_uvd = self._rows(self._centers.clone(), nb)
            self.next_centers_uvd, self.recenter_codes = self._rows(c.nxt, nb), self._rows(c.codes, nb, axis=1)
            if self.track and K == 1:
                self._track[:nv].copy_(c.nxt[:nv])
        self._last = (c.status_j, c.ustatus, nv) if K == 1 else (c.status.view(K, B), c.ustatus.view(K, B), nv)
        if self.smooth is not None and c.filtered is None:
            self._joints_filter(c, dt)
        if self.confidence:
            self._confidence_fields(c)
        if self.surface is not None:
            self._joints_surface(c)
        if self.isolate:
            self.isolated = self._rows(((c.frame >= B) & (c.status == D.OK)).to(torch.int32), nb)
        return self._result(c, given)

    def _result(self, c, given):
        """the call's named tuple, picked by (views, hands, identity, confidence), and the after-call attributes"""
        K, nb = self.hands, c.nb
        xyz, uvd = c.xyz_j, c.uvd_j
        if self.smooth is not None:
            xyz, uvd, ahead, codes = c.filtered
            self.raw_xyz, self.raw_uvd = self._rows(c.xyz_j, nb), self._rows(c.uvd_j, nb)
            self.ahead_xyz, self.filter_codes = self._rows(ahead, nb), self._rows(codes, nb)
        fields = [self._rows(t, nb) for t in (xyz, uvd, c.cxyz, c.M, c.status_j)]
        kind = Prediction
        if K > 1:
            kind = HandsPrediction
            if given or self.identity is not None:
                fields.append((self._rows(c.status, nb, group_first=True) == D.OK).sum(0, dtype=torch.int32))
            else:
                fields.append(self._hands_count[:nb].clamp(max=K))
        if self.identity is not None:
            kind = TrackedHandsPrediction
            self.hand_codes, self.hand_source, self.hands_dropped = self._rows(c.assigned[0], nb), self._rows(c.assigned[2], nb), c.dropped[:nb]
            fields.append(self._id_ids[:, :nb].transpose(0, 1).clone())          # (the state moves on with the next call)
        if self.confidence:
            fields += [self._rows(f, nb) for f in c.fields]
        if self.V > 1:
            kind = ViewPrediction
            per_view = dict(xyz=c.xyz, uvd=c.uvd, M=c.M, center_xyz=c.cxyz, cube=self._cube32, status=c.vstatus, ustatus=c.ustatus)
            if self.engine.conf is not None:
                per_view["conf"] = self.engine.conf[..., 0] if c.weights is None else c.weights
            self.view_outputs = types.SimpleNamespace(**{name: self._rows(t, nb, group_first=True) for name, t in per_view.items()})
            fields += [c.vspread[:nb], c.vused[:nb]]
        return (_CONFIDENT[kind] if self.confidence else kind)(*fields)

    def check(self):
        """Synchronising: raise AwrError naming the first frame of the last batch that could not be predicted, and its status code.  With
        hands >= 2: the first frame whose slot 0 (the nearest hand) is not OK, or a found hand whose un-projection failed; an absent
        second hand is not an error.  With identity: the first frame without ANY slot that is OK; an EMPTY slot 0 is not an error."""
        if self._last is None:
            return
        status, ustatus, nv = self._last
        K = self.hands
        st, ust = (t.view(-1, self.B)[:K, :nv].tolist() for t in (status, ustatus))          # (G, nv); with views only view 0's rows are read
        slot0, absent = (", hand slot 0", "no hand was found and ") if K > 1 else ("", "")
        for b in range(nv):
            if self.identity is not None:      # a slot is an identity, not a depth rank: slot 0 may well be the one that is away
                if all(st[k][b] != D.OK for k in range(K)):
                    raise L.AwrError("predict: frame %d of the batch: no hand slot is OK (slot 0: %s, status %d); no hand was found and its "
                                     "joints are NaN" % (b, D.STATUS_NAMES.get(st[0][b], "invalid"), st[0][b]))
            elif st[0][b] != D.OK:
                raise L.AwrError("predict: frame %d of the batch%s: %s (status %d); %sits joints are NaN"
                                 % (b, slot0, D.STATUS_NAMES.get(st[0][b], "invalid"), st[0][b], absent))
            for k in range(K):
                if st[k][b] == D.OK and ust[k][b] != 0:
                    raise L.AwrError("predict: frame %d of the batch%s: its crop matrix is %s (un-projection status %d); its joints are NaN"
                                     % (b, ", hand slot %d" % k if K > 1 else "", {1: "singular", 2: "not finite"}.get(ust[k][b], "invalid"), ust[k][b]))
