"""The detector's, the tracker's and the predictor's own launches (include/awr_hip.h from "Hand detection on the device" on), each entry
point's argument list stated once.

Plain functions, one per entry point and named after it: the values in ABI order, the float() / int() conversions, the stream, one L.call.
Buffers are device addresses (int; None: NULL) -- L.ptr(t) of a tensor a user handed to a wrapper in detect.py / track.py, t.data_ptr() of
one the Predictor allocated itself; both launch through here, so the list the operator tests prove is the list the product path runs.
Nothing is allocated, validated or computed.  A frame source is its five parts: frames (address), ftype, n_frames, fh, fw.  The conventions:
    edge=None -> +inf (no depth test), and awr_detect_hands instead of awr_detect_hands_edge        fill=None -> 0 (no filling)
    link=None -> the call above; a link -> awr_detect_hands_link, gap=None -> detect.LINK_GAP
    cfg.gate_mm=None (the filter's) -> -1.0 (no gate)                                                joints=None -> (NULL, 0): all joints
    cube_rows: False -> stride 0, one cube for every row | True -> stride 3, an (n, 3) table         the camera: fx, fy, u0, v0, then flip
    seed, fuse and cfg.weight are the names of detect.SEEDS, detect.FUSE_MODES and track.WEIGHTS"""
from . import _lib as L
from .detect import FUSE_MODES, LINK_GAP, SEEDS
from .track import WEIGHTS


def _camera(paras, flip):
    return float(paras[0]), float(paras[1]), float(paras[2]), float(paras[3]), int(flip)


def awr_frames_denoise(frames, ftype, n_frames, fh, fw, frame_idx, n, radius, edge, support, fill, out, status):
    """n frames of the source, filtered -> out (n, fh, fw) uint16"""
    L.call("awr_frames_denoise", frames, int(ftype), int(n_frames), int(fh), int(fw), frame_idx, int(n), int(radius),
           float("inf") if edge is None else float(edge), int(support), 0 if fill is None else int(fill), out, status, L.stream())


def awr_detect(frames, ftype, n_frames, fh, fw, frame_idx, n, seed, seed_centers, depth_range, slab, cube, cube_rows, paras, iters, parts, scratch,
               centers, status):
    """the seed (seed_centers where it is "given") refined iters times -> centers (n, 3) float64, status (n,)"""
    L.call("awr_detect", frames, int(ftype), int(n_frames), int(fh), int(fw), frame_idx, int(n), SEEDS[seed], seed_centers, float(depth_range[0]),
           float(depth_range[1]), float(slab), cube, 3 if cube_rows else 0, float(paras[0]), float(paras[1]), int(iters), int(parts), scratch, centers,
           status, L.stream())


def awr_detect_palm(frames, ftype, n_frames, fh, fw, frame_idx, n, centers, status, depth_range, cube, cube_rows, paras, search, tau, rho2, scratch,
                    center_out, status_out, info):
    """detector centres -> the centres of the palm discs (the outputs may be the inputs); info (n, 4) int32 or NULL"""
    L.call("awr_detect_palm", frames, int(ftype), int(n_frames), int(fh), int(fw), frame_idx, int(n), centers, status, float(depth_range[0]),
           float(depth_range[1]), cube, 3 if cube_rows else 0, float(paras[0]), float(paras[1]), float(search), int(tau[0]), int(tau[1]), int(rho2[0]),
           int(rho2[1]), scratch, center_out, status_out, info, L.stream())


def awr_detect_hands(frames, ftype, n_frames, fh, fw, frame_idx, n, hands, depth_range, reach, edge, slab, min_pixels, scratch, labels, centers, status,
                     info, count, *, link=None, gap=None):
    """the K nearest components' seeds, hand-major; labels (n, fh, fw) int32 or NULL.  edge: None | the join's depth test in millimetres;
    link: None | the depth agreement of a link across an occluder in millimetres, gap: the occluders a link crosses at the most"""
    head = (frames, int(ftype), int(n_frames), int(fh), int(fw), frame_idx, int(n), int(hands), float(depth_range[0]), float(depth_range[1]), float(reach))
    tail = (float(slab), int(min_pixels), scratch, labels, centers, status, info, count, L.stream())
    if link is not None:
        L.call("awr_detect_hands_link", *head, float("inf") if edge is None else float(edge), float(link), LINK_GAP if gap is None else int(gap), *tail)
    elif edge is None:
        L.call("awr_detect_hands", *head, *tail)
    else:
        L.call("awr_detect_hands_edge", *head, float(edge), *tail)


def awr_hands_isolate(frames, ftype, n_frames, fh, fw, frame_idx, n, hands, labels, info, out, status):
    """the frames, their labels and the slots' info rows -> out (K * n, fh, fw) uint16: a frame per hand, hand-major"""
    L.call("awr_hands_isolate", frames, int(ftype), int(n_frames), int(fh), int(fw), frame_idx, int(n), int(hands), labels, info, out, status, L.stream())


def awr_centers_select(a_center, a_status, b_center, b_status, n, out, out_status, which):
    """per row `a` where its status is OK and its centre finite, else `b`; which (n,) int32 or NULL"""
    L.call("awr_centers_select", a_center, a_status, b_center, b_status, int(n), out, out_status, which, L.stream())


def awr_hands_assign(last_uvd, ids, miss, next_id, cand_uvd, cand_status, trk_uvd, trk_status, hands, B, n_valid, cfg, paras, flip, filter_state,
                     filter_count, J, centers, status, code, reset, source, dropped):
    """cfg: a track.Identity.  trk_uvd / trk_status and filter_state / filter_count (with its J, else 0) may be NULL"""
    L.call("awr_hands_assign", last_uvd, ids, miss, next_id, cand_uvd, cand_status, trk_uvd, trk_status, int(hands), int(B), int(n_valid),
           float(cfg.gate_mm), float(cfg.merge_mm), int(cfg.max_miss), *_camera(paras, flip), filter_state, filter_count, int(J), centers, status, code,
           reset, source, dropped, L.stream())


def awr_detect_samples(centers, cube, cube_rows, n_frames, frame_idx, n, dsize, fh, fw, paras, flip, blocks, M, center_xyz, cube32, status):
    """centres -> crop blocks, crop matrices, centres in camera space, float cubes"""
    L.call("awr_detect_samples", centers, cube, 3 if cube_rows else 0, int(n_frames), frame_idx, int(n), int(dsize), int(fh), int(fw),
           *_camera(paras, flip), blocks, M, center_xyz, cube32, status, L.stream())


def awr_joints_unproject(jt, center_xyz, M, cube32, n, J, n_valid, img_size, paras, flip, uvd, xyz, status):
    """normalised joints -> uvd, xyz (n, J, 3) of the first n_valid rows"""
    L.call("awr_joints_unproject", jt, center_xyz, M, cube32, int(n), int(J), int(n_valid), float(img_size), *_camera(paras, flip), uvd, xyz, status,
           L.stream())


def awr_view_centers(centers, status, cube, cube_rows, table, V, B, n_valid, paras, flip, vcenters, vcubes, vframe, vstatus):
    """the centres -> one centre, cube and frame row per view, and the rows' status, view-major"""
    L.call("awr_view_centers", centers, status, cube, 3 if cube_rows else 0, table, int(V), int(B), int(n_valid), *_camera(paras, flip), vcenters,
           vcubes, vframe, vstatus, L.stream())


def awr_view_rotate(blocks, M, status, table, V, B, n_valid):
    """the rotating views' blocks and crop matrices, patched in place"""
    L.call("awr_view_rotate", blocks, M, status, table, int(V), int(B), int(n_valid), L.stream())


def awr_views_fuse(xyz, status, ustatus, weights, fuse, V, B, J, n_valid, paras, flip, fxyz, fuvd, spread, used):
    """the views' joints -> the fused ones; weights (V * B, J) float32, read by "conf" alone, or NULL.  fuse: a name, or a code as it is"""
    L.call("awr_views_fuse", xyz, status, ustatus, weights, FUSE_MODES[fuse] if fuse in FUSE_MODES else int(fuse), int(V), int(B), int(J),
           int(n_valid), *_camera(paras, flip), fxyz, fuvd, spread, used, L.stream())


def awr_joints_center(xyz, center_uvd, center_xyz, cube32, status, ustatus, n, J, n_valid, joints, paras, flip, depth_range, max_shift, center_out,
                      next_out, code):
    """the joints' centre per row, gated.  joints: None | (address of int32 indices, how many)"""
    L.call("awr_joints_center", xyz, center_uvd, center_xyz, cube32, status, ustatus, int(n), int(J), int(n_valid),
           *((None, 0) if joints is None else (joints[0], int(joints[1]))), *_camera(paras, flip), float(depth_range[0]), float(depth_range[1]),
           float(max_shift), center_out, next_out, code, L.stream())


def awr_joints_filter(state, count, xyz, status, ustatus, conf, B, J, n_valid, dt, cfg, paras, flip, xyz_f, uvd_f, ahead, code):
    """cfg: a track.OneEuro.  conf (B, J) float32, read with weight "conf" alone, or NULL"""
    L.call("awr_joints_filter", state, count, xyz, status, ustatus, conf, int(B), int(J), int(n_valid), float(dt), float(cfg.min_cutoff), float(cfg.beta),
           float(cfg.d_cutoff), -1.0 if cfg.gate_mm is None else float(cfg.gate_mm), int(cfg.max_coast), WEIGHTS[cfg.weight], float(cfg.conf_floor),
           *_camera(paras, flip), xyz_f, uvd_f, ahead, code, L.stream())


def awr_confidence_fields(conf, stat, cube32, status, ustatus, n, J, n_valid, conf_out, peak, spread_mm):
    """the engine's conf and stat rows -> conf, peak, spread_mm (n, J) float32"""
    L.call("awr_confidence_fields", conf, stat, cube32, status, ustatus, int(n), int(J), int(n_valid), conf_out, peak, spread_mm, L.stream())
