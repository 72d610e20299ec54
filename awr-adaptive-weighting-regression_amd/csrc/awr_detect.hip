// Hand detection on the device: the crop centre of a raw depth frame by an iterated centre of mass, and from a centre the
// awr_nyu_sample block, crop matrix, camera-space centre and cube that awr_nyu_batch / awr_joints_unproject consume -- a restatement of
// awr_amd/detect.py (detect, sample_blocks), which itself calls nyu_data.center2bounds / crop_geometry / center2transmat.
//
// A pass over a frame is a streaming read (480 x 640 uint16 = 614 KB; 39 MB per pass at B = 64): HBM-bound, no matrix work.  What
// matters is (1) every sum is a 64-bit INTEGER (count, sum of columns, sum of rows, sum of raw uint16 depths): integer addition is
// associative, so any split of a frame over workgroups and any arrival order of the 64-bit integer atomics give the bits numpy gives
// summing in int64 -- there is no floating-point atomic in this file; (2) a frame is split over several workgroups by rows, rows are
// read with 16-byte loads wherever an aligned group of 8 pixels lies inside the window and pixel by pixel at the two ends;
// (3) per-workgroup partial sums meet in LDS and leave as ONE set of four atomics per workgroup; (4) each pass is its own launch and
// keeps its own accumulator slot in the caller's scratch, so the passes are ordered by the stream alone: nothing synchronises, and
// every workgroup of a pass derives the window from the previous pass's sums by the same three double divisions.
// The window arithmetic is awr_frame.h's bounds_window: nyu_data.center2bounds in IEEE double without contraction (this file is compiled
// with -ffp-contract=off).
// Two one-thread-per-frame passes close the loop from the network's output back to a crop centre: joints_center_kernel
// (predicted joints -> the gated next centre, detect.joints_center in IEEE double) and centers_select_kernel (a tracked centre where it is
// usable, the detector's otherwise).  Both are launch-bound; neither is clever.
// Three more of the same kind carry test-time views: view_centers_kernel expands each frame's centre into one centre, cube
// and frame index per view, view_rotate_kernel turns the crop block and crop matrix of a rotating view into the rotated ones, and
// views_fuse_kernel fuses the views' camera-space joints per frame and joint.  Their arithmetic is detect.view_centers / view_rotate /
// fuse_views in IEEE double, in that order of operations; the rotation matrices come ready-made from the host (detect.view_table): no
// kernel here evaluates a transcendental.
#include <limits.h>
#include <math.h>

#include "awr_frame.h"

namespace awr {

constexpr int DET_THREADS = 256;
constexpr int DET_SLOTS = AWR_DET_MAX_ITERS + 2;      // slot 0: smallest depth (NEAREST), slot 1: seed pass, slots 2...: refinement passes
constexpr int DET_MAX_PARTS = 1024;

enum { PASS_MIN = 0, PASS_SEED = 1, PASS_REFINE = 2 };

// centre of mass of an accumulator slot: three double divisions; n == 0 -> NaN
__device__ __forceinline__ void slot_centre(const u64* s, double* c) {
    if (s[0] == 0) { c[0] = c[1] = c[2] = __builtin_nan(""); return; }
    const double n = (double)s[0];
    c[0] = (double)s[1] / n; c[1] = (double)s[2] / n; c[2] = (double)s[3] / n;
}

__global__ __launch_bounds__(DET_THREADS) void detect_init_kernel(u64* __restrict__ slots, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * DET_THREADS + threadIdx.x;
    if (i < n) slots[i] = (i % (DET_SLOTS * 4) == 0) ? ~0ull : 0ull;        // slot 0 word 0 holds a minimum
}

// One pass: grid (parts, B).  kind PASS_MIN: smallest depth in [zmin, zmax] over the frame -> slot 0.  PASS_SEED: centre of mass over the
// frame of [zmin, zmax] (RANGE) or [dmin, min(dmin + slab, zmax)] (NEAREST) -> slot 1.  PASS_REFINE r: window of the centre left by
// pass r - 1 (r = 0: the seed) -> slot 2 + r.
__global__ __launch_bounds__(DET_THREADS) void detect_pass_kernel(const uint16_t* __restrict__ frames, int64_t n_frames, int fh, int fw,
                                                                  const int64_t* __restrict__ frame, int kind, int r, int seed_mode,
                                                                  const double* __restrict__ seed, double zmin, double zmax, double slab,
                                                                  const double* __restrict__ cube, int cube_stride, double fx, double fy,
                                                                  u64* __restrict__ slots) {
    __shared__ u64 red[4][DET_THREADS / 64];
    const int b = blockIdx.y, parts = gridDim.x, part = blockIdx.x, tid = threadIdx.x;
    const int64_t f = frame[b];
    if (f < 0 || f >= n_frames) return;                                     // AWR_DET_BAD_FRAME: nothing of it is read
    u64* S = slots + (int64_t)b * DET_SLOTS * 4;
    Window w{0, fw, 0, fh, 1, 0};
    if (kind == PASS_REFINE) {
        double c[3];
        if (r == 0 && seed_mode == AWR_DET_SEED_GIVEN) { c[0] = seed[3 * b]; c[1] = seed[3 * b + 1]; c[2] = seed[3 * b + 2]; }
        else slot_centre(S + 4 * (1 + r), c);
        w = bounds_window(c, cube + (int64_t)b * cube_stride, fx, fy, fh, fw);
    } else if (kind == PASS_SEED && seed_mode == AWR_DET_SEED_NEAREST) {
        const double dmin = (double)S[0];                                   // (no pixel in range: the sentinel 2^64 - 1 admits none)
        depth_bounds(dmin, fmin(dmin + slab, zmax), w.dlo, w.dhi);
    } else {
        depth_bounds(zmin, zmax, w.dlo, w.dhi);
    }
    if (w.u0 >= w.u1 || w.v0 >= w.v1 || w.dlo > w.dhi) return;
    const int rows = w.v1 - w.v0, per = (rows + parts - 1) / parts;
    const int va = w.v0 + part * per, vb = min(va + per, w.v1);
    if (part * per >= rows) return;                                         // more workgroups than rows
    const uint16_t* F = frames + f * (int64_t)fh * fw;
    const int mis = (int)(((uintptr_t)F >> 1) & 7);                         // pixels by which the frame's origin is past a 16-byte boundary
    const unsigned dlo = (unsigned)w.dlo, dhi = (unsigned)w.dhi;
    u64 n = 0, su = 0, sv = 0, sd = 0;
    unsigned dmin = 0xFFFFFFFFu;
    // (row, aligned group of 8 pixels) pairs of this workgroup's rows, flattened so that narrow windows still fill the lanes.  gpr bounds the
    // groups a row touches; pixel positions count from the 16-byte boundary before the frame's origin, where groups of 8 are aligned.
    const int gpr = ((w.u1 - w.u0) >> 3) + 2, total = (vb - va) * gpr;
    for (int idx = tid; idx < total; idx += DET_THREADS) {
        const int v = va + idx / gpr, gi = idx % gpr;
        const int colbase = mis + v * fw, gs = colbase + w.u0, ge = colbase + w.u1;
        const int g0 = ((gs >> 3) + gi) << 3;
        if (g0 >= ge) continue;
        unsigned rn = 0, ru = 0, rd = 0;
        if (g0 >= gs && g0 + 8 <= ge) {
            const uint4 q = *reinterpret_cast<const uint4*>(F + (g0 - mis));
            const unsigned word[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned d = (word[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu;
                const bool in = d >= dlo && d <= dhi;
                rn += in ? 1u : 0u;
                ru += in ? (unsigned)(g0 + k - colbase) : 0u;
                rd += in ? d : 0u;
                dmin = in ? min(dmin, d) : dmin;
            }
        } else {                                                            // the two ends of a row: pixel by pixel, never outside the window
            for (int g = max(g0, gs); g < min(g0 + 8, ge); ++g) {
                const unsigned d = F[g - mis];
                const bool in = d >= dlo && d <= dhi;
                rn += in ? 1u : 0u;
                ru += in ? (unsigned)(g - colbase) : 0u;
                rd += in ? d : 0u;
                dmin = in ? min(dmin, d) : dmin;
            }
        }
        n += rn; su += ru; sd += rd; sv += (u64)rn * (u64)v;
    }
    if (kind == PASS_MIN) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dmin = min(dmin, (unsigned)__shfl_xor((int)dmin, o, 64));
        if ((tid & 63) == 0) red[0][tid >> 6] = dmin;
        __syncthreads();
        if (tid == 0) {
            u64 m = red[0][0];
            for (int i = 1; i < DET_THREADS / 64; ++i) m = min(m, red[0][i]);
            if (m != 0xFFFFFFFFull) atomicMin(S, m);
        }
        return;
    }
    n = wave_sum(n); su = wave_sum(su); sv = wave_sum(sv); sd = wave_sum(sd);
    if ((tid & 63) == 0) { red[0][tid >> 6] = n; red[1][tid >> 6] = su; red[2][tid >> 6] = sv; red[3][tid >> 6] = sd; }
    __syncthreads();
    if (tid < 4) {
        u64 t = 0;
        for (int i = 0; i < DET_THREADS / 64; ++i) t += red[tid][i];
        u64* dst = S + 4 * (kind == PASS_SEED ? 1 : 2 + r) + tid;
        if (red[0][0] + red[0][1] + red[0][2] + red[0][3] != 0) atomicAdd(dst, t);
    }
}

// centre and status of every frame from its slots, in pass order
__global__ __launch_bounds__(DET_THREADS) void detect_finalize_kernel(int64_t n_frames, const int64_t* __restrict__ frame, int B, int seed_mode,
                                                                      const double* __restrict__ seed, int iters, const u64* __restrict__ slots,
                                                                      double* __restrict__ center, int* __restrict__ status) {
    const int b = blockIdx.x * DET_THREADS + threadIdx.x;
    if (b >= B) return;
    const u64* S = slots + (int64_t)b * DET_SLOTS * 4;
    double c[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
    int st = AWR_DET_OK;
    if (frame[b] < 0 || frame[b] >= n_frames) st = AWR_DET_BAD_FRAME;
    else {
        if (seed_mode == AWR_DET_SEED_GIVEN) { c[0] = seed[3 * b]; c[1] = seed[3 * b + 1]; c[2] = seed[3 * b + 2]; }
        else {
            slot_centre(S + 4, c);
            if (S[4] == 0) st = AWR_DET_EMPTY;
        }
        for (int r = 0; r < iters; ++r) {
            slot_centre(S + 4 * (2 + r), c);
            if (S[4 * (2 + r)] == 0) st = AWR_DET_EMPTY;
        }
    }
    center[3 * b] = c[0]; center[3 * b + 1] = c[1]; center[3 * b + 2] = c[2];
    status[b] = st;
}

// ---- centre -> awr_nyu_sample block, crop matrix, camera-space centre, cube (nyu_device.set_crop + set_normalize, center2transmat) ----
__global__ __launch_bounds__(DET_THREADS) void detect_samples_kernel(const double* __restrict__ center, const double* __restrict__ cube,
                                                                     int cube_stride, int64_t n_frames, const int64_t* __restrict__ frame,
                                                                     int B, int dsize, int fh, int fw, double fx, double fy, double u0, double v0, double flip,
                                                                     awr_nyu_sample* __restrict__ samples, float* __restrict__ M,
                                                                     float* __restrict__ center_xyz, float* __restrict__ cube_out,
                                                                     int* __restrict__ status) {
    const int b = blockIdx.x * DET_THREADS + threadIdx.x;
    if (b >= B) return;
    const double* c = center + 3 * b;
    const double* cb = cube + (int64_t)b * cube_stride;
    awr_nyu_sample s;
    const Bounds bd = center_bounds(c, cb, fx, fy);
    const double us = bd.us, ue = bd.ue, vs = bd.vs, ve = bd.ve;
    bool ok = isfinite(us) && isfinite(ue) && isfinite(vs) && isfinite(ve) && isfinite(c[2]) && isfinite(cb[2]);
    // (a bound outside int32 cannot pass set_crop's tests with a positive extent that resizes to something: refused here)
    ok = ok && fabs(us) < 1073741824.0 && fabs(ue) < 1073741824.0 && fabs(vs) < 1073741824.0 && fabs(ve) < 1073741824.0;
    int ustart = 0, uend = 0, vstart = 0, vend = 0, cw = 0, ch = 0, rw = 0, rh = 0;
    double scale = 0.0;
    if (ok) {
        ustart = (int)us; uend = (int)ue; vstart = (int)vs; vend = (int)ve;
        cw = uend - ustart; ch = vend - vstart;
        ok = cw > 0 && ch > 0 && uend > 0 && vend > 0 && ustart < fw && vstart < fh;
    }
    if (ok) {
        scale = fmin((double)dsize / (double)cw, (double)dsize / (double)ch);        // crop_geometry (loader.py:31-36)
        rw = (int)((double)cw * scale); rh = (int)((double)ch * scale);
        ok = rw > 0 && rh > 0;
    }
    const int64_t f = frame[b];
    if (f < 0 || f >= n_frames) {                                                             // never a block that names a frame outside the store
        ok = false;
        status[b] = AWR_DET_BAD_FRAME;
    }
    for (int i = 0; i < 9; ++i) s.m[i] = 0.0;
    s.op = AWR_NYU_NONE; s.norm32 = 0; s.zstart2 = 0.0; s.zend2 = 0.0;
    if (ok) {
        s.frame = f;
        s.ustart = ustart; s.vstart = vstart; s.cw = cw; s.ch = ch; s.rw = rw; s.rh = rh;
        s.ox = (int)((double)(dsize - rw) / 2.0); s.oy = (int)((double)(dsize - rh) / 2.0);
        s.ifx = 1.0 / ((double)rw / (double)cw); s.ify = 1.0 / ((double)rh / (double)ch);      // nyu_data.resize_nearest: two divisions
        s.zstart = c[2] - cb[2] / 2.0; s.zend = c[2] + cb[2] / 2.0;
        const double half = cb[2] / 2.0;                                                      // set_normalize, float64
        s.half = half; s.far = c[2] + half; s.lo = c[2] - half; s.center_z = c[2];
        // center2transmat (loader.py:211-240): t2 . (sc . t1) in double, stored as float32
        const double tx = floor((double)dsize / 2.0 - (double)rw / 2.0), ty = floor((double)dsize / 2.0 - (double)rh / 2.0);
        float* m = M + 9 * b;
        m[0] = (float)scale; m[1] = 0.f; m[2] = (float)(scale * (double)(-ustart) + tx);
        m[3] = 0.f; m[4] = (float)scale; m[5] = (float)(scale * (double)(-vstart) + ty);
        m[6] = 0.f; m[7] = 0.f; m[8] = 1.f;
    } else {
        // a window set_crop refuses (or a NaN centre): a block that reads no pixel and renders a finite all-background image (rw = rh = 0:
        // nyu_batch_kernel's crop_pixel returns 0 before it touches cw, ch or the frame), a NaN matrix that un-projects to NaN rows
        s.frame = 0;
        s.ustart = s.vstart = s.cw = s.ch = s.rw = s.rh = s.ox = s.oy = 0;
        s.ifx = s.ify = 1.0; s.zstart = 0.0; s.zend = 0.0;
        s.lo = 0.0; s.far = 1.0; s.center_z = 0.0; s.half = 1.0;
        for (int i = 0; i < 9; ++i) M[9 * b + i] = __builtin_nanf("");
        if (status[b] == AWR_DET_OK) status[b] = AWR_DET_BAD_WINDOW;
    }
    samples[b] = s;
    // uvd2xyz of the float64 centre, stored as float32
    center_xyz[3 * b] = (float)uvd2x(c[0], u0, c[2], fx);
    center_xyz[3 * b + 1] = (float)uvd2y(c[1], v0, c[2], fy, flip);
    center_xyz[3 * b + 2] = (float)c[2];
    cube_out[3 * b] = (float)cb[0]; cube_out[3 * b + 1] = (float)cb[1]; cube_out[3 * b + 2] = (float)cb[2];
}

// ---- joints -> the next crop centre (detect.joints_center): one thread per frame, the header's definition line by line ----
__global__ __launch_bounds__(DET_THREADS) void joints_center_kernel(const float* __restrict__ xyz, const double* center_uvd,
                                                                    const float* __restrict__ center_xyz, const float* __restrict__ cube,
                                                                    const int* __restrict__ status, const int* __restrict__ ustatus, int J,
                                                                    int n_valid, const int* __restrict__ joints, int n_sel, double fx, double fy,
                                                                    double u0, double v0, double flip, double zmin, double zmax, double max_shift,
                                                                    double* center_out, double* __restrict__ next_out, int* __restrict__ code) {
    const int b = blockIdx.x * DET_THREADS + threadIdx.x;
    if (b >= n_valid) return;
    const double nan = __builtin_nan("");
    const double c[3] = {center_uvd[3 * b], center_uvd[3 * b + 1], center_uvd[3 * b + 2]};      // read before center_out, which may be it
    double nc[3] = {nan, nan, nan};
    int cd = AWR_RECENTER_KEPT_FRAME;
    if (status[b] == 0 && ustatus[b] == 0) {
        const float* X = xyz + (int64_t)b * J * 3;
        double m[3] = {0.0, 0.0, 0.0};
        bool in_range = true;
        for (int k = 0; k < n_sel; ++k) {                                   // sequential, in index order
            const int j = joints ? joints[k] : k;
            if (j < 0 || j >= J) { in_range = false; break; }               // never a read outside the frame's joints
            m[0] += (double)X[3 * j]; m[1] += (double)X[3 * j + 1]; m[2] += (double)X[3 * j + 2];
        }
        const double n = (double)n_sel;
        m[0] = m[0] / n; m[1] = m[1] / n; m[2] = m[2] / n;
        bool near = true;
        for (int a = 0; a < 3; ++a)
            near = near && fabs(m[a] - (double)center_xyz[3 * b + a]) <= max_shift * ((double)cube[3 * b + a] / 2.0);
        if (!in_range || !(isfinite(m[0]) && isfinite(m[1]) && isfinite(m[2]))) cd = AWR_RECENTER_KEPT_NONFINITE;
        else if (!(zmin <= m[2] && m[2] <= zmax)) cd = AWR_RECENTER_KEPT_DEPTH;
        else if (!near) cd = AWR_RECENTER_KEPT_SHIFT;
        else {
            cd = AWR_RECENTER_MOVED;
            const double yf = m[1] * flip;
            nc[0] = xyz2u(m[0], fx, m[2], u0); nc[1] = xyz2v(yf, fy, m[2], v0); nc[2] = m[2];
        }
    }
    const bool moved = cd == AWR_RECENTER_MOVED;
    for (int a = 0; a < 3; ++a) {
        center_out[3 * b + a] = moved ? nc[a] : c[a];
        if (next_out) next_out[3 * b + a] = nc[a];
    }
    code[b] = cd;
}

// ---- per frame: a where it is a usable centre, b otherwise (detect.select) ----
__global__ __launch_bounds__(DET_THREADS) void centers_select_kernel(const double* __restrict__ a_center, const int* __restrict__ a_status,
                                                                     const double* __restrict__ b_center, const int* __restrict__ b_status, int B,
                                                                     double* __restrict__ out_center, int* __restrict__ out_status,
                                                                     int* __restrict__ which) {
    const int i = blockIdx.x * DET_THREADS + threadIdx.x;
    if (i >= B) return;
    const double a[3] = {a_center[3 * i], a_center[3 * i + 1], a_center[3 * i + 2]};
    const bool take_a = a_status[i] == AWR_DET_OK && isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]);
    for (int k = 0; k < 3; ++k) out_center[3 * i + k] = take_a ? a[k] : b_center[3 * i + k];
    out_status[i] = take_a ? a_status[i] : b_status[i];
    if (which) which[i] = take_a ? 0 : 1;
}

// ---- test-time views (detect.view_centers, view_rotate, fuse_views) ----
// One table row per view, AWR_VIEW_TABLE_DOUBLES doubles (160 bytes: rows stay 16-byte aligned)
enum { VT_R = 0, VT_IR = 9, VT_SCALE = 15, VT_SHIFT = 16, VT_ROTATES = 19 };

// one thread per (view, frame): row v * B + b of the outputs
__global__ __launch_bounds__(DET_THREADS) void view_centers_kernel(const double* __restrict__ center, const int* __restrict__ status,
                                                                   const double* __restrict__ cube, int cube_stride,
                                                                   const double* __restrict__ table, int V, int B, int n_valid, double fx,
                                                                   double fy, double u0, double v0, double flip,
                                                                   double* __restrict__ centers_out, double* __restrict__ cubes_out,
                                                                   int64_t* __restrict__ frame_out, int* __restrict__ status_out) {
    const int i = blockIdx.x * DET_THREADS + threadIdx.x;
    if (i >= V * n_valid) return;
    const int v = i / n_valid, b = i % n_valid;
    const int64_t r = (int64_t)v * B + b;
    const double* T = table + (int64_t)v * AWR_VIEW_TABLE_DOUBLES;
    const double* cb = cube + (int64_t)b * cube_stride;
    const double sx = T[VT_SHIFT], sy = T[VT_SHIFT + 1], sz = T[VT_SHIFT + 2], sc = T[VT_SCALE];
    double c[3] = {center[3 * b], center[3 * b + 1], center[3 * b + 2]};
    if (!(sx == 0.0 && sy == 0.0 && sz == 0.0)) {
        // uvd2xyz, the shift, xyz2uvd: loader.py:112 in double
        const double x = uvd2x(c[0], u0, c[2], fx) + sx;
        const double y = uvd2y(c[1], v0, c[2], fy, flip) + sy;
        const double z = c[2] + sz;
        const double yf = y * flip;
        c[0] = xyz2u(x, fx, z, u0); c[1] = xyz2v(yf, fy, z, v0); c[2] = z;
    }
    centers_out[3 * r] = c[0]; centers_out[3 * r + 1] = c[1]; centers_out[3 * r + 2] = c[2];
    cubes_out[3 * r] = cb[0] * sc; cubes_out[3 * r + 1] = cb[1] * sc; cubes_out[3 * r + 2] = cb[2] * sc;
    frame_out[r] = b;
    status_out[r] = status[b];
}

// one thread per (view, frame): the block and the matrix of a rotating view's AWR_DET_OK row, in place
__global__ __launch_bounds__(DET_THREADS) void view_rotate_kernel(awr_nyu_sample* __restrict__ samples, float* __restrict__ M,
                                                                  const int* __restrict__ status, const double* __restrict__ table, int V,
                                                                  int B, int n_valid) {
    const int i = blockIdx.x * DET_THREADS + threadIdx.x;
    if (i >= V * n_valid) return;
    const int v = i / n_valid, b = i % n_valid;
    const int64_t r = (int64_t)v * B + b;
    const double* T = table + (int64_t)v * AWR_VIEW_TABLE_DOUBLES;
    if (T[VT_ROTATES] == 0.0 || status[r] != AWR_DET_OK) return;
    awr_nyu_sample* s = samples + r;
    s->op = AWR_NYU_AFFINE;
    for (int k = 0; k < 6; ++k) s->m[k] = T[VT_IR + k];
    s->m[6] = 0.0; s->m[7] = 0.0; s->m[8] = 1.0;
    float* m = M + 9 * r;
    double a[9];
    for (int k = 0; k < 9; ++k) a[k] = (double)m[k];
    for (int row = 0; row < 3; ++row)
        for (int col = 0; col < 3; ++col)
            m[3 * row + col] = (float)(((T[VT_R + 3 * row] * a[col]) + (T[VT_R + 3 * row + 1] * a[3 + col])) + (T[VT_R + 3 * row + 2] * a[6 + col]));
}

// the middle of the n smallest of eight values (the unused ones are +infinity): a stable bubble network over registers
__device__ __forceinline__ double median8(double (&a)[AWR_VIEWS_MAX], int n) {
#pragma unroll
    for (int pass = 0; pass < AWR_VIEWS_MAX - 1; ++pass)
#pragma unroll
        for (int k = 0; k < AWR_VIEWS_MAX - 1 - pass; ++k) {
            const double lo = a[k], hi = a[k + 1];
            const bool swap = lo > hi;
            a[k] = swap ? hi : lo; a[k + 1] = swap ? lo : hi;
        }
    double mid = 0.0, below = 0.0;
#pragma unroll
    for (int k = 0; k < AWR_VIEWS_MAX; ++k) {
        mid = (k == n / 2) ? a[k] : mid;
        below = (k + 1 == n / 2) ? a[k] : below;
    }
    return (n & 1) ? mid : (below + mid) / 2.0;
}

// one thread per (frame, joint)
__global__ __launch_bounds__(DET_THREADS) void views_fuse_kernel(const float* __restrict__ xyz, const int* __restrict__ status,
                                                                 const int* __restrict__ ustatus, const float* __restrict__ weights, int mode,
                                                                 int V, int B, int J, int n_valid, double fx, double fy, double u0, double v0,
                                                                 double flip, float* __restrict__ xyz_out, float* __restrict__ uvd_out,
                                                                 float* __restrict__ spread_out, int* __restrict__ used_out) {
    const int64_t i = (int64_t)blockIdx.x * DET_THREADS + threadIdx.x;
    if (i >= (int64_t)n_valid * J) return;
    const int b = (int)(i / J), j = (int)(i % J);
    const double nan = __builtin_nan("");
    double X[3][AWR_VIEWS_MAX], W[AWR_VIEWS_MAX];
    int used = 0;
    const bool frame_ok = status[b] == 0 && ustatus[b] == 0;                // view 0's codes
#pragma unroll
    for (int v = 0; v < AWR_VIEWS_MAX; ++v) {
        X[0][v] = X[1][v] = X[2][v] = INFINITY; W[v] = 0.0;
        if (v < V && frame_ok) {
            const int64_t r = (int64_t)v * B + b;
            const float* p = xyz + (r * J + j) * 3;
            const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
            double w = 1.0;
            bool ok = status[r] == 0 && ustatus[r] == 0 && isfinite(x) && isfinite(y) && isfinite(z);
            if (mode == AWR_FUSE_CONF) {
                w = (double)weights[r * J + j];
                ok = ok && isfinite(w) && w > 0.0;
            }
            if (ok) { X[0][v] = x; X[1][v] = y; X[2][v] = z; W[v] = w; ++used; }
        }
    }
    double m[3] = {nan, nan, nan}, spread = nan;
    if (used > 0) {
        double sw = 0.0, s[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int v = 0; v < AWR_VIEWS_MAX; ++v)
            if (W[v] > 0.0) {                                               // sequentially in view order
                s[0] = s[0] + W[v] * X[0][v]; s[1] = s[1] + W[v] * X[1][v]; s[2] = s[2] + W[v] * X[2][v];
                sw = sw + W[v];
            }
        if (mode == AWR_FUSE_MEDIAN) {
            for (int a = 0; a < 3; ++a) {
                double t[AWR_VIEWS_MAX];
#pragma unroll
                for (int v = 0; v < AWR_VIEWS_MAX; ++v) t[v] = X[a][v];
                m[a] = median8(t, used);
            }
        } else {
            m[0] = s[0] / sw; m[1] = s[1] / sw; m[2] = s[2] / sw;
        }
        double q = 0.0;
#pragma unroll
        for (int v = 0; v < AWR_VIEWS_MAX; ++v)
            if (W[v] > 0.0) {
                const double dx = X[0][v] - m[0], dy = X[1][v] - m[1], dz = X[2][v] - m[2];
                q = q + W[v] * ((dx * dx + dy * dy) + dz * dz);
            }
        spread = sqrt(q / sw);
    }
    const double yf = m[1] * flip;
    float* xo = xyz_out + i * 3;
    float* uo = uvd_out + i * 3;
    xo[0] = (float)m[0]; xo[1] = (float)m[1]; xo[2] = (float)m[2];
    uo[0] = (float)(used ? xyz2u(m[0], fx, m[2], u0) : nan); uo[1] = (float)(used ? xyz2v(yf, fy, m[2], v0) : nan); uo[2] = (float)m[2];
    spread_out[i] = (float)spread;
    used_out[i] = used;
}

}  // namespace awr

using namespace awr;

extern "C" {

int64_t awr_detect_scratch(int B) {
    if (B <= 0 || B > AWR_DET_MAX_BATCH) {
        set_error("awr_detect_scratch: B = %d is outside [1, %d]", B, AWR_DET_MAX_BATCH);
        return -1;
    }
    return (int64_t)B * DET_SLOTS * 4 * (int64_t)sizeof(u64);
}

int awr_detect(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B, int seed_mode,
               const double* seed_uvd, double zmin, double zmax, double slab, const double* cube, int cube_stride, double fx, double fy,
               int iters, int parts, void* scratch, double* center_uvd, int* status, void* stream) {
    AWR_REQUIRE(frames && frame && cube && scratch && center_uvd && status, "awr_detect: NULL pointer");
    if (check_frame_store("awr_detect", frame_type, B, n_frames, fh, fw) != AWR_OK) return AWR_ERR_ARG;
    AWR_REQUIRE(iters >= 0 && iters <= AWR_DET_MAX_ITERS, "awr_detect: iters = %d is outside [0, %d]", iters, AWR_DET_MAX_ITERS);
    AWR_REQUIRE(seed_mode == AWR_DET_SEED_GIVEN || seed_mode == AWR_DET_SEED_RANGE || seed_mode == AWR_DET_SEED_NEAREST,
                "awr_detect: seed_mode %d is none of AWR_DET_SEED_GIVEN / _RANGE / _NEAREST", seed_mode);
    AWR_REQUIRE(seed_mode != AWR_DET_SEED_GIVEN || seed_uvd, "awr_detect: AWR_DET_SEED_GIVEN needs seed_uvd (NULL pointer)");
    AWR_REQUIRE(zmin <= zmax, "awr_detect: depth range needs zmin <= zmax (got %g, %g)", zmin, zmax);
    AWR_REQUIRE(slab >= 0.0, "awr_detect: slab = %g must be >= 0", slab);
    AWR_REQUIRE(cube_stride == 0 || cube_stride == 3, "awr_detect: cube_stride is 0 (one cube) or 3 (one per frame), not %d", cube_stride);
    AWR_REQUIRE(fx != 0.0 && fy != 0.0 && isfinite(fx) && isfinite(fy), "awr_detect: bad intrinsics");
    AWR_REQUIRE(parts >= 0 && parts <= DET_MAX_PARTS, "awr_detect: parts = %d is outside [0, %d] (0: chosen from B and the frame)", parts, DET_MAX_PARTS);
    AWR_REQUIRE(((uintptr_t)frames & 1) == 0 && ((uintptr_t)scratch & 7) == 0, "awr_detect: misaligned frame store / scratch");
    hipStream_t s = as_stream(stream);
    u64* slots = (u64*)scratch;
    const int64_t nw = (int64_t)B * DET_SLOTS * 4;
    const int P = parts ? parts : frame_parts(B, fh, DET_MAX_PARTS);
    const uint16_t* F = (const uint16_t*)frames;
    detect_init_kernel<<<(unsigned)((nw + DET_THREADS - 1) / DET_THREADS), DET_THREADS, 0, s>>>(slots, nw);
    const dim3 grid(P, B);
    if (seed_mode == AWR_DET_SEED_NEAREST)
        detect_pass_kernel<<<grid, DET_THREADS, 0, s>>>(F, n_frames, fh, fw, frame, PASS_MIN, 0, seed_mode, seed_uvd, zmin, zmax, slab, cube,
                                                        cube_stride, fx, fy, slots);
    if (seed_mode != AWR_DET_SEED_GIVEN)
        detect_pass_kernel<<<grid, DET_THREADS, 0, s>>>(F, n_frames, fh, fw, frame, PASS_SEED, 0, seed_mode, seed_uvd, zmin, zmax, slab, cube,
                                                        cube_stride, fx, fy, slots);
    for (int r = 0; r < iters; ++r)
        detect_pass_kernel<<<grid, DET_THREADS, 0, s>>>(F, n_frames, fh, fw, frame, PASS_REFINE, r, seed_mode, seed_uvd, zmin, zmax, slab, cube,
                                                        cube_stride, fx, fy, slots);
    detect_finalize_kernel<<<(B + DET_THREADS - 1) / DET_THREADS, DET_THREADS, 0, s>>>(n_frames, frame, B, seed_mode, seed_uvd, iters, slots,
                                                                                      center_uvd, status);
    return check_launch("awr_detect");
}

int awr_detect_samples(const double* center_uvd, const double* cube, int cube_stride, int64_t n_frames, const int64_t* frame, int B, int dsize,
                       int fh, int fw, double fx, double fy, double u0, double v0, int flip, awr_nyu_sample* samples, float* M, float* center_xyz,
                       float* cube_out, int* status, void* stream) {
    AWR_REQUIRE(center_uvd && cube && frame && samples && M && center_xyz && cube_out && status, "awr_detect_samples: NULL pointer");
    AWR_REQUIRE(B > 0 && B <= AWR_DET_MAX_BATCH, "awr_detect_samples: B = %d is outside [1, %d]", B, AWR_DET_MAX_BATCH);
    AWR_REQUIRE(n_frames > 0, "awr_detect_samples: n_frames = %lld must be positive", (long long)n_frames);
    AWR_REQUIRE(dsize > 0 && dsize <= 4096, "awr_detect_samples: dsize = %d is outside [1, 4096]", dsize);
    AWR_REQUIRE(frame_sides_ok(fh, fw), "awr_detect_samples: frame of %d x %d is outside [1, %d]^2", fh, fw, FRAME_MAX_SIDE);
    AWR_REQUIRE(cube_stride == 0 || cube_stride == 3, "awr_detect_samples: cube_stride is 0 (one cube) or 3 (one per frame), not %d", cube_stride);
    AWR_REQUIRE(fx != 0.0 && fy != 0.0 && isfinite(fx) && isfinite(fy) && (flip == 1 || flip == -1), "awr_detect_samples: bad intrinsics / flip");
    detect_samples_kernel<<<(B + DET_THREADS - 1) / DET_THREADS, DET_THREADS, 0, as_stream(stream)>>>(
        center_uvd, cube, cube_stride, n_frames, frame, B, dsize, fh, fw, fx, fy, u0, v0, (double)flip, samples, M, center_xyz, cube_out, status);
    return check_launch("awr_detect_samples");
}

int awr_joints_center(const float* xyz, const double* center_uvd, const float* center_xyz, const float* cube, const int* status,
                      const int* ustatus, int B, int J, int n_valid, const int* joints, int n_joints, double fx, double fy, double u0, double v0,
                      int flip, double zmin, double zmax, double max_shift, double* center_out, double* next_out, int* code, void* stream) {
    AWR_REQUIRE(xyz && center_uvd && center_xyz && cube && status && ustatus && center_out && code, "awr_joints_center: NULL pointer");
    AWR_REQUIRE(B > 0 && B <= AWR_DET_MAX_BATCH, "awr_joints_center: B = %d is outside [1, %d]", B, AWR_DET_MAX_BATCH);
    AWR_REQUIRE(J > 0 && J <= AWR_RECENTER_MAX_JOINTS, "awr_joints_center: J = %d is outside [1, %d]", J, AWR_RECENTER_MAX_JOINTS);
    AWR_REQUIRE(n_valid >= 0 && n_valid <= B, "awr_joints_center: n_valid = %d is outside [0, B = %d]", n_valid, B);
    AWR_REQUIRE(n_joints >= 0 && n_joints <= J, "awr_joints_center: n_joints = %d is outside [0, J = %d]", n_joints, J);
    AWR_REQUIRE(n_joints == 0 || joints, "awr_joints_center: n_joints = %d needs the index list (NULL pointer)", n_joints);
    AWR_REQUIRE(fx != 0.0 && fy != 0.0 && isfinite(fx) && isfinite(fy) && isfinite(u0) && isfinite(v0) && (flip == 1 || flip == -1),
                "awr_joints_center: bad intrinsics / flip");
    AWR_REQUIRE(zmin <= zmax, "awr_joints_center: depth range needs zmin <= zmax (got %g, %g)", zmin, zmax);
    AWR_REQUIRE(max_shift >= 0.0, "awr_joints_center: max_shift = %g must be >= 0 (infinity: no gate)", max_shift);
    if (n_valid == 0) return AWR_OK;
    const bool all = n_joints == 0;
    joints_center_kernel<<<(n_valid + DET_THREADS - 1) / DET_THREADS, DET_THREADS, 0, as_stream(stream)>>>(
        xyz, center_uvd, center_xyz, cube, status, ustatus, J, n_valid, all ? nullptr : joints, all ? J : n_joints, fx, fy, u0, v0, (double)flip,
        zmin, zmax, max_shift, center_out, next_out, code);
    return check_launch("awr_joints_center");
}

int awr_centers_select(const double* a_center, const int* a_status, const double* b_center, const int* b_status, int B, double* out_center,
                       int* out_status, int* which, void* stream) {
    AWR_REQUIRE(a_center && a_status && b_center && b_status && out_center && out_status, "awr_centers_select: NULL pointer");
    AWR_REQUIRE(B > 0 && B <= AWR_DET_MAX_BATCH, "awr_centers_select: B = %d is outside [1, %d]", B, AWR_DET_MAX_BATCH);
    centers_select_kernel<<<(B + DET_THREADS - 1) / DET_THREADS, DET_THREADS, 0, as_stream(stream)>>>(a_center, a_status, b_center, b_status, B,
                                                                                                   out_center, out_status, which);
    return check_launch("awr_centers_select");
}

static int check_views(const char* who, int V, int B, int n_valid) {
    AWR_REQUIRE(V > 0 && V <= AWR_VIEWS_MAX, "%s: V = %d is outside [1, %d]", who, V, AWR_VIEWS_MAX);
    AWR_REQUIRE(B > 0 && (int64_t)V * B <= AWR_DET_MAX_BATCH, "%s: V * B = %d * %d is outside [1, %d]", who, V, B, AWR_DET_MAX_BATCH);
    AWR_REQUIRE(n_valid >= 0 && n_valid <= B, "%s: n_valid = %d is outside [0, B = %d]", who, n_valid, B);
    return AWR_OK;
}

int awr_view_centers(const double* center_uvd, const int* status, const double* cube, int cube_stride, const double* table, int V, int B,
                     int n_valid, double fx, double fy, double u0, double v0, int flip, double* centers_out, double* cubes_out,
                     int64_t* frame_out, int* status_out, void* stream) {
    AWR_REQUIRE(center_uvd && status && cube && table && centers_out && cubes_out && frame_out && status_out, "awr_view_centers: NULL pointer");
    if (check_views("awr_view_centers", V, B, n_valid) != AWR_OK) return AWR_ERR_ARG;
    AWR_REQUIRE(cube_stride == 0 || cube_stride == 3, "awr_view_centers: cube_stride is 0 (one cube) or 3 (one per frame), not %d", cube_stride);
    AWR_REQUIRE(fx != 0.0 && fy != 0.0 && isfinite(fx) && isfinite(fy) && isfinite(u0) && isfinite(v0) && (flip == 1 || flip == -1),
                "awr_view_centers: bad intrinsics / flip");
    if (n_valid == 0) return AWR_OK;
    view_centers_kernel<<<(V * n_valid + DET_THREADS - 1) / DET_THREADS, DET_THREADS, 0, as_stream(stream)>>>(
        center_uvd, status, cube, cube_stride, table, V, B, n_valid, fx, fy, u0, v0, (double)flip, centers_out, cubes_out, frame_out, status_out);
    return check_launch("awr_view_centers");
}

int awr_view_rotate(awr_nyu_sample* samples, float* M, const int* status, const double* table, int V, int B, int n_valid, void* stream) {
    AWR_REQUIRE(samples && M && status && table, "awr_view_rotate: NULL pointer");
    if (check_views("awr_view_rotate", V, B, n_valid) != AWR_OK) return AWR_ERR_ARG;
    if (n_valid == 0) return AWR_OK;
    view_rotate_kernel<<<(V * n_valid + DET_THREADS - 1) / DET_THREADS, DET_THREADS, 0, as_stream(stream)>>>(samples, M, status, table, V, B,
                                                                                                           n_valid);
    return check_launch("awr_view_rotate");
}

int awr_views_fuse(const float* xyz, const int* status, const int* ustatus, const float* weights, int mode, int V, int B, int J, int n_valid,
                   double fx, double fy, double u0, double v0, int flip, float* xyz_out, float* uvd_out, float* spread_out, int* used_out,
                   void* stream) {
    AWR_REQUIRE(xyz && status && ustatus && xyz_out && uvd_out && spread_out && used_out, "awr_views_fuse: NULL pointer");
    if (check_views("awr_views_fuse", V, B, n_valid) != AWR_OK) return AWR_ERR_ARG;
    AWR_REQUIRE(J > 0 && J <= AWR_RECENTER_MAX_JOINTS, "awr_views_fuse: J = %d is outside [1, %d]", J, AWR_RECENTER_MAX_JOINTS);
    AWR_REQUIRE(mode == AWR_FUSE_MEAN || mode == AWR_FUSE_CONF || mode == AWR_FUSE_MEDIAN,
                "awr_views_fuse: mode %d is none of AWR_FUSE_MEAN / _CONF / _MEDIAN", mode);
    AWR_REQUIRE(mode != AWR_FUSE_CONF || weights, "awr_views_fuse: AWR_FUSE_CONF needs the weights (NULL pointer)");
    AWR_REQUIRE(fx != 0.0 && fy != 0.0 && isfinite(fx) && isfinite(fy) && isfinite(u0) && isfinite(v0) && (flip == 1 || flip == -1),
                "awr_views_fuse: bad intrinsics / flip");
    if (n_valid == 0) return AWR_OK;
    const int64_t n = (int64_t)n_valid * J;
    views_fuse_kernel<<<(unsigned)((n + DET_THREADS - 1) / DET_THREADS), DET_THREADS, 0, as_stream(stream)>>>(
        xyz, status, ustatus, weights, mode, V, B, J, n_valid, fx, fy, u0, v0, (double)flip, xyz_out, uvd_out, spread_out, used_out);
    return check_launch("awr_views_fuse");
}

}  // extern "C"
