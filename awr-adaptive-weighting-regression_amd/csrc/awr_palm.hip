// Forearm-robust palm centre: a detector centre -> the centre of the palm disc, found on the exact squared Euclidean
// distance transform of the hand-plus-arm silhouette -- a restatement of awr_amd/detect.py palm_center, bit for bit.
//
// Everything between the window and the last three divisions is INTEGER arithmetic: the distance transform (squares of pixel
// distances), the medial set (tau[1] * D2 >= tau[0] * m), the three arg-max sweeps, the two counts and the disc sums.  Frame sides are
// at most 16384, so D2 <= 2^28, L = |e2 - e1|^2 <= 2^29, |t| and |s| <= 2^30, s * s <= 2^60, m * L <= 2^57 and tau * D2,
// rho2 * |p - p*|^2 (both factors below 2^31 and 2^29) <= 2^60: every product stays below 2^62 in int64.  An integer max or sum does not
// depend on the order of its operands; every arg-max is a max of (value << 32 | ~raster index), which is the first maximum in raster
// order however the pixels are dealt to lanes and workgroups and in whatever order their 64-bit INTEGER atomics arrive.  There is no
// floating-point atomic and no floating-point reduction in this file.
//
// Shape: a frame's window is split by rows over several workgroups (about four per CU over the batch, at most 64 per frame), each
// stage is its own launch, and the stages meet in sixteen 64-bit words per frame at the head of the caller's scratch (zeroed by the
// first launch): packed maxima by atomicMax, counts and sums by atomicAdd, one set per workgroup after a reduction through LDS.  The
// stream orders the stages; nothing synchronises.  D2 (int32, one word per window pixel) follows the slots in the scratch, fh * fw
// words per frame, and stays L2-resident (a 350 x 350 window is 490 KB).
//   1. palm_scan_kernel: g = distance along the column to the nearest background row.  A thread per column and direction; the scan
//      down writes the low 16 bits of a pixel's word, the scan up the high 16 bits, both from the frame alone.  A workgroup owns a band
//      of rows: a thread first counts the foreground run that reaches its band from outside, sixteen rows loaded per step;
//   2. palm_rows_kernel: over tiles of whole rows of the band, g = the smaller half goes to LDS as uint16 (g <= 16384), every pixel
//      takes min over k of k^2 + g(u +- k)^2 from LDS, four distances per step until k^2 reaches the best so far, and overwrites its
//      word with D2; the arg-max of D2 rides along;
//   3. palm_far_kernel twice (e1, e2), palm_end_kernel twice (the two counts, then p*), palm_disc_kernel (the disc sums): a row per
//      wave, a column per lane, eight loads in flight per lane, no division to recover the row;
//   4. palm_finalize_kernel: one thread per frame writes centre, status and info -- the only stage that writes an output, so the
//      outputs may be the inputs.
// Every stage derives the frame's window from the inputs by the same arithmetic (palm_frame).
// Why several workgroups: the first form was ONE 1024-thread workgroup per frame with the stages between __syncthreads().  Measured
// with device-clock stamps on one MI355X (a 348 x 364 window, B = 1): 0.43 ms -- scans 93 us, row pass 102 us, max + e1 + e2 95 us,
// counts + p* 78 us, disc 46 us, about 45 us per pass over 0.5 MB -- and unmoved by 1, 8 or 32 loads in flight per lane, by dropping the
// divisions, by running the two scans side by side: one CU moved some 12 GB/s whatever it was asked.  This form: 0.10 ms at B = 1.
// The window arithmetic is awr_frame.h's bounds_window with the cube scaled by `search` (compiled with -ffp-contract=off).
#include <limits.h>
#include <math.h>

#include "awr_frame.h"

namespace awr {
namespace {

constexpr int PALM_THREADS = 256;
constexpr int PALM_WAVES = PALM_THREADS / 64;
constexpr int PALM_TILE = FRAME_MAX_SIDE;             // LDS entries of a row tile: at least one row of the widest frame
constexpr int PALM_BATCH = 8;                         // independent loads a lane issues before it uses the first
constexpr int PALM_SCAN = 16;                         // ... and rows a column scan loads ahead of its dependent chain
constexpr int PALM_SLOTS = 16;                        // 64-bit words of a frame's slots
constexpr int PALM_MAX_PARTS = 64;                    // workgroups per frame

// a value and a raster index as one word whose maximum is the first maximum in raster order
__device__ __forceinline__ u64 pack_key(i64 value, int index) { return ((u64)value << 32) | (u64)(0xFFFFFFFFu - (unsigned)index); }
__device__ __forceinline__ int key_index(u64 key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }

// what every stage is handed; a stage recomputes its frame's window from the inputs (the outputs are written by the last stage alone)
struct PalmArgs {
    const uint16_t* frames; int64_t n_frames; int fh, fw;
    const int64_t* frame; const double* center_in; const int* status_in;
    double zmin, zmax; const double* cube; int cube_stride; double fx, fy, search;
    i64 tau0, tau1, rho0, rho1;
    u64* slots; int* D;
};

// per frame PALM_SLOTS 64-bit words: packed maxima (value << 32 | ~raster index) and integer sums, zeroed by the first launch
enum { SL_MAX = 0, SL_E1, SL_E2, SL_B1, SL_B2, SL_PS, SL_N, SL_SU, SL_SV, SL_SD };

struct PalmFrame {
    Window w;
    const uint16_t* F;      // the frame
    int* D;                 // its fh * fw words of the scratch
    u64* S;                 // its slots
    int ww, wh, r0, r1;     // the window's size and this workgroup's rows [r0, r1) of it
    int code;               // AWR_DET_OK: the window holds something to look at | the status the frame ends with
};

// frame blockIdx.y of the batch and the rows of workgroup blockIdx.x of gridDim.x; uniform over the workgroup
__device__ __forceinline__ PalmFrame palm_frame(const PalmArgs& a) {
    PalmFrame pf;
    const int b = blockIdx.y;
    const int64_t f = a.frame[b];
    pf.w = Window{0, 0, 0, 0, 1, 0};
    pf.F = a.frames; pf.D = a.D + (int64_t)b * a.fh * a.fw; pf.S = a.slots + (int64_t)b * PALM_SLOTS;
    pf.ww = pf.wh = pf.r0 = pf.r1 = 0;
    if (f < 0 || f >= a.n_frames) { pf.code = AWR_DET_BAD_FRAME; return pf; }          // nothing of it is read
    pf.code = a.status_in[b];
    if (pf.code != AWR_DET_OK) return pf;                                               // centre and status pass through
    const double c[3] = {a.center_in[3 * b], a.center_in[3 * b + 1], a.center_in[3 * b + 2]};
    pf.w = palm_window(c, a.cube + (int64_t)b * a.cube_stride, a.search, a.fx, a.fy, a.zmin, a.zmax, a.fh, a.fw);
    if (pf.w.u0 >= pf.w.u1 || pf.w.v0 >= pf.w.v1 || pf.w.dlo > pf.w.dhi) { pf.code = AWR_DET_EMPTY; return pf; }
    pf.F = a.frames + f * (int64_t)a.fh * a.fw;
    pf.ww = pf.w.u1 - pf.w.u0; pf.wh = pf.w.v1 - pf.w.v0;
    const int per = (pf.wh + (int)gridDim.x - 1) / (int)gridDim.x;
    pf.r0 = min((int)blockIdx.x * per, pf.wh); pf.r1 = min(pf.r0 + per, pf.wh);
    return pf;
}

// f(row, column, D2) for every pixel of rows [r0, r1) with D2 > 0: a row per wave, a column per lane, PALM_BATCH loads in flight per
// lane, no division to recover the row
template <typename F>
__device__ __forceinline__ void for_foreground(const int* D, int r0, int r1, int ww, F f) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = r0 + wave; i < r1; i += PALM_WAVES) {
        const int* row = D + i * ww;
        for (int j0 = lane; j0 < ww; j0 += 64 * PALM_BATCH) {
            int v[PALM_BATCH];
#pragma unroll
            for (int k = 0; k < PALM_BATCH; ++k) v[k] = (j0 + 64 * k < ww) ? row[j0 + 64 * k] : 0;
#pragma unroll
            for (int k = 0; k < PALM_BATCH; ++k)
                if (v[k] > 0) f(i, j0 + 64 * k, v[k]);
        }
    }
}

}  // namespace

__global__ __launch_bounds__(PALM_THREADS) void palm_init_kernel(u64* __restrict__ slots, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * PALM_THREADS + threadIdx.x;
    if (i < n) slots[i] = 0ull;
}

// 1. g: distance along the column to the nearest background row; the ring rows v0 - 1 and v1 are background.  A thread per column and
// direction: the scan down writes the low 16 bits of a pixel's word, the scan up the high 16 bits (g <= 16384); g is the smaller half.
// A workgroup owns a band of rows: a thread first counts the foreground run that reaches its band from outside (sixteen rows loaded per
// step, never past the window), then scans the band.  Both read the frame alone.
__global__ __launch_bounds__(PALM_THREADS) void palm_scan_kernel(PalmArgs a) {
    const PalmFrame pf = palm_frame(a);
    if (pf.code != AWR_DET_OK || pf.r0 >= pf.r1) return;
    const int ww = pf.ww, wh = pf.wh, fw = a.fw;
    const unsigned dlo = (unsigned)pf.w.dlo, dhi = (unsigned)pf.w.dhi;
    uint16_t* D16 = reinterpret_cast<uint16_t*>(pf.D);
    for (int t = threadIdx.x; t < 2 * ww; t += PALM_THREADS) {
        const int up = t >= ww ? 1 : 0, j = t - up * ww;
        const uint16_t* col = pf.F + pf.w.v0 * fw + pf.w.u0 + j;
        const int step = up ? -1 : 1;                                       // the direction the scan moves in
        const int first = up ? pf.r1 - 1 : pf.r0, n_in = pf.r1 - pf.r0;
        const int n_out = up ? wh - pf.r1 : pf.r0;                          // rows of the window behind the band's first row
        int run = 0;
        bool open = true;
        for (int k0 = 0; k0 < n_out && open; k0 += PALM_SCAN) {             // walking back from the band: first - step, first - 2 step, ...
            unsigned d[PALM_SCAN];
#pragma unroll
            for (int k = 0; k < PALM_SCAN; ++k) d[k] = (k0 + k < n_out) ? col[(first - step * (k0 + k + 1)) * fw] : 0u;
#pragma unroll
            for (int k = 0; k < PALM_SCAN; ++k) {
                open = open && k0 + k < n_out && d[k] >= dlo && d[k] <= dhi;
                run += open ? 1 : 0;
            }
        }
        for (int k0 = 0; k0 < n_in; k0 += PALM_SCAN) {
            unsigned d[PALM_SCAN];
#pragma unroll
            for (int k = 0; k < PALM_SCAN; ++k) d[k] = (k0 + k < n_in) ? col[(first + step * (k0 + k)) * fw] : 0u;
#pragma unroll
            for (int k = 0; k < PALM_SCAN; ++k)
                if (k0 + k < n_in) {
                    run = (d[k] >= dlo && d[k] <= dhi) ? run + 1 : 0;
                    D16[2 * ((first + step * (k0 + k)) * ww + j) + up] = (uint16_t)run;
                }
        }
    }
}

// 2. D2(v, u) = min over u' of (u - u')^2 + g(v, u')^2, g = 0 on the ring columns and beyond; in place, over tiles of whole rows whose g
// sits in LDS as uint16.  The maximum of D2, packed with its raster index, leaves as one 64-bit integer atomic per workgroup.
__global__ __launch_bounds__(PALM_THREADS) void palm_rows_kernel(PalmArgs a) {
    __shared__ uint16_t gl[PALM_TILE];
    __shared__ u64 red[PALM_WAVES];
    const PalmFrame pf = palm_frame(a);
    if (pf.code != AWR_DET_OK || pf.r0 >= pf.r1) return;
    const int ww = pf.ww, tid = threadIdx.x;
    int* D = pf.D;
    const int R = max(1, PALM_TILE / ww);
    u64 best = 0;
    for (int i0 = pf.r0; i0 < pf.r1; i0 += R) {
        const int base = i0 * ww, rows = min(R, pf.r1 - i0), tn = rows * ww;
        for (int idx0 = tid; idx0 < tn; idx0 += PALM_THREADS * PALM_BATCH) {
            int v[PALM_BATCH];
#pragma unroll
            for (int k = 0; k < PALM_BATCH; ++k) v[k] = (idx0 + PALM_THREADS * k < tn) ? D[base + idx0 + PALM_THREADS * k] : 0;
#pragma unroll
            for (int k = 0; k < PALM_BATCH; ++k)
                if (idx0 + PALM_THREADS * k < tn) gl[idx0 + PALM_THREADS * k] = (uint16_t)min(v[k] & 0xFFFF, (v[k] >> 16) & 0xFFFF);
        }
        __syncthreads();
        for (int r = tid >> 6; r < rows; r += PALM_WAVES) {                 // a row per wave, a column per lane
            const uint16_t* row = gl + r * ww;
            for (int j = tid & 63; j < ww; j += 64) {
                const int g = row[j];
                if (g == 0) continue;
                int bd = g * g;
                // (every u' is a member of the minimum, so looking past the point where k^2 reaches the best so far changes nothing:
                // four distances per step, their eight LDS reads independent of one another)
                for (int k = 1; k * k < bd; k += 4) {
                    int ga[4], gb[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        ga[q] = (j - k - q >= 0) ? (int)row[j - k - q] : 0;
                        gb[q] = (j + k + q < ww) ? (int)row[j + k + q] : 0;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) bd = min(bd, (k + q) * (k + q) + min(ga[q] * ga[q], gb[q] * gb[q]));
                }
                const int p = base + r * ww + j;
                D[p] = bd;
                const u64 key = pack_key(bd, p);
                best = key > best ? key : best;
            }
        }
        __syncthreads();
    }
    best = block_reduce<PALM_WAVES>(best, red, MaxU64());
    if (threadIdx.x == 0 && best != 0) atomicMax(pf.S + SL_MAX, best);
}

// 3. which = 1: e1 = argmax over S = {tau1 * D2 >= tau0 * m} of |p - e0|^2; which = 2: e2 = argmax over S of |p - e1|^2
__global__ __launch_bounds__(PALM_THREADS) void palm_far_kernel(PalmArgs a, int which) {
    __shared__ u64 red[PALM_WAVES];
    const PalmFrame pf = palm_frame(a);
    if (pf.code != AWR_DET_OK || pf.r0 >= pf.r1 || pf.S[SL_MAX] == 0) return;
    const int ww = pf.ww;
    const i64 tau0m = a.tau0 * (i64)(pf.S[SL_MAX] >> 32), tau1 = a.tau1;
    const int e = key_index(pf.S[which == 1 ? SL_MAX : SL_E1]);
    const i64 ev = e / ww, eu = e % ww;
    u64 best = 0;
    for_foreground(pf.D, pf.r0, pf.r1, ww, [&](int i, int j, int d) {
        const i64 d2 = d;
        if (tau1 * d2 >= tau0m) {
            const i64 dv = i - ev, du = j - eu;
            const u64 key = pack_key(dv * dv + du * du, i * ww + j);
            best = key > best ? key : best;
        }
    });
    best = block_reduce<PALM_WAVES>(best, red, MaxU64());
    if (threadIdx.x == 0 && best != 0) atomicMax(pf.S + (which == 1 ? SL_E1 : SL_E2), best);
}

// the axis of the medial set from the slots: e1, a = e2 - e1, L = |a|^2
struct PalmAxis { i64 e1v, e1u, av, au, L; };
__device__ __forceinline__ PalmAxis palm_axis(const u64* S, int ww) {
    const int e1 = key_index(S[SL_E1]), e2 = key_index(S[SL_E2]);
    PalmAxis x;
    x.e1v = e1 / ww; x.e1u = e1 % ww;
    x.av = e2 / ww - x.e1v; x.au = e2 % ww - x.e1u;
    x.L = x.av * x.av + x.au * x.au;
    return x;
}

// 4. which = 0: b1 = the mask pixels with t < 0, b2 = those with t > L; which = 1: p* = argmax over N of D2
__global__ __launch_bounds__(PALM_THREADS) void palm_end_kernel(PalmArgs a, int which) {
    __shared__ u64 red[PALM_WAVES];
    const PalmFrame pf = palm_frame(a);
    if (pf.code != AWR_DET_OK || pf.r0 >= pf.r1 || pf.S[SL_MAX] == 0) return;
    const int ww = pf.ww;
    const PalmAxis x = palm_axis(pf.S, ww);
    if (x.L == 0) return;                                                   // p* = e0
    if (which == 0) {
        u64 b1 = 0, b2 = 0;
        for_foreground(pf.D, pf.r0, pf.r1, ww, [&](int i, int j, int) {
            const i64 t = (i - x.e1v) * x.av + (j - x.e1u) * x.au;
            b1 += t < 0 ? 1u : 0u;
            b2 += t > x.L ? 1u : 0u;
        });
        b1 = block_reduce<PALM_WAVES>(b1, red, SumU64());
        b2 = block_reduce<PALM_WAVES>(b2, red, SumU64());
        if (threadIdx.x == 0) {
            if (b1) atomicAdd(pf.S + SL_B1, b1);
            if (b2) atomicAdd(pf.S + SL_B2, b2);
        }
        return;
    }
    const i64 m = (i64)(pf.S[SL_MAX] >> 32), tau0m = a.tau0 * m, tau1 = a.tau1, mL = m * x.L;
    const bool far_end = pf.S[SL_B2] >= pf.S[SL_B1];
    u64 bp = 0;
    for_foreground(pf.D, pf.r0, pf.r1, ww, [&](int i, int j, int d) {
        const i64 d2 = d;
        if (tau1 * d2 >= tau0m) {
            const i64 t = (i - x.e1v) * x.av + (j - x.e1u) * x.au;
            const i64 s = far_end ? x.L - t : t;
            if (s <= 0 || s * s <= mL) {
                const u64 key = pack_key(d2, i * ww + j);
                bp = key > bp ? key : bp;
            }
        }
    });
    bp = block_reduce<PALM_WAVES>(bp, red, MaxU64());
    if (threadIdx.x == 0 && bp != 0) atomicMax(pf.S + SL_PS, bp);
}

// the palm point's raster index in the window: e0 where L == 0, otherwise what palm_end_kernel found (N holds the chosen end itself)
__device__ __forceinline__ int palm_point(const u64* S, int ww, int n) {
    const int e0 = key_index(S[SL_MAX]);
    if (palm_axis(S, ww).L == 0 || S[SL_PS] == 0) return e0;
    const int ps = key_index(S[SL_PS]);
    return (ps < 0 || ps >= n) ? e0 : ps;
}

// 5. the palm disc's sums
__global__ __launch_bounds__(PALM_THREADS) void palm_disc_kernel(PalmArgs a) {
    __shared__ u64 red[PALM_WAVES];
    const PalmFrame pf = palm_frame(a);
    if (pf.code != AWR_DET_OK || pf.r0 >= pf.r1 || pf.S[SL_MAX] == 0) return;
    const int ww = pf.ww, fw = a.fw;
    const int ps = palm_point(pf.S, ww, ww * pf.wh);
    const i64 psv = ps / ww, psu = ps % ww, lim = a.rho0 * (i64)pf.D[ps], rho1 = a.rho1;
    const Window w = pf.w;
    const uint16_t* F = pf.F;
    u64 cn = 0, su = 0, sv = 0, sd = 0;
    for_foreground(pf.D, pf.r0, pf.r1, ww, [&](int i, int j, int) {
        const i64 dv = i - psv, du = j - psu;
        if (rho1 * (dv * dv + du * du) <= lim) {
            cn += 1; su += (u64)(w.u0 + j); sv += (u64)(w.v0 + i);
            sd += F[(w.v0 + i) * fw + w.u0 + j];
        }
    });
    cn = block_reduce<PALM_WAVES>(cn, red, SumU64()); su = block_reduce<PALM_WAVES>(su, red, SumU64());
    sv = block_reduce<PALM_WAVES>(sv, red, SumU64()); sd = block_reduce<PALM_WAVES>(sd, red, SumU64());
    if (threadIdx.x == 0 && cn) {
        atomicAdd(pf.S + SL_N, cn); atomicAdd(pf.S + SL_SU, su); atomicAdd(pf.S + SL_SV, sv); atomicAdd(pf.S + SL_SD, sd);
    }
}

// 6. centre, status and info of every frame from its slots: one thread per frame, grid (1, B) so that palm_frame serves it too
__global__ void palm_finalize_kernel(PalmArgs a, double* center_out, int* status_out, int* __restrict__ info) {
    const int b = blockIdx.y;
    const PalmFrame pf = palm_frame(a);
    const double nan = __builtin_nan("");
    double c[3] = {a.center_in[3 * b], a.center_in[3 * b + 1], a.center_in[3 * b + 2]};      // (read before center_out, which may be it)
    int st = pf.code, pu = -1, pv = -1, r2 = 0, nd = 0;
    if (st == AWR_DET_OK && pf.S[SL_MAX] == 0) st = AWR_DET_EMPTY;           // no pixel of the window is in the depth range
    if (st == AWR_DET_OK) {
        const int ps = palm_point(pf.S, pf.ww, pf.ww * pf.wh);
        const double dn = (double)pf.S[SL_N];
        c[0] = (double)pf.S[SL_SU] / dn; c[1] = (double)pf.S[SL_SV] / dn; c[2] = (double)pf.S[SL_SD] / dn;
        pu = pf.w.u0 + ps % pf.ww; pv = pf.w.v0 + ps / pf.ww; r2 = pf.D[ps]; nd = (int)pf.S[SL_N];
    } else if (a.frame[b] < 0 || a.frame[b] >= a.n_frames || a.status_in[b] == AWR_DET_OK) {
        c[0] = c[1] = c[2] = nan;                                           // BAD_FRAME, or EMPTY found here; a code handed in passes through
    }
    center_out[3 * b] = c[0]; center_out[3 * b + 1] = c[1]; center_out[3 * b + 2] = c[2];
    status_out[b] = st;
    if (info) { info[4 * b] = pu; info[4 * b + 1] = pv; info[4 * b + 2] = r2; info[4 * b + 3] = nd; }
}

}  // namespace awr

using namespace awr;

extern "C" {

int64_t awr_detect_palm_scratch(int B, int fh, int fw) {
    if (B <= 0 || B > AWR_DET_MAX_BATCH || !frame_sides_ok(fh, fw)) {
        set_error("awr_detect_palm_scratch: B = %d is outside [1, %d] or the frame of %d x %d is outside [1, %d]^2", B, AWR_DET_MAX_BATCH, fh,
                  fw, FRAME_MAX_SIDE);
        return -1;
    }
    return (int64_t)B * PALM_SLOTS * (int64_t)sizeof(u64) + (int64_t)B * fh * fw * (int64_t)sizeof(int);
}

int awr_detect_palm(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B,
                    const double* center_in, const int* status_in, double zmin, double zmax, const double* cube, int cube_stride, double fx,
                    double fy, double search, int tau_num, int tau_den, int rho2_num, int rho2_den, void* scratch, double* center_out,
                    int* status_out, int* info, void* stream) {
    AWR_REQUIRE(frames && frame && center_in && status_in && cube && scratch && center_out && status_out, "awr_detect_palm: NULL pointer");
    if (check_frame_store("awr_detect_palm", frame_type, B, n_frames, fh, fw) != AWR_OK) return AWR_ERR_ARG;
    AWR_REQUIRE(zmin <= zmax, "awr_detect_palm: depth range needs zmin <= zmax (got %g, %g)", zmin, zmax);
    AWR_REQUIRE(cube_stride == 0 || cube_stride == 3, "awr_detect_palm: cube_stride is 0 (one cube) or 3 (one per frame), not %d", cube_stride);
    AWR_REQUIRE(fx != 0.0 && fy != 0.0 && isfinite(fx) && isfinite(fy), "awr_detect_palm: bad intrinsics");
    AWR_REQUIRE(search > 0.0 && isfinite(search), "awr_detect_palm: search = %g must be > 0 and finite", search);
    AWR_REQUIRE(tau_num > 0 && tau_num <= tau_den, "awr_detect_palm: tau = %d / %d needs 0 < numerator <= denominator", tau_num, tau_den);
    AWR_REQUIRE(rho2_den > 0 && rho2_den <= rho2_num, "awr_detect_palm: rho2 = %d / %d needs 0 < denominator <= numerator", rho2_num, rho2_den);
    AWR_REQUIRE(((uintptr_t)frames & 1) == 0 && ((uintptr_t)scratch & 7) == 0, "awr_detect_palm: misaligned frame store / scratch");
    hipStream_t s = as_stream(stream);
    PalmArgs a;
    a.frames = (const uint16_t*)frames; a.n_frames = n_frames; a.fh = fh; a.fw = fw;
    a.frame = frame; a.center_in = center_in; a.status_in = status_in;
    a.zmin = zmin; a.zmax = zmax; a.cube = cube; a.cube_stride = cube_stride; a.fx = fx; a.fy = fy; a.search = search;
    a.tau0 = tau_num; a.tau1 = tau_den; a.rho0 = rho2_num; a.rho1 = rho2_den;
    a.slots = (u64*)scratch; a.D = (int*)((u64*)scratch + (int64_t)B * PALM_SLOTS);
    const int64_t nw = (int64_t)B * PALM_SLOTS;
    const dim3 grid(frame_parts(B, fh, PALM_MAX_PARTS), B);
    palm_init_kernel<<<(unsigned)((nw + PALM_THREADS - 1) / PALM_THREADS), PALM_THREADS, 0, s>>>(a.slots, nw);
    palm_scan_kernel<<<grid, PALM_THREADS, 0, s>>>(a);
    palm_rows_kernel<<<grid, PALM_THREADS, 0, s>>>(a);
    palm_far_kernel<<<grid, PALM_THREADS, 0, s>>>(a, 1);
    palm_far_kernel<<<grid, PALM_THREADS, 0, s>>>(a, 2);
    palm_end_kernel<<<grid, PALM_THREADS, 0, s>>>(a, 0);
    palm_end_kernel<<<grid, PALM_THREADS, 0, s>>>(a, 1);
    palm_disc_kernel<<<grid, PALM_THREADS, 0, s>>>(a);
    palm_finalize_kernel<<<dim3(1, B), 1, 0, s>>>(a, center_out, status_out, info);
    return check_launch("awr_detect_palm");
}

}  // extern "C"
