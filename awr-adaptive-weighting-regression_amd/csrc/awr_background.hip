// Static-scene background model: a restatement of awr_amd/background.py learn and foreground, bit for bit.  Every stage
// of the prediction path assumes that the hand is the nearest thing in the frame; with a fixed sensor over a desk it is not.  A model is
// one uint16 depth per pixel (0: no background known here), learnt once from frames of the empty scene, and a pointwise pass in front of
// every other stage keeps a pixel only where it is at least `margin` millimetres nearer than the model.  The rules stand in
// include/awr_hip.h.  Integers only: depths are compared, selected and stepped, never averaged.
//
// awr_frames_foreground: a streaming pass, blockIdx.y the batch row.  VEC form (fw a multiple of 8 and the three bases 16-byte aligned:
// every row of the stores is then aligned too): a thread owns 8 pixels of a row -- ONE 16-byte load of the frame, one of the model, one
// 16-byte store of the output and, in the ADAPT form of a row below n_valid, one of the model: 6 bytes per pixel, 8 with adapt.
// Otherwise a thread per pixel with 2-byte accesses.  ADAPT is a compile-time form: the form without it has no store to the model in
// its code.  A model pixel is read and written by the one thread that owns it (the entry point refuses several rows on one model with
// adapt), so nothing races.  No atomics, no LDS, no floating point on the device, no workgroup waits for another.
//
// awr_background_learn: once per scene.  A workgroup of 256 threads takes 256 consecutive pixels and stages their n <= 64 depths in
// LDS, frame-major (element i * 256 + t: the lanes of a wave read consecutive uint16, two to a bank word, no conflict), 32 KB at most.
// A thread stages and reads its OWN column only, so the workgroup needs no barrier; LDS is there because a column indexed by a loop
// counter in registers would go to scratch.  Element k of the valid depths is built from bit 15 down out of counts, as awr_denoise.hip's
// select_kth does: the k-th smallest is the largest v with #{valid d < v} <= k.
// (depth_floor is awr_frame.h's double arithmetic, on the host only: this file is built with -ffp-contract=off.)
#include "awr_frame.h"

namespace awr {
namespace {

constexpr int BG_THREADS = 256;
static_assert(AWR_BG_MAX_FRAMES * BG_THREADS * 2 <= 32768, "the learning kernel's staged depths fit 32 KB of LDS");

struct FgArgs {
    const uint16_t* frames; int64_t n_frames; int64_t np;
    const int64_t* frame; int n_valid;
    uint16_t* model; int per_row;
    int margin, unknown_keep, step;
    uint16_t* out; int* status;
};

// the rule for one pixel: -> the output depth; with ADAPT, m becomes the stepped model where the pixel is a valid background pixel
template <bool ADAPT>
__device__ __forceinline__ unsigned fg_pixel(unsigned d, unsigned& m, const FgArgs& a) {
    const bool keep = d != 0 && (m == 0 ? a.unknown_keep == 1 : (int)d + a.margin < (int)m);          // (d + margin <= 131070: int)
    if (ADAPT && d != 0 && m != 0 && !keep) m = (unsigned)((int)m + min(max((int)d - (int)m, -a.step), a.step));
    return keep ? d : 0u;
}

template <bool ADAPT>
__device__ __forceinline__ unsigned fg_pair(unsigned d, unsigned& m, const FgArgs& a) {
    unsigned lo = m & 0xFFFFu, hi = m >> 16;
    const unsigned o = fg_pixel<ADAPT>(d & 0xFFFFu, lo, a) | (fg_pixel<ADAPT>(d >> 16, hi, a) << 16);
    m = lo | (hi << 16);
    return o;
}

template <bool VEC, bool ADAPT>
__global__ __launch_bounds__(BG_THREADS) void frames_foreground_kernel(FgArgs a) {
    const int b = blockIdx.y;
    const int64_t f = a.frame[b];
    const bool bad = f < 0 || f >= a.n_frames;                        // outside the store: a zero row, nothing is read, no adaptation
    if (blockIdx.x == 0 && threadIdx.x == 0) a.status[b] = bad ? AWR_DET_BAD_FRAME : AWR_DET_OK;
    const int64_t i = (int64_t)blockIdx.x * BG_THREADS + threadIdx.x;
    const bool adapts = ADAPT && !bad && b < a.n_valid;
    uint16_t* mrow = a.model + (a.per_row ? (int64_t)b * a.np : 0);
    uint16_t* orow = a.out + (int64_t)b * a.np;
    if (VEC) {
        if (i >= a.np / 8) return;
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        if (!bad) {
            const uint4 d = reinterpret_cast<const uint4*>(a.frames + f * a.np)[i];
            uint4 m = reinterpret_cast<const uint4*>(mrow)[i];
            o.x = fg_pair<ADAPT>(d.x, m.x, a); o.y = fg_pair<ADAPT>(d.y, m.y, a);
            o.z = fg_pair<ADAPT>(d.z, m.z, a); o.w = fg_pair<ADAPT>(d.w, m.w, a);
            if (adapts) reinterpret_cast<uint4*>(mrow)[i] = m;
        }
        reinterpret_cast<uint4*>(orow)[i] = o;
    } else {
        if (i >= a.np) return;
        unsigned o = 0;
        if (!bad) {
            unsigned m = mrow[i];
            o = fg_pixel<ADAPT>(a.frames[f * a.np + i], m, a);
            if (adapts) mrow[i] = (uint16_t)m;
        }
        orow[i] = (uint16_t)o;
    }
}

template <bool VEC>
void launch_foreground(const FgArgs& a, bool adapt, dim3 grid, hipStream_t s) {
    if (adapt) frames_foreground_kernel<VEC, true><<<grid, BG_THREADS, 0, s>>>(a);
    else frames_foreground_kernel<VEC, false><<<grid, BG_THREADS, 0, s>>>(a);
}

struct LearnArgs {
    const uint16_t* frames; int64_t n_frames; int64_t np;
    const int64_t* frame; int n;
    int rank, min_valid;
    uint16_t* model; int* status;
};

__global__ __launch_bounds__(BG_THREADS) void background_learn_kernel(LearnArgs a) {
    __shared__ uint16_t col[AWR_BG_MAX_FRAMES * BG_THREADS];
    const int t = threadIdx.x;
    if (blockIdx.x == 0 && t == 0) {
        int st = AWR_DET_OK;
        for (int i = 0; i < a.n; ++i) {
            const int64_t f = a.frame[i];
            if (f < 0 || f >= a.n_frames) st = AWR_DET_BAD_FRAME;
        }
        a.status[0] = st;
    }
    const int64_t p = (int64_t)blockIdx.x * BG_THREADS + t;
    if (p >= a.np) return;
    int nv = 0;                                                        // |V|
    for (int i = 0; i < a.n; ++i) {
        const int64_t f = a.frame[i];
        const uint16_t d = f < 0 || f >= a.n_frames ? (uint16_t)0 : a.frames[f * a.np + p];          // outside the store: no value
        col[i * BG_THREADS + t] = d;
        nv += d != 0 ? 1 : 0;
    }
    unsigned ans = 0;
    if (nv >= a.min_valid) {                                           // (min_valid >= 1: nv >= 1 here)
        const int k = a.rank == AWR_BG_MIN ? 0 : (a.rank == AWR_BG_MAX ? nv - 1 : (nv - 1) / 2);
        for (unsigned bit = 0x8000u; bit != 0; bit >>= 1) {
            const unsigned v = ans | bit;
            int below = 0;
            for (int i = 0; i < a.n; ++i) below += (unsigned)col[i * BG_THREADS + t] - 1u < v - 1u ? 1 : 0;          // d != 0 and d < v
            if (below <= k) ans = v;
        }
    }
    a.model[p] = (uint16_t)ans;
}

inline bool disjoint(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a1 <= b0 || a0 >= b1; }

}  // namespace
}  // namespace awr

using namespace awr;

extern "C" {

int awr_frames_foreground(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B, int n_valid,
                          void* model, int model_rows, int per_row, double margin, int unknown_keep, int adapt, void* out, int* status,
                          void* stream) {
    if (check_frame_store("awr_frames_foreground", frame_type, B, n_frames, fh, fw) != AWR_OK) return AWR_ERR_ARG;
    AWR_REQUIRE(n_valid >= 0 && n_valid <= B, "awr_frames_foreground: n_valid = %d is outside [0, B = %d]", n_valid, B);
    AWR_REQUIRE(per_row == 0 || per_row == 1, "awr_frames_foreground: per_row = %d must be 0 or 1", per_row);
    AWR_REQUIRE(model_rows >= (per_row ? B : 1), "awr_frames_foreground: model_rows = %d is fewer than the %d the call reads (per_row = %d)",
                model_rows, per_row ? B : 1, per_row);
    AWR_REQUIRE(margin >= 0.0, "awr_frames_foreground: margin = %g must be >= 0 (infinity: nothing in front of a known background is kept)",
                margin);                                                                                         // (refuses NaN)
    AWR_REQUIRE(unknown_keep == 0 || unknown_keep == 1, "awr_frames_foreground: unknown_keep = %d must be 0 or 1", unknown_keep);
    AWR_REQUIRE(adapt >= 0 && adapt <= 65535, "awr_frames_foreground: adapt = %d is outside [0, 65535] (0: the model is only read)", adapt);
    AWR_REQUIRE(!(adapt > 0 && per_row == 0 && B > 1), "awr_frames_foreground: adapt = %d with per_row = 0 and B = %d: several rows would "
                "race on one model", adapt, B);
    AWR_REQUIRE(frames && frame && model && out && status, "awr_frames_foreground: NULL pointer");
    AWR_REQUIRE((((uintptr_t)frames | (uintptr_t)out | (uintptr_t)model) & 1) == 0, "awr_frames_foreground: misaligned frame store / output store / model");
    const int64_t np = (int64_t)fh * fw;
    const uintptr_t in0 = (uintptr_t)frames, in1 = in0 + (uintptr_t)(n_frames * np * 2), out0 = (uintptr_t)out,
                    out1 = out0 + (uintptr_t)((int64_t)B * np * 2), m0 = (uintptr_t)model, m1 = m0 + (uintptr_t)((int64_t)model_rows * np * 2);
    AWR_REQUIRE(disjoint(out0, out1, in0, in1), "awr_frames_foreground: out [%p, %p) overlaps the frame store [%p, %p): the pass is not in place",
                (void*)out0, (void*)out1, (void*)in0, (void*)in1);
    AWR_REQUIRE(disjoint(m0, m1, in0, in1), "awr_frames_foreground: the model [%p, %p) overlaps the frame store [%p, %p)", (void*)m0, (void*)m1,
                (void*)in0, (void*)in1);
    AWR_REQUIRE(disjoint(m0, m1, out0, out1), "awr_frames_foreground: the model [%p, %p) overlaps out [%p, %p)", (void*)m0, (void*)m1, (void*)out0,
                (void*)out1);
    FgArgs a;
    a.frames = (const uint16_t*)frames; a.n_frames = n_frames; a.np = np; a.frame = frame; a.n_valid = n_valid;
    a.model = (uint16_t*)model; a.per_row = per_row; a.margin = depth_floor(margin); a.unknown_keep = unknown_keep; a.step = adapt;
    a.out = (uint16_t*)out; a.status = status;
    const bool vec = fw % 8 == 0 && ((in0 | out0 | m0) & 15) == 0;
    if (vec) launch_foreground<true>(a, adapt > 0, dim3((unsigned)((np / 8 + BG_THREADS - 1) / BG_THREADS), B), as_stream(stream));
    else launch_foreground<false>(a, adapt > 0, dim3((unsigned)((np + BG_THREADS - 1) / BG_THREADS), B), as_stream(stream));
    return check_launch("awr_frames_foreground");
}

int awr_background_learn(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int n, int rank,
                         int min_valid, void* model_out, int* status, void* stream) {
    if (check_frame_store("awr_background_learn", frame_type, 1, n_frames, fh, fw) != AWR_OK) return AWR_ERR_ARG;
    AWR_REQUIRE(n >= 1 && n <= AWR_BG_MAX_FRAMES, "awr_background_learn: n = %d listed frames is outside [1, %d]", n, AWR_BG_MAX_FRAMES);
    AWR_REQUIRE(rank == AWR_BG_MIN || rank == AWR_BG_MEDIAN || rank == AWR_BG_MAX, "awr_background_learn: rank = %d is none of AWR_BG_MIN, "
                "AWR_BG_MEDIAN, AWR_BG_MAX", rank);
    AWR_REQUIRE(min_valid >= 1 && min_valid <= n, "awr_background_learn: min_valid = %d is outside [1, n = %d]", min_valid, n);
    AWR_REQUIRE(frames && frame && model_out && status, "awr_background_learn: NULL pointer");
    AWR_REQUIRE((((uintptr_t)frames | (uintptr_t)model_out) & 1) == 0, "awr_background_learn: misaligned frame store / model");
    const int64_t np = (int64_t)fh * fw;
    const uintptr_t in0 = (uintptr_t)frames, in1 = in0 + (uintptr_t)(n_frames * np * 2), m0 = (uintptr_t)model_out, m1 = m0 + (uintptr_t)(np * 2);
    AWR_REQUIRE(disjoint(m0, m1, in0, in1), "awr_background_learn: model_out [%p, %p) overlaps the frame store [%p, %p)", (void*)m0, (void*)m1,
                (void*)in0, (void*)in1);
    LearnArgs a;
    a.frames = (const uint16_t*)frames; a.n_frames = n_frames; a.np = np; a.frame = frame; a.n = n; a.rank = rank; a.min_valid = min_valid;
    a.model = (uint16_t*)model_out; a.status = status;
    background_learn_kernel<<<dim3((unsigned)((np + BG_THREADS - 1) / BG_THREADS)), BG_THREADS, 0, as_stream(stream)>>>(a);
    return check_launch("awr_background_learn");
}

}  // extern "C"
