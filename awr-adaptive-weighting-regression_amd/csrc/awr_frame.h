// What the prediction path's translation units share (awr_detect.hip, awr_palm.hip, awr_hands.hip, awr_isolate.hip, awr_denoise.hip,
// awr_track.hip, awr_assign.hip): the crop window and the camera model as scalar double arithmetic, and the 64-bit integer
// reductions, launch split and frame-store checks of the kernels that stream over a frame.  Each is written once, here.
//
// Part (a) is the single device statement of nyu_data.center2bounds, evaluator.uvd2xyz and evaluator.xyz2uvd: IEEE double in numpy's
// order of operations, which holds only without contraction -- include its double arithmetic only from a translation unit that
// build.SOURCES compiles with -ffp-contract=off (awr_isolate.hip has no such flag and uses the integers and constants alone).  It has
// no HIP type in it and compiles as plain C++ without hip_runtime.h, so tests/native/frame_math_main.cpp runs it on the host and
// tests/test_frame_math_cpu.py holds it to the numpy statements bit for bit.  Part (b) exists under hipcc only.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/awr_hip.h"

#if defined(__HIPCC__)
#include "awr_common.h"
#define AWR_HD __host__ __device__ __forceinline__
#else
#define AWR_HD inline
#endif

namespace awr {

// ---- (a) scalar arithmetic, host and device ------------------------------------------------------------------------------------------
#if !defined(__HIPCC__)
inline int max(int a, int b) { return a > b ? a : b; }      // (hipcc has its own on both sides; the kernels keep those)
inline int min(int a, int b) { return a < b ? a : b; }
#endif

typedef unsigned long long u64;
typedef long long i64;

constexpr int FRAME_MAX_SIDE = 16384;                 // fh, fw: pixel offsets stay inside int32, sums of columns below 2^44, D2 <= 2^28
constexpr int MAX_HANDS = AWR_DET_MAX_HANDS;          // hand slots per frame: registers and slots are sized by it
static_assert(AWR_ASSIGN_MAX_HANDS == AWR_DET_MAX_HANDS, "the assignment permutes the detector's hand slots");

AWR_HD bool frame_sides_ok(int fh, int fw) { return fh > 0 && fw > 0 && fh <= FRAME_MAX_SIDE && fw <= FRAME_MAX_SIDE; }

// workgroups per frame of a streaming stage: about four per CU over the batch, at most `cap` per frame and never more than one per row
// of the frame (a workgroup's share is whole rows)
inline int frame_parts(int B, int fh, int cap) {
    int p = (1024 + B - 1) / B;
    p = p < fh ? p : fh;
    return p < 1 ? 1 : (p > cap ? cap : p);
}

// int() of a finite double whose value may lie outside int32: every use clips to [0, 16384] afterwards, so clamping first changes nothing
AWR_HD int trunc_clamped(double x) {
    return (int)fmin(fmax(trunc(x), -1073741824.0), 1073741824.0);
}

// the largest integer d in [-1, 65535] with (double)d <= zend
AWR_HD int depth_floor(double zend) {
    return (int)fmin(fmax(floor(zend), -1.0), 65535.0);
}

// zstart <= d <= zend and d != 0 for an integer d in [0, 65535]  <=>  dlo <= d <= dhi
AWR_HD void depth_bounds(double zstart, double zend, int& dlo, int& dhi) {
    if (!(zstart <= zend)) { dlo = 1; dhi = 0; return; }                   // NaN or an empty range
    dlo = max(1, (int)fmin(fmax(ceil(zstart), 0.0), 65536.0));
    dhi = depth_floor(zend);
}

// nyu_data.center2bounds (loader.py:181-188) before its int(): the four pixel bounds of the cube around the centre (u, v, d)
struct Bounds {
    double us, ue, vs, ve;
};
AWR_HD Bounds center_bounds(const double* c, const double* cube, double fx, double fy) {
    const double hu = (cube[0] / 2.0) / c[2] * fx, hv = (cube[1] / 2.0) / c[2] * fy;
    return Bounds{c[0] - hu + 0.5, c[0] + hu + 0.5, c[1] - hv + 0.5, c[1] + hv + 0.5};
}

struct Window {
    int u0, u1, v0, v1;       // clipped to the frame; empty when u0 >= u1 or v0 >= v1
    int dlo, dhi;             // raw depths d with dlo <= d <= dhi (dlo >= 1: zero is "no measurement")
};

// center2bounds clipped to the frame; a non-finite centre or bound is an empty window.  within: a depth range {zmin, zmax} that the cube's
// is intersected with, or none
AWR_HD Window bounds_window(const double* c, const double* cube, double fx, double fy, int fh, int fw, const double* within = nullptr) {
    Window w{0, 0, 0, 0, 1, 0};
    const Bounds b = center_bounds(c, cube, fx, fy);
    if (!(isfinite(b.us) && isfinite(b.ue) && isfinite(b.vs) && isfinite(b.ve) && isfinite(c[2]))) return w;
    w.u0 = max(trunc_clamped(b.us), 0); w.u1 = min(trunc_clamped(b.ue), fw);
    w.v0 = max(trunc_clamped(b.vs), 0); w.v1 = min(trunc_clamped(b.ve), fh);
    depth_bounds(c[2] - cube[2] / 2.0, c[2] + cube[2] / 2.0, w.dlo, w.dhi);
    if (within) {
        int lo, hi;
        depth_bounds(within[0], within[1], lo, hi);
        w.dlo = max(w.dlo, lo); w.dhi = min(w.dhi, hi);
    }
    return w;
}

// awr_detect_palm's search window (detect.palm_center, step 2): bounds_window of the cube scaled by `search`, its depth range intersected
// with [zmin, zmax]
AWR_HD Window palm_window(const double* c, const double* cube, double search, double fx, double fy, double zmin, double zmax, int fh,
                          int fw) {
    const double scaled[3] = {search * cube[0], search * cube[1], search * cube[2]}, within[2] = {zmin, zmax};
    return bounds_window(c, scaled, fx, fy, fh, fw, within);
}

// the pinhole camera in double, a function per component (the third passes through), in evaluator.py's order of operations:
// uvd2xyz (util.py:13-20) is (uvd2x, uvd2y, d); xyz2uvd (util.py:3-10) flips first, yf = y * flip, and is (xyz2u, xyz2v(yf), z).
// flip is +1.0 or -1.0.  (Parameters stand in the order the expression uses them: the optimiser orders the operands of a commutative
// operation by it before these are inlined, and the kernels' instruction streams are pinned to this order.)
AWR_HD double uvd2x(double u, double u0, double d, double fx) { return (u - u0) * d / fx; }
AWR_HD double uvd2y(double v, double v0, double d, double fy, double flip) { return (v - v0) * d / fy * flip; }
AWR_HD double xyz2u(double x, double fx, double z, double u0) { return x * fx / z + u0; }
AWR_HD double xyz2v(double yf, double fy, double z, double v0) { return yf * fy / z + v0; }

// ---- (b) device and launcher helpers -------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (u64)__shfl_xor((i64)v, o, 64);
    return v;
}

struct SumU64 { __device__ __forceinline__ u64 operator()(u64 a, u64 b) const { return a + b; } };
struct MinU64 { __device__ __forceinline__ u64 operator()(u64 a, u64 b) const { return b < a ? b : a; } };
struct MaxU64 { __device__ __forceinline__ u64 operator()(u64 a, u64 b) const { return b > a ? b : a; } };

// op over a workgroup of WAVES waves through LDS (`red`: WAVES words); every thread gets the result, and `red` is free again on return
template <int WAVES, typename Op>
__device__ __forceinline__ u64 block_reduce(u64 v, u64* red, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, (u64)__shfl_xor((i64)v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 r = red[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) r = op(r, red[i]);
    __syncthreads();
    return r;
}

// what every entry point that reads a frame store requires of it
inline int check_frame_store(const char* who, int frame_type, int B, int64_t n_frames, int fh, int fw) {
    AWR_REQUIRE(frame_type == AWR_NYU_U16, "%s: the frame store must be uint16 millimetres (AWR_NYU_U16): every sum and label over a frame is an "
                "integer (got frame_type %d)", who, frame_type);
    AWR_REQUIRE(B > 0 && B <= AWR_DET_MAX_BATCH, "%s: B = %d is outside [1, %d]", who, B, AWR_DET_MAX_BATCH);
    AWR_REQUIRE(n_frames > 0, "%s: n_frames = %lld must be positive", who, (long long)n_frames);
    AWR_REQUIRE(frame_sides_ok(fh, fw), "%s: frame of %d x %d is outside [1, %d]^2", who, fh, fw, FRAME_MAX_SIDE);
    return AWR_OK;
}

#endif  // __HIPCC__

}  // namespace awr
