// Joint scoring on the device: the reference's EvalUtil.feed (util/eval_tool.py:20-46) and its pinhole back-projection
// (util/util.py:13-20) for a whole batch per launch -- predicted normalised uvd joints -> original-image uvd -> camera xyz ->
// per-joint Euclidean error in mm against the rescaled ground truth -- a restatement of awr_amd/evaluator.py EvalUtil.feed_batch.
//
// B * J is at most a few thousand elements, so ONE workgroup scores the batch: nothing here is bound by anything but launch
// latency.  What matters is (1) the arithmetic is numpy's, step by step and in numpy's precisions (float32 rescalings, float64
// homogeneous product and back-projection, float32 sum of squares; this file is compiled with -ffp-contract=off), (2) the
// float64 accumulators are updated by an ordered in-workgroup reduction with one writer per word -- no floating-point atomics,
// so two runs over the same batches leave bitwise equal accumulators, (3) a singular or non-finite crop matrix is a status
// code and a NaN row, never a fault.
#include <limits.h>
#include <math.h>

#include "awr_common.h"

namespace awr {

constexpr int EVAL_THREADS = 256;
constexpr int EVAL_ELEMS = 4096;        // (frame, joint) errors of one chunk held in LDS
constexpr int EVAL_FRAMES = 1024;       // frames of one chunk

// rows 0 and 1 of inv(M) (row 2 never reaches the result: eval_tool.py:40-41 keeps [:2] of the homogeneous product) as the adjugate of
// the float32 matrix over its determinant, all in float64 (products of two float32 values are exact there).  Returns the frame's status.
__device__ __forceinline__ int inverse_rows(const float* __restrict__ M, double* r) {
    double m[9];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        m[i] = (double)M[i];
        finite = finite && isfinite(m[i]);
    }
    if (!finite) return AWR_EVAL_NONFINITE;
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[2] * m[7] - m[1] * m[8], c02 = m[1] * m[5] - m[2] * m[4];
    const double c10 = m[5] * m[6] - m[3] * m[8], c11 = m[0] * m[8] - m[2] * m[6], c12 = m[2] * m[3] - m[0] * m[5];
    const double c20 = m[3] * m[7] - m[4] * m[6];
    const double det = (m[0] * c00 + m[1] * c10) + m[2] * c20;
    if (det == 0.0 || !isfinite(det)) return AWR_EVAL_SINGULAR;
    r[0] = c00 / det; r[1] = c01 / det; r[2] = c02 / det;
    r[3] = c10 / det; r[4] = c11 / det; r[5] = c12 / det;
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (!isfinite(r[i])) return AWR_EVAL_SINGULAR;
    return AWR_EVAL_OK;
}

// one predicted joint, normalised uvd -> original-image uvd (u, v, d) and camera x, y in mm (z = d): eval_tool.py:38-41 + util.py:13-20
__device__ __forceinline__ void unproject_joint(const float* __restrict__ p, const float* __restrict__ c, const float* __restrict__ cb,
                                                const double* r, float img_size, double fx, double fy, double u0, double v0, float flip,
                                                float& u, float& v, float& d, float& x, float& y) {
    u = (p[0] + 1.f) * img_size / 2.0f;                          // eval_tool.py:38, float32
    v = (p[1] + 1.f) * img_size / 2.0f;
    d = p[2] * cb[2] / 2.0f + c[2];                              // :39
    const double hu = (double)u, hv = (double)v;                 // :40-41, float64 against inv(M), stored as float32
    u = (float)((r[0] * hu + r[1] * hv) + r[2]);
    v = (float)((r[3] * hu + r[4] * hv) + r[5]);
    x = (float)(((double)u - u0) * (double)d / fx);              // util.py:13-20, float64 against the intrinsics, stored as float32
    y = (float)(((double)v - v0) * (double)d / fy) * flip;
}

// The label-free half of eval_batch_kernel: joints -> original-image uvd and camera xyz, one status code per frame.
__global__ __launch_bounds__(EVAL_THREADS) void joints_unproject_kernel(const float* __restrict__ pred, const float* __restrict__ center,
                                                                        const float* __restrict__ M, const float* __restrict__ cube, int J,
                                                                        int n_valid, float img_size, double fx, double fy, double u0, double v0,
                                                                        float flip, float* __restrict__ uvd_out, float* __restrict__ xyz_out,
                                                                        int* __restrict__ status) {
    for (int e = threadIdx.x; e < n_valid * J; e += EVAL_THREADS) {
        const int64_t b = e / J;
        const int j = e - (int)b * J;
        double r[6];
        const int code = inverse_rows(M + b * 9, r);
        float u, v, d, x, y;
        if (code == AWR_EVAL_OK) unproject_joint(pred + (b * J + j) * 3, center + b * 3, cube + b * 3, r, img_size, fx, fy, u0, v0, flip, u, v, d, x, y);
        else u = v = d = x = y = __builtin_nanf("");
        float* o = uvd_out + (b * J + j) * 3;
        o[0] = u; o[1] = v; o[2] = d;
        float* q = xyz_out + (b * J + j) * 3;
        q[0] = x; q[1] = y; q[2] = d;
        if (j == 0) status[b] = code;
    }
}

__global__ __launch_bounds__(EVAL_THREADS) void eval_batch_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                  const float* __restrict__ center, const float* __restrict__ M,
                                                                  const float* __restrict__ cube, int J, int n_valid, float img_size,
                                                                  double fx, double fy, double u0, double v0, float flip,
                                                                  float* __restrict__ uvd_out, float* __restrict__ err_out, int64_t row,
                                                                  double* __restrict__ acc, int* __restrict__ status) {
    __shared__ float s_err[EVAL_ELEMS];
    __shared__ double s_fmean[EVAL_FRAMES];
    __shared__ int s_code[EVAL_FRAMES];
    __shared__ int s_bad;                  // (frame << 2 | code) of the first bad frame of the batch
    const int tid = threadIdx.x;
    const int chunk = min(EVAL_ELEMS / J, EVAL_FRAMES);
    double jsum = 0.0;                     // thread j < J: error sum of joint j over the batch's frames, in frame order
    double fsum = 0.0, fcnt = 0.0;         // thread 0: sum of the per-frame mean errors, frames scored
    if (tid == 0) s_bad = INT_MAX;
    __syncthreads();
    for (int f0 = 0; f0 < n_valid; f0 += chunk) {
        const int nf = min(chunk, n_valid - f0);
        for (int e = tid; e < nf * J; e += EVAL_THREADS) {
            const int f = e / J, j = e - f * J;
            const int64_t b = f0 + f;
            double r[6];
            const int code = inverse_rows(M + b * 9, r);
            const float* p = pred + (b * J + j) * 3;
            const float* c = center + b * 3;
            const float* cb = cube + b * 3;
            float u, v, d, err;
            if (code == AWR_EVAL_OK) {
                float x, y;
                unproject_joint(p, c, cb, r, img_size, fx, fy, u0, v0, flip, u, v, d, x, y);
                const float* g = gt + (b * J + j) * 3;
                const float dx = (g[0] * (cb[0] / 2.0f) + c[0]) - x;         // :46, float32
                const float dy = (g[1] * (cb[1] / 2.0f) + c[1]) - y;
                const float dz = (g[2] * (cb[2] / 2.0f) + c[2]) - d;
                err = sqrtf((dx * dx + dy * dy) + dz * dz);
            } else {
                u = v = d = err = __builtin_nanf("");
                if (j == 0) atomicMin(&s_bad, (int)((b << 2) | code));
            }
            if (j == 0) s_code[f] = code;
            s_err[e] = err;
            if (uvd_out) {
                float* o = uvd_out + ((row + b) * J + j) * 3;
                o[0] = u; o[1] = v; o[2] = d;
            }
            if (err_out) err_out[(row + b) * J + j] = err;
        }
        __syncthreads();
        if (tid < J)
            for (int f = 0; f < nf; ++f)
                if (s_code[f] == AWR_EVAL_OK) jsum += (double)s_err[f * J + tid];
        for (int f = tid; f < nf; f += EVAL_THREADS) {
            double m = 0.0;
            for (int j = 0; j < J; ++j) m += (double)s_err[f * J + j];
            s_fmean[f] = m / (double)J;
        }
        __syncthreads();
        if (tid == 0)
            for (int f = 0; f < nf; ++f)
                if (s_code[f] == AWR_EVAL_OK) {
                    fsum += s_fmean[f];
                    fcnt += 1.0;
                }
        __syncthreads();                   // the next chunk overwrites s_err / s_code / s_fmean
    }
    // one writer per accumulator word; launches on a stream are ordered, so the running sums depend on the feed order alone
    if (tid < J) acc[tid] += jsum;
    if (tid == 0) {
        acc[J] += fcnt;
        acc[J + 1] += fsum;
        if (s_bad != INT_MAX && status[0] == AWR_EVAL_OK) {      // the first bad frame of a run is the one reported
            status[0] = s_bad & 3;
            status[1] = (int)(row + (s_bad >> 2));
        }
    }
}

}  // namespace awr

using namespace awr;

extern "C" {

int awr_eval_batch(const float* jt_pred, const float* jt_xyz_gt, const float* center_xyz, const float* M, const float* cube, int B, int J,
                   int n_valid, float img_size, double fx, double fy, double u0, double v0, int flip, float* uvd_out, float* err_out,
                   int64_t row, int64_t capacity, double* acc, int* status, void* stream) {
    AWR_REQUIRE(jt_pred && jt_xyz_gt && center_xyz && M && cube && acc && status, "awr_eval_batch: NULL pointer");
    AWR_REQUIRE(B > 0 && B < (1 << 28) && J > 0 && J <= AWR_EVAL_MAX_JOINTS, "awr_eval_batch: bad sizes (B = %d, J = %d; J <= %d)", B, J,
                AWR_EVAL_MAX_JOINTS);
    AWR_REQUIRE(n_valid >= 0 && n_valid <= B, "awr_eval_batch: n_valid = %d is outside [0, B = %d]", n_valid, B);
    AWR_REQUIRE(img_size > 0.f && fx != 0.0 && fy != 0.0 && (flip == 1 || flip == -1), "awr_eval_batch: bad img_size / intrinsics / flip");
    AWR_REQUIRE(row >= 0 && row < INT_MAX - B, "awr_eval_batch: row offset %lld out of range", (long long)row);
    if (uvd_out || err_out)
        AWR_REQUIRE(row + n_valid <= capacity, "awr_eval_batch: rows [%lld, %lld) do not fit the result buffers (%lld rows)", (long long)row,
                    (long long)(row + n_valid), (long long)capacity);
    if (n_valid == 0) return AWR_OK;
    eval_batch_kernel<<<1, EVAL_THREADS, 0, as_stream(stream)>>>(jt_pred, jt_xyz_gt, center_xyz, M, cube, J, n_valid, img_size, fx, fy, u0, v0,
                                                                 (float)flip, uvd_out, err_out, row, acc, status);
    return check_launch("awr_eval_batch");
}

int awr_joints_unproject(const float* jt_pred, const float* center_xyz, const float* M, const float* cube, int B, int J, int n_valid,
                         float img_size, double fx, double fy, double u0, double v0, int flip, float* uvd_out, float* xyz_out, int* status,
                         void* stream) {
    AWR_REQUIRE(jt_pred && center_xyz && M && cube && uvd_out && xyz_out && status, "awr_joints_unproject: NULL pointer");
    AWR_REQUIRE(B > 0 && B < (1 << 20) && J > 0 && J <= AWR_EVAL_MAX_JOINTS, "awr_joints_unproject: bad sizes (B = %d, J = %d; J <= %d)", B, J,
                AWR_EVAL_MAX_JOINTS);
    AWR_REQUIRE(n_valid >= 0 && n_valid <= B, "awr_joints_unproject: n_valid = %d is outside [0, B = %d]", n_valid, B);
    AWR_REQUIRE(img_size > 0.f && fx != 0.0 && fy != 0.0 && (flip == 1 || flip == -1), "awr_joints_unproject: bad img_size / intrinsics / flip");
    if (n_valid == 0) return AWR_OK;
    joints_unproject_kernel<<<1, EVAL_THREADS, 0, as_stream(stream)>>>(jt_pred, center_xyz, M, cube, J, n_valid, img_size, fx, fy, u0, v0, (float)flip,
                                                                       uvd_out, xyz_out, status);
    return check_launch("awr_joints_unproject");
}

}  // extern "C"
