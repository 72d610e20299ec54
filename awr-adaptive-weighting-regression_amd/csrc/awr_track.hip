// Temporal joint filter on the device: a One-Euro low-pass per joint and axis with a measurement gate, confidence
// weighting, coasting over lost frames and a constant-velocity look-ahead -- the restatement of awr_amd/track.py filter_step, whose
// results it equals bit for bit (include/awr_hip.h awr_joints_filter spells the definition out).
//
// B * J is at most a few thousand (frame, joint) pairs and each touches eight state words: the launch is bound by its own latency.  One
// thread per pair owns its six doubles and two ints, so there are no atomics, no LDS and no synchronisation.  What matters is that the
// arithmetic is numpy's: IEEE double + - * /, fabs and comparisons in the statement's order (this file is compiled with
// -ffp-contract=off), no square root (the gate compares squared distances) and no transcendental -- w = 2 pi dt, alpha_d and gate^2 are
// the host's, computed once per call by the entry point.  A NaN or Inf in any input is a code, never a fault.
#include <limits.h>
#include <math.h>

#include "awr_frame.h"

namespace awr {

constexpr int TRACK_THREADS = 256;

__global__ __launch_bounds__(TRACK_THREADS) void joints_filter_kernel(double* __restrict__ state, int* __restrict__ count,
                                                                      const float* __restrict__ xyz, const int* __restrict__ status,
                                                                      const int* __restrict__ ustatus, const float* __restrict__ conf, int J,
                                                                      int n, double dt, double w, double alpha_d, double gate2,
                                                                      double min_cutoff, double beta, int max_coast, double conf_floor,
                                                                      double fx, double fy, double u0, double v0, double flip,
                                                                      float* __restrict__ xyz_out, float* __restrict__ uvd_out,
                                                                      float* __restrict__ ahead_out, int* __restrict__ code_out) {
    const int e = blockIdx.x * TRACK_THREADS + threadIdx.x;          // (b, j) = (e / J, e % J); n = n_valid * J
    if (e >= n) return;
    const int b = e / J;
    double* S = state + (int64_t)e * 6;
    int* C = count + (int64_t)e * 2;
    const double z[3] = {(double)xyz[3 * (int64_t)e], (double)xyz[3 * (int64_t)e + 1], (double)xyz[3 * (int64_t)e + 2]};
    const bool ok = status[b] == 0 && ustatus[b] == 0 && isfinite(z[0]) && isfinite(z[1]) && isfinite(z[2]);
    double x[3] = {S[0], S[1], S[2]}, d[3] = {S[3], S[4], S[5]};
    int age = C[0], coast = C[1], code;
    if (age == 0) {
        if (ok) {
            for (int a = 0; a < 3; ++a) { x[a] = z[a]; d[a] = 0.0; }
            age = 1; coast = 0; code = AWR_FILTER_INIT;
        } else {
            code = AWR_FILTER_NONE;
        }
    } else {
        bool accepted = false;
        double y[3] = {0.0, 0.0, 0.0};
        if (ok) {
            for (int a = 0; a < 3; ++a) y[a] = z[a] - x[a];
            const double g2 = (y[0] * y[0] + y[1] * y[1]) + y[2] * y[2];
            accepted = g2 <= gate2;
        }
        if (accepted) {
            double wgt = 1.0;
            if (conf) {
                const double c = (double)conf[e];
                wgt = conf_floor;
                if (c > conf_floor) wgt = c;                         // (a NaN compares false: the floor)
                if (c > 1.0) wgt = 1.0;
            }
            for (int a = 0; a < 3; ++a) {
                const double dx = y[a] / dt;
                d[a] = d[a] + alpha_d * (dx - d[a]);
                const double cut = min_cutoff + beta * fabs(d[a]);
                const double al = 1.0 / (1.0 + 1.0 / (w * cut));
                x[a] = x[a] + (al * wgt) * y[a];
            }
            if (age < INT_MAX) age += 1;
            coast = 0; code = AWR_FILTER_UPDATED;
        } else {
            coast += 1;
            if (coast > max_coast) {
                if (ok) {                                            // the hand really is somewhere else
                    for (int a = 0; a < 3; ++a) { x[a] = z[a]; d[a] = 0.0; }
                    age = 1; coast = 0; code = AWR_FILTER_REINIT;
                } else {
                    for (int a = 0; a < 3; ++a) { x[a] = 0.0; d[a] = 0.0; }
                    age = 0; coast = 0; code = AWR_FILTER_LOST;
                }
            } else {
                code = ok ? AWR_FILTER_GATED : AWR_FILTER_HELD;
            }
        }
    }
    if (code != AWR_FILTER_NONE) {                                   // (NONE leaves the state untouched)
        for (int a = 0; a < 3; ++a) { S[a] = x[a]; S[3 + a] = d[a]; }
        C[0] = age; C[1] = coast;
    }
    float* X = xyz_out + 3 * (int64_t)e;
    float* U = uvd_out + 3 * (int64_t)e;
    float* A = ahead_out + 3 * (int64_t)e;
    if (age > 0) {
        for (int a = 0; a < 3; ++a) {
            X[a] = (float)x[a];
            A[a] = (float)(x[a] + d[a] * dt);
        }
        U[0] = (float)xyz2u(x[0], fx, x[2], u0);
        U[1] = (float)xyz2v(x[1] * flip, fy, x[2], v0);
        U[2] = (float)x[2];
    } else {
        const float nan = __builtin_nanf("");
        for (int a = 0; a < 3; ++a) X[a] = U[a] = A[a] = nan;
    }
    code_out[e] = code;
}

}  // namespace awr

using namespace awr;

extern "C" {

int awr_joints_filter(double* state, int* count, const float* xyz, const int* status, const int* ustatus, const float* conf, int B, int J,
                      int n_valid, double dt, double min_cutoff, double beta, double d_cutoff, double gate_mm, int max_coast, int weight,
                      double conf_floor, double fx, double fy, double u0, double v0, int flip, float* xyz_out, float* uvd_out,
                      float* ahead_out, int* code, void* stream) {
    AWR_REQUIRE(state && count && xyz && status && ustatus && xyz_out && uvd_out && ahead_out && code, "awr_joints_filter: NULL pointer");
    AWR_REQUIRE(weight == 0 || weight == 1, "awr_joints_filter: weight = %d is neither 0 (none) nor 1 (conf)", weight);
    AWR_REQUIRE(!weight || conf, "awr_joints_filter: weight = conf needs the conf array (NULL pointer)");
    AWR_REQUIRE(J >= 1 && J <= AWR_FILTER_MAX_JOINTS, "awr_joints_filter: J = %d is outside [1, %d]", J, AWR_FILTER_MAX_JOINTS);
    AWR_REQUIRE(B >= 1 && B <= AWR_FILTER_MAX_BATCH, "awr_joints_filter: B = %d is outside [1, %d]", B, AWR_FILTER_MAX_BATCH);
    AWR_REQUIRE(n_valid >= 0 && n_valid <= B, "awr_joints_filter: n_valid = %d is outside [0, B = %d]", n_valid, B);
    AWR_REQUIRE(isfinite(dt) && dt > 0.0, "awr_joints_filter: dt = %g must be finite and positive", dt);
    AWR_REQUIRE(min_cutoff > 0.0 && isfinite(min_cutoff), "awr_joints_filter: min_cutoff = %g must be finite and positive", min_cutoff);
    AWR_REQUIRE(beta >= 0.0 && isfinite(beta), "awr_joints_filter: beta = %g must be finite and >= 0", beta);
    AWR_REQUIRE(d_cutoff > 0.0 && isfinite(d_cutoff), "awr_joints_filter: d_cutoff = %g must be finite and positive", d_cutoff);
    AWR_REQUIRE(gate_mm > 0.0 || gate_mm < 0.0, "awr_joints_filter: gate_mm = %g must be positive, or negative for no gate", gate_mm);
    AWR_REQUIRE(max_coast >= 0, "awr_joints_filter: max_coast = %d must be >= 0", max_coast);
    AWR_REQUIRE(conf_floor > 0.0 && conf_floor <= 1.0, "awr_joints_filter: conf_floor = %g is outside (0, 1]", conf_floor);
    AWR_REQUIRE(flip == 1 || flip == -1, "awr_joints_filter: flip = %d is neither +1 nor -1", flip);
    AWR_REQUIRE(fx != 0.0 && fy != 0.0, "awr_joints_filter: a focal length is zero");
    if (n_valid == 0) return AWR_OK;
    // the constants of a call, in the statement's order (M_PI is Python's math.pi)
    const double w = (2.0 * M_PI) * dt;
    const double alpha_d = 1.0 / (1.0 + 1.0 / (w * d_cutoff));
    const double gate2 = gate_mm < 0.0 ? (double)INFINITY : gate_mm * gate_mm;
    const int n = n_valid * J;
    joints_filter_kernel<<<(n + TRACK_THREADS - 1) / TRACK_THREADS, TRACK_THREADS, 0, as_stream(stream)>>>(
        state, count, xyz, status, ustatus, weight ? conf : nullptr, J, n, dt, w, alpha_d, gate2, min_cutoff, beta, max_coast, conf_floor, fx,
        fy, u0, v0, (double)flip, xyz_out, uvd_out, ahead_out, code);
    return check_launch("awr_joints_filter");
}

}  // extern "C"
