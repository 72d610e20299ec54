// Hand identities across calls on the device: which of this call's detected hands is which identity of the previous call
// -- the restatement of awr_amd/track.py assign_step, whose outputs and state it equals bit for bit (include/awr_hip.h awr_hands_assign
// spells the definition out).
//
// K <= 4 hands, so an exact assignment is a search over at most 4! = 24 permutations: one wave per frame, lane p < K! decodes permutation p
// in the factorial number system and evaluates (pairs inside the gate, their summed squared distance) from a K x K cost matrix that every
// lane holds in registers, and an xor-shuffle reduction over the TOTAL order (pairs descending, sum ascending, p ascending) leaves the
// winner in every lane, whatever the order of the reduction.  What follows -- outcomes, births, state -- is a few dozen scalar steps that
// every lane of the wave repeats on the same values; lane 0 stores.  The wave then zeroes the temporal filter's rows of the slots that
// started or lost an identity.  No atomics, no LDS, no workgroup waits for another; B frames are B waves, the launch is bound by its own
// latency.  The arithmetic is numpy's: IEEE double + - * / and comparisons in the statement's order (this file is compiled with
// -ffp-contract=off), no square root.  A NaN or Inf in any input is a code, never a fault.
#include <limits.h>
#include <math.h>

#include "awr_frame.h"

namespace awr {

constexpr int ASSIGN_THREADS = 256;
constexpr int ASSIGN_FRAMES = ASSIGN_THREADS / WAVE;          // frames (waves) per workgroup

struct assign_args {
    double* last_uvd;
    int* ids;
    int* miss;
    int* next_id;
    const double* cand_uvd;
    const int* cand_status;
    const double* trk_uvd;
    const int* trk_status;
    int K, B, n_valid, max_miss;
    double gate2, merge2, fx, fy, u0, v0, flip;
    double* filter_state;
    int* filter_count;
    int J;
    double* centers;
    int* status;
    int* code;
    int* reset;
    int* source;
    int* dropped;
};

struct vec3 {
    double x, y, z;
};

__device__ __forceinline__ bool finite3(const vec3& c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.z); }

__device__ __forceinline__ double dist2(const vec3& a, const vec3& b) {
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// the p-th permutation of 0 .. K - 1 in lexicographic order: digit i of p in the factorial number system picks among the elements left
__device__ __forceinline__ void decode_permutation(int p, int K, int perm[MAX_HANDS]) {
    int left = (1 << K) - 1;
#pragma unroll
    for (int i = 0; i < MAX_HANDS; ++i) {
        perm[i] = i;
        if (i < K) {
            const int n = K - 1 - i;
            const int f = n == 3 ? 6 : (n == 2 ? 2 : 1);
            int d = p / f;
            p -= d * f;
            int pick = 0;
#pragma unroll
            for (int e = 0; e < MAX_HANDS; ++e) {
                if ((left >> e) & 1) {
                    if (d == 0) pick = e;
                    --d;
                }
            }
            perm[i] = pick;
            left &= ~(1 << pick);
        }
    }
}

__global__ __launch_bounds__(ASSIGN_THREADS) void hands_assign_kernel(const assign_args a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int b = blockIdx.x * ASSIGN_FRAMES + (threadIdx.x >> 6);
    const int K = a.K, B = a.B;
    if (b >= B) return;                                              // (the whole wave)
    const double nan = __builtin_nan("");
    if (b >= a.n_valid) {                                            // the state stays; the outputs say "nothing here"
        if (lane < K) {
            const int64_t e = (int64_t)lane * B + b;
            a.centers[3 * e] = nan; a.centers[3 * e + 1] = nan; a.centers[3 * e + 2] = nan;
            a.status[e] = AWR_DET_EMPTY; a.code[e] = AWR_ASSIGN_FREE; a.reset[e] = 0; a.source[e] = AWR_ASSIGN_SOURCE_NONE;
        }
        if (lane == 0) a.dropped[b] = 0;
        return;
    }
    // ---- every lane loads the frame's K slots and K candidates (the same addresses across the wave) ----
    int ident[MAX_HANDS], ms[MAX_HANDS], cd[MAX_HANDS];
    bool held[MAX_HANDS], usable[MAX_HANDS], released[MAX_HANDS];
    vec3 trk[MAX_HANDS], cand[MAX_HANDS], r[MAX_HANDS], q[MAX_HANDS];
#pragma unroll
    for (int i = 0; i < MAX_HANDS; ++i) {
        ident[i] = 0; ms[i] = 0; cd[i] = AWR_ASSIGN_FREE;
        held[i] = usable[i] = released[i] = false;
        trk[i] = cand[i] = r[i] = q[i] = vec3{nan, nan, nan};
        if (i < K) {
            const int64_t e = (int64_t)i * B + b;
            ident[i] = a.ids[e];
            ms[i] = a.miss[e];
            const vec3 last = {a.last_uvd[3 * e], a.last_uvd[3 * e + 1], a.last_uvd[3 * e + 2]};
            cand[i] = vec3{a.cand_uvd[3 * e], a.cand_uvd[3 * e + 1], a.cand_uvd[3 * e + 2]};
            usable[i] = a.cand_status[e] == AWR_DET_OK && finite3(cand[i]);
            if (a.trk_uvd) {
                trk[i] = vec3{a.trk_uvd[3 * e], a.trk_uvd[3 * e + 1], a.trk_uvd[3 * e + 2]};
                held[i] = ident[i] > 0 && a.trk_status[e] == AWR_DET_OK && finite3(trk[i]);
            }
            const vec3 from = held[i] ? trk[i] : last;                   // uvd2xyz, in double
            r[i] = vec3{uvd2x(from.x, a.u0, from.z, a.fx), uvd2y(from.y, a.v0, from.z, a.fy, a.flip), from.z};
            q[i] = vec3{uvd2x(cand[i].x, a.u0, cand[i].z, a.fx), uvd2y(cand[i].y, a.v0, cand[i].z, a.fy, a.flip), cand[i].z};
        }
    }
    // ---- 1. two tracked centres on one hand: the younger identity is released ----
#pragma unroll
    for (int i = 0; i < MAX_HANDS; ++i) {
#pragma unroll
        for (int j = i + 1; j < MAX_HANDS; ++j) {
            if (held[i] && held[j] && dist2(r[i], r[j]) <= a.merge2) {
                const bool second = ident[j] > ident[i];
                if (second) { held[j] = false; ident[j] = 0; ms[j] = 0; cd[j] = AWR_ASSIGN_MERGED; released[j] = true; }
                else        { held[i] = false; ident[i] = 0; ms[i] = 0; cd[i] = AWR_ASSIGN_MERGED; released[i] = true; }
            }
        }
    }
    // ---- 2. the cost matrix and the admissible pairs ----
    double c[MAX_HANDS][MAX_HANDS];
    bool adm[MAX_HANDS][MAX_HANDS];
#pragma unroll
    for (int i = 0; i < MAX_HANDS; ++i) {
#pragma unroll
        for (int j = 0; j < MAX_HANDS; ++j) {
            c[i][j] = dist2(r[i], q[j]);
            adm[i][j] = ident[i] > 0 && usable[j] && c[i][j] <= a.gate2;        // (a NaN compares false)
        }
    }
    // ---- 3. lane p evaluates permutation p; the best (m descending, s ascending, p ascending) reaches every lane ----
    const int nperm = K == 4 ? 24 : (K == 3 ? 6 : K);
    int perm[MAX_HANDS];
    int m = -1, p = lane;
    double s = 0.0;
    if (lane < nperm) {
        decode_permutation(lane, K, perm);
        m = 0;
#pragma unroll
        for (int i = 0; i < MAX_HANDS; ++i) {
#pragma unroll
            for (int j = 0; j < MAX_HANDS; ++j) {
                if (perm[i] == j && adm[i][j]) { m += 1; s = s + c[i][j]; }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int m2 = __shfl_xor(m, o, WAVE);
        const double s2 = __shfl_xor(s, o, WAVE);
        const int p2 = __shfl_xor(p, o, WAVE);
        const bool other = m2 > m || (m2 == m && (s2 < s || (s2 == s && p2 < p)));
        if (other) { m = m2; s = s2; p = p2; }
    }
    decode_permutation(p, K, perm);
    // ---- 4. every live slot: tracked, matched, coasting or lost (from here on every lane repeats the same scalar steps) ----
    bool consumed[MAX_HANDS] = {false, false, false, false};
    int out[MAX_HANDS];                                              // the candidate index, SOURCE_TRACKED or SOURCE_NONE
#pragma unroll
    for (int i = 0; i < MAX_HANDS; ++i) {
        out[i] = AWR_ASSIGN_SOURCE_NONE;
        if (ident[i] > 0) {
            int j = -1;
#pragma unroll
            for (int e = 0; e < MAX_HANDS; ++e)
                if (perm[i] == e && adm[i][e]) j = e;
            if (held[i]) {
                out[i] = AWR_ASSIGN_SOURCE_TRACKED; ms[i] = 0; cd[i] = AWR_ASSIGN_TRACKED;
            } else if (j >= 0) {
                out[i] = j; ms[i] = 0; cd[i] = AWR_ASSIGN_MATCHED;
            } else {
                ms[i] += 1;
                if (ms[i] <= a.max_miss) {
                    cd[i] = AWR_ASSIGN_COASTING;
                } else {
                    ident[i] = 0; ms[i] = 0; cd[i] = AWR_ASSIGN_LOST; released[i] = true;
                }
            }
#pragma unroll
            for (int e = 0; e < MAX_HANDS; ++e)
                if (j == e) consumed[e] = true;                      // (a tracked slot's match is the same hand seen twice)
        }
    }
    // ---- 5. births, in candidate order: the lowest free slot, else the slot that has coasted longest ----
    int nid = a.next_id[b], ndropped = 0;
    int born[MAX_HANDS] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < MAX_HANDS; ++j) {
        if (j < K && usable[j] && !consumed[j]) {
            int slot = -1;
#pragma unroll
            for (int i = MAX_HANDS - 1; i >= 0; --i)
                if (i < K && ident[i] == 0) slot = i;
            if (slot < 0) {
                int longest = INT_MIN;
#pragma unroll
                for (int i = 0; i < MAX_HANDS; ++i)
                    if (i < K && cd[i] == AWR_ASSIGN_COASTING && ms[i] > longest) { slot = i; longest = ms[i]; }
            }
            if (slot < 0) {
                ndropped += 1;
            } else {
#pragma unroll
                for (int i = 0; i < MAX_HANDS; ++i)
                    if (i == slot) { ident[i] = nid; ms[i] = 0; cd[i] = AWR_ASSIGN_BORN; out[i] = j; born[i] = 1; }
                if (nid < INT_MAX) nid += 1;
            }
        }
    }
    // ---- 6. outputs and state: lane 0 stores ----
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < MAX_HANDS; ++i) {
            if (i < K) {
                const int64_t e = (int64_t)i * B + b;
                vec3 centre = {nan, nan, nan};
                if (out[i] == AWR_ASSIGN_SOURCE_TRACKED) centre = trk[i];
#pragma unroll
                for (int j = 0; j < MAX_HANDS; ++j)
                    if (out[i] == j) centre = cand[j];
                const bool ok = out[i] != AWR_ASSIGN_SOURCE_NONE;
                a.centers[3 * e] = centre.x; a.centers[3 * e + 1] = centre.y; a.centers[3 * e + 2] = centre.z;
                a.status[e] = ok ? AWR_DET_OK : AWR_DET_EMPTY;
                a.code[e] = cd[i]; a.reset[e] = born[i]; a.source[e] = out[i];
                if (ok || ident[i] == 0) {                           // (a coasting slot keeps where it was last seen)
                    a.last_uvd[3 * e] = centre.x; a.last_uvd[3 * e + 1] = centre.y; a.last_uvd[3 * e + 2] = centre.z;
                }
                a.ids[e] = ident[i]; a.miss[e] = ms[i];
            }
        }
        a.next_id[b] = nid;
        a.dropped[b] = ndropped;
    }
    // ---- the temporal filter's rows of a slot that started or lost an identity: no track (the wave strides over them) ----
    if (a.filter_state) {
#pragma unroll
        for (int i = 0; i < MAX_HANDS; ++i) {
            if (i < K && (born[i] || released[i])) {
                const int64_t row = (int64_t)i * B + b;
                double* S = a.filter_state + row * a.J * 6;
                int* C = a.filter_count + row * a.J * 2;
                for (int t = lane; t < a.J * 6; t += WAVE) S[t] = 0.0;
                for (int t = lane; t < a.J * 2; t += WAVE) C[t] = 0;
            }
        }
    }
}

}  // namespace awr

using namespace awr;

extern "C" {

int awr_hands_assign(double* last_uvd, int* ids, int* miss, int* next_id, const double* cand_uvd, const int* cand_status, const double* trk_uvd,
                     const int* trk_status, int K, int B, int n_valid, double gate_mm, double merge_mm, int max_miss, double fx, double fy,
                     double u0, double v0, int flip, double* filter_state, int* filter_count, int J, double* centers, int* status, int* code,
                     int* reset, int* source, int* dropped, void* stream) {
    AWR_REQUIRE(last_uvd && ids && miss && next_id && cand_uvd && cand_status && centers && status && code && reset && source && dropped,
                "awr_hands_assign: NULL pointer");
    AWR_REQUIRE((trk_uvd == nullptr) == (trk_status == nullptr), "awr_hands_assign: trk_uvd and trk_status come together (one is a NULL pointer)");
    AWR_REQUIRE((filter_state == nullptr) == (filter_count == nullptr),
                "awr_hands_assign: filter_state and filter_count come together (one is a NULL pointer)");
    AWR_REQUIRE(K >= 1 && K <= AWR_ASSIGN_MAX_HANDS, "awr_hands_assign: K = %d is outside [1, %d]", K, AWR_ASSIGN_MAX_HANDS);
    AWR_REQUIRE(B >= 1 && B <= AWR_FILTER_MAX_BATCH, "awr_hands_assign: B = %d is outside [1, %d]", B, AWR_FILTER_MAX_BATCH);
    AWR_REQUIRE(n_valid >= 0 && n_valid <= B, "awr_hands_assign: n_valid = %d is outside [0, B = %d]", n_valid, B);
    AWR_REQUIRE(gate_mm > 0.0 && isfinite(gate_mm), "awr_hands_assign: gate_mm = %g must be finite and positive", gate_mm);
    AWR_REQUIRE(merge_mm >= 0.0 && isfinite(merge_mm), "awr_hands_assign: merge_mm = %g must be finite and >= 0", merge_mm);
    AWR_REQUIRE(max_miss >= 0 && max_miss < INT_MAX, "awr_hands_assign: max_miss = %d is outside [0, %d]", max_miss, INT_MAX - 1);
    AWR_REQUIRE(flip == 1 || flip == -1, "awr_hands_assign: flip = %d is neither +1 nor -1", flip);
    AWR_REQUIRE(fx != 0.0 && fy != 0.0, "awr_hands_assign: a focal length is zero");
    AWR_REQUIRE(!filter_state || (J >= 1 && J <= AWR_FILTER_MAX_JOINTS), "awr_hands_assign: J = %d is outside [1, %d]", J, AWR_FILTER_MAX_JOINTS);
    assign_args a;
    a.last_uvd = last_uvd; a.ids = ids; a.miss = miss; a.next_id = next_id;
    a.cand_uvd = cand_uvd; a.cand_status = cand_status; a.trk_uvd = trk_uvd; a.trk_status = trk_status;
    a.K = K; a.B = B; a.n_valid = n_valid; a.max_miss = max_miss;
    a.gate2 = gate_mm * gate_mm; a.merge2 = merge_mm * merge_mm;
    a.fx = fx; a.fy = fy; a.u0 = u0; a.v0 = v0; a.flip = (double)flip;
    a.filter_state = filter_state; a.filter_count = filter_count; a.J = filter_state ? J : 0;
    a.centers = centers; a.status = status; a.code = code; a.reset = reset; a.source = source; a.dropped = dropped;
    hands_assign_kernel<<<(B + ASSIGN_FRAMES - 1) / ASSIGN_FRAMES, ASSIGN_THREADS, 0, as_stream(stream)>>>(a);
    return check_launch("awr_hands_assign");
}

}  // extern "C"
