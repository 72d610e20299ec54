// Synthetic hand frames: a depth ray-caster over unions of capsules (include/awr_hip.h "Synthetic hand frames") -- the
// device form of awr_amd/synth.py render(), the same sequence of float64 operations (this file is compiled with -ffp-contract=off).
//
// One workgroup of 256 threads renders one 64 x 16 pixel tile of one frame: thread (tx, ty) renders the 4 horizontally adjacent pixels
// 4 tx ... 4 tx + 3 of row ty and stores them as ONE 64-bit word of packed uint16 (16 lanes cover 128 contiguous bytes of a row; where
// the frame width is no multiple of 4 or the destination is not 8-byte aligned the four values go out as 16-bit stores).  The frame's
// capsule table (K <= 32 rows of 8 doubles, 2 KB) is staged once into LDS together with what the statement computes once per capsule
// (ba, the dot products of a, b and ba, the constant terms of the three quadratics), so the loop over capsules reads LDS at one address
// per wave-instruction (a broadcast).  A tile that lies outside the frame's box writes background and never touches the table.
//
// Status: synth_status_kernel (one thread per frame) writes EMPTY, or BAD_PRIM for a table with a non-finite used row, before the
// render kernel is launched on the same stream; a workgroup of the render kernel that hit anything clears the EMPTY bit with ONE integer
// atomicAnd (an OR over the workgroup decides).  No float atomics, no host synchronisation.  A BAD_PRIM frame is found again by every
// workgroup from the staged table itself (no read of the word other workgroups update) and rendered as background.
#include <limits.h>
#include <math.h>

#include "awr_common.h"

namespace awr {

constexpr int SYNTH_THREADS = 256;
constexpr int SYNTH_PX = 4;                       // pixels per thread: one 64-bit store
constexpr int SYNTH_TX = 16, SYNTH_TY = 16;       // threads of a tile: 64 x 16 pixels
constexpr int SYNTH_TILE_W = SYNTH_TX * SYNTH_PX, SYNTH_TILE_H = SYNTH_TY;
constexpr int SYNTH_CONST = 14;                  // doubles per staged capsule

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    return x ^ (x >> 16);
}

__device__ __forceinline__ uint32_t hash_u32(uint32_t seed, uint32_t frame, uint32_t pixel) {
    uint32_t h = mix32(seed ^ (frame * 0x9E3779B1u));
    return mix32(h ^ (pixel * 0x85EBCA77u));
}

__device__ __forceinline__ bool row_used(const double* p) { return !(p[6] <= 0.0); }

__device__ __forceinline__ bool row_finite(const double* p) {
    bool f = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) f = f && isfinite(p[j]);
    return f;
}

__global__ void synth_status_kernel(const double* __restrict__ prims, int n, int K, int* __restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* P = prims + (int64_t)i * K * 8;
    int code = AWR_SYNTH_EMPTY;
    for (int k = 0; k < K; ++k)
        if (row_used(P + k * 8) && !row_finite(P + k * 8)) code = AWR_SYNTH_BAD_PRIM;
    status[i] = code;
}

// the value of a pixel that is no hit: 0, or the wall (with its noise)
__device__ __forceinline__ uint16_t background_value(int bg, int noise, uint32_t seed, uint32_t frame, uint32_t pixel) {
    if (bg <= 0 || noise <= 0) return (uint16_t)bg;
    const int nz = (int)(hash_u32(seed, frame, pixel) % (uint32_t)(2 * noise + 1)) - noise;
    return (uint16_t)min(max(bg + nz, 1), 65535);
}

template <bool VEC>
__global__ __launch_bounds__(SYNTH_THREADS) void synth_render_kernel(const double* __restrict__ prims, const int* __restrict__ bbox, int K, int fh,
                                                                     int fw, double fx, double fy, double u0, double v0, double flip, int bg,
                                                                     int noise, uint32_t seed, int64_t frame0, uint16_t* __restrict__ out,
                                                                     int64_t row, int* __restrict__ status) {
    __shared__ double s_c[AWR_SYNTH_MAX_PRIMS * SYNTH_CONST];
    __shared__ int s_used[AWR_SYNTH_MAX_PRIMS];
    const int i = blockIdx.z;
    const int tid = threadIdx.x;
    const int tx = tid % SYNTH_TX, ty = tid / SYNTH_TX;
    const int tu = blockIdx.x * SYNTH_TILE_W, tv = blockIdx.y * SYNTH_TILE_H;
    const int u = tu + tx * SYNTH_PX, v = tv + ty;
    const uint32_t frame = (uint32_t)((uint64_t)(frame0 + i) & 0xFFFFFFFFull);
    // the frame's box, clipped to the frame whatever the caller wrote
    const int ulo = max(bbox[i * 4 + 0], 0), vlo = max(bbox[i * 4 + 1], 0), uhi = min(bbox[i * 4 + 2], fw), vhi = min(bbox[i * 4 + 3], fh);
    const bool tile_in_box = tu < uhi && tu + SYNTH_TILE_W > ulo && tv < vhi && tv + SYNTH_TILE_H > vlo;      // workgroup-uniform

    double best[SYNTH_PX];
#pragma unroll
    for (int p = 0; p < SYNTH_PX; ++p) best[p] = INFINITY;

    if (tile_in_box) {
        const double* P = prims + (int64_t)i * K * 8;
        int bad = 0;
        if (tid < K) {
            const double* q = P + tid * 8;
            const int used = row_used(q);
            s_used[tid] = used;
            if (used) {
                bad = !row_finite(q);
                const double ax = q[0], ay = q[1], az = q[2], bx = q[3], by = q[4], bz = q[5], r = q[6];
                const double oax = -ax, oay = -ay, oaz = -az, obx = -bx, oby = -by, obz = -bz;
                const double bax = bx - ax, bay = by - ay, baz = bz - az;
                const double rr = r * r;
                const double baba = (bax * bax + bay * bay) + baz * baz;
                const double baoa = (bax * oax + bay * oay) + baz * oaz;
                const double oaoa = (oax * oax + oay * oay) + oaz * oaz;
                const double obob = (obx * obx + oby * oby) + obz * obz;
                double* c = s_c + tid * SYNTH_CONST;
                c[0] = bax; c[1] = bay; c[2] = baz;
                c[3] = oax; c[4] = oay; c[5] = oaz;
                c[6] = obx; c[7] = oby; c[8] = obz;
                c[9] = baba; c[10] = baoa;
                c[11] = (baba * oaoa - baoa * baoa) - rr * baba;      // cc
                c[12] = oaoa - rr;                                     // ca
                c[13] = obob - rr;                                     // cb
            }
        }
        bad = __syncthreads_or(bad);              // (also the barrier behind the staging)
        if (!bad && u < uhi && u + SYNTH_PX > ulo && v >= vlo && v < vhi) {
            double dx[SYNTH_PX], dd[SYNTH_PX];
            const double dy = flip * (((double)v - v0) / fy);
#pragma unroll
            for (int p = 0; p < SYNTH_PX; ++p) {
                dx[p] = ((double)(u + p) - u0) / fx;
                dd[p] = (dx[p] * dx[p] + dy * dy) + 1.0;
            }
            for (int k = 0; k < K; ++k) {
                if (!s_used[k]) continue;         // wave-uniform
                const double* c = s_c + k * SYNTH_CONST;
                const double bax = c[0], bay = c[1], baz = c[2], oax = c[3], oay = c[4], oaz = c[5], obx = c[6], oby = c[7], obz = c[8];
                const double baba = c[9], baoa = c[10], cc = c[11], ca = c[12], cb = c[13];
#pragma unroll
                for (int p = 0; p < SYNTH_PX; ++p) {
                    const double bard = (bax * dx[p] + bay * dy) + baz;
                    const double rdoa = (dx[p] * oax + dy * oay) + oaz;
                    const double A = baba * dd[p] - bard * bard;
                    const double B = baba * rdoa - baoa * bard;
                    const double H = B * B - A * cc;
                    bool use_a, use_b;
                    if (A > 0.0) {
                        if (!(H > 0.0)) continue;                     // misses the cylinder the capsule lies in
                        const double tc = (-B - sqrt(H)) / A;
                        const double y = baoa + tc * bard;
                        if (y > 0.0 && y < baba && B < 0.0 && cc > 0.0 && tc < best[p]) best[p] = tc;
                        use_a = y <= 0.0;
                        use_b = y >= baba;
                    } else {
                        use_a = use_b = true;
                    }
                    if (use_a) {
                        const double Hs = rdoa * rdoa - dd[p] * ca;
                        if (Hs > 0.0 && rdoa < 0.0 && ca > 0.0) {
                            const double ts = (-rdoa - sqrt(Hs)) / dd[p];
                            if (ts < best[p]) best[p] = ts;
                        }
                    }
                    if (use_b) {
                        const double rdob = (dx[p] * obx + dy * oby) + obz;
                        const double Hs = rdob * rdob - dd[p] * cb;
                        if (Hs > 0.0 && rdob < 0.0 && cb > 0.0) {
                            const double ts = (-rdob - sqrt(Hs)) / dd[p];
                            if (ts < best[p]) best[p] = ts;
                        }
                    }
                }
            }
        }
    }

    // values, noise, stores
    uint16_t val[SYNTH_PX];
    int any_hit = 0;
#pragma unroll
    for (int p = 0; p < SYNTH_PX; ++p) {
        const int uu = u + p;
        const uint32_t pixel = (uint32_t)v * (uint32_t)fw + (uint32_t)uu;
        bool hit = best[p] < INFINITY && uu >= ulo && uu < uhi;      // (rows outside the box never entered the loop)
        int z = 0;
        if (hit) {
            const double zr = floor(best[p] + 0.5);
            z = (int)fmin(fmax(zr, 1.0), 65535.0);
            if (bg > 0 && !(z < bg)) hit = false;
        }
        if (hit) {
            if (noise > 0) {
                const int nz = (int)(hash_u32(seed, frame, pixel) % (uint32_t)(2 * noise + 1)) - noise;
                z = min(max(z + nz, 1), 65535);
            }
            val[p] = (uint16_t)z;
            any_hit = 1;
        } else {
            val[p] = background_value(bg, noise, seed, frame, pixel);
        }
    }
    if (v < fh && u < fw) {
        uint16_t* dst = out + ((row + i) * (int64_t)fh + v) * (int64_t)fw + u;
        if (VEC) {                                // fw % 4 == 0 and an 8-byte aligned destination: u + 3 < fw
            ushort4 w;
            w.x = val[0]; w.y = val[1]; w.z = val[2]; w.w = val[3];
            *reinterpret_cast<ushort4*>(dst) = w;
        } else {
#pragma unroll
            for (int p = 0; p < SYNTH_PX; ++p)
                if (u + p < fw) dst[p] = val[p];
        }
    }
    if (tile_in_box) {                            // workgroup-uniform: every thread reaches the barrier
        any_hit = __syncthreads_or(any_hit);
        if (any_hit && tid == 0) atomicAnd(status + i, ~AWR_SYNTH_EMPTY);
    }
}

}  // namespace awr

using namespace awr;

extern "C" {

int awr_synth_render(const double* prims, const int* bbox, int n, int K, int fh, int fw, double fx, double fy, double u0, double v0, int flip,
                     int background_mm, int noise_mm, unsigned int seed, int64_t frame0, uint16_t* out, int64_t row, int64_t capacity,
                     int* status, void* stream) {
    AWR_REQUIRE(prims && bbox && out && status, "awr_synth_render: NULL pointer");
    AWR_REQUIRE(n > 0 && n <= AWR_SYNTH_MAX_FRAMES, "awr_synth_render: n = %d is outside [1, %d]", n, AWR_SYNTH_MAX_FRAMES);
    AWR_REQUIRE(K > 0 && K <= AWR_SYNTH_MAX_PRIMS, "awr_synth_render: K = %d is outside [1, %d]", K, AWR_SYNTH_MAX_PRIMS);
    AWR_REQUIRE(fh > 0 && fw > 0 && fh <= AWR_SYNTH_MAX_EDGE && fw <= AWR_SYNTH_MAX_EDGE, "awr_synth_render: frame of %d x %d is outside [1, %d]",
                fh, fw, AWR_SYNTH_MAX_EDGE);
    AWR_REQUIRE(flip == 1 || flip == -1, "awr_synth_render: flip = %d is neither 1 nor -1", flip);
    AWR_REQUIRE(fx != 0.0 && fy != 0.0 && isfinite(fx) && isfinite(fy) && isfinite(u0) && isfinite(v0),
                "awr_synth_render: zero focal length or non-finite intrinsics");
    AWR_REQUIRE(background_mm >= 0 && background_mm <= 65535 && noise_mm >= 0 && noise_mm <= 32767,
                "awr_synth_render: background_mm = %d is outside [0, 65535] or noise_mm = %d outside [0, 32767]", background_mm, noise_mm);
    AWR_REQUIRE(frame0 >= 0, "awr_synth_render: frame0 = %lld is negative", (long long)frame0);
    AWR_REQUIRE(row >= 0 && row + n <= capacity, "awr_synth_render: rows [%lld, %lld) do not fit the output (%lld frames)", (long long)row,
                (long long)(row + n), (long long)capacity);
    hipStream_t s = as_stream(stream);
    synth_status_kernel<<<(n + 255) / 256, 256, 0, s>>>(prims, n, K, status);
    const dim3 grid((fw + SYNTH_TILE_W - 1) / SYNTH_TILE_W, (fh + SYNTH_TILE_H - 1) / SYNTH_TILE_H, n);
    const bool vec = fw % SYNTH_PX == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0;
    if (vec)
        synth_render_kernel<true><<<grid, SYNTH_THREADS, 0, s>>>(prims, bbox, K, fh, fw, fx, fy, u0, v0, (double)flip, background_mm, noise_mm, seed,
                                                                  frame0, out, row, status);
    else
        synth_render_kernel<false><<<grid, SYNTH_THREADS, 0, s>>>(prims, bbox, K, fh, fw, fx, fy, u0, v0, (double)flip, background_mm, noise_mm, seed,
                                                                   frame0, out, row, status);
    return check_launch("awr_synth_render");
}

}  // extern "C"
