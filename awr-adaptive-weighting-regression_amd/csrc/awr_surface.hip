// Label-free check of joints against the depth frame: a restatement of awr_amd/surface.py joints_surface, bit for bit.
// A joint lies inside the hand, a few millimetres behind the surface the sensor sees at its pixel: per joint, and per sample along a bone,
// the window of raw depths around the point's pixel says whether that surface is roughly there (ON), something much nearer covers it
// (OCCLUDED) or only background or nothing is there (OFF).  The rule stands in include/awr_hip.h.
//
// Shape: one wave per row (a workgroup of 64 threads, blockIdx.x the row, only rows below n_valid are launched).  The lanes stride over
// the row's J + n_bones * samples points -- at most 256 + 64 * 7, so a lane loops up to 11 times -- and each gathers its (2 radius + 1)^2
// window with plain 2-byte loads: a hand's joints are scattered over the frame, and a launch of this size is bound by its latency, not by
// the bytes it moves.  A lane keeps its four joint counts and its four sample counts as 16-bit fields of two 64-bit words (a row has at
// most 704 points), which two wave_sums add; lanes 0 ... 7 write the eight counts.  Everything is a comparison or a difference in double; the
// one interpolation is A + (B - A) * t without contraction (this file is built with -ffp-contract=off).  No atomics, no LDS, no private
// array, nothing synchronises.
#include "awr_frame.h"

namespace awr {
namespace {

constexpr int SF_THREADS = 64;
constexpr unsigned SF_NAN = 0x7FC00000u;          // the quiet NaN numpy writes: gaps are compared as bit patterns

struct SurfaceArgs {
    const uint16_t* frames; int64_t n_frames; int64_t np; int fh, fw;
    const int64_t* frame; const float* uvd; const int* status; const int* ustatus; int J;
    const int* bones; int n_bones, samples;
    int radius; double in_mm, out_mm; int min_on;
    int* codes; float* gap; int* counts; int* row_status;
};

// floor(x + 0.5) of a finite double as an int: clamped first, as trunc_clamped is (every use compares with [0, 16384) afterwards)
__device__ __forceinline__ int round_clamped(double x) {
    return (int)fmin(fmax(floor(x + 0.5), -1073741824.0), 1073741824.0);
}

// steps 1 - 7 of the rule for one point of frame `src`: the code, and the gap as float32 bits
__device__ __forceinline__ int point_code(const SurfaceArgs& a, const uint16_t* __restrict__ src, double u, double v, double d, unsigned& gap) {
    gap = SF_NAN;
    if (!(isfinite(u) && isfinite(v) && isfinite(d))) return AWR_SURFACE_OUTSIDE;
    const int pu = round_clamped(u), pv = round_clamped(v);
    if (pu < 0 || pu >= a.fw || pv < 0 || pv >= a.fh) return AWR_SURFACE_OUTSIDE;
    const int x0 = max(pu - a.radius, 0), x1 = min(pu + a.radius, a.fw - 1), y0 = max(pv - a.radius, 0), y1 = min(pv + a.radius, a.fh - 1);
    int n_on = 0, n_front = 0;
    bool any = false;
    double best = 0.0, best_abs = 0.0;
    for (int y = y0; y <= y1; ++y) {
        const uint16_t* row = src + (int64_t)y * a.fw;
        for (int x = x0; x <= x1; ++x) {
            const int dq = row[x];
            if (dq == 0) continue;
            const double g = d - (double)dq, ag = fabs(g);
            n_on += (g >= -a.out_mm && g <= a.in_mm) ? 1 : 0;
            n_front += g > a.in_mm ? 1 : 0;
            if (!any || ag < best_abs || (ag == best_abs && g > best)) { best = g; best_abs = ag; }
            any = true;
        }
    }
    if (any) gap = __float_as_uint((float)best);
    return n_on >= a.min_on ? AWR_SURFACE_ON : (n_front >= 1 ? AWR_SURFACE_OCCLUDED : AWR_SURFACE_OFF);
}

__global__ __launch_bounds__(SF_THREADS) void joints_surface_kernel(SurfaceArgs a) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int64_t f = a.frame[r];
    int* codes = a.codes + (int64_t)r * a.J;
    unsigned* gaps = reinterpret_cast<unsigned*>(a.gap) + (int64_t)r * a.J;
    int rs = AWR_SURFACE_ROW_OK;
    if (a.status[r] != AWR_DET_OK || a.ustatus[r] != 0) rs = AWR_SURFACE_ROW_SKIPPED;
    else if (f < 0 || f >= a.n_frames) rs = AWR_SURFACE_ROW_BAD_FRAME;                // outside the store: nothing of it is read
    if (rs != AWR_SURFACE_ROW_OK) {                                                  // (uniform over the wave)
        for (int j = lane; j < a.J; j += SF_THREADS) { codes[j] = AWR_SURFACE_SKIPPED; gaps[j] = SF_NAN; }
        if (lane < 8) a.counts[(int64_t)r * 8 + lane] = 0;
        if (lane == 0) a.row_status[r] = rs;
        return;
    }
    const float* uvd = a.uvd + (int64_t)r * a.J * 3;
    const uint16_t* src = a.frames + f * a.np;
    const int total = a.J + a.n_bones * a.samples;
    u64 cj = 0, cs = 0;                                                               // four 16-bit counts each: ON, OCCLUDED, OFF, OUTSIDE
    for (int i = lane; i < total; i += SF_THREADS) {
        double u, v, d;
        if (i < a.J) {
            u = (double)uvd[3 * i]; v = (double)uvd[3 * i + 1]; d = (double)uvd[3 * i + 2];
        } else {
            const int k = i - a.J, b = k / a.samples, s = k - b * a.samples + 1;
            const int ja = a.bones[2 * b], jb = a.bones[2 * b + 1];
            u = v = d = __longlong_as_double(0x7FF8000000000000ll);                    // a bone with an index outside [0, J): OUTSIDE
            if (ja >= 0 && ja < a.J && jb >= 0 && jb < a.J) {
                const double t = (double)s / (double)(a.samples + 1);
                const double au = (double)uvd[3 * ja], av = (double)uvd[3 * ja + 1], ad = (double)uvd[3 * ja + 2];
                u = au + ((double)uvd[3 * jb] - au) * t;
                v = av + ((double)uvd[3 * jb + 1] - av) * t;
                d = ad + ((double)uvd[3 * jb + 2] - ad) * t;
            }
        }
        unsigned gap;
        const int code = point_code(a, src, u, v, d, gap);
        if (i < a.J) {
            codes[i] = code; gaps[i] = gap;
            cj += (u64)1 << (16 * code);
        } else {
            cs += (u64)1 << (16 * code);
        }
    }
    cj = wave_sum(cj); cs = wave_sum(cs);
    if (lane < 8) a.counts[(int64_t)r * 8 + lane] = (int)(((lane < 4 ? cj : cs) >> (16 * (lane & 3))) & 0xFFFFu);
    if (lane == 0) a.row_status[r] = AWR_SURFACE_ROW_OK;
}

}  // namespace
}  // namespace awr

using namespace awr;

extern "C" {

int awr_joints_surface(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, const float* uvd,
                       const int* status, const int* ustatus, int n, int J, int n_valid, const int* bones, int n_bones, int samples, int radius,
                       double in_mm, double out_mm, int min_on, int* codes, float* gap_mm, int* counts, int* row_status, void* stream) {
    if (check_frame_store("awr_joints_surface", frame_type, n, n_frames, fh, fw) != AWR_OK) return AWR_ERR_ARG;
    AWR_REQUIRE(J >= 1 && J <= AWR_SURFACE_MAX_JOINTS, "awr_joints_surface: J = %d is outside [1, %d]", J, AWR_SURFACE_MAX_JOINTS);
    AWR_REQUIRE(n_valid >= 0 && n_valid <= n, "awr_joints_surface: n_valid = %d is outside [0, n = %d]", n_valid, n);
    AWR_REQUIRE(radius >= 0 && radius <= AWR_SURFACE_MAX_RADIUS, "awr_joints_surface: radius = %d is outside [0, %d]", radius, AWR_SURFACE_MAX_RADIUS);
    const int most = (2 * radius + 1) * (2 * radius + 1);
    AWR_REQUIRE(isfinite(in_mm) && in_mm >= 0.0, "awr_joints_surface: in_mm = %g must be finite and >= 0", in_mm);
    AWR_REQUIRE(isfinite(out_mm) && out_mm >= 0.0, "awr_joints_surface: out_mm = %g must be finite and >= 0", out_mm);
    AWR_REQUIRE(min_on >= 1 && min_on <= most, "awr_joints_surface: min_on = %d is outside [1, %d]", min_on, most);
    AWR_REQUIRE(n_bones >= 0 && n_bones <= AWR_SURFACE_MAX_BONES, "awr_joints_surface: n_bones = %d is outside [0, %d]", n_bones, AWR_SURFACE_MAX_BONES);
    AWR_REQUIRE(samples >= 1 && samples <= AWR_SURFACE_MAX_SAMPLES, "awr_joints_surface: samples = %d is outside [1, %d]", samples, AWR_SURFACE_MAX_SAMPLES);
    AWR_REQUIRE(frames && frame && uvd && status && ustatus && codes && gap_mm && counts && row_status, "awr_joints_surface: NULL pointer");
    AWR_REQUIRE(n_bones == 0 || bones, "awr_joints_surface: n_bones = %d needs the bone table (NULL pointer)", n_bones);
    AWR_REQUIRE(((uintptr_t)frames & 1) == 0, "awr_joints_surface: misaligned frame store");
    if (n_valid == 0) return AWR_OK;
    SurfaceArgs a;
    a.frames = (const uint16_t*)frames; a.n_frames = n_frames; a.np = (int64_t)fh * fw; a.fh = fh; a.fw = fw;
    a.frame = frame; a.uvd = uvd; a.status = status; a.ustatus = ustatus; a.J = J;
    a.bones = bones; a.n_bones = n_bones; a.samples = samples;
    a.radius = radius; a.in_mm = in_mm; a.out_mm = out_mm; a.min_on = min_on;
    a.codes = codes; a.gap = gap_mm; a.counts = counts; a.row_status = row_status;
    joints_surface_kernel<<<n_valid, SF_THREADS, 0, as_stream(stream)>>>(a);
    return check_launch("awr_joints_surface");
}

}  // extern "C"
