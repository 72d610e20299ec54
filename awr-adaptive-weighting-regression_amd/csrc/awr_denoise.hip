// Edge-preserving depth pre-filter: a restatement of awr_amd/detect.py denoise, bit for bit.  Every stage of the
// prediction path reads the sensor's uint16 frame as it arrives; this pass, in front of all of them, takes per pixel the lower median of
// the window's valid depths within `edge` millimetres of the pixel's own (range noise), optionally removes a pixel with too few such
// neighbours (a flying pixel, a speckle) and optionally fills a zero from its valid neighbours (a hole).  The rule stands in
// include/awr_hip.h.  Integers only: depths are compared and selected, never averaged.
//
// Shape: a workgroup of 256 threads per 64 x 16 tile (the hands kernels' tile), blockIdx.y the batch row.  The tile and a halo -- `radius`
// rows above and below, two columns left and right, so that a thread's window starts on an 8-byte boundary -- are staged once in LDS as
// uint16 pairs, (16 + 2 radius) x 68 pixels = 2448 / 2720 bytes, zeros outside the frame.  A thread owns four pixels along a row: it reads
// 2 radius + 1 rows of 8 pixels as two 8-byte LDS loads each, and for each of its pixels builds the window's keys in registers -- the depth
// where the neighbour is valid, a sentinel above every depth where it is not -- and selects element k of their sort by building the
// answer from bit 15 down: the k-th smallest key is the largest v with #{key < v} <= k, so a bit stays set when the count allows it.
// 16 steps of (2 radius + 1)^2 compares, every index static: no private array is indexed dynamically and nothing goes to scratch.
// VEC form (fw a multiple of 4, both bases 8-byte aligned): the halo is staged with 4-byte loads and the four pixels leave as ONE 8-byte
// store; otherwise 2-byte loads and one 2-byte store per pixel.  No atomics, no floating point on the device, no workgroup waits for
// another.  (depth_floor is awr_frame.h's double arithmetic, on the host only: this file is built with -ffp-contract=off.)
#include "awr_frame.h"

namespace awr {
namespace {

constexpr int DN_THREADS = 256, DN_TW = 64, DN_TH = 16;
constexpr int DN_PITCH = (DN_TW + 4) / 2;          // uint16 pairs per staged row: the tile's 64 columns and two on either side
constexpr unsigned DN_NONE = 0xFFFFFFFFu;          // the key of a neighbour that does not count: above every depth

struct DenoiseArgs {
    const uint16_t* frames; int64_t n_frames; int64_t np; int fh, fw;
    const int64_t* frame; int tiles_x;
    int elim, support, fill;
    uint16_t* out; int* status;
};

// element k of the ascending sort of key[0 .. N): at least k + 1 keys are depths (below 65536)
template <int N>
__device__ __forceinline__ unsigned select_kth(const unsigned (&key)[N], int k) {
    unsigned ans = 0;
    for (unsigned bit = 0x8000u; bit != 0; bit >>= 1) {
        const unsigned v = ans | bit;
        int below = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) below += key[i] < v ? 1 : 0;
        if (below <= k) ans = v;
    }
    return ans;
}

template <int R, bool VEC>
__global__ __launch_bounds__(DN_THREADS) void frames_denoise_kernel(DenoiseArgs a) {
    constexpr int ROWS = DN_TH + 2 * R, SIDE = 2 * R + 1, N = SIDE * SIDE;
    __shared__ __attribute__((aligned(16))) unsigned tile[ROWS * DN_PITCH];
    const int b = blockIdx.y, t = threadIdx.x;
    const int64_t f = a.frame[b];
    const bool bad = f < 0 || f >= a.n_frames;                        // outside the store: a zero row, nothing of it is read
    if (blockIdx.x == 0 && t == 0) a.status[b] = bad ? AWR_DET_BAD_FRAME : AWR_DET_OK;
    const int tx0 = ((int)blockIdx.x % a.tiles_x) * DN_TW, ty0 = ((int)blockIdx.x / a.tiles_x) * DN_TH;
    const int x0 = tx0 + (t & 15) * 4, y = ty0 + (t >> 4);
    uint16_t* orow = a.out + (int64_t)b * a.np + (int64_t)y * a.fw;
    if (!bad) {
        // the tile and its halo: staged pair i of row r is frame row ty0 - R + r, columns tx0 - 2 + 2 i and the next one
        const uint16_t* src = a.frames + f * a.np;
        for (int i = t; i < ROWS * DN_PITCH; i += DN_THREADS) {
            const int r = i / DN_PITCH, c = i - r * DN_PITCH;
            const int sy = ty0 - R + r, sx = tx0 - 2 + 2 * c;
            unsigned pair = 0;
            if (sy >= 0 && sy < a.fh) {
                const uint16_t* p = src + (int64_t)sy * a.fw + sx;
                if (VEC) {                                             // sx and fw are even: a pair is inside or outside as a whole
                    if (sx >= 0 && sx < a.fw) pair = *reinterpret_cast<const unsigned*>(p);
                } else {
                    if (sx >= 0 && sx < a.fw) pair = p[0];
                    if (sx + 1 >= 0 && sx + 1 < a.fw) pair |= (unsigned)p[1] << 16;
                }
            }
            tile[i] = pair;
        }
        __syncthreads();
    }
    if (y >= a.fh || x0 >= a.fw) return;
    unsigned res[4] = {0u, 0u, 0u, 0u};
    if (!bad) {
        // rows y - R ... y + R, columns x0 - 2 ... x0 + 5: the thread's pixel j has its centre at w[R][2 + j]
        unsigned w[SIDE][8];
#pragma unroll
        for (int r = 0; r < SIDE; ++r) {
            const uint2* p = reinterpret_cast<const uint2*>(tile + ((t >> 4) + r) * DN_PITCH + (t & 15) * 2);
            const uint2 lo = p[0], hi = p[1];
            w[r][0] = lo.x & 0xFFFFu; w[r][1] = lo.x >> 16; w[r][2] = lo.y & 0xFFFFu; w[r][3] = lo.y >> 16;
            w[r][4] = hi.x & 0xFFFFu; w[r][5] = hi.x >> 16; w[r][6] = hi.y & 0xFFFFu; w[r][7] = hi.y >> 16;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int dp = (int)w[R][2 + j];
            unsigned key[N];
            int n = 0;                                                 // |S| where dp != 0, |V| where it is 0
#pragma unroll
            for (int r = 0; r < SIDE; ++r) {
#pragma unroll
                for (int c = 0; c < SIDE; ++c) {
                    const int dq = (int)w[r][2 - R + j + c];
                    if (r == R && c == R) {
                        key[r * SIDE + c] = dp != 0 ? (unsigned)dp : DN_NONE;
                    } else {
                        const int diff = dq > dp ? dq - dp : dp - dq;
                        const bool counts = dq != 0 && (dp == 0 || diff <= a.elim);
                        key[r * SIDE + c] = counts ? (unsigned)dq : DN_NONE;
                        n += counts ? 1 : 0;
                    }
                }
            }
            // dp != 0: element n / 2 of S and p; dp == 0: element (n - 1) / 2 of V
            const bool keep = dp != 0 ? n >= a.support : (a.fill > 0 && n >= a.fill);
            if (keep) res[j] = select_kth<N>(key, dp != 0 ? n / 2 : (n - 1) / 2);
        }
    }
    if (VEC) {
        *reinterpret_cast<uint2*>(orow + x0) = make_uint2(res[0] | (res[1] << 16), res[2] | (res[3] << 16));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < a.fw) orow[x0 + j] = (uint16_t)res[j];
    }
}

template <int R>
void launch_denoise(const DenoiseArgs& a, bool vec, dim3 grid, hipStream_t s) {
    if (vec) frames_denoise_kernel<R, true><<<grid, DN_THREADS, 0, s>>>(a);
    else frames_denoise_kernel<R, false><<<grid, DN_THREADS, 0, s>>>(a);
}

}  // namespace
}  // namespace awr

using namespace awr;

extern "C" {

int awr_frames_denoise(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B, int radius,
                       double edge, int support, int fill, void* out, int* status, void* stream) {
    if (check_frame_store("awr_frames_denoise", frame_type, B, n_frames, fh, fw) != AWR_OK) return AWR_ERR_ARG;
    AWR_REQUIRE(radius == 1 || radius == 2, "awr_frames_denoise: radius = %d must be 1 or 2", radius);
    const int most = (2 * radius + 1) * (2 * radius + 1) - 1;
    AWR_REQUIRE(edge >= 0.0, "awr_frames_denoise: edge = %g must be >= 0 (infinity: no depth test)", edge);          // (refuses NaN)
    AWR_REQUIRE(support >= 0 && support <= most, "awr_frames_denoise: support = %d is outside [0, %d]", support, most);
    AWR_REQUIRE(fill >= 0 && fill <= most, "awr_frames_denoise: fill = %d is outside [0, %d] (0: no filling)", fill, most);
    AWR_REQUIRE(frames && frame && out && status, "awr_frames_denoise: NULL pointer");
    AWR_REQUIRE(((uintptr_t)frames & 1) == 0 && ((uintptr_t)out & 1) == 0, "awr_frames_denoise: misaligned frame store / output store");
    const int64_t np = (int64_t)fh * fw;
    const uintptr_t in0 = (uintptr_t)frames, in1 = in0 + (uintptr_t)(n_frames * np * 2), out0 = (uintptr_t)out,
                    out1 = out0 + (uintptr_t)((int64_t)B * np * 2);
    AWR_REQUIRE(out1 <= in0 || out0 >= in1, "awr_frames_denoise: out [%p, %p) overlaps the frame store [%p, %p): the pass is not in place",
                (void*)out0, (void*)out1, (void*)in0, (void*)in1);
    DenoiseArgs a;
    a.frames = (const uint16_t*)frames; a.n_frames = n_frames; a.np = np; a.fh = fh; a.fw = fw; a.frame = frame;
    a.tiles_x = (fw + DN_TW - 1) / DN_TW;
    a.elim = depth_floor(edge); a.support = support; a.fill = fill; a.out = (uint16_t*)out; a.status = status;
    const bool vec = fw % 4 == 0 && ((in0 | out0) & 7) == 0;
    const dim3 grid((unsigned)(a.tiles_x * ((fh + DN_TH - 1) / DN_TH)), B);
    if (radius == 1) launch_denoise<1>(a, vec, grid, as_stream(stream));
    else launch_denoise<2>(a, vec, grid, as_stream(stream));
    return check_launch("awr_frames_denoise");
}

}  // extern "C"
