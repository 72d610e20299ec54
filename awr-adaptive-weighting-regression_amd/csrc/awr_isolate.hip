// A frame per hand: the frame with every OTHER labelled component removed -- a restatement of awr_amd/detect.py isolate,
// bit for bit.  awr_detect_hands keeps a seed per hand and every later stage reads the whole raw frame again, so two hands closer than
// half a crop cube stand in each other's refinement window and in each other's crop.  This pass writes, per frame b and hand slot k, row
// k * B + b of an output store in the FrameStore layout: pixel p of the frame where labels[p] < 0 or labels[p] == root_k, 0 elsewhere; a
// slot without a component (root_k < 0) gets the unchanged frame.  Integer selects only: no arithmetic on a depth.
//
// Shape: one pass per frame, a thread per 8 pixels -- ONE 16-byte load of the frame, two of its labels, K 16-byte stores -- so the frame
// and its labels are read once however large K is: (2 + 4 + 2 K) bytes per pixel, all of it streamed.  The 8-pixel form needs fh * fw to
// be a multiple of 8 and the three bases 16-byte aligned (every row of the stores is then aligned too); anything else takes the scalar
// form, a thread per pixel.  No atomics, no LDS, no workgroup waits for another, nothing synchronises.
// (This file is built WITHOUT -ffp-contract=off: of awr_frame.h it uses the constants and the frame-store checks, none of its doubles.)
#include "awr_frame.h"

namespace awr {
namespace {

constexpr int ISO_THREADS = 256;

struct IsoArgs {
    const uint16_t* frames; int64_t n_frames; int64_t np; int fw;
    const int64_t* frame; int B, K;
    const int* labels; const int* info;
    uint16_t* out; int* status;
};

// the roots of frame b's slots; -1: the slot has no component
__device__ __forceinline__ void iso_roots(const IsoArgs& a, int b, int (&root)[MAX_HANDS]) {
#pragma unroll
    for (int k = 0; k < MAX_HANDS; ++k) {
        root[k] = -1;
        if (k < a.K) {
            const int* in = a.info + 4 * ((int64_t)k * a.B + b);
            const int u = in[0], v = in[1];
            if (u >= 0 && v >= 0) root[k] = v * a.fw + u;
        }
    }
}

__device__ __forceinline__ bool iso_keeps(int label, int root) { return root < 0 || label < 0 || label == root; }

}  // namespace

// a thread per 8 pixels
__global__ __launch_bounds__(ISO_THREADS) void hands_isolate_vec_kernel(IsoArgs a) {
    const int b = blockIdx.y;
    const int64_t f = a.frame[b];
    const bool bad = f < 0 || f >= a.n_frames;                        // outside the store: zero frames, nothing of it is read
    if (blockIdx.x == 0 && threadIdx.x == 0) a.status[b] = bad ? AWR_DET_BAD_FRAME : AWR_DET_OK;
    const int64_t i = (int64_t)blockIdx.x * ISO_THREADS + threadIdx.x;
    if (i >= a.np / 8) return;
    uint4 d = make_uint4(0u, 0u, 0u, 0u);
    int lab[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    int root[MAX_HANDS] = {-1, -1, -1, -1};
    if (!bad) {
        iso_roots(a, b, root);
        d = reinterpret_cast<const uint4*>(a.frames + f * a.np)[i];
        const int4* lp = reinterpret_cast<const int4*>(a.labels + (int64_t)b * a.np) + 2 * i;
        const int4 l0 = lp[0], l1 = lp[1];
        lab[0] = l0.x; lab[1] = l0.y; lab[2] = l0.z; lab[3] = l0.w; lab[4] = l1.x; lab[5] = l1.y; lab[6] = l1.z; lab[7] = l1.w;
    }
    const unsigned w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int k = 0; k < MAX_HANDS; ++k) {
        if (k >= a.K) break;
        unsigned o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[j] = w[j] & ((iso_keeps(lab[2 * j], root[k]) ? 0x0000FFFFu : 0u) | (iso_keeps(lab[2 * j + 1], root[k]) ? 0xFFFF0000u : 0u));
        reinterpret_cast<uint4*>(a.out + ((int64_t)k * a.B + b) * a.np)[i] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// a thread per pixel: any size, any 2-byte aligned base
__global__ __launch_bounds__(ISO_THREADS) void hands_isolate_scalar_kernel(IsoArgs a) {
    const int b = blockIdx.y;
    const int64_t f = a.frame[b];
    const bool bad = f < 0 || f >= a.n_frames;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.status[b] = bad ? AWR_DET_BAD_FRAME : AWR_DET_OK;
    const int64_t p = (int64_t)blockIdx.x * ISO_THREADS + threadIdx.x;
    if (p >= a.np) return;
    uint16_t d = 0;
    int lab = -1;
    int root[MAX_HANDS] = {-1, -1, -1, -1};
    if (!bad) {
        iso_roots(a, b, root);
        d = a.frames[f * a.np + p];
        lab = a.labels[(int64_t)b * a.np + p];
    }
#pragma unroll
    for (int k = 0; k < MAX_HANDS; ++k) {
        if (k >= a.K) break;
        a.out[((int64_t)k * a.B + b) * a.np + p] = iso_keeps(lab, root[k]) ? d : (uint16_t)0;
    }
}

}  // namespace awr

using namespace awr;

extern "C" {

int awr_hands_isolate(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B, int K,
                      const int* labels, const int* info, void* out, int* status, void* stream) {
    if (check_frame_store("awr_hands_isolate", frame_type, B, n_frames, fh, fw) != AWR_OK) return AWR_ERR_ARG;
    AWR_REQUIRE(K >= 1 && K <= MAX_HANDS, "awr_hands_isolate: K = %d hands is outside [1, %d]", K, MAX_HANDS);
    AWR_REQUIRE(frames && frame && labels && info && out && status, "awr_hands_isolate: NULL pointer");
    AWR_REQUIRE(((uintptr_t)frames & 1) == 0 && ((uintptr_t)out & 1) == 0 && ((uintptr_t)labels & 3) == 0,
                "awr_hands_isolate: misaligned frame store / output store / labels");
    IsoArgs a;
    a.frames = (const uint16_t*)frames; a.n_frames = n_frames; a.np = (int64_t)fh * fw; a.fw = fw; a.frame = frame; a.B = B; a.K = K;
    a.labels = labels; a.info = info; a.out = (uint16_t*)out; a.status = status;
    hipStream_t s = as_stream(stream);
    const bool vec = a.np % 8 == 0 && (((uintptr_t)frames | (uintptr_t)out | (uintptr_t)labels) & 15) == 0;
    if (vec) {
        const dim3 grid((unsigned)((a.np / 8 + ISO_THREADS - 1) / ISO_THREADS), B);
        hands_isolate_vec_kernel<<<grid, ISO_THREADS, 0, s>>>(a);
    } else {
        const dim3 grid((unsigned)((a.np + ISO_THREADS - 1) / ISO_THREADS), B);
        hands_isolate_scalar_kernel<<<grid, ISO_THREADS, 0, s>>>(a);
    }
    return check_launch("awr_hands_isolate");
}

}  // extern "C"
