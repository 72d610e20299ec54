// Several hands per frame: the near foreground of a depth frame split into its 4-connected components, the K nearest
// large ones seeded with a centre of mass each -- a restatement of awr_amd/detect.py components and hand_seeds, bit for bit.
//
// Everything up to the last three divisions per slot is INTEGER arithmetic.  A component's label is the smallest raster index v * fw + u
// of its pixels, which is canonical: any correct labelling, in any order, gives these integers.  The labelling is a union-find forest
// over the pixels of the frame, one int32 pointer per pixel, joined by smaller index: to join a and b, find both roots, order them
// a > b, old = atomicMin(&L[a], b); old == a means a was still a root and now hangs under b, otherwise go on from old.  Every pointer
// only ever DECREASES, so every find and every retry ends, and the root that survives is the component's minimum whatever the order in
// which the joins arrive.  Counts and minimum depths per component, the candidates' count and the slab sums are integer atomics and
// integer reductions; the K nearest are K minima of (zc << 32 | root), unique words.  There is no floating-point atomic and no
// floating-point reduction in this file, no kernel waits for another workgroup, and only the stream orders the stages.
//
// Shape, as awr_palm.hip's: a frame is split over several workgroups, a stage is a launch, and the stages meet in the frame's slots
// (64-bit words at the head of the caller's scratch) and in three int32 words per pixel behind them -- L the forest, CNT and ZC the
// pixels and the smallest raw depth of the component whose root the word belongs to.
//   1. hands_init_kernel: the slots.  hands_dmin_kernel: dmin of the foreground, a block minimum and one atomicMin per workgroup;
//   2. hands_tile_kernel: a 64 x 16 tile per workgroup: the mask (foreground with d <= min(dmin + reach, zmax)), a union-find over the
//      tile in LDS (left and upper neighbour), L = the global raster index of the local root, CNT = 0, ZC = INT_MAX;
//   3. hands_border_kernel: joins across the tiles' upper and left borders in global memory;
//      (stages 2 and 3 are the only ones that decide joins.  Each has a compile-time EDGE form for awr_detect_hands_edge, DESIGN.md
//      4.29: a join also needs |d_a - d_b| <= elim, an integer test equal to the statement's float64 comparison against `edge`, since
//      elim = depth_floor(edge).  The forms without it are what awr_detect_hands runs, and hold nothing of the test.
//      awr_detect_hands_link, DESIGN.md 4.33, adds ONE launch here, hands_link_kernel: joins of a rear pixel with the first pixel behind
//      at most `gap` occluders in a row or column, so the fragments a front hand cuts a rear hand into are one component again.)
//   4. hands_flatten_kernel: L = find(L) (and labels_out); CNT and ZC of the root by atomicAdd / atomicMin, the lanes of a wave that
//      share a root summed first;
//   5. hands_roots_kernel: every workgroup's K smallest keys among its roots with CNT >= min_pixels (a sorted list per thread, then K
//      block minima) and the candidates' count; hands_pick_kernel: one workgroup per frame merges them -- at most 64 x 4 words, no pass
//      over the frame (ONE workgroup per frame over the whole frame is what awr_palm.hip's header measured at 12 GB/s);
//   6. hands_sums_kernel: n, su, sv, sd of the chosen components' pixels with d <= min(zc + slab, zmax), a block sum and one 64-bit
//      atomicAdd per workgroup, slot and word;
//   7. hands_finalize_kernel: a thread per frame and slot writes centre, status, info and count, hand-major (row k * B + b).
// The depth tests are the statement's float64 comparisons: for an integer d, d <= x  <=>  d <= floor(x) (awr_frame.h's depth_bounds and
// depth_floor; compiled with -ffp-contract=off; the sums base + span are single double additions).  The block reductions and the split of
// a frame over workgroups are awr_frame.h's too.
#include <limits.h>
#include <math.h>

#include "awr_frame.h"

namespace awr {
namespace {

constexpr int HANDS_THREADS = 256;
constexpr int HANDS_WAVES = HANDS_THREADS / 64;
constexpr int HANDS_TILE_W = 64, HANDS_TILE_H = 16;   // a wave per tile row, four rows per thread
constexpr int HANDS_MAX_PARTS = 64;                   // workgroups per frame of the streaming stages

// a frame's slots: 64-bit words
enum { HS_DMIN = 0, HS_COUNT = 1, HS_KEY = 2, HS_SUM = HS_KEY + MAX_HANDS, HS_PART = HS_SUM + 4 * MAX_HANDS };
constexpr int HANDS_SLOTS = HS_PART + HANDS_MAX_PARTS * MAX_HANDS;
constexpr u64 HANDS_NONE = ~0ull;

struct HandsArgs {
    const uint16_t* frames; int64_t n_frames; int fh, fw;
    const int64_t* frame; int B, K;
    int dlo, dhi;                 // zmin <= d <= zmax and d != 0  <=>  dlo <= d <= dhi
    double zmax, reach, slab; int min_pixels;
    int elim;                     // EDGE kernels only: two neighbouring mask pixels join when |d_a - d_b| <= elim (depth_floor of the edge)
    u64* slots; int* L; int* CNT; int* ZC;
    int* labels_out;
    int llim, gap;                // hands_link_kernel only: a walk of at most `gap` occluders links p and q when |d_p - d_q| <= llim
};

struct HandsFrame {
    const uint16_t* F; u64* S; int* L; int* CNT; int* ZC;
    bool bad;                     // the frame index is outside the store: nothing of it is read
};

__device__ __forceinline__ HandsFrame hands_frame(const HandsArgs& a, int b) {
    HandsFrame hf;
    const int64_t f = a.frame[b], np = (int64_t)a.fh * a.fw;
    hf.bad = f < 0 || f >= a.n_frames;
    hf.F = a.frames + (hf.bad ? 0 : f) * np;
    hf.S = a.slots + (int64_t)b * HANDS_SLOTS;
    hf.L = a.L + b * np; hf.CNT = a.CNT + b * np; hf.ZC = a.ZC + b * np;
    return hf;
}

// the largest integer d in [-1, 65535] with (double)d <= min(base + span, zmax)
__device__ __forceinline__ int hands_limit(int base, double span, double zmax) {
    return depth_floor(fmin((double)base + span, zmax));
}

// pixels [p0, p1) of workgroup blockIdx.x of gridDim.x: whole rows
__device__ __forceinline__ void hands_share(const HandsArgs& a, int& p0, int& p1) {
    const int per = (a.fh + (int)gridDim.x - 1) / (int)gridDim.x;
    const int r0 = min((int)blockIdx.x * per, a.fh), r1 = min(r0 + per, a.fh);
    p0 = r0 * a.fw; p1 = r1 * a.fw;
}

// ---- the forest -------------------------------------------------------------------------------------------------------------------
// (other lanes and workgroups lower these words while they are read: every load is an atomic one, never a cached copy)
__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x at the time of the walk; the path walked is then pointed at it (a root is never above its descendants' indices, so
// atomicMin keeps every pointer decreasing and inside the component)
__device__ __forceinline__ int uf_find(int* L, int x) {
    int r = x, n;
    while ((n = uf_load(L + r)) != r) r = n;
    while (x > r) {
        n = uf_load(L + x);
        if (n > r) atomicMin(L + x, r);
        x = n;
    }
    return r;
}

__device__ __forceinline__ void uf_union(int* L, int a, int b) {
    a = uf_find(L, a); b = uf_find(L, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b);
        if (old == a) break;            // a was a root and hangs under b now
        a = old;                        // a had a parent already: that parent and b are what remains to be joined
    }
}

// the K smallest of the words offered to it, ascending; HANDS_NONE where there are fewer
struct SmallestK {
    u64 k[MAX_HANDS];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < MAX_HANDS; ++i) k[i] = HANDS_NONE;
    }
    __device__ __forceinline__ void offer(u64 v) {
#pragma unroll
        for (int i = 0; i < MAX_HANDS; ++i)
            if (v < k[i]) { const u64 t = k[i]; k[i] = v; v = t; }
    }
    __device__ __forceinline__ void pop() {
#pragma unroll
        for (int i = 0; i + 1 < MAX_HANDS; ++i) k[i] = k[i + 1];
        k[MAX_HANDS - 1] = HANDS_NONE;
    }
};

}  // namespace

__global__ __launch_bounds__(HANDS_THREADS) void hands_init_kernel(u64* __restrict__ slots, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * HANDS_THREADS + threadIdx.x;
    if (i >= n) return;
    const int w = (int)(i % HANDS_SLOTS);
    slots[i] = (w == HS_DMIN || (w >= HS_KEY && w < HS_SUM) || w >= HS_PART) ? HANDS_NONE : 0ull;
}

// 1. dmin: the smallest foreground depth of the frame
__global__ __launch_bounds__(HANDS_THREADS) void hands_dmin_kernel(HandsArgs a) {
    __shared__ u64 red[HANDS_WAVES];
    const HandsFrame hf = hands_frame(a, blockIdx.y);
    if (hf.bad) return;
    int p0, p1;
    hands_share(a, p0, p1);
    const unsigned dlo = (unsigned)a.dlo;
    const int dhi = a.dhi;
    u64 best = HANDS_NONE;
    for (int p = p0 + (int)threadIdx.x; p < p1; p += HANDS_THREADS) {
        const unsigned d = hf.F[p];
        if (d >= dlo && (int)d <= dhi && (u64)d < best) best = d;
    }
    best = block_reduce<HANDS_WAVES>(best, red, MinU64());
    if (threadIdx.x == 0 && best != HANDS_NONE) atomicMin(hf.S + HS_DMIN, best);
}

// 2. a tile: the mask, the tile's own forest in LDS, L = the global raster index of the local root (-1 on background); CNT and ZC of
// every pixel start at "none".  EDGE: the tile's raw depths are staged once next to `lab` (2 KB), and a pixel joins its left or upper
// neighbour only when their depths differ by at most elim; without it nothing of this is compiled in
template <bool EDGE>
__global__ __launch_bounds__(HANDS_THREADS) void hands_tile_kernel(HandsArgs a) {
    __shared__ int lab[HANDS_TILE_W * HANDS_TILE_H];
    __shared__ uint16_t dep[EDGE ? HANDS_TILE_W * HANDS_TILE_H : 1];
    const HandsFrame hf = hands_frame(a, blockIdx.y);
    const int fw = a.fw, fh = a.fh;
    const int tiles_x = (fw + HANDS_TILE_W - 1) / HANDS_TILE_W;
    const int tu = ((int)blockIdx.x % tiles_x) * HANDS_TILE_W, tv = ((int)blockIdx.x / tiles_x) * HANDS_TILE_H;
    const int col = threadIdx.x & 63, row0 = threadIdx.x >> 6;
    const int u = tu + col;
    const u64 dmin = hf.S[HS_DMIN];
    const int dlo = a.dlo;
    const int dhi = (hf.bad || dmin == HANDS_NONE) ? -1 : min(a.dhi, hands_limit((int)dmin, a.reach, a.zmax));
    bool m[4];
    int dq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = row0 + HANDS_WAVES * q, v = tv + row, i = row * HANDS_TILE_W + col;
        const bool inside = u < fw && v < fh;
        m[q] = false;
        dq[q] = 0;
        if (inside && dhi >= dlo) {
            const int d = hf.F[v * fw + u];
            m[q] = d >= dlo && d <= dhi;
            dq[q] = d;
        }
        lab[i] = m[q] ? i : -1;
        if constexpr (EDGE) dep[i] = (uint16_t)dq[q];
        if (inside) { hf.CNT[v * fw + u] = 0; hf.ZC[v * fw + u] = INT_MAX; }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = row0 + HANDS_WAVES * q, i = row * HANDS_TILE_W + col;
        if (!m[q]) continue;
        const auto near = [&](int n) {                                  // the depth test between this pixel and its mask neighbour n
            if constexpr (EDGE) return abs(dq[q] - (int)dep[n]) <= a.elim;
            return true;
        };
        if (col > 0 && uf_load(lab + i - 1) >= 0 && near(i - 1)) uf_union(lab, i, i - 1);
        if (row > 0 && uf_load(lab + i - HANDS_TILE_W) >= 0 && near(i - HANDS_TILE_W)) uf_union(lab, i, i - HANDS_TILE_W);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = row0 + HANDS_WAVES * q, v = tv + row, i = row * HANDS_TILE_W + col;
        if (!(u < fw && v < fh)) continue;
        int label = -1;
        if (m[q]) {
            int r = i, n;
            while ((n = lab[r]) != r) r = n;            // (nothing writes lab any more)
            label = (tv + r / HANDS_TILE_W) * fw + tu + r % HANDS_TILE_W;
        }
        hf.L[v * fw + u] = label;
    }
}

// 3. joins across the tiles' borders: threads 0 ... 63 the tile's first row with the row above it, 64 ... 79 its first column with the
// column left of it.  EDGE: the two raw depths are read from the frame and pass the tile kernel's test
template <bool EDGE>
__global__ __launch_bounds__(128) void hands_border_kernel(HandsArgs a) {
    const HandsFrame hf = hands_frame(a, blockIdx.y);
    const int fw = a.fw, fh = a.fh;
    const int tiles_x = (fw + HANDS_TILE_W - 1) / HANDS_TILE_W;
    const int tu = ((int)blockIdx.x % tiles_x) * HANDS_TILE_W, tv = ((int)blockIdx.x / tiles_x) * HANDS_TILE_H;
    const int t = threadIdx.x;
    int p = -1, q = -1;
    if (t < HANDS_TILE_W) {
        if (tv > 0 && tu + t < fw) { p = tv * fw + tu + t; q = p - fw; }
    } else if (t < HANDS_TILE_W + HANDS_TILE_H) {
        const int v = tv + t - HANDS_TILE_W;
        if (tu > 0 && v < fh) { p = v * fw + tu; q = p - 1; }
    }
    if (p >= 0 && uf_load(hf.L + p) >= 0 && uf_load(hf.L + q) >= 0) {
        if constexpr (EDGE) {
            if (abs((int)hf.F[p] - (int)hf.F[q]) > a.elim) return;      // (labelled pixels: the frame is inside the store)
        }
        uf_union(hf.L, p, q);
    }
}

// 3b. links across an occluder (awr_detect_hands_link), a thread per pixel: a labelled pixel p looks at its four
// neighbours, and where one is an OCCLUDER of p (d != 0 and d_p - d > elim: raw depths, in the mask or not) it walks on in that direction
// over at most `gap` occluders to the first pixel q that is none.  q in the mask with |d_q - d_p| <= llim: p and q are joined in the
// forest, as any other pair.  The walk links nothing where it leaves the frame or where q_1 ... q_{gap + 1} are all occluders; a zero
// pixel is no occluder and ends it.  Only a pixel at the rear side of an occlusion edge walks, gap + 1 two-byte loads of the frame at
// the most.  Integer compares only; every index is inside the row (u) or the column (v) of the frame before it is read
__global__ __launch_bounds__(HANDS_THREADS) void hands_link_kernel(HandsArgs a) {
    const HandsFrame hf = hands_frame(a, blockIdx.y);
    if (hf.bad) return;
    int p0, p1;
    hands_share(a, p0, p1);
    const int fw = a.fw, fh = a.fh, elim = a.elim, llim = a.llim, gap = a.gap;
    for (int p = p0 + (int)threadIdx.x; p < p1; p += HANDS_THREADS) {
        if (uf_load(hf.L + p) < 0) continue;
        const int dp = hf.F[p], u = p % fw, v = p / fw;
#pragma unroll
        for (int dir = 0; dir < 4; ++dir) {                              // right, left, down, up
            const int step = dir == 0 ? 1 : dir == 1 ? -1 : dir == 2 ? fw : -fw;
            const int room = dir == 0 ? fw - 1 - u : dir == 1 ? u : dir == 2 ? fh - 1 - v : v;      // pixels ahead of p inside the frame
            if (room < 2) continue;                                      // (an occluder and a pixel behind it)
            int d = hf.F[p + step];
            if (d == 0 || dp - d <= elim) continue;                      // q_1 is no occluder: p does not walk
            const int last = min(gap + 1, room);
            int t = 2, q = -1;
            for (; t <= last; ++t) {
                d = hf.F[p + t * step];
                if (d == 0 || dp - d <= elim) { q = p + t * step; break; }
            }
            if (q >= 0 && uf_load(hf.L + q) >= 0 && abs(d - dp) <= llim) uf_union(hf.L, p, q);
        }
    }
}

// 4. L = find(L); pixels and smallest depth of every component at its root's words
__global__ __launch_bounds__(HANDS_THREADS) void hands_flatten_kernel(HandsArgs a) {
    const HandsFrame hf = hands_frame(a, blockIdx.y);
    int p0, p1;
    hands_share(a, p0, p1);
    int* out = a.labels_out ? a.labels_out + (int64_t)blockIdx.y * a.fh * a.fw : nullptr;
    const int lane = threadIdx.x & 63;
    for (int base = p0; base < p1; base += HANDS_THREADS) {            // (uniform over the workgroup: the shuffles below see whole waves)
        const int p = base + (int)threadIdx.x;
        int r = -1, d = INT_MAX;
        if (p < p1) {
            if (uf_load(hf.L + p) >= 0) {
                r = uf_find(hf.L, p);
                __hip_atomic_store(hf.L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                d = hf.F[p];
            }
            if (out) out[p] = r;
        }
        u64 left = __ballot(r >= 0);
        while (left) {
            const int leader = __ffsll((i64)left) - 1;
            const int lr = __shfl(r, leader, 64);
            const bool mine = r == lr;
            const u64 same = __ballot(mine);
            int dm = mine ? d : INT_MAX;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) dm = min(dm, __shfl_xor(dm, o, 64));
            if (lane == leader) {
                atomicAdd(hf.CNT + lr, __popcll(same));
                atomicMin(hf.ZC + lr, dm);
            }
            left &= ~same;
        }
    }
}

// 5a. per workgroup: its K smallest (zc << 32 | root) among the roots with CNT >= min_pixels, and how many such roots it holds
__global__ __launch_bounds__(HANDS_THREADS) void hands_roots_kernel(HandsArgs a) {
    __shared__ u64 red[HANDS_WAVES];
    const HandsFrame hf = hands_frame(a, blockIdx.y);
    int p0, p1;
    hands_share(a, p0, p1);
    SmallestK mine;
    mine.clear();
    u64 n = 0;
    for (int p = p0 + (int)threadIdx.x; p < p1; p += HANDS_THREADS) {
        if (hf.L[p] == p && hf.CNT[p] >= a.min_pixels) {
            n += 1;
            mine.offer(((u64)(unsigned)hf.ZC[p] << 32) | (u64)(unsigned)p);
        }
    }
    n = block_reduce<HANDS_WAVES>(n, red, SumU64());
    if (n == 0) return;                                                  // (uniform; the workgroup's words stay "none")
    if (threadIdx.x == 0) atomicAdd(hf.S + HS_COUNT, n);
    for (int i = 0; i < a.K; ++i) {
        const u64 best = block_reduce<HANDS_WAVES>(mine.k[0], red, MinU64());
        if (best == HANDS_NONE) break;
        if (mine.k[0] == best) mine.pop();                               // (the words are unique: one thread holds it)
        if (threadIdx.x == 0) hf.S[HS_PART + (int)blockIdx.x * MAX_HANDS + i] = best;
    }
}

// 5b. per frame: the K smallest of the workgroups' words, ascending
__global__ __launch_bounds__(HANDS_THREADS) void hands_pick_kernel(HandsArgs a) {
    __shared__ u64 red[HANDS_WAVES];
    static_assert(HANDS_MAX_PARTS * MAX_HANDS == HANDS_THREADS, "a word per thread");
    u64* S = a.slots + (int64_t)blockIdx.x * HANDS_SLOTS;
    u64 mine = S[HS_PART + threadIdx.x];
    for (int i = 0; i < a.K; ++i) {
        const u64 best = block_reduce<HANDS_WAVES>(mine, red, MinU64());
        if (best == HANDS_NONE) break;
        if (mine == best) mine = HANDS_NONE;
        if (threadIdx.x == 0) S[HS_KEY + i] = best;
    }
}

// 6. the slab sums of the chosen components
__global__ __launch_bounds__(HANDS_THREADS) void hands_sums_kernel(HandsArgs a) {
    __shared__ u64 red[HANDS_WAVES];
    const HandsFrame hf = hands_frame(a, blockIdx.y);
    if (hf.S[HS_KEY] == HANDS_NONE) return;                             // no candidate at all
    int p0, p1;
    hands_share(a, p0, p1);
    int root[MAX_HANDS], lim[MAX_HANDS];
    u64 acc[MAX_HANDS][4];
#pragma unroll
    for (int k = 0; k < MAX_HANDS; ++k) {
        const u64 key = k < a.K ? hf.S[HS_KEY + k] : HANDS_NONE;
        root[k] = key == HANDS_NONE ? -2 : (int)(key & 0xFFFFFFFFull);
        lim[k] = key == HANDS_NONE ? -1 : min(a.dhi, hands_limit((int)(key >> 32), a.slab, a.zmax));
        acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0;
    }
    const int fw = a.fw;
    for (int p = p0 + (int)threadIdx.x; p < p1; p += HANDS_THREADS) {
        const int l = hf.L[p];
        if (l < 0) continue;
        const int d = hf.F[p];
#pragma unroll
        for (int k = 0; k < MAX_HANDS; ++k)
            if (l == root[k] && d <= lim[k]) {
                acc[k][0] += 1; acc[k][1] += (u64)(p % fw); acc[k][2] += (u64)(p / fw); acc[k][3] += (u64)d;
            }
    }
#pragma unroll
    for (int k = 0; k < MAX_HANDS; ++k) {
        if (root[k] < 0) continue;                                       // (uniform)
        u64 s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = block_reduce<HANDS_WAVES>(acc[k][j], red, SumU64());
        if (threadIdx.x == 0 && s[0]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) atomicAdd(hf.S + HS_SUM + 4 * k + j, s[j]);
        }
    }
}

// 7. a thread per frame and slot: centre, status, info and count, hand-major
__global__ void hands_finalize_kernel(HandsArgs a, double* __restrict__ centers, int* __restrict__ status, int* __restrict__ info,
                                      int* __restrict__ count) {
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= a.K) return;
    const HandsFrame hf = hands_frame(a, b);
    const double nan = __builtin_nan("");
    double c[3] = {nan, nan, nan};
    int st = hf.bad ? AWR_DET_BAD_FRAME : AWR_DET_EMPTY, in[4] = {-1, -1, 0, 0};
    const u64 key = hf.bad ? HANDS_NONE : hf.S[HS_KEY + k];
    if (key != HANDS_NONE) {
        const int root = (int)(key & 0xFFFFFFFFull);
        const u64* s = hf.S + HS_SUM + 4 * k;
        const double dn = (double)s[0];                                  // (the component's nearest pixel is in its slab: n >= 1)
        c[0] = (double)s[1] / dn; c[1] = (double)s[2] / dn; c[2] = (double)s[3] / dn;
        st = AWR_DET_OK;
        in[0] = root % a.fw; in[1] = root / a.fw; in[2] = hf.CNT[root]; in[3] = (int)(key >> 32);
    }
    const int64_t r = (int64_t)k * a.B + b;
    centers[3 * r] = c[0]; centers[3 * r + 1] = c[1]; centers[3 * r + 2] = c[2];
    status[r] = st;
    info[4 * r] = in[0]; info[4 * r + 1] = in[1]; info[4 * r + 2] = in[2]; info[4 * r + 3] = in[3];
    if (k == 0) count[b] = hf.bad ? 0 : (int)hf.S[HS_COUNT];
}

}  // namespace awr

using namespace awr;

// the three entry points: `edge` NULL is awr_detect_hands -- the kernels without a depth test, the launches it always issued; `link` NULL
// is awr_detect_hands_edge -- its launches; with a link the link stage runs between the borders and the flattening
static int detect_hands(const char* who, const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B,
                        int K, double zmin, double zmax, double reach, const double* edge, const double* link, int gap, double slab,
                        int min_pixels, void* scratch, int* labels_out, double* centers, int* status, int* info, int* count, void* stream) {
    if (check_frame_store(who, frame_type, B, n_frames, fh, fw) != AWR_OK) return AWR_ERR_ARG;
    AWR_REQUIRE(K >= 1 && K <= MAX_HANDS, "%s: K = %d hands is outside [1, %d]", who, K, MAX_HANDS);
    AWR_REQUIRE(min_pixels >= 1, "%s: min_pixels = %d must be at least 1", who, min_pixels);
    AWR_REQUIRE(zmin <= zmax, "%s: depth range needs zmin <= zmax (got %g, %g)", who, zmin, zmax);
    AWR_REQUIRE(reach >= 0.0, "%s: reach = %g must be >= 0", who, reach);
    AWR_REQUIRE(!edge || *edge >= 0.0, "%s: edge = %g must be >= 0 (infinity: no depth test)", who, edge ? *edge : 0.0);
    AWR_REQUIRE(!link || *link >= 0.0, "%s: link = %g must be >= 0 (infinity: any two depths agree)", who, link ? *link : 0.0);
    AWR_REQUIRE(!link || (gap >= 1 && gap <= AWR_HANDS_MAX_GAP), "%s: gap = %d is outside [1, %d]", who, gap, AWR_HANDS_MAX_GAP);
    AWR_REQUIRE(slab >= 0.0, "%s: slab = %g must be >= 0", who, slab);
    AWR_REQUIRE(frames && frame && scratch && centers && status && info && count, "%s: NULL pointer", who);
    AWR_REQUIRE(((uintptr_t)frames & 1) == 0 && ((uintptr_t)scratch & 7) == 0, "%s: misaligned frame store / scratch", who);
    hipStream_t s = as_stream(stream);
    const int64_t np = (int64_t)B * fh * fw;
    HandsArgs a;
    a.frames = (const uint16_t*)frames; a.n_frames = n_frames; a.fh = fh; a.fw = fw; a.frame = frame; a.B = B; a.K = K;
    depth_bounds(zmin, zmax, a.dlo, a.dhi);
    a.zmax = zmax; a.reach = reach; a.slab = slab; a.min_pixels = min_pixels;
    a.elim = edge ? depth_floor(*edge) : 65535;      // (for integer depths |d_a - d_b| <= edge  <=>  |d_a - d_b| <= floor(edge))
    a.slots = (u64*)scratch;
    a.L = (int*)(a.slots + (int64_t)B * HANDS_SLOTS); a.CNT = a.L + np; a.ZC = a.CNT + np;
    a.labels_out = labels_out;
    a.llim = link ? depth_floor(*link) : 0; a.gap = link ? gap : 0;
    const int64_t nw = (int64_t)B * HANDS_SLOTS;
    const int tiles = ((fw + HANDS_TILE_W - 1) / HANDS_TILE_W) * ((fh + HANDS_TILE_H - 1) / HANDS_TILE_H);
    const dim3 share(frame_parts(B, fh, HANDS_MAX_PARTS), B), tile(tiles, B);
    hands_init_kernel<<<(unsigned)((nw + HANDS_THREADS - 1) / HANDS_THREADS), HANDS_THREADS, 0, s>>>(a.slots, nw);
    hands_dmin_kernel<<<share, HANDS_THREADS, 0, s>>>(a);
    if (edge) {
        hands_tile_kernel<true><<<tile, HANDS_THREADS, 0, s>>>(a);
        hands_border_kernel<true><<<tile, 128, 0, s>>>(a);
        if (link) hands_link_kernel<<<share, HANDS_THREADS, 0, s>>>(a);
    } else {
        hands_tile_kernel<false><<<tile, HANDS_THREADS, 0, s>>>(a);
        hands_border_kernel<false><<<tile, 128, 0, s>>>(a);
    }
    hands_flatten_kernel<<<share, HANDS_THREADS, 0, s>>>(a);
    hands_roots_kernel<<<share, HANDS_THREADS, 0, s>>>(a);
    hands_pick_kernel<<<B, HANDS_THREADS, 0, s>>>(a);
    hands_sums_kernel<<<share, HANDS_THREADS, 0, s>>>(a);
    hands_finalize_kernel<<<B, MAX_HANDS, 0, s>>>(a, centers, status, info, count);
    return check_launch(who);
}

extern "C" {

int64_t awr_detect_hands_scratch(int B, int fh, int fw) {
    if (B <= 0 || B > AWR_DET_MAX_BATCH || !frame_sides_ok(fh, fw)) {
        set_error("awr_detect_hands_scratch: B = %d is outside [1, %d] or the frame of %d x %d is outside [1, %d]^2", B, AWR_DET_MAX_BATCH, fh,
                  fw, FRAME_MAX_SIDE);
        return -1;
    }
    const int64_t words = 3 * (int64_t)B * fh * fw;                       // (a whole number of 64-bit words: callers allocate those)
    return (int64_t)B * HANDS_SLOTS * (int64_t)sizeof(u64) + (words + (words & 1)) * (int64_t)sizeof(int);
}

int awr_detect_hands(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B, int K, double zmin,
                     double zmax, double reach, double slab, int min_pixels, void* scratch, int* labels_out, double* centers, int* status,
                     int* info, int* count, void* stream) {
    return detect_hands("awr_detect_hands", frames, frame_type, n_frames, fh, fw, frame, B, K, zmin, zmax, reach, nullptr, nullptr, 0, slab,
                        min_pixels, scratch, labels_out, centers, status, info, count, stream);
}

int awr_detect_hands_edge(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B, int K,
                          double zmin, double zmax, double reach, double edge, double slab, int min_pixels, void* scratch, int* labels_out,
                          double* centers, int* status, int* info, int* count, void* stream) {
    return detect_hands("awr_detect_hands_edge", frames, frame_type, n_frames, fh, fw, frame, B, K, zmin, zmax, reach, &edge, nullptr, 0,
                        slab, min_pixels, scratch, labels_out, centers, status, info, count, stream);
}

int awr_detect_hands_link(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B, int K,
                          double zmin, double zmax, double reach, double edge, double link, int gap, double slab, int min_pixels,
                          void* scratch, int* labels_out, double* centers, int* status, int* info, int* count, void* stream) {
    return detect_hands("awr_detect_hands_link", frames, frame_type, n_frames, fh, fw, frame, B, K, zmin, zmax, reach, &edge, &link, gap,
                        slab, min_pixels, scratch, labels_out, centers, status, info, count, stream);
}

}  // extern "C"
