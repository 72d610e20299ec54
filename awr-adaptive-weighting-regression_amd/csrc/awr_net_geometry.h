// Launch geometry of the plan engine (csrc/awr_net.hip): the three GEMM problems of one nn.Conv2d / nn.ConvTranspose2d (k4 s2 p1) with
// their tap and phase tables, the weight packing recipes, and the gradient bucket planner.  Pure host logic: the standard library and the
// plain-C argument blocks of include/awr_hip.h only, so that tests/native/plan_host_main.cpp compiles it without HIP.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/awr_hip.h"

namespace awrnet {

constexpr int N_ALIGN = 128;   // packed weight rows are padded to a multiple of the widest GEMM tile

#ifndef AWR_NET_ROUND_UP
#define AWR_NET_ROUND_UP
static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
#endif

// ------------------------------------------------------------------------------------------
// conv geometry: the three GEMM problems of one nn.Conv2d / nn.ConvTranspose2d (k4 s2 p1)
// ------------------------------------------------------------------------------------------
struct Spec {
    bool deconv = false;
    int cin = 0, cout = 0, k = 1, stride = 1, pad = 0, cin_pad = 0, cout_pad = 0;
    int T() const { return k * k; }
    void out_hw(int h, int w, int& ho, int& wo) const {
        if (!deconv) {
            ho = (h + 2 * pad - k) / stride + 1;
            wo = (w + 2 * pad - k) / stride + 1;
        } else {
            ho = (h - 1) * stride - 2 * pad + k;
            wo = (w - 1) * stride - 2 * pad + k;
        }
    }
};

static Spec make_spec(bool deconv, int cin, int cout, int k, int stride, int pad, int cin_pad = 0, int cout_pad = 0) {
    Spec s;
    s.deconv = deconv;
    s.cin = cin; s.cout = cout; s.k = k; s.stride = stride; s.pad = pad;
    s.cin_pad = cin_pad ? cin_pad : cin;
    s.cout_pad = cout_pad ? cout_pad : cout;
    return s;
}

struct Tap { int dy, dx, wt; };
struct PhaseT { int py, px; std::vector<Tap> taps; };
struct Prob {
    int Hin, Win, Cin, Hout, Wout, N, Hq, Wq, so, si;
    std::vector<PhaseT> phases;
    bool full;
    int k_extent() const {      // terms one output element sums: taps x input channels of the longest phase
        size_t taps = 0;
        for (auto& ph : phases) taps = std::max(taps, ph.taps.size());
        return (int)taps * Cin;
    }
};

static std::vector<PhaseT> gather_taps(const Spec& s) {       // conv-type gather: one phase, taps (ky-p, kx-p, ky*k+kx)
    PhaseT ph{0, 0, {}};
    for (int ky = 0; ky < s.k; ++ky)
        for (int kx = 0; kx < s.k; ++kx) ph.taps.push_back({ky - s.pad, kx - s.pad, ky * s.k + kx});
    return {ph};
}
static std::vector<PhaseT> mirror_taps(const Spec& s) {       // stride-1 data gradient: dx[y] = sum_k dy[y + p - k] w[k]
    PhaseT ph{0, 0, {}};
    for (int ky = 0; ky < s.k; ++ky)
        for (int kx = 0; kx < s.k; ++kx) ph.taps.push_back({s.pad - ky, s.pad - kx, ky * s.k + kx});
    return {ph};
}
static int floordiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
static int pymod(int a, int b) { return a - floordiv(a, b) * b; }
static std::vector<PhaseT> scatter_phases(const Spec& sp) {   // transposed-type (output stride 2): phase (py,px) takes the taps with (py+p-ky) even
    const int s = sp.stride, p = sp.pad, k = sp.k;
    std::vector<PhaseT> out;
    for (int py = 0; py < s; ++py)
        for (int px = 0; px < s; ++px) {
            PhaseT ph{py, px, {}};
            for (int ky = 0; ky < k; ++ky) {
                if (pymod(py + p - ky, s) != 0) continue;
                for (int kx = 0; kx < k; ++kx) {
                    if (pymod(px + p - kx, s) != 0) continue;
                    ph.taps.push_back({floordiv(py + p - ky, s), floordiv(px + p - kx, s), ky * k + kx});
                }
            }
            if (!ph.taps.empty()) out.push_back(ph);
        }
    return out;
}

static Prob fwd_problem(const Spec& s, int hin, int win) {
    int ho, wo;
    s.out_hw(hin, win, ho, wo);
    if (!s.deconv) return Prob{hin, win, s.cin_pad, ho, wo, s.cout_pad, ho, wo, 1, s.stride, gather_taps(s), true};
    auto ph = scatter_phases(s);
    const bool full = ph.size() == 4;
    return Prob{hin, win, s.cin_pad, ho, wo, s.cout_pad, ho / 2, wo / 2, 2, 1, ph, full};
}

// gradient w.r.t. the layer input: reads dY (B,Hout,Wout,cout_pad), writes dX (B,hin,win,cin_pad)
static Prob dgrad_problem(const Spec& s, int hin, int win) {
    int ho, wo;
    s.out_hw(hin, win, ho, wo);
    if (s.deconv) return Prob{ho, wo, s.cout_pad, hin, win, s.cin_pad, hin, win, 1, s.stride, gather_taps(s), true};   // adjoint of a transposed conv is a strided conv
    if (s.stride == 1) return Prob{ho, wo, s.cout_pad, hin, win, s.cin_pad, hin, win, 1, 1, mirror_taps(s), true};
    auto ph = scatter_phases(s);
    const bool full = ph.size() == 4;
    return Prob{ho, wo, s.cout_pad, hin, win, s.cin_pad, hin / 2, win / 2, 2, 1, ph, full};
}

// accum: the launch's accumulation order (0 / 1), resolved by the builder from the plan's modes (Builder::accum)
static void fill_conv_args(awr_conv_args& a, const Prob& p, int B, const float* in, const float* w, const void* w_split, float* out, int T, int accum) {
    memset(&a, 0, sizeof a);
    a.in = in; a.w = w; a.out = out; a.w_split = w_split;
    a.B = B; a.Hin = p.Hin; a.Win = p.Win; a.Cin = p.Cin;
    a.Hq = p.Hq; a.Wq = p.Wq; a.Hout = p.Hout; a.Wout = p.Wout; a.N = p.N;
    a.so = p.so; a.si = p.si; a.T = T;
    a.nphase = (int)p.phases.size();
    a.accum = accum;
    for (int i = 0; i < a.nphase; ++i) {
        a.ph[i].py = p.phases[i].py;
        a.ph[i].px = p.phases[i].px;
        a.ph[i].ntaps = (int)p.phases[i].taps.size();
        for (int t = 0; t < a.ph[i].ntaps; ++t) {
            const Tap& tp = p.phases[i].taps[t];
            a.ph[i].tap[t] = (tp.dy & 0xff) | ((tp.dx & 0xff) << 8) | (tp.wt << 16);
        }
    }
}

// weight packing recipes for awr_pack_weight: (d0, d1, T, transpose, rows, ld)
struct PackRecipe { int d0, d1, T, transpose, rows, ld; };
static PackRecipe fwd_pack(const Spec& s) {
    if (!s.deconv) return {s.cout, s.cin, s.T(), 0, (int)round_up(s.cout_pad, N_ALIGN), s.cin_pad};
    return {s.cin, s.cout, s.T(), 1, (int)round_up(s.cout_pad, N_ALIGN), s.cin_pad};
}
static PackRecipe dgrad_pack(const Spec& s) {
    if (!s.deconv) return {s.cout, s.cin, s.T(), 1, (int)round_up(s.cin_pad, N_ALIGN), s.cout_pad};
    return {s.cin, s.cout, s.T(), 0, (int)round_up(s.cin_pad, N_ALIGN), s.cout_pad};
}

// R[d0][t][d1] in the weight's own (d0,d1) order.  conv: D = dY, G = X; deconv: D = X, G = dY.
struct WProb { bool d_is_dy; int Hd, Wd, Cd, Hg, Wg, Cg, sg, ntaps, d0, d1; int8_t dy[16], dx[16]; };
static WProb wgrad_problem(const Spec& s, int hin, int win) {
    int ho, wo;
    s.out_hw(hin, win, ho, wo);
    WProb w;
    memset(&w, 0, sizeof w);
    w.ntaps = s.T();
    for (int ky = 0; ky < s.k; ++ky)
        for (int kx = 0; kx < s.k; ++kx) {
            w.dy[ky * s.k + kx] = (int8_t)(ky - s.pad);
            w.dx[ky * s.k + kx] = (int8_t)(kx - s.pad);
        }
    w.sg = s.stride;
    if (!s.deconv) {
        w.d_is_dy = true; w.Hd = ho; w.Wd = wo; w.Cd = s.cout_pad; w.Hg = hin; w.Wg = win; w.Cg = s.cin_pad; w.d0 = s.cout; w.d1 = s.cin;
    } else {
        w.d_is_dy = false; w.Hd = hin; w.Wd = win; w.Cd = s.cin_pad; w.Hg = ho; w.Wg = wo; w.Cg = s.cout_pad; w.d0 = s.cin; w.d1 = s.cout;
    }
    return w;
}
static void fill_wgrad_args(awr_wgrad_args& a, const WProb& w, int B, const float* D, const float* G, float* R, int ld) {
    memset(&a, 0, sizeof a);
    a.D = D; a.G = G; a.R = R;
    a.B = B; a.Hd = w.Hd; a.Wd = w.Wd; a.Cd = w.Cd; a.Hg = w.Hg; a.Wg = w.Wg; a.Cg = w.Cg; a.sg = w.sg; a.T = w.ntaps; a.ld = ld;
    memcpy(a.dy, w.dy, 16);
    memcpy(a.dx, w.dx, 16);
}

// ------------------------------------------------------------------------------------------
// gradient buckets
// ------------------------------------------------------------------------------------------
// A gradient write: arena floats [lo, hi) are final once backward op number `ready` has been enqueued.  A bucket has the same shape.
struct Range { int64_t lo, hi; int ready; };

// Group gradient tensors into contiguous arena ranges that become final in backward order: the ranges tile [0, n_active) from
// the arena END downwards (the backward pass finishes the last layers first), ready_op non-decreasing, so bucket k can be
// all-reduced while the backward of the earlier layers still runs.
static std::vector<Range> plan_buckets(std::vector<Range> ws, int64_t n_active, int n_buckets) {
    std::vector<Range> out;
    if (ws.empty()) return out;
    std::stable_sort(ws.begin(), ws.end(), [](const Range& a, const Range& b) { return a.lo > b.lo; });
    int64_t total = 0;
    for (auto& w : ws) total += w.hi - w.lo;
    // The LAST bucket (the arena's first layers: final only when the backward ends) has nothing left to hide its exchange behind, so it is
    // kept small -- the leading tensors up to 1 % of the parameters (ResNet18: the stem and layer1, 0.6 MB of 61.5 MB) -- and the others
    // share the rest equally.  (Equal quarters left 15 MB = a quarter of the all-reduce exposed after the last data-gradient GEMM.)
    int64_t tail = 0;
    if (n_buckets > 2)
        for (size_t i = ws.size(); i-- > 0;) {
            if (tail + (ws[i].hi - ws[i].lo) > total / 100) break;
            tail += ws[i].hi - ws[i].lo;
        }
    const double target = (double)(total - tail) / (double)(n_buckets > 1 ? n_buckets - (tail > 0 ? 1 : 0) : 1);
    int64_t acc = 0, hi_edge = n_active, left = total;
    int ready = -1;
    for (size_t i = 0; i < ws.size(); ++i) {
        acc += ws[i].hi - ws[i].lo;
        left -= ws[i].hi - ws[i].lo;
        if (ws[i].ready > ready) ready = ws[i].ready;
        const bool last = i + 1 == ws.size();
        const bool cut_tail = tail > 0 && left == tail;      // everything below is the small last bucket
        if (last || cut_tail || ((double)acc >= target && (int)out.size() < n_buckets - 1 - (tail > 0 ? 1 : 0))) {
            const int64_t edge = last ? 0 : ws[i].lo;
            out.push_back({edge, hi_edge, ready});
            hi_edge = edge;
            acc = 0;
        }
    }
    for (size_t k = 1; k < out.size(); ++k)      // a later bucket is never launched before an earlier one
        if (out[k].ready < out[k - 1].ready) out[k].ready = out[k - 1].ready;
    return out;
}

}  // namespace awrnet
