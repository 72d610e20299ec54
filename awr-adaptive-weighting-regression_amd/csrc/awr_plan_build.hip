// Network-level engine of libawr_hip.so (include/awr_hip.h, "Network-level API"), building a plan: the AWR backbones as static execution plans.
//
//   awr_plan  one (batch, image size, mode) instance: every activation / gradient buffer allocated once, two flat lists of
//             pre-bound kernel launches (forward, backward).  The backward list is derived at build time by a small static
//             autograd: every forward node registers an emitter for its own gradient kernels; `gtarget` decides
//             write-vs-accumulate per tensor; identity skips alias the upstream gradient buffer.
//
// Builder emits every launch, NetBuilder walks the two backbones, awr_plan_create[_modes] is the entry point (types: csrc/awr_plan.h; replay:
// csrc/awr_plan_run.hip).  Host code only (no kernels): it binds the operator-level entry points of this library (awr_conv_gemm, awr_bn_*, ...).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "awr_plan.h"

using namespace awrnet;

namespace awrnet {

constexpr float BN_EPS = 1e-5f;
constexpr float BN_MOMENTUM = 0.1f;

static int alloc_packed(awr_net* net, Packed& pk, const PackRecipe& r) {
    if (pk.p) return AWR_OK;
    pk.rows = r.rows; pk.T = r.T; pk.ld = r.ld;
    void* p;
    NET_CHECK(dev_alloc(net->owned, (size_t)pk.numel() * 4, true, &p));
    pk.p = (float*)p;
    NET_CHECK(dev_alloc(net->owned, (size_t)pk.numel() * 6, true, &p));      // split image: 3 bf16 pieces per element
    pk.split = p;
    return AWR_OK;
}

struct ConvOpt {
    const float *in_scale = nullptr, *in_shift = nullptr;
    bool relu_in = false;
    const float *out_scale = nullptr, *out_shift = nullptr;
    Tn* res = nullptr;
    bool relu_out = false, want_stats = false, use_bias = true;
};

// K steps (32-channel slices x taps) of a launch's shortest phase: what bounds its split-K depth
int min_k_steps(const awr_conv_args& a) {
    int minsteps = 1 << 30;
    for (int p = 0; p < a.nphase; ++p) minsteps = std::min(minsteps, a.ph[p].ntaps * (a.Cin / 32));
    return minsteps;
}

// The split-K scratch rule: the largest number of raw output copies (a power of two, at most `cap`) a launch of `wgs` 64x64-tile workgroups
// per phase and `nphase` phases gets scratch for -- workgroups x copies below 2048, at least 4 K slices per range at the deepest split and,
// with a byte cap (max_bytes > 0), that many copies of `numel` floats within it.  1 = no scratch.
static int split_k_copies(int64_t wgs, int nphase, int minsteps, int cap, int64_t numel, int64_t max_bytes) {
    int smax = 1;
    while (smax < cap && wgs * nphase * smax < 2048 && minsteps / (smax * 2) >= 4 && (max_bytes <= 0 || numel * 4 * (smax * 2) <= max_bytes)) smax *= 2;
    return smax;
}

struct GradWrite { int64_t lo, hi; int ready; int job; };      // arena range a backward op finishes; job: its entry in the scatter table, or -1

// Builds one plan.  Its members are what the build alone needs: they die with the builder (the backward emitters capture `this`), the plan
// keeps only what a replay, the tuner or an awr_plan_* entry point reads.
struct Builder {
    awr_plan& P;
    awr_net& N;
    int err = AWR_OK;
    std::vector<std::function<int()>> nodes;       // backward emitters, in forward order
    std::map<Tn*, std::vector<awr_conv_args*>> grad_writers;
    std::map<Tn*, int> fork_results;
    int fork_sid = 0;
    std::vector<GradWrite> grad_writes;
    std::vector<awr_unpack_job> unpack_jobs;
    int64_t scratch_used = 0;                      // floats taken from the plan's weight-gradient scratch arena
    explicit Builder(awr_plan& p) : P(p), N(*p.net) {}

    template <typename Tp>
    Tp* alloc(int64_t count, bool zero = false) {
        void* p = nullptr;
        const size_t bytes = (size_t)count * sizeof(Tp);
        if (int e = dev_alloc(P.owned, bytes, zero, &p)) {
            err = e;
            return nullptr;
        }
        P.bytes += (int64_t)bytes;
        if (zero) P.zero_init.push_back({p, bytes});
        return (Tp*)p;
    }
    Tn* new_t(int B, int H, int W, int C, bool needs_grad = true, const std::string& name = "") {
        P.tensors.emplace_back();
        Tn* t = &P.tensors.back();
        t->buf = alloc<float>((int64_t)B * H * W * C);
        t->B = B; t->H = H; t->W = W; t->C = C;
        t->needs_grad = needs_grad;
        t->name = name;
        return t;
    }
    StatBuf stat_buf(int nslots, int C) {
        StatBuf s;
        s.p = alloc<double>((int64_t)nslots * 2 * C, true);
        s.nslots = nslots;
        return s;
    }
    int gemm_slots(int B, int Hq, int Wq, int Nn, int nphase) const {
        if (!P.det) return AWR_STAT_SLOTS;
        return (int)(((int64_t)B * Hq * Wq + 63) / 64) * ((Nn + 63) / 64) * nphase;
    }
    int reduce_slots() const { return P.det ? AWR_REDUCE_MAX_BLOCKS : AWR_STAT_SLOTS; }
    // the accumulation order (awr_conv_args.accum) of a launch of this K extent and kind under the plan's mode; AUTO resolves per launch
    int accum(int k_extent, int kind) const { return awr::resolve_gemm_accum(P.modes, k_extent, kind); }

    // Split-K scratch: a launch of a few workgroups, each walking a long K loop, is latency-bound and gets scratch for up to `cap` raw copies of its
    // output (split_k_copies: 64x64-tile workgroups x phases x copies below 2048, at least 4 K slices per range at the deepest split, the copies within
    // max_bytes if that is positive); awr_conv_gemm picks the depth (fill ~2 workgroups per CU, >= 8 slices per range), the tuner refines it with
    // depth 1 among its candidates.  Counted in the plan's bytes.
    void split_scratch(awr_conv_args* a, int cap, int64_t max_bytes) {
        const int64_t numel = (int64_t)a->B * a->Hout * a->Wout * a->N;
        const int64_t wgs = ((int64_t)a->B * a->Hq * a->Wq + 63) / 64 * ((a->N + 63) / 64);
        const int smax = split_k_copies(wgs, a->nphase, min_k_steps(*a), cap, numel, max_bytes);
        if (smax > 1) {
            a->partial = alloc<float>((int64_t)smax * numel);
            a->split_max = smax;
        }
    }
    // Inference (low batches): 16 copies, no byte limit.  Not with statistics and not in a parity plan (blocked accumulation): the split-K kernel and
    // the fused pair accumulate in their own order -- a plan built in that mode only contains launch forms that honour it.
    void infer_split_scratch(awr_conv_args* a) {
        if (!P.training && !a->stats && a->accum == 0) split_scratch(a, 16, 0);
    }
    // Training (awr_set_train_split_k), forward and data-gradient launches: at most 8 copies and TRAIN_SPLIT_MAX_BYTES (8 MiB) of
    // scratch per launch -- a training plan has five times the launches of an evaluation plan, the inference rule's 16 copies / 32 MiB cost a ResNet18
    // batch-8 plan 962 MB.  Not for launches with a second input tensor, an un-materialised BatchNorm-backward input, partial-coverage data gradients
    // (the reduce pass reads whole copies), the split-operand product mode, or launches a Winograd form has taken (the callers).
    static constexpr int64_t TRAIN_SPLIT_MAX_BYTES = 8ll << 20;
    void train_split_scratch(awr_conv_args* a) {
        if (!P.training || !P.modes.train_split_k || awr_get_gemm_products() != 1 || a->in2 || a->w2 || a->in_bnb_y || a->partial) return;
        if (a->so != 1 && a->nphase != a->so * a->so) return;
        split_scratch(a, 8, TRAIN_SPLIT_MAX_BYTES);
    }

    float* scratch(int64_t n) {        // slice of the split-K scratch arena (zeroed by ONE fill per step)
        n = round_up(n, 4);
        const int64_t off = scratch_used;
        scratch_used += n;
        if (!P.scratch) P.scratch = alloc<float>(P.scratch_cap);
        if (scratch_used > P.scratch_cap) {
            set_error("plan: wgrad scratch arena too small");
            err = AWR_ERR_ARG;
            return nullptr;
        }
        return P.scratch + off;
    }

    // the forward of this stride-1 3x3 layer may run as Winograd F(2x2, 3x3) (mode, kernel constraints, launch-size rule)
    bool wino_fwd_ok(const Spec& spec, int B, int H, int W) const {
        return P.modes.winograd && !P.det && awr_get_gemm_products() == 1 && !spec.deconv && spec.k == 3 && spec.stride == 1 && spec.pad == 1 &&
               awr::wino_eligible(P.modes.winograd, B, H, W, spec.cin_pad, spec.cout_pad);
    }

    Op& push(std::vector<Op>& list, const std::string& name, std::function<int(void*)> fn) {
        list.emplace_back();
        Op& o = list.back();
        o.fn = std::move(fn);
        o.name = name;
        return o;
    }
    Op& f(const std::string& name, std::function<int(void*)> fn) { return push(P.fwd, name, std::move(fn)); }
    Op& b(const std::string& name, std::function<int(void*)> fn) { return push(P.bwd, name, std::move(fn)); }
    // chain-only backward launch: reads and writes nothing a side or branch stream produces except through its own place in the issuing chain
    // (data / stem / weight gradients, BatchNorm-backward passes, pooling / up-sampling backward, gradient adds) -- no join in front of it
    Op& bc(const std::string& name, std::function<int(void*)> fn) {
        Op& o = b(name, std::move(fn));
        o.joins = false;
        return o;
    }

    // ---- GEMM-family launches (conv / stem family: what run_timed reports and a roofline is quoted for) ----
    enum Chain { FWD, BWD };      // the forward list / the backward list as a chain-only launch (bc)
    // The op, with its algorithmic MACs.  Returns nothing on purpose: a reference into the op vector is dead after the next push (side_ok is said here).
    void gemm_op(Chain c, const std::string& name, std::function<int(void*)> fn, double macs, bool side_ok = false) {
        Op& o = c == FWD ? f(name, std::move(fn)) : bc(name, std::move(fn));
        o.gemm = true;
        o.macs = macs;
        o.side_ok = side_ok;
    }
    // The launch as the tuner and awr_plan_gemm see it.  fixed: a launch with one geometry (tm, tn), nothing for the tuner to choose.
    void tunable(const std::string& name, awr_conv_args* ca, awr_wgrad_args* wa, bool fixed = false, int tm = 0, int tn = 0) {
        GemmRef g{ca, wa, name};
        if (fixed) { g.tm = tm; g.tn = tn; g.tuned = true; }
        P.gemms.push_back(g);
    }
    // A conv argument block (stable address) filled for `prob`; kind (AWR_GEMM_FORWARD / _DGRAD / _OTHER) resolves its accumulation order.
    awr_conv_args* conv_args(const Prob& prob, int B, const float* in, const float* w, const void* w_split, float* out, int T, int kind) {
        P.cargs.emplace_back();
        awr_conv_args* a = &P.cargs.back();
        fill_conv_args(*a, prob, B, in, w, w_split, out, T, accum(prob.k_extent(), kind));
        return a;
    }
    // ... and its launch: the op plus its tunable-launch entry
    void gemm_launch(Chain c, const std::string& name, awr_conv_args* a, std::function<int(void*)> fn, double macs, bool fixed = false, int tm = 0, int tn = 0) {
        gemm_op(c, name, std::move(fn), macs);
        tunable(name, a, nullptr, fixed, tm, tn);
    }
    // x may be an un-materialised BatchNorm(+ReLU) output (Tn::lazy): its consumer applies (scale, shift, relu) while it loads -- set in whatever the
    // consumer launches with (a conv block's in_*, the D or G side of a weight-gradient block, a kernel's arguments).  A plain tensor leaves them alone.
    template <typename R>
    static void lazy_input(const Tn* x, const float*& scale, const float*& shift, R& relu) {
        if (x->lazy) scale = x->lz_scale, shift = x->lz_shift, relu = x->lz_relu;
    }
    // a layer's Winograd-domain weights in `list` (P.wino: forward; P.wino_d: mirrored, for the data gradient), allocated on first use (refresh_weights fills them)
    float* wino_weights(std::vector<std::pair<ConvLayer*, float*>>& list, ConvLayer* layer) {
        for (auto& wl : list)
            if (wl.first == layer) return wl.second;
        float* U = alloc<float>((int64_t)16 * layer->spec.cin_pad * layer->spec.cout_pad);
        list.push_back({layer, U});
        return U;
    }

    void note_grad(const float* tensor, int64_t numel, int job = -1) {
        if (!N.grads || !tensor) return;
        const int64_t lo = tensor - N.grads;
        grad_writes.push_back({lo, lo + numel, (int)P.bwd.size() - 1, job});
    }

    // -> (gradient buffer, accumulate?) and marks the gradient as live
    std::pair<float*, bool> gtarget(Tn* t, bool dgrad_writer = false) {
        if (!dgrad_writer) grad_writers[t].push_back(nullptr);
        if (!t->grad) {
            t->grad = alloc<float>(t->numel());
            return {t->grad, false};
        }
        return {t->grad, true};
    }
    // grad(t) += src_grad where src_grad is a finished gradient buffer: alias when first
    void contribute_identity(Tn* t, float* src_grad) {
        if (!t->needs_grad) return;
        grad_writers[t].push_back(nullptr);
        if (!t->grad) {
            t->grad = src_grad;
        } else {
            float* g = t->grad;
            const int64_t n = t->numel();
            bc("awr_add", [=](void* s) { return awr_add(g, src_grad, g, n, s); });
        }
    }
    void use_layer(ConvLayer* l) {
        for (auto* x : P.layers)
            if (x == l) return;
        if (int e = alloc_packed(&N, l->p_fwd, fwd_pack(l->spec))) err = e;
        if (P.training)
            if (int e = alloc_packed(&N, l->p_dgrad, dgrad_pack(l->spec))) err = e;
        P.layers.push_back(l);
    }

    static double gemm_macs(const Prob& fp, int B, const Spec& s) {
        double taps = 0;
        for (auto& ph : fp.phases) taps += ph.taps.size();
        taps /= (double)(fp.so * fp.so);
        return (double)B * fp.Hout * fp.Wout * s.cout * taps * s.cin;
    }

    // ---- forward branches that may run beside the main chain ----
    void fork(int sid) {
        fork_sid = sid;
        Op& o = f("__fork__", nullptr);
        o.kind = OP_FORK;
        o.sid = sid;
    }
    void end_fork(Tn* result) {
        Op& o = f("__endfork__", nullptr);
        o.kind = OP_ENDFORK;
        o.sid = fork_sid;
        fork_results[result] = fork_sid;
    }
    // Backward branches.  The emitters run in reverse node order, so a marker node pushed AFTER a group of nodes is emitted
    // BEFORE that group's backward ops.
    std::function<int()> bwd_marker(int kind, int sid) {      // the emitter of a fork / end-fork / join marker, for a caller that places it itself
        return [=]() {
            Op& o = b(kind == OP_FORK ? "__fork__" : kind == OP_ENDFORK ? "__endfork__" : "__join__", nullptr);
            o.kind = kind;
            o.sid = sid;
            return err;
        };
    }
    void bwd_marker_node(int kind, int sid) { nodes.push_back(bwd_marker(kind, sid)); }
    void join_if(Tn* t) {
        if (!t) return;
        auto it = fork_results.find(t);
        if (it == fork_results.end()) return;
        Op& o = f("__join__", nullptr);
        o.kind = OP_JOIN;
        o.sid = it->second;
        fork_results.erase(it);
    }

    // ---- ops ----
    // The launch just emitted (P.fwd.back() / P.gemms.back()) produces y: remember it when a 2x2 max-pool of y could ride in it -- an inference launch that
    // is a 1x1 convolution at stride 1 with a plain input, the plain epilogue (bias, optional residual), ordered accumulation, the FP32-MFMA product
    // mode and no split-K scratch (awr_conv_args.pool_out, include/awr_hip.h).  maxpool() checks the map's shape and the switches.
    void note_pool_producer(Tn* y, awr_conv_args* a) {
        if (P.training || awr_get_gemm_products() != 1 || a->nphase != 1 || a->ph[0].ntaps != 1 || (a->ph[0].tap[0] & 0xffff) != 0 || a->T != 1 || a->si != 1 ||
            a->so != 1 || a->in_scale || a->relu_in || a->stats || a->out_scale || a->relu_out || a->accum != 0 || a->partial)
            return;
        y->pool_args = a;
        y->pool_op = P.fwd.size() - 1;
        y->pool_gemm = P.gemms.size() - 1;
    }

    // y = conv(x) [+bias] [*s+t] [+res] [relu]
    Tn* conv(Tn* x, ConvLayer* layer, ConvOpt o = ConvOpt()) {
        use_layer(layer);
        const Spec& spec = layer->spec;
        const int B = x->B;
        const Prob prob = fwd_problem(spec, x->H, x->W);
        Tn* y = new_t(B, prob.Hout, prob.Wout, prob.N, true, layer->name + ".out");
        y->conv_out = o.res == nullptr;      // (its gradient has exactly one reader pair: this conv's weight and data gradient)
        y->conv_taps = spec.T();
        {   // half-batch BatchNorm-backward wavefront (bn_bwd / conv_bwd).  OPT-IN: built for VERDICT r4 item 3, parity-green, and measured SLOWER on every
            // shape (ResNet18 12.8 -> 13.4 ms, Hourglass-1 23.5 -> 24.7 ms at 32 768 rows per half: two half-batch data gradients lose more than the
            // hidden apply pass wins; profiles/r05_half_batch_wavefront.txt).  AWR_HALF_BNB_MIN_ROWS = rows of the data-gradient GEMM per half from
            // which a layer takes part (read per plan); 0 = off, the default.
#ifdef AWR_STUDY
            const int64_t half_min = env_int("AWR_HALF_BNB_MIN_ROWS", 0);
#else
            const int64_t half_min = 0;      // (the wavefront's scheduling states exist in study builds only: ADVICE r5)
#endif
            y->half_ok = P.training && half_min > 0 && !o.res && x->needs_grad && B % 2 == 0 && (int64_t)(B / 2) * x->H * x->W >= half_min;
        }
        if (o.want_stats) y->stats = stat_buf(gemm_slots(B, prob.Hq, prob.Wq, prob.N, (int)prob.phases.size()), prob.N);
        const float* bias = o.use_bias ? layer->bias_ptr() : nullptr;
        join_if(o.res);
        lazy_input(x, o.in_scale, o.in_shift, o.relu_in);
        const std::string name = "awr_conv_gemm:" + layer->name;
        const double macs = gemm_macs(prob, B, spec);
        // Winograd F(2x2, 3x3) forward (round 6, awr_set_conv_winograd; csrc/awr_wino.hip): stride-1 3x3 convolutions whose epilogue is bias /
        // ReLU / statistics.  2.25x fewer multiplies, chains of Cin terms instead of 9 Cin (so no blocked accumulation is needed).  Weight and
        // data gradients stay direct: they only need x and d(y).
        // Inference plans (round 6, last step): the folded eval-mode BatchNorm (out_scale / out_shift) and the residual add of a BasicBlock are epilogue
        // forms of the kernel too.
        if (wino_fwd_ok(spec, B, x->H, x->W) && (!P.training || (!o.res && !o.out_scale)) && !(o.out_scale && o.want_stats) &&
            (o.in_scale == nullptr) == (o.in_shift == nullptr) && (o.out_scale == nullptr) == (o.out_shift == nullptr)) {
            P.wino_args.emplace_back();
            awr_wino_args* wa = &P.wino_args.back();
            memset(wa, 0, sizeof *wa);
            wa->in = x->buf; wa->U = wino_weights(P.wino, layer); wa->bias = bias; wa->in_scale = o.in_scale; wa->in_shift = o.in_shift; wa->out = y->buf;
            wa->stats = y->stats.p; wa->nslots = y->stats.p ? y->stats.nslots : 0;
            wa->res = o.res ? o.res->buf : nullptr;
            wa->out_scale = o.out_scale; wa->out_shift = o.out_shift;
            wa->B = B; wa->H = x->H; wa->W = x->W; wa->C = spec.cin_pad; wa->N = spec.cout_pad; wa->relu = o.relu_out; wa->relu_in = o.relu_in;
            gemm_op(FWD, name, [wa](void* s) { return awr_wino_conv(wa, s); }, macs);      // (the kernel has one geometry: no tunable-launch entry)
            P.n_wino++;
            P.wino_macs += macs;
            if (P.training) {
                const bool has_bias = bias != nullptr;
                nodes.push_back([=]() { return conv_bwd(x, y, layer, nullptr, has_bias); });
            }
            return y;
        }
        awr_conv_args* a = conv_args(prob, B, x->buf, layer->p_fwd.p, layer->p_fwd.split, y->buf, spec.T(), P.training ? AWR_GEMM_FORWARD : AWR_GEMM_OTHER);
        a->in_scale = o.in_scale; a->in_shift = o.in_shift; a->bias = bias;
        a->out_scale = o.out_scale; a->out_shift = o.out_shift;
        a->res = o.res ? o.res->buf : nullptr;
        a->stats = y->stats.p;
        a->stat_slots = y->stats.p ? y->stats.nslots : 0;
        a->relu_in = o.relu_in; a->relu_out = o.relu_out;
        infer_split_scratch(a);
        train_split_scratch(a);
        gemm_launch(FWD, name, a, [a](void* s) { return awr_conv_gemm(a, s); }, macs);
        note_pool_producer(y, a);
        if (P.training) {
            Tn* res = o.res;
            const bool has_bias = bias != nullptr;
            nodes.push_back([=]() { return conv_bwd(x, y, layer, res, has_bias); });
        }
        return y;
    }

    // Inference: y = conv3(relu(bn3(conv2(x)))) + res as ONE launch (awr_conv_args.w2): conv2 has 128 output channels, so a 64x128 tile holds
    // every channel of its pixels and feeds the 1x1 conv3 from LDS -- the intermediate never goes to HBM.  o = conv2's epilogue (folded bn3, ReLU).
    // nullptr when the pair does not qualify (shape, product mode, too few workgroups to fill the chip without split-K).
    Tn* conv_pair(Tn* x, ConvLayer* c2, const ConvOpt& o, ConvLayer* c3, Tn* res, DualLayer* dual = nullptr, Tn* xin = nullptr) {
        const bool off = getenv("AWR_NO_FUSE2") != nullptr;                    // same-box A/B hook (read per plan)
        const int min_wgs = env_int("AWR_FUSE2_MIN_WGS", 1024);                 // (tests force the fused form on small batches)
        const bool no_dual = getenv("AWR_NO_FUSE2_DUAL") != nullptr;
        if (dual) c3 = dual->c3;
        const Spec &s2 = c2->spec, &s3 = c3->spec;
        const int64_t wgs = ((int64_t)x->B * x->H * x->W + 63) / 64;
        const int n1 = s2.cout;
        if (off || P.training || accum(s2.T() * s2.cin_pad, AWR_GEMM_OTHER) != 0 || accum(s3.cin_pad, AWR_GEMM_OTHER) != 0 || awr_get_gemm_products() != 1 || s2.deconv || s3.deconv || s2.stride != 1 || s3.k != 1 || s3.stride != 1 ||
            (n1 != 128 && n1 != 64) || s3.cin != n1 || s3.cout != 2 * n1 || wgs < min_wgs || x->lazy || (dual && no_dual))
            return nullptr;
        if (dual && (dual->sk->spec.k != 1 || dual->sk->spec.stride != 1 || dual->sk->spec.cout != s3.cout || dual->sk->spec.cin_pad % 32 != 0 ||
                     xin->lazy || xin->H != x->H || xin->W != x->W || xin->C != dual->sk->spec.cin_pad))
            return nullptr;
        use_layer(c2);
        const int B = x->B;
        const Prob prob = fwd_problem(s2, x->H, x->W);
        if (prob.so != 1 || prob.phases.size() != 1 || prob.N != n1) return nullptr;
        const float *w2, *bias2;
        int n1x = 0;
        if (dual) {
            (void)conv_dual_prepare(dual);      // [W3 | Wskip] side by side, biases summed (the packed buffer conv_dual launches with)
            w2 = dual->p.p;
            bias2 = dual->bias_sum;
            n1x = dual->sk->spec.cin_pad;
        } else {
            use_layer(c3);
            w2 = c3->p_fwd.p;
            bias2 = c3->bias_ptr();
        }
        if (err) return nullptr;
        Tn* y = new_t(B, prob.Hout, prob.Wout, 2 * n1, true, (dual ? dual->name : c3->name) + ".out");
        join_if(res);
        awr_conv_args* a = conv_args(prob, B, x->buf, c2->p_fwd.p, c2->p_fwd.split, y->buf, s2.T(), AWR_GEMM_OTHER);
        a->N1 = n1;
        a->N = 2 * n1;
        a->w2 = w2;
        a->bias = c2->bias_ptr();
        a->bias2 = bias2;
        a->in_scale = o.in_scale; a->in_shift = o.in_shift; a->relu_in = o.relu_in;
        a->out_scale = o.out_scale; a->out_shift = o.out_shift; a->relu_out = o.relu_out;
        a->res = res ? res->buf : nullptr;
        if (dual) { a->in2 = xin->buf; a->N1x = n1x; }
        if (n1 == 64) a->tile_m = env_int("AWR_FUSE2_TM64", 2), a->tile_n = 1;      // 128x64 tile (what the tuner picks for this conv on its own)
        y->pair_args = a;
        const std::string tail = dual ? "conv3+skip_layer" : c3->name.substr(c3->name.rfind('.', c3->name.rfind('.') - 1) + 1);
        const std::string name = "awr_conv_gemm:" + c2->name + "+" + tail;
        const double macs = gemm_macs(prob, B, s2) + gemm_macs(fwd_problem(s3, prob.Hout, prob.Wout), B, s3) +
                            (dual ? gemm_macs(fwd_problem(dual->sk->spec, prob.Hout, prob.Wout), B, dual->sk->spec) : 0.0);
        gemm_launch(FWD, name, a, [a](void* s) { return awr_conv_gemm(a, s); }, macs, true, n1 == 64 ? a->tile_m : 1, n1 == 64 ? 1 : 2);      // (one geometry)
        return y;
    }

    // registers a dual layer with the plan (packed [W3 | Wskip] buffer + summed bias, refreshed with the weights); idempotent
    int conv_dual_prepare(DualLayer* d) {
        use_layer(d->c3);
        use_layer(d->sk);
        bool seen = false;
        for (auto* q : P.dual_layers) seen = seen || q == d;
        const int cin1 = d->c3->spec.cin_pad, cin2 = d->sk->spec.cin_pad, cout = d->c3->spec.cout;
        if (!seen) {
            if (!d->p.p) {
                PackRecipe r{cout, cin1 + cin2, 1, 0, (int)round_up(cout, N_ALIGN), cin1 + cin2};
                if (int e = alloc_packed(&N, d->p, r)) err = e;
                void* bs = nullptr;
                if (int e = dev_alloc(N.owned, (size_t)cout * 4, true, &bs)) err = e;
                d->bias_sum = (float*)bs;
            }
            P.dual_layers.push_back(d);
        }
        return err;
    }

    // y = conv3(a) + skip(x) (+ both biases) as ONE launch (FP32-MFMA mode): the skip branch's output is never written or re-read.
    // Backward: the two layers' own weight / data gradients, both reading d(y).
    Tn* conv_dual(Tn* a, Tn* x, DualLayer* d, bool want_stats) {
        (void)conv_dual_prepare(d);
        const int cin1 = d->c3->spec.cin_pad, cin2 = d->sk->spec.cin_pad, cout = d->c3->spec.cout;
        const int B = a->B;
        Spec spec = make_spec(false, cin1 + cin2, cout, 1, 1, 0);
        const Prob prob = fwd_problem(spec, a->H, a->W);
        Tn* y = new_t(B, prob.Hout, prob.Wout, prob.N, true, d->name + ".out");
        if (want_stats) y->stats = stat_buf(gemm_slots(B, prob.Hq, prob.Wq, prob.N, 1), prob.N);
        awr_conv_args* ca = conv_args(prob, B, a->buf, d->p.p, nullptr, y->buf, 1, P.training ? AWR_GEMM_FORWARD : AWR_GEMM_OTHER);
        ca->in2 = x->buf;
        ca->Cin1 = cin1;
        lazy_input(a, ca->in_scale, ca->in_shift, ca->relu_in);
        ca->bias = d->bias_sum;
        ca->stats = y->stats.p;
        ca->stat_slots = y->stats.p ? y->stats.nslots : 0;
        gemm_launch(FWD, "awr_conv_gemm:" + d->name, ca, [ca](void* s) { return awr_conv_gemm(ca, s); },
                    gemm_macs(fwd_problem(d->c3->spec, a->H, a->W), B, d->c3->spec) + gemm_macs(fwd_problem(d->sk->spec, x->H, x->W), B, d->sk->spec));
        note_pool_producer(y, ca);
        if (P.training) {
            ConvLayer *c3 = d->c3, *sk = d->sk;
            nodes.push_back([=]() {
                NET_CHECK(conv_bwd(a, y, c3, nullptr, true));
                return conv_bwd(x, y, sk, nullptr, true);
            });
        }
        return y;
    }

    int conv_bwd(Tn* x, Tn* y, ConvLayer* layer, Tn* res, bool has_bias) {
        const Spec& spec = layer->spec;
        const int B = x->B, H = x->H, W = x->W;
        float* dy = y->grad;
        if (!dy) {
            set_error("plan: no gradient reached %s", y->name.c_str());
            return AWR_ERR_ARG;
        }
        // the bias gradient (column sums of dY) falls out of the slices a conv's wgrad kernel stages anyway; only a biased
        // TRANSPOSED conv (none in the reference nets) needs the stand-alone reduction
        const bool fused_bias = has_bias && !spec.deconv;
        if (has_bias && !fused_bias) {
            float* tgt = layer->gbias;
            const int64_t npix = y->npix();
            const int C = y->C;
            b("awr_bias_grad", [=](void* s) { return awr_bias_grad(dy, npix, C, tgt, 0, s); });
            note_grad(tgt, C);
        }
        // weight gradient: split-K partial sums into a packed buffer, then scatter to checkpoint layout
        const WProb wp = wgrad_problem(spec, H, W);
        const int ld = wp.Cg;
        const int64_t rsize = (int64_t)wp.Cd * wp.ntaps * ld;
        const float* D = wp.d_is_dy ? dy : x->buf;
        const float* G = wp.d_is_dy ? x->buf : dy;
        P.wargs.emplace_back();
        awr_wgrad_args* wa = &P.wargs.back();
        fill_wgrad_args(*wa, wp, B, D, G, nullptr, ld);
        if (wp.d_is_dy) lazy_input(x, wa->g_scale, wa->g_shift, wa->g_relu);      // (x is the G side when d(y) is the D side)
        else lazy_input(x, wa->d_scale, wa->d_shift, wa->d_relu);
        int nsum = 1, rstride = 0, bslots = AWR_STAT_SLOTS, bstride = y->C;
        float *R = nullptr, *bsum = nullptr;
        if (P.det) {
            // every K-chunk stores its own copy of the packed gradient (+ bias column sums); the batched scatter sums them in order
            wa->split_stride = rsize;
            const int tiles64 = ((wp.Cd + 63) / 64) * ((wp.Cg + 63) / 64) * wp.ntaps;
            int ms = (2048 + tiles64 - 1) / tiles64;
            wa->max_split = ms < 1 ? 1 : (ms > 256 ? 256 : ms);
            wa->R = const_cast<float*>(D);          // placeholder for the query
            int ns = 0;
            NET_CHECK(awr_conv_wgrad_splits(wa, &ns));
            nsum = ns; rstride = (int)rsize; bslots = ns; bstride = wp.Cd;
            wa->max_split = ns;      // the copies that exist: a later tile / target change can never make the kernel write beyond them
            R = alloc<float>((int64_t)nsum * rsize);
            if (fused_bias) bsum = alloc<float>((int64_t)nsum * wp.Cd);
        } else {
            R = scratch(rsize);
            if (fused_bias) bsum = scratch((int64_t)AWR_STAT_SLOTS * y->C);
        }
        if (err) return err;
        wa->R = R;
        wa->d_colsum = bsum;
        const std::string wname = "awr_conv_wgrad:" + layer->name;
        const double layer_macs = gemm_macs(fwd_problem(spec, H, W), B, spec);      // forward, data gradient and weight gradient cost the same
        if (y->lz_g) {      // d(y) for the weight gradient: written on ITS stream, right in front of it (the data gradient below does not wait for it)
            const float *g = y->lz_g, *yb = y->buf, *mean = y->lz_mean, *invstd = y->lz_invstd, *coef = y->lz_coef;
            const int64_t npix = y->npix();
            const int C = y->C;
            Op& aop = bc("awr_bn_bwd_apply", [=](void* s) { return awr_bn_bwd_apply_only(g, nullptr, yb, mean, invstd, nullptr, nullptr, coef, npix, C, dy, nullptr, nullptr, s); });
            aop.side_ok = (res == nullptr);
            aop.pair_next = true;
        }
        // Winograd-domain weight gradient (winograd = "full"; csrc/awr_wino.hip): stride-1 3x3 layers with channel counts in multiples of 64 whose K loop
        // is long enough to pay for the per-split copies; writes the same packed R (and slot 0 of the bias column sums) the direct kernel accumulates into
        const bool wino_w = (P.modes.winograd & 3) >= 2 && !P.det && awr_get_wgrad_products() == 1 && spec.k == 3 && spec.stride == 1 && spec.pad == 1 &&
                            !spec.deconv && !layer->head && wp.d_is_dy && awr::wino_wgrad_eligible(P.modes.winograd, B, H, W, spec.cin_pad, spec.cout_pad);
        float* wscratch = nullptr;
        if (wino_w) {
            wscratch = alloc<float>(awr_wino_wgrad_scratch(B, H, W, spec.cin_pad, spec.cout_pad));
            if (err) return err;
            P.n_wino++;
            P.wino_macs += layer_macs;
        }
        // safe to run beside the main chain when dY is written once before this node and nobody touches it again.  With a fused
        // residual, d(res) ALIASES dY and later nodes accumulate into it in place -> stays on the main stream.
        const bool side_ok = res == nullptr;
        if (wino_w) {
            const float *wx = x->buf, *wsc = nullptr, *wsh = nullptr;
            int wrelu = 0;
            lazy_input(x, wsc, wsh, wrelu);
            const int wC = spec.cin_pad, wN = spec.cout_pad;
            gemm_op(BWD, wname, [=](void* s) { return awr_wino_wgrad(wx, dy, wsc, wsh, wrelu, B, H, W, wC, wN, wscratch, R, ld, bsum, s); }, layer_macs, side_ok);
        } else {
            gemm_op(BWD, wname, [wa](void* s) { return awr_conv_wgrad(wa, s); }, layer_macs, side_ok);
        }
        // 128 -> 128 3x3 layers on >= 64x64 maps (the Hourglass residuals at full resolution): the one-wave-per-tap-row kernel stages
        // D and the halo'd G patch once for all nine taps (measured: 124 vs 114 TF in isolation, Hourglass-1 step 26.44 -> 25.79 ms; writing relu(bn2(.)) out for them on top: 25.87); on
        // every other shape the workgroup-per-tap kernel is equal or faster (profiles/r02_microbench_wgrad_algos.txt)
        if (!P.det && awr_get_wgrad_products() == 1 && spec.k == 3 && spec.stride == 1 && !spec.deconv && spec.cin == 128 && spec.cout == 128 &&
            H * W >= 4096 && (int64_t)B * H * W >= (1 << 17) && x->lazy)      // (a plain input takes the kernel-row kernel: awr_conv_wgrad's default)
            wa->algo = 2;
        if (!wino_w) tunable(wname, nullptr, wa);      // (tiles / algorithm of the direct kernel)
        // scattered back to checkpoint layout by a batched launch (end of backward / end of its bucket)
        auto add_job = [&](const float* packed, float* grad, int d0, int d1, int T_, int ld_, int slots, int stride, int64_t numel) {
            awr_unpack_job j;
            memset(&j, 0, sizeof j);
            j.packed = packed; j.grad = grad; j.d0 = d0; j.d1 = d1; j.T = T_; j.ld = ld_; j.slots = slots; j.slot_stride = stride;
            unpack_jobs.push_back(j);
            note_grad(grad, numel, (int)unpack_jobs.size() - 1);
        };
        if (!layer->head) {
            const int d0 = spec.deconv ? spec.cin : spec.cout, d1 = spec.deconv ? spec.cout : spec.cin;
            add_job(R, layer->gw, d0, d1, spec.T(), ld, nsum, rstride, (int64_t)d0 * d1 * spec.T());
            if (bsum) add_job(bsum, layer->gbias, 1, spec.cout, 1, spec.cout, bslots, bstride, spec.cout);
        } else {
            const int J = layer->J, cin = spec.cin;
            add_job(R, layer->gw1, 3 * J, cin, 1, ld, nsum, rstride, (int64_t)3 * J * cin);
            add_job(R + (int64_t)3 * J * ld, layer->gw2, J, cin, 1, ld, nsum, rstride, (int64_t)J * cin);
            if (bsum) {
                add_job(bsum, layer->gb1, 1, 3 * J, 1, 3 * J, bslots, bstride, 3 * J);
                add_job(bsum + 3 * J, layer->gb2, 1, J, 1, J, bslots, bstride, J);
            }
        }
        // data gradient
        if (x->needs_grad) {
            const Prob dp = dgrad_problem(spec, H, W);
            auto tgt = gtarget(x, true);
            float* gx = tgt.first;
            bool acc = tgt.second;
            if (!dp.full && !acc) {
                Op& z = b("__zero__", nullptr);
                z.kind = OP_ZERO;
                z.p = gx;
                z.bytes = (size_t)x->numel() * 4;
                acc = true;
            }
            awr_conv_args* da = conv_args(dp, B, y->lz_g ? y->lz_g : dy, layer->p_dgrad.p, layer->p_dgrad.split, gx, spec.T(), AWR_GEMM_DGRAD);
            if (y->lz_g) { da->in_bnb_y = y->buf; da->in_bnb_coef = y->lz_lin4; }
            da->res = acc ? gx : nullptr;
            // remember who wrote d(x), in order: a full-coverage dgrad that is the LAST producer can host the fused BN-backward reduction
            grad_writers[x].push_back(dp.full ? da : nullptr);
            const std::string dname = "awr_conv_dgrad:" + layer->name;
#ifdef AWR_STUDY
            if (y->half_dy && res == nullptr) {      // d(y) arrives half by half (bn_bwd): part 0 now, part 1 behind the record of half B
                gemm_op(BWD, dname, [da](void* s) { return awr_conv_gemm_part(da, 2, 0, s); }, 0.5 * layer_macs);
                b("__halfwait__", nullptr).kind = OP_HALFWAIT;
                gemm_op(BWD, dname + "/b", [da](void* s) { return awr_conv_gemm_part(da, 2, 1, s); }, 0.5 * layer_macs);
            } else
#endif
            {
                if (y->half_dy) b("__halfwait__", nullptr).kind = OP_HALFWAIT;      // (cannot happen: half_ok excludes a fused residual) -- still correct: wait for half B first
                // Winograd data gradient (round 6): same eligibility as the forward; the launch decides from the COMPLETED argument block whether it
                // implements its epilogue (plain, accumulate, BatchNorm-backward reduction) and runs the direct kernel otherwise
                float* Ud = nullptr;
                if ((P.modes.winograd & 3) == 2 && !P.det && awr_get_gemm_products() == 1 && !spec.deconv && spec.k == 3 && spec.stride == 1 && spec.pad == 1 &&
                    dp.full && !y->lz_g && awr::wino_eligible(P.modes.winograd, B, dp.Hin, dp.Win, spec.cout_pad, spec.cin_pad)) {
                    Ud = wino_weights(P.wino_d, layer);
                    P.wino_dg.push_back({da, layer_macs});
                }
                if (!Ud) train_split_scratch(da);      // (in_bnb_y / partial-coverage launches are refused inside)
                if (Ud) gemm_op(BWD, dname, [da, Ud](void* s) { return awr_wino_dgrad_or_direct(da, Ud, s); }, layer_macs);
                else gemm_op(BWD, dname, [da](void* s) { return awr_conv_gemm(da, s); }, layer_macs);
            }
            tunable(dname, da, nullptr);
        }
        if (res) contribute_identity(res, dy);
        return err;
    }

    // inference: per-channel (scale, shift) of an eval-mode BatchNorm, refreshed with the weights
    std::pair<const float*, const float*> fold_bn(BNLayer* bn) {
        float *sc = alloc<float>(bn->C), *sh = alloc<float>(bn->C);
        const int C = bn->C;
        const float *g = bn->gamma, *bt = bn->beta, *rm = bn->rmean, *rv = bn->rvar;
        push(P.pack_ops, "awr_bn_fold_eval", [=](void* s) { return awr_bn_fold_eval(C, g, bt, rm, rv, BN_EPS, sc, sh, s); });
        return {sc, sh};
    }

    float bn_momentum() const { return (float)(1.0 - pow(1.0 - (double)BN_MOMENTUM, (double)P.bn_repeat)); }

    // training-mode BatchNorm (+residual) (+ReLU): a = [relu](bn(y) [+ res]).  lazy (no residual): the normalised tensor is NOT
    // written; the returned handle carries (scale, shift, relu) for its consumers
    Tn* bn_act(Tn* y, BNLayer* bn, bool relu, Tn* res = nullptr, bool lazy = false) {
        const int B = y->B, H = y->H, W = y->W, C = y->C;
        const int64_t npix = y->npix();
        StatBuf own = y->stats;
        if (!own.p) {
            own = stat_buf(reduce_slots(), C);
            const float* xb = y->buf;
            double* sp = own.p;
            const int ns = own.nslots;
            if (y->fstats && !y->fstats->sp) {      // the max-pool / up-sampling add that wrote y accumulates them on the way (round 5): no pass of its own
                y->fstats->sp = sp;
                y->fstats->ns = ns;
            } else {
                f("awr_channel_stats", [=](void* s) { return awr_channel_stats(xb, npix, C, sp, ns, s); });
            }
        }
        // several BNs may normalise the same tensor (hourglass): finalize zeroes the accumulator, so every BN gets its own
        y->stats = StatBuf();
        float* coef4 = alloc<float>(4 * (int64_t)C);     // [scale | shift | mean | invstd][C]: one buffer so fused consumers take one pointer
        float *sc = coef4, *sh = coef4 + C, *mean = coef4 + 2 * C, *invstd = coef4 + 3 * C;
        const float mom = bn_momentum();
        {
            double* sp = own.p;
            const int ns = own.nslots;
            const float *g = bn->gamma, *bt = bn->beta;
            float *rm = bn->rmean, *rv = bn->rvar;
            f("awr_bn_finalize", [=](void* s) { return awr_bn_finalize(sp, C, npix, g, bt, rm, rv, mom, BN_EPS, sc, sh, mean, invstd, ns, s); });
        }
        Tn* a;
        if (lazy && !res) {
            P.tensors.emplace_back();
            a = &P.tensors.back();
            *a = Tn();
            a->buf = y->buf; a->B = B; a->H = H; a->W = W; a->C = C;
            a->name = bn->name + ".act(lazy)";
            a->lazy = true; a->lz_scale = sc; a->lz_shift = sh; a->lz_relu = relu;
        } else {
            a = new_t(B, H, W, C, true, bn->name + ".act");
            join_if(res);
            const float* xb = y->buf;
            const float* rb = res ? res->buf : nullptr;
            float* ob = a->buf;
            f("awr_bn_apply", [=](void* s) { return awr_bn_apply(xb, sc, sh, rb, relu ? 1 : 0, ob, npix, C, s); });
            if (!relu && !res) { a->bn_y = y->buf; a->bn_coef4 = coef4; }
        }
        nodes.push_back([=]() { return bn_bwd(y, a, bn, relu, res, mean, invstd, sc, sh, coef4); });
        return a;
    }

    int bn_bwd(Tn* y, Tn* a, BNLayer* bn, bool relu, Tn* res, float* mean, float* invstd, float* sc, float* sh, float* coef4) {
        float* da = a->grad;
        if (!da) {
            set_error("plan: no gradient reached %s", a->name.c_str());
            return AWR_ERR_ARG;
        }
        const int C = y->C;
        const int64_t npix = y->npix();
        float* coef = alloc<float>(3 * (int64_t)C);
        // Fused reduction: when the ONLY producer of d(a) is one full-coverage data-gradient GEMM (a BN+ReLU output read by a
        // single conv, materialised or not), that GEMM's epilogue masks with the re-derived ReLU and accumulates sum g /
        // sum g*xhat itself -- the separate reduction pass over d(a) and y disappears and the apply pass needs no mask.
        // With a residual added before the ReLU (ResNet block outputs: d(a) = the next block's skip gradient + its conv1 data gradient)
        // the LAST producer qualifies: it adds its tile onto the earlier contributions in place, takes the mask from the stored
        // activation, reduces, and leaves the MASKED gradient behind -- which is also d(res).
        auto& writers = grad_writers[a];
        awr_conv_args* ga = (!writers.empty() && relu) ? writers.back() : nullptr;
        if (ga && ga->res && (ga->res != ga->out || !res)) ga = nullptr;      // accumulating producers only for the residual form, in place
        if (ga && !ga->res && writers.size() != 1) ga = nullptr;
        const bool fused = ga != nullptr;
        StatBuf sums;
        if (fused) {
            sums = stat_buf(gemm_slots(ga->B, ga->Hq, ga->Wq, ga->N, ga->nphase), C);
            ga->bnr_y = y->buf;
            ga->bnr_coef = coef4;
            ga->bnr_act = res ? a->buf : nullptr;
            ga->stats = sums.p;
            ga->stat_slots = sums.nslots;
            // the residual is itself a BatchNorm output (no ReLU of its own: the downsample projection): its backward needs sum g and
            // sum g * xhat over the SAME masked gradient -- reduced here too, its stand-alone reduction pass disappears
            static const bool no_bnr2 = getenv("AWR_NO_BNR2") != nullptr;      // same-box A/B hook
            if (res && res->bn_y && res->needs_grad && res->C == C && !no_bnr2) {
                res->pre_sums = stat_buf(sums.nslots, C);
                ga->bnr2_y = res->bn_y;
                ga->bnr2_coef = res->bn_coef4;
                ga->stats2 = res->pre_sums.p;
            }
        } else if (a->pre_sums.p && !relu && !res) {
            sums = a->pre_sums;
        } else {
            sums = stat_buf(reduce_slots(), C);
        }
        // ReLU mask: without a residual the activation is re-derived from y (no read of `a`); with one it needs `a`; a fused producer
        // has applied it already
        const float* act = (relu && res && !fused) ? a->buf : nullptr;
        const float* msc = (relu && !res && !fused) ? sc : nullptr;
        const float* msh = (relu && !res && !fused) ? sh : nullptr;
        const float* yb = y->buf;
        double* sp = sums.p;
        const int ns = sums.nslots;
        const bool pre_reduced = !fused && a->pre_sums.p && !relu && !res;
        if (!fused && !pre_reduced) bc("awr_bn_bwd_reduce", [=](void* s) { return awr_bn_bwd_reduce(da, act, yb, mean, invstd, msc, msh, npix, C, sp, ns, s); });
        float* gy;
        bool acc = false;
        if (y->needs_grad) {
            auto t = gtarget(y);
            gy = t.first;
            acc = t.second;
        } else {
            gy = alloc<float>(y->numel());
        }
        float *g_out = nullptr, *post_add = nullptr;
        if (res && res->needs_grad && relu && !fused) {      // the masked gradient is d(res): written out by the apply kernel
            grad_writers[res].push_back(nullptr);
            if (!res->grad) {
                res->grad = alloc<float>(res->numel());
                g_out = res->grad;
            } else {
                g_out = alloc<float>(res->numel());
                post_add = g_out;
            }
        }
        // Off the critical chain (round 4): when the masked gradient g is already in memory (fused reduction, no residual: nobody accumulates
        // into that buffer later) and y is a plain conv output, the data gradient of that conv evaluates the BatchNorm backward itself from
        // (g, y) and four coefficient vectors -- only the small finalize stays between the two dependent data-gradient GEMMs; the apply pass
        // that writes d(y) for the weight gradient is emitted by conv_bwd on the weight gradient's side stream.
        // Measured (profiles/r04_bn_bwd_lazy.txt) and NOT the default: the implicit GEMM re-stages every input element once per tap, so a 3x3
        // data gradient pays the arithmetic and the second tensor's traffic NINE times (ResNet18 13.28 -> 14.2 ms, Hourglass-1 24.1 -> 25.9 ms
        // with every eligible BatchNorm); restricted to single-tap (1x1) convolutions it is a wash (Hourglass-1 23.9 vs 24.1 ms).  The upper
        // bound -- the step with the apply passes simply left out -- is 12.76 / 21.7 ms, so the pass IS exposed, but the consumer is the
        // wrong place to hide it.  AWR_LAZY_BNB: 0 = never (default), 1 = 1x1 convolutions, 2 = every eligible BatchNorm.
        const int lazy_mode = env_int("AWR_LAZY_BNB", 0);
        const bool lazy_bnb = lazy_mode > 0 && fused && relu && !res && !acc && !g_out && y->conv_out && (lazy_mode > 1 || y->conv_taps == 1) && y->needs_grad &&
                              C <= 512 && awr_get_gemm_products() == 1 && awr_get_gemm_staging() == 2;
        {
            const float* gam = bn->gamma;
            float *gg = bn->ggamma, *gb = bn->gbeta;
            const float* dy_add = acc ? gy : nullptr;
            if (lazy_bnb) {
                float* lin4 = alloc<float>(4 * (int64_t)C);
                bc("awr_bn_bwd_finalize", [=](void* s) { return awr_bn_bwd_finalize_lin(sp, C, npix, gam, mean, invstd, coef, lin4, gg, gb, 0, ns, s); });
                y->lz_g = da; y->lz_lin4 = lin4; y->lz_mean = mean; y->lz_invstd = invstd; y->lz_coef = coef;
            } else if (y->half_ok && y->needs_grad) {
                // Half-batch wavefront (round 5): the reduction needs the whole batch, the apply and the data gradient behind it do
                // not.  finalize -> apply(half A) on the issuing chain -> apply(half B) on the stream the layer's weight gradient is about to take
                // (it waits for the chain, i.e. starts when half A is done, and the weight gradient queues behind it: it needs both halves anyway)
                // -> conv_bwd issues dgrad(half A) beside it, waits for half B's record, then dgrad(half B).  The HBM-bound pass runs beside an
                // MFMA-bound one instead of alone; no extra stream (the runtime's four hardware queues are taken).
                bc("awr_bn_bwd_finalize", [=](void* s) { return awr_bn_bwd_finalize(sp, C, npix, gam, invstd, coef, gg, gb, 0, ns, s); });
                const int64_t hp = npix / 2, off = hp * C;
                bc("awr_bn_bwd_apply", [=](void* s) {
                    return awr_bn_bwd_apply_only(da, act, yb, mean, invstd, msc, msh, coef, hp, C, gy, dy_add, g_out, s);
                });
                Op& hb = bc("awr_bn_bwd_apply", [=](void* s) {
                    return awr_bn_bwd_apply_only(da + off, act ? act + off : nullptr, yb + off, mean, invstd, msc, msh, coef, npix - hp, C, gy + off,
                                                 dy_add ? dy_add + off : nullptr, g_out ? g_out + off : nullptr, s);
                });
                hb.side_ok = true;
                hb.pair_next = true;
                hb.half_sig = true;
                y->half_dy = true;
            } else {
                bc("awr_bn_bwd_apply", [=](void* s) {
                    return awr_bn_bwd_apply(da, act, yb, mean, invstd, gam, msc, msh, sp, coef, npix, C, gy, dy_add, g_out, gg, gb, 0, ns, s);
                });
            }
        }
        note_grad(bn->ggamma, C);
        note_grad(bn->gbeta, C);
        if (post_add) {
            float* rg = res->grad;
            const int64_t n = res->numel();
            bc("awr_add", [=](void* s) { return awr_add(rg, post_add, rg, n, s); });
        }
        if (res && res->needs_grad && (!relu || fused)) contribute_identity(res, da);      // d(a) itself (already masked when fused) is d(res)
        return err;
    }

    // y is written by a max-pool / up-sampling add that can accumulate the next BatchNorm's statistics on the way (round 5): the slot bn_act fills in
    // when it takes the offer (nullptr: no offer)
    FusedStats* offer_stats(Tn* y) {
        if (!P.training || !env_int("AWR_FUSED_POOL_STATS", 1) || y->C % 4 != 0 || (y->C > 1024 && y->C % 1024 != 0)) return nullptr;
        P.fstats.emplace_back();
        return y->fstats = &P.fstats.back();
    }

    // May the 2x2 max-pool of x be written by the 1x1 launch that produces x?  The width rule is checked against the widest tile the launch can run
    // with before it is tuned (the launcher's heuristic takes 128-row tiles -- 64 columns -- for K extents of at most 64); the tuner and
    // awr_plan_set_gemm keep to the tiles the map's width admits.
    bool gemm_pool_ok(Tn* x, int k, int s_, int p) const {
        const awr_conv_args* a = x->pool_args;
        if (P.training || !a || a->pool_out || k != 2 || s_ != 2 || p != 0 || x->lazy || x->H % 2 != 0) return false;
        const int tm = a->tile_m ? a->tile_m : a->Cin <= 64 ? 2 : 1;
        return x->W % (32 * tm) == 0 && env_int("AWR_PAIR_POOL", 1) && env_int("AWR_GEMM_POOL", 1) && awr_get_gemm_staging() != 0;
    }

    Tn* maxpool(Tn* x, int k, int s_, int p) {
        const int B = x->B, H = x->H, W = x->W, C = x->C;
        const int Ho = (H + 2 * p - k) / s_ + 1, Wo = (W + 2 * p - k) / s_ + 1;
        Tn* y = new_t(B, Ho, Wo, C, true, x->name + ".pool");
        uint8_t* arg = P.training ? alloc<uint8_t>((int64_t)B * Ho * Wo * C) : nullptr;
        {
            const float* xb = x->buf;
            const float *ls = nullptr, *lt = nullptr;
            int lr = 0;
            lazy_input(x, ls, lt, lr);
            float* ob = y->buf;
            FusedStats* fs = offer_stats(y);
            // inference: a 2x2 / stride-2 pool of a fused pair's output is written by the pair itself (awr_conv_args.pool_out: 2D workgroup tiles, the
            // windows reduced in the epilogue) -- no pass that re-reads the full-resolution tensor.  AWR_PAIR_POOL=0: the separate pass (A/B hook)
            awr_conv_args* pa = x->pair_args;
            const int pbm = pa && pa->N1 == 64 && pa->tile_m == 2 ? 128 : 64;
            if (!P.training && pa && !pa->pool_out && k == 2 && s_ == 2 && p == 0 && !x->lazy && H % 2 == 0 && W % (pbm / 2) == 0 && env_int("AWR_PAIR_POOL", 1) &&
                awr_get_gemm_staging() != 0 && env_int("AWR_FUSE2_DMA", 1) && !pa->in_scale && !pa->relu_in) {
                pa->pool_out = ob;
            } else if (gemm_pool_ok(x, k, s_, p)) {
                // ... and so is the pool of a plain / two-tensor 1x1 launch's output (conv3 (+ skip) of a residual whose pair did not form: Winograd plans, low
                // batches, AWR_NO_FUSE2).  AWR_GEMM_POOL=0: this form off (A/B hook, read per plan); AWR_PAIR_POOL=0: no pool rides in any GEMM launch
                x->pool_args->pool_out = ob;
                P.fwd[x->pool_op].name += "+pool";
                P.gemms[x->pool_gemm].name += "+pool";
            } else {
                f("awr_maxpool_fwd", [=](void* s) {
                    return fs && fs->sp ? awr_maxpool_fwd_stats(xb, ls, lt, lr, B, H, W, C, k, s_, p, ob, arg, fs->sp, fs->ns, s)
                                        : awr_maxpool_fwd(xb, ls, lt, lr, B, H, W, C, k, s_, p, ob, arg, s);
                });
            }
        }
        if (P.training) {
            nodes.push_back([=]() {
                if (!x->needs_grad) return (int)AWR_OK;
                auto t = gtarget(x);
                float* gx = t.first;
                const int acc = t.second ? 1 : 0;
                float* gyb = y->grad;
                bc("awr_maxpool_bwd", [=](void* s) { return awr_maxpool_bwd(gyb, arg, B, H, W, C, k, s_, p, gx, acc, s); });
                return err;
            });
        }
        return y;
    }

    // out = up1 + nearest_upsample_x2(low)   (hourglass.py:77,:88)
    Tn* upsample_add(Tn* up1, Tn* low) {
        const int B = low->B, Hl = low->H, Wl = low->W, C = low->C;
        join_if(up1);
        Tn* y = new_t(B, 2 * Hl, 2 * Wl, C, true, up1->name + ".upadd");
        {
            const float *ub = up1->buf, *lb = low->buf;
            float* ob = y->buf;
            FusedStats* fs = offer_stats(y);
            f("awr_upsample2_add", [=](void* s) {
                return fs && fs->sp ? awr_upsample2_add_stats(ub, lb, B, Hl, Wl, C, ob, fs->sp, fs->ns, s) : awr_upsample2_add(ub, lb, B, Hl, Wl, C, ob, s);
            });
        }
        if (P.training) {
            nodes.push_back([=]() {
                auto t = gtarget(low);
                float* gl = t.first;
                const int acc = t.second ? 1 : 0;
                float* gyb = y->grad;
                bc("awr_upsample2_bwd", [=](void* s) { return awr_upsample2_bwd(gyb, B, Hl, Wl, C, gl, acc, s); });
                contribute_identity(up1, y->grad);
                return err;
            });
        }
        return y;
    }

    // NHWC (B,F,F,Cp) dense map -> the reference's NCHW (B,4J,F,F) tensor (+ gradient bridge)
    void head_out(Tn* pred, int J, float* out, float* gout) {
        const int B = pred->B, F = pred->H, Cp = pred->C;
        {
            const float* pb = pred->buf;
            f("awr_nhwc_to_nchw", [=](void* s) { return awr_nhwc_to_nchw(pb, B, F * F, Cp, 4 * J, out, s); }).boundary = true;
        }
        const int stage = (int)P.outputs.size();
        P.outputs.push_back(out);
        P.grad_outs.push_back(gout);
        P.head_preds.push_back(pred);
        P.head_grads.push_back(nullptr);
        if (P.training) {
            nodes.push_back([=]() {
                if (!(P.supervised & (1u << stage))) return (int)AWR_OK;   // no loss on this stage (hourglass: only the last stage, train.py:116-121)
                auto t = gtarget(pred);
                float* g = t.first;
                if (t.second) {
                    float* tmp = alloc<float>(pred->numel());
                    const int64_t n = pred->numel();
                    b("awr_nchw_to_nhwc", [=](void* s) { return awr_nchw_to_nhwc(gout, B, F * F, Cp, 4 * J, tmp, s); });
                    bc("awr_add", [=](void* s) { return awr_add(g, tmp, g, n, s); });
                } else {
                    b("awr_nchw_to_nhwc", [=](void* s) { return awr_nchw_to_nhwc(gout, B, F * F, Cp, 4 * J, g, s); }).boundary = true;
                    P.head_grads[stage] = g;      // the only producer: a caller on the NHWC boundary writes d(pred) here itself
                }
                return err;
            });
        }
    }

    // Stems as the fused kernels of awr_stem.hip -- the un-normalised full-resolution conv output is never written, forward or
    // backward.  pool: ResNet (resnet_deconv.py:31-36, :118-121): conv 5x5 (1 -> 64, no bias) -> BatchNorm -> ReLU -> MaxPool(3,2,1),
    // the result is the pooled map.  !pool: hourglass (hourglass.py:112): conv 5x5 (bias) -> BatchNorm -> ReLU at full resolution.
    Tn* stem(float* img, ConvLayer* conv, BNLayer* bn, int H, int W, bool pool) {
        const int B = P.B;
        Tn* y = pool ? new_t(B, H / 2, W / 2, 64, true, conv->name + ".pool") : new_t(B, H, W, 64, true, conv->name + ".act");
        const float *w = conv->w, *bias = conv->bias;
        const std::string tag = ":" + conv->name;
        const int64_t npix = (int64_t)B * H * W;
        float* yb = y->buf;
        const double macs = (double)npix * 64 * 25;     // algorithmic work: the conv once forward, its weight gradient once backward
        // the forward launch: conv -> (sc, sh) -> ReLU [-> max-pool, its argmax to `arg` in training]
        auto forward = [&](const float* sc, const float* sh, uint8_t* arg) {
            if (pool) gemm_op(FWD, "awr_stem_pool" + tag, [=](void* s) { return awr_stem_pool(img, w, sc, sh, B, H, W, yb, arg, s); }, macs);
            else gemm_op(FWD, "awr_stem_conv" + tag, [=](void* s) { return awr_stem_conv(img, w, bias, sc, sh, 1, B, H, W, yb, s); }, macs);
        };
        if (!P.training) {
            auto ss = fold_bn(bn);
            forward(ss.first, ss.second, nullptr);
            return y;
        }
        int ns_stats = AWR_STAT_SLOTS, ns_dw = AWR_STAT_SLOTS;
        if (P.det && awr_stem_slots(B, H, W, &ns_stats, &ns_dw)) err = AWR_ERR_ARG;
        StatBuf stats = stat_buf(ns_stats, 64);
        float* coef4 = alloc<float>(4 * 64);
        uint8_t* arg = pool ? alloc<uint8_t>((int64_t)B * (H / 2) * (W / 2) * 64) : nullptr;
        const float mom = bn_momentum();
        {
            double* sp = stats.p;
            gemm_op(FWD, "awr_stem_stats" + tag, [=](void* s) { return awr_stem_stats(img, w, bias, B, H, W, sp, ns_stats, s); }, 0.0);
            const float *g = bn->gamma, *bt = bn->beta;
            float *rm = bn->rmean, *rv = bn->rvar;
            f("awr_bn_finalize", [=](void* s) {
                return awr_bn_finalize(sp, 64, npix, g, bt, rm, rv, mom, BN_EPS, coef4, coef4 + 64, coef4 + 128, coef4 + 192, ns_stats, s);
            });
            forward(coef4, coef4 + 64, arg);
        }
        nodes.push_back([=]() {
            if (!y->grad) {
                set_error("plan: no gradient reached the stem");
                return (int)AWR_ERR_ARG;
            }
            StatBuf sums = stat_buf(ns_stats, 64);
            float* coef = alloc<float>(3 * 64);
            float* slots = alloc<float>((int64_t)ns_dw * 64 * 26, true);
            float* dp = y->grad;
            double* sp = sums.p;
            gemm_op(BWD, "awr_stem_bwd_reduce" + tag, [=](void* s) { return awr_stem_bwd_reduce(img, w, bias, coef4, dp, arg, B, H, W, sp, ns_stats, s); }, 0.0);
            const float* gam = bn->gamma;
            float *gg = bn->ggamma, *gb = bn->gbeta;
            bc("awr_bn_bwd_finalize", [=](void* s) { return awr_bn_bwd_finalize(sp, 64, npix, gam, coef4 + 192, coef, gg, gb, 0, ns_stats, s); });
            note_grad(bn->ggamma, 64);
            note_grad(bn->gbeta, 64);
            float *gw = conv->gw, *gbias = bias ? conv->gbias : nullptr;
            gemm_op(BWD, "awr_stem_bwd_wgrad" + tag,
                    [=](void* s) { return awr_stem_bwd_wgrad(img, w, bias, coef4, coef, dp, arg, B, H, W, slots, gw, gbias, ns_dw, s); }, macs);
            note_grad(conv->gw, 64 * 25);
            if (gbias) note_grad(gbias, 64);
            return err;
        });
        return y;
    }
};


static int make_unpack_op(Builder& bld, const std::vector<int>& job_ids, Op& out) {
    std::vector<awr_unpack_job> jobs;
    int64_t total = 0;
    for (int id : job_ids) {
        awr_unpack_job j = bld.unpack_jobs[id];
        j.first = total;                 // one workgroup per gradient row
        total += j.d0;
        jobs.push_back(j);
    }
    void* tab = nullptr;
    NET_CHECK(upload_table(bld.P, jobs.data(), jobs.size() * sizeof(awr_unpack_job), &tab));
    const int n = (int)jobs.size();
    out = Op();
    out.name = "awr_unpack_wgrads_batched";
    out.scatter = true;
    out.fn = [=](void* s) { return awr_unpack_wgrads_batched((const awr_unpack_job*)tab, n, total, s); };
    return AWR_OK;
}

static int build_backward(Builder& bld) {
    awr_plan& P = bld.P;
    // split-K scratch for every weight gradient, as one arena (capacity = all packed gradients of the used layers)
    P.scratch_cap = 64;
    for (auto* l : P.layers)
        P.scratch_cap += round_up(!l->spec.deconv ? l->p_fwd.numel() : l->p_dgrad.numel(), 4) + AWR_STAT_SLOTS * round_up(l->spec.cout_pad, 4);
    const size_t first = P.bwd.size();
    bld.b("__zero__", nullptr).kind = OP_ZERO;       // placeholder for the scratch fill (kept in place so recorded op indices stay valid)
    for (size_t i = bld.nodes.size(); i-- > 0;) NET_CHECK(bld.nodes[i]());
    if (bld.err) return bld.err;
    if (P.scratch) {
        P.bwd[first].p = P.scratch;
        P.bwd[first].bytes = (size_t)bld.scratch_used * 4;
    } else {
        P.bwd[first].p = bld.alloc<float>(4);
        P.bwd[first].bytes = 16;
    }
    const int64_t n_active = P.net->layout.n_active;
    if (P.n_buckets <= 1 || bld.grad_writes.empty()) {
        if (!bld.unpack_jobs.empty()) {       // ONE launch scatters every packed weight gradient back to checkpoint layout
            std::vector<int> ids(bld.unpack_jobs.size());
            for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int)i;
            Op op;
            NET_CHECK(make_unpack_op(bld, ids, op));
            P.bwd.push_back(op);
        }
        P.buckets = {{0, n_active, (int)P.bwd.size() - 1}};
    } else {
        // data-parallel overlap: each bucket's weight gradients are scattered into the arena as soon as the backward has passed
        // its layers, then a marker lets the host start that bucket's all-reduce while the backward continues
        std::vector<Range> writes;
        for (auto& w : bld.grad_writes) writes.push_back({w.lo, w.hi, w.ready});
        P.buckets = plan_buckets(writes, n_active, P.n_buckets);
        struct Ins { int pos; std::vector<Op> ops; };
        std::vector<Ins> inserts;
        for (auto& bk : P.buckets) {
            std::vector<int> ids;
            for (auto& w : bld.grad_writes)
                if (w.job >= 0 && bk.lo <= w.lo && w.lo < bk.hi) ids.push_back(w.job);
            Ins in;
            in.pos = bk.ready + 1;
            if (!ids.empty()) {
                Op op;
                NET_CHECK(make_unpack_op(bld, ids, op));
                in.ops.push_back(op);
            }
            Op m;
            m.kind = OP_BUCKET;
            m.name = "__bucket__";
            m.lo = bk.lo;
            m.hi = bk.hi;
            in.ops.push_back(m);
            inserts.push_back(in);
        }
        std::stable_sort(inserts.begin(), inserts.end(), [](const Ins& a, const Ins& b) { return a.pos > b.pos; });
        for (auto& in : inserts) P.bwd.insert(P.bwd.begin() + in.pos, in.ops.begin(), in.ops.end());
    }
    P.built_bwd = true;
    return AWR_OK;
}

// ---- the two backbones (nets.py: ResNet18Deconv.build / HourglassNet.build) ----------------------------------
struct NetBuilder {
    Builder& b;
    awr_plan& P;
    awr_net& N;
    std::vector<std::function<int()>>& nodes;      // the builder's backward emitters: the block builders below reorder them
    explicit NetBuilder(Builder& bb) : b(bb), P(bb.P), N(bb.N), nodes(bb.nodes) {}
    ConvLayer* C(const std::string& k) { return &N.convs.at(k); }
    BNLayer* BN(const std::string& k) { return &N.bns.at(k); }

    // conv -> BatchNorm [-> +res] [-> ReLU]; fused into one GEMM epilogue in inference.  lazy (training): the BN+ReLU output is
    // not materialised -- legal when every consumer is a conv / max-pool loader
    Tn* cbr(Tn* x, const std::string& conv, const std::string& bn, bool relu, Tn* res = nullptr, bool lazy = false) {
        ConvLayer* cl = C(conv);
        ConvOpt o;
        o.use_bias = cl->bias_ptr() != nullptr;
        if (P.training) {
            o.want_stats = true;
            Tn* y = b.conv(x, cl, o);
            return b.bn_act(y, BN(bn), relu, res, lazy && !res);
        }
        auto ss = b.fold_bn(BN(bn));
        o.out_scale = ss.first; o.out_shift = ss.second; o.res = res; o.relu_out = relu;
        return b.conv(x, cl, o);
    }

    void resnet(float* img, int H, float* out, float* gout) {
        Tn* c = b.stem(img, C("pre.0"), BN("pre.1"), H, H, true);      // conv 5x5 -> BN -> ReLU -> MaxPool(3,2,1), one fused kernel family
        const bool bott = N.depth != 18;
        const int* nb = resnet_blocks(N.depth);
        for (int li = 1; li <= 4; ++li)
            for (int bi = 0; bi < nb[li - 1]; ++bi) {
                const std::string p = fmt("layer%d.%d", li, bi);
                Tn* r;
                const size_t n0 = nodes.size();
                size_t n1 = n0;
                if (N.convs.count(p + ".downsample.0")) {   // 1x1 projection (+ stride) + its BatchNorm: independent of the main branch until the residual add
                    b.fork(0);
                    r = cbr(c, p + ".downsample.0", p + ".downsample.1", false);
                    b.end_fork(r);
                    n1 = nodes.size();
                } else {
                    r = c;
                }
                // bn1 (+ bn2 of a Bottleneck) + ReLU feed ONE conv only: un-materialised (applied by that conv's loaders) while that is
                // cheaper than one write + read of the tensor -- the loader arithmetic costs 8-15 % of a GEMM whose K grows with the
                // channel count, the tensor pass does not: beyond 128 channels the activation is written out
                Tn* o = cbr(c, p + ".conv1", p + ".bn1", true, nullptr, C(p + ".conv1")->spec.cout <= 128);
                if (!bott) {
                    c = cbr(o, p + ".conv2", p + ".bn2", true, r);
                } else {
                    o = cbr(o, p + ".conv2", p + ".bn2", true, nullptr, C(p + ".conv2")->spec.cout <= 128);
                    c = cbr(o, p + ".conv3", p + ".bn3", true, r);
                }
                // Backward of a block with a projection (the emitters run in reverse node order).  Two things are arranged here:
                // (i) the projection's data gradient covers only one of the four stride phases of d(c) (zero fill + accumulate), conv1's
                // covers all of it: with the projection's backward emitted FIRST, conv1's data gradient is the LAST producer of d(c) -- a
                // full-coverage GEMM that adds in place and can host the fused BatchNorm-backward reduction of the previous block's
                // output (with the projection's own BatchNorm reduced in this block's bn-output GEMM, bn_bwd: no stand-alone reduction
                // pass is left in a ResNet step);  (ii) the projection's backward (BatchNorm apply, a small 1x1 weight and data gradient)
                // only needs the masked d(out) and only meets the main chain again at conv1's data gradient: it runs on a branch stream
                // beside the block's conv backward.  Emission: bn_last, FORK, projection, ENDFORK, ..., bn1, JOIN, conv1.
                // The forward launch order is untouched.
                static const bool no_reorder = getenv("AWR_NO_DS_REORDER") != nullptr;      // same-box A/B hooks
                static const bool no_branch = getenv("AWR_NO_DS_BRANCH") != nullptr;
                if (P.training && n1 > n0 && !no_reorder) {
                    std::vector<std::function<int()>> ds(nodes.begin() + n0, nodes.begin() + n1), mn(nodes.begin() + n1, nodes.end());
                    std::vector<std::function<int()>> order;
                    order.push_back(mn.front());                                   // conv1 (its data gradient: last producer of d(c))
                    if (!no_branch) order.push_back(b.bwd_marker(OP_JOIN, 0));
                    for (size_t i = 1; i + 1 < mn.size(); ++i) order.push_back(mn[i]);
                    if (!no_branch) order.push_back(b.bwd_marker(OP_ENDFORK, 0));
                    for (auto& f : ds) order.push_back(f);
                    if (!no_branch) order.push_back(b.bwd_marker(OP_FORK, 0));
                    order.push_back(mn.back());                                    // the block output's BatchNorm
                    nodes.erase(nodes.begin() + n0, nodes.end());
                    for (auto& f : order) nodes.push_back(f);
                }
            }
        for (int i = 0; i < N.ndeconv; ++i)   // feeds the next transposed conv (K = 4 x 256 per phase: materialised) or the 1x1 head GEMM (lazy)
            c = cbr(c, fmt("deconv_layers.%d", 3 * i), fmt("deconv_layers.%d", 3 * i + 1), true, nullptr, i == N.ndeconv - 1);
        Tn* pred = b.conv(c, C("head"));
        b.head_out(pred, N.J, out, gout);
    }

    DualLayer* dual_for(const std::string& p) {
        // conv3 + skip_layer as one launch: FP32-MFMA mode only (the split-operand kernels take one input tensor)
        static const bool no_dual = getenv("AWR_NO_DUAL") != nullptr;      // bisecting hook (tools/diag_parity.py)
        if (no_dual || awr_get_gemm_products() != 1 || !N.convs.count(p + ".skip_layer")) return nullptr;
        DualLayer& d = N.duals[p];
        if (!d.c3) {
            d.c3 = C(p + ".conv3");
            d.sk = C(p + ".skip_layer");
            d.name = p + ".conv3+skip_layer";
        }
        return &d;
    }

    Tn* residual(Tn* x, const std::string& p) {
        ConvLayer* skip = N.convs.count(p + ".skip_layer") ? C(p + ".skip_layer") : nullptr;
        DualLayer* dual = dual_for(p);
        ConvOpt o;
        if (P.training) {
            // the three pre-activations feed exactly one conv each: never written to HBM
            Tn* a = b.bn_act(x, BN(p + ".bn1"), true, nullptr, true);
            o.want_stats = true;
            // (bn2's output feeds the 3x3 conv2, whose nine taps each re-apply the loader arithmetic; writing it out instead puts conv2's
            // forward on the pure-DMA GEMM and its weight gradient on the kernel-row kernel -- re-measured in round 4 with those kernels:
            // Hourglass-1 23.19-23.34 vs 23.12-23.23 ms, config 5 281.1 vs 279.4 ms and +10.7 GB of plan: still not worth the pass.
            // AWR_HG_WRITE_BN2=1 is the A/B hook; profiles/r04_hg_materialised_bn2.txt)
            static const bool write_bn2 = getenv("AWR_HG_WRITE_BN2") != nullptr;
            a = b.bn_act(b.conv(a, C(p + ".conv1"), o), BN(p + ".bn2"), true, nullptr, !write_bn2);
            a = b.bn_act(b.conv(a, C(p + ".conv2"), o), BN(p + ".bn3"), true, nullptr, true);
            if (dual) return b.conv_dual(a, x, dual, true);
            Tn* r = skip ? b.conv(x, skip) : x;
            o.res = r;
            return b.conv(a, C(p + ".conv3"), o);
        }
        // inference: bn1 stays a loader affine (x also feeds the skip path un-normalised); bn2 / bn3 + ReLU normalise tensors that only
        // conv2 / conv3 read, so they fold into the EPILOGUE of the conv that produces them
        auto s1 = b.fold_bn(BN(p + ".bn1")), s2 = b.fold_bn(BN(p + ".bn2")), s3 = b.fold_bn(BN(p + ".bn3"));
        o.in_scale = s1.first; o.in_shift = s1.second; o.relu_in = true;
        o.out_scale = s2.first; o.out_shift = s2.second; o.relu_out = true;
        Tn* y = b.conv(x, C(p + ".conv1"), o);
        ConvOpt o2;
        o2.out_scale = s3.first; o2.out_shift = s3.second; o2.relu_out = true;
        // conv2 and conv3 (+ the skip conv, as extra K of the second GEMM) in one launch when the batch fills the chip -- unless the Winograd mode takes
        // conv2 (2.25x fewer multiplies beat the saved round trip of its output: profiles/r06_winograd.txt)
        if (b.wino_fwd_ok(C(p + ".conv2")->spec, y->B, y->H, y->W)) {
        } else if (dual) {
            if (Tn* fused = b.conv_pair(y, C(p + ".conv2"), o2, nullptr, nullptr, dual, x)) return fused;
        } else if (!skip) {
            if (Tn* fused = b.conv_pair(y, C(p + ".conv2"), o2, C(p + ".conv3"), x)) return fused;
        }
        y = b.conv(y, C(p + ".conv2"), o2);
        if (dual) return b.conv_dual(y, x, dual, false);
        Tn* r = skip ? b.conv(x, skip) : x;
        ConvOpt o3;
        o3.res = r;
        return b.conv(y, C(p + ".conv3"), o3);
    }

    Tn* hg(Tn* x, const std::string& p, int depth) {
        // the skip branch of a level only meets the low-resolution path again at the up-sampling add: issued on its own side
        // stream, its full-resolution GEMMs fill the chip while the main stream walks the small (<= 16x16) levels
        const size_t n0 = nodes.size();
        b.fork(depth);
        Tn* up1 = residual(x, p + ".up1");
        b.end_fork(up1);
        const size_t n1 = nodes.size();
        Tn* pooled = b.maxpool(x, 2, 2, 0);
        // backward branches for the two outer levels only (64x64 / 32x32 skip residuals): one stream each, no false dependencies
        // (measured: branches for the inner levels too change nothing, 25.7 ms either way vs 26.8-27.3 without any)
        const bool bwd_branch = P.training && depth >= 3;
        if (bwd_branch) b.bwd_marker_node(OP_JOIN, depth);      // emitted right before maxpool's backward: d(x) += ... waits for the branch
        Tn* low = residual(pooled, p + ".low1");
        low = depth > 1 ? hg(low, p + ".low2", depth - 1) : residual(low, p + ".low2");
        low = residual(low, p + ".low3");
        if (bwd_branch) {
            // Backward of the level: d(out) feeds the up1 residual (large full-resolution GEMMs) and, through the up-sampling, the
            // whole low-resolution path (hundreds of small launches): independent until both add into d(x).  The up1 emitters are
            // moved behind the low path's, i.e. emitted FIRST and bracketed by fork / end-fork markers: up1's backward is the
            // first writer of d(x) on a branch stream, the low path runs beside it on the main stream, and the join above orders
            // the max-pool backward's accumulation into d(x) after the branch.  (d(out) itself is read by the up-sampling backward
            // BEFORE the fork and may be accumulated into in place by the branch afterwards: the identity skip aliases it.)
            std::rotate(nodes.begin() + n0, nodes.begin() + n1, nodes.end());
            const size_t nlow = nodes.size() - (n1 - n0);       // up1's emitters now start here
            nodes.insert(nodes.begin() + nlow, b.bwd_marker(OP_ENDFORK, depth));      // emitted after up1's backward
            b.bwd_marker_node(OP_FORK, depth);                    // emitted right after the up-sampling add's backward
        }
        return b.upsample_add(up1, low);
    }

    void hourglass(float* img, int H, float* const* outs, float* const* gouts) {
        Tn* c = b.stem(img, C("pre.0"), BN("pre.0.bn"), H, H, false);      // conv 5x5 + bias -> BN -> ReLU at full resolution
        c = residual(c, "pre.1");
        c = b.maxpool(c, 2, 2, 0);
        c = residual(c, "pre.3");
        c = residual(c, "pre.4");
        for (int i = 0; i < N.nstack; ++i) {
            Tn* h = hg(c, fmt("hgs.%d.0", i), 4);
            Tn* ft = residual(h, fmt("features.%d.0", i));
            ft = cbr(ft, fmt("features.%d.1", i), fmt("features.%d.1.bn", i), true, nullptr, true);      // head / merge GEMMs
            Tn* pred = b.conv(ft, C(fmt("head.%d", i)));
            b.head_out(pred, N.J, outs[i], gouts ? gouts[i] : nullptr);
            if (i < N.nstack - 1) {
                ConvOpt o;
                o.res = c;
                Tn* m = b.conv(pred, C(fmt("merge_preds.%d.conv", i)), o);
                ConvOpt o2;
                o2.res = m;
                o2.want_stats = true;
                c = b.conv(ft, C(fmt("merge_features.%d.conv", i)), o2);
            }
        }
    }
};

}  // namespace awrnet

extern "C" {

int awr_plan_create(awr_net* n, int B, int H, int training, unsigned supervised_mask, int bn_repeat, int n_buckets, float* img, float* const* outs,
                    float* const* grad_outs, awr_plan** out) {
    return awr_plan_create_modes(n, B, H, training, supervised_mask, bn_repeat, n_buckets, img, outs, grad_outs, nullptr, out);
}

int awr_plan_create_modes(awr_net* n, int B, int H, int training, unsigned supervised_mask, int bn_repeat, int n_buckets, float* img, float* const* outs,
                          float* const* grad_outs, const awr_plan_modes* modes, awr_plan** out) {
    awr_plan_modes m;
    if (modes) {
        m = *modes;
    } else {      // the process-wide modes (awr_set_gemm_accum[_auto], awr_set_conv_winograd, awr_set_train_split_k)
        m.accum = awr_get_gemm_accum();
        awr_get_gemm_accum_auto(&m.accum_auto_k, &m.accum_auto_dgrad);
        m.winograd = awr_get_conv_winograd();
        m.train_split_k = awr_get_train_split_k();
    }
    if (int e = awr::check_gemm_accum(m.accum)) return e;
    if (m.accum == 2)
        if (int e = awr::check_gemm_accum_auto(m.accum_auto_k)) return e;
    if (int e = awr::check_conv_winograd(m.winograd)) return e;
    if (int e = awr::check_train_split_k(m.train_split_k)) return e;
    AWR_REQUIRE(n && out && img && outs, "plan_create: null pointer");
    AWR_REQUIRE(n->params, "plan_create: bind the parameter arenas first (awr_net_bind)");
    AWR_REQUIRE(B >= 1 && H >= 16 && H % 16 == 0, "plan_create: B=%d, H=%d (multiples of 16)", B, H);
    AWR_REQUIRE(!training || grad_outs, "plan_create: a training plan needs the gradient inputs");
    AWR_REQUIRE(bn_repeat >= 1 && n_buckets >= 1, "plan_create: bn_repeat / n_buckets must be >= 1");
    awr_plan* p = new awr_plan();
    p->net = n;
    p->B = B;
    p->H = H;
    p->training = training != 0;
    p->det = awr_get_deterministic() != 0;
    p->modes = m;
    p->bn_repeat = bn_repeat;
    p->n_buckets = n_buckets;
    p->supervised = supervised_mask;
    p->img = img;
    Builder bld(*p);
    NetBuilder nb(bld);
    if (n->kind == 0) nb.resnet(img, H, outs[0], grad_outs ? grad_outs[0] : nullptr);
    else nb.hourglass(img, H, outs, grad_outs);
    int rc = bld.err;
    if (!rc && p->training) rc = build_backward(bld);
    if (!rc) rc = bld.err;
    if (rc) {
        destroy_plan(p);
        return rc;
    }
    n->plans.push_back(p);
    *out = p;
    return AWR_OK;
}

}  // extern "C"
