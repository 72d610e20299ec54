// Network-level engine of libawr_hip.so (include/awr_hip.h, "Network-level API"), using a plan: the weight refresh, the replay of a launch
// list over the library's streams, the timed replay, the tuner, the process-wide stream pool, the hook-up of a data-parallel communicator
// (csrc/awr_dp.hip) and every awr_plan_* entry point but awr_plan_create[_modes] (csrc/awr_plan_build.hip).  Replaying a list allocates
// nothing and never synchronises the host: a whole step can be captured in one hipGraph.  Host code but for the stream pool's probe
// (spin_kernel): it calls the operator-level entry points of this library and the HIP runtime for memory, streams and events.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include "awr_plan.h"

extern "C" unsigned long long awr_dp_generation(const awr_dp* d);      // csrc/awr_dp.hip: generation of a communicator that has not been destroyed, else 0

using namespace awrnet;

namespace awrnet {

int upload_table(awr_plan& P, const void* host, size_t bytes, void** dev) {
    void* p = nullptr;
    NET_CHECK(dev_alloc(P.owned, bytes, false, &p));
    HIP_TRY(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
    *dev = p;
    return AWR_OK;
}

// ---- replay ----------------------------------------------------------------------------------------------------
// Re-pack every conv weight (and re-fold eval BNs) from the parameter arena: one batched launch for the plain layers, a few
// extra calls for the fused heads.
static int refresh_weights(awr_plan& P, void* stream) {
    const int ws = awr_get_gemm_products() != 1 ? 1 : 0;      // split images are only written for the mode that reads them
    if (!P.pack_built[ws]) {
        std::vector<awr_pack_job> jobs[2];
        int64_t total[2] = {0, 0};
        for (auto* l : P.layers) {
            if (l->head) continue;
            const PackRecipe rc[2] = {fwd_pack(l->spec), dgrad_pack(l->spec)};
            Packed* dst[2] = {&l->p_fwd, &l->p_dgrad};
            for (int k = 0; k < 2; ++k) {
                if (!dst[k]->p) continue;
                awr_pack_job j;
                memset(&j, 0, sizeof j);
                j.src = l->w; j.dst = dst[k]->p; j.split = ws ? dst[k]->split : nullptr;
                j.d0 = rc[k].d0; j.d1 = rc[k].d1; j.T = rc[k].T; j.transpose = rc[k].transpose; j.rows = rc[k].rows; j.ld = rc[k].ld;
                j.first = total[k];
                total[k] += rc[k].rows;
                jobs[k].push_back(j);
            }
        }
        for (auto* d : P.dual_layers) {       // [W3 row | Wskip row] side by side in one K-contiguous buffer (FP32 mode only: no split image)
            const int cin1 = d->c3->spec.cin_pad, cin2 = d->sk->spec.cin_pad;
            const ConvLayer* src[2] = {d->c3, d->sk};
            const int colsv[2] = {cin1, cin2}, offs[2] = {0, cin1};
            for (int k = 0; k < 2; ++k) {
                awr_pack_job j;
                memset(&j, 0, sizeof j);
                j.src = src[k]->w; j.dst = d->p.p + offs[k]; j.split = nullptr;
                j.d0 = src[k]->spec.cout; j.d1 = src[k]->spec.cin; j.T = 1; j.transpose = 0; j.rows = d->p.rows; j.ld = d->p.ld; j.cols = colsv[k];
                j.first = total[0];
                total[0] += d->p.rows;
                jobs[0].push_back(j);
            }
        }
        for (int k = 0; k < 2; ++k) {
            if (!jobs[k].empty()) NET_CHECK(upload_table(P, jobs[k].data(), jobs[k].size() * sizeof(awr_pack_job), &P.pack_tab[ws][k]));
            P.pack_njobs[ws][k] = (int)jobs[k].size();
            P.pack_rows[ws][k] = total[k];
        }
        P.pack_built[ws] = true;
    }
    if (P.pack_njobs[ws][0])
        NET_CHECK(awr_pack_weights_batched((const awr_pack_job*)P.pack_tab[ws][0], P.pack_njobs[ws][0], P.pack_rows[ws][0], stream));
    // (packing the data-gradient layouts on a side stream under the forward's GEMMs was measured in rounds 2 and 3: no gain, 14.04 vs
    // 14.04 ms -- profiles/r03_summary.md -- so both tables go to the caller's stream)
    if (P.pack_njobs[ws][1])
        NET_CHECK(awr_pack_weights_batched((const awr_pack_job*)P.pack_tab[ws][1], P.pack_njobs[ws][1], P.pack_rows[ws][1], stream));
    for (auto& wl : P.wino)
        NET_CHECK(awr_wino_weights(wl.first->w, wl.first->spec.cout, wl.first->spec.cin, wl.first->spec.cout_pad, wl.first->spec.cin_pad, 0, wl.second, stream));
    for (auto& wl : P.wino_d)        // data-gradient form: output channels = the layer's Cin, contraction over its Cout, taps mirrored
        NET_CHECK(awr_wino_weights(wl.first->w, wl.first->spec.cin, wl.first->spec.cout, wl.first->spec.cin_pad, wl.first->spec.cout_pad, 1, wl.second, stream));
    hipStream_t st = awr::as_stream(stream);
    for (auto* l : P.layers) {
        if (!l->head) continue;
        const int J = l->J, cin = l->spec.cin, rows = l->p_fwd.rows;
        NET_CHECK(awr_pack_weight(l->w1, 3 * J, cin, 1, 0, 3 * J, cin, l->p_fwd.p, stream));
        NET_CHECK(awr_pack_weight(l->w2, J, cin, 1, 0, rows - 3 * J, cin, l->p_fwd.p + (int64_t)3 * J * cin, stream));
        if (l->p_dgrad.p)    // P[cin][1][cp]: columns [0,3J) from w1, [3J,4J) from w2 = the transpose of the forward pack
            NET_CHECK(awr_pack_weight(l->p_fwd.p, l->cp, cin, 1, 1, l->p_dgrad.rows, l->cp, l->p_dgrad.p, stream));
        if (ws) {
            NET_CHECK(awr_split_weight(l->p_fwd.p, l->p_fwd.split, l->p_fwd.numel(), stream));
            if (l->p_dgrad.p) NET_CHECK(awr_split_weight(l->p_dgrad.p, l->p_dgrad.split, l->p_dgrad.numel(), stream));
        }
        HIP_TRY(hipMemcpyAsync(l->bias_cat, l->b1, (size_t)3 * J * 4, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(l->bias_cat + 3 * J, l->b2, (size_t)J * 4, hipMemcpyDeviceToDevice, st));
    }
    for (auto* d : P.dual_layers) NET_CHECK(awr_add(d->c3->bias, d->sk->bias, d->bias_sum, d->c3->spec.cout, stream));
    for (auto& op : P.pack_ops) NET_CHECK(op.fn(stream));
    return AWR_OK;
}

// the next event of the plan's pool, which grows up to 2048 events (large enough that an event is never re-recorded within one pass: hundreds of
// waits per Hourglass backward) and is cycled through from then on
static int next_event(awr_plan& P, hipEvent_t* out) {
    if (P.events.size() < 2048) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        P.events.push_back(e);
    }
    *out = P.events[P.ev_next++ % P.events.size()];
    return AWR_OK;
}

// waiter waits for everything enqueued on signaler so far (capturable: event record + stream wait)
static int stream_wait(awr_plan& P, hipStream_t waiter, hipStream_t signaler) {
    hipEvent_t e;
    NET_CHECK(next_event(P, &e));
    HIP_TRY(hipEventRecord(e, signaler));
    HIP_TRY(hipStreamWaitEvent(waiter, e, 0));
    return AWR_OK;
}

// Replays one op list on `stream`.  Backward: weight-gradient GEMMs that qualify are issued round-robin on the side streams and
// run concurrently with the data-gradient chain (two DIFFERENT kernels co-resident on a CU are never in lock-step: each fills
// the other's prologue / epilogue / barrier bubbles); with a bucket callback, a bucket's scatter and its collective go to the
// comm stream so the main stream never waits for the side streams in the middle of the backward.  Forward: fork / join
// pseudo-ops route independent branches to the side streams.
static int run_list(awr_plan& P, std::vector<Op>& ops, void* stream, bool is_bwd) {
    hipStream_t main = awr::as_stream(stream);
    const bool use_side = !P.side.empty();
    const bool wside = is_bwd && use_side;
    // (no callback needed: a single-GPU plan built with several buckets uses the hand-off just to scatter its weight gradients early,
    // off the tail of the step)
    hipStream_t comm = (wside && P.n_buckets > 1) ? P.comm : nullptr;
    bool pending = false, handed = false;
    size_t nside = 0;
    void* cur = stream;
    bool after_join = false;
    hipEvent_t half_ev = nullptr;      // "half B of the last split BatchNorm-backward apply is written" (OP_HALFWAIT)
    auto hand_off = [&]() -> int {       // everything the bucket needs (main chain so far + weight gradients) -> comm stream
        NET_CHECK(stream_wait(P, comm, main));
        for (auto st : P.side)
            if (st != comm) NET_CHECK(stream_wait(P, comm, st));
        for (auto st : P.branch) NET_CHECK(stream_wait(P, comm, st));
        return AWR_OK;
    };
    for (auto& op : ops) {
        if (op.boundary && P.nhwc_boundary) continue;
        if (comm && op.kind == OP_CALL && op.scatter) {
            NET_CHECK(hand_off());
            handed = true;
            NET_CHECK(op.fn((void*)comm));
            continue;
        }
        if (comm && op.kind == OP_BUCKET) {
            if (!handed) NET_CHECK(hand_off());
            handed = false;
            if (P.bucket_cb) P.bucket_cb(P.bucket_user, op.lo, op.hi, (void*)comm);
            continue;
        }
        if (wside && pending && (op.kind == OP_CALL || op.kind == OP_BUCKET) && op.joins) {
            // join before anything that consumes the weight-gradient scratch (scatter, buckets)
            for (auto st : P.side) NET_CHECK(stream_wait(P, main, st));
            for (auto st : P.branch) NET_CHECK(stream_wait(P, main, st));
            pending = false;
            after_join = true;      // ... and issue it on MAIN: inside an open fork region `cur` is a branch stream that did not wait
        }
        switch (op.kind) {
            case OP_ZERO:      // (on the issuing chain: a zero fill inside a branch belongs to the branch's data gradient)
                HIP_TRY(hipMemsetAsync(op.p, 0, op.bytes, awr::as_stream(cur)));
                continue;
            case OP_COPY:
                HIP_TRY(hipMemcpyAsync(op.p, op.q, op.bytes, hipMemcpyDeviceToDevice, awr::as_stream(cur)));
                continue;
            case OP_BUCKET:
                if (P.bucket_cb) P.bucket_cb(P.bucket_user, op.lo, op.hi, stream);
                continue;
            case OP_FORK:
                if (use_side) {
                    hipStream_t st = is_bwd ? P.branch[op.sid % P.branch.size()] : P.side[op.sid % P.side.size()];
                    NET_CHECK(stream_wait(P, st, main));
                    cur = (void*)st;
                    if (is_bwd) pending = true;      // the end-of-list join has to cover the branch streams
                }
                continue;
            case OP_ENDFORK:
                cur = stream;
                continue;
            case OP_JOIN:
                if (use_side) NET_CHECK(stream_wait(P, main, is_bwd ? P.branch[op.sid % P.branch.size()] : P.side[op.sid % P.side.size()]));
                continue;
            case OP_HALFWAIT:      // the second half of a BatchNorm-backward apply went to a side stream: its record, not the stream's tail
                if (half_ev) {
                    HIP_TRY(hipStreamWaitEvent(awr::as_stream(cur), half_ev, 0));
                    half_ev = nullptr;
                }
                continue;
            default:
                break;
        }
        int rc;
        if (wside && op.side_ok) {
            hipStream_t st = P.side[nside % P.side.size()];
            if (!op.pair_next) ++nside;
            // (issued BESIDE its layer's data gradient; behind it -- i.e. beside the memory-bound BatchNorm-backward passes that follow -- was re-measured in
            // round 4 with the LDS-DMA kernels: ResNet18 12.8 -> 13.9-14.0 ms, Hourglass-1 23.5 -> 23.9 ms, profiles/r04_wgrad_late.txt)
            NET_CHECK(stream_wait(P, st, awr::as_stream(cur)));      // its operands (dY, x) are final at this point of the issuing chain
            rc = op.fn((void*)st);
            pending = true;
            if (op.half_sig && rc == AWR_OK) {
                NET_CHECK(next_event(P, &half_ev));
                HIP_TRY(hipEventRecord(half_ev, st));
            }
        } else {
            rc = op.fn(after_join ? stream : cur);
        }
        after_join = false;
        if (rc) return rc;
    }
    if (wside && (pending || comm)) {
        for (auto st : P.side) NET_CHECK(stream_wait(P, main, st));
        for (auto st : P.branch) NET_CHECK(stream_wait(P, main, st));
        if (comm) NET_CHECK(stream_wait(P, main, comm));      // next step's scratch fill / optimiser must see the scatters
    }
    if (is_bwd && P.dp && !P.dp_error && awr_dp_generation(P.dp) != P.dp_gen) {
        P.dp = nullptr;
        P.dp_lost = true;
    }
    if (is_bwd && P.dp_lost) {      // sticky: replicas that skipped an exchange have diverged -- no later backward may report success
        P.dp_error = 0;
        set_error("plan: the data-parallel communicator attached with awr_plan_set_dp has been destroyed (detach it with awr_plan_set_dp(plan, NULL) first); "
                  "gradients were NOT exchanged -- attach a communicator (or NULL) with awr_plan_set_dp to continue");
        return AWR_ERR_ARG;
    }
    if (is_bwd && P.dp && P.n_buckets <= 1 && !P.dp_error)        // a one-bucket plan has no markers: one exchange after the backward
        P.dp_error = awr_dp_allreduce(P.dp, P.net->grads, P.net->layout.n_active, stream);
    if (is_bwd && P.dp) NET_CHECK(awr_dp_wait(P.dp, stream));      // ... and the reduced gradients
    if (is_bwd && P.dp_error) {
        const int e = P.dp_error;
        P.dp_error = 0;
        return e;
    }
    return AWR_OK;
}

// serial replay with a HIP-event pair around every conv / stem launch: ms[i] per op of the list (0 for the others)
static int run_timed(awr_plan& P, std::vector<Op>& ops, void* stream, float* ms) {
    hipStream_t main = awr::as_stream(stream);
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev(ops.size(), {nullptr, nullptr});
    int rc = AWR_OK;
    for (size_t i = 0; i < ops.size() && rc == AWR_OK; ++i) {
        Op& op = ops[i];
        if (op.kind == OP_ZERO) { if (hipMemsetAsync(op.p, 0, op.bytes, main) != hipSuccess) rc = AWR_ERR_HIP; continue; }
        if (op.kind == OP_COPY) { if (hipMemcpyAsync(op.p, op.q, op.bytes, hipMemcpyDeviceToDevice, main) != hipSuccess) rc = AWR_ERR_HIP; continue; }
        if (op.kind != OP_CALL || (op.boundary && P.nhwc_boundary)) continue;
        // (every launch gets its event pair; callers that only want the GEMM family filter by the op flags)
        (void)hipEventCreate(&ev[i].first);
        (void)hipEventCreate(&ev[i].second);
        (void)hipEventRecord(ev[i].first, main);
        rc = op.fn(stream);
        (void)hipEventRecord(ev[i].second, main);
    }
    if (hipStreamSynchronize(main) != hipSuccess && rc == AWR_OK) {
        set_error("run_timed: hipStreamSynchronize failed");
        rc = AWR_ERR_HIP;
    }
    for (size_t i = 0; i < ops.size(); ++i) {
        ms[i] = 0.f;
        if (ev[i].first) {
            if (rc == AWR_OK) (void)hipEventElapsedTime(&ms[i], ev[i].first, ev[i].second);
            (void)hipEventDestroy(ev[i].first);
            (void)hipEventDestroy(ev[i].second);
        }
    }
    return rc;
}

// Pick the fastest workgroup tile (and split-K depth) for every GEMM launch of this static plan by timing the candidates in
// place with HIP events.  Runs right after a first replay (buffers hold real data; the next step rebuilds whatever the tuner
// scribbles on) and re-zeroes every atomic accumulator the launches touched.
static int autotune(awr_plan& P, int reps, void* stream) {
    if (P.det) return AWR_OK;      // a timing-dependent tile / split-K choice would change summation orders from run to run
    hipStream_t main = awr::as_stream(stream);
    NET_CHECK(refresh_weights(P, stream));
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    auto launch = [&](GemmRef& g) { return g.ca ? awr_conv_gemm(g.ca, stream) : awr_conv_wgrad(g.wa, stream); };
    int rc = AWR_OK;
    for (auto& g : P.gemms) {
        if (g.ca && g.ca->w2) continue;             // the fused conv pair has one geometry
        struct Cand { int tm, tn, tb, algo = 0; };
        std::vector<Cand> cands;
        if (g.wa && g.wa->algo == 2) {
            // The wave-per-tap kernel has one geometry and stays.  AWR_TUNE_TAPS=1 (study hook) times it against the kernel-row kernel's split-K
            // depths: isolated, the row kernel with its in-LDS BatchNorm loader wins on these layers (127 vs 122.5 TF) and the tuner takes it --
            // and the Hourglass-1 step gets 0.3 ms SLOWER (23.6 -> 23.9 ms, three interleaved repetitions, profiles/r04_loop_exits.txt): a
            // weight gradient is a side-stream kernel, what counts is how it shares the CUs with the data-gradient chain it runs beside, and
            // 256 twelve-wave workgroups share better than 768-1280 four-wave ones that can fill every SIMD's register file.
            static const bool tune_taps = getenv("AWR_TUNE_TAPS") != nullptr;
            if (!tune_taps || !awr_conv_wgrad_algo_ok(g.wa, 3)) continue;
            cands = {{1, 1, 0, 2}};
            for (int tb : {768, 1024, 1280, 1536, 2048}) cands.push_back({1, 1, tb, 3});
        } else if (g.ca) {
            cands = {{1, 1, 0}, {2, 1, 0}};
            if (g.ca->N > 64) { cands.push_back({1, 2, 0}); cands.push_back({2, 2, 0}); }
            if (g.ca->pool_out)      // a launch that carries a max-pool: only tiles whose 2D patch (32 tile_m columns) divides the map's width
                cands.erase(std::remove_if(cands.begin(), cands.end(), [&](const Cand& c) { return g.ca->Wq % (32 * c.tm) != 0; }), cands.end());
            if (g.ca->partial && g.ca->split_max > 1 && awr_get_gemm_products() == 1) {      // (tile, split-K depth) pairs; tb = depth
                std::vector<Cand> withk;
                const int minsteps = min_k_steps(*g.ca);
                for (auto& c : cands)
                    for (int sk = 1; sk <= g.ca->split_max; sk *= 2) {
                        // blocked accumulation: only depths the accumulation rule admits (a whole 128-k block per K range, awr_hip.h)
                        if (sk > 1 && g.ca->accum == 1 && (minsteps + sk - 1) / sk < 4) continue;
                        withk.push_back({c.tm, c.tn, sk});
                    }
                cands.swap(withk);
            }
        } else {
            cands = {{1, 1, 2048}, {1, 1, 3072}, {1, 1, 4096}};
            if (g.wa->Cd > 64) { cands.push_back({2, 1, 1536}); cands.push_back({2, 1, 2048}); }
            if (g.wa->Cg > 64) cands.push_back({1, 2, 2048});
            if (g.wa->Cd > 64 && g.wa->Cg > 64 && awr_get_wgrad_products() != 1) { cands.push_back({2, 2, 1024}); cands.push_back({2, 2, 2048}); }
            // one workgroup per kernel row (3x3 stride 1): its own split-K depths; the per-tap candidates above then run as algo 1
            if ((g.wa->algo == 0 || g.wa->algo == 3) && awr_conv_wgrad_algo_ok(g.wa, 3)) {
                for (auto& c : cands) c.algo = 1;
                for (int tb : {768, 1024, 1280, 1536, 2048}) cands.push_back({1, 1, tb, 3});
            }
        }
        float best_t = 1e30f;
        Cand best = cands[0];
        for (auto& c : cands) {
            if (g.ca) { g.ca->tile_m = c.tm; g.ca->tile_n = c.tn; if (c.tb) g.ca->split_k = c.tb; }
            else { g.wa->tile_m = c.tm; g.wa->tile_n = c.tn; g.wa->target_blocks = c.tb; if (c.algo) g.wa->algo = c.algo; }
            if ((rc = launch(g))) break;      // warm-up
            (void)hipEventRecord(e0, main);
            for (int r = 0; r < reps && rc == AWR_OK; ++r) rc = launch(g);
            (void)hipEventRecord(e1, main);
            (void)hipEventSynchronize(e1);
            float t = 0.f;
            (void)hipEventElapsedTime(&t, e0, e1);
            t /= (float)reps;
            if (t < best_t) { best_t = t; best = c; }
        }
        if (rc) break;
        if (g.ca) { g.ca->tile_m = best.tm; g.ca->tile_n = best.tn; if (best.tb) g.ca->split_k = best.tb; }
        else { g.wa->tile_m = best.tm; g.wa->tile_n = best.tn; g.wa->target_blocks = best.tb; if (best.algo) g.wa->algo = best.algo; }
        g.tm = best.tm; g.tn = best.tn; g.tb = best.tb; g.us = best_t * 1e3f; g.tuned = true;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    for (auto& z : P.zero_init) HIP_TRY(hipMemsetAsync(z.first, 0, z.second, main));
    if (P.scratch) HIP_TRY(hipMemsetAsync(P.scratch, 0, (size_t)P.scratch_cap * 4, main));
    HIP_TRY(hipStreamSynchronize(main));
    return AWR_OK;
}

void destroy_plan(awr_plan* p) {
    for (auto e : p->events) (void)hipEventDestroy(e);
    if (p->comm && p->comm_owned) (void)hipStreamDestroy(p->comm);      // (side / branch streams belong to the process-wide pool)
    free_all(p->owned);
    delete p;
}

}  // namespace awrnet

extern "C" {

int awr_plan_destroy(awr_plan* p) {
    if (!p) return AWR_OK;
    auto& v = p->net->plans;
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i] == p) {
            v.erase(v.begin() + i);
            break;
        }
    destroy_plan(p);
    return AWR_OK;
}

int awr_plan_info(const awr_plan* p, int64_t* bytes, int* deterministic, int* n_fwd, int* n_bwd, int* n_buckets, int* n_gemm, int* n_bn) {
    AWR_REQUIRE(p, "plan_info: null pointer");
    if (bytes) *bytes = p->bytes;
    if (deterministic) *deterministic = p->det ? 1 : 0;
    if (n_fwd) *n_fwd = (int)p->fwd.size();
    if (n_bwd) *n_bwd = (int)p->bwd.size();
    if (n_buckets) *n_buckets = (int)p->buckets.size();
    if (n_gemm) *n_gemm = (int)p->gemms.size();
    if (n_bn) {
        int c = 0;
        for (auto& o : p->fwd) c += o.name == "awr_bn_finalize";
        *n_bn = c;
    }
    return AWR_OK;
}

int awr_plan_winograd(const awr_plan* p, int* n, double* macs) {
    AWR_REQUIRE(p, "plan_winograd: null pointer");
    int nd = 0;
    double md = 0;
    for (auto& c : p->wino_dg)
        if (awr_wino_dgrad_supported(c.first)) { ++nd; md += c.second; }
    if (n) *n = p->n_wino + nd;
    if (macs) *macs = p->wino_macs + md;
    return AWR_OK;
}

int awr_plan_bucket(const awr_plan* p, int i, int64_t* lo, int64_t* hi, int* ready_op) {
    AWR_REQUIRE(p && i >= 0 && i < (int)p->buckets.size(), "plan_bucket: index out of range");
    if (lo) *lo = p->buckets[i].lo;
    if (hi) *hi = p->buckets[i].hi;
    if (ready_op) *ready_op = p->buckets[i].ready;
    return AWR_OK;
}

int awr_plan_head_nhwc(const awr_plan* p, int stage, const float** pred, float** grad, int* Cp) {
    AWR_REQUIRE(p && stage >= 0 && stage < (int)p->head_preds.size(), "plan_head_nhwc: stage out of range");
    if (pred) *pred = p->head_preds[stage]->buf;
    if (grad) *grad = p->head_grads[stage];
    if (Cp) *Cp = p->head_preds[stage]->C;
    return AWR_OK;
}

int awr_plan_set_nhwc_boundary(awr_plan* p, int on) {
    AWR_REQUIRE(p, "plan_set_nhwc_boundary: null pointer");
    if (on && p->net->J > 56) {      // Cp = 4J rounded up to 32 > 224: the NHWC head kernels' LDS tile would exceed 64 KB (awr_head.hip: nhwc_geometry)
        set_error("plan_set_nhwc_boundary: the NHWC head / loss kernels serve at most 56 joints (got %d): use the NCHW boundary", p->net->J);
        return AWR_ERR_UNSUPPORTED;
    }
    if (on && p->training) {
        for (size_t s = 0; s < p->head_grads.size(); ++s)
            if ((p->supervised & (1u << s)) && !p->head_grads[s]) {
                set_error("plan_set_nhwc_boundary: the gradient of stage %d has a second producer inside the network (a later stack reads the prediction): "
                          "it has to be accumulated through grad_outs", (int)s);
                return AWR_ERR_UNSUPPORTED;
            }
    }
    p->nhwc_boundary = on != 0;
    return AWR_OK;
}

int awr_plan_tensor(const awr_plan* p, int i, const char** name, int dims[4], float** buf, float** grad, int* lazy, const float** lz_scale,
                    const float** lz_shift) {
    AWR_REQUIRE(p, "plan_tensor: null pointer");
    if (i < 0 || i >= (int)p->tensors.size()) return AWR_ERR_ARG;      // (no error string: callers iterate until this)
    const Tn& t = p->tensors[i];
    if (name) *name = t.name.c_str();
    if (dims) { dims[0] = t.B; dims[1] = t.H; dims[2] = t.W; dims[3] = t.C; }
    if (buf) *buf = t.buf;
    if (grad) *grad = t.grad;
    if (lazy) *lazy = t.lazy ? (t.lz_relu ? 2 : 1) : 0;
    if (lz_scale) *lz_scale = t.lz_scale;
    if (lz_shift) *lz_shift = t.lz_shift;
    return AWR_OK;
}

int awr_plan_op(const awr_plan* p, int list, int i, const char** name, double* macs, int* flags) {
    AWR_REQUIRE(p && (list == 0 || list == 1), "plan_op: list must be 0 (forward) or 1 (backward)");
    const auto& v = list ? p->bwd : p->fwd;
    AWR_REQUIRE(i >= 0 && i < (int)v.size(), "plan_op: index out of range");
    if (name) *name = v[i].name.c_str();
    if (macs) *macs = v[i].macs;
    if (flags) *flags = (v[i].side_ok ? 1 : 0) | (v[i].gemm ? 2 : 0) | (v[i].scatter ? 4 : 0) | (v[i].joins ? 8 : 0);
    return AWR_OK;
}

}  // extern "C"

// ---- library streams --------------------------------------------------------------------------------------------------------
// HIP multiplexes streams onto a few hardware queues (4 by default); two streams on one queue run their kernels one after the other,
// and which streams share depends on how many streams the process created before (a communication library's, the framework's).
// Side streams only help when they sit on a queue of their own, so the library keeps ONE process-wide pool and orders it by a probe:
// a 100 us spin kernel on two streams at once takes 100 us when they are independent, 200 us when they share a queue.  pool[0..k) are
// mutually independent and independent of the null stream; the rest follow.  Plans borrow from the pool (never destroy).
namespace awrnet {

__global__ void spin_kernel(long long ticks) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) {}
}

static float probe_pair_ms(hipStream_t a, hipStream_t b, hipEvent_t e0, hipEvent_t e1, hipEvent_t eb) {
    const long long ticks = 10000;      // 100 us of the 100 MHz wall clock
    (void)hipEventRecord(e0, a);
    (void)hipStreamWaitEvent(b, e0, 0);
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, a, ticks);
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, b, ticks);
    (void)hipEventRecord(eb, b);
    (void)hipStreamWaitEvent(a, eb, 0);
    (void)hipEventRecord(e1, a);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    return ms;
}

struct StreamPool {
    std::vector<hipStream_t> ordered;      // independent ones first
    int n_independent = 0;
};

static StreamPool& stream_pool() {
    // one pool per HIP device (streams belong to the device that was current when they were created), built once under a lock
    static std::map<int, StreamPool> pools;
    static std::mutex mtx;
    std::lock_guard<std::mutex> lock(mtx);
    int devid = 0;
    (void)hipGetDevice(&devid);
    auto it = pools.find(devid);
    if (it != pools.end()) return it->second;
    StreamPool& pool = pools[devid];
    const int NC = 8;
    std::vector<hipStream_t> cand;
    for (int i = 0; i < NC; ++i) {
        hipStream_t s;
        // AWR_SIDE_PRIORITY=low: the side / branch streams (weight gradients, forked branches) yield to the caller's stream, so that the
        // dependent chain on it runs at solo speed and the side work fills what it leaves (same-box A/B hook)
        static const bool low_prio = []() { const char* e = getenv("AWR_SIDE_PRIORITY"); return e && e[0] == 'l'; }();
        int least = 0, greatest = 0;
        if (low_prio) (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if ((low_prio ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least) : hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) break;
        cand.push_back(s);
    }
    hipEvent_t e0, e1, eb;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventCreate(&eb);
    hipStream_t null_stream = nullptr;
    if (!cand.empty()) (void)probe_pair_ms(null_stream, cand[0], e0, e1, eb);      // warm-up (code load)
    std::vector<hipStream_t> indep, rest;
    for (auto c : cand) {
        bool ok = probe_pair_ms(null_stream, c, e0, e1, eb) < 0.15f;
        for (size_t k = 0; ok && k < indep.size(); ++k) ok = probe_pair_ms(indep[k], c, e0, e1, eb) < 0.15f;
        (ok ? indep : rest).push_back(c);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipEventDestroy(eb);
    pool.n_independent = (int)indep.size();
    pool.ordered = indep;
    pool.ordered.insert(pool.ordered.end(), rest.begin(), rest.end());
    return pool;
}

}  // namespace awrnet

extern "C" {

int awr_stream_pool_info(int* n_streams, int* n_independent) {
    StreamPool& sp = stream_pool();
    if (n_streams) *n_streams = (int)sp.ordered.size();
    if (n_independent) *n_independent = sp.n_independent;
    return AWR_OK;
}

int awr_plan_set_streams(awr_plan* p, int n_side, int comm) {
    AWR_REQUIRE(p && n_side >= 0 && n_side <= 4, "plan_set_streams: 0..4 side streams");
    p->side.clear();
    p->branch.clear();
    if (p->comm) {
        if (p->comm_owned) (void)hipStreamDestroy(p->comm);
        p->comm = nullptr;
    }
    StreamPool& sp = stream_pool();      // (the pool of the CURRENT device: call with the plan's device current, like every other entry point)
    // branch streams only for plans whose backward forks (every stream beyond the device's few hardware queues shares one with another
    // stream and serialises with it: measured on the data-parallel ResNet18 step, whose comm stream is the fourth)
    int nfork = 0;
    for (auto& op : p->bwd) nfork += op.kind == OP_FORK ? 1 : 0;
    const int nbranch = n_side > 0 && nfork > 0 ? 2 : 0;
    AWR_REQUIRE((int)sp.ordered.size() >= n_side + nbranch, "plan_set_streams: could not create the library's streams");
    for (int i = 0; i < n_side; ++i) p->side.push_back(sp.ordered[i]);
    for (int i = 0; i < nbranch; ++i) p->branch.push_back(sp.ordered[n_side + i]);
    // the "comm stream" buckets are handed to is the LAST side stream when there is one: a bucket's scatter has to wait for the weight
    // gradients on it anyway, and a stream of its own would be one too many for the hardware queues -- the collective itself runs on
    // the communication library's stream behind an event
    if (comm) {
        if (!p->side.empty()) {
            p->comm = p->side.back();
            p->comm_owned = false;
        } else {
            HIP_TRY(hipStreamCreateWithFlags(&p->comm, hipStreamNonBlocking));
            p->comm_owned = true;
        }
    }
    return AWR_OK;
}

int awr_plan_set_bucket_callback(awr_plan* p, awr_bucket_cb cb, void* user) {
    AWR_REQUIRE(p, "plan_set_bucket_callback: null pointer");
    if (p->dp) {      // takes effect when the communicator is detached
        p->saved_cb = cb;
        p->saved_user = user;
        return AWR_OK;
    }
    p->bucket_cb = cb;
    p->bucket_user = user;
    return AWR_OK;
}

// the plan's own bucket callback while a communicator is attached: gradient arena [lo, hi) is final in `stream` order
static int dp_dead(awr_plan* p) {      // the host destroyed the communicator before detaching it (awr_plan_set_dp(plan, NULL)): fail, do not dereference
    if (awr_dp_generation(p->dp) == p->dp_gen) return 0;
    awr::set_error("plan: the data-parallel communicator attached with awr_plan_set_dp has been destroyed (detach it with awr_plan_set_dp(plan, NULL) first)");
    p->dp = nullptr;
    p->dp_lost = true;
    return AWR_ERR_ARG;
}
static void dp_bucket(void* user, int64_t lo, int64_t hi, void* stream) {
    awr_plan* p = static_cast<awr_plan*>(user);
    if (p->dp_error || !p->dp) return;
    if ((p->dp_error = dp_dead(p))) return;
    p->dp_error = awr_dp_allreduce(p->dp, p->net->grads + lo, hi - lo, stream);
}

int awr_plan_set_dp(awr_plan* p, awr_dp* dp) {
    AWR_REQUIRE(p && p->built_bwd, "plan_set_dp: needs a training plan");
    AWR_REQUIRE(!dp || awr_dp_generation(dp) != 0, "plan_set_dp: not a live communicator");      // (before any state changes)
    // the host's own callback is saved when the plan's takes its place -- not when it is ALREADY in place (a re-attach after a lost
    // communicator, p->dp == NULL with bucket_cb == dp_bucket, must not overwrite the saved callback with dp_bucket itself)
    if (dp && p->bucket_cb != dp_bucket) {
        p->saved_cb = p->bucket_cb;
        p->saved_user = p->bucket_user;
    }
    p->dp = dp;
    p->dp_gen = dp ? awr_dp_generation(dp) : 0;
    p->dp_error = 0;
    p->dp_lost = false;
    if (dp) {
        p->bucket_cb = dp_bucket;
        p->bucket_user = p;
    } else {
        p->bucket_cb = p->saved_cb;
        p->bucket_user = p->saved_user;
    }
    return AWR_OK;
}

int awr_plan_refresh_weights(awr_plan* p, void* stream) {
    AWR_REQUIRE(p, "plan_refresh_weights: null pointer");
    return refresh_weights(*p, stream);
}

int awr_plan_forward(awr_plan* p, void* stream) {
    AWR_REQUIRE(p, "plan_forward: null pointer");
    return run_list(*p, p->fwd, stream, false);
}

int awr_plan_backward(awr_plan* p, void* stream) {
    AWR_REQUIRE(p && p->built_bwd, "plan_backward: not a training plan");
    return run_list(*p, p->bwd, stream, true);
}

int awr_plan_run_timed(awr_plan* p, int list, void* stream, float* ms) {
    AWR_REQUIRE(p && ms && (list == 0 || list == 1), "plan_run_timed: bad arguments");
    return run_timed(*p, list ? p->bwd : p->fwd, stream, ms);
}

int awr_plan_autotune(awr_plan* p, int reps, void* stream) {
    AWR_REQUIRE(p && reps >= 1, "plan_autotune: bad arguments");
    return autotune(*p, reps, stream);
}

int awr_plan_gemm(const awr_plan* p, int i, const char** name, int* tile_m, int* tile_n, int* target_blocks, float* us, int* tuned) {
    AWR_REQUIRE(p && i >= 0 && i < (int)p->gemms.size(), "plan_gemm: index out of range");
    const GemmRef& g = p->gemms[i];
    if (name) *name = g.name.c_str();
    if (tile_m) *tile_m = g.tm;
    if (tile_n) *tile_n = g.tn;
    if (target_blocks) {
        *target_blocks = g.tb;
        if (!g.tb && g.ca && g.ca->partial && g.ca->split_max > 1) {      // conv launches with scratch, not tuned: the heuristic depth they run with
            int depth = 0;
            if (awr_conv_split_depth(g.ca, &depth) == AWR_OK) *target_blocks = depth;
        }
    }
    if (us) *us = g.us;
    if (tuned) *tuned = g.tuned ? 1 : 0;
    return AWR_OK;
}

int awr_plan_set_gemm(awr_plan* p, int i, int tile_m, int tile_n, int target_blocks, float us) {
    AWR_REQUIRE(p && i >= 0 && i < (int)p->gemms.size(), "plan_set_gemm: index out of range");
    AWR_REQUIRE((tile_m == 1 || tile_m == 2) && (tile_n == 1 || tile_n == 2) && target_blocks >= 0, "plan_set_gemm: tiles in {1,2}");
    GemmRef& g = p->gemms[i];
    AWR_REQUIRE(!(p->det && g.wa), "plan_set_gemm: a deterministic plan sizes the per-chunk copies of its weight gradients for the default geometry");
    if (g.ca) {
        AWR_REQUIRE(!(g.ca->pool_out && !g.ca->w2) || g.ca->Wq % (32 * tile_m) == 0,
                    "plan_set_gemm: launch %d (%s) also writes the max-pool of its output: tile_m = %d needs a map width that is a multiple of %d (it is %d)",
                    i, g.name.c_str(), tile_m, 32 * tile_m, g.ca->Wq);
        g.ca->tile_m = tile_m; g.ca->tile_n = tile_n;
        if (target_blocks && g.ca->partial && target_blocks <= g.ca->split_max) g.ca->split_k = target_blocks;      // conv launches: split-K depth
    } else {
        g.wa->tile_m = tile_m; g.wa->tile_n = tile_n; if (target_blocks) g.wa->target_blocks = target_blocks;
    }
    g.tm = tile_m; g.tn = tile_n; g.tb = target_blocks; g.us = us; g.tuned = true;
    return AWR_OK;
}

int awr_plan_gemm_algo(const awr_plan* p, int i, int* algo) {
    AWR_REQUIRE(p && algo && i >= 0 && i < (int)p->gemms.size(), "plan_gemm_algo: index out of range");
    *algo = p->gemms[i].wa ? p->gemms[i].wa->algo : 0;
    return AWR_OK;
}

int awr_plan_set_gemm_algo(awr_plan* p, int i, int algo) {
    AWR_REQUIRE(p && i >= 0 && i < (int)p->gemms.size(), "plan_set_gemm_algo: index out of range");
    GemmRef& g = p->gemms[i];
    if (!g.wa) {
        AWR_REQUIRE(algo == 0, "plan_set_gemm_algo: launch %d is not a weight gradient", i);
        return AWR_OK;
    }
    AWR_REQUIRE(!p->det, "plan_set_gemm_algo: a deterministic plan keeps the default geometry of its weight gradients");
    AWR_REQUIRE(algo >= 0 && algo <= 3 && awr_conv_wgrad_algo_ok(g.wa, algo), "plan_set_gemm_algo: algo %d does not serve launch %d", algo, i);
    g.wa->algo = algo;
    return AWR_OK;
}

}  // extern "C"
