// Stand-alone host program over the plan engine's pure host logic (csrc/awr_net_layout.h, csrc/awr_net_geometry.h): prints, as one JSON
// object, the checkpoint layouts, the launch geometry of a fixed list of layer specs and the gradient buckets of the write lists named by
// argv[1].  tests/test_host_cpu.py builds it with the address and undefined-behaviour sanitizers and compares every figure with the Python
// statements (engine.NetHandle.layout, ops.ConvSpec / make_conv_args / make_wgrad_args, engine.plan_buckets).
//
// Bucket input (text): the number of cases, then per case "n_active n_buckets n_writes" followed by n_writes lines "lo hi ready".
#include <stdio.h>

#include "../../awr-adaptive-weighting-regression_amd/csrc/awr_net_geometry.h"
#include "../../awr-adaptive-weighting-regression_amd/csrc/awr_net_layout.h"

using namespace awrnet;

static void layout_json(const char* name, Layout& L, bool last) {
    L.assign();
    printf("\"%s\":{\"n_params\":%lld,\"n_active\":%lld,\"n_buffers\":%lld,\"n_counters\":%d,\"entries\":[", name, (long long)L.n_params,
           (long long)L.n_active, (long long)L.n_buffers, L.n_counters);
    for (size_t i = 0; i < L.e.size(); ++i) {
        const Entry& e = L.e[i];
        printf("%s[\"%s\",[", i ? "," : "", e.key.c_str());
        for (int d = 0; d < e.ndim; ++d) printf("%s%lld", d ? "," : "", (long long)e.shape[d]);
        printf("],%d,%lld,%d]", e.kind, (long long)e.off, e.unused ? 1 : 0);
    }
    printf("]}%s\n", last ? "" : ",");
}

constexpr int MAX_TAPS = 16;      // awr_phase.tap[16], awr_wgrad_args.dy[16] / dx[16]: a longer phase has no argument block

static void prob_json(const char* name, const Prob& p, int B, int T) {
    printf("\"%s\":{\"Hin\":%d,\"Win\":%d,\"Cin\":%d,\"Hout\":%d,\"Wout\":%d,\"N\":%d,\"Hq\":%d,\"Wq\":%d,\"so\":%d,\"si\":%d,\"full\":%d,\"k_extent\":%d,\"phases\":[",
           name, p.Hin, p.Win, p.Cin, p.Hout, p.Wout, p.N, p.Hq, p.Wq, p.so, p.si, p.full ? 1 : 0, p.k_extent());
    bool fits = p.phases.size() <= 4;
    for (size_t i = 0; i < p.phases.size(); ++i) {
        const PhaseT& ph = p.phases[i];
        fits = fits && ph.taps.size() <= MAX_TAPS;
        printf("%s[%d,%d,[", i ? "," : "", ph.py, ph.px);
        for (size_t t = 0; t < ph.taps.size(); ++t) printf("%s[%d,%d,%d]", t ? "," : "", ph.taps[t].dy, ph.taps[t].dx, ph.taps[t].wt);
        printf("]]");
    }
    printf("],\"args\":");
    if (!fits) {
        printf("null}");
        return;
    }
    awr_conv_args a;
    fill_conv_args(a, p, B, nullptr, nullptr, nullptr, nullptr, T, 0);
    printf("{\"B\":%d,\"Hin\":%d,\"Win\":%d,\"Cin\":%d,\"Hq\":%d,\"Wq\":%d,\"Hout\":%d,\"Wout\":%d,\"N\":%d,\"so\":%d,\"si\":%d,\"T\":%d,\"nphase\":%d,\"accum\":%d,\"ph\":[",
           a.B, a.Hin, a.Win, a.Cin, a.Hq, a.Wq, a.Hout, a.Wout, a.N, a.so, a.si, a.T, a.nphase, a.accum);
    for (int i = 0; i < a.nphase; ++i) {
        printf("%s[%d,%d,%d,[", i ? "," : "", a.ph[i].py, a.ph[i].px, a.ph[i].ntaps);
        for (int t = 0; t < a.ph[i].ntaps; ++t) printf("%s%d", t ? "," : "", (int)a.ph[i].tap[t]);
        printf("]]");
    }
    printf("]}}");
}

static void pack_json(const char* name, const PackRecipe& r) {
    printf("\"%s\":[%d,%d,%d,%d,%d,%d]", name, r.d0, r.d1, r.T, r.transpose, r.rows, r.ld);
}

static void geometry_json(int index, const Spec& s, int h, int B, bool last) {
    int ho, wo;
    s.out_hw(h, h, ho, wo);
    printf("{\"spec\":%d,\"h\":%d,\"out_hw\":[%d,%d],", index, h, ho, wo);
    prob_json("fwd", fwd_problem(s, h, h), B, s.T());
    printf(",");
    prob_json("dgrad", dgrad_problem(s, h, h), B, s.T());
    printf(",");
    pack_json("fwd_pack", fwd_pack(s));
    printf(",");
    pack_json("dgrad_pack", dgrad_pack(s));
    printf(",\"wgrad\":");
    if (s.T() > MAX_TAPS) {
        printf("null");
    } else {
        const WProb w = wgrad_problem(s, h, h);
        const int ld = w.Cg;
        awr_wgrad_args a;
        fill_wgrad_args(a, w, B, nullptr, nullptr, nullptr, ld);
        printf("{\"d_is_dy\":%d,\"d0\":%d,\"d1\":%d,\"B\":%d,\"Hd\":%d,\"Wd\":%d,\"Cd\":%d,\"Hg\":%d,\"Wg\":%d,\"Cg\":%d,\"sg\":%d,\"T\":%d,\"ld\":%d,\"dy\":[", w.d_is_dy ? 1 : 0,
               w.d0, w.d1, a.B, a.Hd, a.Wd, a.Cd, a.Hg, a.Wg, a.Cg, a.sg, a.T, a.ld);
        for (int t = 0; t < a.T; ++t) printf("%s%d", t ? "," : "", (int)a.dy[t]);
        printf("],\"dx\":[");
        for (int t = 0; t < a.T; ++t) printf("%s%d", t ? "," : "", (int)a.dx[t]);
        printf("]}");
    }
    printf("}%s\n", last ? "" : ",");
}

static int buckets_json(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 1;
    }
    int ncases = 0;
    if (fscanf(f, "%d", &ncases) != 1) return 1;
    for (int c = 0; c < ncases; ++c) {
        long long n_active = 0;
        int n_buckets = 0, n = 0;
        if (fscanf(f, "%lld %d %d", &n_active, &n_buckets, &n) != 3 || n < 0) return 1;
        std::vector<Range> ws;
        for (int i = 0; i < n; ++i) {
            long long lo = 0, hi = 0;
            int ready = 0;
            if (fscanf(f, "%lld %lld %d", &lo, &hi, &ready) != 3) return 1;
            ws.push_back({(int64_t)lo, (int64_t)hi, ready});
        }
        const std::vector<Range> out = plan_buckets(ws, n_active, n_buckets);
        printf("%s[", c ? "," : "");
        for (size_t k = 0; k < out.size(); ++k) printf("%s[%lld,%lld,%d]", k ? "," : "", (long long)out[k].lo, (long long)out[k].hi, out[k].ready);
        printf("]\n");
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    printf("{\"layouts\":{\n");
    {
        Layout r18, hg1, hg2;
        resnet_layout(r18, 18, 14, 2);
        hourglass_layout(hg1, 1, 14, 256);
        hourglass_layout(hg2, 2, 21, 256);
        layout_json("resnet_18", r18, false);
        layout_json("hourglass_1", hg1, false);
        layout_json("hourglass_2", hg2, true);
    }
    printf("},\"geometry\":[\n");
    const Spec specs[6] = {
        make_spec(false, 64, 128, 1, 1, 0),        // conv 1x1 s1
        make_spec(false, 64, 64, 3, 1, 1),         // conv 3x3 s1 p1
        make_spec(false, 64, 128, 3, 2, 1),        // conv 3x3 s2 p1
        make_spec(false, 3, 64, 7, 2, 3, 32),      // conv 7x7 s2 p3, cin_pad 32
        make_spec(false, 64, 128, 1, 2, 0),        // conv 1x1 s2
        make_spec(true, 128, 64, 4, 2, 1),         // deconv 4x4 s2 p1
    };
    const int sizes[2] = {8, 32};
    for (int i = 0; i < 6; ++i)
        for (int k = 0; k < 2; ++k) geometry_json(i, specs[i], sizes[k], 2, i == 5 && k == 1);
    printf("],\"buckets\":[\n");
    if (argc > 1 && buckets_json(argv[1])) return 1;
    printf("]}\n");
    return 0;
}
