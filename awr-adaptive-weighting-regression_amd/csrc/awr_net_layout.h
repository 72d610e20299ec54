// Checkpoint layout of the AWR backbones: the ordered state_dict entries of ResNet-deconv and the stacked hourglass, their
// shapes and their offsets in the parameter / buffer arenas.  Pure host logic of the plan engine (csrc/awr_net.hip): standard library
// only, so that tests/native/plan_host_main.cpp compiles it without HIP.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <string>
#include <vector>

namespace awrnet {

#ifndef AWR_NET_ROUND_UP
#define AWR_NET_ROUND_UP
static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
#endif

// ------------------------------------------------------------------------------------------
// checkpoint layout: ordered state_dict entries
// ------------------------------------------------------------------------------------------
enum Kind { CONV_W = 0, DECONV_W = 1, CONV_B = 2, BN_W = 3, BN_B = 4, BN_MEAN = 5, BN_VAR = 6, COUNTER = 7 };
static inline bool is_param(int k) { return k <= BN_B; }

struct Entry {
    std::string key;
    int ndim;
    int64_t shape[4];
    int kind;
    int64_t off = 0;     // floats into the parameter arena (params) / buffer arena (running stats); index for counters
    int64_t numel = 1;
    bool unused = false;  // parameters that never receive a gradient (hourglass skip_layers with inp == out)
};

struct Layout {
    std::vector<Entry> e;
    int64_t n_params = 0, n_active = 0, n_buffers = 0;
    int n_counters = 0;
    std::map<std::string, int> index;

    void add(const std::string& key, std::vector<int64_t> shape, int kind) {
        Entry en;
        en.key = key;
        en.kind = kind;
        en.ndim = (int)shape.size();
        for (int i = 0; i < 4; ++i) en.shape[i] = i < en.ndim ? shape[i] : 1;
        for (int i = 0; i < en.ndim; ++i) en.numel *= shape[i];
        index[key] = (int)e.size();
        e.push_back(en);
    }
    void bn(const std::string& p, int c) {
        add(p + ".weight", {c}, BN_W);
        add(p + ".bias", {c}, BN_B);
        add(p + ".running_mean", {c}, BN_MEAN);
        add(p + ".running_var", {c}, BN_VAR);
        add(p + ".num_batches_tracked", {}, COUNTER);
    }
    const Entry& at(const std::string& key) const { return e[index.at(key)]; }
    bool has(const std::string& key) const { return index.count(key) != 0; }

    // arena offsets: live parameters first, never-trained ones at the tail (the optimiser / all-reduce cover [0, n_active)
    // only -- exactly torch's `p.grad is None` skip); every view 16-byte aligned
    void assign() {
        int64_t off = 0;
        for (int pass = 0; pass < 2; ++pass) {
            for (auto& en : e) {
                if (!is_param(en.kind) || en.unused != (pass == 1)) continue;
                en.off = off;
                off = round_up(off + en.numel, 4);
            }
            if (pass == 0) n_active = off;
        }
        n_params = off;
        int64_t boff = 0;
        int ci = 0;
        for (auto& en : e) {
            if (en.kind == BN_MEAN || en.kind == BN_VAR) {
                en.off = boff;
                boff += round_up(en.shape[0], 4);
            } else if (en.kind == COUNTER) {
                en.off = ci++;
            }
        }
        n_buffers = boff;
        n_counters = ci;
    }
};

static std::string fmt(const char* f, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// get_deconv_net(depth, J, downsample).state_dict() (resnet_deconv.py:8-16, :31-53): BasicBlock [2,2,2,2] for depth 18, Bottleneck
// (expansion 4) [3,4,6,3] / [3,4,23,3] / [3,8,36,3] for 50 / 101 / 152.  Registration order inside a block: conv1, bn1, conv2, bn2,
// (conv3, bn3,) downsample (resnet_deconv.py:148-156, :182-195).
static const int* resnet_blocks(int depth) {
    static const int b18[4] = {2, 2, 2, 2}, b50[4] = {3, 4, 6, 3}, b101[4] = {3, 4, 23, 3}, b152[4] = {3, 8, 36, 3};
    return depth == 50 ? b50 : depth == 101 ? b101 : depth == 152 ? b152 : b18;
}

static void resnet_layout(Layout& L, int depth, int J, int downsample) {
    const bool bott = depth != 18;
    const int exp = bott ? 4 : 1;
    const int* nb = resnet_blocks(depth);
    L.add("pre.0.weight", {64, 1, 5, 5}, CONV_W);
    L.bn("pre.1", 64);
    int cin = 64;
    const int planes_[4] = {64, 128, 256, 512};
    for (int li = 1; li <= 4; ++li) {
        const int planes = planes_[li - 1];
        for (int bi = 0; bi < nb[li - 1]; ++bi) {
            const std::string p = fmt("layer%d.%d", li, bi);
            if (!bott) {
                L.add(p + ".conv1.weight", {planes, cin, 3, 3}, CONV_W);
                L.bn(p + ".bn1", planes);
                L.add(p + ".conv2.weight", {planes, planes, 3, 3}, CONV_W);
                L.bn(p + ".bn2", planes);
            } else {
                L.add(p + ".conv1.weight", {planes, cin, 1, 1}, CONV_W);
                L.bn(p + ".bn1", planes);
                L.add(p + ".conv2.weight", {planes, planes, 3, 3}, CONV_W);
                L.bn(p + ".bn2", planes);
                L.add(p + ".conv3.weight", {planes * exp, planes, 1, 1}, CONV_W);
                L.bn(p + ".bn3", planes * exp);
            }
            if (bi == 0 && (li > 1 || cin != planes * exp)) {      // _make_layer: stride != 1 or inplanes != planes * expansion
                L.add(p + ".downsample.0.weight", {planes * exp, cin, 1, 1}, CONV_W);
                L.bn(p + ".downsample.1", planes * exp);
            }
            cin = planes * exp;
        }
    }
    int lg = 0;
    while ((1 << lg) < downsample) ++lg;
    for (int i = 0; i < 4 - lg; ++i) {
        L.add(fmt("deconv_layers.%d.weight", 3 * i), {cin, 256, 4, 4}, DECONV_W);
        L.bn(fmt("deconv_layers.%d", 3 * i + 1), 256);
        cin = 256;
    }
    L.add("final1.weight", {3 * J, 256, 1, 1}, CONV_W);
    L.add("final1.bias", {3 * J}, CONV_B);
    L.add("final2.weight", {J, 256, 1, 1}, CONV_W);
    L.add("final2.bias", {J}, CONV_B);
}

static void hgconv_keys(Layout& L, const std::string& p, int cin, int cout, int k, bool bn) {
    L.add(p + ".conv.weight", {cout, cin, k, k}, CONV_W);
    L.add(p + ".conv.bias", {cout}, CONV_B);
    if (bn) L.bn(p + ".bn", cout);
}

// hourglass.py:28-42 -- registration order bn1, conv1, bn2, conv2, bn3, conv3, skip_layer (present even when unused)
static void residual_keys(Layout& L, const std::string& p, int cin, int cout) {
    const int h = cout / 2;
    L.bn(p + ".bn1", cin);
    hgconv_keys(L, p + ".conv1", cin, h, 1, false);
    L.bn(p + ".bn2", h);
    hgconv_keys(L, p + ".conv2", h, h, 3, false);
    L.bn(p + ".bn3", h);
    hgconv_keys(L, p + ".conv3", h, cout, 1, false);
    hgconv_keys(L, p + ".skip_layer", cin, cout, 1, false);
}

static void hourglass_keys(Layout& L, const std::string& p, int depth, int f) {
    residual_keys(L, p + ".up1", f, f);
    residual_keys(L, p + ".low1", f, f);
    if (depth > 1) hourglass_keys(L, p + ".low2", depth - 1, f);
    else residual_keys(L, p + ".low2", f, f);
    residual_keys(L, p + ".low3", f, f);
}

// PoseNet('hourglass_<nstack>', J).state_dict() (hourglass.py:105-142)
static void hourglass_layout(Layout& L, int nstack, int J, int f) {
    hgconv_keys(L, "pre.0", 1, 64, 5, true);
    residual_keys(L, "pre.1", 64, 128);
    residual_keys(L, "pre.3", 128, 256);
    residual_keys(L, "pre.4", 256, f);
    for (int i = 0; i < nstack; ++i) hourglass_keys(L, fmt("hgs.%d.0", i), 4, f);
    for (int i = 0; i < nstack; ++i) {
        residual_keys(L, fmt("features.%d.0", i), f, f);
        hgconv_keys(L, fmt("features.%d.1", i), f, f, 1, true);
    }
    for (int i = 0; i < nstack; ++i) {
        L.add(fmt("outs_1.%d.weight", i), {3 * J, f, 1, 1}, CONV_W);
        L.add(fmt("outs_1.%d.bias", i), {3 * J}, CONV_B);
    }
    for (int i = 0; i < nstack; ++i) {
        L.add(fmt("outs_2.%d.weight", i), {J, f, 1, 1}, CONV_W);
        L.add(fmt("outs_2.%d.bias", i), {J}, CONV_B);
    }
    for (int i = 0; i < nstack - 1; ++i) hgconv_keys(L, fmt("merge_features.%d.conv", i), f, f, 1, false);
    for (int i = 0; i < nstack - 1; ++i) hgconv_keys(L, fmt("merge_preds.%d.conv", i), 4 * J, f, 1, false);
    // Residual.skip_layer exists in every block but only runs when inp_dim != out_dim (hourglass.py:38-47)
    for (auto& en : L.e) {
        const size_t pos = en.key.find(".skip_layer.");
        if (pos == std::string::npos) continue;
        const Entry& w = L.e[L.index.at(en.key.substr(0, pos) + ".skip_layer.conv.weight")];
        if (w.shape[0] == w.shape[1]) en.unused = true;
    }
}

}  // namespace awrnet
