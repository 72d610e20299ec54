// Network-level engine of libawr_hip.so (include/awr_hip.h, "Network-level API"), the model.  awr_net: the checkpoint layout of one backbone
// (model/resnet_deconv.py:19-136, model/hourglass.py:105-165) -- state_dict keys, shapes and arena offsets -- and its conv / BatchNorm layers bound
// to caller-owned parameter / gradient / buffer arenas, with packed GEMM copies of the weights.  Plans over it: csrc/awr_plan_build.hip,
// csrc/awr_plan_run.hip; shared types: csrc/awr_plan.h.  Host code only (no kernels).
#include <string.h>

#include "awr_plan.h"

using namespace awrnet;

namespace awrnet {

int dev_alloc(std::vector<void*>& owner, size_t bytes, bool zero, void** out) {
    void* p = nullptr;
    if (bytes == 0) bytes = 16;
    HIP_TRY(hipMalloc(&p, bytes));
    if (zero) HIP_TRY(hipMemset(p, 0, bytes));
    owner.push_back(p);
    *out = p;
    return AWR_OK;
}

void free_all(std::vector<void*>& v) {
    for (void* p : v) (void)hipFree(p);
    v.clear();
}

static ConvLayer conv_layer(awr_net* n, const std::string& wkey, const Spec& spec, const std::string& bkey = "") {
    ConvLayer c;
    c.spec = spec;
    c.w = n->P(wkey);
    c.gw = n->G(wkey);
    if (!bkey.empty()) {
        c.bias = n->P(bkey);
        c.gbias = n->G(bkey);
    }
    c.name = wkey.substr(0, wkey.rfind('.'));
    return c;
}

static BNLayer bn_layer(awr_net* n, const std::string& prefix) {
    BNLayer b;
    b.C = (int)n->layout.at(prefix + ".weight").numel;
    b.gamma = n->P(prefix + ".weight");
    b.beta = n->P(prefix + ".bias");
    b.ggamma = n->G(prefix + ".weight");
    b.gbeta = n->G(prefix + ".bias");
    b.rmean = n->Bf(prefix + ".running_mean");
    b.rvar = n->Bf(prefix + ".running_var");
    b.name = prefix;
    return b;
}

static int head_layer(awr_net* n, ConvLayer& h, int cin, const std::string& a, const std::string& b, const std::string& name) {
    h = ConvLayer();
    h.head = true;
    h.J = n->J;
    h.cp = (int)round_up(4 * n->J, 32);
    h.spec = make_spec(false, cin, 4 * n->J, 1, 1, 0, 0, h.cp);
    h.w1 = n->P(a + ".weight"); h.gw1 = n->G(a + ".weight"); h.b1 = n->P(a + ".bias"); h.gb1 = n->G(a + ".bias");
    h.w2 = n->P(b + ".weight"); h.gw2 = n->G(b + ".weight"); h.b2 = n->P(b + ".bias"); h.gb2 = n->G(b + ".bias");
    h.w = h.w1; h.gw = h.gw1;
    h.name = name;
    void* p;
    NET_CHECK(dev_alloc(n->owned, (size_t)h.cp * 4, true, &p));
    h.bias_cat = (float*)p;
    return AWR_OK;
}

// name -> layer objects bound to the current arenas (nets.py: _make_layers)
static int make_layers(awr_net* n) {
    n->convs.clear();
    n->bns.clear();
    n->duals.clear();
    if (n->kind == 0) {
        n->convs["pre.0"] = conv_layer(n, "pre.0.weight", make_spec(false, 25, 64, 1, 1, 0, 32));
        n->bns["pre.1"] = bn_layer(n, "pre.1");
        int cin = 64;
        const int planes_[4] = {64, 128, 256, 512}, stride_[4] = {1, 2, 2, 2};
        const bool bott = n->depth != 18;
        const int exp = bott ? 4 : 1;
        const int* nb = resnet_blocks(n->depth);
        for (int li = 1; li <= 4; ++li)
            for (int bi = 0; bi < nb[li - 1]; ++bi) {
                const std::string p = fmt("layer%d.%d", li, bi);
                const int planes = planes_[li - 1], s = bi == 0 ? stride_[li - 1] : 1;
                if (!bott) {
                    n->convs[p + ".conv1"] = conv_layer(n, p + ".conv1.weight", make_spec(false, cin, planes, 3, s, 1));
                    n->bns[p + ".bn1"] = bn_layer(n, p + ".bn1");
                    n->convs[p + ".conv2"] = conv_layer(n, p + ".conv2.weight", make_spec(false, planes, planes, 3, 1, 1));
                    n->bns[p + ".bn2"] = bn_layer(n, p + ".bn2");
                } else {      // Bottleneck: 1x1 -> 3x3 (carries the stride) -> 1x1 x4 (resnet_deconv.py:177-215)
                    n->convs[p + ".conv1"] = conv_layer(n, p + ".conv1.weight", make_spec(false, cin, planes, 1, 1, 0));
                    n->bns[p + ".bn1"] = bn_layer(n, p + ".bn1");
                    n->convs[p + ".conv2"] = conv_layer(n, p + ".conv2.weight", make_spec(false, planes, planes, 3, s, 1));
                    n->bns[p + ".bn2"] = bn_layer(n, p + ".bn2");
                    n->convs[p + ".conv3"] = conv_layer(n, p + ".conv3.weight", make_spec(false, planes, planes * exp, 1, 1, 0));
                    n->bns[p + ".bn3"] = bn_layer(n, p + ".bn3");
                }
                if (n->layout.has(p + ".downsample.0.weight")) {
                    n->convs[p + ".downsample.0"] = conv_layer(n, p + ".downsample.0.weight", make_spec(false, cin, planes * exp, 1, s, 0));
                    n->bns[p + ".downsample.1"] = bn_layer(n, p + ".downsample.1");
                }
                cin = planes * exp;
            }
        for (int i = 0; i < n->ndeconv; ++i) {
            n->convs[fmt("deconv_layers.%d", 3 * i)] = conv_layer(n, fmt("deconv_layers.%d.weight", 3 * i), make_spec(true, cin, 256, 4, 2, 1));
            n->bns[fmt("deconv_layers.%d", 3 * i + 1)] = bn_layer(n, fmt("deconv_layers.%d", 3 * i + 1));
            cin = 256;
        }
        NET_CHECK(head_layer(n, n->convs["head"], 256, "final1", "final2", "final"));
        return AWR_OK;
    }
    const int cp = (int)round_up(4 * n->J, 32);
    for (const auto& en : n->layout.e) {
        const std::string& key = en.key;
        if (en.kind == CONV_W && key.size() > 12 && key.compare(key.size() - 12, 12, ".conv.weight") == 0) {
            if (en.unused) continue;
            const std::string pfx = key.substr(0, key.size() - 12);
            const int cout = (int)en.shape[0], cin = (int)en.shape[1], k = (int)en.shape[2];
            Spec spec;
            if (pfx == "pre.0") spec = make_spec(false, 25, 64, 1, 1, 0, 32);
            else if (pfx.compare(0, 11, "merge_preds") == 0) spec = make_spec(false, cin, cout, 1, 1, 0, cp);
            else spec = make_spec(false, cin, cout, k, 1, (k - 1) / 2);
            n->convs[pfx] = conv_layer(n, key, spec, pfx + ".conv.bias");
        } else if (en.kind == BN_W) {
            const std::string pfx = key.substr(0, key.size() - 7);
            n->bns[pfx] = bn_layer(n, pfx);
        }
    }
    for (int i = 0; i < n->nstack; ++i)
        NET_CHECK(head_layer(n, n->convs[fmt("head.%d", i)], n->f, fmt("outs_1.%d", i), fmt("outs_2.%d", i), fmt("outs.%d", i)));
    return AWR_OK;
}

}  // namespace awrnet

extern "C" {

int awr_net_create(int kind, int nstack, int J, int downsample, awr_net** out) {
    AWR_REQUIRE(out, "net_create: null pointer");
    AWR_REQUIRE(kind == 0 || kind == 1, "net_create: kind must be 0 (ResNet18-deconv) or 1 (stacked hourglass)");
    AWR_REQUIRE(J >= 1 && J <= 64, "net_create: J=%d joints", J);
    AWR_REQUIRE(kind == 1 || downsample == 1 || downsample == 2 || downsample == 4, "net_create: downsample must be 1, 2 or 4 (config.py:31)");
    AWR_REQUIRE(kind == 0 || (nstack >= 1 && nstack <= 8), "net_create: nstack=%d", nstack);
    AWR_REQUIRE(kind == 1 || nstack == 0 || nstack == 1 || nstack == 18 || nstack == 50 || nstack == 101 || nstack == 152,
                "net_create: kind 0 takes the ResNet depth in `nstack`: 18 (also 0 / 1), 50, 101 or 152 (resnet_deconv.py:9-13), got %d", nstack);
    awr_net* n = new awr_net();
    n->kind = kind;
    n->J = J;
    if (kind == 0) {
        n->depth = nstack <= 1 ? 18 : nstack;
        n->nstack = n->nstage = 1;
        n->downsample = downsample;
        int lg = 0;
        while ((1 << lg) < downsample) ++lg;
        n->ndeconv = 4 - lg;
        resnet_layout(n->layout, n->depth, J, downsample);
    } else {
        n->nstack = n->nstage = nstack;
        n->downsample = 2;
        hourglass_layout(n->layout, nstack, J, n->f);
    }
    n->layout.assign();
    *out = n;
    return AWR_OK;
}

int awr_net_destroy(awr_net* n) {
    if (!n) return AWR_OK;
    for (auto* p : n->plans) destroy_plan(p);
    free_all(n->owned);
    delete n;
    return AWR_OK;
}

int awr_net_sizes(const awr_net* n, int64_t* n_tensors, int64_t* n_params, int64_t* n_active, int64_t* n_buffers, int* n_counters, int* nstage) {
    AWR_REQUIRE(n, "net_sizes: null pointer");
    if (n_tensors) *n_tensors = (int64_t)n->layout.e.size();
    if (n_params) *n_params = n->layout.n_params;
    if (n_active) *n_active = n->layout.n_active;
    if (n_buffers) *n_buffers = n->layout.n_buffers;
    if (n_counters) *n_counters = n->layout.n_counters;
    if (nstage) *nstage = n->nstage;
    return AWR_OK;
}

int awr_net_tensor_info(const awr_net* n, int64_t i, const char** key, int* kind, int* ndim, int64_t shape[4], int64_t* offset, int* unused) {
    AWR_REQUIRE(n && i >= 0 && i < (int64_t)n->layout.e.size(), "net_tensor_info: index out of range");
    const Entry& e = n->layout.e[i];
    if (key) *key = e.key.c_str();
    if (kind) *kind = e.kind;
    if (ndim) *ndim = e.ndim;
    if (shape) memcpy(shape, e.shape, sizeof e.shape);
    if (offset) *offset = e.off;
    if (unused) *unused = e.unused ? 1 : 0;
    return AWR_OK;
}

int awr_net_bind(awr_net* n, float* params, float* grads, float* buffers) {
    AWR_REQUIRE(n && params && grads && buffers, "net_bind: null pointer");
    AWR_REQUIRE((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)buffers) & 15) == 0, "net_bind: arenas must be 16-byte aligned");
    for (auto* p : n->plans) destroy_plan(p);      // plans hold raw pointers into the old arenas
    n->plans.clear();
    free_all(n->owned);
    n->params = params;
    n->grads = grads;
    n->buffers = buffers;
    return make_layers(n);
}

}  // extern "C"
