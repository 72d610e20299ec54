// Shared types of the network-level engine (include/awr_hip.h, "Network-level API"), and nothing else: the layers of a backbone bound to
// the caller's arenas (awr_net), one static execution plan (awr_plan: tensors, two flat lists of pre-bound launches, the tunable launches),
// the error macros, and the few functions that cross the engine's translation units:
//
//   awr_net.hip         the model: make_layers, awr_net_create / destroy / sizes / tensor_info / bind
//   awr_plan_build.hip  building a plan: Builder (every launch and its backward emitter), the two backbones, awr_plan_create[_modes]
//   awr_plan_run.hip    using a plan: weight refresh, replay, timing, the tuner, the stream pool, the awr_dp hook-up, the awr_plan_* entry points
#pragma once
#include <deque>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "awr_common.h"
#include "awr_conv_modes.h"
#include "awr_net_geometry.h"      // conv / weight-gradient problems, pack recipes, bucket planner (host logic, no HIP)
#include "awr_net_layout.h"        // checkpoint layout (host logic, no HIP)

namespace awrnet {

using awr::env_int;
using awr::set_error;

#define NET_CHECK(call)                 \
    do {                                \
        if (int e__ = (call)) return e__; \
    } while (0)

#define HIP_TRY(call)                                              \
    do {                                                           \
        hipError_t e__ = (call);                                   \
        if (e__ != hipSuccess) {                                   \
            set_error("%s: %s", #call, hipGetErrorString(e__));    \
            return AWR_ERR_HIP;                                    \
        }                                                          \
    } while (0)

// ------------------------------------------------------------------------------------------
// layers bound to the arenas
// ------------------------------------------------------------------------------------------
struct Packed {
    float* p = nullptr;
    void* split = nullptr;
    int rows = 0, T = 0, ld = 0;
    int64_t numel() const { return (int64_t)rows * T * ld; }
};

struct ConvLayer {
    Spec spec;
    float *w = nullptr, *gw = nullptr, *bias = nullptr, *gbias = nullptr;
    Packed p_fwd, p_dgrad;
    std::string name;
    // fused head: final1 (256->3J) and final2 (256->J) 1x1 convs as one 256->Cp GEMM (resnet_deconv.py:52-53,:133-136 /
    // hourglass.py:137-138,:153-157); Cp = 4J rounded up to 32, extra rows zero
    bool head = false;
    int J = 0, cp = 0;
    float *w1 = nullptr, *gw1 = nullptr, *b1 = nullptr, *gb1 = nullptr, *w2 = nullptr, *gw2 = nullptr, *b2 = nullptr, *gb2 = nullptr, *bias_cat = nullptr;
    const float* bias_ptr() const { return head ? bias_cat : bias; }
};

// conv3 + skip_layer of a hourglass residual whose skip path is a 1x1 conv (hourglass.py:38-47, :44-59), forward-fused: one GEMM
// over K = [conv3's input channels | the block input's channels], packed weight rows [W3 row | Wskip row], bias b3 + bskip
struct DualLayer {
    ConvLayer *c3 = nullptr, *sk = nullptr;
    Packed p;
    float* bias_sum = nullptr;
    std::string name;
};

struct BNLayer {
    int C = 0;
    float *gamma = nullptr, *beta = nullptr, *ggamma = nullptr, *gbeta = nullptr, *rmean = nullptr, *rvar = nullptr;
    std::string name;
};

}  // namespace awrnet

struct awr_plan;

struct awr_net {
    int kind = 0, nstack = 1, J = 14, downsample = 2, f = 256;
    int depth = 18;                      // kind 0: ResNet depth (18 BasicBlock; 50 / 101 / 152 Bottleneck)
    int nstage = 1, ndeconv = 3;
    awrnet::Layout layout;
    float *params = nullptr, *grads = nullptr, *buffers = nullptr;
    std::map<std::string, awrnet::ConvLayer> convs;
    std::map<std::string, awrnet::BNLayer> bns;
    std::map<std::string, awrnet::DualLayer> duals;
    std::vector<void*> owned;            // packed weights (device), freed with the net
    std::vector<awr_plan*> plans;
    std::vector<std::string> key_storage;

    float* P(const std::string& key) const { return params + layout.at(key).off; }
    float* G(const std::string& key) const { return grads + layout.at(key).off; }
    float* Bf(const std::string& key) const { return buffers + layout.at(key).off; }
};

namespace awrnet {

// ------------------------------------------------------------------------------------------
// plan-time tensor handle: an NHWC fp32 buffer plus (later) its gradient buffer
// ------------------------------------------------------------------------------------------
struct StatBuf {
    double* p = nullptr;
    int nslots = 0;
};

struct FusedStats { double* sp = nullptr; int ns = 0; };      // set by bn_act when the BatchNorm takes the producer's statistics

struct Tn {
    float* buf = nullptr;
    float* grad = nullptr;
    int B = 0, H = 0, W = 0, C = 0;
    bool needs_grad = true;
    StatBuf stats;
    // lazy: the tensor this handle stands for is relu(buf*scale+shift) -- a BatchNorm(+ReLU) output that is never written to
    // HBM; its consumers (conv / wgrad / maxpool loaders) apply the affine on the fly
    bool lazy = false, lz_relu = false;
    const float *lz_scale = nullptr, *lz_shift = nullptr;
    // a materialised BatchNorm output WITHOUT ReLU or residual (the ResNet downsample projection's): what a consumer that adds it to
    // another BatchNorm's output before a ReLU needs to reduce this BatchNorm's backward sums together with its own
    const float *bn_y = nullptr, *bn_coef4 = nullptr;
    StatBuf pre_sums;      // set by that consumer's backward: sum g / sum g*xhat of THIS BatchNorm are already in here
    // a conv output y whose BatchNorm's backward is NOT on the critical chain (set by bn_bwd, consumed by the conv's conv_bwd): the conv's data
    // gradient reads g = d(loss)/d(bn(y)) (masked) and y itself and forms d(y) = a1 g + a2 (y - mean) + a3 on the fly (awr_conv_args.in_bnb_y);
    // d(y) is still written -- by an apply launch that travels with the weight gradient on its side stream
    bool conv_out = false;
    awr_conv_args* pair_args = nullptr;       // written by a fused inference pair (conv_pair): a 2x2 max-pool of it can ride in that launch (pool_out)
    // ... or by a plain / two-tensor 1x1 inference launch whose form admits pool_out (Builder::note_pool_producer); its op and tunable-launch entry get
    // the "+pool" suffix when a max-pool takes the offer
    awr_conv_args* pool_args = nullptr;
    size_t pool_op = 0, pool_gemm = 0;
    struct FusedStats* fstats = nullptr;      // produced by a max-pool / up-sampling add that can accumulate the next BatchNorm's statistics itself
    bool half_ok = false;     // conv output whose data gradient may run as two half-batch parts (set by conv())
    bool half_dy = false;     // ... and whose BatchNorm backward writes d(y) half by half: the second half on the weight gradient's stream
    int conv_taps = 0;
    const float *lz_g = nullptr, *lz_lin4 = nullptr, *lz_mean = nullptr, *lz_invstd = nullptr, *lz_coef = nullptr;
    std::string name;
    int64_t npix() const { return (int64_t)B * H * W; }
    int64_t numel() const { return npix() * C; }
};

enum OpKind { OP_CALL = 0, OP_ZERO, OP_COPY, OP_BUCKET, OP_FORK, OP_ENDFORK, OP_JOIN, OP_HALFWAIT };

struct Op {
    int kind = OP_CALL;
    std::function<int(void*)> fn;
    std::string name;
    void* p = nullptr;        // OP_ZERO / OP_COPY destination
    const void* q = nullptr;  // OP_COPY source
    size_t bytes = 0;
    int64_t lo = 0, hi = 0;   // OP_BUCKET
    int sid = 0;              // fork / join stream id
    bool side_ok = false;     // weight-gradient launch that may run on a side stream
    bool pair_next = false;   // side_ok launch that shares the side stream of the NEXT side_ok launch (its producer: awr_bn_bwd_apply -> awr_conv_wgrad)
    bool half_sig = false;    // side_ok launch (the second half of a BatchNorm-backward apply): record "half B is written" behind it; OP_HALFWAIT makes the
                              // issuing chain wait for that record (NOT for the weight gradient queued behind it on the same side stream)
    bool gemm = false;        // conv / stem family (timed by run_timed)
    bool boundary = false;    // NCHW <-> NHWC bridge at the reference boundary: skipped while the plan's NHWC boundary is on
    bool scatter = false;     // the batched gradient scatter (make_unpack_op): a plan with a comm stream hands it to that stream
    bool joins = true;        // backward: not issued before the side and branch streams have joined -- it may read what they write (the weight-gradient
                              // scratch, a bucket's gradients).  The safe default; the emitters of chain-only launches opt out (Builder::bc)
    double macs = 0.0;
};

struct GemmRef {              // what autotune iterates over
    awr_conv_args* ca = nullptr;
    awr_wgrad_args* wa = nullptr;
    std::string name;
    int tm = 0, tn = 0, tb = 0;
    float us = 0.f;
    bool tuned = false;
};

}  // namespace awrnet

typedef void (*awr_bucket_cb)(void* user, int64_t lo, int64_t hi, void* stream);

struct awr_plan {
    awr_net* net = nullptr;
    int B = 0, H = 0;
    bool training = false, det = false;
    awr_plan_modes modes{};                    // what the plan was built with (awr_plan_create_modes); every build-time decision reads these
    int bn_repeat = 1, n_buckets = 1;
    unsigned supervised = 0;
    std::vector<awrnet::Op> fwd, bwd, pack_ops;
    std::vector<awrnet::ConvLayer*> layers;               // layers whose packed copies this plan refreshes
    int n_wino = 0;      // forward (and weight-gradient) launches that run as Winograd F(2x2, 3x3)
    std::vector<std::pair<awrnet::ConvLayer*, float*>> wino_d;      // (layer, mirrored U[16][cout_pad][cin_pad])
    std::vector<std::pair<const awr_conv_args*, double>> wino_dg;      // candidate data-gradient launches (argument block, MACs): Winograd if the COMPLETED block is supported
    double wino_macs = 0;            // algorithmic multiply-adds of those launches (they execute 16 / 36 of them)
    std::vector<std::pair<awrnet::ConvLayer*, float*>> wino;      // ... and whose forward runs as Winograd F(2x2, 3x3): (layer, U[16][cin_pad][cout_pad])
    std::deque<awr_wino_args> wino_args;                  // argument blocks of those forward launches (stable addresses)
    std::vector<awrnet::DualLayer*> dual_layers;
    std::deque<awrnet::Tn> tensors;
    std::deque<awr_conv_args> cargs;
    std::deque<awrnet::FusedStats> fstats;      // (deque: stable addresses, the forward launches and bn_act share them)
    std::deque<awr_wgrad_args> wargs;
    std::vector<void*> owned;
    std::vector<std::pair<void*, size_t>> zero_init;   // atomic accumulators that must be zero before the first real step
    int64_t bytes = 0;
    float* img = nullptr;
    std::vector<float*> outputs, grad_outs;
    std::vector<awrnet::Tn*> head_preds;               // per stage: the head GEMM's NHWC output
    std::vector<float*> head_grads;            // per stage: NHWC buffer the backward reads d(pred) from (nullptr: second producer)
    bool nhwc_boundary = false;
    // wgrad split-K scratch arena
    float* scratch = nullptr;
    int64_t scratch_cap = 0;
    std::vector<awrnet::GemmRef> gemms;
    std::vector<awrnet::Range> buckets;
    bool built_bwd = false;
    // pack tables (device) for refresh_weights: [want_split][0 = forward layouts (+ dual layers), 1 = data-gradient layouts]
    void* pack_tab[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    int pack_njobs[2][2] = {{0, 0}, {0, 0}};
    int64_t pack_rows[2][2] = {{0, 0}, {0, 0}};
    bool pack_built[2] = {false, false};

    // streams
    std::vector<hipStream_t> side;
    std::vector<hipStream_t> branch;      // backward branches (an hourglass level's full-resolution skip residual)
    hipStream_t comm = nullptr;
    bool comm_owned = false;
    std::vector<hipEvent_t> events;
    size_t ev_next = 0;
    awr_bucket_cb bucket_cb = nullptr;
    void* bucket_user = nullptr;
    awr_dp* dp = nullptr;                 // native RCCL exchange of the buckets (awr_plan_set_dp)
    int dp_error = 0;
    unsigned long long dp_gen = 0;      // generation of the attached communicator (awr_dp_generation at awr_plan_set_dp)
    bool dp_lost = false;               // the attached communicator was destroyed under the plan: EVERY backward fails until awr_plan_set_dp is called again
    awr_bucket_cb saved_cb = nullptr;     // the host's callback while dp is attached
    void* saved_user = nullptr;
};

// ---- functions that cross the translation units ----------------------------------------------------------------------------------------
namespace awrnet {

int dev_alloc(std::vector<void*>& owner, size_t bytes, bool zero, void** out);      // awr_net.hip: hipMalloc (+ memset) owned by `owner`
void free_all(std::vector<void*>& v);
int upload_table(awr_plan& P, const void* host, size_t bytes, void** dev);          // awr_plan_run.hip: a host table copied to plan-owned device memory
void destroy_plan(awr_plan* p);
int min_k_steps(const awr_conv_args& a);                                            // awr_plan_build.hip: what bounds a launch's split-K depth

}  // namespace awrnet
