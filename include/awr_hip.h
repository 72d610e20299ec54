/*
 * awr_hip.h -- C ABI of libawr_hip.so: the MI355X (gfx950) implementation of the AWR hot path.
 *
 * The reference (Elody-07/AWR-Adaptive-Weighting-Regression) has no FFI layer: its hot path is
 * plain Python over torch ops.  Each entry point below therefore cites the reference Python
 * interface it replaces (file:line under the reference tree).  The Python host side in
 * awr-adaptive-weighting-regression_amd/ binds these with ctypes and mirrors the reference's
 * call surface (get_deconv_net, PoseNet, FeatureModule, My_SmoothL1Loss, Trainer step).
 *
 * Conventions
 *   - every function returns 0 on success, a negative code otherwise; awr_last_error() returns a
 *     thread-local description.  Nothing throws across the ABI.
 *   - all pointers are DEVICE pointers to fp32 unless stated; the caller owns every buffer.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).  One call = kernels enqueued
 *     on that stream; no call synchronises the device.
 *   - activations inside the backbone are NHWC; the reference-facing tensors (depth image, dense
 *     offset map, joints) keep the reference's NCHW / (B,J,3) layouts.
 */
#ifndef AWR_HIP_H
#define AWR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AWR_OK 0
#define AWR_ERR_ARG (-1)
#define AWR_ERR_HIP (-2)
#define AWR_ERR_UNSUPPORTED (-3)

/* BatchNorm statistic accumulators are [AWR_STAT_SLOTS][2][C] doubles: producers spread their atomics over
 * the slots (less L2 serialisation), awr_bn_finalize sums the slots and zeroes them.  Every entry point that touches
 * such an accumulator takes `nslots` (0 = AWR_STAT_SLOTS): the number of copies the caller allocated. */
#define AWR_STAT_SLOTS 16
/* upper bound of the workgroup count of awr_channel_stats / awr_bn_bwd_reduce launches */
#define AWR_REDUCE_MAX_BLOCKS 1024

/* Deterministic mode (process-wide flag, default 0 or $AWR_DETERMINISTIC): the library itself only stores it; callers
 * that see it set give every producer workgroup its OWN accumulator copy, which makes all results independent of the
 * order in which workgroups finish:
 *   - statistic accumulators ([nslots][2][C] doubles): pass nslots >= the producer's workgroup count (a single add onto a
 *     zeroed copy is exact); the finalize kernels sum the copies in a fixed order;
 *   - weight gradients: awr_wgrad_args.split_stride > 0 makes K-chunk y STORE its partial tile at R + y*split_stride
 *     (and its bias column sums at d_colsum + y*Cd) instead of atomically adding into R; awr_conv_wgrad_splits tells how
 *     many copies a launch writes and awr_unpack_job.slots sums them in order.
 * Cost: see DESIGN.md / profiles. */
int awr_set_deterministic(int on);
int awr_get_deterministic(void);

int awr_version(void);
const char* awr_last_error(void);
/* number of compute units / device name of the current device (diagnostics for bench.py) */
int awr_device_info(int* n_cu, int* clock_mhz, char* name, int name_len);

/* ------------------------------------------------------------------------------------------
 * AWR head.  offset: (B,4J,F,F) NCHW, channels [0,3J) unit offsets (joint-major, xyz-minor),
 * [3J,4J) closeness heat maps.  img: (B,1,H,H) normalised depth; the head samples img[b,0,y*H/F,
 * x*H/F] (nearest F.interpolate).  jt: (B,J,3).
 * -----------------------------------------------------------------------------------------*/

/* replaces FeatureModule.offset2joint_softmax (util/feature_tool.py:41-65).
 * stat (optional, B*J*2): per (b,j) softmax max-logit and sum-exp, consumed by the backward. */
int awr_head_forward(const float* offset, const float* img, int B, int J, int F, int H, float ks,
                     float* jt, float* stat, void* stream);

/* replaces autograd's backward of offset2joint_softmax (implicit in train.py:130).
 * g_offset (B,4J,F,F) = d(sum(jt*g_jt))/d(offset); accumulate!=0 adds into g_offset. */
int awr_head_backward(const float* offset, const float* img, const float* jt, const float* stat,
                      const float* g_jt, int B, int J, int F, int H, float ks, float* g_offset,
                      int accumulate, void* stream);

/* replaces FeatureModule.joint2offset (util/feature_tool.py:12-39): GT dense map (B,4J,F,F). */
int awr_joint2offset(const float* jt_gt, const float* img, int B, int J, int F, int H, float ks,
                     float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Losses.  My_SmoothL1Loss (model/loss.py:8-25) == Huber(delta) averaged over all elements.
 * Partial sums are accumulated in a device double (`acc`); the caller zeroes it (awr_zero_f64)
 * and reads it through awr_loss_finalize.  (In deterministic mode the 8 bytes hold a 2^-50 fixed-point
 * integer and the partials are added with integer atomics: order-independent.  Only
 * awr_loss_finalize may interpret `acc`.)
 * -----------------------------------------------------------------------------------------*/

/* acc[0] += weight * mean(huber(x-y)); gx (optional) = weight * clamp(x-y,+-delta)/n
 * (accumulate!=0 adds into gx).  Replaces criterion(x, y) + its autograd (train.py:125-130). */
int awr_huber(const float* x, const float* y, int64_t n, float delta, float weight, double* acc,
              float* gx, int accumulate, void* stream);

/* Fused GT-map synthesis + dense Huber forward + backward: never materialises the GT map.
 * Equivalent to weight*criterion(offset_pred, FM.joint2offset(jt_gt, img, ks, F)) and its
 * gradient w.r.t. offset_pred (train.py:113, :126, :130).  g_offset optional. */
int awr_dense_loss(const float* offset_pred, const float* jt_gt, const float* img, int B, int J,
                   int F, int H, float ks, float delta, float weight, double* acc, float* g_offset,
                   int accumulate, void* stream);

/* NHWC forms (round 3) for a host that keeps the dense map in the backbone's own layout: pred / grad are (B, F*F, Cp) rows, Cp = 4J
 * rounded up to 32 (channel 3j+c = offset component c of joint j, 3J+j = its heat map; padding channels zero), as awr_plan_head_nhwc
 * hands them out -- no NCHW transposes on either side of the loss.  scratch: awr_head_nhwc_scratch(B, J, F) floats.
 * awr_head_forward_nhwc = FeatureModule.offset2joint_softmax (util/feature_tool.py:41-65).
 * awr_head_loss_step_nhwc = train.py:118-127 in one call: joints + (max, sum) statistics, the coordinate Huber loss (acc[0] +=
 * coord_weight * mean) and, when coord_weight != 0, its gradient through the head; the fused GT map + dense Huber loss (acc[1] +=
 * dense_weight * mean; util/feature_tool.py:12-39, model/loss.py:8-25); the total gradient w.r.t. the dense map written (not
 * accumulated) to grad.  coord_weight == 0 reads the map once (one pass + a merge kernel), otherwise twice.  acc: two doubles the call
 * ADDS onto; they must be zero on entry -- zeroed once by the caller (awr_zero_f64), afterwards by awr_loss_finalize_reset, which reads
 * the losses out and re-arms the accumulator in the same launch (a step that fails between the two calls must zero acc itself). */
int64_t awr_head_nhwc_scratch(int B, int J, int F);
int awr_head_forward_nhwc(const float* pred, int Cp, const float* img, int B, int J, int F, int H, float ks, float* scratch,
                          float* jt, float* stat /* optional */, void* stream);
int awr_head_loss_step_nhwc(const float* pred, int Cp, const float* img, const float* jt_gt, int B, int J, int F, int H, float ks,
                            float delta, float coord_weight, float dense_weight, float* scratch, float* jt, float* stat,
                            float* g_jt /* needed when coord_weight != 0 */, double* acc, float* grad, void* stream);
/* awr_head_eval_nhwc = the loss of a scoring pass (test.py:73-86) next to its joints, in one read-only pass over the map: joints (+ the
 * optional (max, sum) statistics) exactly as awr_head_forward_nhwc writes them, acc[0] += coord_weight * mean Huber(joints - jt_gt),
 * acc[1] += dense_weight * mean Huber(pred - GT map), the GT map (util/feature_tool.py:12-39) computed on the fly as in
 * awr_head_loss_step_nhwc -- but no gradient: pred is only read, nothing of the size of the map is written.  Both means are over the first
 * n_valid images (0 <= n_valid <= B): the zero-padded tail of a ragged last batch gets its joints and adds nothing to acc (n_valid == 0: acc
 * is untouched; coord_weight == 0: acc[0] is untouched).  Geometry rules: awr_head_forward_nhwc's.  acc ACCUMULATES: a caller sums stages
 * (test.py:74-80) and batches on the device and reads the result with awr_loss_finalize / awr_loss_finalize_reset; the encoding of acc follows
 * the deterministic mode as in awr_head_loss_step_nhwc.  One streaming launch + the merge launch. */
int awr_head_eval_nhwc(const float* pred, int Cp, const float* img, const float* jt_gt, int B, int J, int F, int H, int n_valid,
                       float ks, float delta, float coord_weight, float dense_weight, float* scratch, float* jt,
                       float* stat /* may be NULL */, double* acc /* [0] += coord term, [1] += dense term */, void* stream);
/* Per-joint confidence and vote spread from the dense map: a second pass with the joints and the softmax statistics of a
 * head forward known.  In the reference's terms (util/feature_tool.py:57-63), for image b and joint j over the pixels i of the map:
 *   mask_i = img_i < 0.99,  h_i = offset_ht_i * mask_i,  w_i = softmax_i(30 h_i)                       (offset_ht_norm, :57-60)
 *   vote_i = offset_vec_i * mask_i * (ks - h_i * ks) + coords_i   (the summand of :63; jt = sum_i w_i vote_i is the head's output)
 *   conf   = sum_i w_i h_i                        the expected closeness under the aggregation weights
 *   var_c  = sum_i w_i (vote_i,c - jt_c)^2        c in {u, v, d}: the weighted scatter of the votes about the joint the head WROTE
 * conf (B, J, 4) fp32 = [conf, var_u, var_v, var_d] per (b, j), normalised crop units; every entry is a sum of non-negative terms.
 * jt (B, J, 3) and stat (B, J, 2) = (max logit, sum-exp) are the outputs of awr_head_forward / awr_head_forward_nhwc / awr_head_eval_nhwc on
 * the SAME map and image; stat[..., 0] / 30 is the largest masked heat value ("peak").  Read-only passes: nothing of the size of the map is
 * written.  No atomics: two runs on the same buffers give the same bits, in the deterministic mode and out of it.
 * awr_head_confidence_nhwc: pred (B, F*F, Cp) rows and scratch (awr_head_nhwc_scratch floats; may be the head forward's) under
 * awr_head_forward_nhwc's geometry rules; one streaming launch + a merge launch.  awr_head_confidence: the (B, 4J, F, F) layout, any J,
 * one workgroup per (b, j). */
int awr_head_confidence_nhwc(const float* pred, int Cp, const float* img, const float* jt, const float* stat, int B, int J, int F, int H,
                             float ks, float* scratch, float* conf /* (B, J, 4) */, void* stream);
int awr_head_confidence(const float* offset, const float* img, const float* jt, const float* stat, int B, int J, int F, int H, float ks,
                        float* conf /* (B, J, 4) */, void* stream);
/* What a caller reads next to a joint, rows [0, n_valid): conf (B, J) = conf4[..., 0]; peak (B, J) = stat[..., 0] / 30; spread_mm (B, J) =
 * sqrt(var_u (cube_x / 2)^2 + var_v (cube_y / 2)^2 + var_d (cube_z / 2)^2) with cube (B, 3) float32 millimetres as awr_detect_samples
 * writes it -- NOMINAL millimetres: the crop maps the cube onto [-1, 1].  status / ustatus (B) int32, each optional: a frame with a
 * non-zero code (awr_detect's, awr_joints_unproject's) gets NaN rows, like its joints.  One small launch. */
int awr_confidence_fields(const float* conf4, const float* stat, const float* cube, const int* status, const int* ustatus, int B, int J,
                          int n_valid, float* conf, float* peak, float* spread_mm, void* stream);
int awr_zero_f64(double* p, int64_t n, void* stream);
/* out[i] = (float)acc[i] for i<n, out[n] = sum -- e.g. {coord, dense, total} */
int awr_loss_finalize(const double* acc, int n, float* out, void* stream);
/* the same, and acc[0..n) is left zeroed: a step loop needs no awr_zero_f64 launch between steps */
int awr_loss_finalize_reset(double* acc, int n, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimiser: torch.optim.Adam defaults semantics (train.py:66-67, :131) over flat arenas.
 * g is multiplied by grad_scale first (1/world_size after the RCCL sum all-reduce).
 * -----------------------------------------------------------------------------------------*/
int awr_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                  void* stream);
/* SGD with momentum (train.py:68-69): buf = mom*buf + g (buf = g on step 1); p -= lr*buf */
int awr_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, float momentum,
                 float weight_decay, int64_t step, float grad_scale, void* stream);
/* The two rules above with a second gradient source and a scale that lives on the device.  g2 (may be NULL): the
 * gradient element is the float32 sum g[i] + g2[i].  dev_scale (may be NULL): one float on the device; the scale is the float32 product
 * grad_scale * dev_scale[0].  Nothing else differs: every form is one kernel body, and with both NULL the result is bit for bit what
 * awr_adam_step / awr_sgd_step write.  awr_adam_step_dev needs g2 16-byte aligned like the other arenas. */
int awr_adam_step_dev(float* p, const float* g, const float* g2, const float* dev_scale, float* m, float* v, int64_t n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale, void* stream);
int awr_sgd_step_dev(float* p, const float* g, const float* g2, const float* dev_scale, float* buf, int64_t n, float lr, float momentum,
                     float weight_decay, int64_t step, float grad_scale, void* stream);
/* Gradient accumulation: acc[i] = g[i] (first != 0: the first micro-step of a window) or acc[i] = acc[i] + g[i], one float32 add per
 * element.  Both arenas 16-byte aligned. */
int awr_grad_accumulate(float* acc, const float* g, int64_t n, int first, void* stream);
/* Weight EMA: ema[i] = ema[i] + (src[i] - ema[i]) * w for i < n: three float32 operations, each rounded on its own (no
 * contraction), the lerp form awr_adam_step uses for exp_avg.  src is only read.  w in (0, 1] (w = 1 copies src; an element with
 * src[i] == ema[i] keeps its bits for every w).  ema / src 16-byte aligned, n > 0, the ranges must not overlap; anything else -- a NULL
 * pointer, w outside (0, 1] or NaN included -- returns AWR_ERR_ARG before any launch.  Non-finite inputs are not guarded: a NaN or Inf in
 * src[i] or ema[i] makes ema[i] non-finite and it stays so. */
int awr_ema_update(float* ema, const float* src, int64_t n, float w, void* stream);
/* Global gradient norm and clip coefficient, left on the device (nothing synchronises):
 *   norm_out[0]  = (double)grad_scale * sqrt(sum_i (double)(float)(g[i] + g2[i])^2)      g2 may be NULL; the add is the float32 add the
 *                  optimiser kernel makes, the squares and the sum are float64
 *   scale_out[0] = 1.0f when max_norm <= 0 or +inf; otherwise, c = max_norm / (norm + 1e-6) in float64, c < 1 ? (float)c : 1.0f
 *                  (torch.nn.utils.clip_grad_norm_'s coefficient).  A norm that is not finite gives NaN, whatever max_norm is.
 * Two launches and no floating-point atomics: a grid that is a function of n alone writes one float64 partial per workgroup into
 * scratch (awr_grad_norm_scratch(n) bytes, at most 8 KB), one workgroup adds the partials in index order.  Two calls on the same input
 * leave bitwise equal results, and so do two data-parallel ranks that hold the same reduced gradient.  g / g2 16-byte aligned. */
int64_t awr_grad_norm_scratch(int64_t n);
int awr_grad_norm(const float* g, const float* g2, int64_t n, float grad_scale, double max_norm, double* scratch, double* norm_out,
                  float* scale_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backbone building blocks (replace the torch.nn modules used by model/resnet_deconv.py:19-215
 * and model/hourglass.py:6-165 and their autograd).  Activations NHWC fp32.
 * -----------------------------------------------------------------------------------------*/

/* Weight repack between the checkpoint layout W[d0][d1][T] (Conv2d: O,I,kh*kw; ConvTranspose2d:
 * I,O,kh*kw) and the GEMM layout P[n][T][ld] (K-contiguous rows, zero padded: n < n_pad rows,
 * ld >= inner extent).  transpose==0: P[d0][t][d1] = W[d0][d1][t]; transpose!=0: P[d1][t][d0]. */
int awr_pack_weight(const float* w, int d0, int d1, int T, int transpose, int n_pad, int ld,
                    float* packed, void* stream);
/* grad[d0][d1][t] (+)= P[d0][t][d1] (P has row length ld): wgrad GEMM output -> checkpoint layout */
int awr_unpack_wgrad(const float* packed, int d0, int d1, int T, int ld, float* grad, int accumulate,
                     void* stream);

/* Batched forms of the two calls above: ONE launch repacks / scatters every layer of a network, one workgroup
 * per row (pack: packed row of T*ld floats; unpack: gradient row of d1*T floats).  The descriptor tables live
 * in DEVICE memory (built once per plan); `first` is the running ROW offset of each job (`rows` rows per pack
 * job, d0 rows per unpack job), `total_rows` their sum = the number of workgroups.
 * LIMIT: T <= 255 in every job (the plans' largest is 16).  A row travels through an 8192-float LDS tile in chunks of
 * (8192 / (T | 1)) & ~31 columns; from T = 256 on that is ZERO columns and the chunk loop of the kernel never ends.  The
 * entry points cannot check it -- the table is in device memory -- so the caller that builds the table must. */
typedef struct awr_pack_job {
    const float* src;
    float* dst;
    void* split;          /* optional: split image of dst (awr_split_weight layout), written in the same pass */
    int d0, d1, T, transpose, rows, ld;
    int64_t first;
    int cols;             /* 0 = ld.  < ld: only columns [0, cols) of each ld-float line are written (two jobs fill one buffer side by side) */
    int reserved;
} awr_pack_job;
typedef struct awr_unpack_job {
    const float* packed;
    float* grad;
    int d0, d1, T, ld;
    int64_t first;
    int slots, slot_stride; /* slots > 1: the value is the sum of `slots` copies of the packed buffer, slot_stride floats apart */
} awr_unpack_job;
/* Split image of a packed weight buffer of n fp32 elements (n % 32 == 0) for the 6- / 9-product modes of awr_conv_gemm:
 * every 32-element K-slice becomes 192 bytes [h: 32 bf16 | m: 32 bf16 | l: 32 bf16] with x == h + m + l exactly
 * (truncating 8+8+8-bit cut of the fp32 significand).  Weights are split once per optimiser step instead of once per
 * workgroup that stages them.
 * DOMAIN of "exactly": x finite and a multiple of 2^-133, the smallest bf16 denormal -- in particular x == 0 and every
 * |x| >= 2^-110 (7.7e-34), FLT_MIN included (smaller values whose lowest set bit is 2^-133 or above are exact too).  Below that a residual x - h (or x - h - m) is an fp32 denormal whose bits
 * under 2^-133 no bf16 holds: the pieces then sum to x truncated toward zero to a multiple of 2^-133 (an fp32 denormal
 * below 2^-133 splits into three zeros).  No weight is that small; nothing is done about it. */
int awr_split_weight(const float* packed, void* split, int64_t n, void* stream);
int awr_pack_weights_batched(const awr_pack_job* jobs_dev, int njobs, int64_t total_rows, void* stream);
int awr_unpack_wgrads_batched(const awr_unpack_job* jobs_dev, int njobs, int64_t total_rows, void* stream);

/* Geometry of one implicit-GEMM convolution-like gather:
 *   out[b, qy*so+py, qx*so+px, n] = sum_{tap in phase} sum_c in[b, qy*si+dy, qx*si+dx, c] * P[n][wt][c]
 * conv kxk stride s pad p      : so=1, si=s, one phase, taps (dy,dx,wt)=(ky-p,kx-p,ky*k+kx)
 * transposed conv k4 s2 p1     : so=2, si=1, four phases (py,px), taps with (py+p-ky) even,
 *                                dy=(py+p-ky)/2 (likewise x), wt=ky*k+kx
 * Tensors must stay below 4 GB (the kernels use 32-bit buffer offsets with hardware bounds checking).
 * Built by the host (awr-adaptive-weighting-regression_amd/ops.py: ConvSpec.fwd_problem / dgrad_problem / wgrad_problem). */
typedef struct awr_phase {
    int py, px, ntaps;
    int32_t tap[16];   /* (dy & 0xff) | (dx & 0xff) << 8 | wt << 16 : one scalar load per K-slice */
} awr_phase;

typedef struct awr_conv_args {
    const float* in;        /* (B,Hin,Win,Cin) */
    const float* w;         /* packed P[n_pad][T][Cin] */
    float* out;             /* (B,Hout,Wout,N) */
    const float* in_scale;  /* optional per-input-channel affine applied while loading ...     */
    const float* in_shift;  /* ... in-bounds pixels only (padding stays 0)                       */
    const float* bias;      /* optional per-output-channel bias                                  */
    const float* out_scale; /* optional per-output-channel affine after bias (folded eval BN)    */
    const float* out_shift;
    const float* res;       /* optional tensor added element-wise, same shape as out            */
    double* stats;          /* optional [stat_slots][2][N]: += sum and sum of squares of the stored
                               value (taken after bias/affine/res, before relu_out)              */
    const float* bnr_y;     /* optional fused BatchNorm-backward reduction (data-gradient launches): the result v (after `res`) */
    const float* bnr_coef;  /* is d(loss)/d(relu(bn(y)));  with coef = [scale|shift|mean|invstd][N] the kernel stores */
                            /* g = v * (y*scale+shift > 0) and accumulates sum g, sum g*(y-mean)*invstd into `stats` */
    int B, Hin, Win, Cin;
    int Hq, Wq;             /* per-phase output grid */
    int Hout, Wout, N;
    int so, si, T;
    int relu_in, relu_out;
    int nphase;
    int tile_m, tile_n;     /* workgroup tile in units of 64 rows / 64 columns ({1,2} each); 0,0 = built-in heuristic.
                               Static plans autotune this per launch (engine.Plan.autotune). */
    awr_phase ph[4];
    const void* w_split;    /* split image of w (awr_split_weight); required when awr_get_gemm_products() != 1 */
    int stat_slots;         /* slot copies in `stats` (0 = AWR_STAT_SLOTS); workgroup i adds into copy (stat_slot_base + i) % stat_slots.
                               ceil(M/64)*ceil(N/64)*nphase copies (the 64x64 tile's workgroup count) = one per workgroup */
    int stat_slot_base;
    const float* in2;       /* optional second input (B,Hin,Win,Cin-Cin1) of a single-tap launch: K = [Cin1 channels of `in` | the channels of
                               `in2`], P rows [n][Cin] hold the two weight rows side by side; in_scale / in_shift / relu_in apply to `in` only.
                               out = W_a.in + W_x.in2: the hourglass residual's conv3 + skip_layer in one launch (FP32-MFMA mode only) */
    int Cin1;
    float* partial;         /* optional scratch of split_max * B*Hout*Wout*N floats: enables split-K (small launches whose few workgroups
                               would each walk a long K loop -- low-batch inference): blockIdx.z takes a contiguous range of the K
                               slices and stores its raw partial tile, a second kernel sums the copies in index order and applies the
                               launch's whole epilogue: bias, output affine, residual, ReLU, and -- training launches -- the `stats`
                               sums or the fused BatchNorm-backward reductions (bnr_y / bnr_act / in-place `res` / bnr2_y), exactly as
                               defined above, accumulated in fp64.  Reduce workgroup i (one per 64 output pixels x 64 channels) adds
                               into statistics copy (stat_slot_base + i) % stat_slots, one add per (slot, statistic, channel): with
                               stat_slots >= ceil(B*Hout*Wout / 64) * ceil(N / 64) (never more than the unsplit launch's 64x64-tile
                               workgroup count) every address receives exactly one add.  FP32-MFMA mode; no in2 / fused pair (w2) /
                               in_bnb_y / in_split, and every output pixel must belong to a phase (so == 1, or so * so phases).
                               With accum = 1 every K range is accumulated blocked and the sum over the copies is the outer fold;
                               a depth whose nominal range, ceil(slices / S), is shorter than one 128-k block is refused (see `accum`) */
    int split_k;            /* K ranges (1 = off, 0 = heuristic from the workgroup count and K depth), <= split_max */
    int split_max;
    const float* bnr_act;   /* with bnr_y: take the ReLU mask from this stored activation (act > 0) instead of re-deriving it from y -- the
                               BatchNorm whose output had a residual added before the ReLU (resnet_deconv.py:74-78).  `res` may then be
                               set as well: the launch is the LAST producer of the gradient, adds its tile onto the earlier
                               contributions, masks, reduces and stores the masked gradient in place */
    const float* bnr2_y;    /* with bnr_y: a SECOND BatchNorm whose output was added to the first one's before the ReLU (the ResNet downsample */
    const float* bnr2_coef; /* projection: a = relu(bn2(y) + bn_ds(y2))) shares the masked gradient g: also accumulate sum g, */
    double* stats2;         /* sum g*(y2-mean2)*invstd2 into stats2 (same slot geometry as `stats`); coef2 = [scale|shift|mean|invstd][N] */
    const float* w2;        /* optional: TWO convolutions in one launch (inference; FP32-MFMA mode).  The conv described above has N1 = 128 */
    const float* bias2;     /* or 64 output channels: bias / out_scale / out_shift / relu_out apply to THAT intermediate, which never leaves */
    int N1;                 /* the chip; a 1x1 conv with the packed weights w2 [N][1][N1 + N1x] follows, its epilogue takes bias2 and `res`; */
    int N1x;                /* `out` and N = 2 N1 describe the second conv's output.  N1x > 0: the second conv's K extent continues with N1x */
                            /* channels of `in2` at the same pixel (no `res` then).  hourglass.py:44-59: conv2 -> bn3 -> ReLU -> conv3 + skip */
                            /* (identity skip = `res`; skip conv = [W3 | Wskip] over [intermediate | block input]) */
    const float* in_bnb_y;  /* optional (data gradients): `in` is g = d(loss)/d(bn(y)) (ReLU mask already applied) of a BatchNorm whose backward is NOT */
    const float* in_bnb_coef; /* materialised; the GEMM input is d(y) = a1 g + a2 (y - mean) + a3 per channel with y = in_bnb_y (same shape as `in`) and */
                            /* coef = [a1 | a2 | a3 | mean][Cin] (awr_bn_bwd_finalize_lin), formed while the operand is fed to the matrix pipe; padding */
                            /* taps stay zero.  Replaces the awr_bn_bwd_apply pass between two dependent data-gradient GEMMs.  LDS-DMA staging only */
    int accum;              /* 0 = one k-ordered accumulation chain over the whole K extent (v_mfma_f32_32x32x2_f32 after v_mfma ...); 1 = BLOCKED: every */
                            /* 128 k the running sum is folded into a second accumulator set and restarted (chains of 128 + K / 128 terms, the */
                            /* rounding behaviour of oneDNN's blocked kernels that the reference's CPU numbers come from).  LDS-DMA staging, K > 256. */
                            /* A SPLIT-K launch (partial / split_k) honours accum = 1 in its own kernel: each K range folds every 128 k counted from its */
                            /* first slice, the ordered sum over the S copies is the outermost fold (chains of 128 + range / 128 + S terms).  Admissible */
                            /* while the NOMINAL range holds at least one whole 128-k block (ceil(slices / S) * 32 >= 128; the last range is what is left */
                            /* over and may be shorter -- a shorter chain): the split then adds no more outer terms than blocking itself has.  A depth that breaks the rule is an ERROR (never a silent downgrade to ordered sums); */
                            /* the heuristic depth (>= 8 slices per range) always satisfies it */
    const void* in_split;   /* optional (split-operand mode): the PRE-CUT image of `in` -- [pixel][Cin / 32][h | m | l][32] bf16, 6 bytes per element, written */
                            /* by awr_split_act (or a producer's epilogue): both operands then travel global -> LDS by DMA and the K loop holds no cutting */
                            /* arithmetic.  Excludes in_scale / relu_in (the producer applies them before it cuts), in2, in_bnb_y, split-K */
    float* pool_out;        /* optional: also write MaxPool2d(2, 2) of the launch's output, (B, Hout / 2, Wout / 2, N), bit-identical to awr_maxpool_fwd -- the */
                            /* workgroup tiles become 2D patches (two image rows x 32 / 64 columns) so that every window meets in the epilogue.  Accepted on a  */
                            /* fused pair (w2), or on a plain / two-tensor (in2) 1x1 launch: FP32-MFMA mode with LDS-DMA staging, one phase, one tap, stride 1, */
                            /* plain input (no in_scale / relu_in / in_bnb_y / in_split), plain epilogue (bias, optional res: no stats / bnr_y / output affine  */
                            /* / ReLU), accum = 0, no split-K (a resolved depth of 1).  Both need an even map height and a width that is a multiple of the      */
                            /* patch width (32 tile_m for the 1x1 form, with the tile the launch actually runs).  Anything else with pool_out set is an error:  */
                            /* it is never left unwritten.  model/hourglass.py:65-70: every level's input feeds up1 AND a pool                                  */
    int out_nt;             /* cache policy of the output stores and of the epilogue's operand loads (res / bnr_y / bnr_act): 0 = automatic, 1 = cached, */
                            /* 2 = streaming (`buffer_store ... nt`: a short-K launch's 32 KB tile per workgroup does not evict the operand lines the K loops */
                            /* of its neighbours still want -- DESIGN.md 4.2) */
} awr_conv_args;

/* conv / transposed conv forward and data-gradient (all are the same gather-GEMM).
 * Replaces nn.Conv2d / nn.ConvTranspose2d forward and their dgrad. */
int awr_conv_gemm(const awr_conv_args* a, void* stream);
#ifdef AWR_STUDY
/* STUDY BUILDS ONLY (-DAWR_STUDY; the default library does not export it): one of `nparts` equal batch parts of that launch (B % nparts == 0) --
 * the half-batch BatchNorm-backward wavefront of round 5 (AWR_HALF_BNB_MIN_ROWS), measured slower on every shape */
int awr_conv_gemm_part(const awr_conv_args* a, int nparts, int part, void* stream);
#endif
/* test hook: force the (TM,TN) in {1,2}^2 workgroup tile of awr_conv_gemm / awr_conv_wgrad
 * (0,0 = automatic choice).  Not for production use. */
int awr_debug_force_tile(int tm, int tn);
/* How awr_conv_gemm / awr_conv_wgrad form their fp32 products (process-wide; default 1, or $AWR_GEMM_PRODUCTS):
 *   1 = v_mfma_f32_32x32x2_f32 on fp32 operands (bit-equal to an fmaf chain);
 *   6 = every operand is cut EXACTLY into three bf16 pieces (x == h + m + l, 8+8+8 significand bits) and each fp32 product
 *       is formed from six of its nine bf16 x bf16 partial products on v_mfma_f32_32x32x16_bf16 -- each partial product
 *       exact, accumulated in fp32; the three dropped ones (m*l, l*m, l*l) weigh <= 2^-23 of the product, i.e. less than
 *       the rounding of the fp32 accumulation that both modes share.  16x faster matrix pipe, 6 passes: see DESIGN.md.
 * Replaces nothing in the reference (torch's conv precision is whatever cuDNN / oneDNN pick; cuDNN defaults to TF32). */
int awr_set_gemm_products(int n);
int awr_get_gemm_products(void);
#ifdef AWR_STUDY
/* STUDY BUILDS ONLY (-DAWR_STUDY; the default library exports neither this nor the kernel that reads awr_conv_args.in_split: 15-40 % slower than
 * the in-register cut, profiles/r05_split_mode_studies.txt).  Split image of an activation tensor x (npix, C), C % 32 == 0: every element [relu](x * scale[c] + shift[c]) (scale / shift optional) cut EXACTLY
 * into three bf16 pieces, element idx -> shorts (idx / 32) * 96 + idx % 32 + {0, 32, 64} (the format of awr_split_weight).  What awr_conv_args.in_split
 * reads: a BatchNorm + ReLU output that the FP32 mode never materialises is written ONCE here instead of being cut per (tap, column tile) in the GEMM. */
int awr_split_act(const float* x, const float* scale, const float* shift, int relu, int64_t npix, int C, void* split, void* stream);
#endif
/* the product mode awr_conv_wgrad runs in: awr_get_gemm_products(), unless $AWR_WGRAD_SPLIT=0 sends the split mode's weight gradients to the FP32-MFMA
 * kernels (a measured-slower study arm: profiles/r05_split_mode_studies.txt) */
int awr_get_wgrad_products(void);
/* How the FP32-MFMA forward / data-gradient GEMM stages its operands (process-wide; default 2, or $AWR_DMA):
 *   2 = LDS-DMA: `buffer_load_dwordx4 ... lds` straight into swizzled, unpadded LDS rows, 16-float stages, double-buffered
 *       (weights always; activations whenever no fused input affine / ReLU has to touch them on the way in);
 *   0 = global -> registers -> ds_write -> LDS (rounds 1-3; kept as the same-box A/B reference and for split-K / fused pairs).
 * Results are bit-identical between the two (same k order).  Replaces nothing in the reference. */
/* Launch-path study knobs (cached at load from $AWR_DEEP / $AWR_DEEP_1X1 / $AWR_FAST_STATS): "deep" = deep pipeline for small launches (1),
 * "deep_1x1" = ... for every single-tap launch (0), "fast_stats" = BatchNorm statistics summed from the accumulators (1).  Results are
 * bit-identical either way except the statistics' summation order ("fast_stats"); tests and same-box A/Bs only. */
int awr_debug_set_knob(const char* name, int value);
int awr_set_gemm_staging(int mode);
int awr_get_gemm_staging(void);
/* Accumulation order of the forward / data-gradient GEMMs of a plan.  awr_set_gemm_accum / awr_set_gemm_accum_auto set the process-wide DEFAULT
 * (2, or $AWR_ACCUM), which a plan created without a modes block captures (awr_plan_create, awr_plan_create_modes(..., NULL, ...)); a plan
 * created with one takes awr_plan_modes.accum / accum_auto_k / accum_auto_dgrad and never looks at the default.
 * 0 = ordered, 1 = blocked (awr_conv_args.accum), 2 = AUTO (the default): a plain FORWARD launch of a TRAINING plan (FP32-MFMA, LDS-DMA
 * staging, no fused pair / split-K: what the blocked kernel exists for) is blocked when its K extent (taps x input channels of its longest
 * phase) reaches min_k terms (default 576: every 3x3 convolution from 64 channels up and the transposed convolutions), everything else --
 * data gradients, evaluation plans -- is ordered.  Why this split: the joints a network returns are a function of its forward GEMMs only;
 * training-mode BatchNorm divides by batch statistics, which is where a long ordered chain's rounding error (it grows with the chain) gets
 * amplified, while eval-mode plans measure no difference (1.851e-4 mm from the oracle either way); and blocking costs a second accumulator
 * set (occupancy 4 -> 2-3 waves per SIMD on the 128x128 tile), +4.5 % on the ResNet18 step when every launch is blocked, +1.3 % for the
 * training forward alone (profiles/r06_accum_modes.txt) -- for which the joints of the two-image training-mode fixtures land CLOSER to
 * float64 than the fp32 oracle's own.  awr_set_gemm_accum_auto(min_k, dgrad): the threshold, and whether data-gradient launches follow the
 * same rule (default no).  Blocked = every launch the blocked kernel exists for: the parity mode (InferEngine(parity=True),
 * TrainEngine(accum="blocked")).  awr_resolve_gemm_accum: what a launch of that K extent and kind gets under the process-wide default (plan
 * builders apply the same rule to their plan's modes and store the result in awr_conv_args.accum, which itself only takes 0 / 1). */
#define AWR_GEMM_OTHER 0        /* evaluation-plan forward, fused pairs, anything else */
#define AWR_GEMM_FORWARD 1      /* forward launch of a training plan */
#define AWR_GEMM_DGRAD 2        /* data gradient */
int awr_set_gemm_accum(int mode);
int awr_get_gemm_accum(void);
int awr_set_gemm_accum_auto(int min_k, int dgrad);
int awr_get_gemm_accum_auto(int* min_k, int* dgrad);
int awr_resolve_gemm_accum(int k_extent, int kind);
/* the split-K depth awr_conv_gemm runs the launch `a` with (1 = unsplit): the explicit split_k, or the heuristic from the workgroup count and the K
 * depth -- a pure function of the argument block and the process-wide modes; the same errors as awr_conv_gemm for a depth the launch cannot honour */
int awr_conv_split_depth(const awr_conv_args* a, int* depth);
/* Split-K for TRAINING plans (awr_plan_modes.train_split_k; awr_set_train_split_k sets the process-wide default -- 0, or $AWR_TRAIN_SPLIT_K -- that a plan
 * created without a modes block captures): 1 = the forward and data-gradient launches
 * of a training plan that have few workgroups and a long K loop (64x64-tile workgroups x phases well below two per CU, at least 8 K slices per
 * range) get `partial` scratch (capped per launch, counted in awr_plan_info's bytes) and run split: the BatchNorm statistics / fused
 * BatchNorm-backward reductions then come from the reduce kernel (awr_conv_args.partial).  awr_plan_autotune times depth 1 against the split depths
 * per launch; deterministic plans take the heuristic depth.  Launches taken by a Winograd form, fused pairs, in2 / in_bnb_y launches, partial-coverage
 * data gradients and the split-operand product mode stay unsplit.  0: a plan is launch-for-launch what it was without the mode.  Replaces nothing in the
 * reference (a scheduling choice for its batch_size = 32 default, train.py). */
int awr_set_train_split_k(int on);
int awr_get_train_split_k(void);

/* weight gradient:  R[cd][t][cg] += sum_m D[m][cd] * G[pix(m,t)][cg]
 * D: dense operand (B,Hd,Wd,Cd); G: gathered operand (B,Hg,Wg,Cg) read at (y*sg+dy[t], x*sg+dx[t]).
 * conv wgrad: D=dY, G=X, (dy,dx)=(ky-p,kx-p), sg=stride -> R == packed [Cout][T][Cin].
 * deconv wgrad: D=X, G=dY, sg=2 -> R == [Cin][T][Cout].  R (row length ld>=Cg) must be zeroed by
 * the caller; split-K partial sums are combined with fp32 atomics. */
typedef struct awr_wgrad_args {
    const float* D;
    const float* G;
    float* R;
    const float* d_scale;   /* optional per-channel affine (+ReLU) applied to D / G while staging: the operand is */
    const float* d_shift;   /* then relu(t*scale+shift) of the stored tensor, i.e. a BatchNorm+ReLU output that  */
    const float* g_scale;   /* was never materialised (zero padding of the gather stays zero)                    */
    const float* g_shift;
    float* d_colsum;        /* optional [AWR_STAT_SLOTS][Cd]: slot copies whose SUM += column sums of D over all pixels (for conv
                               wgrad, D = dY, this IS the bias gradient -- it falls out of the slices the kernel stages anyway);
                               zeroed by the caller.  Slots: hundreds of workgroups add to the same Cd addresses */
    int d_relu, g_relu;
    int B, Hd, Wd, Cd, Hg, Wg, Cg, sg, T, ld;
    int tile_m, tile_n;     /* (cd, cg) tile in units of 64; 0,0 = heuristic */
    int target_blocks;      /* split-K: aim for this many workgroups; 0 = heuristic */
    int algo;               /* 0 = automatic; 1 = one workgroup per (tap, channel tile, pixel chunk); 2 = one WAVE per tap: a
                               workgroup owns a 64x64 channel tile for all taps and stages D / halo'd G patches once
                               (3x3 stride 1/2 and 4x4 stride-2 filters on power-of-two maps); 3 = one workgroup per KERNEL ROW: the three
                               taps of a row share the staged D pixels and one halo'd G row segment, three accumulators per wave, operands by
                               LDS-DMA (3x3 stride-1 filters, power-of-two maps at least 8 wide, D without a fused affine) */
    int8_t dy[16], dx[16];
    int64_t split_stride;   /* 0: split-K partial sums are combined with atomics in R.  > 0 (deterministic mode): K-chunk y stores its
                               tile at R + y*split_stride floats and its column sums at d_colsum + y*Cd; nothing needs zeroing */
    int max_split;          /* with split_stride: number of copies the caller allocated (caps the split-K depth) */
} awr_wgrad_args;
int awr_conv_wgrad(const awr_wgrad_args* a, void* stream);
/* 1 if awr_wgrad_args.algo = `algo` serves this geometry in the current product / staging mode (what a tuner may try), else 0 */
int awr_conv_wgrad_algo_ok(const awr_wgrad_args* a, int algo);
/* number of K-chunk copies the launch described by `a` writes (split_stride mode) */
int awr_conv_wgrad_splits(const awr_wgrad_args* a, int* nsplit);

/* Fused stems: conv 5x5 pad 2 of the one-channel depth image (1 -> 64 channels) -> BatchNorm -> ReLU [-> MaxPool(3,2,1)], their
 * autograd and the BatchNorm's running-stat update.  ResNet18-deconv (model/resnet_deconv.py:31-36, :118-121): no conv bias, pooled;
 * stacked hourglass (model/hourglass.py:112, Conv(1, 64, 5, 1, bn=True, relu=True)): conv bias, no pooling.  The un-normalised
 * full-resolution conv output is NEVER written: every kernel recomputes it from the image on the FP32 matrix pipe.  img (B,1,H,W),
 * H and W multiples of 16; w = the conv weight in checkpoint layout [64][25]; bias [64] or NULL; all maps NHWC.
 *   awr_stem_stats       stats[nslots][2][64] += per-channel sum / sum of squares of conv + bias
 *                        (feed awr_bn_finalize with count = B*H*W)
 *   awr_stem_pool        pooled (B,H/2,W/2,64) = maxpool(relu(conv * scale + shift)); argmax (optional, training) = window code
 *                        ky*3+kx of the first maximum, the format awr_maxpool_fwd writes
 *   awr_stem_conv        out (B,H,W,64) = [relu]((conv + bias) * scale + shift)
 *   awr_stem_bwd_reduce  sums[nslots][2][64] += sum g, sum g*xhat with g = relu' * dg; coef4 = [scale|shift|mean|invstd][64] of the
 *                        forward (feed awr_bn_bwd_finalize).  argmax != NULL: dg is the gradient of the POOLED map, routed through
 *                        the max-pool backward; argmax == NULL: dg is the dense gradient of awr_stem_conv's output
 *   awr_stem_bwd_wgrad   grad[64][25] = sum_pixels dY * image taps, gbias[64] (optional) = sum_pixels dY, dY = BatchNorm backward of
 *                        g with bwd_coef = [mean g | mean g*xhat | gamma*invstd][64]; dw_slots: nslots*64*26 floats of scratch,
 *                        zero before the first call (the call re-arms it) */
int awr_stem_stats(const float* img, const float* w, const float* bias, int B, int H, int W, double* stats, int nslots,
                   void* stream);
int awr_stem_pool(const float* img, const float* w, const float* scale, const float* shift, int B, int H, int W,
                  float* pooled, uint8_t* argmax, void* stream);
int awr_stem_conv(const float* img, const float* w, const float* bias, const float* scale, const float* shift, int relu,
                  int B, int H, int W, float* out, void* stream);
int awr_stem_bwd_reduce(const float* img, const float* w, const float* bias, const float* coef4, const float* dg,
                        const uint8_t* argmax, int B, int H, int W, double* sums, int nslots, void* stream);
int awr_stem_bwd_wgrad(const float* img, const float* w, const float* bias, const float* coef4, const float* bwd_coef,
                       const float* dg, const uint8_t* argmax, int B, int H, int W, float* dw_slots, float* grad,
                       float* gbias, int nslots, void* stream);
/* workgroup counts of awr_stem_stats / awr_stem_bwd_reduce (stats_slots) and of awr_stem_bwd_wgrad (wgrad_slots, also the
 * number of 64*26-float copies in dw_slots): that many slot copies = one per workgroup.  nslots = 0 means AWR_STAT_SLOTS. */
int awr_stem_slots(int B, int H, int W, int* stats_slots, int* wgrad_slots);

/* 5x5 stem (Cin=1): im2col of the depth image into (B,H,W,32) rows (25 taps + 7 zeros) so the
 * stem conv and its wgrad run on the same MFMA GEMMs (resnet_deconv.py:32, hourglass.py:112). */
int awr_stem_im2col(const float* img, int B, int H, int W, float* cols, void* stream);

/* BatchNorm2d (training): stats -> (scale, shift, mean, invstd) + running-stat update
 * (momentum, unbiased running var); zeroes `stats` afterwards.  nn.BatchNorm2d forward, train. */
int awr_bn_finalize(double* stats, int C, int64_t count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps,
                    float* scale, float* shift, float* mean, float* invstd, int nslots, void* stream);
/* eval-mode fold: scale = gamma/sqrt(var+eps), shift = beta - mean*scale */
int awr_bn_fold_eval(int C, const float* gamma, const float* beta, const float* running_mean,
                     const float* running_var, float eps, float* scale, float* shift, void* stream);
/* per-channel sum / sum of squares of an NHWC tensor (for BNs whose input is not a conv output);
 * stats is [AWR_STAT_SLOTS][2][C] like the conv epilogue's */
int awr_channel_stats(const float* x, int64_t npix, int C, double* stats, int nslots, void* stream);
/* awr_maxpool_fwd / awr_upsample2_add that ALSO accumulate the per-channel sum and sum of squares of the tensor they write (the slot layout of
 * awr_channel_stats): the BatchNorm that follows needs no statistics pass of its own over that tensor (model/hourglass.py:62-88: every pooled /
 * up-sampled-and-added map enters a pre-activation residual) */
int awr_maxpool_fwd_stats(const float* x, const float* in_scale, const float* in_shift, int in_relu, int B, int H, int W, int C, int k, int s, int p,
                          float* out, uint8_t* argmax, double* stats, int nslots, void* stream);
int awr_upsample2_add_stats(const float* up1, const float* low, int B, int Hl, int Wl, int C, float* out, double* stats, int nslots, void* stream);
/* out = [relu]( x*scale[c] + shift[c] [+ res] ) */
int awr_bn_apply(const float* x, const float* scale, const float* shift, const float* res, int relu,
                 float* out, int64_t npix, int C, void* stream);
/* backward pass 1: g = dout * relu_mask ; sums[slot][0][c] += sum g ; sums[slot][1][c] += sum g*xhat
 * (sums is [AWR_STAT_SLOTS][2][C] doubles, zero before the first use; pass 2 re-arms it).
 * relu_mask: (act > 0) if act is given; (y*mask_scale+mask_shift > 0) if mask_scale/shift are given (the
 * activation is re-derived from y with the forward's scale/shift: no read of the activation tensor); else 1. */
int awr_bn_bwd_reduce(const float* dout, const float* act, const float* y, const float* mean,
                      const float* invstd, const float* mask_scale, const float* mask_shift, int64_t npix,
                      int C, double* sums, int nslots, void* stream);
/* backward pass 2: dy = gamma*invstd*(g - sum_g/n - xhat*sum_gx/n) [+ dy_add]; optional g_out = g
 * (residual branch); dgamma/dbeta (+)= sums (accumulate); zeroes sums afterwards.  dy may alias
 * dy_add or dout.  coef: 3*C floats of scratch (per-channel coefficients collapsed from the slots). */
int awr_bn_bwd_apply(const float* dout, const float* act, const float* y, const float* mean,
                     const float* invstd, const float* gamma, const float* mask_scale,
                     const float* mask_shift, double* sums, float* coef, int64_t npix, int C,
                     float* dy, const float* dy_add, float* g_out, float* dgamma, float* dbeta,
                     int accumulate, int nslots, void* stream);
/* first half of awr_bn_bwd_apply on its own: collapse the slot-spread sums into coef = [mean g | mean g*xhat |
 * gamma*invstd][C], emit dgamma / dbeta, zero the sums (for fused consumers such as awr_stem_bwd_wgrad) */
int awr_bn_bwd_finalize(double* sums, int C, int64_t count, const float* gamma, const float* invstd, float* coef,
                        float* dgamma, float* dbeta, int accumulate, int nslots, void* stream);
/* awr_bn_bwd_finalize that ALSO writes lin4 = [a1 | a2 | a3 | mean][C] with d(y) = a1 g + a2 (y - mean) + a3: the form a consumer GEMM evaluates
 * on the fly (awr_conv_args.in_bnb_y / in_bnb_coef) when d(y) is not written to HBM on the critical chain.  Same reference lines as above. */
int awr_bn_bwd_finalize_lin(double* sums, int C, int64_t count, const float* gamma, const float* mean, const float* invstd, float* coef,
                            float* lin4, float* dgamma, float* dbeta, int accumulate, int nslots, void* stream);
/* second half of awr_bn_bwd_apply on its own: d(y) from coef (awr_bn_bwd_finalize / _lin), no reduction, no parameter gradients */
int awr_bn_bwd_apply_only(const float* dout, const float* act, const float* y, const float* mean, const float* invstd,
                          const float* mask_scale, const float* mask_shift, const float* coef, int64_t npix, int C, float* dy,
                          const float* dy_add, float* g_out, void* stream);
/* plain ReLU backward / mask: g = dout * (act > 0) */
int awr_relu_bwd(const float* dout, const float* act, float* g, int64_t n, void* stream);
/* out = a + b (n elements); out may alias a */
int awr_add(const float* a, const float* b, float* out, int64_t n, void* stream);
/* per-channel bias gradient: db[c] (+)= sum over pixels dy[pix][c] */
int awr_bias_grad(const float* dy, int64_t npix, int C, float* db, int accumulate, void* stream);

/* MaxPool2d(k,s,p) NHWC forward (+ uint8 argmax) and backward; nn.MaxPool2d(3,2,1)/(2,2).
 * in_scale/in_shift (optional): pool relu(x*scale+shift) instead of x (fused BatchNorm+ReLU input). */
int awr_maxpool_fwd(const float* x, const float* in_scale, const float* in_shift, int in_relu, int B, int H,
                    int W, int C, int k, int s, int p, float* out, uint8_t* argmax, void* stream);
int awr_maxpool_bwd(const float* dout, const uint8_t* argmax, int B, int H, int W, int C, int k,
                    int s, int p, float* dx, int accumulate, void* stream);
/* hourglass.py:88: out = up1 + nearest_upsample2(low)  and its backward (dlow = 2x2 sums of dout) */
int awr_upsample2_add(const float* up1, const float* low, int B, int Hl, int Wl, int C, float* out,
                      void* stream);
int awr_upsample2_bwd(const float* dout, int B, int Hl, int Wl, int C, float* dlow, int accumulate,
                      void* stream);

/* layout bridges at the reference boundary: NHWC (C padded to Cp) <-> NCHW (C channels) */
int awr_nhwc_to_nchw(const float* in, int B, int P, int Cp, int C, float* out, void* stream);
int awr_nchw_to_nhwc(const float* in, int B, int P, int Cp, int C, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Network-level API: the two backbones as natively built and replayed static plans.
 * Replaces get_deconv_net(18, J, downsample) / PoseNet('hourglass_<n>', J) construction, forward and
 * autograd backward (model/resnet_deconv.py:8-16,:19-136,:145-174; model/hourglass.py:6-165;
 * train.py:52-58, :116-130).  The Python host keeps only the nn.Module shell (state_dict views,
 * autograd hook, optimiser plumbing).
 *
 * Ownership: the caller owns the parameter / gradient / BatchNorm-buffer arenas (awr_net_bind) and
 * the boundary tensors handed to awr_plan_create (depth batch, NCHW dense maps and their gradients);
 * the library owns packed weights, activations, gradients and scratch (freed by *_destroy).  Calls
 * on one net / plan come from one host thread.
 * -----------------------------------------------------------------------------------------*/
typedef struct awr_net awr_net;
typedef struct awr_plan awr_plan;

/* kind 0: ResNet-deconv -- `nstack` carries the depth: 18 (also 0 / 1; BasicBlock) or 50 / 101 / 152 (Bottleneck), resnet_deconv.py:9-13;
 * kind 1: stacked hourglass (downsample ignored, feature size H/2).
 * Creates the checkpoint layout only: no device memory is touched until awr_net_bind. */
int awr_net_create(int kind, int nstack, int J, int downsample, awr_net** out);
int awr_net_destroy(awr_net* net);
/* state_dict entries (parameters, running stats, counters) in the reference's order; arena sizes in floats.
 * [0, n_active) of the parameter arena receives gradients; the tail holds hourglass skip_layers that never run */
int awr_net_sizes(const awr_net* net, int64_t* n_tensors, int64_t* n_params, int64_t* n_active,
                  int64_t* n_buffers, int* n_counters, int* nstage);
/* entry i: torch key, kind (0 conv weight OIHW, 1 transposed-conv weight IOHW, 2 conv bias, 3 BN weight, 4 BN bias,
 * 5 running_mean, 6 running_var, 7 num_batches_tracked), shape, offset in floats into the parameter arena (kinds 0-4)
 * or the buffer arena (5, 6), counter index (7); unused = never receives a gradient */
int awr_net_tensor_info(const awr_net* net, int64_t i, const char** key, int* kind, int* ndim,
                        int64_t shape[4], int64_t* offset, int* unused);
/* attach 16-byte aligned device arenas (n_params, n_params, n_buffers floats); destroys the net's plans */
int awr_net_bind(awr_net* net, float* params, float* grads, float* buffers);

/* One static plan for (B, H, mode).  img (B,1,H,H); outs[stage] (B,4J,F,F) NCHW dense maps; grad_outs[stage] their
 * gradients (training plans; zero the stages you do not supervise).  supervised_mask: bit s = stage s receives a
 * gradient (hourglass training supervises the last stage only, train.py:116-121); bn_repeat: BatchNorm momentum is
 * applied that many times per forward (the reference runs `stacks` forwards per iteration); n_buckets > 1: the backward
 * hands out gradient-arena ranges through the bucket callback as soon as they are final. */
int awr_plan_create(awr_net* net, int B, int H, int training, unsigned supervised_mask, int bn_repeat,
                    int n_buckets, float* img, float* const* outs, float* const* grad_outs, awr_plan** out);
/* The build modes of ONE plan: passed in, stored in the plan, and read from the plan by every decision its builder takes.
 * NOT in the block, because the launch dispatchers (awr_conv_gemm, awr_conv_wgrad, the head and loss kernels) read them at every launch and not
 * only the builder, so a per-plan value would have to travel in awr_conv_args / awr_wgrad_args: the product mode (awr_set_gemm_products), the
 * staging mode (awr_set_gemm_staging), the deterministic mode (captured from the process when the plan is created; awr_plan_info reports it)
 * and the awr_debug_set_knob knobs.  For the same reason bits 4 and 8 of `winograd` decide a plan's launch LIST from this block, while
 * awr_wino_conv still picks its tile form (64-channel or not) from the process-wide code when it launches (awr_wino_args has no field for it). */
typedef struct awr_plan_modes {
    int accum;             /* 0 ordered, 1 blocked, 2 auto  (awr_set_gemm_accum) */
    int accum_auto_k;      /* accum == 2: K extent from which a launch blocks (>= 256, awr_set_gemm_accum_auto) ... */
    int accum_auto_dgrad;  /* ... forward launches only (0) or data gradients too (1) */
    int winograd;          /* code of awr_set_conv_winograd, 0 ... 15 */
    int train_split_k;     /* 0 / 1 (awr_set_train_split_k); ignored by evaluation plans */
} awr_plan_modes;
/* awr_plan_create with the plan's modes given by the caller; modes == NULL: the process-wide defaults, which is what awr_plan_create passes.
 * The block is validated (the setters' ranges) before anything else. */
int awr_plan_create_modes(awr_net* net, int B, int H, int training, unsigned supervised_mask, int bn_repeat, int n_buckets,
                          float* img, float* const* outs, float* const* grad_outs, const awr_plan_modes* modes, awr_plan** out);
int awr_plan_destroy(awr_plan* plan);
int awr_plan_info(const awr_plan* plan, int64_t* bytes, int* deterministic, int* n_fwd, int* n_bwd,
                  int* n_buckets, int* n_gemm, int* n_bn);
/* forward and data-gradient launches of the plan that run as Winograd F(2x2, 3x3) (awr_set_conv_winograd): how many, and their ALGORITHMIC multiply-adds per replay
 * (the matrix pipe executes 16 / 36 of them) */
int awr_plan_winograd(const awr_plan* plan, int* n, double* macs);
int awr_plan_bucket(const awr_plan* plan, int i, int64_t* lo, int64_t* hi, int* ready_op);
/* op i of the forward (list 0) / backward (list 1) launch list: name, algorithmic MACs (GEMM-family launches),
 * flags bit 0 = weight gradient that may run on a side stream, bit 1 = conv / stem family (the launches a roofline is quoted for),
 * bit 2 = the batched gradient scatter (a plan with a comm stream hands it to that stream), bit 3 = a backward replay joins the side and
 * branch streams before it issues this op (set unless the op's emitter declared it chain-only; forward replays ignore it) */
int awr_plan_op(const awr_plan* plan, int list, int i, const char** name, double* macs, int* flags);
/* parity / debugging introspection: activation tensor i of the plan in build order (i past the end returns AWR_ERR_ARG): name
 * ("<layer>.out" = a conv's raw output, "<bn>.act" = a materialised BatchNorm(+ReLU) output, "<bn>.act(lazy)" = one that is never
 * written, ...), NHWC dims {B,H,W,C}, the value buffer and, after a backward replay, its gradient buffer (NULL if none; identity skips
 * alias the buffer of the tensor they come from).  lazy != 0: the handle stands for buf * scale[c] + shift[c] (2: with a ReLU on top) of
 * ANOTHER tensor's buffer, applied by the consumers' loaders; lz_scale / lz_shift are those per-channel coefficients. */
int awr_plan_tensor(const awr_plan* plan, int i, const char** name, int dims[4], float** buf, float** grad, int* lazy,
                    const float** lz_scale, const float** lz_shift);
/* NHWC boundary (round 3): stage s's dense map as the head GEMM leaves it, (B, F*F, Cp) rows, and -- training plans, supervised stages
 * -- the buffer the backward reads its gradient from (NULL when that stage's gradient has a second producer and must go through
 * grad_outs).  awr_plan_set_nhwc_boundary(plan, 1): the plan stops transposing to / from the NCHW boundary tensors (outs / grad_outs are
 * then neither written nor read): the caller runs awr_head_forward_nhwc / awr_head_loss_step_nhwc on these buffers between
 * awr_plan_forward and awr_plan_backward.  Refused (AWR_ERR_UNSUPPORTED) when a supervised stage has no NHWC gradient buffer. */
int awr_plan_head_nhwc(const awr_plan* plan, int stage, const float** pred, float** grad, int* Cp);
int awr_plan_set_nhwc_boundary(awr_plan* plan, int on);
/* n_side extra HIP streams (weight gradients in the backward, forked branches in the forward); comm != 0 adds the
 * stream buckets are handed to */
int awr_plan_set_streams(awr_plan* plan, int n_side, int comm);      /* n_side in 0..4 */
typedef void (*awr_bucket_cb)(void* user, int64_t lo, int64_t hi, void* stream);
/* cb(user, lo, hi, stream): grads[lo, hi) is final in `stream` order -- start its all-reduce there */
int awr_plan_set_bucket_callback(awr_plan* plan, awr_bucket_cb cb, void* user);
/* The library's side / branch streams come from ONE process-wide pool, ordered by a probe (a 100 us spin kernel on two streams at once):
 * the first n_independent streams share a hardware queue neither with the null stream nor with each other -- HIP multiplexes streams onto
 * a few hardware queues and streams on one queue serialise, so which streams a plan gets decides whether its side streams overlap anything.
 * Built on first use (a few milliseconds, synchronises the device once). */
int awr_stream_pool_info(int* n_streams, int* n_independent);
/* repack every conv weight (and re-fold eval BatchNorms) from the arena; forward; backward */
int awr_plan_refresh_weights(awr_plan* plan, void* stream);
int awr_plan_forward(awr_plan* plan, void* stream);
int awr_plan_backward(awr_plan* plan, void* stream);
/* serial replay with a HIP-event pair around every launch: ms[i] per op, 0 for fills / copies / markers (synchronises the stream) */
int awr_plan_run_timed(awr_plan* plan, int list, void* stream, float* ms);
/* time the tile / split-K candidates of every GEMM launch in place (no-op in deterministic mode); read / preset choices
 * (target_blocks: weight gradients = workgroup target of the split over pixels; conv launches with `partial` scratch = split-K depth -- the tuned
 * one, or, before / without tuning, the depth the heuristic gives the launch: awr_conv_split_depth) */
int awr_plan_autotune(awr_plan* plan, int reps, void* stream);
int awr_plan_gemm(const awr_plan* plan, int i, const char** name, int* tile_m, int* tile_n, int* target_blocks,
                  float* us, int* tuned);
int awr_plan_set_gemm(awr_plan* plan, int i, int tile_m, int tile_n, int target_blocks, float us);
/* ... and the algorithm of a weight-gradient launch (awr_wgrad_args.algo: 0 automatic, 1 workgroup per tap, 2 wave per tap, 3 workgroup
 * per kernel row; always 0 for conv launches): what a tuning cache stores beside the tile.  set: AWR_ERR_ARG if the launch cannot run it. */
int awr_plan_gemm_algo(const awr_plan* plan, int i, int* algo);
int awr_plan_set_gemm_algo(awr_plan* plan, int i, int algo);

/* ------------------------------------------------------------------------------------------
 * Data-parallel API (net-new w.r.t. the reference, which hard-wires one GPU: train.py:29,:233).
 * One process per GPU.  The library opens librccl.so at run time (dlopen; AWR_RCCL_LIB overrides the path) -- libawr_hip.so has
 * no link-time dependency on RCCL and a host that exchanges gradients itself (awr_plan_set_bucket_callback) never loads it.
 *   rank 0:      awr_dp_unique_id(id)            -> ship the 128 bytes to the other ranks out of band (file, socket, MPI, ...)
 *   every rank:  awr_dp_init(rank, world, id, &dp)   (collective; the communicator lives on the CURRENT device)
 *                awr_dp_broadcast(dp, params, n, 0, stream) / (..., bn_buffers, ...): identical replicas
 *                awr_plan_set_dp(plan, dp): awr_plan_backward all-reduces (SUM) every gradient bucket as soon as it is final -- on the
 *                communicator's own stream, behind the bucket's scatter, overlapping the rest of the backward -- and returns with the
 *                caller's stream ordered after all of them; pass grad_scale = 1/world to awr_adam_step / awr_sgd_step.
 * BatchNorm statistics stay rank-local (what stock DDP does).  awr_dp_allreduce / awr_dp_broadcast order themselves behind `stream`
 * and run on the communicator's stream; awr_dp_wait(dp, stream) orders `stream` behind everything issued so far.
 * -----------------------------------------------------------------------------------------*/
#define AWR_DP_ID_BYTES 128
typedef struct awr_dp awr_dp;
int awr_dp_available(int* version, const char** path);          /* AWR_OK if librccl.so and its symbols were found */
int awr_dp_unique_id(void* id128);
int awr_dp_init(int rank, int world, const void* id128, awr_dp** out);
int awr_dp_destroy(awr_dp* dp);
int awr_dp_info(const awr_dp* dp, int* rank, int* world, int* device);
int awr_dp_allreduce(awr_dp* dp, float* buf, int64_t n, void* stream);               /* in place, SUM */
int awr_dp_broadcast(awr_dp* dp, float* buf, int64_t n, int root, void* stream);     /* in place */
int awr_dp_wait(awr_dp* dp, void* stream);
/* dp != NULL: the plan's gradient buckets (n_buckets of awr_plan_create; 1 = one exchange after the backward) go through `dp`;
 * NULL detaches.  Replaces the bucket callback while set.  Lifetime: the plan keeps the pointer, not a reference -- detach (NULL) before
 * awr_dp_destroy; a backward that finds its communicator destroyed fails with AWR_ERR_ARG instead of calling into it. */
int awr_plan_set_dp(awr_plan* plan, awr_dp* dp);

/* ------------------------------------------------------------------------------------------
 * Winograd F(2x2, 3x3) on the FP32 matrix pipe (round 6, csrc/awr_wino.hip): stride-1 pad-1 3x3 convolutions with 2.25x fewer multiplies than the
 * direct implicit GEMM -- nn.Conv2d(C, N, 3, 1, 1) of model/resnet_deconv.py:139-142,:161-165 / model/hourglass.py:35.
 *   U[pos][c][n] = (G g G^T)[pos]            awr_wino_weights: from the checkpoint tensor (OIHW), once per optimiser step; mirror != 0 = the
 *                                            data-gradient form (N = the layer's Cin, C = its Cout)
 *   V = B^T d B per 4x4 input window, M[pos] = sum_c V U (16 independent GEMMs on v_mfma_f32_32x32x2_f32), Y = A^T M A per 2x2 output patch
 * awr_wino2_conv3x3: out (B, H, W, N) = conv([relu](in * in_scale + in_shift)) [+ bias] [ReLU], NHWC; the raw input tile of a workgroup (a 2-D
 * block of 64 patches of one image, or several small images) is staged in LDS once per K stage, padding stays zero under the fused input affine;
 * `stats` (optional) += per-channel sum / sum of squares of the stored output ([nslots][2][N] doubles, awr_bn_finalize's layout).  Power-of-two map
 * sizes >= 4, C % 8 == 0, N % 32 == 0, fewer than 2^31 input elements.  Results are NOT bit-compatible with awr_conv_gemm: Winograd's
 * rounding differs -- measured 0.3-0.6x the direct kernel's error against float64 (chains of Cin terms instead of 9 Cin).
 * awr_wino_conv3x3 is the first form (windows gathered from global memory; kb = channels per stage, + 100 = 256-thread workgroups), kept for the
 * measurements in profiles/r06_winograd.txt.
 * Plans: the Winograd code 1 | 2 (awr_plan_modes.winograd; awr_set_conv_winograd sets the process-wide default -- $AWR_WINOGRAD or 0 -- that a plan
 * created without a modes block captures, and that awr_wino_eligible / awr_wino_wgrad_eligible answer for; 2 = also the data and weight
 * gradients, + 4 = ignore the launch-size rules: tests, + 8 = never the 64-channel tile form: A/B) makes plan builders run the FORWARD
 * of every eligible layer (awr_wino_eligible: maps >= 8 x 8, at least 256 workgroups; epilogue = bias / ReLU / statistics) through
 * awr_wino2_conv3x3, the DATA GRADIENT of those layers (mirrored transform, accumulate / BatchNorm-backward-reduction epilogues) through
 * awr_wino_dgrad_or_direct, and the WEIGHT GRADIENT of the layers awr_wino_wgrad_eligible names through awr_wino_wgrad (below).  Inference plans take the
 * forward form with the folded eval-mode BatchNorm and a residual add in the epilogue (awr_wino_args.out_scale / out_shift / res); a Hourglass residual then runs
 * conv2 as Winograd followed by the direct conv3 (+ skip) GEMM instead of the fused two-GEMM launch (awr_conv_args.w2).
 * -----------------------------------------------------------------------------------------*/
int awr_wino_weights(const float* w, int N, int C, int Npad, int Cpad, int mirror, float* U, void* stream);
int awr_wino_conv3x3(const float* in, const float* U, const float* bias, float* out, int B, int H, int W, int C, int N, int relu, int kb, void* stream);
int awr_wino2_conv3x3(const float* in, const float* U, const float* bias, const float* in_scale, const float* in_shift, int relu_in, float* out,
                      double* stats, int nslots, int B, int H, int W, int C, int N, int relu, void* stream);
/* the same kernel through an argument block, with the data-gradient epilogue forms of awr_conv_args (res = accumulate in place, bnr_y / bnr_coef /
 * bnr_act = mask with the re-derived ReLU and reduce sum g, sum g * xhat into `stats` for the BatchNorm backward) */
typedef struct awr_wino_args {
    const float *in, *U, *bias, *in_scale, *in_shift;
    float* out;
    double* stats;
    const float *res, *bnr_y, *bnr_coef, *bnr_act;
    int B, H, W, C, N, relu, relu_in, nslots;
    const float *out_scale, *out_shift;      /* optional per-output-channel affine after the bias (a folded eval-mode BatchNorm: inference plans):
                                                out = [relu]((acc + bias) * out_scale + out_shift [+ res]); `res` may then be any (B,H,W,N) tensor */
} awr_wino_args;
int awr_wino_conv(const awr_wino_args* a, void* stream);
/* plans: the data gradient of a stride-1 3x3 convolution described by the DIRECT kernel's argument block `d` -- as Winograd (U = awr_wino_weights(...,
 * mirror = 1)) when this kernel implements everything `d` asks for, through awr_conv_gemm(d) otherwise (decided at launch: plan builders complete
 * `d` after they have created the launch) */
int awr_wino_dgrad_or_direct(const awr_conv_args* d, const float* U, void* stream);
int awr_wino_dgrad_supported(const awr_conv_args* d);
int awr_set_conv_winograd(int on);
int awr_get_conv_winograd(void);
int awr_wino_eligible(int B, int H, int W, int C, int N);
/* Weight gradient of a stride-1 3x3 convolution in the Winograd domain: dg = G^T [sum_patches (B^T d B) (.) (A dY A^T)] G -- 16 GEMMs over the patches,
 * 2.25x fewer multiplies than the nine taps of awr_conv_wgrad.  x (B,H,W,C) is the convolution's input (optionally behind a fused per-channel affine
 * + ReLU: a BatchNorm output that was never written), dy (B,H,W,N) the gradient of its output.  ASSIGNS R[N][9][ld] (the packed layout awr_conv_wgrad
 * accumulates into for D = dY, G = X; ld >= C) and, if not NULL, bias_grad[N] = sum of dy over the pixels.  `scratch`: awr_wino_wgrad_scratch(...)
 * floats (one copy of the transformed-domain tile per K split; summed in a fixed order: deterministic).  C, N multiples of 64, power-of-two maps >= 8 x 8.
 * awr_wino_wgrad_eligible: 1 where a plan should use it (every split keeps a long enough K loop to pay for the copy it stores). */
int awr_wino_wgrad(const float* x, const float* dy, const float* x_scale, const float* x_shift, int x_relu, int B, int H, int W, int C, int N,
                   float* scratch, float* R, int ld, float* bias_grad, void* stream);
int64_t awr_wino_wgrad_scratch(int B, int H, int W, int C, int N);
int awr_wino_wgrad_eligible(int B, int H, int W, int C, int N);

/* ------------------------------------------------------------------------------------------
 * NYU data path on the device (csrc/awr_nyu.hip).  Replaces the IMAGE work of the reference's per-sample loader --
 * Loader.crop (dataloader/loader.py:19-51: center2bounds window, bounds2crop zero padding + cube clamp :190-208, cv2.resize
 * INTER_NEAREST, paste), Loader.augment (:75-86) with recrop = cv2.warpPerspective + fringe clean-up + cube clamp (:123-137) or
 * cv2.warpAffine (:140-160), and Loader.normalize (:88-101) -- for a whole batch per launch.  The host keeps what is tiny and
 * sequential: the RandomState draws, the 3x3 matrices in float64 / float32 exactly as numpy computes them, the label arithmetic
 * (awr_amd.nyu_device builds one awr_nyu_sample per image).  Results are bit-identical to awr_amd.nyu_data (the numpy restatement,
 * itself bit-exact against the reference everywhere except cv2's three resamplers, which no cv2-produced vector pins: README).
 *   frames: the decoded depth frames of the dataset, resident in HBM ([n_frames][fh][fw], uint16 millimetres = G*256 + B of the
 *           PNG, dataloader/nyu_loader.py:71-74; or float32); a sample addresses its frame by index.
 *   All per-pixel coordinate arithmetic is IEEE double / float without contraction (the file is built with -ffp-contract=off).
 * -----------------------------------------------------------------------------------------*/
#define AWR_NYU_NONE 0
#define AWR_NYU_PERSPECTIVE 1       /* translate / scale: recrop through a homography (loader.py:103-137, :163-179) */
#define AWR_NYU_AFFINE 2            /* rotate (loader.py:140-160) */
#define AWR_NYU_U16 0
#define AWR_NYU_F32 1
typedef struct awr_nyu_sample {
    int64_t frame;              /* row of the frame store */
    int32_t ustart, vstart;     /* crop window origin in the frame; may be negative (zero padding, loader.py:196-200) */
    int32_t cw, ch;             /* window extent uend - ustart, vend - vstart */
    int32_t rw, rh;             /* extent after cv2.resize(..., INTER_NEAREST) (loader.py:37-40) */
    int32_t ox, oy;             /* where the resized window is pasted into the dsize x dsize crop (loader.py:43-47) */
    double ifx, ify;            /* resizeNN's inverse scale factors 1. / (rw / cw), 1. / (rh / ch) (two divisions, in this order) */
    double zstart, zend;        /* depth range of the cube: below -> zstart, above -> 0, zero stays zero (loader.py:202-206) */
    int32_t op;                 /* AWR_NYU_NONE / _PERSPECTIVE / _AFFINE */
    int32_t norm32;             /* normalisation arithmetic: 0 = float64 (numpy's promotion for a float64 centre or cube), 1 = float32 */
    double m[9];                /* destination -> source map: _PERSPECTIVE inv(M_new . inv(M)) row-major; _AFFINE the inverted 2x3 in m[0..5] */
    double zstart2, zend2;      /* cube clamp of the recrop (loader.py:131-135) */
    double lo, far, center_z, half;   /* normalize: x in {depth_max, 0} -> far; clip(lo, far); (x - center_z) / half (loader.py:88-101) */
} awr_nyu_sample;

/* Loader.crop (loader.py:19-51) for B samples: crop (B, dsize, dsize) float32; stats (B, 2) float32 = {max of the crop (augment's
 * depth_max, loader.py:76), smallest positive value (recrop's nv_val + 1, loader.py:116; +inf if none)}.  One workgroup per sample. */
int awr_nyu_crop(const void* frames, int frame_type, int fh, int fw, const awr_nyu_sample* samples, int B, int dsize, float* crop,
                 float* stats, void* stream);
/* The resamplers alone, cv2.warpPerspective / cv2.warpAffine with INTER_LINEAR + BORDER_CONSTANT (OpenCV's fixed-point rule: source
 * coordinates in 1/32 pixel, 10-bit affine increments): dst (B, dh, dw) from src (B, sh, sw); m (B, 9) doubles as awr_nyu_sample.m. */
int awr_nyu_warp(const float* src, int sh, int sw, const double* m, int op, float border, int B, int dh, int dw, float* dst, void* stream);
/* Loader.normalize (loader.py:88-101) alone: out[b] = normalize(depth_max[b], img[b], centre, cube) over n pixels per sample */
int awr_nyu_normalize(const float* img, const float* depth_max, const awr_nyu_sample* samples, int B, int64_t n, float* out, void* stream);
/* Loader.augment's image half (loader.py:75-86) from materialised crops: warp per `op`, fringe clean-up against stats, cube clamp,
 * normalize -> out (B, 1, dsize, dsize).  status[b] (optional) = 1 where a recrop found no positive pixel (the reference raises). */
int awr_nyu_augment(const float* crop, const float* stats, const awr_nyu_sample* samples, int B, int dsize, float* out, int* status,
                    void* stream);
/* The production entry: crop + augment + normalize in ONE launch, one workgroup per sample, the crop staged in LDS (never written to
 * HBM) when dsize * dsize floats fit (dsize <= 160); larger crops go through `scratch` (B * (dsize * dsize + 2) floats, else may be
 * NULL) with the two kernels above.  Test-time samples (nyu_loader.py:59-60) are op = AWR_NYU_NONE. */
int awr_nyu_batch(const void* frames, int frame_type, int fh, int fw, const awr_nyu_sample* samples, int B, int dsize, float* out,
                  int* status, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Joint scoring on the device (csrc/awr_eval.hip).  Replaces EvalUtil.feed (util/eval_tool.py:20-46) with its pinhole back-projection
 * uvd2xyz (util/util.py:13-20) -- per sample, on the host, behind a device sync in train.py:141-148 / test.py:67-86 -- for a whole batch
 * per launch, with the running sums the epoch metric needs kept on the device.  One workgroup scores the batch.
 *   jt_pred     (B, J, 3)  predicted joints, normalised uvd in [-1, 1]: the head's output as it is
 *   jt_xyz_gt   (n, J, 3)  ground truth, cube-normalised xyz          center_xyz (n, 3)  crop centre, mm
 *   M           (n, 3, 3)  crop matrix, original-image -> crop pixels  cube       (n, 3)  cube extent, mm
 *   n = n_valid <= B: only rows [0, n_valid) of ANY argument are read (a padded last batch keeps its padding rows out of everything).
 *   img_size: crop side in pixels; fx, fy, u0, v0: the camera intrinsics; flip: +1 / -1, the sign of the camera's y axis.
 * Arithmetic, step by step as numpy does it on the host (awr_amd.evaluator.EvalUtil.feed_batch; no fused multiply-adds):
 *   float32  u, v = (p + 1) * img_size / 2;  d = p_z * cube_z / 2 + center_z                         (eval_tool.py:38-39)
 *   float64  (u, v) <- rows 0, 1 of inv(M) . (u, v, 1), stored as float32.  inv(M) is the adjugate of the float32 M over its determinant
 *            in float64 (the host inverts in float32 with LAPACK: the device form is the closer one to exact)   (:40-41)
 *   float64  x = (u - u0) * d / fx, y = (v - v0) * d / fy, stored as float32; y *= flip; z = d        (util.py:13-20)
 *   float32  gt_mm = gt * (cube / 2) + center;  err = sqrt((dx^2 + dy^2) + dz^2)                      (:46)
 * Outputs (uvd_out and err_out may each be NULL: nothing per frame is written; `capacity` = rows of the result buffers):
 *   uvd_out  rows [row, row + n_valid) of a (capacity, J, 3) buffer: original-image uvd, what test.py:105-108 writes to the results file
 *   err_out  rows [row, row + n_valid) of a (capacity, J) buffer: errors in mm
 *   acc      J + 2 doubles the call ADDS onto (zero them with awr_zero_f64 before the first batch of a run):
 *            acc[0..J) per-joint error sum, acc[J] frames scored, acc[J + 1] sum over frames of the frame's mean error over its joints.
 *            Ordered in-workgroup reduction, one writer per word, no floating-point atomics: bitwise reproducible run to run.
 *   status   2 ints, zero before the first batch of a run: {code, frame}.  Where numpy raises (np.linalg.inv of a singular matrix) the
 *            kernel writes NaN to the frame's rows, leaves it out of `acc`, and records the FIRST such frame of the run: code
 *            AWR_EVAL_SINGULAR (determinant zero, or an inverse that overflows) or AWR_EVAL_NONFINITE (M holds Inf / NaN), frame = row + its
 *            position in the batch.  The other frames of the batch are scored as usual.  The caller reads status when it reads results.
 * J <= AWR_EVAL_MAX_JOINTS.  Nothing synchronises; batches fed on one stream accumulate in feed order.
 * -----------------------------------------------------------------------------------------*/
#define AWR_EVAL_OK 0
#define AWR_EVAL_SINGULAR 1
#define AWR_EVAL_NONFINITE 2
#define AWR_EVAL_MAX_JOINTS 256
int awr_eval_batch(const float* jt_pred, const float* jt_xyz_gt, const float* center_xyz, const float* M, const float* cube, int B, int J,
                   int n_valid, float img_size, double fx, double fy, double u0, double v0, int flip, float* uvd_out, float* err_out,
                   int64_t row, int64_t capacity, double* acc, int* status, void* stream);

/* Joints without labels: the first half of awr_eval_batch (the same device code: eval_tool.py:38-41 and uvd2xyz, util.py:13-20, in the
 * precisions listed above) for callers that have a prediction and no ground truth -- awr_amd.predictor.Predictor.
 *   jt_pred (B, J, 3) normalised uvd; center_xyz (B, 3), M (B, 3, 3), cube (B, 3) float32 as awr_detect_samples writes them.
 *   Only rows [0, n_valid) of any argument are read or written.
 *   uvd_out (B, J, 3)  original-image uvd: bit for bit what awr_eval_batch stores in its uvd_out
 *   xyz_out (B, J, 3)  camera millimetres: evaluator.uvd2xyz(uvd_out, paras, flip) bit for bit
 *   status  (B) int32  per frame AWR_EVAL_OK / _SINGULAR / _NONFINITE; a frame that is not OK gets NaN rows (a NaN matrix is how
 *                      awr_detect_samples marks a frame it could not crop).
 * One workgroup; nothing synchronises. */
int awr_joints_unproject(const float* jt_pred, const float* center_xyz, const float* M, const float* cube, int B, int J, int n_valid,
                         float img_size, double fx, double fy, double u0, double v0, int flip, float* uvd_out, float* xyz_out, int* status,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Hand detection on the device (csrc/awr_detect.hip): the crop centre of a raw depth frame by an iterated centre of
 * mass, and from a centre everything awr_nyu_batch and awr_joints_unproject need -- so a frame without a dataset index, a refined
 * centre file or labels goes to camera-space joints without a host round trip.  The numpy restatement is awr_amd/detect.py
 * (detect, center_of_mass, sample_blocks); results are bit-identical to it.
 *   frames: [n_frames][fh][fw] uint16 millimetres (the FrameStore layout; frame_type must be AWR_NYU_U16 -- float32 is refused);
 *           frame (B) int64 addresses each image's frame.
 * Centre of mass of a pixel set: n, sum of columns u, sum of rows v, sum of raw depths d as 64-bit INTEGERS, centre = (su / n, sv / n,
 * sd / n) as three double divisions.  Integer sums do not depend on order: any split over workgroups and any order of the 64-bit integer
 * atomics give numpy's int64 bits.  No floating-point atomic is involved.  A pixel with d = 0 never counts.
 *   seed    AWR_DET_SEED_GIVEN    seed_uvd (B, 3) doubles
 *           AWR_DET_SEED_RANGE    centre of mass of the pixels of the whole frame with zmin <= d <= zmax
 *           AWR_DET_SEED_NEAREST  dmin = the smallest such d; centre of mass of the pixels with dmin <= d <= min(dmin + slab, zmax)
 *   refine  `iters` times (0 ... AWR_DET_MAX_ITERS, no convergence test): window and depth range of the current centre by
 *           nyu_data.center2bounds(centre, cube, (fx, fy)) (loader.py:181-188: IEEE double in that expression order, int() truncating),
 *           clipped to the frame; centre of mass of the window's pixels with zstart <= d <= zend.
 *   cube    doubles on the device: 3 (cube_stride 0) or B x 3 (cube_stride 3).
 *   parts   workgroups per frame and pass: 0 = chosen from B and fh (about four per CU over the batch); a workgroup's share is whole
 *           rows of the window, read with 16-byte loads between its unaligned ends.
 *   scratch awr_detect_scratch(B) bytes, 8-byte aligned: one accumulator slot per frame and pass (the call initialises it).
 * Outputs: center_uvd (B, 3) doubles; status (B) int32:
 *   AWR_DET_OK
 *   AWR_DET_EMPTY      some pass found no pixel: the centre is NaN, and stays NaN through the later passes, awr_detect_samples and
 *                      awr_joints_unproject (NaN rows; never a fault, never a read outside the store)
 *   AWR_DET_BAD_FRAME  frame[b] is outside [0, n_frames): nothing is read, the centre is NaN
 * Each pass is one launch on `stream`; nothing synchronises.
 * -----------------------------------------------------------------------------------------*/
#define AWR_DET_OK 0
#define AWR_DET_EMPTY 1
#define AWR_DET_BAD_FRAME 2
#define AWR_DET_BAD_WINDOW 3
#define AWR_DET_SEED_GIVEN 0
#define AWR_DET_SEED_RANGE 1
#define AWR_DET_SEED_NEAREST 2
#define AWR_DET_MAX_ITERS 8
#define AWR_DET_MAX_BATCH 65535
int64_t awr_detect_scratch(int B);        /* bytes; -1 for a B outside [1, AWR_DET_MAX_BATCH] */
int awr_detect(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B, int seed_mode,
               const double* seed_uvd, double zmin, double zmax, double slab, const double* cube, int cube_stride, double fx, double fy,
               int iters, int parts, void* scratch, double* center_uvd, int* status, void* stream);
/* Centres -> what the rest of the pipeline consumes, per frame:
 *   samples     the awr_nyu_sample block nyu_device.set_crop + set_normalize write for a float64 centre (op = AWR_NYU_NONE, norm32 = 0),
 *               field for field: window by center2bounds, rw / rh = int(w * scale), ox / oy = int((dsize - size) / 2.0), ifx / ify as
 *               two divisions, the cube's depth range, normalize's lo / far / center_z / half
 *   M           (3, 3) float32: nyu_data.center2transmat in double, stored as float32
 *   center_xyz  (3) float32: evaluator.uvd2xyz of the float64 centre       cube_out (3) float32
 * status (B) is read and updated (zero it, or hand over awr_detect's): a window set_crop refuses (it misses the frame or resizes to
 * nothing) or a NaN centre sets AWR_DET_BAD_WINDOW on a frame that was AWR_DET_OK; a frame index outside [0, n_frames) sets
 * AWR_DET_BAD_FRAME.  Such a frame gets a block that reads no pixel (frame 0, rw = rh = 0: awr_nyu_batch renders a constant background
 * image) and a NaN matrix, which awr_joints_unproject turns into NaN rows. */
int awr_detect_samples(const double* center_uvd, const double* cube, int cube_stride, int64_t n_frames, const int64_t* frame, int B, int dsize,
                       int fh, int fw, double fx, double fy, double u0, double v0, int flip, awr_nyu_sample* samples, float* M,
                       float* center_xyz, float* cube_out, int* status, void* stream);

/* Forearm-robust palm centre (csrc/awr_palm.hip; the numpy statement is awr_amd/detect.py palm_center, results are
 * bit-identical to it).  A centre of mass inside a cube is dragged up a forearm that lies at the hand's depth; the palm is the widest
 * part of the hand-plus-arm silhouette, and the hand is at the end of its medial set beyond which more silhouette lies (the fingers).
 * Per frame b, from a detector centre center_in[b] with status_in[b]:
 *   1. frame[b] outside [0, n_frames): AWR_DET_BAD_FRAME, NaN centre, nothing is read.  Otherwise status_in[b] != AWR_DET_OK: centre and
 *      status pass through unchanged.  Either way info = (-1, -1, 0, 0).
 *   2. Window W = nyu_data.center2bounds(centre, (search * cube[0], search * cube[1], search * cube[2]), (fx, fy)) clipped to the frame,
 *      as awr_detect clips it.  mask(v, u): the pixel is inside W, d != 0, zstart <= d <= zend of that call and zmin <= d <= zmax.  A
 *      NaN or infinite centre or bound, an empty window or an empty mask: NaN centre, AWR_DET_EMPTY, info = (-1, -1, 0, 0).
 *   3. D2, the exact squared Euclidean distance transform of the mask: everything outside W -- the one-pixel ring around it, and beyond
 *      the frame too -- is background; D2(p) = min over background q of |p - q|^2, 0 on background.  As two passes: g(v, u) = the
 *      distance along the column to the nearest background row (the ring rows v0 - 1 and v1 count), then
 *      D2(v, u) = min over u' in [u0 - 1, u1] of (u - u')^2 + g(v, u')^2 with g = 0 on the ring columns.
 *   4. m = max D2 (>= 1).  The medial set S = {p : tau_den * D2(p) >= tau_num * m}.
 *   5. Every argmax takes the FIRST maximum in raster order (smallest v, then smallest u):
 *      e0 = argmax_S D2;  e1 = argmax_S |p - e0|^2;  e2 = argmax_S |p - e1|^2;  a = e2 - e1;  L = |a|^2.
 *   6. L == 0: p* = e0.  Otherwise t(p) = (p - e1) . a;  b1 = the mask pixels with t < 0;  b2 = the mask pixels with t > L;
 *      s(p) = L - t(p) if b2 >= b1, else t(p);  N = {p in S : s <= 0 or s * s <= m * L} (within one palm radius of the chosen end along
 *      the axis);  p* = argmax_N D2.
 *   7. r2 = D2(p*).  The palm disc: the mask pixels with rho2_den * |p - p*|^2 <= rho2_num * r2.  n, sum of u, sum of v, sum of raw
 *      depths over the disc as 64-bit integers; centre = (su / n, sv / n, sd / n) as three double divisions; AWR_DET_OK;
 *      info = (p*.u, p*.v, r2, n) in frame pixels.
 * Everything between the window (awr_detect's double arithmetic, the cube scaled by `search`) and the last three divisions is integer:
 * with fh, fw <= 16384, D2 <= 2^28, L <= 2^29, |t|, |s| <= 2^30, so s * s <= 2^60, m * L <= 2^57 and, the four ratio terms being
 * positive ints, tau * D2 and rho2 * |p - p*|^2 <= 2^60: every product stays below 2^62.  Larger frames are refused.  Integer sums and
 * maxima packed with their raster index do not depend on launch geometry or arrival order: a frame is split by rows over several
 * workgroups whose partial maxima and sums meet in 64-bit INTEGER atomics; there is no floating-point atomic and no floating-point
 * reduction.
 *   search > 0 and finite; 0 < tau_num <= tau_den; 0 < rho2_den <= rho2_num.  The defaults of the statement are 2.0, 1 / 3, 25 / 4.
 *   cube: doubles on the device, 3 (cube_stride 0) or B x 3 (cube_stride 3).  Only uint16 frames (AWR_NYU_U16).
 *   scratch: awr_detect_palm_scratch(B, fh, fw) bytes, 8-byte aligned (sixteen 64-bit accumulator words per frame, which the call
 *   initialises, then one int32 word per pixel and frame: D2); nothing is written past it.
 *   center_out (B, 3) doubles may be center_in; status_out (B) int32 may be status_in; info (B, 4) int32 may be NULL.
 * Nine launches on `stream`, one per stage (the slots, the column scans, the row pass, e1, e2, the counts, p*, the disc, the outputs),
 * ordered by the stream alone; only the last writes an output.  Nothing synchronises; nothing outside the frame store is read. */
int64_t awr_detect_palm_scratch(int B, int fh, int fw);        /* bytes; -1 for a B outside [1, AWR_DET_MAX_BATCH] or a side outside [1, 16384] */
int awr_detect_palm(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B,
                    const double* center_in, const int* status_in, double zmin, double zmax, const double* cube, int cube_stride, double fx,
                    double fy, double search, int tau_num, int tau_den, int rho2_num, int rho2_den, void* scratch, double* center_out,
                    int* status_out, int* info, void* stream);

/* Several hands per frame (csrc/awr_hands.hip; the numpy statements are awr_amd/detect.py components and hand_seeds,
 * results are bit-identical to them).  awr_detect's "nearest" seed is the centre of mass of EVERY pixel of the frame within `slab` of the
 * nearest one: with two hands in view it lies between them, and at most one hand is ever reported.  This entry splits the near
 * foreground into connected components and seeds the K nearest large ones; each seed is then refined by the unchanged awr_detect with
 * AWR_DET_SEED_GIVEN.  Per frame b:
 *   1. frame[b] outside [0, n_frames): AWR_DET_BAD_FRAME and a NaN centre in every slot, info = (-1, -1, 0, 0), count = 0, labels -1;
 *      nothing is read.
 *   2. Foreground: zmin <= d <= zmax and d != 0 (awr_detect's rule).  dmin = the smallest foreground depth.  The mask is the foreground
 *      with d <= min(dmin + reach, zmax), compared in double.
 *   3. Two mask pixels are connected when they are 4-neighbours; there is no depth test.  A pixel's label is the smallest raster index
 *      v * fw + u of its component, -1 on background: canonical integers, whatever the algorithm and the order.
 *   4. Candidates: the components with n >= min_pixels pixels; count[b] = their number (it may exceed K).  A candidate's key is
 *      (zc, root): zc its smallest raw depth, root its label.  The K smallest keys fill slots 0 ... K - 1 in ascending order: slot 0 is
 *      the nearest hand, and a tie in depth goes to the smaller root.
 *   5. A slot's seed: n, sum of u, sum of v, sum of raw depths over the component's pixels with d <= min(zc + slab, zmax) as 64-bit
 *      integers, centre = (su / n, sv / n, sd / n) as three double divisions -- the "nearest" rule per component; AWR_DET_OK;
 *      info = (root % fw, root / fw, n of the component, zc).  A slot past the candidates: NaN centre, AWR_DET_EMPTY, (-1, -1, 0, 0).
 * Outputs are HAND-MAJOR: slot k of frame b is row k * B + b of centers (K, B, 3) doubles, status (K, B) and info (K, B, 4) int32 -- the
 * layout of the test-time views, so awr_detect, awr_detect_palm, awr_detect_samples and what follows take K * B rows as they are.
 * count (B) int32.  labels_out (B, fh, fw) int32 may be NULL.
 *   K in [1, AWR_DET_MAX_HANDS], B in [1, AWR_DET_MAX_BATCH], fh, fw in [1, 16384], min_pixels >= 1, zmin <= zmax, reach >= 0 and
 *   slab >= 0 (infinity allowed, NaN not): anything else returns AWR_ERR_ARG with a message, before any launch.  Only uint16 frames.
 *   scratch: awr_detect_hands_scratch(B, fh, fw) bytes, 8-byte aligned: per batch row 278 64-bit words, which the call initialises, then
 *   three int32 words per pixel and batch row (the forest, and pixels and smallest depth per root); nothing is written past it.  The same
 *   frame twice in a batch uses two independent regions.
 * The labelling is a union-find forest joined by smaller index with integer atomicMin -- every pointer only ever decreases, so the root
 * that survives is the component's smallest index in any order; sums, counts and minima are integer atomics.  There is no floating-point
 * atomic and no floating-point reduction.  Nine launches on `stream`, one per stage (the slots, dmin, the tiles, the tile borders, the
 * flattening, the roots, the pick, the slab sums, the outputs); only the stream orders them, no workgroup waits for another, nothing
 * synchronises, nothing outside the frame store is read. */
#define AWR_DET_MAX_HANDS 4
int64_t awr_detect_hands_scratch(int B, int fh, int fw);       /* bytes; -1 for a B outside [1, AWR_DET_MAX_BATCH] or a side outside [1, 16384] */
int awr_detect_hands(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B, int K,
                     double zmin, double zmax, double reach, double slab, int min_pixels, void* scratch,
                     int* labels_out /* B*fh*fw, may be NULL */, double* centers /* K,B,3 */, int* status /* K,B */,
                     int* info /* K,B,4 */, int* count /* B */, void* stream);

/* awr_detect_hands with a depth test on the join (the statements are components / hand_seeds with edge=...): everything
 * above holds, except step 3, which becomes
 *   3'. Two mask pixels are JOINED when they are 4-neighbours and |d_a - d_b| <= edge, their raw depths compared in double; the
 *       components are the transitive closure of that relation (a ramp whose neighbouring pixels differ by at most `edge` is ONE
 *       component, however far apart its ends are).  Labels stay canonical: the smallest raster index of the component, -1 off the mask.
 * so a hand held in front of another one, `edge` millimetres or more nearer along the whole contact line, is a component of its own.
 * What it does not separate: hands that touch in depth, and an occluded hand that the front one cuts into fragments -- each fragment
 * of min_pixels or more pixels is a candidate.  edge >= 0 (infinity allowed: awr_detect_hands' labels, as every edge >= 65535; NaN
 * not): anything else returns AWR_ERR_ARG with a message that names it, before any launch.  For integer depths the test equals
 * |d_a - d_b| <= floor(min(edge, 65535)), which is what the kernels compare.  The same nine launches, scratch and outputs: only the
 * tile and the border stage differ (compile-time forms of the same two kernels; awr_detect_hands runs the forms without the test). */
int awr_detect_hands_edge(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B, int K,
                          double zmin, double zmax, double reach, double edge, double slab, int min_pixels, void* scratch,
                          int* labels_out /* B*fh*fw, may be NULL */, double* centers /* K,B,3 */, int* status /* K,B */,
                          int* info /* K,B,4 */, int* count /* B */, void* stream);

/* awr_detect_hands_edge with links across an occluder (the statements are components / hand_seeds with edge=, link=,
 * gap=): the fragments a front hand cuts a rear hand into are joined again.  Everything above holds; the components are the transitive
 * closure of the joins of 3' and of these links.  For every mask pixel p (raw depth d_p) and each of the four directions (right, left,
 * down, up), with q_t the pixel t steps from p in that direction:
 *   a. a pixel o is an OCCLUDER of p when d_o != 0 and d_p - d_o > edge -- raw depths only: it need not lie in the mask and may be nearer
 *      than zmin;
 *   b. n = the number of consecutive occluders q_1 ... q_n, counted up to gap.  Nothing happens when n == 0, when q_1 ... q_gap and
 *      q_{gap+1} are all occluders, or when the walk leaves the frame before it ends;
 *   c. otherwise q = q_{n+1} is the first pixel that is no occluder; when q is a mask pixel and |d_q - d_p| <= link, p and q are joined.
 * The test is p's alone: one direction of a pair may hold and the other not, and either one joins.  A zero pixel inside the gap is no
 * occluder and ends the walk (sensor shadows break links).  An edge >= 65535 makes no pixel an occluder: awr_detect_hands' labels.  Two
 * DIFFERENT hands at similar depth with a nearer object of gap pixels or fewer between them are linked.  Labels stay canonical.
 * link >= 0 (infinity allowed, NaN not), gap in [1, AWR_HANDS_MAX_GAP], edge >= 0: anything else returns AWR_ERR_ARG with a message that
 * names the entry point and the argument, before any launch.  For integer depths the tests equal d_p - d_o > floor(min(edge, 65535)) and
 * |d_q - d_p| <= floor(min(link, 65535)), which is what the kernel compares.  Ten launches: awr_detect_hands_edge's nine and, between
 * the tile borders and the flattening, the link stage -- a thread per pixel, at most gap + 1 loads of the frame per direction for a
 * pixel at the rear side of an occlusion edge, joins by the forest's atomicMin.  The same scratch and outputs. */
#define AWR_HANDS_MAX_GAP 64
int awr_detect_hands_link(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B, int K,
                          double zmin, double zmax, double reach, double edge, double link, int gap, double slab, int min_pixels,
                          void* scratch, int* labels_out /* B*fh*fw, may be NULL */, double* centers /* K,B,3 */, int* status /* K,B */,
                          int* info /* K,B,4 */, int* count /* B */, void* stream);

/* A frame per hand (csrc/awr_isolate.hip; the numpy statement is awr_amd/detect.py isolate, results are bit-identical
 * to it).  awr_detect_hands keeps a seed per hand, and awr_detect, awr_detect_palm, awr_detect_samples and the renderer read the whole raw
 * frame again: two hands closer than half a crop cube stand in each other's window and crop.  This entry gives each hand a frame that
 * holds only its own component.  Rule, per frame b and slot k, with labels (B, fh, fw) as awr_detect_hands' labels_out and
 * root_k = info[1] * fw + info[0] of the slot's info row (info (K, B, 4), hand-major, as awr_detect_hands writes it):
 *   output k equals the frame with every pixel set to 0 where labels >= 0 and labels != root_k;
 *   when root_k < 0 (an EMPTY slot: info = (-1, -1, 0, 0)), output k is the unchanged frame;
 *   unlabelled pixels stay: background, depth 0, and foreground beyond dmin + reach;
 *   debris components below min_pixels are labelled, so they are removed from EVERY hand's frame.
 * out: an output store in the FrameStore layout, (K * B, fh, fw) uint16, row k * B + b -- hand-major, so awr_detect and what follows take
 * the rows as frame indices.  It may be rows of the allocation that holds `frames`, past the n_frames rows that are read.  status (B):
 * AWR_DET_OK, or AWR_DET_BAD_FRAME where frame[b] is outside [0, n_frames): that frame's K outputs are zero frames and nothing is read.
 *   K in [1, AWR_DET_MAX_HANDS], B in [1, AWR_DET_MAX_BATCH], fh, fw in [1, 16384]: anything else returns AWR_ERR_ARG with a message,
 *   before any launch.  Only uint16 frames.
 * ONE launch on `stream`: a thread per 8 pixels reads one 16-byte word of the frame and its 8 labels and writes K 16-byte words, so the
 * frame and its labels are read once however large K is ((6 + 2 K) bytes per pixel); where fh * fw is no multiple of 8 or a base is not
 * 16-byte aligned a thread per pixel does the same.  No atomics, no LDS, nothing synchronises. */
int awr_hands_isolate(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B, int K,
                      const int* labels /* B,fh,fw */, const int* info /* K,B,4 */, void* out /* K*B,fh,fw uint16 */, int* status /* B */,
                      void* stream);

/* Edge-preserving depth pre-filter (csrc/awr_denoise.hip; the numpy statement is awr_amd/detect.py denoise, results are
 * bit-identical to it).  Output row b of `out` (B rows in the FrameStore layout) is the filtered frame frame[b].  The rule:
 *
 * Every output pixel is a function of the INPUT frame alone. It is a single pass: not iterated, not in place.
 * Definitions for pixel p with depth d_p:
 *   - W is the set of in-frame pixels of the (2 * radius + 1)^2 window around p, without p itself.
 *   - elim = 65535 for edge=None, else floor(min(edge, 65535)). This is awr_frame.h's depth_floor, the integer form 4.29 already uses.
 *   - A pixel is valid when its depth is not 0.
 *   - The lower median of n values is element (n - 1) // 2 of the ascending sort. It is a value that occurs in the window, never an
 *     average.
 * Output:
 *   - If d_p != 0: let S = { q in W : d_q != 0 and |d_q - d_p| <= elim }.
 *       - If |S| < support the output is 0. This removes a flying pixel or speckle.
 *       - Otherwise the output is the lower median of S and p together, which is element |S| // 2 of its sort.
 *   - If d_p == 0: let V = { q in W : d_q != 0 }.
 *       - If fill is given and |V| >= fill, the output is the lower median of V.
 *       - Otherwise the output is 0.
 * Out-of-frame positions and zero pixels are indistinguishable under this rule, because both thresholds are absolute counts. The frame
 * behaves as if surrounded by zeros, and the kernel may stage its halo that way.
 *
 * Here edge = +infinity is edge=None (no depth test) and fill = 0 is fill=None (no filling).  status (B): AWR_DET_OK, or
 * AWR_DET_BAD_FRAME where frame[b] is outside [0, n_frames): that row is a zero frame and nothing is read.
 *   radius 1 or 2; edge >= 0 (NaN and negative values are refused); support in [0, (2 radius + 1)^2 - 1]; fill in [0, the same];
 *   B in [1, AWR_DET_MAX_BATCH], fh, fw in [1, 16384]; only uint16 frames; `out` must not overlap the n_frames rows of the frame store
 *   (the pass is not in place): anything else returns AWR_ERR_ARG with a message that names the entry point and the value, before any
 *   launch.
 * ONE launch on `stream`: a workgroup of 256 threads per 64 x 16 tile and batch row stages the tile and its halo in LDS as uint16, a
 * thread filters four pixels of a row and writes them as one 8-byte store (fw a multiple of 4 and both bases 8-byte aligned; otherwise
 * 2-byte loads and stores do the same).  The median is selected bit by bit from counts of the window's keys, integers only.  No atomics,
 * no floating-point arithmetic on a depth, nothing synchronises. */
int awr_frames_denoise(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame, int B, int radius,
                       double edge, int support, int fill, void* out /* B,fh,fw uint16 */, int* status /* B */, void* stream);

/* Joints -> the next crop centre, per frame, with a gate (the numpy statement is awr_amd/detect.py joints_center,
 * results are bit-identical to it):
 *   xyz (B, J, 3) camera mm, as awr_joints_unproject writes xyz_out; center_uvd (B, 3) doubles, the centres this pass was cropped at;
 *   center_xyz (B, 3), cube (B, 3) float32 as awr_detect_samples writes them; status, ustatus (B): awr_detect(_samples)'s and
 *   awr_joints_unproject's codes; joints: n_joints device indices into [0, J) (NULL / 0 = all joints); zmin, zmax, max_shift: the gate.
 * Per frame b < n_valid, all arithmetic in IEEE double without contraction, in this order:
 *   1. status[b] != 0 || ustatus[b] != 0                                  -> AWR_RECENTER_KEPT_FRAME
 *   2. m = sum over the selected joints of (double)xyz[b][j][:], accumulated sequentially in index order, divided by their number
 *      (one division per axis)
 *   3. a component of m is not finite                                     -> AWR_RECENTER_KEPT_NONFINITE
 *   4. zmin <= m.z <= zmax does not hold                                  -> AWR_RECENTER_KEPT_DEPTH
 *   5. |m - (double)center_xyz[b]| <= max_shift * ((double)cube[b] / 2.0) fails on an axis (per axis on purpose: no sum of squares)
 *                                                                         -> AWR_RECENTER_KEPT_SHIFT
 *   6. otherwise AWR_RECENTER_MOVED; the new centre is evaluator.xyz2uvd of m in its expression order (util.py:3-10):
 *      y = m.y * flip;  u = m.x * fx / m.z + u0;  v = y * fy / m.z + v0;  d = m.z
 * A joint index outside [0, J) can only be seen on the device: such a frame gets AWR_RECENTER_KEPT_NONFINITE, never an out-of-range read.
 *   center_out (B, 3)  the new centre where the frame is re-centred, center_uvd's row otherwise; may alias center_uvd
 *   next_out   (B, 3)  the new centre where re-centred, NaN otherwise (may be NULL)
 *   code       (B)     AWR_RECENTER_*
 * Rows >= n_valid are neither read nor written.  J <= AWR_RECENTER_MAX_JOINTS, B <= AWR_DET_MAX_BATCH; max_shift >= 0 (infinity: no
 * shift gate).  One thread per frame, one small launch; nothing synchronises. */
#define AWR_RECENTER_KEPT_FRAME 0
#define AWR_RECENTER_MOVED 1
#define AWR_RECENTER_KEPT_NONFINITE 2
#define AWR_RECENTER_KEPT_DEPTH 3
#define AWR_RECENTER_KEPT_SHIFT 4
#define AWR_RECENTER_MAX_JOINTS 256
int awr_joints_center(const float* xyz, const double* center_uvd, const float* center_xyz, const float* cube, const int* status,
                      const int* ustatus, int B, int J, int n_valid, const int* joints, int n_joints, double fx, double fy, double u0, double v0,
                      int flip, double zmin, double zmax, double max_shift, double* center_out, double* next_out, int* code, void* stream);
/* Per frame, a first-choice centre or a fallback: out = a where a_status == AWR_DET_OK and all three components of a_center are finite,
 * otherwise b with b's centre and b's status (whatever they are).  which (B, may be NULL): 0 = a, 1 = b.  The outputs alias no input.
 * One small launch; nothing synchronises. */
int awr_centers_select(const double* a_center, const int* a_status, const double* b_center, const int* b_status, int B, double* out_center,
                       int* out_status, int* which, void* stream);

/* Test-time views (the numpy statements are awr_amd/detect.py view_table, view_centers, view_rotate and fuse_views, results
 * are bit-identical to them): the same hand under V <= AWR_VIEWS_MAX in-plane rotations, cube scales and centre shifts -- the three
 * augmentations of loader.py:75-86 -- carried in the batch dimension of one plan, VIEW-MAJOR: view v of frame b is row v * B + b of every
 * (V * B, ...) array below, so view 0 occupies the rows a batch without views would.
 *   table (V, AWR_VIEW_TABLE_DOUBLES) doubles, built on the host by detect.view_table and uploaded once; per view
 *     [0, 9)   R       the forward rotation in crop pixels, cv2.getRotationMatrix2D((dsize / 2, dsize / 2), -mod(rot, 360), 1) as
 *                      loader.py:140-160 calls it, extended by the row 0 0 1
 *     [9, 15)  iR      its inverse as cv2.warpAffine takes it (nyu_data._invert_affine): the destination -> source map of AWR_NYU_AFFINE
 *     [15]     scale   factor on the three cube edges          [16, 19) shift, camera millimetres added to the centre
 *     [19]     rotates 1.0 where the view rotates (the reference's own test, not allclose(rot, 0)), else 0.0
 *   The device evaluates no cosine or sine: device libm and the host's need not agree in the last bit, the table's bits are the host's.
 * All arithmetic below is IEEE double without contraction, in the order written.
 *
 * awr_view_centers: one thread per (view, frame b < n_valid); rows with b >= n_valid are not written.
 *   centers_out (V * B, 3) doubles: center_uvd[b]'s bits where the view's shift is (0, 0, 0); otherwise evaluator.xyz2uvd(uvd2xyz(c) + shift)
 *     in their expression order (util.py:3-20, loader.py:112): x = (u - u0) * d / fx + sx;  y = (v - v0) * d / fy * flip + sy;  z = d + sz;
 *     u' = x * fx / z + u0;  v' = (y * flip) * fy / z + v0;  d' = z
 *   cubes_out (V * B, 3) doubles = cube[b] * scale (cube: 3 doubles with cube_stride 0, B x 3 with cube_stride 3)
 *   frame_out (V * B) int64 = b           status_out (V * B) int32 = status[b]
 *   These are awr_detect_samples' center_uvd, cube (cube_stride 3), frame and status over V * B rows.
 *
 * awr_view_rotate, after awr_detect_samples: one thread per (view, frame b < n_valid), in place.  A row of a rotating view whose status is
 *   AWR_DET_OK gets op = AWR_NYU_AFFINE, m[0..5] = iR, m[6..8] = 0, 0, 1 in its block, and its crop matrix becomes M_v = float32(R . float64(M)),
 *   row times column, each element ((a * b) + (c * d)) + (e * f): original-image pixels -> pixels of the rotated crop, which is all that
 *   awr_joints_unproject needs to undo the rotation.  Every other row is left as it is (an AWR_DET_BAD_WINDOW row keeps its pixel-free block
 *   and NaN matrix).
 *
 * awr_views_fuse: one thread per (frame b < n_valid, joint j); the <= 8 values per axis stay in registers.
 *   xyz (V * B, J, 3) camera mm as awr_joints_unproject writes xyz_out; status, ustatus (V * B) the rows' codes; weights (V * B, J) float32,
 *   read only by AWR_FUSE_CONF (may be NULL otherwise): the head's conf (awr_confidence_fields' first output before its NaN masking).
 *   1. status or ustatus of view 0's row is non-zero -> the joint is NaN, views_used = 0, the spread is NaN
 *   2. view v is used iff both its codes are zero, its three coordinates are finite and, for AWR_FUSE_CONF, its weight is finite and > 0
 *      (the weight max(conf, 0), with zero weights dropped); w_v = 1 for AWR_FUSE_MEAN and AWR_FUSE_MEDIAN, the weight for AWR_FUSE_CONF
 *   3. no view used -> the joint is NaN, views_used = 0, the spread is NaN
 *   4. AWR_FUSE_MEAN / _CONF: m = (sum w_v x_v) / (sum w_v), both sums sequentially in view order from 0.0, one division per axis
 *   5. AWR_FUSE_MEDIAN: per axis the middle of the used views' values in ascending order (a stable sort), or (lower + upper) / 2.0 of the
 *      middle two
 *   6. spread_out = float32(sqrt((sum w_v ((dx^2 + dy^2) + dz^2)) / (sum w_v))) with d = x_v - m, sequentially in view order
 *   7. uvd_out = float32 of evaluator.xyz2uvd(m) as awr_joints_center's step 6 spells it      8. xyz_out = float32(m)
 *   xyz_out, uvd_out (B, J, 3) float32; spread_out (B, J) float32; used_out (B, J) int32.  Rows >= n_valid are neither read nor written.
 * V <= AWR_VIEWS_MAX, V * B <= AWR_DET_MAX_BATCH, J <= AWR_RECENTER_MAX_JOINTS: anything else returns AWR_ERR_ARG with a message, before
 * any launch.  Each entry is one small launch on `stream`, without atomics; nothing synchronises. */
#define AWR_VIEWS_MAX 8
#define AWR_VIEW_TABLE_DOUBLES 20
#define AWR_FUSE_MEAN 0
#define AWR_FUSE_CONF 1
#define AWR_FUSE_MEDIAN 2
int awr_view_centers(const double* center_uvd, const int* status, const double* cube, int cube_stride, const double* table, int V, int B,
                     int n_valid, double fx, double fy, double u0, double v0, int flip, double* centers_out, double* cubes_out,
                     int64_t* frame_out, int* status_out, void* stream);
int awr_view_rotate(awr_nyu_sample* samples, float* M, const int* status, const double* table, int V, int B, int n_valid, void* stream);
int awr_views_fuse(const float* xyz, const int* status, const int* ustatus, const float* weights, int mode, int V, int B, int J, int n_valid,
                   double fx, double fy, double u0, double v0, int flip, float* xyz_out, float* uvd_out, float* spread_out, int* used_out,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Synthetic hand frames (csrc/awr_synth.hip; statement: awr_amd/synth.py render)
 *
 * awr_synth_render casts one depth ray per pixel against a union of capsules and writes raw uint16 millimetre frames -- the input of
 * awr_detect and awr_nyu_batch -- into rows [row, row + n) of `out`, a (capacity, fh, fw) uint16 frame store.
 *   prims (n, K, 8) doubles, rows `ax ay az bx by bz r 0` in camera millimetres: the segment a -> b swept by a sphere of radius r; r <= 0
 *     marks an unused row; a == b is a sphere.  All trigonometry is the host's: the device evaluates + - * / and square roots only.
 *   bbox (n, 4) int32 `u_lo v_lo u_hi v_hi`: pixels outside [u_lo, u_hi) x [v_lo, v_hi) are background; the box is clipped to the frame.
 *   Pixel (u, v) of frame i: the ray t * ((u - u0) / fx, flip * ((v - v0) / fy), 1); the depth is the smallest t at which it ENTERS a used
 *     capsule (the operation order, capsule by capsule, is written out at the top of awr_amd/synth.py and repeated in the kernel: every
 *     dot product (x x' + y y') + z z', no fused multiply-add; whether a capsule counts is decided by signs of polynomials in the inputs,
 *     square roots only place the hit).  Value: floor(t + 0.5) clipped to [1, 65535]; with background_mm > 0 (a wall) a value >=
 *     background_mm is the wall's.  Background: 0 or the wall.  noise_mm = a > 0 adds hash(seed, frame0 + i, v * fw + u) % (2 a + 1) - a
 *     (a uint32 hash, the same in awr_amd.synth.hash_u32) to hit pixels and to the wall and clips to [1, 65535] again: the GLOBAL frame
 *     index enters the hash, so a store rendered in chunks equals one rendered by a single call.
 *   status (n) int32: AWR_SYNTH_OK, AWR_SYNTH_EMPTY (no pixel was hit: the frame is all background) or AWR_SYNTH_BAD_PRIM (a used row holds
 *     Inf / NaN: the frame is all background; the other frames of the call are not affected).  Nothing in the table can fault.
 * Two launches on `stream` (one thread per frame writes the status, then one workgroup per 64 x 16 pixel tile; a workgroup that hit
 * something clears the EMPTY bit with one integer atomic); no float atomics, nothing synchronises.  NULL pointers, n outside
 * [1, AWR_SYNTH_MAX_FRAMES], K outside [1, AWR_SYNTH_MAX_PRIMS], fh or fw outside [1, AWR_SYNTH_MAX_EDGE], flip not +-1, a zero focal
 * length, background_mm outside [0, 65535], noise_mm outside [0, 32767], a negative frame0 and rows that do not fit `capacity` return
 * AWR_ERR_ARG with a message, before any launch. */
#define AWR_SYNTH_OK 0
#define AWR_SYNTH_EMPTY 1
#define AWR_SYNTH_BAD_PRIM 2
#define AWR_SYNTH_MAX_PRIMS 32
#define AWR_SYNTH_MAX_FRAMES 65535
#define AWR_SYNTH_MAX_EDGE 16384
int awr_synth_render(const double* prims, const int* bbox, int n, int K, int fh, int fw, double fx, double fy, double u0, double v0, int flip,
                     int background_mm, int noise_mm, unsigned int seed, int64_t frame0, uint16_t* out, int64_t row, int64_t capacity,
                     int* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * Temporal joint filter (csrc/awr_track.hip; statement: awr_amd/track.py filter_step, results are bit-identical to it)
 *
 * awr_joints_filter runs one step of a One-Euro low-pass per (batch slot, joint, axis) over camera-space joints, with a measurement gate,
 * an optional confidence weight, coasting over frames without a usable measurement and a constant-velocity look-ahead.
 *   state (B, J, 6) doubles `x0 x1 x2 d0 d1 d2`: the filtered position in camera mm and the filtered velocity in mm/s; count (B, J, 2)
 *     int32 `age coast`; age == 0: no track.  Both zeroed make an empty filter; both are updated in place and stay on the device.
 *   xyz (B, J, 3) float32 camera mm as awr_joints_unproject / awr_views_fuse write it; status, ustatus (B) the frame's codes;
 *   conf (B, J) float32, read only with weight = 1 (may be NULL otherwise).
 * Constants of a call, computed by the entry point on the host in double, in this order:
 *   w = (2.0 * M_PI) * dt;  alpha_d = 1.0 / (1.0 + 1.0 / (w * d_cutoff));  gate2 = gate_mm * gate_mm, +infinity for gate_mm < 0 (no gate)
 * Per b < n_valid and j, z[a] = (double)xyz[b][j][a], everything in IEEE double without contraction, in the order written:
 *   ok = status[b] == 0 && ustatus[b] == 0 && z[0], z[1], z[2] are finite
 *   age == 0:  ok -> x = z, d = 0, age = 1, coast = 0: AWR_FILTER_INIT;  otherwise AWR_FILTER_NONE: NaN outputs, state untouched
 *   age != 0 and ok:  y[a] = z[a] - x[a];  g2 = (y0 * y0 + y1 * y1) + y2 * y2;  the measurement is accepted iff g2 <= gate2
 *   accepted:  wgt = 1.0; with weight = 1 and c = (double)conf[b][j]:  wgt = conf_floor; if (c > conf_floor) wgt = c; if (c > 1.0) wgt = 1.0
 *     (a NaN gives the floor); then per axis
 *       dx = y[a] / dt;  d[a] = d[a] + alpha_d * (dx - d[a]);  cut = min_cutoff + beta * fabs(d[a]);  al = 1.0 / (1.0 + 1.0 / (w * cut));
 *       x[a] = x[a] + (al * wgt) * y[a]
 *     age += 1 (saturating at INT_MAX), coast = 0: AWR_FILTER_UPDATED
 *   not accepted (gated, or not ok):  coast += 1;
 *     coast > max_coast and ok      -> the state is set as by INIT: AWR_FILTER_REINIT
 *     coast > max_coast and not ok  -> age = coast = 0, the six state words are zeroed, NaN outputs: AWR_FILTER_LOST
 *     otherwise x and d stay and the outputs are the held ones: AWR_FILTER_GATED if ok, else AWR_FILTER_HELD
 *   outputs where age != 0 after the step:  xyz_out[a] = (float)x[a];  ahead_out[a] = (float)(x[a] + d[a] * dt);
 *     uvd_out = (float) of (x0 * fx / x2 + u0, (x1 * flip) * fy / x2 + v0, x2), awr_joints_center's step 6
 *   xyz_out, uvd_out, ahead_out (B, J, 3) float32; code (B, J) int32.  Rows >= n_valid are neither read nor written.
 * The device evaluates + - * /, fabs, comparisons and the float conversions only: no square root, no transcendental.  One thread per
 * (b, j), 256 per workgroup, one launch on `stream`; each thread owns its state words: no atomics, no LDS, nothing synchronises.
 * A NULL pointer (conf with weight = 0 excepted), J outside [1, AWR_FILTER_MAX_JOINTS], B outside [1, AWR_FILTER_MAX_BATCH], n_valid
 * outside [0, B], dt not finite or <= 0, min_cutoff <= 0, beta < 0, d_cutoff <= 0, gate_mm zero or NaN, max_coast < 0, conf_floor
 * outside (0, 1], weight not 0 / 1, flip not +-1 or a zero focal length return AWR_ERR_ARG with a message, before any launch;
 * n_valid = 0 returns AWR_OK without one.  A NaN or Inf anywhere in xyz or conf is a code, never a fault. */
#define AWR_FILTER_NONE 0
#define AWR_FILTER_INIT 1
#define AWR_FILTER_UPDATED 2
#define AWR_FILTER_GATED 3
#define AWR_FILTER_HELD 4
#define AWR_FILTER_REINIT 5
#define AWR_FILTER_LOST 6
#define AWR_FILTER_MAX_JOINTS 256
#define AWR_FILTER_MAX_BATCH (1 << 20)
int awr_joints_filter(double* state, int* count, const float* xyz, const int* status, const int* ustatus, const float* conf, int B, int J,
                      int n_valid, double dt, double min_cutoff, double beta, double d_cutoff, double gate_mm, int max_coast, int weight,
                      double conf_floor, double fx, double fy, double u0, double v0, int flip, float* xyz_out, float* uvd_out,
                      float* ahead_out, int* code, void* stream);

/* ------------------------------------------------------------------------------------------
 * Hand identities across calls (csrc/awr_assign.hip; statement: awr_amd/track.py assign_step, results are bit-identical to it)
 *
 * awr_hands_assign decides, per frame, which of this call's K detected hands is which identity of the previous call.  Every (K, B, ...)
 * array is HAND-MAJOR: slot or candidate k of frame b is row k * B + b.
 *   state, updated in place:  last_uvd (K, B, 3) doubles, the uvd centre an identity was last seen at (NaN: a free slot);  ids (K, B)
 *     int32, > 0 an identity, 0 a free slot;  miss (K, B) int32, calls without a candidate;  next_id (B) int32, the next identity of
 *     the frame's batch slot (start: 1; identities are never used again; it saturates at INT_MAX).
 *   cand_uvd (K, B, 3) doubles, cand_status (K, B): this call's hands, awr_detect's outputs over awr_detect_hands' seeds.
 *   trk_uvd, trk_status: awr_detect's outputs over last_uvd as given seeds -- the tracker -- or both NULL.
 * Constants of a call, on the host in double: gate2 = gate_mm * gate_mm, merge2 = merge_mm * merge_mm.  Positions are compared in camera
 * millimetres: xyz(c) = ((c.u - u0) * c.d / fx, (c.v - v0) * c.d / fy * flip, c.d), evaluator.uvd2xyz's order;
 * |a - b|^2 = (dx * dx + dy * dy) + dz * dz.  IEEE double without contraction, + - * / and comparisons only: no square root.
 * Per frame b < n_valid:
 *   1. slot i is live iff ids > 0; with trk_*, a live slot is HELD iff its trk_status is AWR_DET_OK and its trk_uvd row is finite.
 *      r_i = xyz(trk_uvd) if held, else xyz(last_uvd).  For the pairs i < j in lexicographic order, both still held and
 *      |r_i - r_j|^2 <= merge2: the one with the larger id is released (id 0, miss 0, last_uvd NaN, AWR_ASSIGN_MERGED) and takes no further part.
 *   2. candidate j is usable iff its status is AWR_DET_OK and its row is finite; c_ij = |r_i - xyz(cand_j)|^2; (i, j) is admissible iff
 *      slot i is live, candidate j usable and c_ij <= gate2 (a NaN is not).
 *   3. over the K! permutations p of 0 .. K - 1 in lexicographic order: m(p) = the admissible (i, p[i]), s(p) = the sum of their c from
 *      0.0 in ascending i.  The largest m, then the smallest s, then the first p wins; its admissible pairs are the matches.
 *   4. a live slot that is held: centre = trk_uvd, AWR_ASSIGN_TRACKED, miss = 0, source AWR_ASSIGN_SOURCE_TRACKED; its match, if any, is
 *      consumed (the same hand seen twice).  Not held but matched: the candidate's centre, AWR_ASSIGN_MATCHED, miss = 0, source j.
 *      Neither: miss += 1, no centre; AWR_ASSIGN_COASTING while miss <= max_miss, beyond it released as in 1. with AWR_ASSIGN_LOST.
 *   5. births: the usable candidates not consumed, in ascending j, each take the lowest free slot; if none is free, the COASTING slot of
 *      this step with the largest miss (the lowest index on ties), whose identity ends; if there is neither, dropped[b] += 1.  A birth:
 *      id = next_id++, miss = 0, AWR_ASSIGN_BORN, reset = 1, source j.
 *   6. centers (K, B, 3) doubles: the slot's centre bit for bit, NaN without one;  status (K, B): AWR_DET_OK with a centre, else
 *      AWR_DET_EMPTY;  code (K, B): AWR_ASSIGN_*;  reset (K, B): 1 for a birth;  source (K, B);  dropped (B).  last_uvd takes the centre
 *      where the status is AWR_DET_OK.  With filter_state ((K * B, J, 6) doubles) and filter_count ((K * B, J, 2) int32), awr_joints_filter's
 *      state over the same rows (both NULL: none), the rows of every slot with reset = 1 or a released identity are zeroed: no track.
 * Frames >= n_valid keep their state; their outputs are NaN / AWR_DET_EMPTY / AWR_ASSIGN_FREE / 0 / AWR_ASSIGN_SOURCE_NONE / 0.
 * One wave per frame, four frames per 256-thread workgroup: lane p < K! evaluates permutation p, an xor-shuffle reduction over the total
 * order of 3. picks the winner; no atomics, no LDS, nothing synchronises, one launch on `stream`.  A NULL pointer (trk_* and filter_*
 * excepted, each pair NULL together), K outside [1, AWR_ASSIGN_MAX_HANDS], B outside [1, AWR_FILTER_MAX_BATCH], n_valid outside [0, B],
 * gate_mm not finite or <= 0, merge_mm not finite or < 0, max_miss outside [0, INT_MAX), flip not +-1, a zero focal length or, with
 * filter_state, J outside [1, AWR_FILTER_MAX_JOINTS] return AWR_ERR_ARG with a message, before any launch.  K = 1 is legal. */
#define AWR_ASSIGN_FREE 0
#define AWR_ASSIGN_BORN 1
#define AWR_ASSIGN_MATCHED 2
#define AWR_ASSIGN_TRACKED 3
#define AWR_ASSIGN_COASTING 4
#define AWR_ASSIGN_LOST 5
#define AWR_ASSIGN_MERGED 6
#define AWR_ASSIGN_SOURCE_NONE (-1)
#define AWR_ASSIGN_SOURCE_TRACKED (-2)
#define AWR_ASSIGN_MAX_HANDS 4
int awr_hands_assign(double* last_uvd, int* ids, int* miss, int* next_id, const double* cand_uvd, const int* cand_status, const double* trk_uvd,
                     const int* trk_status, int K, int B, int n_valid, double gate_mm, double merge_mm, int max_miss, double fx, double fy,
                     double u0, double v0, int flip, double* filter_state, int* filter_count, int J, double* centers, int* status, int* code,
                     int* reset, int* source, int* dropped, void* stream);

/* ------------------------------------------------------------------------------------------
 * Label-free check of joints against the depth frame (csrc/awr_surface.hip; statement: awr_amd/surface.py joints_surface, results are
 * bit-identical to it)
 *
 * awr_joints_surface asks, per joint and per sample along a bone, what the sensor saw at the point's pixel.  Inputs per row r < n:
 *   uvd (n, J, 3) float32: original-image pixel u, v and depth in millimetres, as awr_joints_unproject / awr_views_fuse write it;
 *   the row's frame frame[r] of the frame store: uint16 millimetres, 0 means no measurement;  status, ustatus (n): the row's codes.
 *   bones: n_bones pairs of int32 joint indices on the device (NULL with n_bones = 0);  samples points along each bone.
 * The rule:
 *
 * A point is a triple (u, v, d) in float64. A joint's point is its float32 values converted exactly. Sample s = 1 ... samples of bone
 * (a, b) is p = A + (B - A) * (s / (samples + 1)), per component in float64, in exactly this order. It is linear in uvd, not in camera
 * space.
 * For one point:
 *   1. If u, v or d is not finite, the code is OUTSIDE.
 *   2. Otherwise pu = floor(u + 0.5) and pv = floor(v + 0.5), clamped before the integer conversion as awr_frame.h's trunc_clamped does.
 *      If pu is not in [0, fw) or pv is not in [0, fh), the code is OUTSIDE.
 *   3. W is the set of in-frame pixels of the (2 * radius + 1)^2 window around (pu, pv). The centre is included and the window is
 *      clipped at the frame's edges.
 *   4. For q in W with d_q != 0: g_q = d - (double)d_q.
 *   5. n_on = #{-out_mm <= g_q <= in_mm}, n_front = #{g_q > in_mm}.
 *   6. The code is ON (0) if n_on >= min_on; else OCCLUDED (1) if n_front >= 1; else OFF (2). A window of zeros only is OFF too.
 *   7. The gap is the g_q of smallest |g_q|, the positive one on a tie of +g and -g, rounded to float32. It is NaN if no pixel of W is
 *      valid, and NaN for OUTSIDE. It is a value, not a position, so the scan order cannot matter.
 * A row whose status is not AWR_DET_OK or whose ustatus is not 0 is SKIPPED: every code of the row is 4, its gaps are NaN, its counts are
 * 0 and its row_status is 1; its frame index is not looked at. Otherwise a row whose frame index lies outside [0, n_frames) gets
 * row_status 2 and the same outputs. Rows at or past n_valid are not written at all.
 * A bone with an index outside [0, J) yields OUTSIDE samples, never a fault.
 *
 * Outputs per row:  codes (n, J) int32;  gap_mm (n, J) float32 (every NaN is the quiet NaN 0x7FC00000);  counts (n, 8) int32: joints
 * ON / OCCLUDED / OFF / OUTSIDE, then bone samples ON / OCCLUDED / OFF / OUTSIDE;  row_status (n) int32.
 *   radius in [0, AWR_SURFACE_MAX_RADIUS]; in_mm, out_mm finite and >= 0; min_on in [1, (2 radius + 1)^2]; n_bones in
 *   [0, AWR_SURFACE_MAX_BONES]; samples in [1, AWR_SURFACE_MAX_SAMPLES]; J in [1, AWR_SURFACE_MAX_JOINTS]; n in [1, AWR_DET_MAX_BATCH],
 *   n_valid in [0, n], fh, fw in [1, 16384]; only uint16 frames: anything else returns AWR_ERR_ARG with a message that names the entry
 *   point and the value, before any launch; n_valid = 0 returns AWR_OK without one.
 * ONE launch on `stream`: one wave per row, its lanes stride over the row's J + n_bones * samples points, each lane gathers its window
 * with 2-byte loads and the eight counts are two packed wave sums.  Comparisons and exact differences in double, the one interpolation
 * without contraction.  No atomics, no LDS, no scratch, nothing synchronises. */
#define AWR_SURFACE_ON 0
#define AWR_SURFACE_OCCLUDED 1
#define AWR_SURFACE_OFF 2
#define AWR_SURFACE_OUTSIDE 3
#define AWR_SURFACE_SKIPPED 4
#define AWR_SURFACE_ROW_OK 0
#define AWR_SURFACE_ROW_SKIPPED 1
#define AWR_SURFACE_ROW_BAD_FRAME 2
#define AWR_SURFACE_MAX_RADIUS 3
#define AWR_SURFACE_MAX_JOINTS 256
#define AWR_SURFACE_MAX_BONES 64
#define AWR_SURFACE_MAX_SAMPLES 7
int awr_joints_surface(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame /* n */,
                       const float* uvd /* n,J,3 */, const int* status /* n */, const int* ustatus /* n */, int n, int J, int n_valid,
                       const int* bones /* n_bones,2 or NULL */, int n_bones, int samples, int radius, double in_mm, double out_mm,
                       int min_on, int* codes /* n,J */, float* gap_mm /* n,J */, int* counts /* n,8 */, int* row_status /* n */,
                       void* stream);

/* Static-scene background model (csrc/awr_background.hip; the numpy statements are awr_amd/background.py learn and
 * foreground, results are bit-identical to them).  Every other stage assumes that the hand is the nearest thing in the frame; with a
 * fixed sensor there may be static things nearer than it.  A model is learnt once from frames of the scene without a hand, and a pass in
 * front of every other stage keeps only what is nearer than the model.
 *
 * Learning a model.  The model is one uint16 depth per pixel, and 0 means "no background known here".
 *
 *   Input: n listed frames of the store, 1 <= n <= AWR_BG_MAX_FRAMES = 64, a rank in {MIN, MEDIAN, MAX}, min_valid in [1, n].
 *   For pixel p: V = the multiset { frame_i[p] : frame_i[p] != 0 }, over the listed frames whose index lies inside the store.
 *     - If |V| < min_valid the model is 0.
 *     - Otherwise the model is element k of the ascending sort of V: k = 0 (MIN), (|V| - 1) // 2 (MEDIAN, the lower median), |V| - 1 (MAX).
 *       It is a value that occurs, never an average.
 *   A listed frame index outside the store contributes no value to any pixel; the call's one status word is then AWR_DET_BAD_FRAME, else
 *   AWR_DET_OK.
 *
 * MEDIAN survives sensor noise and a hand that crosses a pixel in fewer than half the frames; MIN is the conservative choice for an
 * empty-scene capture; MAX suits a capture in which a person walks through.
 *   n, rank, min_valid outside those ranges, model_out overlapping the n_frames rows of the store, a frame store check_frame_store
 *   refuses (only uint16 frames; fh, fw in [1, 16384]): AWR_ERR_ARG with a message that names the entry point and the value, before any
 *   launch.
 * ONE launch on `stream`: a workgroup of 256 threads stages n x 256 depths in at most 32 KB of LDS, frame-major, and each thread selects
 * element k of its pixel's column by building the answer from bit 15 down out of counts.  No atomics, integers only. */
#define AWR_BG_MAX_FRAMES 64
#define AWR_BG_MIN 0
#define AWR_BG_MEDIAN 1
#define AWR_BG_MAX 2
int awr_background_learn(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame /* n */, int n, int rank,
                         int min_valid, void* model_out /* fh,fw uint16 */, int* status /* 1 */, void* stream);

/* Applying it.  The pass is pointwise.  Every output pixel depends on that pixel of the input frame and of the model alone.
 *
 *   d = input depth, m = model depth, both as int. margin = floor(min(margin_mm, 65535)) (awr_frame.h's depth_floor, the integer form 4.29
 *   and 4.30 use; negative or NaN is refused before any launch). unknown_keep in {0, 1}.
 *     keep = d != 0 and ( m == 0 ? unknown_keep == 1 : d + margin < m )        -- int arithmetic: d + margin may reach 131070 and must not wrap
 *     out  = keep ? d : 0
 *   With adapt = step >= 1, for rows b < n_valid only, and only at pixels with d != 0, m != 0 and not keep (a valid background pixel):
 *     m' = m + min(max(d - m, -step), step)                                    -- between m and d, so it stays in [1, 65535]
 *   Every other model pixel keeps its value. adapt = 0: the model is only read.
 *   Row b reads frame index frame[b] (outside the store: a zero output row, status AWR_DET_BAD_FRAME, no adaptation) and model row
 *   (per_row ? b : 0).
 *
 * So an all-zero model with unknown_keep = 1 passes every frame through unchanged; a hand is foreground and is never absorbed by adapt;
 * furniture moved NEARER after learning stays foreground until the model is learnt again (a stated limitation).
 * out: B rows in the FrameStore layout.  model: model_rows rows of fh x fw uint16.  status (B).
 *   Refused with AWR_ERR_ARG and a message, before any launch: `out` overlapping the n_frames rows of the frame store, or the model_rows
 *   rows of the model overlapping either; adapt > 0 with per_row == 0 and B > 1 (several rows would race on one model); model_rows <
 *   (per_row ? B : 1); n_valid outside [0, B]; margin negative or NaN; unknown_keep or per_row outside {0, 1}; adapt outside [0, 65535];
 *   B outside [1, AWR_DET_MAX_BATCH], fh, fw outside [1, 16384], frames that are not uint16.
 * ONE launch on `stream`, about 6 bytes per pixel, 8 with adapt: a thread owns 8 pixels of a row -- one 16-byte load of the frame, one of
 * the model, one 16-byte store of the output and, with adapt, one of the model (fw a multiple of 8 and the three bases 16-byte aligned;
 * otherwise a thread per pixel with 2-byte accesses).  adapt is a compile-time form of the same kernel: the form without it never writes
 * the model.  A model pixel is read and written by one thread only.  No atomics, no LDS, no floating point on the device, nothing
 * synchronises. */
int awr_frames_foreground(const void* frames, int frame_type, int64_t n_frames, int fh, int fw, const int64_t* frame /* B */, int B,
                          int n_valid, void* model /* model_rows,fh,fw uint16 */, int model_rows, int per_row, double margin,
                          int unknown_keep, int adapt, void* out /* B,fh,fw uint16 */, int* status /* B */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AWR_HIP_H */
