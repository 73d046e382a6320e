/* medt_abi.h -- C ABI of libmedt_hip.so, the MI355X (gfx950) implementation of
 * Medical-Transformer's gated axial-attention hot path.
 *
 * The reference has no FFI / plugin interface for this path: it is ~5.6 kLoC of
 * Python whose hot path lives behind a *Python module surface*
 * (lib/models/axialnet.py).  The drop-in boundary is therefore that module
 * surface (mirrored in medical-transformer_amd/lib/), and THIS header is the
 * boundary underneath it: what the mirrored modules' forward/backward bind
 * through ctypes instead of the stock torch ops the reference dispatches.
 * Each entry point cites the reference lines it replaces.
 *
 * Conventions
 *   - plain C: no C++ or torch types cross the boundary.
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch's
 *     allocator); the library never allocates, frees or retains device memory.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); all work
 *     is enqueued on it, nothing synchronises -> the calls are hipGraph-capturable.
 *   - tensors are contiguous NCHW float32 unless stated.
 *   - alignment: tensors are expected 16-byte aligned (what every device allocator returns; sub-tensor views at channel or
 *     image granularity keep it because H*W is a multiple of 4 for every shape of the networks).  Kernels that stage 16-byte
 *     pieces through LDS check the pointers per call and fall back to element-wise movers when a tensor is not.
 *   - return 0 on success, <0 on error (MEDT_E*); medt_last_error() returns a
 *     thread-local message.  No global mutable state: safe to call concurrently
 *     from several host threads on different streams (nn.DataParallel's
 *     thread-per-replica model, reference train.py:104-107).
 */
#ifndef MEDT_ABI_H
#define MEDT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 11: medt_seg_loss_*.  The medt_augment_* entry points were added under the same number: additions only, nothing that
 * version 11 declared was removed or changed, so a caller built against the earlier header keeps working.  The medt_edt_*
 * entry points were added under the same number: additions only, nothing that version 11 declared was removed or changed,
 * so a caller built against the earlier header keeps working.  The medt_label_* entry points were added under the same
 * number: additions only, nothing that version 11 declared was removed or changed, so a caller built against the earlier
 * header keeps working.  medt_label_boxes and medt_pair_hausdorff were added under the same number, in the same way.
 * medt_signed_edt and the medt_boundary_* entry points were added under the same number, in the same way.  medt_object_edt2
 * and the medt_border_* entry points were added under the same number, in the same way.  The medt_split_* and medt_grow_*
 * entry points were added under the same number, in the same way.  medt_augment_warp was added under
 * the same number, in the same way. */
#define MEDT_ABI_VERSION 11

#define MEDT_OK            0
#define MEDT_EINVAL       -1   /* bad descriptor / null pointer / size mismatch            */
#define MEDT_EUNSUPPORTED -2   /* geometry outside what the kernels are built for            */
#define MEDT_ELAUNCH      -3   /* hipLaunchKernel / hipGetLastError reported a failure        */
#define MEDT_EWORKSPACE   -4   /* workspace smaller than medt_*_workspace_bytes()             */

int         medt_abi_version(void);
const char* medt_last_error(void);

/* ------------------------------------------------------------------------- *
 * Deferred, grouped execution of the work no later LAYER waits for (optional).
 *   The reference's loss.backward() / optimizer.step() (train.py:159-161) makes every Conv2d weight gradient, bias
 *   gradient and BatchNorm bookkeeping update its own kernel launch in the middle of the dependent chain.  With a
 *   queue bound to a stream, the layer entry points below RECORD those launches instead (weight / bias gradients and
 *   the reductions of their partial slabs, the relative-table / gate reductions, the saved-statistics + running-stat
 *   finalisation and BatchNorm parameter gradients of the fused small-layer kernels) and medt_queue_flush() issues
 *   everything recorded as a few grouped launches -- call it after the forward pass (backward reads the saved
 *   statistics) and after the backward pass (the optimizer reads the gradients).  The caller must keep every buffer
 *   it passed to a recording call (inputs, outputs, saved tensors, workspace) alive and unmodified until the flush.
 *   Same kernel bodies as the immediate launches; results are identical except that weight gradients are summed over
 *   differently sized position chunks (fp32 rounding, ~1e-7 relative).
 *   Without a bound queue every call launches immediately (the default).
 * ------------------------------------------------------------------------- */
void*  medt_queue_create(void);
int    medt_queue_destroy(void* queue);
int    medt_queue_bind(void* queue, void* stream);      /* queue == NULL: unbind the stream */
size_t medt_queue_pending(const void* queue);            /* recorded, not yet flushed */
int    medt_queue_flush(void* queue, void* stream);      /* enqueue everything recorded on `stream` */
/* ... with the dedicated MFMA weight-gradient launches on `aux_stream` (another stream of the caller's, idle by now; NULL or == stream:
 * medt_queue_flush), forked from and joined back into `stream` by events: after the call everything is ordered on `stream` (ABI v9) */
int    medt_queue_flush2(void* queue, void* stream, void* aux_stream);
int    medt_queue_discard(void* queue);                  /* drop everything recorded WITHOUT launching it (error paths: the
                                                            buffers the jobs point into are about to be released) */

/* ------------------------------------------------------------------------- *
 * Axial attention layer
 *   replaces AxialAttention.forward          lib/models/axialnet.py:52-92
 *            AxialAttention_dynamic.forward  lib/models/axialnet.py:142-189
 *            AxialAttention_wopos.forward    lib/models/axialnet.py:222-253
 *   and their autograd backward.
 * ------------------------------------------------------------------------- */
typedef struct medt_axial_desc {
    int32_t N, C, H, W;     /* input (N,C,H,W); in_planes == out_planes == C                     */
    int32_t G;              /* heads ("groups", always 8 in the reference); gp = C/G, gp even    */
    int32_t axis;           /* 0: attend along H (width=False, :146); 1: along W (width=True)    */
    int32_t has_pos;        /* 1: relative-position tables + BN2d(3G) (:155-167); 0: wopos       */
    int32_t stride;         /* AvgPool2d(stride) after the layer (:186-187); 1 or 2              */
    int32_t training;       /* 1: batch statistics + running-stat update; 0: running statistics  */
    int32_t bn_groups;      /* BN statistic groups along N (N % bn_groups == 0).  1 normally; 16
                               when the 16 LoGo patches (:661-700) are stacked patch-major on N:
                               each group is normalised with its own statistics and the running
                               stats receive the groups' updates in order.        */
    float   eps;            /* 1e-5 */
    float   momentum;       /* 0.1  */
    int32_t out_relu;       /* 1: fuse the block's ReLU after the width layer (:333) into the output pass */
    int32_t gate_mode;      /* 0: f_* multiply as stored (axialnet.py:163-164,175-176);
                               1: sigmoid(f_*) multiplies -- AxialAttention_gated_sig, lib/models/model_codes.py:279-280,
                                  292-293; the gate gradients returned are then wrt the stored (pre-sigmoid) values;
                               2: one set of gates PER SEQUENCE -- AxialAttention_gated_data, model_codes.py:406-407,420-421:
                                  params.f_qr points to a (B*, 4) tensor with columns (qr, kr, sv, sve), B* = N*W (axis 0) or
                                  N*H (axis 1), sequence b = n*Bo + s; f_kr / f_sve / f_sv are ignored; grads.gates receives the
                                  (B*, 4) gradient in the same layout; the generic (not the bandwidth-tuned) kernels run */
    int32_t act_dtype;      /* storage type of saved->qkv_raw and saved->stacked: 0 float32 (the reference's arithmetic and
                               storage), 1 bfloat16 (BASELINE.json configs[1]: half the attention path's HBM bytes;
                               accumulation, statistics, x / y / dx and every gradient stay float32).  has_pos only. */
} medt_axial_desc;

typedef struct medt_bn_ptrs {
    const float* weight;            /* (CH)                                            */
    const float* bias;              /* (CH)                                            */
    float*       running_mean;      /* (CH)  updated in place when training            */
    float*       running_var;       /* (CH)                                            */
    int64_t*     num_batches_tracked; /* 0-d int64, += bn_groups when training; may be NULL */
} medt_bn_ptrs;

typedef struct medt_axial_params {
    const float* w_qkv;             /* qkv_transform.weight (2C, C[,1])                 :114 */
    medt_bn_ptrs bn_qkv;            /* BatchNorm1d(2C)                                  :116 */
    medt_bn_ptrs bn_similarity;     /* BatchNorm2d(3G)  (G when !has_pos)               :117 */
    medt_bn_ptrs bn_output;         /* BatchNorm1d(2C)  (C when !has_pos)               :118 */
    const float* relative;          /* (2gp, 2L-1); NULL when !has_pos                  :131 */
    const float* f_qr;              /* 0-d gates (:124-127); NULL == 1.0 (AxialAttention)    */
    const float* f_kr;
    const float* f_sve;
    const float* f_sv;
} medt_axial_params;

/* Activations kept between forward and backward (caller-allocated). */
typedef struct medt_axial_saved {
    void*  qkv_raw;   /* (N, 2C, H, W)  qkv_transform output before bn_qkv; float32 or bfloat16 (desc.act_dtype) */
    void*  stacked;   /* (N, OC, H, W)  sv|sve before bn_output, channel 2(g*gp+c)+{0:sv,1:sve};
                         OC = 2C (has_pos) or C (wopos: sv only); float32 or bfloat16 (desc.act_dtype)  */
    float* lse;       /* (N, G, H, W)   log2-domain log-sum-exp of every softmax row           */
    float* stats;     /* medt_axial_stats_floats() floats: per-BN mean / rstd / scale / shift  */
} medt_axial_saved;

typedef struct medt_axial_grads {   /* all written (not accumulated) by medt_axial_layer_bwd */
    float* w_qkv;                   /* (2C, C)                                   */
    float* bn_qkv_weight;  float* bn_qkv_bias;        /* (2C)                    */
    float* bn_sim_weight;  float* bn_sim_bias;        /* (3G) or (G)             */
    float* bn_out_weight;  float* bn_out_bias;        /* (2C) or (C)             */
    float* relative;                /* (2gp, 2L-1) or NULL                       */
    float* gates;                   /* 4 floats [f_qr, f_kr, f_sve, f_sv] or NULL (skip) */
} medt_axial_grads;

size_t medt_axial_stats_floats(const medt_axial_desc*);
size_t medt_axial_workspace_bytes(const medt_axial_desc*);   /* max over fwd and bwd */

/* x (N,C,H,W) -> y (N,C,H/stride,W/stride).  `saved` may have NULL lse when !training
 * is used for inference only (qkv_raw, stacked and stats are always needed as scratch). */
int medt_axial_layer_fwd(const medt_axial_desc*, const medt_axial_params*, const float* x, float* y,
                         const medt_axial_saved*, void* workspace, size_t workspace_bytes, void* stream);

/* dy (N,C,H/stride,W/stride) -> dx (N,C,H,W) + parameter gradients.  Training-mode
 * statistics are differentiated through (the reference's autograd does); with
 * desc.training == 0 the BatchNorms are the affine maps of their running stats. */
int medt_axial_layer_bwd(const medt_axial_desc*, const medt_axial_params*, const float* x, const float* y,
                         const float* dy, const medt_axial_saved*, float* dx, const medt_axial_grads*,
                         void* workspace, size_t workspace_bytes, void* stream);
/* y: forward output, needed iff out_relu. */

/* The stages of the attention core on their own, for benchmarks / profiling (bench.py's roofline legs): the bn_similarity
 * statistics pass (closed form: one read of q,k) and the fused logits + softmax + sv|sve pass, given the BN scale/shift
 * already in saved->stats.  Same kernels the layer entry points launch.  Call medt_axial_layer_fwd once with the same
 * descriptor and workspace first: it leaves the sliding-window tables the statistics kernel reads in the workspace. */
int medt_axial_core_stats(const medt_axial_desc*, const medt_axial_params*, const medt_axial_saved*,
                          void* workspace, size_t workspace_bytes, void* stream);
int medt_axial_core_fwd(const medt_axial_desc*, const medt_axial_params*, const medt_axial_saved*,
                        void* workspace, size_t workspace_bytes, void* stream);
/* The two L x L backward passes (bn_similarity backward statistics; dq/dk/dv + relative-table and gate gradients) on
 * their own, for benchmarks: call medt_axial_layer_bwd once with the same descriptor and workspace first (it leaves the
 * bn_output / bn_similarity backward coefficients these passes read in the workspace).  Same kernels as the layer call. */
int medt_axial_core_bwd(const medt_axial_desc*, const medt_axial_params*, const medt_axial_saved*, const float* dy,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * A whole AxialBlock_wopos forward as ONE launch (lib/models/axialnet.py:368-391):
 *   y = relu( bn2(conv_up( relu(width_block(hight_block( relu(bn1(conv_down(x))) ))) )) + x )
 * for the deep blocks of the LoGo local branch (:661-700), whose BatchNorm group (4 images on 4x4 maps) fits one
 * workgroup: stride 1, no downsample, in_planes == out_planes == C, attention width `width`.  The saved tensors are
 * exactly those medt_conv_block_fwd / medt_axial_layer_fwd would have produced for the four stages, so the backward runs
 * through medt_conv_block_bwd / medt_axial_layer_bwd unchanged.  medt_wopos_block_workspace_bytes() returns 0 for shapes
 * the fused kernel is not built for (the caller then uses the per-stage entry points).
 * ------------------------------------------------------------------------- */
typedef struct medt_block_desc {
    int32_t N, C, width, H, W;   /* x, y: (N,C,H,W); the attention layers work on (N,width,H,W)      */
    int32_t G;                   /* heads                                                            */
    int32_t training, bn_groups; /* as in medt_axial_desc                                            */
    float   eps, momentum;
} medt_block_desc;

typedef struct medt_block_params {
    const float*      w_down;    /* conv_down.weight (width, C)                                 :355 */
    medt_bn_ptrs      bn1;       /* BatchNorm2d(width)                                          :356 */
    medt_axial_params height;    /* hight_block: w_qkv + the three BatchNorms (relative / f_* NULL)  */
    medt_axial_params width;     /* width_block                                                      */
    const float*      w_up;      /* conv_up.weight (C, width)                                   :359 */
    medt_bn_ptrs      bn2;       /* BatchNorm2d(C)                                              :360 */
} medt_block_params;

typedef struct medt_block_saved {
    float* z1;                   /* (N,width,H,W) conv_down output before bn1                        */
    float* y1;                   /* (N,width,H,W) relu(bn1(z1)) = input of the height layer          */
    float* stats1;               /* medt_conv_stats_floats() of the conv_down block                  */
    medt_axial_saved height;     /* as medt_axial_layer_fwd fills it for the height layer            */
    float* y_h;                  /* (N,width,H,W) height layer output = input of the width layer     */
    medt_axial_saved width;
    float* y_w;                  /* (N,width,H,W) relu(width layer output) = input of conv_up        */
    float* z2;                   /* (N,C,H,W) conv_up output before bn2                              */
    float* stats2;               /* medt_conv_stats_floats() of the conv_up block                    */
} medt_block_saved;

size_t medt_wopos_block_workspace_bytes(const medt_block_desc*);      /* 0: not a shape of the fused kernel */
int medt_wopos_block_fwd(const medt_block_desc*, const medt_block_params*, const float* x, float* y,
                         const medt_block_saved*, void* workspace, size_t workspace_bytes, void* stream);

/* The STRIDE-2 first block of a layer with its downsample path as one launch (round 6, ABI v9): AxialBlock_wopos(C -> width ->
 * 2*width, stride 2) + downsample = Sequential(conv1x1(C, 2*width, stride 2), BatchNorm2d) -- lib/models/axialnet.py:368-391 with
 * :596-606 -- x (N,C,H,W) -> y (N,2*width,H/2,W/2).  `blk` fields as above except: width.stats / y_w describe the width layer
 * WITH its AvgPool2d(2) (y_w: (N,width,H/2,W/2), pooled and ReLU'd), z2 / stats2: (N,2*width,H/2,W/2).  zd / yd / statsd: the
 * downsample block's conv output, its BatchNorm output (the identity added behind bn2) and its saved statistics
 * (medt_conv_stats_floats of that block).  Fused shape: 4x4 maps, C = width = 128, 4 images per BatchNorm group (layer4_p.0 of
 * MedT at 128 px); medt_wopos_block_s2_workspace_bytes() returns 0 otherwise (or with MEDT_BLOCK_S2=0). */
typedef struct medt_block_s2_params {
    medt_block_params blk;
    const float*      w_ds;      /* downsample[0].weight (2*width, C)                           :600 */
    medt_bn_ptrs      bn_ds;     /* downsample[1]                                               :601 */
} medt_block_s2_params;
typedef struct medt_block_s2_saved {
    medt_block_saved blk;
    float *zd, *yd, *statsd;
} medt_block_s2_saved;
size_t medt_wopos_block_s2_workspace_bytes(const medt_block_desc*);
int medt_wopos_block_s2_fwd(const medt_block_desc*, const medt_block_s2_params*, const float* x, float* y,
                            const medt_block_s2_saved*, void* workspace, size_t workspace_bytes, void* stream);

/* The same block's BACKWARD as one launch: dy -> dx through bn2, conv_up, the two attention layers, bn1 and conv_down,
 * the identity's gradient and `dx_add` (the other consumers' contribution to d(x), may be NULL) summed in the last phase;
 * every parameter gradient in `grads` is written (not accumulated) -- when a queue is bound to the stream the weight
 * gradients and the BatchNorm parameter reductions are recorded for the grouped flush exactly like the per-stage entry
 * points record theirs.  `saved` is what medt_wopos_block_fwd (or the four per-stage forwards) filled, `y` the block output.
 * medt_wopos_block_bwd_workspace_bytes() returns 0 when this path is not available for the shape or not enabled
 * (on by default, MEDT_BLOCK_BWD=0 disables; the caller then runs medt_conv_block_bwd / medt_axial_layer_bwd for the four stages).
 * State: verified against the reference fixture on the CPU lane emulator (tests/test_lane_emu.py) and on the MI355X
 * (tests/test_block_gpu.py); default since round 5 (profiles/r05_never_run_kernels.txt, profiles/r05_step_ab.json). */
typedef struct medt_block_grads {
    float *w_down, *bn1_weight, *bn1_bias;
    medt_axial_grads height, width;          /* relative / gates: NULL (position-free layers)                 */
    float *w_up, *bn2_weight, *bn2_bias;
} medt_block_grads;
size_t medt_wopos_block_bwd_workspace_bytes(const medt_block_desc*);
int medt_wopos_block_bwd(const medt_block_desc*, const medt_block_params*, const float* x, const float* y, const float* dy,
                         const medt_block_saved*, float* dx, const float* dx_add, const medt_block_grads*,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Convolution block:  y = act( BN( conv2d(x, w) + bias ) + res )
 *   replaces the nn.Conv2d / nn.BatchNorm2d / ReLU / residual-add sequences of
 *   AxialBlock*.forward (lib/models/axialnet.py:285-300, 327-342, 373-389), the stems
 *   (:475-483, :623-632, :666-678), downsample (:450-454), decoders / adjust (:434-439, :493-502).
 * ------------------------------------------------------------------------- */
typedef struct medt_conv_desc {
    int32_t N, Cin, H, W, Cout;
    int32_t K, stride, pad;       /* square kernels: 1, 3 or 7                                   */
    int32_t has_bias;             /* nn.Conv2d bias                                              */
    int32_t has_bn;               /* BatchNorm2d on the conv output                              */
    int32_t has_res;              /* residual added after BN (block identity / downsample)       */
    int32_t relu;                 /* ReLU last                                                   */
    int32_t training, bn_groups;  /* as in medt_axial_desc.  `training` also means "a backward pass follows this forward":
                                     for has_bn == 0 it changes no result, but a training-mode forward of a 3x3 layer whose
                                     backward-data runs on the MFMA kernel leaves that kernel's flipped weights in `stats`
                                     (below) -- pass the same value to medt_conv_block_bwd                                */
    float   eps, momentum;
    int32_t lean;                 /* scheduling hint, no effect on results.  1: the caller runs CU-filling kernels on ANOTHER
                                     stream at the same time (MedT's global branch at 256 px: persistent attention kernels that
                                     hold ~all of a CU's LDS): keep to the per-stage kernels, whose workgroups co-reside with
                                     anything, instead of the fused BatchNorm-backward + dgrad kernel (tens of KB of LDS per
                                     workgroup -- measured: +0.5 ms on the 5.7 ms MedT-256 step, -0.02 ms on the MedT-128 step) */
} medt_conv_desc;

/* Floats the caller must allocate for `stats` -- ALWAYS size it with this call, never by formula (ABI v9).  Layout:
 *   [0, 4*bn_groups*Cout)                    saved BatchNorm statistics (mean, rstd, scale, shift) when has_bn, else empty;
 *   [align_up(that, 64), + Cout*Cin*K*K)     only for training-mode K == 3 layers whose backward-data takes the MFMA kernel
 *                                            (has_bn or not): the flipped / transposed weights, written by the forward (or by
 *                                            the flush of the queue bound to its stream) and read by medt_conv_block_bwd.
 * 0 means "no stats buffer needed" (pass NULL or a dummy).  The same buffer goes to medt_conv_block_fwd and _bwd. */
size_t medt_conv_stats_floats(const medt_conv_desc*);
size_t medt_conv_workspace_bytes(const medt_conv_desc*);   /* max over fwd and bwd              */

/* z: conv output (N,Cout,Ho,Wo), kept for backward when has_bn (pass z == y otherwise). */
int medt_conv_block_fwd(const medt_conv_desc*, const float* x, const float* w, const float* bias,
                        const medt_bn_ptrs* bn, const float* res, float* z, float* y, float* stats,
                        void* workspace, size_t workspace_bytes, void* stream);
/* Two INDEPENDENT blocks A and B (neither reads what the other writes) in side-by-side launches: the arguments of
 * medt_conv_block_fwd twice, each member with its own workspace sized by medt_conv_workspace_bytes.  Every output (z, y, stats, the
 * recorded jobs of a bound queue, A's before B's) is bit-identical to medt_conv_block_fwd(A) followed by medt_conv_block_fwd(B).
 * Where both members take the same kernel family (1x1 + BatchNorm: the fused small-group kernel, or convolution + statistics/apply)
 * each stage is ONE launch whose grid carries both problems; any other combination runs the two single plans.  Built for the first
 * unit of a layer, where conv_down and the downsample path read the same x (axialnet.py:327, 339-340). */
int medt_conv_block_pair_fwd(const medt_conv_desc* da, const float* xa, const float* wa, const float* biasa,
                             const medt_bn_ptrs* bna, const float* resa, float* za, float* ya, float* statsa,
                             void* workspace_a, size_t workspace_a_bytes,
                             const medt_conv_desc* db, const float* xb, const float* wb, const float* biasb,
                             const medt_bn_ptrs* bnb, const float* resb, float* zb, float* yb, float* statsb,
                             void* workspace_b, size_t workspace_b_bytes, void* stream);
/* dx, dbias, dres may be NULL (not needed).  dw, dbn_weight, dbn_bias are written, not accumulated.
 * dx_add (optional, same shape as dx): dx = conv-backward + dx_add.  The input of an AxialBlock feeds conv_down AND the
 * residual / downsample path (axialnet.py:327,339-340) and the decoder skips (:494-500); the reference's autograd sums
 * those gradients with separate add kernels, here the last producer adds the others in its epilogue. */
int medt_conv_block_bwd(const medt_conv_desc*, const float* x, const float* w, const medt_bn_ptrs* bn,
                        const float* z, const float* y, const float* stats, const float* dy,
                        float* dx, float* dw, float* dbias, float* dbn_weight, float* dbn_bias, float* dres,
                        const float* dx_add, void* workspace, size_t workspace_bytes, void* stream);

/* The gate network of AxialAttention_gated_data (lib/models/model_codes.py:371-380):
 *   xn = mean over the sequence of x (B*, C);  h = relu(fcn1(xn));  o = relu(fcn2(h));  gates = sigmoid(o)   (B*, 4)
 * xn, h (B*, C) and o (B*, 4) are kept for the backward.  bwd: scratch = B* * (4 + 2C) floats; dw1 (C,C), db1 (C), dw2 (4,C),
 * db2 (4) and dx (N,C,H,W: the gradient that reaches x THROUGH the gates) are written, not accumulated. */
int medt_gate_mlp_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* xn, float* h,
                      float* o, float* gates, int N, int C, int H, int W, int axis, void* stream);
int medt_gate_mlp_bwd(const float* dgates, const float* gates, const float* o, const float* h, const float* xn,
                      const float* w1, const float* w2, float* scratch, float* dw1, float* db1, float* dw2, float* db2,
                      float* dx, int N, int C, int H, int W, int axis, void* stream);

/* y = relu(bilinear_x2(x)) + skip       F.interpolate(scale_factor=(2,2), mode='bilinear') + relu + torch.add
 * (lib/models/axialnet.py:493-501, 650-652, 690-698).  x (NC,H,W) -> y (NC,2H,2W); skip may be NULL.
 * Backward: dskip = dy (aliased by the caller), dx via medt_up2x_relu_bwd (needs x to rebuild the ReLU mask). */
int medt_up2x_relu_add_fwd(const float* x, const float* skip, float* y, int NC, int H, int W, void* stream);
int medt_up2x_relu_bwd(const float* x, const float* dy, float* dx, int NC, int H, int W, void* stream);

/* LoGo local branch plumbing (lib/models/axialnet.py:658-702): gather the G x G grid of P-px patches of
 * x (N,C,S,S) into (G*G*N, C, P, P), patch-major;  y = x + x_loc with x_loc = x overwritten by the patches. */
int medt_patch_gather(const float* x, float* xp, int N, int C, int S, int P, int G, void* stream);
int medt_logo_merge_fwd(const float* x, const float* yp, float* y, int N, int C, int S, int P, int G, void* stream);
int medt_logo_merge_bwd(const float* dy, float* dx, float* dyp, int N, int C, int S, int P, int G, void* stream);

/* LogNLLLoss.forward == F.cross_entropy(mean, ignore_index) (metrics.py:17-20).  logits (N,K,HW) float,
 * target (N,HW) int64.  loss_out: 3 floats [mean loss, number of counted pixels, number of targets outside [0,K) that
 * are not ignore_index].  F.cross_entropy raises on such targets; a kernel cannot, so they are excluded from the mean
 * and COUNTED -- the host side (medt_amd.ops.cross_entropy, TrainStep.check_targets) raises from the count.  All pixels
 * ignored -> 0/0 = NaN, as in torch.  partials: medt_ce_partials() floats. */
size_t medt_ce_partials(int N, int HW);
int medt_ce_fwd(const float* logits, const int64_t* target, float* partials, float* loss_out, int N, int K, int HW,
                int ignore_index, void* stream);
int medt_ce_bwd(const float* logits, const int64_t* target, const float* loss_out, const float* dloss, float* dlogits,
                int N, int K, int HW, int ignore_index, void* stream);

/* Segmentation loss = ce_scale * CE + dice_scale * Dice (either scale may be 0: that term is then left out).
 *   p = softmax over the K classes; a pixel is VALID when its target is not ignore_index and lies in [0, K).
 *   CE   = sum_valid w[t_i] (-log p_i,t_i) / sum_valid w[t_i]      F.cross_entropy(weight=w, reduction='mean'), what the
 *          reference's LogNLLLoss(weight=...) computes (metrics.py:17-20); class_weight NULL: w = 1 (medt_ce_fwd's value);
 *          a zero denominator gives NaN, as in torch.
 *   Dice = 1 - mean over images n and classes k of (2 I_nk + eps) / (P_nk + T_nk + eps), with I_nk = sum p_ik [t_i = k],
 *          P_nk = sum p_ik, T_nk = sum [t_i = k] over the valid pixels of image n ONLY (per image, not per batch: with equal
 *          shards the mean of the ranks' gradients is the gradient of the global batch).  Needs 2 <= K <= 8; the weighted
 *          cross entropy alone (dice_scale == 0) takes any K >= 1.  eps >= 0.
 * logits (N,K,HW) float, target (N,HW) int64, class_weight K floats or NULL.
 * out: medt_seg_loss_out_floats() floats = [loss, sum of counted weights (the pixel count when class_weight is NULL),
 * number of targets outside [0,K) that are not ignore_index (excluded and counted, as medt_ce_fwd does), CE, Dice] followed
 * by the 2*N*K per-(image, class) coefficients of dDice/dp the backward reads (written when dice_scale != 0).
 * partials: medt_seg_loss_workspace() floats.  fwd is two launches, bwd one (recomputes the softmax; dloss: one device float
 * or NULL = 1; writes all K channels of dlogits, exactly 0 at pixels that are not valid).  No float atomics: every sum has
 * a fixed order, so results are bit-identical from run to run.  bwd must be given the scales, eps and class_weight of fwd. */
size_t medt_seg_loss_workspace(int N, int K, int HW);
size_t medt_seg_loss_out_floats(int N, int K);
int medt_seg_loss_fwd(const float* logits, const int64_t* target, const float* class_weight, float* partials, float* out,
                      int N, int K, int HW, int ignore_index, float ce_scale, float dice_scale, float eps, void* stream);
int medt_seg_loss_bwd(const float* logits, const int64_t* target, const float* class_weight, const float* out,
                      const float* dloss, float* dlogits, int N, int K, int HW, int ignore_index, float ce_scale,
                      float dice_scale, float eps, void* stream);

/* torch.optim.Adam(lr, betas, eps, weight_decay) over one flat buffer (train.py:111-112,161).
 * state: 3 device floats [step, 1-b1^step, 1-b2^step], zero-initialised; advanced on the device so a captured
 * hipGraph replays the right bias correction.  g is multiplied by gscale first (1/world_size after all-reduce). */
int medt_adam_step(float* p, const float* g, float* m, float* v, float* state, size_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, float gscale, void* stream);

/* out = a * (y > 0) elementwise (ReLU backward by output sign). */
int medt_relu_mask(const float* a, const float* y, float* out, size_t n, void* stream);

/* Scoring without MATLAB (performancemetrics_monuseg.m:19-84, performancemetrics_glas.m): per-image confusion
 * counts of the prediction test.py writes (logits[:,1] >= threshold, test.py:131-137) against target > 0.
 * logits (N,K,HW) float, target (N,HW) int64, counts (N,4) int32 = {tp, fp, fn, tn}; the call zeroes counts itself. */
int medt_seg_counts(const float* logits, const int64_t* target, int32_t* counts, int N, int K, int HW, float threshold,
                    void* stream);

/* Sliding-window inference on an image larger than the network input (not in the reference, which resizes the dataset
 * offline; medt_amd/window.py).  The image is cut into T = ny*nx overlapping S x S windows, numbered row-major
 * (t = iy*nx + ix), window t with its top-left corner at (oy[iy], ox[ix]).  oy (ny) and ox (nx) are int32 DEVICE
 * arrays, so the launches do not depend on where the windows lie.  ny*nx*channels*S*S and channels*H*W must stay
 * below 2^31 (MEDT_EUNSUPPORTED above).
 *
 * gather: image (C,H,W) -> windows (T,C,S,S); source coordinates are clamped to the image, which is edge replication
 * where H < S or W < S.
 *
 * blend: window logits (T,K,S,S) -> blended (K,H,W) and / or mask (H,W) uint8 {0,255} = blended[1] >= threshold
 * (test.py:131-137's rule; needs K >= 2); either output may be NULL, not both.  Window pixel (i, j) weighs
 * w(i) w(j), w(i) = min(i + 1, S - i).  Every output pixel is computed by one work-item that visits the windows
 * covering it in ascending t and divides sum(w l) by sum(w) once: no atomics, bit-identical from run to run.  A pixel
 * that ONE window covers receives that window's value unchanged; a pixel that none covers (no plan of
 * medt_amd.window.plan_windows leaves one) receives 0.  16-byte stores when W % 4 == 0 and the outputs are aligned
 * (blended to 16 bytes, mask to 4), element stores otherwise. */
int medt_window_gather(const float* image, float* windows, const int32_t* oy, const int32_t* ox, int C, int H, int W, int S,
                       int ny, int nx, void* stream);
int medt_window_blend(const float* win_logits, float* blended, uint8_t* mask, const int32_t* oy, const int32_t* ox, int K,
                      int H, int W, int S, int ny, int nx, float threshold, void* stream);

/* Test-time augmentation at inference (not in the reference; medt_amd/tta.py): the network runs on flipped and transposed
 * copies of its input, each prediction is mapped back and the results are averaged.  A view is a 3-bit code v: bit 2
 * transpose, bit 1 flip rows, bit 0 flip columns, the transpose first -- in torch terms, for a (..., H, W) tensor,
 *   forward  F_v(a): t = a.transpose(-1, -2) if v & 4 else a;  F_v(a) = t.flip([-2 if v & 2] + [-1 if v & 1])
 *   inverse  B_v(l): m = l.flip(the same dims);                B_v(l) = m.transpose(-1, -2) if v & 4 else m
 * (0 identity, 1 left-right mirror, 2 up-down mirror, 3 rotation by 180 degrees, 4 transpose, 5 rot90(k=-1), 6 rot90(k=1),
 * 7 anti-transpose).  `views` is a bitmask, bit v set when code v takes part, V = popcount(views); the views are visited in
 * ascending code.  0 < views <= 0xFF; a view with bit 2 needs H == W (MEDT_EINVAL otherwise); N*V*channels*H*W must stay
 * below 2^31 (MEDT_EUNSUPPORTED above).
 *
 * expand: x (N,C,H,W) -> out (N*V,C,H,W), out[n*V + j] = F_vj(x[n]) with v_j the j-th set bit: a permutation, every element
 * a bit copy.  out must not be x.
 *
 * merge: view_logits (N*V,K,H,W) -> merged (N,K,H,W) = (B_v0(l_0) + B_v1(l_1) + ... + B_vV-1(l_V-1)) / (float)V: the
 * additions in that order by the one work-item that owns the output element, then one IEEE division (V = 1: the value passes
 * through unchanged) -- no atomics, no reassociation, bit-identical from run to run;  mask (N,H,W) uint8 {0,255} =
 * merged[:,1] >= threshold (test.py:131-137's rule);  votes (N,H,W) uint8 = the number of views whose own mapped-back
 * l_j[:,1] >= threshold (0 .. V).  Any of the three outputs may be NULL, not all; mask and votes need K >= 2; merged must not
 * be view_logits.
 *
 * The views without bit 2 are row copies; the views with bit 2 pass through a padded tile in LDS, so no view reads or writes
 * global memory at stride W.  16-byte accesses when W % 4 == 0 and the pointers are aligned (floats to 16 bytes, mask and
 * votes to 4), element accesses otherwise. */
int medt_tta_expand(const float* x, float* out, int N, int C, int H, int W, unsigned views, void* stream);
int medt_tta_merge(const float* view_logits, float* merged, uint8_t* mask, uint8_t* votes, int N, int K, int H, int W,
                   unsigned views, float threshold, void* stream);

/* Joint augmentation of a training batch on the device (medt_amd/augment.py; the reference's JointTransform2D.__call__,
 * utils.py:70-98, does it per item with torchvision on the host): random crop, horizontal flip, colour jitter (image only)
 * and a random affine map (image and mask), in that order.
 * image (N,H,W,C) uint8, C = 1 or 3, channels as decoded; mask (N,H,W) uint8 -> out_image (N,C,th,tw) float32 in [0,1],
 * out_mask (N,th,tw) int64.  params: a DEVICE table of N records of medt_augment_param_floats() floats, drawn on the host:
 *   [0] cy [1] cx  crop origin    [2] flip (!= 0)    [3] identity (!= 0: the affine step is skipped, no float round trip)
 *   [4..9] m00 m01 m02 m10 m11 m12   the INVERSE affine map, output pixel centre -> cropped image
 *   [10..13] operation of jitter slot k: 0 none, 1 brightness, 2 contrast, 3 saturation, 4 hue    [14..17] its factor
 *   [18] elastic (medt_augment_warp, below; medt_augment_apply ignores it)    [19] reserved, 0
 * Output pixel (i, j): fx = m00 (j+.5) + m01 (i+.5) + m02, fy = m10 (j+.5) + m11 (i+.5) + m12, sx = floor(fx), sy = floor(fy)
 * (PIL's Image.transform(AFFINE, NEAREST)).  Outside [0,tw) x [0,th) -- tested on the floats, so non-finite or huge
 * coordinates are outside -- the image receives 0.0 and the mask 0, neither jittered.  Flip: sx -> tw-1-sx.  Source pixel
 * (cy+sy, cx+sx), clamped to the input: no table makes a kernel read out of bounds.  v = u8 / 255 (IEEE division), then the
 * slots in order, torchvision's float path, g = 0.299 c0 + 0.587 c1 + 0.114 c2 over the channels as stored:
 *   brightness clamp(b v, 0, 1); saturation clamp(s v + (1-s) g, 0, 1); contrast clamp(c v + (1-c) mean_g, 0, 1);
 *   hue: RGB -> HSV, H = (H + h) mod 1, HSV -> RGB (hexcone).  C == 1: g = v, saturation and hue are the identity.
 * mean_g: the mean of g over the cropped th x tw image after the slots in front of the record's (one) contrast slot.
 *
 * medt_augment_stats computes the per-image sums of g into workspace (medt_augment_workspace() floats: partial sums, then
 * N means); fixed summation order, no atomics, the same bits on every run.  medt_augment_apply does everything else: one
 * launch; use_stats != 0 reads the sums (call stats first), use_stats == 0 takes mean_g = 0 -- for batches without a
 * contrast slot, whose workspace may be NULL.  A non-NULL workspace receives the N means used.  16-byte stores when
 * tw % 4 == 0 and both outputs are 16-byte aligned, element stores otherwise.  N*H*W*C and N*C*th*tw must stay below 2^31
 * (MEDT_EUNSUPPORTED above). */
size_t medt_augment_param_floats(void);
size_t medt_augment_workspace(int N, int th, int tw);
int medt_augment_stats(const uint8_t* image, const float* params, float* workspace, int N, int H, int W, int C, int th,
                       int tw, void* stream);
int medt_augment_apply(const uint8_t* image, const uint8_t* mask, const float* params, float* workspace, float* out_image,
                       int64_t* out_mask, int N, int H, int W, int C, int th, int tw, int use_stats, void* stream);

/* Elastic deformation inside the joint augmentation (U-Net's random displacement vectors on a coarse grid; not in the
 * reference): medt_augment_warp is medt_augment_apply with a cubic B-spline free-form deformation of the records whose slot
 *   [18] elastic (!= 0)      ([19] stays reserved, 0; a record keeps medt_augment_param_floats() == 20 floats)
 * is set.  field: a DEVICE table (N,2,G+3,G+3) float32, the control lattice of G x G cells per image in pixels, channel 0 =
 * dx, channel 1 = dy, 1 <= G <= 8.  Output pixel (i, j) of a th x tw crop whose record has the flag:
 *   tx = (j+.5) G / tw, cx = min(floor(tx), G-1), u = tx - cx;   ty, cy, v likewise from i and th
 *   B0 = (1-u)^3/6, B1 = (3u^3-6u^2+4)/6, B2 = (-3u^3+3u^2+3u+1)/6, B3 = u^3/6        (non-negative, sum 1)
 *   d = sum_a B_a(v) (sum_b B_b(u) field[.][cy+a][cx+b])      summed b ascending inside, a ascending outside
 *   p = (j+.5+dx, i+.5+dy);  f = M p with the record's inverse affine map, f = p under the identity flag
 *   inside: 0 <= fx < tw and 0 <= fy < th on the floats (NaN and huge coordinates are outside); outside, image 0, class 0
 *   mask: nearest, floor(f).  image: bilinear about the pixel centres, ux = fx-.5, x0 = floor(ux), wx = ux-x0, taps x0 and
 *   x0+1, likewise in y; tap indices are clamped to [0,tw-1] x [0,th-1] of the (flipped) crop, mirrored when flip, offset by
 *   the crop origin and clamped to the input.  Every tap is u8/255 and runs through the record's jitter slots BEFORE the
 *   blend (1-wy)((1-wx) t00 + wx t01) + wy((1-wx) t10 + wx t11); mean_g is medt_augment_stats' mean of the unwarped crop.
 * A record without the flag gets medt_augment_apply's nearest path and its bits, whatever the other records of the batch
 * hold; a set flag with an all-zero lattice and the identity flag gives those bits too (the weights are exactly 0 and 1).
 * Lattice indices are clamped to [0,G+2]: no table makes a read leave its buffer.  No atomics, the same bits on every run.
 * Refusals: those of medt_augment_apply, a NULL field, G outside 1..8 (MEDT_EINVAL). */
int medt_augment_warp(const uint8_t* image, const uint8_t* mask, const float* params, const float* field, int G, float* workspace,
                      float* out_image, int64_t* out_mask, int N, int H, int W, int C, int th, int tw, int use_stats, void* stream);

/* Exact squared Euclidean distance transform of binary masks on the device, in two passes -- the building block of the
 * surface-distance scores (metrics.surface_scores: Hausdorff distance, its 95th percentile, average symmetric surface
 * distance; not in the reference, whose users take them from SciPy / MedPy on the host).
 *   edt_sq(F)[y,x] = min over (y',x') in F of (y-y')^2 + (x-x')^2 = distance_transform_edt(~F)**2, exactly, as int32;
 *   every pixel of an image whose F is empty holds MEDT_EDT_NONE.
 * The foreground of a mask is mask != 0.  Its BORDER is the foreground pixels with at least one 4-neighbour outside the
 * foreground, pixels outside the image counting as outside (A & ~binary_erosion(A, cross, border_value=0), MedPy's
 * surface): a foreground pixel on the image edge is always border.
 *
 * medt_edt_cols: mask (N,H,W) uint8 -> g2 (N,H,W) int32, g2[y,x] = (y-y')^2 for the feature pixel (y',x) of column x nearest
 * to y, MEDT_EDT_NONE when the column has none.  border_mode == 0: the features are the foreground; != 0: its border,
 * derived from the mask on the fly (never stored).  One work-item per (image, column); g2 is scratch of the pass as well
 * (written by the downward sweep, read back and overwritten by the upward one), so it must not alias mask.
 * medt_edt_rows: g2 (N,H,W) int32 from medt_edt_cols -> d2 (N,H,W) int32, d2[y,x] = min over x' of (x-x')^2 + g2[y,x'],
 * MEDT_EDT_NONE when the image has no feature pixel.  select == NULL: every pixel.  select (N,H,W) uint8: only the border
 * pixels of select != 0 receive the value, every other pixel receives -1 (the distances from the surface of one mask to the
 * surface of another in one map).  One workgroup per (image, row), the row of g2 in LDS; d2 must not alias g2.
 * cols(mask, 0) + rows(select NULL) is edt_sq of the foreground; cols(b, 1) + rows(select a) the surface distances a -> b.
 *
 * Integers throughout, no atomics: exact, and bit-identical from run to run.  The sentinel never enters a sum.  16-byte
 * accesses when W % 4 == 0 and the pointers are aligned (g2, d2 to 16 bytes, mask to 4), element accesses otherwise.
 * 1 <= H, W <= MEDT_EDT_MAX_DIM and N*H*W below 2^31 (MEDT_EUNSUPPORTED beyond, checked on the host before any launch).
 * The caller owns all memory. */
#define MEDT_EDT_NONE    2147483647   /* INT32_MAX: no feature pixel in the image (d2) / in the column (g2) */
#define MEDT_EDT_MAX_DIM 4096
int medt_edt_cols(const uint8_t* mask, int32_t* g2, int N, int H, int W, int border_mode, void* stream);
int medt_edt_rows(const int32_t* g2, const uint8_t* select, int32_t* d2, int N, int H, int W, void* stream);

/* Boundary loss of the training step (Kervadec et al., "Boundary loss for highly unbalanced segmentation", MIDL 2019): the
 * signed distance map of the label map the step holds on the device, and the term built on it.
 *
 * medt_signed_edt: target (N,H,W) int64 class indices -> sd2 (N,H,W) int32, in two launches (columns, rows).  The foreground
 * F is {target == fg} (fg >= 0; a pixel equal to ignore_index is never in F); every other pixel -- ignored, out of range, any
 * other class -- is outside F.  Outside F sd2 = +d^2 to the nearest pixel of F (>= 1), inside F sd2 = -d^2 to the nearest pixel
 * outside F (<= -1); an image without a pixel of F holds 0 everywhere, and so does an image that is all F.  g2: N*H*W int32 of
 * scratch (the signed column map: > 0 outside F, < 0 inside, see elementwise.hip), must not alias sd2.  Exact: integers
 * throughout, no atomics, bit-identical from run to run.  Element accesses only: no alignment beyond the elements' own.
 * Limits as medt_edt_*: 1 <= H, W <= MEDT_EDT_MAX_DIM, N*H*W below 2^31 (MEDT_EUNSUPPORTED beyond, before any launch).
 *
 * medt_boundary_fwd / _bwd: logits (N,K,HW) float32, target (N,HW) int64, sd2 (N,HW) from medt_signed_edt; K >= 2, 0 <= fg < K.
 *   s = softmax(logits)[fg];  phi = sqrt(sd2) where sd2 > 0, -(sqrt(-sd2) - 1) where sd2 < 0, 0 where sd2 == 0 (computed on the
 *   fly, never stored);  B = mean over images n of ( sum over the valid pixels p of phi_n(p) s_n(p) / max(1, V_n) ), V_n the
 *   number of valid pixels of image n; a pixel is valid when its target is in [0, K) and is not ignore_index.
 * alpha: ONE float32 in device memory, read on the device when the kernels run (the finalize reads it and hands it on in
 * out[2], where the backward of the same step reads it) -- a captured step follows a schedule that refills it in place; no
 * launch argument depends on its value.  base: NULL, or one device float (the region loss, out[0] of
 * medt_seg_loss_fwd / loss_out[0] of medt_ce_fwd).
 *   out: medt_boundary_out_floats(N) floats = [base + alpha B (alpha B when base is NULL), B, alpha as read,
 *   1 / (N max(1, V_n)) for n < N];  partials: medt_boundary_workspace(N, HW) floats.  fwd is two launches (partial sums, one
 *   finalize in double), bwd one; every sum has a fixed order, no float atomics.
 *   bwd: dlogits[n,k,p] = dloss alpha phi / (N max(1, V_n)) s (delta(k,fg) - p_k) at the valid pixels (dloss: one device float,
 *   NULL = 1).  accumulate == 0 writes dlogits, zeros at the pixels that are not valid included; accumulate != 0 ADDS into the
 *   dlogits that medt_seg_loss_bwd / medt_ce_bwd has just written for the same logits and targets (which holds the zeros
 *   already): one gradient buffer for region + boundary term. */
int medt_signed_edt(const int64_t* target, int32_t* g2, int32_t* sd2, int N, int H, int W, int fg, int ignore_index, void* stream);
size_t medt_boundary_workspace(int N, int HW);
size_t medt_boundary_out_floats(int N);
int medt_boundary_fwd(const float* logits, const int64_t* target, const int32_t* sd2, const float* alpha, const float* base,
                      float* partials, float* out, int N, int K, int HW, int fg, int ignore_index, void* stream);
int medt_boundary_bwd(const float* logits, const int64_t* target, const int32_t* sd2, const float* out, const float* dloss,
                      float* dlogits, int N, int K, int HW, int fg, int ignore_index, int accumulate, void* stream);

/* Border weight of the training step for touching objects (Ronneberger et al., "U-Net", MICCAI 2015: w0 exp(-(d1 + d2)^2 /
 * (2 sigma^2)), d1 and d2 the distances to the nearest and the second-nearest object), as an additive term of the loss.
 *
 * medt_object_edt2: labels (N,H,W) int32 as medt_label_components writes them (0: no object, l > 0: object l; values <= 0 are
 * no object) -> d1sq, d2sq (N,H,W) int32, in two launches (columns, rows).  d1sq: the squared distance to the nearest pixel
 * with a label > 0 (0 inside an object).  d2sq: the squared distance to the nearest pixel with a label > 0 other than the label
 * that attains d1sq -- the second smallest of the per-object minimum distances; inside object l the distance to the nearest
 * other object.  MEDT_EDT_NONE where there is no such object: d1sq in an image without an object, d2sq in an image with fewer
 * than two.  Labels are not returned: under ties the nearest label is not unique, the two distances are.
 * scratch: 4 * N*H*W int32, four planes of N*H*W each: g1 | a | g2 | b -- per pixel the squared distance along its column to
 * the nearest labelled pixel of the column and that pixel's label, then the same for the nearest pixel of the column whose
 * label is not a (2^30 and label 0 where the column has none); must not alias d1sq or d2sq, which must differ.  Exact: integers
 * throughout, no atomics, no workgroup waits for another, bit-identical from run to run.  Element accesses only: no alignment
 * beyond the elements' own.  Limits as medt_edt_*: 1 <= H, W <= MEDT_EDT_MAX_DIM, N*H*W below 2^31 (MEDT_EUNSUPPORTED beyond,
 * before any launch).
 *
 * medt_border_fwd / _bwd: logits (N,K,HW) float32, target (N,HW) int64, d1sq / d2sq (N,HW) from medt_object_edt2 over the
 * components of F = {target == fg}; K >= 2, 0 <= fg < K, sigma > 0 and finite (MEDT_EINVAL otherwise).
 *   e = exp(-(sqrt(d1sq) + sqrt(d2sq))^2 / (2 sigma^2)) at the pixels whose target is not fg and whose d2sq is not
 *   MEDT_EDT_NONE, 0 elsewhere (computed on the fly, never stored);  nll = -log softmax(logits)[target];
 *   R = mean over images n of ( sum over the valid pixels p of e_n(p) nll_n(p) / max(1, V_n) ), valid and V_n as medt_boundary_fwd.
 * w0: ONE float32 in device memory, read on the device and handed on in out[2], as medt_boundary_fwd's alpha.  base: NULL, or
 * one device float (the region loss).
 *   out: medt_border_out_floats(N) floats = [base + w0 R (w0 R when base is NULL), R, w0 as read, 1 / (N max(1, V_n)) for n < N];
 *   partials: medt_border_workspace(N, HW) floats.  fwd is two launches (partial sums, one finalize in double), bwd one; every
 *   sum has a fixed order, no float atomics.
 *   bwd: dlogits[n,k,p] = dloss w0 e / (N max(1, V_n)) (p_k - delta(k, target)) at the valid pixels (dloss: one device float,
 *   NULL = 1).  accumulate == 0 writes dlogits, zeros where e is 0 included; accumulate != 0 ADDS into the dlogits that
 *   medt_seg_loss_bwd / medt_ce_bwd has just written for the same logits and targets. */
int medt_object_edt2(const int32_t* labels, int32_t* scratch, int32_t* d1sq, int32_t* d2sq, int N, int H, int W, void* stream);
size_t medt_border_workspace(int N, int HW);
size_t medt_border_out_floats(int N);
int medt_border_fwd(const float* logits, const int64_t* target, const int32_t* d1sq, const int32_t* d2sq, float sigma,
                    const float* w0, const float* base, float* partials, float* out, int N, int K, int HW, int fg,
                    int ignore_index, void* stream);
int medt_border_bwd(const float* logits, const int64_t* target, const int32_t* d1sq, const int32_t* d2sq, float sigma,
                    const float* out, const float* dloss, float* dlogits, int N, int K, int HW, int fg, int ignore_index,
                    int accumulate, void* stream);

/* Connected-component labelling of binary masks on the device, the per-component tables and a table-driven select pass -- the
 * building blocks of the object-level scores (metrics.object_scores: GlaS object F1 / Dice, AJI, PQ) and of the two mask
 * clean-ups "drop objects below an area" and "fill holes" (not in the reference, whose users call scipy.ndimage.label or
 * MATLAB's bwlabel on the host).
 *
 * medt_label_components: mask (N,H,W) uint8 -> labels (N,H,W) int32, count (N,) int32.  The labelled set is mask != 0, with
 * background != 0 it is mask == 0.  connectivity 4 (edge neighbours) or 8 (edge and corner neighbours).  labels is 0 outside
 * the labelled set and 1..count[n] inside, numbered per image in raster order of each component's first pixel: the array
 * scipy.ndimage.label(mask, structure) returns (structure None / ones((3,3))).  Components never cross from one image into the
 * next.  Scheme: union-find in LDS per MEDT_LABEL_TILE_H x MEDT_LABEL_TILE_W tile, atomicMin across the tile edges on a parent
 * map in the workspace, flatten, a fixed-order two-level prefix sum of the root flags, renumber; six launches, no workgroup
 * ever waits on another, every loop ends by its own progress.  A component's provisional label is its smallest pixel index
 * whatever order the merges land in and the ranks are integers summed in a fixed order, so the result is exact and
 * bit-identical from run to run.  workspace: medt_label_workspace_bytes(N,H,W) bytes (the parent map and the scan partials),
 * 16-byte aligned; a smaller workspace_bytes is MEDT_EWORKSPACE.  mask, labels and the workspace must not overlap.
 *
 * medt_label_tables: labels (N,H,W) int32 with values in [0, stride) -> area (N,stride) int32, area[n,l] = pixels of label l
 * (slot 0: the unlabelled rest), frame (N,stride) uint8, frame[n,l] = 1 when component l >= 1 has a pixel in row 0, row H-1,
 * column 0 or column W-1, else 0 (slot 0 stays 0).  The call clears both tables itself.  max_count: the largest count of the
 * batch as the caller knows it; stride <= max_count is MEDT_EINVAL.  Labels outside [0, stride) are not counted.
 *
 * medt_label_select: out[n,y,x] = 255 when keep[n, labels[n,y,x]] != 0 or (mask != NULL and mask[n,y,x] != 0), else 0; keep
 * (N,stride) uint8, out (N,H,W) uint8 (may be mask itself).  A keep table of area >= A over a foreground labelling is "drop
 * small objects"; a keep table of frame == 0 over a 4-connected background labelling, OR-ed with the mask, is "fill holes".
 *
 * Integer atomics only (order-independent).  16-byte accesses when W % 4 == 0 and the pointers are aligned (int32 maps to 16
 * bytes, uint8 maps to 4), element accesses otherwise.  1 <= H, W <= MEDT_LABEL_MAX_DIM and N*H*W below 2^31
 * (MEDT_EUNSUPPORTED beyond, checked on the host before any launch).  Null pointers, a connectivity other than 4 or 8 and
 * stride <= max_count are MEDT_EINVAL.  The caller owns all memory. */
#define MEDT_LABEL_TILE_H  16
#define MEDT_LABEL_TILE_W  64
#define MEDT_LABEL_MAX_DIM 4096
size_t medt_label_workspace_bytes(int N, int H, int W);      /* 0 for a geometry the calls refuse */
int medt_label_components(const uint8_t* mask, int32_t* labels, int32_t* count, void* workspace, size_t workspace_bytes, int N,
                          int H, int W, int connectivity, int background, void* stream);
int medt_label_tables(const int32_t* labels, int32_t* area, uint8_t* frame, int N, int H, int W, int stride, int max_count,
                      void* stream);
int medt_label_select(const int32_t* labels, const uint8_t* keep, const uint8_t* mask, uint8_t* out, int N, int H, int W,
                      int stride, void* stream);

/* Bounding boxes of the components and directed squared Hausdorff distances of pairs of them -- the building blocks of the
 * object-level Hausdorff distance of GlaS (metrics.object_hausdorff), added under version 11 as the calls above were.
 *
 * medt_label_boxes: labels (N,H,W) int32 with values in [0, stride) -> box (N,stride,4) int32, box[n,l] = (y0, x0, y1, x1),
 * inclusive, of label l >= 1; a label without a pixel holds (H, W, -1, -1), and so does slot 0, which only the call's own
 * initialisation writes.  Integer atomicMin / atomicMax, reduced per workgroup in LDS first: independent of any order.
 * Arguments, checks and limits as medt_label_tables; N*stride*4 must stay below 2^31 (MEDT_EUNSUPPORTED).
 *
 * medt_pair_hausdorff: la, lb (N,H,W) int32 label maps; jobs: a DEVICE table of n_jobs records of MEDT_PAIR_JOB_INTS int32,
 * one per (pair, direction):
 *    0 n          image                     1 query label           2 feature label
 *    3 swap       0: the query object is in la and the feature object in lb; 1: the other way round
 *    4..7         y0, y1, x0, x1 of the query object's bounding box (inclusive)
 *    8, 9         x0, x1 of the feature object's bounding box
 *   10, 11        first and last row the column pass sweeps: the union of the two objects' row ranges
 *   12 offset     of the job's g2 in scratch, in elements; the job owns (query rows) x (feature columns) of them
 *   13 slot       index into out that receives the job's result
 *   14, 15        blocks the jobs in front of this one take in the column launch (ceil(feature columns / 256) each) and in
 *                 the row launch (query rows each): non-decreasing prefix sums that start at 0; col_blocks / row_blocks are
 *                 their totals over all n_jobs jobs
 * out[slot] = max(out[slot], max over the pixels of the query object of the squared Euclidean distance to the nearest pixel
 * of the feature object), an exact int32; a feature label without a pixel inside its box gives MEDT_EDT_NONE.  clear_out != 0
 * zeroes the n_out int32 of out first (the first chunk of a job list that is issued in several calls so that the scratch
 * stays bounded).  Two launches: the column pass of the exact distance transform over the union of the two row ranges with
 * the feature test label == feature label, storing the query object's rows only, and the row pass, one workgroup per query
 * row, whose maxima leave as one integer atomicMax per workgroup.  A workgroup finds its job by binary search over column
 * 14 / 15.  A record that does not fit the images, scratch_elems or n_out is skipped on the device; which labels have a
 * pixel is the caller's knowledge (medt_label_boxes).  No workgroup waits on another, no float atomics: the same bits on
 * every run.  Null pointers, counts below 1 and a scratch of 0 elements are MEDT_EINVAL; geometry limits as above. */
#define MEDT_PAIR_JOB_INTS 16
int medt_label_boxes(const int32_t* labels, int32_t* box, int N, int H, int W, int stride, int max_count, void* stream);
int medt_pair_hausdorff(const int32_t* la, const int32_t* lb, const int32_t* jobs, int32_t* scratch, int32_t* out, int n_jobs,
                        int col_blocks, int row_blocks, size_t scratch_elems, int n_out, int clear_out, int N, int H, int W,
                        void* stream);

/* Splitting touching objects of a mask: peak markers of the distance transform and marker-controlled growth -- the building
 * blocks of medt_amd.ops.split_markers / grow_labels / split_objects and of test.py --split, added under version 11 as the calls
 * above were.  All integers; every result is independent of the order work-items and workgroups run in.
 *
 * medt_split_cmax: depth2 (N,H,W) int32 squared depths (medt_edt_* of the complement mask), comp (N,H,W) int32 component labels
 * with values in [0, stride) -> cmax (N,stride) int32, cmax[n,l] = the largest depth2 over component l >= 1 (slot 0 and a label
 * without a pixel hold 0).  The call clears the table itself.  Integer atomicMax, reduced per workgroup in LDS first.
 * stride <= max_count is MEDT_EINVAL.
 *
 * medt_split_markers: -> marker (N,H,W) uint8, 255 at the marker pixels, 0 elsewhere.  With M(p) the maximum of depth2 over the
 * (2 distance + 1)^2 window centred on p (pixels beyond the image count 0), a pixel with comp > 0 is a marker when
 * sqrt(M) - sqrt(depth2) <= tolerance -- evaluated exactly in int64: e = M - depth2 - tolerance^2, e <= 0 or
 * e^2 <= 4 tolerance^2 depth2 -- or when depth2 == cmax[n, comp].  One workgroup per MEDT_LABEL_TILE_H x MEDT_LABEL_TILE_W tile
 * with the tile and its halo in LDS, the maximum taken separably.  1 <= distance <= MEDT_SPLIT_MAX_DISTANCE and
 * 0 <= tolerance <= MEDT_SPLIT_MAX_TOLERANCE (MEDT_EINVAL otherwise).
 *
 * medt_grow_*: every pixel of mask != 0 takes the label of the seed at the smallest geodesic distance (steps at `connectivity`
 * through the mask), ties to the smallest label; a pixel no seed reaches takes 0.  The workspace
 * (medt_grow_workspace_bytes(N,H,W) bytes, a multiple of 16, 16-byte aligned) holds one packed 64-bit key (distance << 32 | label) per pixel and
 * two int32 flags per tile.
 *   medt_grow_init    seeds (N,H,W) int32 (> 0: a seed with that label; anything else: none), mask (N,H,W) uint8 -> the keys.
 *                     A seed outside the mask is ignored (the caller refuses it).
 *   medt_grow_passes  n_passes (1 .. MEDT_GROW_MAX_PASSES) relaxation passes, numbered first_pass, first_pass + 1, ...
 *                     (first_pass >= 0: 0 directly behind medt_grow_init, then the passes issued so far).  One workgroup per tile
 *                     relaxes its tile and a 1-pixel halo in LDS until a sweep changes nothing (at most (TILE_H + 2) (TILE_W + 2)
 *                     sweeps) and stores its own pixels only; a tile whose own and eight neighbours' keys did not change in the
 *                     pass before exits at once.  changed: n_passes int32 of device memory, changed[i] = 1 when pass i lowered a
 *                     key, else 0 (the call clears them first).  The growth is complete behind the first pass that changed
 *                     nothing; further passes leave everything as it is.  No workgroup waits on another.
 *   medt_grow_labels  -> labels (N,H,W) int32 and, when dist is not NULL, dist (N,H,W) int32: the number of steps to the seed,
 *                     -1 where no seed was reached or outside the mask.
 * Limits and checks as medt_label_*: 1 <= H, W <= MEDT_LABEL_MAX_DIM, N*H*W below 2^31 (MEDT_EUNSUPPORTED), null pointers and a
 * connectivity other than 4 or 8 MEDT_EINVAL, a smaller workspace_bytes MEDT_EWORKSPACE.  Element accesses only: no alignment
 * beyond the elements' own (the workspace apart). */
#define MEDT_SPLIT_MAX_DISTANCE  32
#define MEDT_SPLIT_MAX_TOLERANCE 8
#define MEDT_GROW_MAX_PASSES     64
int medt_split_cmax(const int32_t* depth2, const int32_t* comp, int32_t* cmax, int N, int H, int W, int stride, int max_count,
                    void* stream);
int medt_split_markers(const int32_t* depth2, const int32_t* comp, const int32_t* cmax, uint8_t* marker, int N, int H, int W,
                       int stride, int distance, int tolerance, void* stream);
size_t medt_grow_workspace_bytes(int N, int H, int W);       /* 0 for a geometry the calls refuse */
int medt_grow_init(const int32_t* seeds, const uint8_t* mask, void* workspace, size_t workspace_bytes, int N, int H, int W,
                   void* stream);
int medt_grow_passes(void* workspace, size_t workspace_bytes, int32_t* changed, int n_passes, int first_pass, int N, int H, int W,
                     int connectivity, void* stream);
int medt_grow_labels(const void* workspace, size_t workspace_bytes, int32_t* labels, int32_t* dist, int N, int H, int W,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MEDT_ABI_H */
