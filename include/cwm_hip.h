/*
 * cwm_hip.h -- C ABI of libcwm_hip.so: the MI355X (gfx950) VMAE predictor forward pass.
 *
 * This is the drop-in boundary for ONE path of neuroailab/CounterfactualWorldModels: everything
 * executed inside `self.predictor(x, mask)` at cwm/models/prediction.py:419-422, i.e.
 * `PretrainVisionTransformer.forward` (cwm/models/VideoMAE/vmae.py:539-560) with the primitives of
 * cwm/models/VideoMAE/utils.py (PatchEmbed :156-198, Attention :57-121, Mlp :37-54, Block :124-153),
 * plus the two thin wrapper steps either side of it: `_preprocess` / `imagenet_normalize`
 * (prediction.py:304-312, utils.py:15-21) and `pred_patches_to_video` (prediction.py:245-259).
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer named *_dev is a HIP device pointer owned by the
 *     caller; `stream` is a hipStream_t passed as void* (NULL = default stream)
 *   - functions return 0 on success, a negative code on failure, never throw; the message is
 *     available from cwm_last_error() (thread-local)
 *   - the library owns packed (bf16 hi/lo) weights and a workspace per model handle; no caller
 *     tensor is retained past a call
 *   - one process per GPU; a model handle lives on the device that was current at create time
 */
#ifndef CWM_HIP_H
#define CWM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The shared objects are built with -fvisibility=hidden: the entry points declared here (and, in libcwm_hip_dev.so, those of cwm_hip_dev.h)
 * are all they export. */
#define CWM_API __attribute__((visibility("default")))

#define CWM_OK 0
#define CWM_ERR_INVALID (-1) /* bad argument / precondition (mirrors the reference's shape errors) */
#define CWM_ERR_HIP (-2)     /* a HIP runtime call failed */
#define CWM_ERR_MASK (-3)    /* rows of `mask` do not all have n_vis visible tokens (vmae.py:167 reshape) */

/* Arithmetic mode of the GEMM / attention kernels. */
#define CWM_MODE_FAST 1   /* bf16 MFMA operands, fp32 accumulate                         */
#define CWM_MODE_PARITY 2 /* split-bf16 (hi+lo, 3 MFMAs per product): <=1e-3 vs fp32 CPU */

/* Mirrors the constructor arguments of PretrainVisionTransformer (vmae.py:261-297) that the
 * factories vmae.py:563-619 set; tubelet_size is 1 on this path. */
typedef struct cwm_config {
    int32_t img_h, img_w;   /* 224, 224 */
    int32_t patch;          /* 8 (base_8x8), 4 (large_4x4), 16 */
    int32_t num_frames;     /* 2 */
    int32_t in_chans;       /* 3 */
    int32_t enc_dim, enc_depth, enc_heads;
    int32_t dec_dim, dec_depth, dec_heads;
    int32_t mlp_ratio;      /* 4 */
    float ln_eps;           /* 1e-6 */
} cwm_config;

typedef struct cwm_model cwm_model;
struct cwm_kernel_stats;

/* replaces: model construction via the factories, vmae.py:597-619 */
CWM_API int cwm_model_create(const cwm_config* cfg, cwm_model** out);
CWM_API void cwm_model_destroy(cwm_model* m);

/* replaces: `model.load_state_dict(...)` (prediction.py:81-107).  `key` is the reference state-dict
 * name, `data` fp32 in PyTorch layout, on the host (on_device=0) or on the
 * model's device (on_device=1).  The tensor is copied and packed; the caller's buffer is not kept.
 * Re-loading a key overwrites it.  Unknown key or wrong shape -> CWM_ERR_INVALID. */
CWM_API int cwm_model_load_weight(cwm_model* m, const char* key, const float* data, int on_device, const int64_t* shape, int ndim);
/* Number of state-dict tensors not loaded yet (0 = ready); fills `buf` with the first missing key. */
CWM_API int cwm_model_missing_weights(cwm_model* m, char* buf, int buflen);

typedef struct cwm_forward_args {
    uint32_t struct_size;    /* sizeof(cwm_forward_args) of the header the CALLER was compiled against: fields added at the end by later versions
                              * are read only when the size covers them; a size below the first version's or above 4096 is CWM_ERR_INVALID (0.6 inserted this
                              * field FIRST: an ABI break against 0.5, whose callers must be rebuilt -- their x_dev pointer fails the upper bound) */
    /* frames: element (b, c, t, y, x) at x_dev[b*x_stride_b + c*x_stride_c + t*x_stride_t + y*W + x]
     * (so both [B,C,T,H,W] and the wrapper's [B,T,C,H,W] layouts are accepted without a copy) */
    const float* x_dev;
    int64_t x_stride_b, x_stride_c, x_stride_t;
    /* 1: x_dev is the raw [0,1] wrapper input and (x-mean)/std is fused into the frame load
     * (prediction.py:309-310); 0: x_dev is already what the model should see (vmae.py:539 seam) */
    int32_t normalize;
    const uint8_t* mask_dev; /* bool [B, Nt], 1 = masked (torch.bool storage) */
    int32_t batch;
    int32_t n_vis;           /* visible tokens per row; every row must have exactly this many */
    float* y_tokens_dev;     /* out [B, Nt - n_vis, in_chans*patch*patch] fp32, feature order (ph pw c); n_vis == Nt (nothing masked):
                              * [B, Nt, ...] = head(norm(x)) of every token, as vmae.py:250-253 (y_video_dev must then be NULL) */
    /* optional fused `pred_patches_to_video`: out [B, T, C, H, W]; visible patches are copied from
     * xraw_dev (same strides as x_dev; NULL = use x_dev, valid when normalize=1) */
    float* y_video_dev;
    const float* xraw_dev;
    int32_t mode;            /* CWM_MODE_FAST or CWM_MODE_PARITY */
    int32_t check;           /* 1: synchronise the stream and verify the mask precondition */
    void* stream;
} cwm_forward_args;

/* replaces: `self.predictor(self._preprocess(x), mask)` prediction.py:419-422
 *           = PretrainVisionTransformer.forward vmae.py:539-560,
 * and optionally `pred_patches_to_video` prediction.py:245-259. */
CWM_API int cwm_forward(cwm_model* m, const cwm_forward_args* args);

/* Batch lanes (no counterpart in the reference: an execution option of this library).  lanes = 2 (default): a call with
 * batch >= 2 whose halves keep >= 3000 encoder rows (ViT-B/8: batch >= 8; ViT-L/4: batch >= 2) runs as two half batches, the first on args->stream and the second on a stream owned by the model, forked and joined
 * with events inside cwm_forward, so the caller sees ordinary stream semantics; results are those of the single-lane call up to the
 * kernel choice per GEMM shape (fp32 re-association, < 1e-5).  lanes = 1: everything on args->stream. */
CWM_API int cwm_model_set_lanes(cwm_model* m, int lanes); /* 1 .. 4 (lane l owns batch rows [ceil(B l / n), ceil(B (l + 1) / n)); fewer lanes are used when a lane would keep < 3000 encoder rows); more than two lanes measured slower on MI355X */
/* Ragged batches.  0 (the default): every row of a cwm_forward has args->n_vis visible tokens, anything else is CWM_ERR_MASK -- the reference's failing
 * reshape `x[~mask].reshape(B, -1, C)` (vmae.py:167), which its wrappers avoid by un-masking random masked patches of the shorter rows until the counts agree
 * (RectangularizeMasks, prediction.py:421).  n_vis_min > 0: a row may have between n_vis_min and args->n_vis visible tokens (args->n_vis is the cap;
 * n_vis_min > args->n_vis is CWM_ERR_INVALID; with args->check a row outside the range is CWM_ERR_MASK, naming the range).  Every row is then predicted
 * from exactly the tokens its own mask leaves visible, as the reference predicts it alone at batch 1: the encoder runs args->n_vis rows per sample and
 * row b's attention reads its first Nv_b only, whatever the rows behind them hold.  y_tokens_dev is [B, Nt - n_vis_min, out]: the predictions of row b
 * are its LAST Nt - Nv_b rows, in ascending token order; the rows before them are unspecified.  y_video_dev as before.  Per handle because
 * cwm_forward_args is frozen.  Lanes, options and modes are unaffected. */
CWM_API int cwm_model_set_ragged(cwm_model* m, int n_vis_min);

/* Execution options of ONE model handle (no counterpart in the reference).  The defaults are the measured best and what production callers run;
 * the other values exist for same-box A/B measurements and for the bitwise cross-checks of the test suite.  Options are per handle: two models in
 * one process never see each other's settings (until round 4 these were process-wide switches).  Unknown key -> CWM_ERR_INVALID.  Results do not
 * depend on an option beyond fp32 re-association (< 1e-5).  (The timing-only ablation bits 1 / 2 / 8 of "gemm_debug" -- skip the epilogue's stores / the
 * epilogue / every LayerNorm: wrong outputs -- are REFUSED here with CWM_ERR_INVALID; the development library sets them through cwm_debug_set.)
 *   "gemm_tile"    0 automatic per shape, 1: 128x128 tiles, 4: 256x256 8-phase kernel, 6: 8-phase rounds + 128x128 remainder rows
 *   "gemm_direct"  1: bf16-output epilogues store 16 bytes per lane straight from the accumulators; 2: the fp32-output ones too; 0: LDS-staged
 *   "gemm_staged"  0: the per-fragment epilogue of round 1
 *   "gemm_debug"   bit mask of result-preserving A/B switches: 4 no 4-stage ring for small launches, 32 no split-K, 128 the one-lane tile choice also inside a two-lane call, 256 small launches
 *                  keep 128-row tiles, 512 bf16-output GEMMs with K < 512 stay on 128x128 tiles, 1024 no half-width column tiles in the 8-phase kernel,
 *                  2048 no half-height row tiles in the 8-phase kernel
 *   "attn_kernel"  0 automatic, 1: 4-wave kernel, 3: software-pipelined kernel
 *   "attn_remap"   0: plain workgroup order instead of one XCD per (batch, head) with the ragged query tiles last
 *   "attn_tail"    0: the regular schedule also for a ragged last query tile of <= 32 rows
 *   "attn_ksplit"  0: a nearly empty last round of workgroups runs its items whole instead of cutting them into key ranges
 *   "index_fused"       0: the index prologue (mask -> permutation, its inverse, the row check, the patch gather) as the four launches of rounds 1-4
 *   "prune_last_block"  0: the last decoder block runs over all tokens
 *   "mask_token_tables" 0: the first decoder block computes LN1 and Q / K / V of the mask-token rows in every call instead of copying them from a per-position
 *                       table built once per weight set and mode (plain predictor, rectangular batches with masked tokens; outputs bit-identical)
 *   "min_lane_rows"     encoder rows per half batch from which a forward splits into two lanes (0: the default, 3000 / 12000 for the IMU model)
 *   "conj_attn"         0: the fp32 VALU cross / context attention kernels of the IMU-conditioned model instead of the MFMA ones
 *   "conj_ctx_stream"   0: the IMU-conditioned model's context stream on the lane's own stream instead of a side stream */
CWM_API int cwm_model_set_option(cwm_model* m, const char* key, int value);

/* ---- IMU-conditioned conjoined padded predictor (BASELINE configs[4]) ------------------------------
 * replaces: ConjoinedPaddedVisionTransformer.forward for the `imu400_base_4x4patch_2frames_1tube` family
 * (cwm/models/VideoMAE/conjoined_vmae.py:889-1011, 852-887; factory :1230-1243), i.e. two token streams
 * (RGB + IMU) with null-token padding (:49-165), ImuEncoder tokenisation (:1013-1147) and
 * CrossAttentionTransformerBlock / BidirectionalCrossAttention (cwm/models/transformer.py:253-378, 442-583). */
typedef struct cwm_conj_config {
    cwm_config main;            /* RGB stream (patch 4, 768/12/12 - 384/6/4 for the shipped factory) */
    int32_t main_max_pad;       /* max_padding_tokens of the RGB stream (64) */
    int32_t ctx_in_chans, ctx_seq_len, ctx_tubelet;   /* 6, 400, 16 */
    int32_t ctx_enc_dim, ctx_dec_dim, ctx_enc_heads, ctx_dec_heads; /* 384, 192, 12, 6 */
    int32_t ctx_max_pad;        /* 25 */
    int32_t n_enc_cross, enc_cross[16]; /* cross block BEFORE these encoder layers (0,3,6,9) */
    int32_t n_dec_cross, dec_cross[16]; /* cross block AFTER these decoder layers (0,1,2,3) */
    int32_t cross_heads, cross_mlp_ratio; /* 4, 2 */
} cwm_conj_config;

typedef struct cwm_conj_model cwm_conj_model;
CWM_API int cwm_conj_create(const cwm_conj_config* cfg, cwm_conj_model** out);
CWM_API void cwm_conj_destroy(cwm_conj_model* m);
CWM_API int cwm_conj_load_weight(cwm_conj_model* m, const char* key, const float* data, int on_device, const int64_t* shape, int ndim);
CWM_API int cwm_conj_missing_weights(cwm_conj_model* m, char* buf, int buflen);

/* ---- conjoined variants (0.8) ---------------------------------------------------------------------
 * The unpadded `ConjoinedPretrainVisionTransformer` (conjoined_vmae.py:212-887) of the flow -> IMU head-motion predictor
 * `imu400_8x8patch_2frames_1tube_flowbackrgb01` (:1218-1228) runs on the same engine.  cwm_conj_config has no size field, so
 * the variant is a struct of its own; cwm_conj_create(cfg) is cwm_conj_create_ex(cfg, NULL, out) with the padded defaults.
 *   padded = 0: no null-token padding (main_max_pad and ctx_max_pad must be 0), no `null_token_*` weights, and every row of
 *     a call has the same visible count in each stream (the reference's `x[~mask].reshape(B, -1, C)`, vmae.py:155-167);
 *     other masks are CWM_ERR_INVALID.
 *   ctx_dummy_token = 1: the ImuEncoder's `concat_dummy_token` (conjoined_vmae.py:1013-1147): the learned weight
 *     `context_stream.encoder.dummy_token` [1, ctx_in_chans, ctx_tubelet, 1, 1] is appended to the IMU as sample block
 *     ctx_seq_len / ctx_tubelet, always visible (`_concat_excess_tokens` :595-609), with that position row of both tables.
 *   main_input = CWM_CONJ_INPUT_FLOWBACK_RGB01: the main stream's 7 channels are `FlowBackRGB01` (preprocessor.py:208-277, 356):
 *     [forward flow / (W/2, H/2), backward flow / (W/2, H/2), frame 1], gathered in-kernel from the flow_* arguments of
 *     cwm_conj_forward_args and x_dev (config: main.in_chans = 7, main.num_frames = 1).
 * Two variants are accepted: {padded = 1, ctx_dummy_token = 0, CWM_CONJ_INPUT_FRAMES} (the default) and {padded = 0,
 * ctx_dummy_token = 1, CWM_CONJ_INPUT_FLOWBACK_RGB01}; any other combination is CWM_ERR_INVALID. */
#define CWM_CONJ_INPUT_FRAMES 0
#define CWM_CONJ_INPUT_FLOWBACK_RGB01 1
typedef struct cwm_conj_variant {
    uint32_t struct_size;        /* sizeof(cwm_conj_variant) as the caller knows it; fields beyond it take their defaults */
    int32_t padded;              /* 1 (ConjoinedPaddedVisionTransformer) or 0 (ConjoinedPretrainVisionTransformer) */
    int32_t ctx_dummy_token;     /* 0 or 1 */
    int32_t main_input;          /* CWM_CONJ_INPUT_* */
} cwm_conj_variant;
CWM_API int cwm_conj_create_ex(const cwm_conj_config* cfg, const cwm_conj_variant* variant, cwm_conj_model** out);

typedef struct cwm_conj_forward_args {
    uint32_t struct_size;        /* sizeof(cwm_conj_forward_args) as the caller knows it (see cwm_forward_args): y_ctx_tokens_dev, added in 0.5, is read only
                                  * when the size covers it */
    const float* x_dev;          /* frames, strides as in cwm_forward_args */
    int64_t x_stride_b, x_stride_c, x_stride_t;
    int32_t normalize;
    const uint8_t* mask_dev;     /* bool [B, Nt]; rows MAY have different visible counts (null-token padding) */
    int32_t batch;
    int32_t n_vis_max;           /* max over rows of the visible count (max - min must be <= main_max_pad) */
    const float* ctx_dev;        /* IMU [B, ctx_in_chans, ctx_seq_len] contiguous fp32 */
    const uint8_t* ctx_mask_dev; /* bool [B, ctx_seq_len / ctx_tubelet] */
    int32_t n_vis_ctx_max;
    float* y_tokens_dev;         /* out [B, Nt + main_max_pad - n_vis_max, in_chans*patch*patch]; rows at masked pad slots are 0 */
    int32_t mode;
    int32_t check;
    void* stream;
    /* optional (NULL: not computed): the context stream's predictions, out [B, ctx tokens + ctx_max_pad - n_vis_ctx_max, ctx_in_chans*ctx_tubelet],
     * rows at masked pad slots are 0 -- `forward(..., output_context=True)` returns it, alone or in a tuple with y_tokens
     * (conjoined_vmae.py:852-887, 990-1011) */
    float* y_ctx_tokens_dev;
    /* CWM_CONJ_INPUT_FLOWBACK_RGB01 only (added in 0.8, read only when struct_size covers them): the forward and backward flow of
     * frames 0 -> 1, each fp32 [B, 2, H, W] in pixels (x, y), element (b, c, y, x) at b*stride_b + c*stride_c + y*W + x, 16-byte
     * aligned with strides that are multiples of 4.  x_dev then points at frame 1 ([B, 3, H, W] with x_stride_b / x_stride_c;
     * normalize as above).  For this input y_tokens_dev may be NULL: the main head is skipped, the main decoder still runs. */
    const float* flow_fwd_dev;
    int64_t flow_fwd_stride_b, flow_fwd_stride_c;
    const float* flow_bwd_dev;
    int64_t flow_bwd_stride_b, flow_bwd_stride_c;
} cwm_conj_forward_args;

/* replaces: `self.predictor(self._preprocess(x), mask, x_context=..., mask_context=...)` (prediction.py:419-422) */
CWM_API int cwm_conj_forward(cwm_conj_model* m, const cwm_conj_forward_args* args);
CWM_API int cwm_conj_set_lanes(cwm_conj_model* m, int lanes); /* 1 or 2 (anything else: CWM_ERR_INVALID) -- as cwm_model_set_lanes (here the halves must keep >= 12000 encoder rows: batch >= 8); the halves keep the call's n_vis_max / n_vis_ctx_max */
CWM_API int cwm_conj_set_option(cwm_conj_model* m, const char* key, int value); /* as cwm_model_set_option */
CWM_API int cwm_conj_timing_enable(cwm_conj_model* m, int kclass, int enable);
CWM_API int cwm_conj_timing_collect(cwm_conj_model* m, int kclass, struct cwm_kernel_stats* out);

/* ---- timing hooks (bench.py roofline): HIP events around every launch of one kernel class ------ */
#define CWM_KCLASS_GEMM 0        /* every GEMM launch: 2*M*N*K with M the rows the launch computes (a pruned block: B * kept rows) and K rounded up to 64 (the
                                  * operand is zero-padded to whole 64-element K tiles, which the hardware executes: K = 48 and 96, the patch-4 and IMU embeds, book 64 and 128) */
#define CWM_KCLASS_ATTENTION 1   /* 4 * n_q * N * 64 per (batch, head): n_q query rows against N keys -- n_q = N, except the pruned last decoder block ("prune_last_block"),
                                  * whose launch computes the Nm rows the head reads.  A ragged handle (cwm_model_set_ragged) is booked by launch extent: every class takes
                                  * the cap args->n_vis as the rows per sample, and attention the full N although row b reads its first Nv_b keys only (the counts live
                                  * on the device) */
#define CWM_KCLASS_GEMM_WIDE 2   /* the GEMM launches that ran the 256x256 8-phase kernel (wide N with at least half a round of tiles: qkv, fc1, whole rounds of fc2) */
#define CWM_KCLASS_GEMM_NARROW 3 /* ... the 128x128 kernels (proj, narrow N, head, patch embed, mixed-tiling remainders); both enabled / collected with class 0 */
/* HBM-bound edge kernels (SURVEY.md 8d "reported separately as achieved GB/s"): for these classes `total_flops` holds the
 * algorithmic BYTES of the launches (each input element read once, each output element written once), not FLOPs */
#define CWM_KCLASS_LAYERNORM 4    /* rows * D * (4 read + 2 * planes written) */
#define CWM_KCLASS_PATCH_GATHER 5 /* visible tokens * C*P*P * (4 read + 2 * planes written); the fused index prologue ("index_fused", one launch) adds B * Nt * (1 mask byte
                                   * read + 4 permutation written + 4 inverse permutation written when y_video_dev is set); with "index_fused" = 0 only the gather launch
                                   * of the four is booked */
#define CWM_KCLASS_FILL_MASK 6    /* the mask-token fill: B * Nm * Dd * 4 written (the positional rows come from L2; a ragged handle: Nm = Nt - n_vis_min, the rows its launch
                                   * covers; no launch when Nm = 0) -- and, with "mask_token_tables", the copy of decoder block 0's mask-token Q / K / V rows from the
                                   * table: one more launch of B * (Nt - n_vis) * 3 * Dd * 2 * planes written (the table's rows come from L2) */
#define CWM_KCLASS_UNEMBED 7      /* B * T*C*H*W * (4 read + 4 written) */
/* IMU-conditioned model only (cwm_conj_timing_*): FLOPs again */
#define CWM_KCLASS_CROSS_ATTN 8   /* BidirectionalCrossAttention, both directions: 2 * (4 * N * M * hd) per head */
#define CWM_KCLASS_SMALL_ATTN 9   /* the context stream's self-attention (25..50 tokens) */
#define CWM_KCLASS_COUNT 10
typedef struct cwm_kernel_stats {
    int64_t launches;
    double total_ms;    /* sum of launch durations (HIP events on the launch stream) */
    double total_flops; /* algorithmic FLOPs (2*M*N*K with K rounded up to 64; attention 4*n_q*N*hd per head) of those launches; BYTES for classes 4-7 */
} cwm_kernel_stats;
CWM_API int cwm_timing_enable(cwm_model* m, int kclass, int enable);
/* Synchronises the recorded events, accumulates, and resets the event pool. */
CWM_API int cwm_timing_collect(cwm_model* m, int kclass, cwm_kernel_stats* out);

/* ---- stand-alone kernel entry points (kernel-level parity tests; same kernels the model uses) -- */
/* fp32 -> bf16 hi (and lo if lo_dev != NULL) */
CWM_API int cwm_split_bf16(const float* x_dev, int64_t n, void* hi_dev, void* lo_dev, void* stream);
/* C[M,N] (fp32, ldc=N) = A[M,K] * W[N,K]^T + bias (+ resid), all fp32 device inputs; the library
 * splits/pads the operands exactly as the model path does.  replaces: F.linear (VideoMAE/utils.py:48-53) */
CWM_API int cwm_linear(const float* a_dev, const float* w_dev, const float* bias_dev, const float* resid_dev, float* c_dev,
               int M, int N, int K, int gelu, int mode, void* stream);
/* O[B,N,H*64] = softmax(q k^T) v per head from a packed qkv activation [B,N,3*H*64] (fp32 device),
 * q scaled by 64^-0.5 after bias as in VideoMAE/utils.py:94-113. */
CWM_API int cwm_attention(const float* qkv_dev, float* o_dev, int B, int N, int H, int mode, void* stream);
/* The same with a key count per batch row: row b attends to keys [0, key_len_dev[b]) of its N rows (N stays the row stride), and O rows
 * [0, key_len_dev[b]) of row b are written -- the others keep what o_dev held.  What rows b's q, k and v hold at and past its count never reaches a
 * written row, NaN and Inf included (those keys are not staged; a partly valid key tile re-reads the row's last valid key).  This is the kernel a
 * predictor needs for rows with different numbers of visible tokens: the reference's gather `x[~mask].reshape(B, -1, C)` (vmae.py:167) takes one
 * count for the whole batch, which is why its wrapper first un-masks random masked patches until the counts agree (RectangularizeMasks,
 * prediction.py:421).  With every count = N the result is bit-identical to cwm_attention under options "attn_tail" = 0, "attn_ksplit" = 0: ragged
 * launches run the regular schedule.  A count outside [1, N] is checked on the device: CWM_ERR_INVALID after the call's synchronisation, and
 * o_dev is not written at all. */
CWM_API int cwm_attention_ragged(const float* qkv_dev, const int32_t* key_len_dev, float* o_dev, int B, int N, int H, int mode, void* stream);
/* y = LayerNorm(x) (fp32 in/out, eps, affine).  replaces nn.LayerNorm at VideoMAE/utils.py:148-149 */
CWM_API int cwm_layernorm(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* y_dev, int rows, int D,
                  float eps, void* stream);
/* perm[B,Nt] = [visible ascending | masked ascending]; returns CWM_ERR_MASK if a row's visible
 * count != n_vis (synchronises).  replaces the boolean gathers vmae.py:167,555-556 */
CWM_API int cwm_mask_to_perm(const uint8_t* mask_dev, int B, int Nt, int n_vis, int32_t* perm_dev, void* stream);
/* replaces pred_patches_to_video (prediction.py:245-259); x is [B,T,C,H,W] contiguous raw frames */
CWM_API int cwm_unembed(const float* y_tokens_dev, const float* x_dev, const uint8_t* mask_dev, int B, int T, int C, int H, int W,
                int P, int n_vis, float* out_dev, void* stream);

typedef struct cwm_patch_error_args {
    uint32_t struct_size;          /* sizeof(cwm_patch_error_args); anything else: CWM_ERR_INVALID naming struct_size */
    const float* y_tokens_dev;     /* [B, Nt - n_vis, C*P*P] predicted tokens, feature order (ph pw c), as cwm_forward writes them; may be NULL when n_vis == Nt */
    /* frames: element (b, t, c, y, x) at x_dev[b*x_stride_b + t*x_stride_t + c*x_stride_c + y*W + x]; a batch stride of 0 shares one movie among the rows */
    const float* x_dev;
    int64_t x_stride_b, x_stride_t, x_stride_c;
    const float* target_dev;       /* the frames the prediction is compared with, with their own strides; NULL = x_dev */
    int64_t target_stride_b, target_stride_t, target_stride_c;
    const uint8_t* mask_dev;       /* bool [B, Nt], 1 = masked: the mask the tokens were predicted for */
    const float* region_dev;       /* [B, T, H/P, W/P] fp32 weights of the mean; NULL = ones */
    int32_t batch, T, C, H, W, P;  /* C <= 8; P 4, 8 or 16; H and W multiples of P */
    int32_t n_vis;                 /* visible tokens per row of mask_dev (y_tokens_dev has Nt - n_vis rows per sample) */
    int32_t frame;                 /* the predicted frame that is compared with EVERY target frame, or -1: frame t with target frame t */
    float* map_dev;                /* out [B, T, H/P, W/P] or NULL */
    float* mean_dev;               /* out [B] or NULL */
    float* scratch_dev;            /* [B, T, H/P, W/P] floats, needed only when map_dev is NULL and mean_dev is not */
    void* stream;
} cwm_patch_error_args;

/* Per-patch prediction error without the predicted video.
 * replaces: `_get_error` prediction.py:324-329 (MSELoss summed over the channels) of `predict` against the target, and the avg_pool3d over each patch,
 *           the region weighting and the mean of `get_error_on_target_region` prediction.py:553-574:
 *   map[b][t][i][j] = (1 / P^2) sum_{pixels of patch (i,j)} sum_c (pred_f - target_t)^2,  pred_f = frame f of pred_patches_to_video(y, x, mask): y at the masked
 *                     patches of frame f, x at its visible ones; f = frame, or t when frame = -1
 *   mean[b]         = sum(map * region) / max(sum(region), 1)
 * Asynchronous on `stream`: nothing is allocated and the host is not synchronised.  The row of y_tokens_dev that belongs to a masked token is its rank among
 * the row's masked tokens, counted on the device and clamped into [0, Nt - n_vis): no mask content makes the call read outside its buffers.  All sums have a
 * fixed order (no atomics): two calls on the same inputs give the same bits. */
CWM_API int cwm_patch_error(const cwm_patch_error_args* args);

typedef struct cwm_token_response_args {
    uint32_t struct_size;            /* sizeof(cwm_token_response_args); anything else: CWM_ERR_INVALID naming struct_size */
    /* read: y_tokens_dev, mask_dev, batch, T, C, H, W, P, n_vis, frame (0 .. T-1), map_dev ([B, H/P, W/P] or NULL), scratch_dev, stream; the frame, target,
     * region and mean fields are ignored, and so is base.struct_size */
    cwm_patch_error_args base;
    const float* y_ref_dev;          /* [B or 1, Nt - n_vis, C*P*P]: the prediction the tokens are compared against, same layout and same mask */
    int64_t y_ref_stride_b;          /* elements between its rows' token blocks; 0 shares one reference prediction among all rows */
    float* pixel_map_dev;            /* out [B, H, W] or NULL */
    int32_t* peak_index_dev;         /* out [B] or NULL: Y*W + X of the peak */
    float* stats_dev;                /* out [B, 4] or NULL: peak, mass, centroid_y, centroid_x */
} cwm_token_response_args;

/* Where two predictions of the same prompt geometry differ, without either predicted video: the response of a perturbation (the reference's marker
 * counterfactuals, `AddMarkers` cwm/models/perturbation.py:356-476: "where does this point go") read from the predicted tokens of the perturbed rows and of
 * the clean one.
 * replaces: `predict` prediction.py:406-454 of both prompts, their squared difference summed over the channels, and its argmax / sum / centroid in torch.
 *   With f = base.frame, n = (H/P)(W/P), pixel (Y, X) of frame f in patch (i, j), token tau = f n + i (W/P) + j:
 *   r[b][Y][X] = sum_c (y[b][row][k] - y_ref[b][row][k])^2, c = 0 .. C-1 in that order from 0.f; row = the rank of tau among the masked tokens of row b,
 *                clamped into [0, Nt - n_vis); k = (ph P + pw) C + c;  r = 0 where tau is visible (both predictions copy the same input pixel there)
 *   base.map_dev   the mean of r over each patch, summed in the order cwm_patch_error sums
 *   peak_index     the first maximum of r in linear order over ALL pixels of the frame (torch.argmax); a NaN is the maximum, the first NaN wins
 *   stats          peak = r at that pixel; mass = sum r; centroid = sum r (Y, X) / mass, and the peak position (as floats) when mass == 0
 * Asynchronous on base.stream: nothing is allocated and the host is not synchronised.  All sums have a fixed order (no atomics): two calls on the same
 * inputs give the same bits.  base.scratch_dev, [B, H/P, 8] floats of per-workgroup partials, is required whenever peak_index_dev or stats_dev is set.
 * Limits as cwm_patch_error: P 4, 8 or 16, C <= 8, W/P <= 256.  Argument errors: CWM_ERR_INVALID with a message, before anything is launched. */
CWM_API int cwm_token_response(const cwm_token_response_args* args);

typedef struct cwm_unmask_step_args {
    uint32_t struct_size;            /* sizeof(cwm_unmask_step_args); anything else: CWM_ERR_INVALID naming struct_size */
    /* num_reveal > 0: every field as cwm_patch_error reads it (map_dev or scratch_dev is required: the selection reads the map from it); base.struct_size is
     * ignored.  num_reveal == 0: only mask_dev, batch, T, H, W, P and the stream are read */
    cwm_patch_error_args base;
    int32_t frame;                   /* 0 .. T-1: the frame of the mask whose cells are measured and revealed */
    int32_t num_reveal;              /* k, 0 .. 64 cells revealed per row; 0: dist_dev and frontier_dev only */
    int32_t mode;                    /* 0 top: key = err; 1 race: key = max(err, 0) / e (a NaN err stays NaN) */
    int32_t self_mask;               /* dist_dev: non-zero gives the visible cells the grid's maximum (patch_distance_transform's self_mask) */
    const float* threshold_dev;      /* [1] on the device: frontier = masked and d <= threshold; a negative value (or NULL) = every masked cell */
    const float* e_dev;              /* [B, n] positive draws of the race (torch.empty(...).exponential_()); race mode only */
    uint8_t* mask_out_dev;           /* out [B, Nt] or NULL: base.mask_dev with the picks cleared; must not overlap base.mask_dev */
    int32_t* picks_dev;              /* out [B, k] or NULL: token indices in pick order; -1 once the frame of a row has no masked cell left */
    float* dist_dev;                 /* out [B, n] or NULL */
    uint8_t* frontier_dev;           /* out [B, n] uint8 or NULL */
} cwm_unmask_step_args;

/* One step of unmasking that grows outward from what is visible, guided by where the prediction is still wrong, without a host read-back.
 * replaces: `patch_distance_transform` cwm/models/masking.py:32-56 and `patches_adjacent_to_visible` masking.py:58-71 (the integer-radius branch), as
 *           `get_nearby_patches` prediction.py:345-351 uses them, on device masks; the selection is what `EnergySampleUnmask` (perturbation.py:589-640, which
 *           does not run in the reference) was meant to do.
 *   With f = frame, gh = H/P, gw = W/P, n = gh gw, sy = (gh-1)/2, sx = (gw-1)/2 (integer divisions) and cell = i gw + j:
 *   d[b][cell]        = min over the visible cells v of frame f of row b of max(|i - vi| / sy, |j - vj| / sx) in fp32, bit-equal to the reference; 0 everywhere when
 *                       the frame has no visible cell; with self_mask the visible cells hold the maximum of d over the grid
 *   frontier[b][cell] = cell is masked and (threshold < 0 or d <= threshold).  The host computes the threshold as the reference does:
 *                       float32(radius * (1 / ((min(gh, gw) - 1) / 2)))
 *   err[b][cell]      = map[b][f][cell] of cwm_patch_error on `base` (launched first: base.map_dev and base.mean_dev hold what that call writes, bit for bit), times
 *                       base.region_dev[b][f][cell] when a region is given
 *   The k cells revealed in row b are the first k masked cells of frame f in the order: frontier cells before the other masked cells; the higher key first, a NaN
 *   above every number (torch.sort) and -0 equal to +0; the lower index first.  picks[b][r] = f n + cell of the r-th; a row with fewer than k masked cells
 *   in the frame leaves its surplus picks at -1 and clears nothing for them.
 * Asynchronous on base.stream: nothing is allocated, the host is not synchronised, no atomics, fixed order -- two calls on the same inputs give the same bits.
 * One workgroup per row holds the frame's state in LDS.  No mask content makes the call read or write outside its buffers.
 * Limits: gh, gw >= 3 (the reference divides by sy and sx), n <= 4096, k <= 64, and with k > 0 the limits of cwm_patch_error.  Argument errors: CWM_ERR_INVALID with
 * a message, before anything is launched. */
CWM_API int cwm_unmask_step(const cwm_unmask_step_args* args);

typedef struct cwm_segment_step_args {
    uint32_t struct_size;            /* sizeof(cwm_segment_step_args); anything else: CWM_ERR_INVALID naming struct_size */
    /* read: batch, T (must be 2), H, W, P and stream.  Every other field of base is ignored, base.struct_size included */
    cwm_patch_error_args base;
    const float* flows_dev;          /* f[b][c][y][x][s] at flows_dev[b st[0] + c st[1] + y st[2] + x st[3] + s st[4]] (elements), st = flow_strides, as
                                      * cwm_flow_filter_stats takes them; NULL (with S = 0) is the init step */
    int64_t flow_strides[5];
    int32_t C, S;                    /* C = 2 (0: x-displacement, 1: y-displacement); 1 <= S <= 255 */
    const int32_t* seeds_dev;        /* [B, 2] (y, x) pixels, clamped into the image on the device */
    const float* dirs_dev;           /* [S, 2] (dy, dx), shared by all rows, or NULL: no direction test */
    float min_seed_mag, abs_thresh, rel_thresh, vote_frac, cos_min, inside_frac;  /* vote_frac must not be a NaN */
    int32_t k_active, k_passive;     /* 0 .. 64 each; k_active = 0: no selection (k_passive is ignored) */
    int32_t ring_radius;             /* >= 1, in cells */
    const float* keys_dev;           /* [B, 2, n]: [b][0] ranks the active picks, [b][1] the passive ones; NULL = every key 0 (index order) */
    float* seed_ref_dev;             /* out [B, S], required with flows (the vote pass reads it): ref_s, a NaN where sample s is not valid */
    uint8_t* votes_dev;              /* out [B, H, W], required with flows (the component pass reads it); optional in the init step, which writes zeros */
    uint8_t* segment_dev;            /* out [B, H, W] 0 / 1, or NULL */
    float* cover_dev;                /* out [B, H/P, W/P] or NULL */
    int32_t* stats_dev;              /* out [B, 4] or NULL: n_valid, area, n_candidates, seed_hit */
    int32_t* picks_dev;              /* out [B, k_active + k_passive] or NULL: n + cell (tokens of frame 1), active picks first; -1: the slot found no cell */
    uint8_t* active_out_dev;         /* out [B, 2 n] or NULL: frame 0 all 0, frame 1 all 1 with the active picks cleared (0 = active) */
    uint8_t* passive_out_dev;        /* out [B, 2 n] or NULL: the same with the passive picks cleared (0 = passive and visible) */
} cwm_segment_step_args;

/* One step of Spelke-object segmentation: from the S counterfactual flows of a seed point to the connected region that moves with it, and to the patches the
 * next round of counterfactuals moves and pins -- on the device, without a read-back.  No counterpart in the reference, whose README names the use ("asking which
 * points would also move along with a selected point is a way of segmenting a scene into independently movable Spelke objects") and lists the algorithm as coming.
 *   With gh = H/P, gw = W/P, n = gh gw, Nt = 2 n, per row b, in this order:
 *   1 magnitude   m_s(p) = sqrtf(u u + v v) of sample s at pixel p (u: channel 0, v: channel 1): the flow-sample filter's form
 *   2 seed cell   (y, x) = seeds[b] clamped into [0, H-1] x [0, W-1];  c0 = (y/P) gw + x/P
 *   3 seed ref    ref_s = (sum of m_s over the P P pixels of cell c0 in row-major order, from 0.f, plain fp32 adds by one thread) / (float)(P P)
 *   4 valid       sample s is valid iff ref_s >= min_seed_mag (a NaN is not); n_valid = their number
 *   5 votes       pixel p votes in a valid sample s iff m_s(p) >= fmaxf(abs_thresh, rel_thresh * ref_s) (fmaxf: a NaN operand is ignored) and, with dirs,
 *                 u dx + v dy >= (cos_min * m_s(p)) * sqrtf(dx dx + dy dy); a NaN compares false.  votes[p] = the number of samples p votes in
 *   6 candidates  need = max(1, (int)ceilf(vote_frac * (float)n_valid));  candidate[p] = n_valid > 0 && votes[p] >= need
 *   7 segment     the union of the 4-connected components of `candidate` that hold a candidate pixel of cell c0; empty when the cell has none (seed_hit 0 / 1)
 *   8 cover       cover[cell] = (#segment pixels of the cell) / (float)(P P): exact
 *   9 stats       (n_valid, area = #segment pixels, n_candidates, seed_hit)
 *  10 selection   only when k_active > 0.  inside[cell] = cover >= inside_frac; touched = cover > 0; ring[cell] = !touched and some touched cell lies within
 *                 Chebyshev distance ring_radius.  Order: the rule of cwm_unmask_step -- the higher key first, a NaN above every number, -0 equal to +0, the
 *                 lower index first.  Active picks: c0 first and always, then the first k_active - 1 inside cells other than c0.  Passive picks: the first
 *                 k_passive ring cells.  active_out / passive_out / picks as described at their fields (the convention of cwm_prompt_table_expand).
 *  11 init step   flows_dev == NULL: no flows, an empty segment -- active_out holds c0 alone, passive_out nothing, votes / segment / cover / stats are zeros.
 * Three passes: the seed references (one thread per (b, s)); the votes (many workgroups stream the flows once; coalesced for the sample-outermost view of the
 * flow model's output and for the packed [B,2,H,W,S] layout, any other strides take a strided form); then one workgroup per row holds the candidate and reached
 * bitmaps in LDS as bit rows, fills components by whole-word sweeps (bounded by H W + 1 sweeps whatever the input), counts coverage and selects.
 * Asynchronous on base.stream: nothing is allocated, the host is not synchronised, no atomics, fixed order -- two calls on the same inputs give the same bits.
 * No content of a device table (seeds, flows, keys, NaN or inf among them) makes the call read or write outside its buffers.
 * Limits: C = 2; P 4, 8 or 16; H % P == 0, W % P == 0; H W <= 2^18 and H ceil(W / 32) <= 8192 (the bit rows); 1 <= S <= 255, or S = 0 with NULL flows; n <= 4096;
 * k_active, k_passive <= 64; ring_radius >= 1.  Argument errors: CWM_ERR_INVALID with a message that names the field, before anything is launched. */
CWM_API int cwm_segment_step(const cwm_segment_step_args* args);

typedef struct cwm_segment_merge_args {
    uint32_t struct_size;            /* sizeof(cwm_segment_merge_args); anything else: CWM_ERR_INVALID naming struct_size */
    /* read: batch, T (must be 2), H, W, P and the stream.  Every other field of base is ignored, base.struct_size included */
    cwm_patch_error_args base;
    int32_t K;                       /* 1 .. 64 candidate segments per row */
    const uint8_t* segs_dev;         /* candidate (b, k) is the contiguous H W bytes at segs_dev + b seg_strides[0] + k seg_strides[1]; nonzero = in */
    int64_t seg_strides[2];          /* elements (bytes), not negative: a slice [:, :k] of a [B, Kmax, H, W] buffer, or a [B K, H, W] result, is read in place */
    const float* scores_dev;         /* [B, K] or NULL: every score 0, which gives index order */
    int32_t min_area, max_area;      /* >= 0 pixels; max_area == 0 means H W */
    float iou_thresh, contain_thresh;
    int32_t absorb;                  /* 0 / 1: paint the absorbed candidates' pixels with their absorber's label */
    void* work_dev;                  /* 16-byte aligned; its contents on entry do not matter */
    uint64_t work_bytes;             /* >= cwm_segment_merge_work_bytes(batch, K, H, W) */
    uint8_t* labels_dev;             /* out [B, H, W] or NULL: 0 = no object, m = 1 .. num_labels */
    int32_t* owner_dev;              /* out [B, K] or NULL */
    int32_t* area_dev;               /* out [B, K] or NULL */
    int32_t* label_area_dev;         /* out [B, K] or NULL */
    int32_t* inter_dev;              /* out [B, K, K] or NULL */
    float* cover_dev;                /* out [B, H/P, W/P] or NULL */
    int32_t* stats_dev;              /* out [B, 4] or NULL: n_valid, num_labels, labelled pixels, n_absorbed */
} cwm_segment_merge_args;

/* Scene segmentation, the merge: K candidate segments per row -- what K seeds of cwm_segment_step found -- become one label map on the device, without a
 * read-back.  No counterpart in the reference, whose README names the use and lists the algorithm as coming.
 *   With gh = H/P, gw = W/P, per row b, in this order:
 *   1 area        area[k] = the number of nonzero pixels of candidate k
 *   2 valid       valid[k] = area[k] >= max(1, min_area) && area[k] <= max_area (0: H W).  An empty segment is never valid
 *   3 inter       inter[j][k] = the number of pixels in both j and k, all K K pairs, valid or not: symmetric, the diagonal is area
 *   4 order       the valid candidates in the order of cwm_unmask_step: the higher score first, a NaN above every number, -0 equal to +0, the lower index first
 *   5 suppression walk the order.  k is ABSORBED by the first already-kept j, in the order they were kept, for which
 *                     (float)inter[j][k] > iou_thresh * (float)(area[j] + area[k] - inter[j][k])   or
 *                     (float)inter[j][k] > contain_thresh * (float)min(area[j], area[k])
 *                 (one fp32 multiply and one compare each; a NaN threshold compares false); otherwise k is KEPT and gets the next label 1, 2, ....  Always the
 *                 candidates' own segments, never a union: the result does not chain.  owner[k] = k's label if kept, its absorber's if absorbed, 0 if not valid
 *   6 paint       the painting set of label m: its keeper's segment, plus the segments of the candidates it absorbed when `absorb` is set.  labels[p] = the
 *                 lowest m whose painting set holds p, 0 where there is none: overlaps between kept objects go to the higher-ranked one.  A label's region
 *                 may end up disconnected
 *   7 label_area  label_area[m - 1] = the number of pixels with label m, m = 1 .. K; 0 for labels that do not exist
 *   8 cover       cover[cell] = (#pixels of the cell with a label > 0) / (float)(P P): exact
 *   9 stats       (n_valid, num_labels, #labelled pixels, n_absorbed = n_valid - num_labels)
 * Five kernels behind one memset: the bytes are packed into bit words once, pair intersections are popcounts of ANDed words, one wave per row ranks and walks the
 * candidates, one workgroup per patch row paints.  Sums across workgroups are INTEGER atomics into tables the call zeroes itself on the stream: the same bits
 * in any order, two calls on the same inputs give the same bits, and the contents of work_dev on entry do not matter.
 * Asynchronous on base.stream: nothing is allocated and the host is not synchronised.  No content of a device table (NaN and inf scores among them) makes the
 * call read or write outside its buffers.
 * Limits: 1 <= K <= 64; P 4, 8 or 16; H % P == 0, W % P == 0; H W <= 2^18; (H/P)(W/P) <= 4096; batch <= 65535; min_area, max_area >= 0; absorb 0 or 1; work_dev
 * non-NULL and 16-byte aligned, work_bytes large enough.  Argument errors: CWM_ERR_INVALID with a message that names the field, before anything is launched.
 * cwm_segment_merge_work_bytes returns 0 for sizes the call would refuse. */
CWM_API int cwm_segment_merge(const cwm_segment_merge_args* args);
CWM_API size_t cwm_segment_merge_work_bytes(int B, int K, int H, int W);

typedef struct cwm_seed_select_args {
    uint32_t struct_size;            /* sizeof(cwm_seed_select_args); anything else: CWM_ERR_INVALID naming struct_size */
    /* read: batch, H, W, P and the stream.  Every other field of base is ignored, base.struct_size and base.T included */
    cwm_patch_error_args base;
    const float* map_dev;            /* the score map: pixels (cells == 0) or one value per cell (cells == 1) */
    int32_t cells;                   /* 0: map [B, H, W], pixel (b, y, x) at map_dev[b map_strides[0] + y map_strides[1] + x] (elements), so a channel of a
                                      * [B, C, H, W] tensor or a padded buffer is read in place; 1: map [B, H/P, W/P] contiguous, map_strides ignored */
    int64_t map_strides[2];          /* batch and row stride, not negative; the row stride is at least W */
    const uint8_t* free_dev;         /* [B, n] or NULL: a cell with 0 is no candidate; NULL = every cell is free */
    const float* e_dev;              /* [B, n] or NULL: non-NULL selects race mode, key = max(v, 0) / e */
    const int32_t* prior_dev;        /* [B, n_prior] or NULL (with n_prior 0): cells of earlier seeds; entries outside 0 .. n-1 (-1 by convention) are ignored */
    int32_t n_prior;                 /* 0 .. 64 */
    int32_t K;                       /* 1 .. 64 seeds per row */
    int32_t radius;                  /* 0 .. 64, Chebyshev, in cells: the spacing of the picks, the window of the peak test, the reach of the prior cells */
    int32_t peaks_only;              /* 0 / 1: only peaks (step 4) are candidates */
    float abs_thresh, rel_thresh;    /* abs_thresh: not a NaN, -inf disables it; rel_thresh: finite, <= 0 disables it */
    void* work_dev;                  /* pixels form only: 16-byte aligned; its contents on entry do not matter.  Not read in the cells form (may be NULL) */
    uint64_t work_bytes;             /* pixels form: >= cwm_seed_select_work_bytes(batch, H, W, P) */
    int32_t* seeds_dev;              /* out [B, K, 2] (y, x) or NULL: (-1, -1) for a dead slot */
    int32_t* cells_dev;              /* out [B, K] or NULL: -1 for a dead slot */
    float* values_dev;               /* out [B, K] or NULL: v of the picked cell, 0 for a dead slot */
    float* pooled_dev;               /* out [B, n] or NULL: v */
    uint8_t* peaks_dev;              /* out [B, n] or NULL: step 4, written whether peaks_only is set or not */
    int32_t* stats_dev;              /* out [B, 4] or NULL: free non-NaN cells, candidates, picks made, 0 */
} cwm_seed_select_args;

/* Seed selection: a score map -- a keypoint map, a movability map, the patch distribution of a scene loop -- becomes at most K well-spaced seed pixels per row on
 * the device, without a read-back: the strongest peaks first, or an exponential race in proportion to the map, both under non-maximum suppression and both
 * excluding the neighbourhood of earlier seeds.  No counterpart in the reference, whose `sample_patches_from_energy` and `sample_and_visualize_keypoints` only
 * ever sample and never space.
 *   With gh = H/P, gw = W/P, n = gh gw, cell c = i gw + j, r = radius, per row b, in this order:
 *   1 pool        pixels form: v[c] = the maximum over the P P pixels of cell c, NaN pixels ignored; the seed pixel of c is the first pixel in row-major order
 *                 that attains it (-0 and +0 are equal; v is that pixel's own value); a cell whose pixels are all NaN has v = NaN (and no seed pixel).
 *                 cells form: v[c] = map[c]; the seed pixel is the cell's centre (i P + P/2, j P + P/2)
 *   2 row maximum m = the maximum of v over the non-NaN cells of the row, free or not; a row without one has no candidates
 *   3 threshold   t = abs_thresh if rel_thresh <= 0, else max(abs_thresh, rel_thresh * m): one fp32 multiply
 *   4 peak        c is a peak iff v[c] is not a NaN and its word (v in the order of cwm_unmask_step, the lower index higher) is the maximum of the words of the
 *                 non-NaN cells within Chebyshev distance r, free or not, the window clipped at the border: a plateau has one peak per window, its lowest index
 *   5 candidates  c is free, v[c] is not a NaN, v[c] >= t, c is a peak (with peaks_only), and no prior cell lies within Chebyshev distance r of c (r = 0: the
 *                 prior cells themselves are excluded)
 *   6 key         v[c]; in race mode max(v[c], 0) / e[b][c], one correctly rounded division (a NaN key ranks above every number, as in cwm_unmask_step)
 *   7 selection   K rounds: the candidate that is first in the order of cwm_unmask_step (the higher key first, -0 equal to +0, the lower index first) is picked,
 *                 then every candidate within Chebyshev distance r of it, itself included, is removed.  A round without a candidate is a dead slot
 * Two kernels: the pool pass streams the map once (workgroups over (band of cells, cell row, b), 16-byte loads where the addresses allow them, a fixed-order
 * reduction) into work_dev; one workgroup per row then holds v and the rank words in LDS, tests peaks by a separable windowed maximum and runs the rounds.
 * The cells form skips the pool pass.  Asynchronous on base.stream: nothing is allocated, the host is not synchronised, no atomics, fixed order -- two calls on
 * the same inputs give the same bits, and the contents of work_dev on entry do not matter.  No content of a device table (NaN, inf, prior entries out of range)
 * makes the call read or write outside its buffers.
 * Limits: P 4, 8 or 16; H % P == 0, W % P == 0; H W <= 2^18; n <= 4096; batch <= 65535; 1 <= K <= 64; 0 <= radius <= 64; 0 <= n_prior <= 64; at least one
 * output.  Argument errors: CWM_ERR_INVALID with a message that names the field, before anything is launched.  cwm_seed_select_work_bytes returns 0 for sizes
 * the call would refuse. */
CWM_API int cwm_seed_select(const cwm_seed_select_args* args);
CWM_API size_t cwm_seed_select_work_bytes(int B, int H, int W, int P);

typedef struct cwm_segment_track_args {
    uint32_t struct_size;            /* sizeof(cwm_segment_track_args); anything else: CWM_ERR_INVALID naming struct_size */
    /* read: batch, H, W and the stream.  Every other field of base is ignored, base.struct_size, base.T and base.P included */
    cwm_patch_error_args base;
    const uint8_t* prev_dev;         /* row b: the H W contiguous bytes at prev_dev + b prev_stride, the previous frame's track map (0: none, 1 .. 64: a slot); a
                                      * frame [:, t] of a [B, T, H, W] buffer is read in place.  NULL: no previous frame */
    int64_t prev_stride;             /* bytes, not negative */
    const uint8_t* cur_dev;          /* the same with cur_stride: this frame's label map as cwm_segment_merge writes it.  NULL: no segmentation for this frame */
    int64_t cur_stride;
    const float* flow_dev;           /* pixel (b, c, y, x) at flow_dev[b flow_strides[0] + c flow_strides[1] + y W + x] (elements); c = 0 horizontal, 1 vertical, in
                                      * pixels, from THIS frame to the PREVIOUS one, on this frame's grid.  NULL: zero motion */
    int64_t flow_strides[2];         /* not negative */
    const int32_t* track_id_in_dev;  /* [B, 64]: 0 = the slot is free, otherwise its persistent id.  The three state inputs are given together or all NULL (an */
    const int32_t* age_in_dev;       /* [B, 64]                                                       empty state with next_id 1) */
    const int32_t* next_id_in_dev;   /* [B] */
    float iou_thresh;
    int32_t min_inter, min_area;     /* >= 0 pixels */
    int32_t max_age;                 /* >= 0 frames a track may coast */
    int32_t carry;                   /* 0 / 1: unlinked tracks with warped pixels coast */
    void* work_dev;                  /* 16-byte aligned; its contents on entry do not matter */
    uint64_t work_bytes;             /* >= cwm_segment_track_work_bytes(batch, H, W) */
    uint8_t* out_dev;                /* out or NULL: row b is the H W bytes at out_dev + b out_stride (a frame of a [B, T, H, W] buffer is written in place) */
    int64_t out_stride;              /* bytes, at least H W (read with out_dev only) */
    int32_t* track_id_out_dev;       /* out [B, 64] or NULL.  The state outputs are separate buffers: in and out may NOT alias */
    int32_t* age_out_dev;            /* out [B, 64] or NULL */
    int32_t* next_id_out_dev;        /* out [B] or NULL */
    int32_t* area_dev;               /* out [B, 64] or NULL */
    int32_t* bbox_dev;               /* out [B, 64, 4] or NULL: (y0, x0, y1, x1) inclusive, (0, 0, -1, -1) for an empty slot */
    int64_t* moments_dev;            /* out [B, 64, 2] int64 or NULL: (sum y, sum x) */
    int32_t* slot_of_cur_dev;        /* out [B, 64] or NULL: entry c-1 = the slot of label c, or 0 */
    int32_t* linked_cur_dev;         /* out [B, 64] or NULL: entry p-1 = the label linked to slot p, or 0 */
    int32_t* table_dev;              /* out [B, 65, 65] or NULL: n[c][p] */
    uint8_t* warped_dev;             /* out [B, H, W] or NULL: w */
    int32_t* stats_dev;              /* out [B, 8] or NULL: linked, born, coasting, ended, dropped labels, live slots out, labelled pixels, 0 */
} cwm_segment_track_args;

/* Scene segments through a movie: the previous frame's track map is warped onto this frame by the backward flow, its overlaps with this frame's label map are
 * counted, tracks and labels are linked one to one, unlinked tracks coast or end, unlinked labels are born into free slots, and the result is painted -- on the
 * device, one call per frame, without a read-back.  No counterpart in the reference.  There are 64 track SLOTS, numbered 1 .. 64.  Per row b, in this order:
 *   0 inputs   as described at their fields.  A prev or cur byte above 64 counts as 0; a prev slot whose track_id_in is 0 counts as 0.  A slot is LIVE iff its
 *              track_id_in is not 0
 *   1 warp     fx = (float)x + u, fy = (float)y + v (one fp32 add each); rx = rintf(fx), ry = rintf(fy) (half to even); the source is inside iff
 *              rx >= 0 && rx <= W-1 && ry >= 0 && ry <= H-1 in fp32 (a NaN or an inf is outside); w(y,x) = prev[(int)ry][(int)rx] inside, else 0
 *   2 table    n[c][p] = the number of pixels with cur == c and w == p, c and p in 0 .. 64; area_cur[c] = sum_p n[c][p]; area_w[p] = sum_c n[c][p]
 *   3 link     (c >= 1, p >= 1) is a candidate iff n[c][p] >= max(1, min_inter) and (float)n[c][p] > iou_thresh * (float)(area_cur[c] + area_w[p] - n[c][p])
 *              (one fp32 multiply and one compare; a NaN threshold compares false).  Up to 64 rounds in the order of cwm_unmask_step: key (float)n[c][p], the
 *              higher first, ties to the lower index (c-1) 64 + (p-1).  The winner is linked, slot_of[c] = p; every candidate sharing its c or its p is removed
 *   4 coast    a live slot p that no pair linked COASTS iff carry && area_w[p] > 0 && age_in[p] + 1 <= max_age: it keeps its id, age_out = age_in + 1.
 *              Otherwise it ENDS: track_id_out = 0, age_out = 0.  A linked slot keeps its id and gets age 0
 *   5 births   the unlinked labels c >= 1 with area_cur[c] >= max(1, min_area), in ascending c, each take the lowest slot that was free on entry or ended in
 *              step 4 and that no earlier birth took; id = the running next_id, counting up from next_id_in (32-bit wrap-around), age 0.  Without a free slot
 *              the label is dropped, slot_of[c] = 0; unlinked labels below min_area are dropped too.  next_id_out = next_id_in + the number of births
 *   6 paint    out(y,x) = slot_of[cur(y,x)] where that is > 0; elsewhere w(y,x) if that slot coasts; elsewhere 0
 *   7 read-outs area, bbox, moments per slot s over the pixels of out with value s
 *   8 tables   slot_of_cur, linked_cur, table, warped as described at their fields
 *   9 stats    linked, born, coasting, ended, dropped labels (area_cur >= 1 and no slot), live slots out (track_id_out != 0), labelled pixels of out, 0
 * Four kernels behind one memset: a count pass (16 pixels per thread, 16-byte loads where the addresses allow them, the warped map kept in work_dev), one
 * workgroup per row that links, coasts and gives birth, a paint pass, one wave per row that writes the read-outs.  Sums across workgroups are INTEGER atomics
 * into tables the call zeroes itself on the stream: the same bits in any order, two calls on the same inputs give the same bits, and the contents of work_dev on
 * entry do not matter.  Asynchronous on base.stream: nothing is allocated and the host is not synchronised.  No content of a device buffer (label and slot
 * bytes above 64, NaN, inf and huge flows, garbage state) makes the call read or write outside its buffers.  The state buffers in and out may not alias, and
 * out_dev may not overlap prev_dev or cur_dev.
 * Limits: 1 <= batch <= 65535; H and W positive multiples of 4, H W <= 2^18; max_age, min_inter, min_area >= 0; carry 0 or 1; strides not negative; the three
 * state inputs together or not at all; at least one output; work_dev non-NULL and 16-byte aligned, work_bytes large enough.  Argument errors: CWM_ERR_INVALID
 * with a message that names the field, before anything is launched.  cwm_segment_track_work_bytes returns 0 for sizes the call would refuse. */
CWM_API int cwm_segment_track(const cwm_segment_track_args* args);
CWM_API size_t cwm_segment_track_work_bytes(int B, int H, int W);

typedef struct cwm_flow_consistency_args {
    uint32_t struct_size;            /* sizeof(cwm_flow_consistency_args); anything else: CWM_ERR_INVALID naming struct_size */
    /* read: batch, H, W, P (for cell_dev only) and the stream.  Every other field of base is ignored, base.struct_size and base.T included */
    cwm_patch_error_args base;
    const float* a_dev;              /* the flow being checked: pixel (b, c, y, x) at a_dev[b a_strides[0] + c a_strides[1] + y W + x] (elements), as flow_dev of
                                      * cwm_segment_track; c = 0 horizontal, 1 vertical, in pixels, on its own grid A, pointing to the other frame.  A
                                      * [B, T-1, 2, H, W] tensor viewed as B (T-1) rows and one pair of a larger tensor are read in place */
    int64_t a_strides[2];            /* not negative */
    const float* o_dev;              /* the other flow, the same with o_strides: on the other frame's grid, pointing back */
    int64_t o_strides[2];
    float alpha, beta;               /* finite, >= 0: thr = alpha mag + beta */
    int32_t both;                    /* 0 / 1: also direction d = 1, the roles of a and o exchanged; D = 1 + both */
    uint8_t* code_dev;               /* out [D, B, H, W] or NULL: 0 consistent, 1 inconsistent, 2 the target lies outside */
    float* res_dev;                  /* out [D, B, H, W] or NULL: the squared residual, +inf for code 2 and for a NaN */
    float* masked_dev;               /* out [D, B, 2, H, W] or NULL: the checked flow where code == 0, the quiet NaN 0x7fc00000 elsewhere */
    float* cell_dev;                 /* out [D, B, H/P, W/P] or NULL: the fraction of a cell's pixels with code != 0 */
    int32_t* stats_dev;              /* out [D, B, 4] or NULL: pixels with code 0, code 1, code 2, then 0 */
} cwm_flow_consistency_args;

/* Forward-backward flow consistency: an occlusion code, the residual and an occlusion-masked flow per pixel, in one call on the device, without a read-back.
 * No counterpart in the reference.  The masked flow feeds cwm_segment_track as it is: that call treats a NaN flow as "falls outside", so a disoccluded pixel
 * warps nothing in.  Every arithmetic step below is ONE correctly rounded fp32 operation in the stated order; nothing is contracted into a fused
 * multiply-add.  Per row b and pixel (y, x) of grid A, with (u, v) = a[:, y, x]:
 *   1 target   fx = (float)x + u, fy = (float)y + v; the pixel is INSIDE iff fx >= 0 && fx <= W-1 && fy >= 0 && fy <= H-1, tested in fp32 before anything is
 *              converted to an integer (NaN, inf and huge flows are outside).  Outside: code = 2, res = +inf, and nothing of o is read
 *   2 sample   x0f = floorf(fx), wx = fx - x0f, ix0 = (int)x0f, ix1 = min(ix0 + 1, W-1); the same in y.  Per channel c of o, with o00 = o[c][iy0][ix0],
 *              o01 = o[c][iy0][ix1], o10 = o[c][iy1][ix0], o11 = o[c][iy1][ix1]: top = o00 + wx (o01 - o00), bot = o10 + wx (o11 - o10),
 *              s_c = top + wy (bot - top).  A target exactly on the last column or row is inside, and the clamp keeps its taps in the plane
 *   3 residual ru = u + s_0, rv = v + s_1, res = ru ru + rv rv; mag = (u u + v v) + (s_0 s_0 + s_1 s_1); thr = alpha mag + beta
 *   4 decision code = 0 iff res <= thr (equality is consistent), otherwise 1: a NaN anywhere (a NaN or inf sample of o) compares false and gives 1.
 *              res_out = res if res == res, else +inf
 *   5 masked   m[:, y, x] = a[:, y, x] where code == 0; elsewhere both channels are the quiet NaN 0x7fc00000
 *   6 cells    (with cell_dev) cell[i][j] = (the number of the cell's P P pixels with code != 0) / (float)(P P): an integer count and one exact division
 *   7 stats    per row the numbers of pixels with code 0, code 1 and code 2, then 0: integer sums
 * both = 1 also produces everything with the roles of a and o exchanged, as direction d = 1 of the outputs' leading dimension.
 * One kernel (4 pixels per thread, 16 x 64 pixels per workgroup, 16-byte loads and stores where the addresses allow them; the cell counts stay inside a
 * workgroup), behind one memset of stats_dev, into which the workgroups add with INTEGER atomics: the same bits in any order, two calls on the same inputs give
 * the same bits.  There is no workspace.  Asynchronous on base.stream: nothing is allocated and the host is not synchronised.  No content of a device buffer
 * (NaN, inf and huge flows) makes the call read or write outside its buffers.  The outputs may not overlap the inputs.
 * Limits: 1 <= batch <= 65535; H and W positive multiples of 4, H W <= 2^18; a_dev and o_dev non-NULL, strides not negative; alpha and beta finite and >= 0;
 * both 0 or 1; at least one output; cell_dev needs P 4, 8 or 16 and H and W multiples of P.  Argument errors: CWM_ERR_INVALID with a message that names the
 * field, before anything is launched or written. */
CWM_API int cwm_flow_consistency(const cwm_flow_consistency_args* args);

typedef struct cwm_object_motion_args {
    uint32_t struct_size;            /* sizeof(cwm_object_motion_args); anything else: CWM_ERR_INVALID naming struct_size */
    /* read: batch (B), T, H, W and the stream.  Every other field of base is ignored, base.struct_size and base.P included.  Rows r = b T + t, R = B T */
    cwm_patch_error_args base;
    const uint8_t* labels_dev;       /* the slot map of frame A: row (b, t) is the H W contiguous bytes at labels_dev + b labels_strides[0] + t labels_strides[1]
                                      * (0: none, 1 .. 64: a slot; a byte above 64 reads as 0).  A [B, T, H, W] buffer, a [:, :-1] or [:, 1:] slice of one and a
                                      * plain [B, H, W] (T = 1) are read in place */
    int64_t labels_strides[2];       /* batch and frame stride in elements, not negative */
    const float* flow_dev;           /* the flow from A to the other frame on A's grid: pixel (b, t, c, y, x) at flow_dev[b flow_strides[0] + t flow_strides[1] +
                                      * c flow_strides[2] + y W + x]; c = 0 horizontal, 1 vertical, in pixels */
    int64_t flow_strides[3];         /* batch, frame and channel stride in elements, not negative */
    const uint8_t* code_dev;         /* NULL, or what cwm_flow_consistency wrote for this flow, addressed as labels_dev with code_strides */
    int64_t code_strides[2];
    const uint8_t* other_dev;        /* NULL, or the slot map of the other frame, addressed as labels_dev with other_strides; given iff occ_dev is */
    int64_t other_strides[2];
    int32_t min_pixels;              /* >= 1: a slot with fewer class-0 pixels has no model */
    int32_t min_affine;              /* >= 3: a slot with fewer class-0 pixels gets a translation only */
    double min_det;                  /* finite, > 0, in px^4: so does a slot whose det is below it */
    int64_t* sums_dev;               /* out [R, 65, 16] int64: step 4, entries 14 and 15 are 0 */
    int32_t* counts_dev;             /* out [R, 65, 4]: pixels of class 0 (believed), 1 (inconsistent), 2 (unusable or leaving the frame), then 0 */
    double* model_dev;               /* out [R, 65, 12] float64: step 6 */
    int32_t* occ_dev;                /* out [R, 65, 65] or NULL: occ[l][m], the pixels of slot l that were hidden where slot m stands in the other frame */
} cwm_object_motion_args;

/* Per-object motion and occlusion order: how every slot of a slot map (cwm_segment_merge, cwm_segment_track) moves between two frames, and which slot stands in
 * front of which, from the flow, the codes of cwm_flow_consistency and the other frame's slot map, in one call on the device, without a read-back.  Slot 0,
 * everything that is no object, is summed like any other: its model is the camera's own motion.  No counterpart in the reference, whose README lists read-outs
 * of this kind as coming ("using counterfactuals to estimate other scene properties").  Per row and pixel (x, y):
 *   1 slot     l = labels[y][x], or 0 if that is above 64
 *   2 target   (u, v) = flow[:, y, x]; USABLE iff both are finite and |u| <= 4096 and |v| <= 4096; fx = (float)x + u, fy = (float)y + v (one fp32 add each);
 *              INSIDE iff fx >= 0 && fx <= W-1 && fy >= 0 && fy <= H-1, in fp32 and before anything is converted: step 1 of cwm_flow_consistency
 *   3 class    k = 2 if the vector is not usable or the pixel not inside; otherwise 1 if code_dev is given and code[y][x] != 0; otherwise 0.
 *              counts[l][k] += 1; counts[l][3] stays 0
 *   4 sums     k = 0 only: qu = (int)rintf(u * 256.0f), qv likewise (the multiply is exact, |q| <= 2^20: the flow is held in 1/256 px).  sums[l][0..13] +=
 *              1, x, y, x x, x y, y y, qu, qv, x qu, y qu, x qv, y qv, qu qu, qv qv.  x, y < 2^16, so over the at most 2^18 pixels of a row sum x x <= 2^50,
 *              sum x qu <= 2^54 and sum qu qu <= 2^58: nothing wraps
 *   5 occluder k = 1 only, and only with other_dev: m = other[(int)rintf(fy)][(int)rintf(fx)], or 0 if that is above 64; occ[l][m] += 1.  The row is the slot
 *              that was hidden, the column what stands there in the other frame; the diagonal is counted too (a flow that is wrong on the object itself)
 *   6 model    per row and slot, after all pixels.  Every operator is ONE correctly rounded binary64 operation, evaluated as parenthesised: no fused
 *              multiply-add, no reciprocal; a sum enters through a round-to-nearest int64 -> double conversion.  With n = (double)N, N = sums[l][0], and S.. the
 *              other sums:
 *                mx = (Sx/n)  my = (Sy/n)  mu = (Su/n)  mv = (Sv/n)
 *                cxx = ((Sxx/n) - (mx mx))  cxy = ((Sxy/n) - (mx my))  cyy = ((Syy/n) - (my my))
 *                cxu = ((Sxu/n) - (mx mu))  cyu = ((Syu/n) - (my mu))  cxv = ((Sxv/n) - (mx mv))  cyv = ((Syv/n) - (my mv))
 *                det = ((cxx cyy) - (cxy cxy))
 *                tu = (mu 2^-8)  tv = (mv 2^-8)  var_u = (((Suu/n) - (mu mu)) 2^-16)  var_v = (((Svv/n) - (mv mv)) 2^-16)
 *                a11 = ((((cxu cyy) - (cyu cxy)) / det) 2^-8)  a12 = ((((cyu cxx) - (cxu cxy)) / det) 2^-8)  a21, a22: the same with cxv, cyv
 *              model[l] = (valid, tu, tv, a11, a12, a21, a22, mx, my, var_u, var_v, 0): the predicted flow of a pixel of the object is t + A ((x, y) - (mx, my)).
 *              valid = 0 and all twelve 0 if N < min_pixels; valid = 2 if N >= min_affine and det >= min_det; otherwise valid = 1 and A = 0
 * Two kernels behind the memsets of the three integer outputs, which are the accumulation targets (the call zeroes them itself on the stream; there is no
 * workspace): an accumulate pass (4 pixels per thread, 1024 per workgroup, the tables in LDS, a wave that holds one slot sums over the wave first) that adds its
 * non-zero entries with INTEGER atomics -- the same bits in any order, two calls on the same inputs give the same bits --, and one thread per (row, slot) for
 * step 6.  Asynchronous on base.stream: nothing is allocated and the host is not synchronised.  No content of a device buffer (label bytes above 64, NaN, inf and
 * huge flows, any code byte) makes the call read or write outside its buffers.  The outputs may not overlap the inputs.
 * Limits: 1 <= batch, 1 <= T, batch T <= 65535; H and W positive multiples of 4, H W <= 2^18; labels_dev and flow_dev non-NULL; strides not negative;
 * min_pixels >= 1, min_affine >= 3, min_det finite and > 0; sums_dev, counts_dev and model_dev non-NULL; occ_dev non-NULL iff other_dev is.  Argument errors:
 * CWM_ERR_INVALID with a message that names the field, before anything is launched or written. */
CWM_API int cwm_object_motion(const cwm_object_motion_args* args);

typedef struct cwm_point_track_args {
    uint32_t struct_size;            /* sizeof(cwm_point_track_args); anything else: CWM_ERR_INVALID naming struct_size */
    /* read: batch (B), T (the number of FRAMES), H, W and the stream.  Every other field of base is ignored, base.struct_size and base.P included */
    cwm_patch_error_args base;
    const float* fwd_dev;            /* [B, T-1, 2, H, W] in PAIR order: entry t is the flow from frame t to frame t+1 on frame t's grid; pixel (b, t, c, y, x) at
                                      * fwd_dev[b fwd_strides[0] + t fwd_strides[1] + c fwd_strides[2] + y W + x]; c = 0 horizontal, 1 vertical, in pixels */
    int64_t fwd_strides[3];          /* batch, pair and channel stride in elements, not negative */
    const float* bwd_dev;            /* NULL, or the same shape in pair order, addressed with bwd_strides: entry t is the flow from frame t+1 back to frame t on
                                      * frame t+1's grid */
    int64_t bwd_strides[3];
    float alpha, beta;               /* finite, >= 0: thr = alpha mag + beta of the forward-backward test (read with bwd_dev, checked always) */
    const uint8_t* labels_dev;       /* NULL, or the slot maps [B, T, H, W]: frame (b, t) is the H W contiguous bytes at labels_dev + b labels_strides[0] +
                                      * t labels_strides[1]; a byte above 64 reads as 0 */
    int64_t labels_strides[2];       /* batch and frame stride in elements, not negative */
    const double* model_dev;         /* NULL, or [B, T, 65, 12] float64 as cwm_object_motion writes model_dev: row (b, t, slot) is the 12 contiguous doubles at
                                      * model_dev + b model_strides[0] + t model_strides[1] + 12 slot; entry t describes the pair (t, t+1) in the slots of frame
                                      * t; entry T-1 is not read.  Needs labels_dev; 8-byte aligned */
    int64_t model_strides[2];        /* batch and frame stride in elements (doubles), not negative */
    const float* points_dev;         /* [B, K, 2] contiguous: (x, y) in pixels */
    const int32_t* start_dev;        /* NULL (every point begins in frame 0), or [B, K] contiguous: the frame a point begins in.  A value outside 0 .. T-1 gives
                                      * a point that is never started */
    int32_t K;                       /* 1 .. 65536 points per row */
    int32_t max_coast;               /* >= 0: a point hidden for more than this many consecutive frames is lost */
    float* xy_dev;                   /* out [B, T, K, 2]: the point in frame t, the quiet NaN 0x7fc00000 twice for a terminal or not-started entry */
    uint8_t* state_dev;              /* out [B, T, K]: 0 visible, 1 hidden and coasting, 2 left the frame, 3 lost, 255 not started yet */
    uint8_t* under_dev;              /* out [B, T, K]: the slot the point stands on in frame t (0 without labels, and for a terminal or not-started entry) */
    uint8_t* owner_dev;              /* out [B, K]: the slot the point stood on in its start frame: the object it is tracked with */
} cwm_point_track_args;

/* Point tracks through a movie: where K query points per row go over T frames and when they are hidden, in one call and one kernel launch on the device,
 * without a read-back.  A point follows the forward flow of its pair while it stands on the object it started on and the flow can be believed; otherwise it
 * coasts on the affine motion model of its object (cwm_object_motion's model_dev: its first consumer) or, without one, on its last believed flow vector, and is
 * picked up again when it stands on its object once more.  No counterpart in the reference.  Every fp32 step below is ONE correctly rounded fp32 operation in
 * the stated order and every float64 step one binary64 operation: nothing is contracted into a fused multiply-add.  Per row b and point k, with
 * s = start[b][k] (0 without start_dev), p_s = points[b][k], last = (0, 0), run = 0; for t = s .. T-1, until a terminal state, which then holds to the last frame:
 *   1 inside   p = (px, py) is INSIDE iff px >= 0 && px <= W-1 && py >= 0 && py <= H-1, in fp32 and before anything is converted (a NaN or inf point is
 *              outside).  Outside: state 2 from this frame on
 *   2 under    under_t = labels[t][(int)rintf(py)][(int)rintf(px)], or 0 if that is above 64, or 0 without labels_dev.  owner = under_s (0 if p_s is outside)
 *   3 hidden   with labels_dev hidden_t = (under_t != owner); without, hidden_t = (t > s and the step into frame t was a coast).  run = hidden_t ? run + 1 : 0;
 *              run > max_coast: state 3 from this frame on.  Otherwise state_t = hidden_t ? 1 : 0, xy_t = p, and for t < T-1 the point steps:
 *   4 flow     tried iff under_t == owner (always without labels_dev).  a_c = the bilinear sample of fwd[t] channel c at p by step 2 of cwm_flow_consistency:
 *              x0f = floorf(px), wx = px - x0f, ix0 = (int)x0f, ix1 = min(ix0 + 1, W-1), the same in y; top = o00 + wx (o01 - o00),
 *              bot = o10 + wx (o11 - o10), a_c = top + wy (bot - top).  USABLE iff |a_0| <= 4096 && |a_1| <= 4096 (false for a NaN).
 *              q = (px + a_0, py + a_1).  Usable and q not INSIDE: the point leaves, p_{t+1} = q (step 1 makes that state 2).  Usable, q inside and bwd_dev
 *              given: o_c = the same sample of bwd[t] at q; ru = a_0 + o_0, rv = a_1 + o_1, res = ru ru + rv rv; mag = (a_0 a_0 + a_1 a_1) + (o_0 o_0 + o_1 o_1);
 *              thr = alpha mag + beta (steps 3 and 4 of cwm_flow_consistency with (u, v) = a and s = o).  BELIEVED iff usable, q inside and (no bwd_dev or
 *              res <= thr).  Believed: p_{t+1} = q, last = a
 *   5 coast    when the flow step was not tried, or tried and neither believed nor leaving.  c = last.  With model_dev and m = model[b][t][owner],
 *              m.valid >= 1 (false for a NaN): dx = (double)px - mx, dy = (double)py - my; e0 = a11 dx, e1 = a12 dy, cu = e0 + e1, cu = tu + cu; e0 = a21 dx,
 *              e1 = a22 dy, cv = e0 + e1, cv = tv + cv; f = ((float)cu, (float)cv), rounded to nearest; c = f if both are finite (valid == 1 has a zero
 *              matrix: the same lines serve both values).  p_{t+1} = (px + c_0, py + c_1); the step into t+1 counts as a coast
 * Frames before s, and every frame of a point whose start is outside 0 .. T-1, are state 255.  A terminal (2, 3) or not-started (255) entry has xy = the quiet
 * NaN 0x7fc00000 twice and under = 0; the owner of a point that never started, or started outside, is 0.  The outputs are frame-major, so that one frame's
 * points are one slice.
 * One kernel: a thread owns a point and walks its frames, 64 points (one wave) per workgroup, so that few points still spread over many CUs -- the work of a
 * point is a chain of dependent cache round trips (the label byte, the eight taps of fwd, the eight taps of bwd where the first eight point, rarely the model
 * row) that only other waves hide.  Only vector stores; no atomics, no workspace: two calls on the same inputs give the same bits.  Asynchronous on
 * base.stream: nothing is allocated and the host is not synchronised.  No content of a device buffer (NaN, inf and huge flows, points or model entries, label
 * bytes above 64, any start) makes the call read or write outside its buffers.  The outputs may not overlap the inputs.
 * Limits: 1 <= batch <= 65535; 2 <= T <= 4096; H, W >= 1 (no multiple of 4 is asked for), H W <= 2^18; 1 <= K <= 65536; max_coast >= 0; fwd_dev and points_dev
 * non-NULL; strides not negative; alpha and beta finite and >= 0; model_dev only with labels_dev, and 8-byte aligned; the float and int32 buffers 4-byte
 * aligned; all four outputs non-NULL.  Argument errors: CWM_ERR_INVALID with a message that names the field, before anything is launched or written. */
CWM_API int cwm_point_track(const cwm_point_track_args* args);

typedef struct cwm_object_response_args {
    uint32_t struct_size;            /* sizeof(cwm_object_response_args); anything else: CWM_ERR_INVALID naming struct_size */
    /* read: batch (B scenes), T (K pushes per scene), H, W and the stream.  Every other field of base is ignored, base.struct_size and base.P included.
     * Rows r = b K + k, R = B K */
    cwm_patch_error_args base;
    const float* flows_dev;          /* the counterfactual flow samples [R, 2, H, W, S]: element (r, c, y, x, s) at flows_dev[r st[0] + c st[1] + y st[2] + x st[3] +
                                      * s st[4]] (elements), st = flow_strides, as cwm_segment_step takes them: the `_batch_to_samples` view of the flow model's
                                      * output is read in place.  c = 0 horizontal, 1 vertical, in pixels */
    int64_t flow_strides[5];         /* not negative */
    int32_t S;                       /* 1 .. 255 samples per push */
    const uint8_t* labels_dev;       /* the slot map of (b, k): H W contiguous bytes at labels_dev + b labels_strides[0] + k labels_strides[1] (0: none, 1 .. 64: a
                                      * slot; a byte above 64 reads as 0).  labels_strides[1] = 0 is the normal case: all K pushes of a scene read one map */
    int64_t labels_strides[2];       /* scene and push stride in elements, not negative */
    const int32_t* pushed_dev;       /* [R]: the slot pushed in row r; anything outside 1 .. 64 is a dead row */
    const int32_t* dirs_dev;         /* NULL, or [S, 2] (dy, dx): the shift of sample s in pixels, each |d| <= 4096, shared by all rows */
    int64_t min_q2;                  /* >= 0: the squared motion threshold in (1/256 px)^2; for a threshold of m pixels, round(256 m)^2 */
    int32_t min_pixels;              /* >= 1: a sample is valid only if the pushed slot has that many usable pixels */
    double self_frac, move_frac;     /* finite, in [0, 1]: the share of a slot's usable pixels that must have moved, for the pushed slot and for the others */
    int64_t* tab_dev;                /* out [R, S, 65, 8] int64: step 4; entry 7 counts the pixels whose flow is not usable */
    uint8_t* valid_dev;              /* out [R, S]: step 5, 0 / 1 */
    int64_t* agg_dev;                /* out [R, 65, 4] int64: step 6, (N, M, A, V) */
    double* coupling_dev;            /* out [R, 65, 4] float64: step 7, (c0, c1, c2, c3) */
    int32_t* stats_dev;              /* out [R, 4]: step 8 */
} cwm_object_response_args;

/* Object interactions: which slots of a slot map (cwm_segment_merge, cwm_segment_track) move when one of them is pushed, from the S counterfactual flow samples of
 * each of K pushes per scene, in one call on the device, without a read-back.  Where cwm_segment_step asks which PIXELS move with a seed, this asks which OBJECTS
 * move with an object.  No counterpart in the reference, whose README describes the covariance it reads out ("objects adjacent to one another tend to move
 * together, as some motion counterfactuals include collisions between them").  Every step is an integer operation or ONE correctly rounded binary64 operation,
 * evaluated as parenthesised.  Per row r, sample s and pixel (x, y):
 *   1 slot     l = labels[y][x], or 0 if that is above 64
 *   2 usable   (u, v) = flows[r, :, y, x, s]; USABLE iff |u| <= 4096 and |v| <= 4096 (false for a NaN and an inf).  Not usable: tab[r][s][l][7] += 1 and nothing
 *              else happens
 *   3 quantise qu = (int)rintf(u * 256.0f), qv likewise (the multiply is exact); q2 = (int64)qu qu + (int64)qv qv; moved = q2 >= min_q2: an integer comparison,
 *              no fp32 magnitude exists whose last bit a compiler could move
 *   4 table    tab[r][s][l][0..6] += 1, moved, qu, qv, moved ? qu : 0, moved ? qv : 0, q2.  |q| <= 2^20 and H W <= 2^18: every sum stays below 2^59
 * Then per row, with a = pushed[r] and n_l(s), m_l(s), su_l(s), sv_l(s) = entries 0 .. 3 of tab[r][s][l]:
 *   5 valid    sample s is VALID iff a is in 1 .. 64, n_a(s) >= min_pixels and ((double)m_a(s) / (double)n_a(s)) >= self_frac: the pushed object itself moved.
 *              valid[r][s] = 1 / 0; n_valid = the number of valid samples
 *   6 agg      per slot l = 0 .. 64, over the valid samples only: N_l = sum n_l(s); M_l = sum m_l(s); A_l = sum (su_l(s) dx_s + sv_l(s) dy_s), int64, at most 2^59,
 *              0 without dirs_dev; V_l = the number of valid s with n_l(s) > 0 and ((double)m_l(s) / (double)n_l(s)) >= move_frac.  agg[r][l] = (N, M, A, V)
 *   7 coupling c0 = ((double)V_l / (double)n_valid), or 0 if n_valid = 0: the share of valid pushes in which l moved
 *              c1 = ((double)M_l / (double)N_l), or 0 if N_l = 0
 *              c2 = (((double)A_l / (double)N_l) 2^-8), or 0 if N_l = 0: the mean displacement of l along the push
 *              c3 = (((double)A_l / (double)N_l) / ((double)A_a / (double)N_a)), or 0 if N_l = 0, N_a = 0 or A_a = 0: the gain, 1 where l moves as far as a
 *              Slot 0 is a row like any other: how much the background gives way
 *   8 stats    (n_valid, a or 0 for a dead row, n_a(0) + tab[r][0][a][7] -- the area of the pushed slot; 0 for a dead row --, 0)
 * Two kernels behind one memset of tab_dev, which is the accumulation target (the call zeroes it itself on the stream; there is no workspace): an accumulate
 * pass over (chunks of 1024 pixels, S, R) -- 4 pixels per thread, the 65 x 8 table in LDS, a wave that holds one slot sums over the wave first; 16-byte loads
 * where the view has contiguous planes on their alignment, a scalar form through all five strides otherwise -- that adds its non-zero entries with INTEGER
 * atomics: the same bits in any order, two calls on the same inputs give the same bits; and one workgroup per row for steps 5 - 8.  Asynchronous on
 * base.stream: nothing is allocated and the host is not synchronised.  No content of a device buffer (label bytes above 64, NaN, inf and huge flows, any
 * pushed_dev entry) makes the call read or write outside its buffers.  The outputs may not overlap the inputs.
 * Limits: 1 <= batch, 1 <= T, batch T <= 65535; H and W positive multiples of 4, H W <= 2^18; 1 <= S <= 255; strides not negative; flows_dev, labels_dev,
 * pushed_dev and all five outputs non-NULL (dirs_dev may be NULL); min_q2 >= 0; min_pixels >= 1; self_frac and move_frac finite and in [0, 1].  Argument errors:
 * CWM_ERR_INVALID with a message that names the field, before anything is launched or written. */
CWM_API int cwm_object_response(const cwm_object_response_args* args);

typedef struct cwm_parallax_args {
    uint32_t struct_size;            /* sizeof(cwm_parallax_args); anything else: CWM_ERR_INVALID naming struct_size */
    /* read: batch (R rows), H, W and the stream.  Every other field of base is ignored, base.struct_size, base.T and base.P included */
    cwm_patch_error_args base;
    const float* flows_dev;          /* the S ego-motion flow samples [R, 2, H, W, S]: element (r, c, y, x, s) at flows_dev[r st[0] + c st[1] + y st[2] + x st[3] +
                                      * s st[4]] (elements), st = flow_strides: the `_batch_to_samples` view of the flow model's output is read in place.
                                      * c = 0 horizontal, 1 vertical, in pixels */
    int64_t flow_strides[5];         /* not negative */
    int32_t S;                       /* 1 .. 64 samples */
    const int32_t* dirs_dev;         /* NULL, or [S, 2] (dy, dx): the image motion sample s was asked for, in pixels, each |d| <= 4096, shared by all rows */
    const uint8_t* labels_dev;       /* NULL, or the slot map of row r: H W contiguous bytes at labels_dev + r labels_stride (0: none, 1 .. 64: a slot; a byte
                                      * above 64 reads as 0) */
    int64_t labels_stride;           /* row stride in elements, not negative */
    int32_t ref_slot;                /* -1, or 0 .. 64 (needs labels_dev): without dirs_dev the reference motion is measured on the pixels of this slot only */
    int32_t min_pixels;              /* >= 1: a sample is live only if its reference motion rests on that many pixels */
    int64_t min_ref_q;               /* 1 .. 2^21: the smallest reference motion, in 1/256 px */
    int32_t min_samples;             /* 1 .. S: a pixel with fewer live, usable samples has no parallax */
    float* par_dev;                  /* out [R, H, W]: step 5, the lower median of the motion along the reference, in units of the reference motion */
    float* spread_dev;               /* out [R, H, W] or NULL: step 5, the interquartile range of the same values */
    float* off_dev;                  /* out [R, H, W] or NULL: step 5, the lower median of the motion across the reference */
    uint8_t* cnt_dev;                /* out [R, H, W] or NULL: step 5, the number of live, usable samples */
    double* ref_dev;                 /* out [R, S, 4] float64, 8-byte aligned: step 3, (mu, mv, den, live).  Without dirs_dev it is also where the sums are gathered */
    int32_t* hist_dev;               /* out [R, 65, 256] int32, 16-byte aligned; needed with labels_dev, ignored without: step 6 */
    int32_t* slot_tab_dev;           /* out [R, 65, 8] int32; needed with labels_dev, ignored without: step 7 */
} cwm_parallax_args;

/* Motion parallax: from S flow samples of one scene under S different motions of the VIEWER (a pan of anchored patches, or a head motion given to an
 * IMU-conditioned predictor) to a per-pixel parallax map and a per-slot depth table, in one call on the device, without a read-back.  Under a translation of the
 * viewer near things sweep across the image faster than far ones: the parallax of a pixel is how far it moves along the motion of a reference (the whole image,
 * or the pixels of one slot), as a multiple of that motion; the median over the samples is the read-out, a slot's histogram of it the depth cue.  A pure
 * rotation of the viewer moves every pixel alike and gives a flat map.  No counterpart in the reference, whose README lists "using counterfactuals to estimate
 * other scene properties" as coming.  Every step is an integer operation or ONE correctly rounded binary64 (where stated: binary32) operation, evaluated as
 * parenthesised; nothing is contracted into a fused multiply-add.  Per row r, sample s and pixel (x, y):
 *   1 usable   (u, v) = flows[r, :, y, x, s]; USABLE iff |u| <= 4096 and |v| <= 4096 (false for a NaN and an inf): step 2 of cwm_object_response
 *   2 quantise qu = (int64)rintf(u * 256.0f), qv likewise (round half even; the multiply is exact).  A sample that is not usable contributes nothing anywhere
 *   3 ref      per (r, s).  With dirs_dev: mu = (double)(256 dx_s), mv = (double)(256 dy_s), N = H W.  Without: SU, SV, N = the int64 sums of qu, qv and 1 over
 *              the usable pixels of the row in sample s -- with ref_slot >= 0 only over those whose label (a byte above 64 reads as 0) equals ref_slot --;
 *              mu = ((double)SU / (double)N), mv = ((double)SV / (double)N), both 0 if N = 0.  den = ((mu mu) + (mv mv)): two multiplies and one add, each rounded
 *              on its own.  The sample is LIVE for the row iff N >= min_pixels and den >= ((double)min_ref_q (double)min_ref_q).  ref[r][s] = (mu, mv, den,
 *              live ? 1.0 : 0.0)
 *   4 project  for a usable pixel of a live sample: p = ((((double)qu mu) + ((double)qv mv)) / den), c = (|((double)qu mv) - ((double)qv mu)| / den).  The
 *              conversions are exact (|q| <= 2^20)
 *   5 order    n = the number of live, usable samples of the pixel; cnt = n.  n < min_samples: par, spread and off are the quiet NaN 0x7fc00000.  Otherwise
 *              the n values p are put in ascending order WITH TIES BROKEN BY THE SAMPLE INDEX (-0.0 and +0.0 compare equal: only a stable order makes the
 *              bits of the result determinate), P[0 .. n-1]; med = P[(n-1)/2] (the lower median), par = (float)med; spread = (float)(P[3(n-1)/4] - P[(n-1)/4]),
 *              one binary64 subtraction; off = (float)C[(n-1)/2] with the c values ordered by the same rule.  Each is rounded once to binary32, to nearest
 *   6 hist     only with labels_dev, l = the pixel's label (above 64: 0).  n >= min_samples: b = floor(med 32.0) + 128.0, clamped to 0 .. 255 as a double and
 *              then converted; hist[r][l][b] += 1.  Otherwise slot_tab[r][l][1] += 1
 *   7 slots    only with labels_dev: slot_tab[r][l] = (n, n_bad, b_med, b_q1, b_q3, b_min, b_max, 0) with n = the sum of hist[r][l], n_bad from step 6, and
 *              b_med, b_q1, b_q3 the bins of the order statistics k = (n-1)/2, (n-1)/4, 3(n-1)/4 of step 5: the lowest bin b whose cumulative count
 *              hist[r][l][0] + .. + hist[r][l][b] exceeds k; b_min and b_max the lowest and highest bin that is not empty.  n = 0: all five are -1
 * A bin is 1/32 of the reference motion wide and bin 128 starts at 0: the centre of bin b is (b - 127.5) / 32.
 * Three kernels behind the memsets of the tables the workgroups add into (hist_dev, slot_tab_dev and, without dirs_dev, ref_dev: the call zeroes them itself on
 * the stream; there is no workspace): the reference sums (skipped with dirs_dev) -- 4 pixels per thread, 16-byte loads where the view has contiguous planes on
 * their alignment, a scalar form through all five strides otherwise, wave sums, INTEGER atomics --; the pixels -- a thread per pixel whose S projections live in
 * LDS, ranked by counting; the histogram of the workgroup's first slot is gathered in LDS, and every count reaches memory as an INTEGER atomic --; and the
 * finalise pass, a wave per (row, slot).  Integer atomics give the same bits in any order: two calls on the same inputs give the same bits.  Asynchronous on
 * base.stream: nothing is allocated and the host is not synchronised.  No content of a device buffer (label bytes above 64, NaN, inf and huge flows, any
 * dirs_dev entry) makes the call read or write outside its buffers.  The outputs may not overlap the inputs.
 * Limits: 1 <= batch <= 65535; H and W positive multiples of 4, H W <= 2^18; 1 <= S <= 64; strides not negative; flows_dev, par_dev and ref_dev non-NULL, and
 * with labels_dev hist_dev and slot_tab_dev; ref_slot -1 or 0 .. 64, and only with labels_dev; min_pixels >= 1; 1 <= min_ref_q <= 2^21; 1 <= min_samples <= S.
 * Argument errors: CWM_ERR_INVALID with a message that names the field, before anything is launched or written. */
CWM_API int cwm_parallax(const cwm_parallax_args* args);

/* `RectangularizeMasks` (masking.py:90-132) on device masks without reading them back.  The reference equalises the masked count of
 * the rows of a batch by un-masking / masking `torch.randperm(#candidates)[:surplus]` of a row's masked / visible tokens (one draw of the global CPU
 * generator per changed row, in row order).  The draws depend on the per-row COUNTS alone, so:
 *   cwm_mask_row_counts  counts_dev[b] = number of masked (non-zero) tokens of row b                       (the host reads back 4 B per row)
 *   cwm_mask_flip_picks  applies the host's picks in place.  table_dev (int32): [R | rows[R] | offsets[R+1] | to_value[R] | picks[offsets[R]]] --
 *                        for changed row rows[i], every pick k in picks[offsets[i] .. offsets[i+1]) sets the k-th token (ascending position, 0-based,
 *                        counted on the row as it was BEFORE the call) whose state is not to_value[i] (0 = un-mask a masked token, 1 = mask a
 *                        visible one) to to_value[i].  n_rows = R.  Rows of at most 16384 tokens.  A table row whose rows[i] is outside [0, B) is skipped:
 *                        nothing is written for it.  Both asynchronous on `stream`. */
CWM_API int cwm_mask_row_counts(const uint8_t* mask_dev, int B, int Nt, int32_t* counts_dev, void* stream);
CWM_API int cwm_mask_flip_picks(uint8_t* mask_dev, int B, int Nt, const int32_t* table_dev, int n_rows, void* stream);

/* Motion-counterfactual prompt construction for B*S prompts at once.
 * replaces: the per-sample loop of FlowGenerator.create_motion_counterfactuals (segmentation.py:324-338)
 *           = PatchPerturbation.forward + ShiftPatchesAndMask.perturb (perturbation.py:99-113, 245-289)
 *           on make_static_movie(x) when fix_passive=1 (prediction.py:731-739), or on MakeStatic(x, masks)
 *           when fix_passive=2 (perturbation.py:120-145 as called at prediction.py:802-803: the patches `masks`
 *           leaves visible take their frame-0 pixels), BEFORE the final mask_rectangularizer call (host).  x [B,T,C,H,W]; active/masks [B*S,Nt] bool ('(b s)' order,
 *           0 = active patch / 0 = passive visible patch); shifts [B*S,2] (dy,dx) in patch units;
 *           outputs x_out [B*S,T,C,H,W], mask_out [B*S,Nt]; either one may be NULL (masks only: what rank 0 of the sharded loop needs
 *           for all prompts before the rectangulariser; frames only: the rows a rank predicts -- x_dev may be NULL with x_out_dev).
 *           Asynchronous on `stream`. */
/* The prompt table of a counterfactual batch -> the dense operands of cwm_shift_prompts, in one launch (no counterpart in the reference, which builds the
 * masks prompt by prompt on the host: interface.py:370-377, segmentation.py:324-338).  table_dev int32 [S,4] rows (active_h, active_w, dy, dx): ONE active
 * patch of frame `frame` (>= 1) per prompt, moved by (dy, dx) patches, nothing passive.  Writes passive [S,Nt] (frame 0 visible, later frames masked),
 * active [S,Nt] (= passive with the prompt's patch cleared) and shifts [S,2].  A row whose cell is outside the grid (active_h outside [0, grid_h) or active_w
 * outside [0, grid_w)) clears nothing -- the kernel tests both coordinates, not the linear index -- and its shift is still copied.  Asynchronous on `stream`. */
CWM_API int cwm_prompt_table_expand(const int32_t* table_dev, int S, int T, int grid_h, int grid_w, int frame, uint8_t* active_dev, uint8_t* passive_dev,
                            int32_t* shifts_dev, void* stream);
CWM_API int cwm_shift_prompts(const float* x_dev, int B, int T, int C, int H, int W, int P, int frame, int S, int fix_passive,
                      const uint8_t* active_dev, const uint8_t* masks_dev, const int32_t* shifts_dev, float* x_out_dev,
                      uint8_t* mask_out_dev, void* stream);

/* Multi-shift prompts (0.10.3): K steps per prompt, each moving ITS OWN set of patches of frame `frame` by ITS OWN pixel shift, for R = B*S prompts at once.
 * replaces: MultiShiftPatchesAndMask.forward (perturbation.py:644-779; the generator's `multi_patch_shifter`, prediction.py:59-64) = K rounds of
 *           ShiftPatchesAndMask.perturb in fractional mode (:227-289: pad / centre-crop / patchify / blend of the whole frame per step), looped per sample,
 *           BEFORE the mask rectangulariser (host).
 * Tables, one row per prompt i = b*S + s ('(b s)' order; prompt i reads movie i / S), Nt = T (H/P) (W/P) tokens, n = (H/P)(W/P):
 *   points_dev [R,K,Nt] uint8  A_k: non-zero = this patch is moved at step k (the reference's perturbation_points_sequence[i,:,k]; only frame `frame` moves).
 *                              STEP-MAJOR, not the reference's [R,Nt,K]: adjacent threads handle adjacent cells of one step, so a wave's reads of a step are
 *                              consecutive bytes instead of bytes K apart.
 *   masks_dev  [R,mask_steps,Nt] uint8  M_k: non-zero = masked (mask_sequence[i,:,k]); mask_steps = K, or 1 for one base mask shared by every step.
 *                              NULL = the reference's call without points (A_k := ~M_k, no base mask: pass ~M_k as points_dev).
 *   shifts_dev [R,K,2] int32   (sy_k, sx_k) in PIXELS, any sign, not tied to P.  max_abs_shift is the caller's bound on |s| over the table (the library does
 *                              not read device tables on the host); it must be < min(H, W).  The kernels test every access against the grid and the image
 *                              whatever the table holds.
 * With my_k = sign(sy_k) (|sy_k| / P) (truncated toward zero: sy = -3, P = 8 gives 0), mx_k likewise, f = frame:
 *   mask:   shifted_k[t,pi,pj] = !A_k[f, pi - my_k, pj - mx_k] for t == f (1 if that cell is outside the grid), !A_k[t,pi,pj] for t != f;
 *           step_k = (M_k | A_k) & shifted_k with masks_dev, shifted_k without;  mask_out [R,Nt] = AND_k step_k (visible if any step leaves it visible).
 *   frames: x_out [R,T,C,H,W]; frames t != f are copies.  For pixel (y, x) of frame f keep a position (cy, cx) = (y, x) and walk k = K .. 1: if the cell
 *           (cy / P - my_k, cx / P - mx_k) is inside the grid and A_k is set there in frame f, (cy, cx) -= (sy_k, sx_k); a position that leaves the image
 *           makes the pixel 0 (the reference's constant padding; only the sub-patch remainder at a border does that).  The output is the input pixel at the
 *           final position: steps compose in order, a later step wins where destinations overlap, and the result is bit-exact.
 * fix_passive: 0 = the movie as given, 1 = every output frame reads frame 0 (make_static_movie, prediction.py:731-739).  Requires W % 4 == 0, H % P == 0,
 * W % P == 0, 1 <= K <= 8, 16-byte aligned frames; a violation is CWM_ERR_INVALID and nothing is launched.  x_out_dev or mask_out_dev may be NULL (x_dev too
 * with x_out_dev), as in cwm_shift_prompts.  K = 1 with a whole-patch shift is cwm_shift_prompts with active = !A, masks = M, fix_passive 0 / 1.
 * Not reproduced from the reference: `_check_shapes` assigning to the read-only property `num_shifts` (:668-682 against :171-175; forward cannot run as
 * written), and `m_seq.expand(1, 1, num_shifts)` (:709) failing for a [B,N] mask with [B,N,K] points (mask_steps = 1 here).  Asynchronous on `stream`. */
CWM_API int cwm_multi_shift_prompts(const float* x_dev, int B, int T, int C, int H, int W, int P, int frame, int S, int K, int fix_passive,
                            const uint8_t* points_dev, const uint8_t* masks_dev, int mask_steps, const int32_t* shifts_dev, int max_abs_shift,
                            float* x_out_dev, uint8_t* mask_out_dev, void* stream);

/* ---- flow-sample statistics: the reductions over the S counterfactual flow samples -------------
 * flows: fp32 device tensor addressed as flows[b*strides[0] + c*strides[1] + y*strides[2] + x*strides[3] + s*strides[4]]
 * (elements), so both the reference's [B,C,H,W,S] view and the sample-major [(b s),C,H,W] batch the flow model emits work
 * without a copy.  All asynchronous on `stream`.
 *
 * cwm_flow_features   x[B][P][S], P = (H/ds)(W/ds): ds x ds average pool per channel, then sqrt(mean_c(.^2))
 *                     replaces: the `_ds` + `distance_func` (= ChannelMSE(dim=1) against zeros) prologue of
 *                     FlowGenerator.compute_flow_corrs (segmentation.py:503-513; utils.py:510-513)
 * cwm_flow_cov        out[B][nrows][P] = rows [row0, row0+nrows) of torch.cov(x[b]) (use_covariance) or torch.corrcoef(x[b])
 *                     over the S samples, NaN -> 0.  replaces: segmentation.py:538-546.  Work buffers: xc [B][P][S], inv_std [B][P].
 *                     Row slabs let ranks that all-gathered `x` each produce a part of the [P,P] matrix (dist.py).
 * cwm_flow_motion_sum sum[B][H*W] = sum_s |flow| (magnitude over channels), each sample first range-normalised over (H,W)
 *                     with max(range, eps) if normalize_per_sample (work buffer: cwm_flow_motion_work_bytes(B, S) bytes, 16-byte aligned).
 *                     replaces: compute_flow_samples_magnitude + the `.mean(-1)` numerator (segmentation.py:250-255, :264-268)
 *                     NaN / Inf as torch.amin / amax / clamp have them: with normalize_per_sample a NaN anywhere in a sample makes that sample's range NaN and
 *                     so every pixel of sum[b] NaN; an infinite magnitude gives NaN at its own pixel and 0 from that sample elsewhere.
 * cwm_flow_map_finish map = map*scale (scale = 1/S_total), then (map - min)/max(max - min, eps) per b if normalize.
 *                     replaces: segmentation.py:273-275.  Split from the sum so that sample shards can be all-reduced in between.
 *                     With normalize, one NaN in map[b] makes all of map[b] NaN (the range is NaN and the clamp keeps it); a +Inf becomes NaN at its pixel, 0 elsewhere. */
CWM_API int cwm_flow_features(const float* flows_dev, const int64_t* strides, int B, int C, int H, int W, int S, int downsample,
                      float* x_dev, void* stream);
/* cwm_flow_transform  the optional prologues of compute_flow_corrs on the pooled features, in place, in the reference's order
 *                     (segmentation.py:519-538; x[b] is its [P, S] matrix): spearman: every row -> argsort over its samples (as floats);
 *                     thresh_mode 1: x * (x > thresh), 2: (x > thresh), 3: ((x - min_P) > thresh * (max_P - min_P)) ("range_thresh");
 *                     normalize: x / max(max_P, eps); zscore: (x - mean_P) / max(std_P, eps), statistics over the P positions per sample.
 *                     stats_work_dev: cwm_flow_transform_work_bytes(B, P, S) bytes, 16-byte aligned (needed by mode 3, normalize, zscore): the [B][S] column
 *                     statistics and the per-chunk partials of the one-pass column reduction */
CWM_API size_t cwm_flow_transform_work_bytes(int B, int P, int S);
CWM_API int cwm_flow_transform(float* x_dev, int B, int P, int S, int spearman, int thresh_mode, float thresh, int normalize, int zscore, float eps,
                       float* stats_work_dev, void* stream);
CWM_API int cwm_flow_cov(const float* x_dev, int B, int P, int S, int row0, int nrows, int use_covariance, float* xc_work_dev,
                 float* inv_std_work_dev, float* out_dev, void* stream);
CWM_API size_t cwm_flow_motion_work_bytes(int B, int S);
CWM_API int cwm_flow_motion_sum(const float* flows_dev, const int64_t* strides, int B, int C, int H, int W, int S,
                        int normalize_per_sample, float eps, float* minmax_work_dev, float* sum_dev, void* stream);
CWM_API int cwm_flow_map_finish(float* map_dev, int B, int HW, float scale, int normalize, float eps, void* stream);

/* ---- the flow-sample filter (0.10): which of the S counterfactual flow samples are kept ------------------------------
 * replaces: cwm/models/sampling.py FlowSampleFilter.compute_flow_magnitude :163-205, filter_by_patch_magnitude :207-215,
 *           filter_by_flow_area :217-228, filter_by_num_corners :230-250 and forward :252-286
 * flows: as above, [B,2,H,W,S] by five element strides (H == W, as the reference asserts).  Coalesced for the sample-outermost view of the
 * flow model's [(b s),1,2,H,W] output (every (b,s,c) plane H W contiguous floats) and for the packed sample-innermost layout; any other
 * strides take a strided form.  active: the bool / uint8 mask [B,Np,S] (0 = active) by three element strides, Np = 2 h w patches of two frames,
 * h = w = int((Np/2)**0.5); only frame 2 (rows h w .. Np-1) is read.
 *
 * cwm_flow_filter_stats  per (b, s), all [B][S] contiguous:
 *     patch_mag     fp32: mean over the active patches of frame 2 of the bilinearly resized (F.interpolate(size=[h,w], mode='bilinear'),
 *                   align_corners=False, no antialiasing: source max((dst+.5) H/h - .5, 0), neighbours clamped to the last row / column)
 *                   magnitude sqrt(u^2 + v^2), evaluated at the active patches only; an empty active set gives 0 / 1e-12 = 0.  (The
 *                   reference multiplies the whole resized map by the 0/1 mask, so a NaN under an INACTIVE patch's taps makes its
 *                   patch_mag NaN; here only a NaN under an active patch does.)  Summed in a fixed order: bitwise reproducible.
 *     area_count    int32: #pixels with magnitude > flow_magnitude_threshold (the reference's flow_area is area_count / (H W))
 *     corner_count  int32: how many of the four corner pixels exceed the threshold
 *     reject        uint8: the OR over the enabled `methods` bits of  patch_mag < flow_magnitude_threshold,
 *                   area_count / (H W) > flow_area_threshold,  corner_count >= num_corners_threshold  (NaN compares false, as in torch)
 *   The streaming pass reads every flow element once; the patch mean then reads the 8 floats under each active patch's four taps.
 * cwm_flow_filter_apply  zeroes, in place, both channels of every sample with reject != 0; reads no flow element and writes no other byte.
 * cwm_flow_filter_pack   out[B][2][H][W][S] (contiguous) = the sample-outermost flows with rejected samples as zeros (not read): the packed tensor
 *                   `forward` returns (`flow_samples.contiguous()`, :286).  Every sample must be one contiguous [2,H,W] block.
 * CWM_ERR_INVALID: C != 2, H != W, Np odd or not 2 h w, S < 1, a null pointer, unknown method bits.  All asynchronous on `stream`. */
#define CWM_FLOW_FILTER_PATCH_MAGNITUDE 1
#define CWM_FLOW_FILTER_FLOW_AREA 2
#define CWM_FLOW_FILTER_NUM_CORNERS 4
CWM_API int cwm_flow_filter_stats(const float* flows_dev, const int64_t* strides, int B, int C, int H, int W, int S, const uint8_t* active_dev,
                          const int64_t* active_strides, int Np, int methods, float flow_magnitude_threshold, float flow_area_threshold,
                          float num_corners_threshold, float* patch_mag_dev, int32_t* area_count_dev, int32_t* corner_count_dev,
                          uint8_t* reject_dev, void* stream);
CWM_API int cwm_flow_filter_apply(float* flows_dev, const int64_t* strides, int B, int C, int H, int W, int S, const uint8_t* reject_dev, void* stream);
CWM_API int cwm_flow_filter_pack(const float* flows_dev, const int64_t* strides, int B, int C, int H, int W, int S, const uint8_t* reject_dev,
                         float* out_dev, void* stream);

/* ---- collectives around the sharded counterfactual-sampling loop (SURVEY.md 8e / 8b "comm"; BASELINE configs[3]) ----------
 * The reference has no multi-GPU code: it chunks the S prompts of one frame pair over ONE device (prediction.py:513-540,
 * segmentation.py:423-430).  Here the prompts are sharded over one process per GPU and these entry points are the only
 * communication: RCCL (over xGMI) called directly, asynchronous on `stream`, byte counts, device pointers.
 *   cwm_comm_unique_id   rank 0: a fresh 128-byte id, to be handed to the other ranks by any out-of-band means
 *                        (counterfactualworldmodels_amd/dist.py uses the torch.distributed store of the launcher)
 *   cwm_comm_init        collective over all ranks; binds the communicator to the CURRENT HIP device
 *   cwm_broadcast        in place, from `root`: the packed {frame pair | prompt table | masks} buffer
 *   cwm_allgather        equal blocks: recv[r*bytes_per_rank ...] = rank r's send block
 *   cwm_allgatherv       blocks of counts[r] bytes at offsets[r] of recv (host arrays of length nranks); send may alias its own slot
 *   cwm_allreduce_sum_f32  in place (sample-sharded motion map, segmentation.py:257-276)
 * cwm_comm_load(path) optionally names the RCCL shared object to bind (default: the copy already mapped into the process --
 * PyTorch's -- else the ROCm install); cwm_comm_version() returns its NCCL_VERSION_CODE or -1. */
#define CWM_COMM_ID_BYTES 128
typedef struct cwm_comm cwm_comm;
CWM_API int cwm_comm_load(const char* rccl_path);
CWM_API int cwm_comm_version(void);
CWM_API int cwm_comm_unique_id(uint8_t* id_out);
CWM_API int cwm_comm_init(int rank, int nranks, const uint8_t* id_in, cwm_comm** out);
CWM_API void cwm_comm_destroy(cwm_comm* c);
CWM_API int cwm_comm_rank(const cwm_comm* c);
CWM_API int cwm_comm_size(const cwm_comm* c);
CWM_API int cwm_broadcast(cwm_comm* c, void* buf_dev, size_t bytes, int root, void* stream);
CWM_API int cwm_allgather(cwm_comm* c, const void* send_dev, void* recv_dev, size_t bytes_per_rank, void* stream);
CWM_API int cwm_allgatherv(cwm_comm* c, const void* send_dev, void* recv_dev, const size_t* offsets, const size_t* counts, void* stream);
CWM_API int cwm_allreduce_sum_f32(cwm_comm* c, float* buf_dev, size_t count, void* stream);

/* ---- RAFT-large optical flow (0.9) --------------------------------------------------------------------
 * replaces: `load_raft_model(...)` / `RAFT.forward` of cwm/models/raft/raft_model.py:55-300 in the reference's inference
 * configuration (BasicEncoder fnet with instance norm, cnet with eval batch norm, 4 correlation levels of radius 4,
 * BasicUpdateBlock with SepConvGRU, convex upsampling; alternate_corr = False; output_dim = None or 1).
 * Arithmetic, chosen per call by cwm_raft_forward_args.mode (0.10.2; one handle serves both, alternating, without re-packing or reallocation):
 *   parity (mode 0 or CWM_MODE_PARITY, the default)  every convolution with split-bf16 operands (hi + lo, 3 MFMAs per product), fp32 accumulate:
 *                                                    <= 1e-2 px from the fp32 reference at 24 iterations
 *   fast   (CWM_MODE_FAST; the reference's --mixed_precision)  every convolution of fnet, cnet, the motion encoder, the GRU, the flow head, the
 *                                                    mask head and output_block.0 with ONE bf16 plane per operand (activation and folded weight
 *                                                    rounded to bf16), fp32 accumulate and fp32 epilogue
 * In both modes the activations between the convolutions, the instance-norm statistics, the residual join, the all-pairs correlation, its pooling
 * and lookup, the coordinates and the flow update, the GRU's pointwise update, output_block.2 and both convex upsamplings are fp32.
 * Weights: the reference's 179 state-dict keys and shapes (`num_batches_tracked` is accepted and ignored).
 * The output head (0.10.1; raft_model.py:152-159, 257-267, output_dim = 1: the keypoint predictor of the demo notebook) is four more keys,
 * `output_block.0.weight [256,128,3,3]`, `output_block.0.bias [256]`, `output_block.2.weight [1,256,1,1]`, `output_block.2.bias [1]`: optional
 * (cwm_raft_missing_weights does not count them; a model without them is the flow model), needed only by a forward that sets `head_dev`. */
typedef struct cwm_raft_model cwm_raft_model;
CWM_API int cwm_raft_create(cwm_raft_model** out);
CWM_API void cwm_raft_destroy(cwm_raft_model* m);
CWM_API int cwm_raft_load_weight(cwm_raft_model* m, const char* key, const float* data, int on_device, const int64_t* shape, int ndim);
CWM_API int cwm_raft_missing_weights(cwm_raft_model* m, char* buf, int buflen);

typedef struct cwm_raft_forward_args {
    uint32_t struct_size;          /* sizeof(cwm_raft_forward_args) */
    /* the frame pair (b, t), t < max(pairs, 1): image1 at image1_dev + b*image1_stride_b + t*image1_stride_t, channel c at + c*image1_stride_c,
     * rows of `width` contiguous (fp32 [3, H, W]); image2 likewise.  The model sees 2 * (v * input_scale / 255) - 1: input_scale 255 for
     * frames in [0, 1] (the multi-frame call, scale_inputs = True), 1 for frames in [0, 255] (the two-image call) */
    const float* image1_dev;
    int64_t image1_stride_b, image1_stride_t, image1_stride_c;
    const float* image2_dev;
    int64_t image2_stride_b, image2_stride_t, image2_stride_c;
    int32_t batch, pairs;
    int32_t height, width;         /* multiples of 8, H / 8 and W / 8 at least 16 */
    float input_scale;
    int32_t iters;                 /* >= 1 */
    /* out: flow_up of the last iteration, pixels (x, y): element (c, Y, X) of pair (b, t) at flow_dev + b*flow_stride_b + t*flow_stride_t +
     * c*flow_stride_c + Y*width + X (strides may be negative: the reversed pair order of the backward multi-frame call) */
    float* flow_dev;               /* may be NULL (since 0.10.1) when head_dev is given: the flow's full-resolution upsampling is then skipped */
    int64_t flow_stride_b, flow_stride_t, flow_stride_c;
    float* flow_low_dev;           /* optional: coords1 - coords0, [batch * pairs, 2, H/8, W/8] contiguous (the two-image call's first output) */
    void* stream;
    /* appended in 0.10.1, read only when struct_size covers them (a caller that passes the 0.10.0 size gets the 0.10.0 behaviour).
     * out, optional: the convex-upsampled (times 8, as a flow) output_block(net) of the last iteration in place of the flow: element (Y, X) of
     * pair (b, t) at head_dev + b*head_stride_b + t*head_stride_t + Y*width + X (strides may be negative).  head_stride_c is the channel stride
     * of the [.., output_dim, H, W] tensor; with output_dim = 1 it addresses nothing.  CWM_ERR_INVALID, naming the first missing key, unless all
     * four output_block weights are loaded.  At least one of flow_dev / head_dev must be given. */
    float* head_dev;
    int64_t head_stride_b, head_stride_t, head_stride_c;
    /* appended in 0.10.2, read only when struct_size covers it (a caller that passes the 0.10.0 or 0.10.1 size gets parity).
     * 0 or CWM_MODE_PARITY: parity arithmetic; CWM_MODE_FAST: bf16-operand convolutions (see above); anything else is CWM_ERR_INVALID. */
    int32_t mode;
} cwm_raft_forward_args;
CWM_API int cwm_raft_forward(cwm_raft_model* m, const cwm_raft_forward_args* args);

/* The same forward with RAFT's warm start and its per-iteration outputs (0.10.4).
 * replaces: the `flow_init` and `test_mode=False` arguments of `RAFT._forward_two_images` (raft_model.py:199-274): `coords1 = coords1 + flow_init`
 * (raft_model.py:241-242) and the list `flow_predictions` of every iteration's upsampled prediction (raft_model.py:244-274); through
 * raft_model.py:297 the multi-frame `RAFT.forward` hands both to every pair.
 * With the three optional pointers NULL this is cwm_raft_forward(m, &args->base), launch for launch: the mask head and the upsampling run once, after
 * the last iteration.  With flow_iters_dev or head_iters_dev they run in every iteration (the reference always does), and the final outputs of
 * `base`, when asked for, are produced as well.  cwm_raft_forward_args is frozen; what is added to the forward is added here. */
typedef struct cwm_raft_forward_ex_args {
    uint32_t struct_size;            /* sizeof(cwm_raft_forward_ex_args); anything else: CWM_ERR_INVALID naming struct_size */
    cwm_raft_forward_args base;      /* as for cwm_raft_forward, base.struct_size rules included; base.flow_dev and base.head_dev may both be NULL when
                                      * a per-iteration output is given; base.flow_low_dev receives coords1 - coords0 with the init included (the
                                      * reference's first return value); base.mode chooses parity or fast */
    /* in, optional: the initial flow in 1/8-resolution pixels, channel 0 = x: element (c, y, x) of pair (b, t) at flow_init_dev + b*flow_init_stride_b +
     * t*flow_init_stride_t + c*flow_init_stride_c + y*(W/8) + x, rows of W/8 contiguous.  A stride may be 0: one field for all pairs (stride_t) or for
     * all batch rows (stride_b) */
    const float* flow_init_dev;
    int64_t flow_init_stride_b, flow_init_stride_t, flow_init_stride_c;
    /* out, optional: flow_up of iteration i (0 <= i < base.iters) in the block at flow_iters_dev + i*flow_iters_stride_i, addressed inside the block
     * as base.flow_dev is: with base.flow_stride_b / _t / _c (a negative _t included) */
    float* flow_iters_dev;
    int64_t flow_iters_stride_i;
    /* out, optional: the convex-upsampled output_block(net) of iteration i at head_iters_dev + i*head_iters_stride_i, addressed inside the block
     * with base.head_stride_b / _t / _c.  Needs the four output_block weights: otherwise CWM_ERR_INVALID naming the first missing key, as head_dev */
    float* head_iters_dev;
    int64_t head_iters_stride_i;
} cwm_raft_forward_ex_args;
/* At least one of base.flow_dev, base.head_dev, flow_iters_dev, head_iters_dev must be given. */
CWM_API int cwm_raft_forward_ex(cwm_raft_model* m, const cwm_raft_forward_ex_args* args);

/* Stand-alone RAFT kernels (kernel tests; the same launches as the model):
 *   cwm_raft_corr_lookup      fmap1 / fmap2 [P, h8, w8, 256] (NHWC), coords [P, h8, w8, 2] (x, y) -> out [P, h8, w8, 324]: CorrBlock (corr.py:12-60)
 *                             built and indexed at coords, feature l*81 + a*9 + b sampled at (x / 2^l + a - 4, y / 2^l + b - 4).  Synchronises.
 *   cwm_raft_convex_upsample  flow [P, 2, h8, w8], mask [P, h8, w8, 576] (NHWC, already scaled) -> out [P, 2, 8 h8, 8 w8] (RAFT.upsample_flow)
 *   cwm_raft_head_project     hidden [M, 256] (NHWC rows: output_block.0's result, before its ReLU), weight [256], bias [1] -> value [M] =
 *                             bias + sum_c weight[c] relu(hidden[m, c]) in fp32 (output_block.1 and .2); 16-byte aligned hidden / weight
 *   cwm_raft_convex_upsample1 value [P, h8, w8], mask as above -> out [P, 1, 8 h8, 8 w8]: upsample_flow of a one-channel map */
CWM_API int cwm_raft_corr_lookup(const float* fmap1_dev, const float* fmap2_dev, const float* coords_dev, int P, int h8, int w8, float* out_dev,
                                 void* stream);
CWM_API int cwm_raft_convex_upsample(const float* flow_dev, const float* mask_dev, int P, int h8, int w8, float* out_dev, void* stream);
CWM_API int cwm_raft_head_project(const float* hidden_dev, const float* weight_dev, const float* bias_dev, int64_t M, float* value_dev, void* stream);
CWM_API int cwm_raft_convex_upsample1(const float* value_dev, const float* mask_dev, int P, int h8, int w8, float* out_dev, void* stream);

/* The correlation computed at lookup time (added after 0.10.4; the version string is unchanged).
 * replaces: `AlternateCorrBlock` (raft/corr.py:63-91; `args.alternate_corr`), whose CUDA extension `alt_cuda_corr` the reference does not ship.
 * A handle builds, per forward, either the all-pairs correlation volume and its three poolings (CorrBlock, corr.py:12-60: 4 * M * sum_l h_l * w_l bytes
 * for the M = batch * pairs * H/8 * W/8 low-resolution pixels of a call, about 5.3 * (H/8 * W/8)^2 bytes per pair) or only fmap2's three poolings
 * (1024 * batch * pairs * sum_{l>=1} h_l * w_l bytes), from which every iteration's lookup computes the correlations of the taps it reads: per level the
 * 256-long dot products of the 11 x 11 integer positions around the sample window, fp32 FMA in a fixed order, blended with the all-pairs lookup's taps and
 * weights.  Pooling is linear, so the two agree up to fp32 summation order (about 5e-6 on values of order 1); both are deterministic.  The on-the-fly form
 * costs 4 * 100 * 2 * 256 = 204.8 kFLOP per low-resolution pixel and iteration in place of 2 * 256 * H/8 * W/8 once: fewer above about 640 x 960 at 24
 * iterations, and the only form that fits when the volume does not.
 *   cwm_raft_set_corr         CWM_RAFT_CORR_ALL_PAIRS (the default) or CWM_RAFT_CORR_ON_THE_FLY for the forwards of this handle that follow, in either
 *                             arithmetic mode; the next forward re-plans the workspace when the value changed (the pyramid is not allocated on the fly).
 *                             Any other value: CWM_ERR_INVALID, and the handle keeps what it had.  Per handle because cwm_raft_forward_args is frozen.
 *   cwm_raft_workspace_bytes  the bytes of activation workspace the handle holds now (0 before the first forward): what its last plan asked for.
 *   cwm_raft_corr_lookup_on_the_fly  cwm_raft_corr_lookup (arguments, checks, output, synchronisation) from the feature maps alone: what it allocates
 *                             inside is fmap2's poolings, not P * (h8 * w8)^2 floats.  As there, h8 and w8 from 8 to 15 are accepted but leave level 3
 *                             with a side of 1, whose normalisation divides by side - 1 = 0: the 81 features of that level are then NaN (nothing is
 *                             read out of bounds).  cwm_raft_forward refuses such sizes; give both calls h8, w8 >= 16 for finite output. */
#define CWM_RAFT_CORR_ALL_PAIRS 0
#define CWM_RAFT_CORR_ON_THE_FLY 1
CWM_API int cwm_raft_set_corr(cwm_raft_model* m, int corr);
CWM_API int cwm_raft_workspace_bytes(cwm_raft_model* m, uint64_t* out);
CWM_API int cwm_raft_corr_lookup_on_the_fly(const float* fmap1_dev, const float* fmap2_dev, const float* coords_dev, int P, int h8, int w8, float* out_dev,
                                            void* stream);

/* The encoders once per distinct frame of a call (added after 0.10.4; the version string is unchanged).
 * replaces: the per-pair encoder passes of the reference's multi-frame loop (raft_model.py:276-300 calls the two-image forward, fnet on both images and
 * cnet on the first, for every pair), and of `predict_counterfactual_videos_and_flows` (segmentation.py:431), whose S predicted videos of one movie
 * all begin with the same frame 0.
 * A forward's two image sources already say which images repeat: two images are the same frame when their device address and their channel stride are
 * equal.  With sharing on, the forward recognises, from batch, pairs and the two sources' strides alone (on the host: no device read, no upload),
 *   P1  a source with stride_t == 0 and pairs > 1: one frame per batch row;
 *   P2  a source with stride_b == 0 and batch > 1: one frame for all rows;
 *   P3  two sources of identical strides with image2 = image1 + k * stride_t, k in {0, +1, -1}: one frame repeated, a movie (pairs + 1 frames per row
 *       in place of 2 * pairs), a movie whose pairs run backwards;
 * P1 and P2 per source, independently.  fnet then runs once per distinct frame and cnet once per distinct first image, and the correlation, the
 * lookup and the GRU's initial state find each pair's maps by frame.  Any other call (partial overlaps, a negative stride, different channel strides)
 * runs as with sharing off: 2 * batch * pairs fnet images and batch * pairs cnet images, launch for launch.  Images whose addresses differ are never
 * merged.  The GEMM plan of an encoder pass depends on its row count, so a shared forward agrees with an unshared one as the same pair does in batches
 * of different sizes (up to fp32 summation order), not bit for bit; the workspace is planned from the distinct counts and never grows.
 *   cwm_raft_set_share_frames  on = 1 / 0 (the default) for the forwards of this handle that follow.  Any other value: CWM_ERR_INVALID, and the handle
 *                              keeps what it had.  Per handle because cwm_raft_forward_args is frozen.
 *   cwm_raft_encoder_images    how many images the handle's last forward ran through fnet and through cnet; both 0 before the first forward. */
CWM_API int cwm_raft_set_share_frames(cwm_raft_model* m, int on);
CWM_API int cwm_raft_encoder_images(cwm_raft_model* m, int* fnet_images, int* cnet_images);

/* RAFT's forward interpolation on the device: a low-resolution flow carried along itself onto the next frame's grid, which is what the warm-start
 * protocol feeds to the next pair as `flow_init` (added after 0.10.4; the version string is unchanged).
 * replaces: `forward_interpolate` (raft/utils.py:28-56): a `.cpu().numpy()` copy and two scipy `griddata(..., method='nearest')` queries per field.
 * in:  P planar fields [2, h8, w8] (channel 0 = dx, 1 = dy, 1/8-resolution pixels), rows of w8 contiguous: element (c, y, x) of field p at
 *      flow_dev + p*stride_p + c*stride_c + y*w8 + x (strides in elements, of either sign).
 * out: out_dev [P, 2, h8, w8] contiguous.
 * Source pixel i = y0*w8 + x0 lands at x1 = x0 + dx[i], y1 = y0 + dy[i], summed in double (exact).  It is valid iff
 * x1 > 0 && x1 < w8 && y1 > 0 && y1 < h8, all four strict, so a NaN or infinite component is invalid.  Target (gx, gy) takes both channels of the valid
 * source with the smallest (gx - x1)^2 + (gy - y1)^2 in double; among equal distances the lowest i wins.  With no valid source the field is zeros (a
 * cold start; scipy returns NaN or raises there).  Brute force: h8*w8 <= 65536.  CWM_ERR_INVALID when out_dev overlaps what is read (every target
 * reads other pixels' sources), and for a null pointer, P < 1, h8 < 1 or w8 < 1.  No model handle; does not synchronise the stream. */
CWM_API int cwm_raft_forward_interpolate(const float* flow_dev, int64_t stride_p, int64_t stride_c, int P, int h8, int w8, float* out_dev, void* stream);

CWM_API const char* cwm_last_error(void);
/* "cwm_hip <version> gfx950" */
CWM_API const char* cwm_version(void);
/* Hash of the sources this library was built from (counterfactualworldmodels_amd/build.py: source_hash); the Python
 * binding compares it at load time so that a stale in-tree .so is rebuilt instead of silently bound. */
CWM_API const char* cwm_source_hash(void);
/* `HIP version ...; AMD clang version ...` of the hipcc that compiled this library.  The kernels carry hand-counted s_waitcnt instructions whose
 * correctness depends on the ISA the compiler emits around them; tools/asm_lds_lint.py checks that ISA and records the compiler it passed on
 * (csrc/LINT_PASSED.json), build.py and bench.py compare the two. */
CWM_API const char* cwm_compiler_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CWM_HIP_H */
