/*
 * cwm_hip_dev.h -- the development entry points of libcwm_hip_dev.so (built by `python -m counterfactualworldmodels_amd.build --dev`):
 * every object of libcwm_hip.so plus csrc/dev.hip.  For tools/ and for the tests that cross-check kernel variants bit for bit; the production
 * library exports none of this.
 */
#ifndef CWM_HIP_DEV_H
#define CWM_HIP_DEV_H

#include "cwm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tuning hook (tools/autotune_step.py): fix the output-tile configuration of every GEMM launch of one shape -- M, N, K as launched (K padded to
 * 64), epi 0 fp32 / 1 bf16+GELU / 2 bf16 / 3 QKV scatter, overlapped = inside a two-lane forward -- to cfg 1 (128x128), 4 (256x256 8-phase) or 6 (4 for
 * the whole rounds + 1 for the remaining rows); cfg 0 removes the entry, M <= 0 clears the table.  Every configuration gives bit-identical results,
 * except that a small launch on 128x128 tiles may split K (a re-associated, deterministic fp32 sum; "gemm_debug" 32 switches the split off).
 * The table is process-wide; it reaches the launches of this thread's stand-alone calls and of models created on this thread AFTER the first call. */
CWM_API int cwm_gemm_tile_override(int M, int N, int K, int epi, int overlapped, int cfg);

/* What the library decides before a GEMM launch of M x N x K (K a multiple of 64, N of 16; epi as above; mode CWM_MODE_*; overlapped = inside a two-lane
 * forward) under THIS THREAD's options (cwm_debug_set "gemm_tile", "gemm_debug" ..., cwm_gemm_tile_override): the tile configuration 1, 4 or 6 and, for each
 * of its one or two kernel launches, the rows, the kernel and the number of K ranges.  forced_cfg > 0 stands for a "gemm_tile" of that value; cus = the
 * compute units to plan for, 0: the current device's (256 without one).  Launches nothing and needs no device. */
#define CWM_DEV_GEMM_KERNEL_128 0     /* 128x128 tiles, 2-stage ring */
#define CWM_DEV_GEMM_KERNEL_DEEP128 1 /* 128x128 tiles, 4-stage ring (at most one tile per CU) */
#define CWM_DEV_GEMM_KERNEL_DEEP64 2  /* 64x128 tiles, 4-stage ring */
#define CWM_DEV_GEMM_KERNEL_8PHASE 3  /* 256x256 tiles, 8-phase main loop */
typedef struct cwm_dev_gemm_plan_out {
    int32_t cfg, nparts;
    struct {
        int32_t m_offset, M; /* rows [m_offset, m_offset + M) */
        int32_t kernel;      /* CWM_DEV_GEMM_KERNEL_* */
        int32_t splitk;      /* 1: K is not split */
    } part[2];               /* part[1] is zero when nparts is 1 */
} cwm_dev_gemm_plan_out;
CWM_API int cwm_dev_gemm_plan(int M, int N, int K, int epi, int mode, int overlapped, int forced_cfg, int cus, cwm_dev_gemm_plan_out* out);

/* Which kernel form each entry point that takes flow samples [B, C, H, W, S] would launch (csrc/flow_view.h: the same functions the entry points call): element
 * strides, sizes, the address of the flows and the entry point's other address -- cwm_flow_features: the output; cwm_flow_motion_sum: the work buffer (0: none) --,
 * and for cwm_flow_filter_stats the mask [B, 2 patches_per_frame, S]: its strides (b, patch, s) and its address.  CWM_DEV_FLOW_REFUSED where the entry point refuses the flows or
 * the layout (the filter's: C != 2, H != W ...; the checks of an entry point's other arguments are not part of this).  Launches nothing and needs no device. */
#define CWM_DEV_FLOW_REFUSED (-1)
#define CWM_DEV_FLOW_FEATURES_SCALAR 0
#define CWM_DEV_FLOW_FEATURES_VEC4 1    /* four samples per thread, 16-byte loads */
#define CWM_DEV_FLOW_MOTION_STRIDED 0
#define CWM_DEV_FLOW_MOTION_TILE 1      /* packed: magnitudes of a pixel tile in LDS */
#define CWM_DEV_FLOW_MOTION_ROWS16 2    /* packed: 16 / 32 / 64 lanes x 16 bytes own a pixel's samples (S = 64 / 128 / a multiple of 256) */
#define CWM_DEV_FLOW_MOTION_ROWS32 3
#define CWM_DEV_FLOW_MOTION_ROWS64 4
#define CWM_DEV_FLOW_COUNT_PLANES 0     /* also the strided form */
#define CWM_DEV_FLOW_COUNT_PLANES_VEC 1
#define CWM_DEV_FLOW_COUNT_PACKED 2
#define CWM_DEV_FLOW_COUNT_PACKED_VEC 3
#define CWM_DEV_FLOW_FINISH_V1 0
#define CWM_DEV_FLOW_FINISH_V4 1        /* the mask bytes of four samples per 32-bit load */
#define CWM_DEV_FLOW_ZERO_PLANES 0
#define CWM_DEV_FLOW_ZERO_PLANES_VEC 1
#define CWM_DEV_FLOW_ZERO_SCATTER 2
#define CWM_DEV_FLOW_PACK_TRANSPOSE 0
typedef struct cwm_dev_flow_forms_out {
    int32_t features, motion; /* cwm_flow_features, cwm_flow_motion_sum */
    int32_t count, finish;    /* cwm_flow_filter_stats: the counting pass and the finish kernel */
    int32_t zero, pack;       /* cwm_flow_filter_apply, cwm_flow_filter_pack */
} cwm_dev_flow_forms_out;
CWM_API int cwm_dev_flow_forms(const int64_t* strides, int B, int C, int H, int W, int S, uint64_t flows_addr, uint64_t aux_addr, int normalize_per_sample,
                               const int64_t* mask_strides, uint64_t mask_addr, int patches_per_frame, cwm_dev_flow_forms_out* out);

/* ---- diagnostics: single-kernel micro-benchmarks on random operands (tools/microbench.py) ---------
 * epi: 0 = fp32 out + bias + in-place residual (proj/fc2 form), 1 = bias + GELU -> bf16 (fc1 form),
 *      3 = QKV head scatter (N must be 3*64*heads, M = batch*n_tok with n_tok = M / batch).
 * Runs `iters` back-to-back launches after 3 warm-up launches and returns the mean launch time. */
CWM_API int cwm_bench_gemm(int M, int N, int K, int mode, int epi, int iters, double* avg_us);
CWM_API int cwm_bench_attention(int B, int H, int N, int mode, int iters, double* avg_us);
/* Sets one execution option (the keys of cwm_model_set_option, cwm_hip.h) in THIS THREAD's copy of the options: the stand-alone entry points
 * (cwm_linear, cwm_attention, cwm_bench_* ...) called on the thread afterwards use it, and model handles created on the thread afterwards start from it.
 * A model that already exists is changed with cwm_model_set_option / cwm_conj_set_option.  Also the profiling queries "attn_prof" / "gemm_prof"
 * (per-workgroup timers of builds with -DCWM_ATTN_PROF / -DCWM_GEMM_PROF), and
 * "pretend_device" = d: this thread's wrong-device checks (cwm_forward, cwm_conj_forward, cwm_*_load_weight, the collectives) see device d as current instead of
 * hipGetDevice's answer (-1: off) -- how the refusal is tested on a one-GPU box. */
CWM_API int cwm_debug_set(const char* key, int value);
/* The value of an option in this thread's copy (what a handle created on this thread now would start from). */
CWM_API int cwm_debug_get(const char* key, int* value);

/* ---- RAFT kernels one at a time (tests/test_raft_kernels_gpu.py) -------------------------------------------------------------------------------
 * The launches of csrc/raft_model.hip on caller-owned device buffers, with this thread's execution options (cwm_debug_set).  Activations are fp32
 * NHWC.  Every entry point synchronises the stream before it returns; none checks that the buffers are as large as the geometry says. */

/* One channel segment of a convolution input (kernels.h ConvSrc): pixel `pix` of the [n_img][H][W] grid at p + pix * ld, C channels.  The value read is
 * relu?((v - mean) * rstd) * sigmoid(gate[pix * gate_ld + c])?, with (mean, rstd) = stats[(img * C + c) * 2 ..]; or, with `coords` ([pix][2], C = 2),
 * coords - (x, y). */
typedef struct cwm_dev_conv_src {
    const float* p;
    int32_t ld, C;
    const float* stats; /* optional */
    int32_t relu;
    const float* gate;  /* optional */
    int32_t gate_ld;
    const float* coords; /* optional: instead of p */
} cwm_dev_conv_src;

/* One weight part [n][cin][kh][kw] with bias [n]; bn_gamma != NULL folds the eval-mode batch norm (gamma, beta, running mean, running var, each [n])
 * that follows the convolution, as the model does when it packs its weights. */
typedef struct cwm_dev_conv_part {
    const float* w;
    const float* b;
    int32_t n;
    const float *bn_gamma, *bn_beta, *bn_mean, *bn_var;
} cwm_dev_conv_part;

#define CWM_DEV_CONV_OPERAND_ONLY 1 /* stop after writing the A operand (no weights, no output needed) */
#define CWM_DEV_CONV_KEEP_OPERAND 2 /* do not write the operand: run the GEMM on `A` as it is (convc1 on the lookup's operand) */

/* One convolution as the RAFT model runs it: out[m][col0 + j] = bias[j] + sum_k A[m][k] W[j][k] over the rows m = (img, oy, ox) of the output grid
 * OH = (H + 2 pad_h - kh) / stride + 1 (OW likewise), K order (ky, kx, c), input channels = src[0] then src[1].  Output columns j < round_up(sum n, 16)
 * are written (those beyond sum n as 0), nothing else of a row of ldc floats. */
typedef struct cwm_dev_raft_conv_args {
    uint32_t struct_size;
    int32_t nsrc; /* 1 or 2; ignored with image[0] */
    cwm_dev_conv_src src[2];
    /* image[0] != NULL: the input frames instead of src (3 channels).  Image i of the call is pair (img0 + i) % P of frame (img0 + i) / P (0: image[0],
     * 1: image[1]), pair pr = (g, t) = (pr / ppg, pr % ppg), element (c, y, x) at image[f] + g * image_sb[f] + t * image_st[f] + c * image_sc[f] + y * W + x;
     * the value is 2 * (v * scale / 255) - 1 */
    const float* image[2];
    int64_t image_sb[2], image_st[2], image_sc[2];
    int32_t P, ppg;
    float scale;
    int32_t img0;
    int32_t n_img, H, W, kh, kw, stride, pad_h, pad_w;
    int32_t nparts; /* 1 or 2: the output channels are part[0]'s then part[1]'s (the GRU's stacked z and r) */
    cwm_dev_conv_part part[2];
    float bn_eps;
    float* out;
    int32_t ldc, col0;
    int32_t mode;       /* CWM_MODE_PARITY or CWM_MODE_FAST */
    int32_t c_lo, c_hi; /* c_hi > c_lo (multiples of 8): rewrite only input channels [c_lo, c_hi) of every tap; the rest of A is kept (needs `A`) */
    /* optional: the operand buffer, [n_img * OH * OW] rows of planes * Kpad bf16 (Kpad = round_up(kh * kw * cin, 64); planes 2 parity, 1 fast) in the
     * layout of csrc/common.h a_pos; NULL: allocated inside */
    void* A;
    int32_t flags; /* CWM_DEV_CONV_* */
    void* stream;
} cwm_dev_raft_conv_args;
CWM_API int cwm_dev_raft_conv(const cwm_dev_raft_conv_args* args);

/* cwm_raft_corr_lookup's pyramid and lookup, written as convc1's operand: [P * h8 * w8] rows of planes * 384 bf16 (features 0..323, then zeros) */
CWM_API int cwm_dev_raft_corr_lookup_operand(const float* fmap1_dev, const float* fmap2_dev, const float* coords_dev, int P, int h8, int w8, int mode,
                                             void* A_dev, void* stream);
/* the same operand from cwm_raft_corr_lookup_on_the_fly's form (AlternateCorrBlock, raft/corr.py:63-91): fmap2's poolings and the lookup that computes its taps */
CWM_API int cwm_dev_raft_corr_lookup_on_the_fly_operand(const float* fmap1_dev, const float* fmap2_dev, const float* coords_dev, int P, int h8, int w8, int mode,
                                                        void* A_dev, void* stream);
/* InstanceNorm2d statistics of x [n_img][HW][C]: stats [n_img][C][2] = (mean, 1 / sqrt(biased var + eps)) */
CWM_API int cwm_dev_raft_instnorm_stats(const float* x_dev, int n_img, int HW, int C, float eps, float* stats_dev, void* stream);
/* out[pix][c] = relu(X + Y) over Y->C channels, both read as a cwm_dev_conv_src (no gate / coords); out [n_img * HW][C] may be X->p */
CWM_API int cwm_dev_raft_residual_join(const cwm_dev_conv_src* X, const cwm_dev_conv_src* Y, int n_img, int HW, float* out_dev, void* stream);
/* cn [M][256] -> h [M][128] = tanh(cn[:, :128]), x[m * 256 + c] = relu(cn[:, 128:]) for c < 128 */
CWM_API int cwm_dev_raft_cnet_split(const float* cn_dev, int64_t M, float* h_dev, float* x_dev, void* stream);
/* ---- frames shared between the pairs of a forward (cwm_hip.h cwm_raft_set_share_frames; tests/test_raft_share_*.py) ----
 * cwm_dev_raft_frame_slots is the forward's frame plan made queryable, on the host alone (no GPU, nothing is read through the pointers): for the call
 * `args` describes (batch, pairs, the two image sources) and share = 0 / 1, pair p = b * pairs + t has its image1 at slot1[p] and its image2 at slot2[p]
 * of the n_fnet frames fnet runs on, and its context at cslot[p] of the n_cnet frames cnet runs on.  slot1 / slot2 / cslot: host arrays of
 * batch * max(pairs, 1) ints.
 * The four consumers of the encoders' maps, addressed by slot: the map of pair (g, t) = (p / ppg, p % ppg) lies g * sb + t * st maps past the operand's
 * pointer (sb = ppg, st = 1: one map per pair, the forms above).  None checks that the buffers reach as far as the strides say.
 *   cwm_dev_raft_corr_lookup_slots             cwm_raft_corr_lookup with fmap1 / fmap2 [frames, h8, w8, 256] addressed by (s1b, s1t) / (s2b, s2t)
 *   cwm_dev_raft_fmap_pool_slots               out [n_out, h / 2, w / 2, C] = avg_pool2d(2) of the input map at (j / nt) * in_sb + (j % nt) * in_st, j < n_out
 *   cwm_dev_raft_corr_lookup_on_the_fly_slots  the lookup of cwm_raft_corr_lookup_on_the_fly on the caller's four levels of fmap2 (an array of four device
 *                                              pointers, on the host): level 0 addressed by (s2b, s2t), the pooled levels by (s2pb, s2pt), fmap1 by (s1b, s1t)
 *   cwm_dev_raft_cnet_split_slots              cwm_dev_raft_cnet_split with cn [frames, hw8, 256] addressed by (sb, st); h and x stay per pair */
CWM_API int cwm_dev_raft_frame_slots(const cwm_raft_forward_args* args, int share, int* slot1, int* slot2, int* cslot, int* n_fnet, int* n_cnet);
CWM_API int cwm_dev_raft_corr_lookup_slots(const float* fmap1_dev, const float* fmap2_dev, const float* coords_dev, int P, int ppg, int h8, int w8, int64_t s1b,
                                           int64_t s1t, int64_t s2b, int64_t s2t, float* out_dev, void* stream);
CWM_API int cwm_dev_raft_fmap_pool_slots(const float* in_dev, int n_out, int nt, int64_t in_sb, int64_t in_st, int h, int w, int C, float* out_dev, void* stream);
CWM_API int cwm_dev_raft_corr_lookup_on_the_fly_slots(const float* fmap1_dev, const float* const* fmap2_levels_dev, const float* coords_dev, int P, int ppg, int h8,
                                                      int w8, int64_t s1b, int64_t s1t, int64_t s2b, int64_t s2t, int64_t s2pb, int64_t s2pt, float* out_dev,
                                                      void* stream);
CWM_API int cwm_dev_raft_cnet_split_slots(const float* cn_dev, int64_t M, int64_t hw8, int ppg, int64_t sb, int64_t st, float* h_dev, float* x_dev, void* stream);
/* x [M][256]: columns 128..253 -> relu, 254 / 255 = coords [M][2] - (x, y) of the pixel on the h8 x w8 grid */
CWM_API int cwm_dev_raft_motion_finish(float* x_dev, const float* coords_dev, int64_t M, int h8, int w8, void* stream);
/* h [M][128] = (1 - z) h + z tanh(q), z = sigmoid(zr[m * 256 + c]), q [M][128] */
CWM_API int cwm_dev_raft_gru_update(float* h_dev, const float* zr_dev, const float* q_dev, int64_t M, void* stream);
/* coords [M][2] += delta[m * ld + (0, 1)] */
CWM_API int cwm_dev_raft_flow_update(float* coords_dev, const float* delta_dev, int ld, int64_t M, void* stream);

/* ---- the operand gathers one launch at a time (tests/test_gather_kernels_gpu.py) ----------------------------------------------------------------
 * launch_patch_gather / launch_index_gather / launch_flow_rgb_gather / launch_imu_gather (csrc/kernels.h) on caller-owned device buffers; the
 * stream is synchronised before the call returns.  `out` is the GEMM A operand, [B * n_rows] rows of planes * ld bf16 in the layout of csrc/common.h
 * a_pos (planes 2 parity, 1 fast); the caller's buffers must be as large as the geometry says. */
#define CWM_DEV_GATHER_PATCH 0         /* reads perm */
#define CWM_DEV_GATHER_INDEX 1         /* reads mask; writes perm, rank (optional) and err_rows[B] = (visible count of the row != n_vis) */
#define CWM_DEV_GATHER_FLOW_RGB 2      /* reads perm; 7 channels [fwd x, fwd y, bwd x, bwd y, R, G, B] of one frame */
#define CWM_DEV_GATHER_IMU 3           /* reads perm; x = imu [B][C][L], token l = samples tubelet * l .. of every channel */
#define CWM_DEV_GATHER_INDEX_UNFUSED 4 /* what INDEX replaced: mask_to_perm, patch gather, perm_to_rank; err_rows[0] = (any row's count != n_vis) */
typedef struct cwm_dev_gather_args {
    uint32_t struct_size;
    int32_t kind; /* CWM_DEV_GATHER_* */
    int32_t mode; /* CWM_MODE_PARITY or CWM_MODE_FAST */
    int32_t normalize; /* imagenet-normalise the RGB channels in the kernel */
    const float* x; /* frames: element (b, c, t, y, x) at b * sb + c * sc + t * st + y * W + x (FLOW_RGB: one frame, st unused); IMU: the signal */
    int64_t sb, sc, st;
    const float *fwd, *bwd; /* FLOW_RGB: forward / backward flow, element (b, c, y, x) at b * f_sb + c * f_sc + y * W + x (b_sb, b_sc likewise) */
    int64_t f_sb, f_sc, b_sb, b_sc;
    int32_t B, C, H, W, P;
    int32_t L, tubelet; /* IMU */
    int32_t Nt;          /* real tokens per sample: permutation entries >= Nt are pad slots (zero rows) */
    int32_t n_rows;      /* rows gathered per sample */
    int32_t perm_stride; /* slots per row of mask / perm / rank; 0: Nt */
    int32_t n_vis;       /* INDEX, INDEX_UNFUSED: the visible count every mask row must have */
    const uint8_t* mask; /* INDEX, INDEX_UNFUSED: [B][slots], 0 = visible */
    int32_t* perm;       /* [B][slots] */
    int32_t* rank;       /* [B][slots] */
    int32_t* err_rows;   /* [B] */
    void* out;
    int32_t ld;
    void* stream;
} cwm_dev_gather_args;
CWM_API int cwm_dev_gather(const cwm_dev_gather_args* args);

/* The index prologue of a ragged batch (cwm_model_set_ragged; tests/test_ragged_kernels_gpu.py): args as above with kind INDEX or INDEX_UNFUSED, args->n_vis the
 * CAP of the rows' visible counts, n_vis_min the least count a row may have and counts_dev [B] (device) the rows' visible counts, written by the launch.
 *   INDEX          launch_index_gather(..., n_vis_min, counts): err_rows[b] = (count of row b outside [n_vis_min, n_vis]); operand rows [count, n_rows) of a sample are zeros
 *   INDEX_UNFUSED  what csrc/model.hip issues with "index_fused" = 0: memset of err_rows, launch_mask_to_perm_ragged, launch_patch_gather, launch_perm_to_rank;
 *                  err_rows[0] = (any row outside the range); operand rows [count, n_rows) are the tokens perm[count ..], i.e. masked ones (written, values unspecified)
 * Nothing of n_vis_min / counts_dev is checked here: the launchers' own refusals come back (before their launch; the unfused form's memset of err_rows has
 * been issued by then, as in the model). */
CWM_API int cwm_dev_gather_ragged(const cwm_dev_gather_args* args, int n_vis_min, int32_t* counts_dev);

/* ---- the conjoined predictor's attention and padding kernels one call at a time (tests/test_conj_kernels_gpu.py) -------------------------------
 * csrc/conj_kernels.hip (fp32 VALU forms, padding bookkeeping) and csrc/conj_attention.hip (MFMA forms) on caller-owned device buffers; the stream
 * is synchronised before a call returns.  Outputs named "operand" are rows of planes * width bf16 in the layout of csrc/common.h a_pos (planes 2
 * parity, 1 fast).  A shape that the chosen form's precondition rejects (cross_attention_mfma_ok / cross_attention_mfma_fits, cross_attention_ok,
 * small_attention_mfma_ok) comes back as an error before anything is launched or allocated: the outputs are untouched. */
#define CWM_DEV_CONJ_VALU 0 /* launch_cross_attention / launch_small_attention */
#define CWM_DEV_CONJ_MFMA 1 /* launch_cross_attention_mfma_roles / launch_small_attention_mfma */

/* `BidirectionalCrossAttention.forward` on the projected tensors, D = heads * head_dim: per head the first head_dim columns of the 2 * head_dim slice
 * of qk / qk_src give y = softmax_M(scale q1 k1^T) v_src, the second give y_src = softmax_N(scale q2_src k2^T) v.  The MFMA form reads qk and v in the
 * operand layout: the entry stages them itself (the common.h writers).  scores_t and partial are allocated inside. */
typedef struct cwm_dev_conj_cross_attention_args {
    uint32_t struct_size;
    int32_t mode;  /* CWM_MODE_PARITY or CWM_MODE_FAST */
    int32_t impl;  /* CWM_DEV_CONJ_* */
    int32_t roles; /* bit 0: the main-stream update (y), bit 1: the context update (y_src); MFMA: 1, 2 or 3 (both on `stream`), VALU: 3 */
    const float* qk;     /* [B * N][2 D] */
    const float* v;      /* [B * N][D] */
    const float* qk_src; /* [B * M][2 D] */
    const float* v_src;  /* [B * M][D] */
    int32_t B, N, M, heads, head_dim;
    float scale;
    void* y;     /* operand, [B * N] rows of width D */
    void* y_src; /* operand, [B * M] rows of width D */
    void* stream;
} cwm_dev_conj_cross_attention_args;
CWM_API int cwm_dev_conj_cross_attention(const cwm_dev_conj_cross_attention_args* args);

/* `Attention.forward` of the context stream on qkv [B * n_tok][3 * heads * head_dim] (bias added, q not yet scaled): o = softmax(q k^T / sqrt(head_dim)) v
 * in columns [0, heads * head_dim) of operand rows of width ldo (a multiple of 32, >= heads * head_dim); the other columns are not written. */
typedef struct cwm_dev_conj_small_attention_args {
    uint32_t struct_size;
    int32_t mode;
    int32_t impl; /* CWM_DEV_CONJ_*: VALU n_tok <= 64 and head_dim <= 64, MFMA n_tok <= 64 and head_dim 32 */
    const float* qkv;
    int32_t B, n_tok, heads, head_dim;
    void* o;
    int32_t ldo;
    void* stream;
} cwm_dev_conj_small_attention_args;
CWM_API int cwm_dev_conj_small_attention(const cwm_dev_conj_small_attention_args* args);

#define CWM_DEV_CONJ_PAD_MASK 0          /* ext_mask [B][N + P] = [mask [B][N] | pad slot j masked unless j < vmax - visible(b)] */
#define CWM_DEV_CONJ_FIX_PAD_ROWS 1      /* rows i of x [B * n_rows][D] with perm[b][i] >= n_real := token [D] */
#define CWM_DEV_CONJ_ZERO_PAD_OUT_ROWS 2 /* rows j of x [B * n_rows][D] with perm[b][n_vis + j] >= n_real := 0 */
#define CWM_DEV_CONJ_IMU_APPEND_DUMMY 3  /* out [B][C][L + T] = [imu [B][C][L] | dummy [C][T]], ext_mask [B][N + 1] = [mask [B][N] | 0] */
typedef struct cwm_dev_conj_pad_args {
    uint32_t struct_size;
    int32_t kind; /* CWM_DEV_CONJ_PAD_* .. CWM_DEV_CONJ_IMU_APPEND_DUMMY */
    int32_t B;
    const uint8_t* mask; /* PAD_MASK, IMU_APPEND_DUMMY: [B][N], non-zero = masked */
    int32_t N, P, vmax;
    uint8_t* ext_mask;
    float* x;            /* FIX_PAD_ROWS, ZERO_PAD_OUT_ROWS */
    const int32_t* perm; /* [B][perm_stride] */
    int32_t perm_stride, n_rows, n_vis, n_real, D;
    const float* token;
    const float* imu;    /* IMU_APPEND_DUMMY */
    const float* dummy;
    int32_t C, L, T;
    float* out;
    void* stream;
} cwm_dev_conj_pad_args;
CWM_API int cwm_dev_conj_pad(const cwm_dev_conj_pad_args* args);

/* ---- the ViT engine's own launch forms one at a time (tests/test_engine_kernels_gpu.py) -----------------------------------------------------------
 * launch_gemm / launch_attention / launch_layernorm / launch_fill_mask_tokens (csrc/kernels.h) with the parameters only csrc/engine.hip builds -- row
 * maps, the Q/K/V scatter, a query window, mapped LayerNorm rows -- on caller-owned device buffers, with this thread's execution options; the stream
 * is synchronised before a call returns.  "Operand" buffers are rows of planes * width bf16 in the layout of csrc/common.h a_pos (planes 2 parity, 1
 * fast).  What the launchers refuse (and what the checks named below refuse) comes back as an error before anything is launched; none of the entry
 * points checks that the buffers are as large as the geometry says. */

/* One GEMM out = a w^T + bias through launch_gemm: a [M][K], w [N][K], bias [N] (optional) are fp32 and staged exactly as cwm_linear stages them (K
 * zero-padded to a multiple of 64, the weight packed by the engine's packer); everything else is csrc/kernels.h GemmParams as it stands:
 *   rows: rows_in == 0: identity.  Else row m = b * rows_in + i -> out row b * rows_out + i + out_row_offset; residual row = resid_rowmap ?
 *         resid_rowmap[b * map_stride + i] : the out row.  (Needs M % rows_in == 0 and i + out_row_offset < rows_out.)
 *   epi 0: C[out row][0..N) (row stride ldc) = acc + bias (+ resid[residual row][..], row stride ldr; resid may be C itself)
 *   epi 1 / 2: out[out row][0..N) (operand, width ldo) = split(gelu(acc + bias)) / split(acc + bias)
 *   epi 3: N = 3 * heads * head_dim, rows_in = n_tok: column c = which * D + h * head_dim + d of row (b, tok) -> {q_out, k_out, v_out}[which]
 *          [(b * heads + h) * n_tok + tok][d], Q times q_scale; the lo plane lies qk_plane elements behind the hi plane (parity mode only) */
typedef struct cwm_dev_gemm_args {
    uint32_t struct_size;
    int32_t mode; /* CWM_MODE_PARITY or CWM_MODE_FAST */
    int32_t epi;  /* 0 .. 3, as for cwm_gemm_tile_override */
    const float* a;
    const float* w;
    const float* bias; /* optional */
    int32_t M, N, K;
    int32_t rows_in, rows_out, out_row_offset, map_stride;
    const int32_t* resid_rowmap; /* optional: [M / rows_in][map_stride] */
    float* C;
    int32_t ldc;
    const float* resid; /* optional */
    int32_t ldr;
    void* out;
    int32_t ldo;
    void *q_out, *k_out, *v_out;
    int64_t qk_plane;
    int32_t heads, head_dim, n_tok;
    float q_scale;
    int32_t* plan_forms; /* optional, host: [2] = the epilogue form gemm_plan chose for THIS launch (staged, direct) */
    void* stream;
} cwm_dev_gemm_args;
CWM_API int cwm_dev_gemm(const cwm_dev_gemm_args* args);

/* Self-attention of head_dim 64 over the queries [q_off, q_off + n_q) of every sample (n_q == 0: all N): qkv [B][N][3 * H * 64] fp32 is scattered to
 * Q (times 0.125), K, V as cwm_attention does, then launch_attention writes O as an operand of [B * (n_q ? n_q : N)] rows of width ldo (>= 64 H; a multiple
 * of 32 in parity mode, of 4 in fast mode), head h at columns 64 h ..; other rows and columns of `o` are not written. */
typedef struct cwm_dev_attention_args {
    uint32_t struct_size;
    int32_t mode;
    const float* qkv;
    int32_t B, N, H, q_off, n_q;
    void* o;
    int32_t ldo;
    void* stream;
} cwm_dev_attention_args;
CWM_API int cwm_dev_attention(const cwm_dev_attention_args* args);
/* The same launch with a key count per batch row, as the encoder blocks of a ragged batch issue it (AttnParams.key_len, device [B]; Engine::run_block):
 * sample b attends to keys [0, key_len[b]) and only its O rows [0, key_len[b]) are written -- in place, into whatever `o` holds (the engine: LN1's rows);
 * a length outside [1, N] writes nothing for that sample.  A query window (n_q > 0) together with key_len is refused before anything is launched. */
CWM_API int cwm_dev_attention_ragged(const cwm_dev_attention_args* args, const int32_t* key_len_dev);

/* LayerNorm of `rows` rows of D columns: output row r reads input row (r / rows_out_per_b) * rows_in_per_b + in_offset + r % rows_out_per_b of x (row
 * stride ldx; rows_out_per_b == 0: row r) and writes row r of the operand `out` (width ldo >= D: a multiple of 32 in parity mode, of 8 in fast mode;
 * columns >= D are not written) and, if given, of out_f32 [rows][D]. */
typedef struct cwm_dev_layernorm_args {
    uint32_t struct_size;
    int32_t mode;
    const float* x;
    int32_t ldx;
    const float* gamma;
    const float* beta;
    float eps;
    int32_t D, rows, rows_out_per_b, rows_in_per_b, in_offset;
    void* out;
    int32_t ldo;
    float* out_f32; /* optional */
    void* stream;
} cwm_dev_layernorm_args;
CWM_API int cwm_dev_layernorm(const cwm_dev_layernorm_args* args);

/* x_full [B][Nt][D]: rows n_vis .. Nt - 1 of every sample = mask_token [D] + pos[perm[b][row]] (pos rows of D floats, perm [B][Nt]); D a multiple of 4 */
CWM_API int cwm_dev_fill_mask_tokens(float* x_full_dev, const float* mask_token_dev, const float* pos_dev, const int32_t* perm_dev, int B, int Nt, int n_vis,
                                     int D, void* stream);
/* launch_fill_mask_tokens_ragged: the same for rows [counts[b], Nt) of sample b (counts device [B], every one >= n_vis_min > 0); rows [0, counts[b]) are not
 * written, whatever n_vis_min.  n_vis_min == Nt launches nothing. */
CWM_API int cwm_dev_fill_mask_tokens_ragged(float* x_full_dev, const float* mask_token_dev, const float* pos_dev, const int32_t* perm_dev,
                                            const int32_t* counts_dev, int B, int Nt, int n_vis_min, int D, void* stream);

/* cwm_unembed (cwm_hip.h) on frames addressed as the engine addresses them: element (b, t, c, y, x) of x at b x_stride_b + t x_stride_t + c x_stride_c + y W + x
 * (rows and pixels contiguous; x_stride_c >= H W).  mask -> permutation -> rank -> launch_unembed: out [B,T,C,H,W] contiguous = y at masked patches, x at visible
 * ones.  C == 3 with 16-byte aligned x / y / out and strides that are multiples of 4 takes the three-channel kernel, everything else the generic one.
 * CWM_ERR_MASK if a row does not have n_vis visible tokens. */
CWM_API int cwm_dev_unembed(const float* y_tokens_dev, const float* x_dev, int64_t x_stride_b, int64_t x_stride_c, int64_t x_stride_t, const uint8_t* mask_dev,
                            int B, int T, int C, int H, int W, int P, int n_vis, float* out_dev, void* stream);
/* The un-embed of a ragged batch (csrc/model.hip forward_lane): rows of n_vis_min .. n_vis visible tokens, y_tokens [B][Nt - n_vis_min][P*P*C] with row j of every
 * sample = decoder row n_vis_min + j, so a sample's own predictions are its LAST Nt - count rows.  mask -> permutation (launch_mask_to_perm_ragged) -> rank ->
 * launch_unembed with n_vis = n_vis_min, Nm = Nt - n_vis_min.  CWM_ERR_MASK if a row's count is outside [n_vis_min, n_vis] (out_dev is written all the same). */
CWM_API int cwm_dev_unembed_ragged(const float* y_tokens_dev, const float* x_dev, int64_t x_stride_b, int64_t x_stride_c, int64_t x_stride_t, const uint8_t* mask_dev,
                                   int B, int T, int C, int H, int W, int P, int n_vis_min, int n_vis, float* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CWM_HIP_DEV_H */
