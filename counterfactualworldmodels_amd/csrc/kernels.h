// Internal launch interfaces of the HIP kernels (not part of the C ABI; see include/cwm_hip.h).
#pragma once
#include "common.h"

struct cwm_patch_error_args;  // include/cwm_hip.h

namespace cwm {

// Execution options of one model handle (cwm_model_set_option / cwm_conj_set_option) -- every switch that was a process-wide global of the library
// until round 4.  The defaults are the measured best; the other values exist for same-box A/B measurements and for the bitwise cross-checks of the
// test suite.  A launch reads them through its parameter struct (GemmParams.tune, AttnParams.tune; nullptr = the defaults), a forward through its
// Engine -- never from a global, so two models in one process cannot change each other's kernels.
struct Tuning {
    int gemm_tile = 0;     // 0 automatic per shape (gemm_plan), 1: 128x128, 4: 256x256 8-phase, 6: 8-phase rounds + 128x128 remainder rows
    int gemm_debug = 0;    // bit mask of ablations / A-B switches: 1 skip the epilogue's global stores, 2 skip the epilogue, 4 no 4-stage ring for small launches,
                           // 8 skip every LayerNorm launch (timing only), 32 no split-K, 128 the one-lane tile choice also inside a two-lane call, 256 small launches keep
                           // 128-row tiles where the default takes 64x128 ones, 512 bf16-output GEMMs with K < 512 stay on 128x128 tiles, 1024 no half-width column tiles in the
                           // 8-phase kernel (and N = 384 back on 128x128 tiles), 2048 no half-height row tiles in the 8-phase kernel (a ragged last row tile of at most
                           // 128 rows runs as a full tile)
    int gemm_staged = 1;   // 0: the per-fragment epilogue of round 1 everywhere (it stays the fallback for unaligned widths)
    int gemm_direct = 1;   // 1: bf16-output epilogues store 16 bytes per lane straight from the accumulators; 2: the fp32-output ones too; 0: LDS-staged everywhere
    int attn_kernel = 0;   // 0 automatic, 1: 4-wave kernel (attention.hip), 3: software-pipelined kernel (attention_pipe.hip)
    int attn_remap = 1;    // 0: plain workgroup order instead of one XCD per (batch, head) with the ragged query tiles last
    int attn_tail = 1;     // 0: the regular schedule also for a ragged last query tile of <= 32 rows (attention_tail.h)
    int attn_ksplit = 1;   // 0: a nearly empty last round of workgroups runs its items whole instead of cutting them into key ranges
    int index_fused = 1;       // 0: the index prologue as the four launches of rounds 1-4 (memset, mask_to_perm, patch_gather, perm_to_rank) instead of one
    int prune_last_block = 1;  // 0: the last decoder block runs over all tokens
    int mask_token_tables = 1; // 0: decoder block 0 runs LN1 and the Q/K/V projection over the mask-token rows too instead of copying them from the per-position table
    int min_lane_rows = 0;     // encoder rows per half batch from which a forward splits into two lanes; 0: the model family's default (engine.h)
    int conj_ctx_stream = 1;   // 0: the IMU-conditioned model's context stream on the lane's own stream
    int conj_attn = 1;         // 0: the fp32 VALU cross / context attention kernels instead of the MFMA ones
    // development library only (csrc/dev.hip, cwm_gemm_tile_override): per-shape tile configuration, 0 = no opinion
    int (*tile_hook)(int M, int N, int K, int epi, int overlapped) = nullptr;
};
const Tuning& default_tuning();
// What the stand-alone entry points (cwm_linear, cwm_attention ...) use and what a new model handle starts from: the defaults, unless the
// development library's cwm_debug_set changed this THREAD's copy (libcwm_hip.so exports no way to)
Tuning& thread_tuning();
int tuning_set(Tuning& t, const char* key, int value);  // 0, or -1 for an unknown key
int tuning_set_production(Tuning& t, const char* key, int value);  // the production setters: -2 for the timing-only ablation bits of "gemm_debug" (engine.hip)
int tuning_get(const Tuning& t, const char* key, int* value);

enum GemmEpilogue : int {
    EPI_F32 = 0,        // C = acc + bias (+ resid[rowmap])            fp32 out
    EPI_BF16_GELU = 1,  // out = split_bf16(gelu_erf(acc + bias))      bf16 plane(s) out
    EPI_BF16 = 2,       // out = split_bf16(acc + bias)                bf16 plane(s) out
    EPI_QKV = 3,        // per-head scatter: Q (scaled), K, V -> [B*H,N,hd]
};

struct GemmParams {
    // operands (bf16, K-contiguous) in the A-operand layout of the mode (common.h a_pos): fast A[M][lda], W[Npad][K];
    // parity A[M][2*lda], W[Npad][2*K] with hi/lo interleaved per 32-k block.  lda / K are LOGICAL k counts.
    const bf16* A;
    const bf16* W;
    int lda;
    int M, N, K;
    int m_offset;       // this launch covers rows [m_offset, m_offset + M) of the problem (the parts of gemm_plan's mixed-tile split); usually 0
    const float* bias;  // [N] or nullptr
    int epi;
    // row mapping (rows_in == 0: identity).  m = b*rows_in + i  ->  out row b*rows_out + i,
    // residual row = resid_rowmap ? resid_rowmap[b*map_stride + i] : out row
    int rows_in, rows_out, map_stride;
    int out_row_offset;  // added to the out row (and to the default residual row): writes a per-sample row block (last decoder block)
    const int* resid_rowmap;
    // EPI_F32
    float* C;
    int ldc;
    const float* resid;
    int ldr;
    // EPI_BF16*
    bf16* out_hi;
    int64_t out_plane;
    int ldo;
    // EPI_QKV
    bf16* q_out;
    bf16* k_out;
    bf16* v_out;
    int64_t qk_plane;
    int qkv_dim, heads, head_dim, n_tok;
    float q_scale;
    // split-K of the latency-bound small launches (gemm.hip, deep-ring kernels).  The workspace is the launching stream's, attached by whoever plans the
    // launch (Engine::run_gemm: the engine's own; launch_gemm: the process-wide table) when a part of the plan splits K
    int splitk;              // set by launch_gemm_part from the plan: K is cut into this many ranges, one workgroup each (1: off)
    float* sk2_slabs;        // [tiles * splitk][128 * 128] fp32 partial accumulators
    unsigned* sk2_count;     // [tiles] arrival counters (0 between launches)
    int staged;  // set by launch_gemm_part from the plan: epilogue through LDS with full-line global accesses (gemm.hip)
    int direct;  // set by launch_gemm_part from the plan: 16-byte stores straight from the accumulators, W tile staged with permuted rows (gemm_device.h epilogue_direct)
    int overlapped;  // set by the engine: the launch runs beside another lane's kernels, so a partly filled last round of workgroups is not lost
    int debug;  // set by launch_gemm_part from tune->gemm_debug (the kernels read bits 0 / 1: skip the epilogue's global stores / the epilogue)
    const Tuning* tune;  // execution options of the calling model (nullptr: defaults)
};

// The EPI_QKV fields of a launch, written here and nowhere else: samples of n_in rows (the first n_in of n_tok tokens each) scattered per head into
// q / k / v [B * heads][n_tok][head_dim], Q times head_dim^-0.5.  (With a LinearW: engine.h qkv_gemm.)
inline void set_qkv_epilogue(GemmParams& p, int n_in, int n_tok, int D, int head_dim, bf16* q, bf16* k, bf16* v, int64_t qk_plane) {
    p.epi = EPI_QKV;
    p.rows_in = n_in; p.rows_out = n_tok; p.map_stride = n_tok;
    p.q_out = q; p.k_out = k; p.v_out = v;
    p.qk_plane = qk_plane;
    p.qkv_dim = D; p.heads = D / head_dim; p.head_dim = head_dim; p.n_tok = n_tok;
    p.q_scale = 1.0f / sqrtf((float)head_dim);
}

constexpr int kSplitKSlots = 512;  // >= CUs: a split launch has at most one part per CU
int splitk_workspace_alloc(float** slabs, unsigned** counts, hipStream_t stream);  // counters zeroed on `stream`
// Everything decided before a GEMM launch, by gemm_plan and nowhere else; launch_gemm_part turns part i into one kernel launch.
enum GemmKernel : int {
    GEMM_KERNEL_128 = 0,      // 128x128 tiles, 2-stage ring, two workgroups per CU
    GEMM_KERNEL_DEEP128 = 1,  // 128x128 tiles, 4-stage ring: at most one tile per CU; may split K
    GEMM_KERNEL_DEEP64 = 2,   // 64x128 tiles, 4-stage ring: at most half a 128-row tile per CU; may split K
    GEMM_KERNEL_8PHASE = 3,   // 256x256 tiles, 8-phase main loop
};
struct GemmPlan {
    int cfg;     // the tile configuration in the vocabulary of Tuning.gemm_tile: 1, 4, or 6 (two parts: 8-phase rounds, then the remaining rows)
    int nparts;  // 1 or 2
    struct Part {
        int m_offset, M;  // rows [m_offset, m_offset + M) of the problem
        int kernel;       // GemmKernel
        int splitk;       // K ranges (1: no split-K; more only on the deep-ring kernels)
    } part[2];
    int staged, direct;  // epilogue form (GemmParams)
    bool splits_k() const { return part[0].splitk > 1 || (nparts == 2 && part[1].splitk > 1); }
};
// Checks the arguments and fills `plan` for a device of `cus` compute units; forced_cfg > 0 replaces the options' and the rule's tile choice.  No HIP call.
int gemm_plan(const GemmParams& p, int planes, int forced_cfg, int cus, GemmPlan* plan);
// One kernel launch: part i of the plan made from `p`.  A part that splits K needs p.sk2_slabs / p.sk2_count.
int launch_gemm_part(const GemmParams& p, int planes, const GemmPlan& plan, int i, hipStream_t stream);
// Plan + launch for callers outside an engine (cwm_linear, the development entry points); split-K workspace from a process-wide per-(device, stream) table
int launch_gemm(const GemmParams& p, int planes, hipStream_t stream);
int gemm_cu_count();  // compute units of the current device, rounded down to a multiple of the 8 XCDs (256 on MI355X)
int gemm_prof_dump();  // builds with -DCWM_GEMM_PROF: per-workgroup timers of gemm8p_kernel -> /tmp/gemm_blocks.bin

struct AttnParams {
    const bf16* q;   // [planes][B*H][N][64]   (q pre-scaled by hd^-0.5)
    const bf16* k;   // [planes][B*H][N][64]
    const bf16* v;   // [planes][B*H][N][64]  (row-major like K; transposed on the LDS read)
    int64_t qk_plane;
    bf16* o;         // [planes][B*N][ldo]  (head h at columns h*64..)
    int64_t o_plane;
    int ldo;
    int n_tok, heads, batch;
    int remap;       // set by launch_attention: XCD-aware workgroup -> (query tile, head) mapping (attention_device.h; "attn_remap" switch)
    int q_off, n_q;  // queries = rows [q_off, q_off + n_q) of every (batch, head); n_q == 0: all n_tok.  O rows are b * n_q + (q - q_off)
    // key-split tail round (attention_pipe.hip, "attn_ksplit" switch), set by launch_attention_pipe: work items [0, ks_main) run whole; each of the
    // remaining items is cut into ks_parts key ranges, one workgroup each, which leave (O^T unnormalised, max, sum) in ks_scratch for
    // attention_combine_kernel.  ks_parts == 0: off
    int ks_main, ks_parts, ks_nqb;
    float* ks_scratch;  // [items - ks_main][ks_parts][128 queries][68]: O[64], max, sum, -, -
    int tail_split;  // set by launch_attention: a ragged last query tile of at most 32 rows splits the KEYS over its four waves (attention_tail.h; "attn_tail" switch)
    const Tuning* tune;  // execution options of the calling model (nullptr: defaults)
    // Ragged batches (device, one entry per batch row; nullptr: every row attends to all n_tok keys -- the launch of every caller before it existed).
    // Batch row b attends to keys [0, key_len[b]); n_tok stays the row stride and the capacity.  Query rows at and past key_len[b] are not written.
    // A length outside [1, n_tok] makes the row's workgroups exit without a store.  Needs n_q == 0; runs the regular schedule (no key-split tail tile,
    // no key-split last round: DESIGN.md section 8.14).  Last member, so that the offsets of the fields above are those of the rectangular launch.
    const int* key_len;
};

// Attention over all N tokens of B * H (batch, head) pairs, O rows of ldo columns; q_off / n_q (a query window), key_len and tune are the caller's to set
inline AttnParams attn_dense(const bf16* q, const bf16* k, const bf16* v, int64_t qk_plane, bf16* o, int64_t o_plane, int ldo, int B, int H, int N) {
    AttnParams a = {};
    a.q = q; a.k = k; a.v = v; a.qk_plane = qk_plane;
    a.o = o; a.o_plane = o_plane; a.ldo = ldo;
    a.n_tok = N; a.heads = H; a.batch = B;
    return a;
}

int launch_attention(const AttnParams& p, int planes, hipStream_t stream);
int attention_pipe_prof(int i);  // per-phase s_memtime totals of block 0 wave 0 (builds with -DCWM_ATTN_PROF only)
int launch_attention_pipe(const AttnParams& p, int planes, hipStream_t stream);  // attention_pipe.hip; arguments checked by launch_attention

struct LayerNormParams {
    const float* x;  // rows of length D, row stride ldx
    int ldx;
    const float* gamma;
    const float* beta;
    float eps;
    int D;
    int rows;        // number of output rows
    // input row for output row r: (r / rows_out_per_b) * rows_in_per_b + in_offset + (r % rows_out_per_b)
    // (rows_out_per_b == 0: identity)
    int rows_out_per_b, rows_in_per_b, in_offset;
    bf16* out;       // [planes][rows][ldo]
    int64_t out_plane;
    int ldo;
    float* out_f32;  // optional fp32 copy of the normalised rows ([rows][D]); may be nullptr
};

// `rows` rows of D columns into out [planes][rows][ldo]; rows_out_per_b > 0: the per-sample row window of the struct (the other two are not read without it)
inline LayerNormParams layernorm_rows(const float* x, int ldx, int D, const float* gamma, const float* beta, float eps, int rows, bf16* out, int ldo,
                                      int rows_out_per_b = 0, int rows_in_per_b = 0, int in_offset = 0) {
    LayerNormParams p = {};
    p.x = x; p.ldx = ldx; p.gamma = gamma; p.beta = beta; p.eps = eps; p.D = D; p.rows = rows;
    p.rows_out_per_b = rows_out_per_b; p.rows_in_per_b = rows_in_per_b; p.in_offset = in_offset;
    p.out = out; p.out_plane = (int64_t)rows * ldo; p.ldo = ldo;
    return p;
}

int launch_layernorm(const LayerNormParams& p, int planes, hipStream_t stream);

// mask[B,Nt] (1 = masked) -> perm[B,Nt] = [visible tokens ascending | masked tokens ascending];
// err[0] is set to 1 if any row's visible count != n_vis.
// Ragged batches (n_vis_min > 0): err[0] is set for a row of fewer than n_vis_min or more than n_vis visible tokens, counts[b] = the row's visible count
int launch_mask_to_perm(const uint8_t* mask, int B, int Nt, int n_vis, int* perm, int* err, hipStream_t stream, int n_vis_min = 0, int* counts = nullptr);
// RectangularizeMasks on device masks (elementwise.hip): masked count per row; apply the host's picks [R | rows | offsets | to_value | picks] in place
int launch_mask_row_counts(const uint8_t* mask, int B, int Nt, int* counts, hipStream_t stream);
int launch_mask_flip_picks(uint8_t* mask, int B, int Nt, const int* table, int n_rows, hipStream_t stream);  // table rows outside [0, B) are skipped

struct PatchGatherParams {
    const float* x;  // frames; element (b,c,t,y,x) at b*sb + c*sc + t*st + y*W + x
    int64_t sb, sc, st;
    int normalize;   // apply (x - mean_c)/std_c in-kernel (prediction.py:309-310)
    int C, H, W, P;
    const int* perm; // [B][perm_stride]
    int Nt, n_rows;  // real tokens per sample; rows per sample to gather (= n_vis)
    int perm_stride; // 0 = Nt; padded predictors: Nt + max_padding_tokens (entries >= Nt are pad slots)
    int B;
    bf16* out;       // [planes][B*n_rows][ld]  patch vector order (c, ph, pw), zero-padded to ld
    int64_t out_plane;
    int ld;
};

int launch_patch_gather(const PatchGatherParams& p, int planes, hipStream_t stream);

// The 7-channel `FlowBackRGB01` tubelet gather of the flow -> IMU predictor (elementwise.hip flow_rgb_gather_kernel):
// K order (c, ph, pw) over c = [fwd x, fwd y, bwd x, bwd y, R, G, B], flow scaled by 2/W (x) and 2/H (y), RGB as patch_gather.
struct FlowRgbGatherParams {
    const float* fwd;  // forward flow, element (b,c,y,x) at b*f_sb + c*f_sc + y*W + x
    const float* bwd;  // backward flow, the same with b_sb / b_sc
    int64_t f_sb, f_sc, b_sb, b_sc;
    const float* x;    // frame 1, element (b,c,y,x) at b*sb + c*sc + y*W + x
    int64_t sb, sc;
    int normalize;     // imagenet-normalise the RGB channels in-kernel
    int H, W, P;
    const int* perm;   // [B][perm_stride]; entries >= Nt are pad slots (zero rows)
    int Nt, n_rows, perm_stride, B;
    bf16* out;         // [planes][B*n_rows][ld], zero-padded to ld
    int64_t out_plane;
    int ld;
};
int launch_flow_rgb_gather(const FlowRgbGatherParams& p, int planes, hipStream_t stream);
// mask[B][L] (L = perm_stride or Nt) -> perm[B][L], rank[B][L] (inverse; may be nullptr), err_rows[b] = (visible count of row b != n_vis), and the
// gather of the first n_rows visible tokens of every sample, in one launch (elementwise.hip index_gather_kernel); p.perm is not read
// Ragged batches (n_vis_min > 0): err_rows[b] = (count outside [n_vis_min, n_vis]), counts[b] = the row's visible count; rows behind it are gathered as zeros
int launch_index_gather(const PatchGatherParams& p, const uint8_t* mask, int n_vis, int* perm, int* rank, int* err_rows, int planes, hipStream_t stream,
                        int n_vis_min = 0, int* counts = nullptr);

// x_full[b][n_vis + j][:] = mask_token + pos[perm[b][n_vis + j]]   (vmae.py:556-557)
// counts != nullptr (ragged batches): the same for rows [counts[b], Nt) of sample b (counts[b] >= n_vis_min > 0; rows below n_vis_min are never touched, n_vis is not read)
int launch_fill_mask_tokens(float* x_full, const float* mask_token, const float* pos, const int* perm, int B, int Nt, int n_vis, int D, hipStream_t stream,
                            const int* counts = nullptr, int n_vis_min = 0);

// Decoder block 0's Q / K / V rows of the mask tokens, copied from the per-position table (engine.hip Engine::dec0_table):
// {q, k, v}[pl * qk_plane + ((b * H + h) * Nt + j) * 64 ..] = tab[(which * planes + pl) * Nt * H * 64 + (h * Nt + perm[b * Nt + j]) * 64 ..] for j in [n_vis, Nt),
// planes = 1 (fast: hi only) or 2 (hi, lo).  16-byte copies; a perm entry outside [0, Nt) is clamped.
int launch_dec0_gather(const bf16* tab, const int* perm, bf16* q, bf16* k, bf16* v, int64_t qk_plane, int B, int Nt, int n_vis, int H, int planes, hipStream_t stream);
// perm[i] = i for i < n (the table's own rows are the token positions in order)
int launch_iota(int* perm, int n, hipStream_t stream);

struct UnembedParams {
    const float* y;  // [B][Nm][P*P*C], feature order (ph, pw, c)
    const float* x;  // raw frames, element (b,t,c,y,x) at b*sb + t*st + c*sc + y*W + x
    int64_t sb, sc, st;
    const uint8_t* mask;  // [B][Nt]
    const int* rank;      // [B][Nt]: position of token tau in perm (>= n_vis for masked tokens)
    int B, T, C, H, W, P, n_vis, Nm;
    float* out;           // [B][T][C][H][W] contiguous
};

int launch_unembed(const UnembedParams& p, hipStream_t stream);

// The geometry every token read-out shares (readout.hip, unmask.hip, segment.hip): a batch of T frames of C x H x W pixels cut into P x P patches, n_vis visible
// tokens per row and Nm = Nt - n_vis predicted ones, and the frame that is read.  patch_grid_of is the only place that derives Nm; check_patch_grid is the only
// statement of what a geometry must satisfy.  It always checks batch, T, P, H and W; `needs` names what else the caller reads.  Messages start with `who`,
// which ends in the prefix of the field names ("cwm_segment_step: base." gives "cwm_segment_step: base.P = 5, ...").
struct PatchGrid {
    int B, T, C, H, W, P;  // C <= 8, P in {4, 8, 16}
    int n_vis, Nm;         // Nm = Nt - n_vis rows of y per sample; the row index is clamped into [0, Nm)
    int frame;
};
enum : unsigned {
    kGridChannels = 1,   // 1 <= C <= 8
    kGridTokens = 2,     // 0 <= n_vis <= Nt and Nm = Nt - n_vis
    kGridFrame = 4,      // 0 <= frame < T
    kGridFrameEach = 8,  // the same, or -1: each frame against its own
};
PatchGrid patch_grid_of(const cwm_patch_error_args& a);
int check_patch_grid(const char* who, const PatchGrid& g, unsigned needs);  // 0 or CWM_ERR_INVALID with a message that names the field

// Per-patch squared error of the prediction against target frames, from the predicted tokens (readout.hip patch_error_map_kernel):
// map[b][t][i][j] = (1 / P^2) sum_{pixels of patch (i,j)} sum_c (pred_f - target_t)^2, pred_f = frame f of what launch_unembed would build (f = frame, or t when
// frame < 0); mean[b] = sum(map * region) / max(sum(region), 1).  No allocation, no synchronisation, no atomics: two calls on the same inputs are bit-equal.
struct PatchErrorParams {
    const float* y;        // [B][Nm][P*P*C], feature order (ph, pw, c), as UnembedParams::y; the row of a masked token is its rank among the row's masked tokens
    const float* x;        // frames, element (b,t,c,y,x) at b*sb + t*st + c*sc + y*W + x
    int64_t sb, st, sc;
    const float* target;   // the same with tb / tt / tc; nullptr = x
    int64_t tb, tt, tc;
    const uint8_t* mask;   // [B][Nt]
    const float* region;   // [B][T][H/P][W/P] weights; nullptr = ones
    PatchGrid g;           // frame: the predicted frame compared with EVERY target frame, or -1: frame t with target frame t
    float* map;            // [B][T][H/P][W/P] or nullptr
    float* mean;           // [B] or nullptr
    float* scratch;        // [B][T][H/P][W/P]: holds the map when only the mean is asked for (map == nullptr)
};

int launch_patch_error(const PatchErrorParams& p, hipStream_t stream);

// Response of a perturbation, from the predicted tokens of the perturbed rows and of the clean one (readout.hip token_response_kernel):
// r[b][Y][X] = sum_c (y - y_ref)^2 at the masked patches of frame `frame`, 0 at its visible ones; its per-patch mean, its first maximum, its sum and its
// centroid.  No allocation, no synchronisation, no atomics: two calls on the same inputs are bit-equal.
struct TokenResponseParams {
    const float* y;        // [B][Nm][P*P*C], as PatchErrorParams::y
    const float* y_ref;    // the same for the clean prediction; row b at b * ref_sb (0: one reference for all rows)
    int64_t ref_sb;
    const uint8_t* mask;   // [B][Nt]: the mask of y AND y_ref
    PatchGrid g;           // frame: 0 .. T-1
    float* map;            // [B][H/P][W/P] or nullptr
    float* pixel_map;      // [B][H][W] or nullptr
    int* peak_index;       // [B] or nullptr: Y * W + X
    float* stats;          // [B][4] or nullptr: peak, mass, centroid_y, centroid_x
    float* scratch;        // [B][H/P][8]: per-workgroup partials (peak, its index as int bits, mass, sum r Y, sum r X); needed with peak_index or stats
};

int launch_token_response(const TokenResponseParams& p, hipStream_t stream);

// One step of frontier unmasking on frame `frame` of a mask (unmask.hip unmask_select_kernel): the L-inf distance transform of the frame's grid (the reference's
// patch_distance_transform, bit for bit), the frontier d <= threshold on the masked cells, and the reveal of the k masked cells that rank first by (frontier,
// key descending with NaN first, index ascending).  One workgroup per batch row; no allocation, no synchronisation, no atomics.
constexpr int kUnmaskMaxCells = 4096;  // patches per frame (the row's state lives in LDS)
constexpr int kUnmaskMaxReveal = 64;
struct UnmaskStepParams {
    const uint8_t* mask;     // [B][T * gh * gw]
    int B, T, gh, gw, frame;
    int k;                   // cells revealed per row; 0: dist and frontier only, map / region / e are not read
    int race;                // 0: key = err; 1: key = max(err, 0) / e (a NaN err stays NaN)
    int self_mask;           // dist: the visible cells get the grid's maximum
    const float* threshold;  // [1] on the device; negative (or nullptr): every masked cell is frontier
    const float* map;        // [B][T][gh][gw]: err = map[b][frame] ...
    const float* region;     // ... times region[b][frame] when given
    const float* e;          // [B][gh * gw], race mode
    uint8_t* mask_out;       // [B][T * gh * gw] or nullptr: mask with the picks cleared; must not overlap mask
    int* picks;              // [B][k] or nullptr: token indices in pick order, -1 once the frame has no masked cell left
    float* dist;             // [B][gh * gw] or nullptr
    uint8_t* frontier;       // [B][gh * gw] or nullptr
};

int check_unmask_select(const UnmaskStepParams& p);  // the argument checks of the launch alone: 0 or CWM_ERR_INVALID with a message
int launch_unmask_select(const UnmaskStepParams& p, hipStream_t stream);

// One step of Spelke-object segmentation (segment.hip; the definition: include/cwm_hip.h cwm_segment_step): seed references, votes over the S flow samples, the
// 4-connected region of the candidates that hangs on the seed cell, per-patch coverage and the active / passive picks of the next round of counterfactuals.
// No allocation, no synchronisation, no atomics.
constexpr int kSegmentMaxSamples = 255;   // votes are bytes
constexpr int kSegmentMaxPixels = 1 << 18;
constexpr int kSegmentMaxWords = 8192;    // H ceil(W / 32) words per bitmap: two bitmaps of a row in 64 KiB of LDS
constexpr int kSegmentMaxPicks = 64;
struct SegmentStepParams {
    const float* f;          // flows by five element strides, or nullptr: the init step (S = 0)
    int64_t sb, sc, sh, sw, ss;
    int B, H, W, S, P;
    const int* seeds;        // [B][2] (y, x), clamped on the device
    const float* dirs;       // [S][2] (dy, dx) or nullptr
    float min_seed_mag, abs_thresh, rel_thresh, vote_frac, cos_min, inside_frac;
    int k_active, k_passive, ring_radius;
    const float* keys;       // [B][2][n] or nullptr
    float* seed_ref;         // [B][S]: ref_s, NaN where the sample is not valid
    uint8_t* votes;          // [B][H W]
    uint8_t* segment;        // [B][H W] or nullptr
    float* cover;            // [B][n] or nullptr
    int* stats;              // [B][4] or nullptr
    int* picks;              // [B][k_active + k_passive] or nullptr
    uint8_t* active_out;     // [B][2 n] or nullptr
    uint8_t* passive_out;    // [B][2 n] or nullptr
};
int check_segment_step(const SegmentStepParams& p);  // 0 or CWM_ERR_INVALID with a message that names the field
int launch_segment_step(const SegmentStepParams& p, hipStream_t stream);

// Seed selection (seed_select.hip; the definition: include/cwm_hip.h cwm_seed_select): a score map pooled to the patch grid, its peaks, and K rounds of
// arg-max under non-maximum suppression.  No allocation, no synchronisation, no atomics.
constexpr int kSeedMaxPicks = 64;
constexpr int kSeedMaxRadius = 64;
constexpr int kSeedMaxPrior = 64;
constexpr int kSeedMaxPixels = 1 << 18;
struct SeedSelectParams {
    const float* map;        // pixels: (b, y, x) at b sb + y sr + x; cells: [B][n] contiguous
    int cells;               // 0 pixels, 1 cells
    int64_t sb, sr;
    int B, H, W, P;
    const uint8_t* free;     // [B][n] or nullptr
    const float* e;          // [B][n] or nullptr: race mode
    const int* prior;        // [B][n_prior] or nullptr
    int n_prior, K, radius, peaks_only;
    float abs_thresh, rel_thresh;
    float* w_pooled;         // workspace (pixels form): [B][n] v ...
    uint8_t* w_offset;       // ... and [B][n] the seed pixel's offset py P + px inside its cell
    int* seeds;              // [B][K][2] or nullptr
    int* picks;              // [B][K] or nullptr
    float* values;           // [B][K] or nullptr
    float* pooled;           // [B][n] or nullptr
    uint8_t* peaks;          // [B][n] or nullptr
    int* stats;              // [B][4] or nullptr
};
int launch_seed_pool(const SeedSelectParams& p, hipStream_t stream);    // pixels form: fills w_pooled and w_offset
int launch_seed_select(const SeedSelectParams& p, hipStream_t stream);  // the pool pass where the form needs it, then the selection

struct ShiftPromptParams {
    const float* x;         // [B][T][C][H][W] contiguous frames
    int B, S, T, C, H, W, P, frame, fix_passive;
    const uint8_t* active;  // [B*S][Nt], 0 at the active (moved) patches
    const uint8_t* masks;   // [B*S][Nt], 0 at the passive (kept visible) patches
    const int* shifts;      // [B*S][2] (dy, dx) in patch units
    float* x_out;           // [B*S][T][C][H][W]
    uint8_t* mask_out;      // [B*S][Nt]
};

int launch_shift_prompts(const ShiftPromptParams& p, hipStream_t stream);
int launch_prompt_table_expand(const int* table, int S, int gh, int gw, int T, int frame, uint8_t* active, uint8_t* passive, int* shifts, hipStream_t stream);

constexpr int kMultiShiftMaxSteps = 8;  // K of cwm_multi_shift_prompts (a backward walk of K dependent table reads per pixel)
struct MultiShiftParams {
    const float* x;         // [B][T][C][H][W] contiguous frames
    int B, S, K, T, C, H, W, P, frame, fix_passive, mask_steps;
    const uint8_t* points;  // [B*S][K][Nt], non-zero at the patches step k moves (step-major: a wave reads adjacent cells of ONE step)
    const uint8_t* masks;   // [B*S][mask_steps][Nt] base masks (non-zero = masked), mask_steps = K or 1 (one mask for every step); NULL = none
    const int* shifts;      // [B*S][K][2] (sy, sx) in pixels
    float* x_out;           // [B*S][T][C][H][W]
    uint8_t* mask_out;      // [B*S][Nt]
};

int launch_multi_shift_prompts(const MultiShiftParams& p, hipStream_t stream);

// ---- IMU-conditioned conjoined predictor (conj_kernels.hip) ------------------------------------------
struct SmallAttnParams {
    const float* qkv;  // [B*n_tok][3*heads*head_dim] fp32 (bias already added; q NOT yet scaled)
    int B, n_tok, heads, head_dim;
    bf16* o;           // [planes][B*n_tok][ldo]
    int64_t o_plane;
    int ldo;
};
int launch_small_attention(const SmallAttnParams& p, int planes, hipStream_t stream);       // conj_kernels.hip: fp32 VALU form (any head_dim <= 64)
int launch_small_attention_mfma(const SmallAttnParams& p, int planes, hipStream_t stream);  // conj_attention.hip: head_dim 32
bool small_attention_mfma_ok(int n_tok, int head_dim);

// ext_mask[b] = [mask[b] | pad slot j masked unless j < vmax - visible(b)]  (conjoined_vmae.py:49-116)
int launch_pad_mask(const uint8_t* mask, int B, int N, int P, int vmax, uint8_t* ext_mask, hipStream_t stream);
// rows of x[B*n_rows][D] whose permutation entry is a pad slot (>= n_real) are set to `token` (null_token_enc)
int launch_fix_pad_rows(float* x, const int* perm, int B, int perm_stride, int n_rows, int n_real, int D, const float* token, hipStream_t stream);
// rows j of y[B][n_out][D] whose slot perm[b][n_vis + j] is a pad slot are zeroed (x * ~null_mask, conjoined_vmae.py:998-1002)
int launch_zero_pad_out_rows(float* y, const int* perm, int B, int perm_stride, int n_vis, int n_out, int n_real, int D, hipStream_t stream);

struct ImuGatherParams {
    const float* imu;  // [B][C][L]
    int B, C, L, tubelet;
    const int* perm;   // [B][perm_stride]
    int perm_stride, n_rows, n_real;
    bf16* out;         // [planes][B*n_rows][ld], K order (c, s), zero padded
    int64_t out_plane;
    int ld;
};
int launch_imu_gather(const ImuGatherParams& p, int planes, hipStream_t stream);
// ImuEncoder concat_dummy_token (conjoined_vmae.py:1124-1147): out[b] = [imu[b] (C x L) | dummy (C x T)] as [B][C][L + T], and
// mask_out[b] = [mask[b] (n) | 0] as [B][n + 1] (the dummy token is always visible)
int launch_imu_append_dummy(const float* imu, const uint8_t* mask, const float* dummy, int B, int C, int L, int T, int n, float* out, uint8_t* mask_out,
                            hipStream_t stream);

struct CrossAttnParams {
    const float* qk;      // [B*N][2D] main stream (fp32)                 -- VALU kernels (conj_kernels.hip)
    const float* v;       // [B*N][D]
    const bf16* qk_op;    // the same projections in the GEMM A-operand layout (common.h a_pos, row width 2D / D) -- MFMA kernel (conj_attention.hip)
    const bf16* v_op;
    const float* qk_src;  // [B*M][2D] context stream
    const float* v_src;   // [B*M][D]
    int B, N, M, heads, head_dim;  // D = heads*head_dim
    float scale;
    bf16* y;              // [planes][B*N][D]  main-stream update (softmax over the M context tokens)
    int64_t y_plane;
    bf16* y_src;          // [planes][B*M][D]  context update (softmax over the N main tokens)
    int64_t y_src_plane;
    float* scores_t;      // scratch [B][heads][M][N]
    float* partial;       // scratch, cross_attention_partial_floats(B, heads, M, head_dim) floats
};
int launch_cross_attention(const CrossAttnParams& p, int planes, hipStream_t stream);       // fp32 VALU kernels: qk / v fp32, scores_t + partial scratch
size_t cross_attention_partial_floats(int B, int heads, int M, int head_dim);
size_t cross_attention_lds_bytes(int M, int head_dim);  // what the VALU main kernel asks for ...
bool cross_attention_ok(int M, int head_dim);           // ... and whether it fits (M <= 64, head_dim a multiple of 32 <= 256, the LDS of one workgroup)
int launch_cross_attention_mfma(const CrossAttnParams& p, int planes, hipStream_t stream);  // MFMA kernel: qk_op / v_op, partial scratch
int launch_cross_attention_mfma_roles(const CrossAttnParams& p, int planes, hipStream_t stream_a, hipStream_t stream_b, int roles);  // bit 0: main update on stream_a, bit 1: context update on stream_b
bool cross_attention_mfma_ok(int head_dim, int M);
bool cross_attention_mfma_fits(int B, int N, int heads, int head_dim);  // the MFMA kernel's 32-bit offsets hold this lane (else: the VALU kernels)
size_t cross_attention_mfma_partial_floats(int B, int heads, int M, int head_dim);

int launch_perm_to_rank(const int* perm, int* rank, int B, int Nt, hipStream_t stream);

int launch_split_bf16(const float* x, int64_t n, bf16* hi, bf16* lo, hipStream_t stream);

// ---- RAFT-large optical flow (raft_kernels.hip) ------------------------------------------------------
// One channel segment of a convolution input: fp32 NHWC, pixel `pix` at p + pix * ld.  The value a consumer reads is
// relu?((v - mean) * rstd) * sigmoid(gate)?, or, with `coords`, the flow coords[pix] - (x, y) of a 2-channel coordinate field.
struct ConvSrc {
    const float* p;
    int ld, C;
    const float* stats;  // [img][C] (mean, rstd) pairs (instance norm) or nullptr
    int relu;
    const float* gate;   // multiply by sigmoid(gate[pix * gate_ld + c]) (the GRU's r * h) or nullptr
    int gate_ld;
    const float* coords; // [pix][2] coordinates: value = coords - (x, y)
};
// The input frames of the encoders: image i of a launch is pair (img0 + i) % P of frame (img0 + i) / P (0: image1, 1: image2); pair pr is
// (g, t) = (pr / ppg, pr % ppg); element (c, y, x) at base[which][g * sb + t * st + c * sc + y * W + x], scaled to 2 * (v * scale / 255) - 1
struct ImageSrc {
    const float* base[2];
    int64_t sb[2], st[2], sc[2];
    int P, ppg;
    float scale;
};
// One run of distinct frames of a forward that shares frames (FramePlan): frame j is (g, t) = (j / nt, j % nt) at base + g * sb + t * st, n of them.
// As an ImageSrc it is {base, -} with P = n and ppg = nt: the launches of a run read "image1" only.
struct FrameRun {
    const float* base;
    int64_t sb, st, sc;
    int n, nt;
};
// Where the per-frame operand of pair pr = (g, t) = (pr / ppg, pr % ppg) lies, in units of one frame's map: g * sb + t * st past the operand's pointer.
// One map per pair, in pair order (a forward that shares nothing): {1, 1, 0}.
struct SlotMap {
    int ppg;
    int64_t sb, st;
};
constexpr SlotMap kPairSlots = {1, 1, 0};
// Which frames a forward's encoders run on, and where each pair finds the maps of its two images (raft_model.hip raft_frame_plan).  Made on the host from
// the call's two image sources alone: two images are one frame when their address and channel stride are equal, and the plan merges only what one of
// three patterns shows to be equal -- P1: a source with stride_t == 0 is one frame per batch row; P2: a source with stride_b == 0 is one frame for all
// rows; P3: two sources of identical strides with image2 = image1 + k * stride_t, k in {0, +1, -1} (one frame repeated, a movie, a movie backwards) are
// one run of pairs + |k| frames per row.  Anything else (and every call with `share` off, or with a negative stride) runs every pair's two images: 2 P fnet and P cnet images.
struct FramePlan {
    bool shared;         // false: nothing merged (the slot maps are the identity)
    int n_fnet, n_cnet;  // frames through fnet / cnet
    int n2;              // distinct image2 frames (what the on-the-fly correlation pools)
    FrameRun frun[2];    // the frames of fnet in slot order: run 0, then run 1 (n = 0: none); n_fnet = frun[0].n + frun[1].n
    FrameRun crun;       // the frames of cnet (image1's own): n_cnet = crun.n
    int64_t base1, base2;    // pair (g, t): fmap1 at slot base1 + s1, fmap2 at base2 + s2 of fnet's output, the context map at slot sc of cnet's,
    SlotMap s1, s2, sc, s2p; // the pooled levels of fmap2 at slot s2p of image2's own frame order;
    SlotMap pool;            // image2's frame j lies at slot base2 + pool(j) of fnet's output
};
FramePlan raft_frame_plan(int batch, int ppg, const float* const img[2], const int64_t sb[2], const int64_t st[2], const int64_t sc[2], bool share);
// the slot of pair pr under a map, on the host
inline int64_t slot_at(const SlotMap& m, int64_t pr) { return (pr / m.ppg) * m.sb + (pr % m.ppg) * m.st; }
struct Im2colParams {
    ConvSrc src[2];  // the input channels are src[0] then src[1] (nsrc = 2: the GRU's [h | x])
    int nsrc;
    ImageSrc image;  // image.base[0] != nullptr: the frames instead of src (conv1 of the encoders; src[0].C = 3)
    int img0;
    int n_img, H, W, OH, OW, kh, kw, stride, pad_h, pad_w;
    int c_lo, c_hi;  // c_hi > c_lo: rewrite only input channels [c_lo, c_hi) of every tap (the rest of A, K padding included, is kept)
    bf16* A;         // [n_img * OH * OW] rows of Kpad (planes = 1) or 2 * Kpad (planes = 2, parity layout), K order (ky, kx, c), zero padded
    int Kpad;
};
struct CorrLookupParams {
    const float* pyr[4];  // level l: [M][h[l]][w[l]]
    int h[4], w[4], levels;
    const float* coords;  // [M][2]
    int64_t M;
    bf16* A;              // [M] rows of Kpad (planes = 1) or 2 * Kpad (planes = 2, parity layout), feature l*81 + a*9 + b, zero padded
    int Kpad;
    float* out;           // instead of A (out != nullptr): fp32 [M][out_ld], features [0, levels*81) (cwm_raft_corr_lookup)
    int out_ld;
};
// The same lookup without the correlation volume (AlternateCorrBlock, corr.py:63-91): the two feature maps, fmap2 also pooled to levels 1 .. 3
struct CorrOnTheFlyParams {
    const float* fmap1;     // [M][256]
    const float* fmap2[4];  // level l: [P][h[l]][w[l]][256], l times avg_pool2d(2, stride 2) of fmap2
    int h[4], w[4];
    const float* coords;    // [M][2]
    int64_t M, hw8;         // rows, and rows per pair (h[0] * w[0])
    bf16* A;                // as CorrLookupParams
    int Kpad;
    float* out;
    int out_ld;
    // frames shared between pairs (ppg > 0; all zero: fmap1 and every level hold one map per pair, in pair order): the maps of pair (g, t) are
    // g * sb + t * st maps past fmap1 (s1) and past fmap2[l] (s2[l]: level 0 lies in the encoder's frame order, the pooled levels in image2's own)
    int ppg;
    int64_t s1b, s1t, s2b[4], s2t[4];
};
// RAFT.upsample_flow of a C-channel low-resolution field (C = 2: the flow, C = 1: the output head's map): the 3 x 3 neighbourhood times 8, combined
// with the softmax of the 9 x 64 mask
struct ConvexUpParams {
    const float* coords;  // [P][h8][w8][2]: the field is the flow coords - (x, y) (C = 2 only), or nullptr:
    const float* value;   // the field itself, planar [P][C][h8][w8]
    const float* mask;    // [P][h8][w8][mask_ld]: channel k*64 + i*8 + j, times mask_scale
    int mask_ld;
    float mask_scale;
    int C, P, ppg, h8, w8;
    float* out;           // pair pr = (g, t): out + g * out_sb + t * out_st + c * out_sc + Y * 8w8 + X
    int64_t out_sb, out_st, out_sc;
};
// the params of a launch on a mask of 576 channels per pixel; the field is `coords` (C = 2) or `value`, one of them null
ConvexUpParams convex_up_params(int C, const float* coords, const float* value, const float* mask, float mask_scale, int P, int ppg, int h8, int w8, float* out,
                                int64_t out_sb, int64_t out_st, int64_t out_sc);
// A convolution is three statements, each made once here for the model (raft_model.hip run_conv / prepare) and the development entry point (dev.hip
// cwm_dev_raft_conv): its geometry in the im2col params, its weight parts packed into one GEMM operand, and the GEMM's params.  The launch of the GEMM is the
// caller's (Engine::run_gemm, or launch_gemm with the thread's options).
// n_img images of H x W under a kh x kw kernel: the output size OH x OW and the rest of the geometry (the sources, c_lo / c_hi and A are the caller's)
void set_conv_geometry(Im2colParams& ip, int n_img, int H, int W, int kh, int kw, int stride, int pad_h, int pad_w, int Kpad);
// One weight part [n][cin][kh][kw] (+ bias [n]) of a convolution; gamma != nullptr folds the eval-mode batch norm (gamma, beta, mean, var, each [n]) that
// follows the convolution
struct ConvPartW {
    const float *w, *b, *gamma, *beta, *mean, *var;
    int n;
};
// part i -> rows row0 .. row0 + n of the packed operand (w_il: parity layout, w_hi: fast) and bias[row0 ..], row0 = the output channels of the parts before it
int pack_conv_parts(const ConvPartW* parts, int nparts, float eps, int cin, int kh, int kw, int Kpad, bf16* w_il, bf16* w_hi, float* bias, hipStream_t s);
// C[:, 0:N] (row stride ldc: a column slice of an NHWC buffer) = A W^T + bias in fp32; W in the layout of the launch's planes
GemmParams conv_gemm(const bf16* A, const bf16* W, const float* bias, int M, int N, int Kpad, float* C, int ldc);
// planes: the layout of A (common.h a_pos): 2 = split-bf16 hi / lo (parity), 1 = one bf16 plane (fast); the same for launch_corr_lookup
int launch_im2col(const Im2colParams& p, int planes, hipStream_t s);
// stats [n_img][C] (mean, rstd) pairs; work: 2 * n_img * kInstNormMaxChunks * C doubles
constexpr int kInstNormMaxChunks = 16;
int launch_instnorm_stats(const float* x, int n_img, int HW, int C, float eps, float* stats, double* work, hipStream_t s);
int launch_residual_join(const ConvSrc& X, const ConvSrc& Y, int n_img, int HW, float* out, hipStream_t s);
// `cs`: where pair pr's context map [hw8][256] lies in cn (kPairSlots: cn is [M][256], one map per pair)
int launch_cnet_split(const float* cn, int64_t M, float* h, float* x, hipStream_t s, int64_t hw8 = 1, SlotMap cs = kPairSlots);
int launch_coords_init(float* coords, int64_t M, int h8, int w8, hipStream_t s);
// coords = grid + init (the warm start): element (c, y, x) of pair (g, t) = (pr / ppg, pr % ppg) of the planar field at init[g * sb + t * st + c * sc + y * w8 + x]
int launch_coords_init_flow(float* coords, int P, int ppg, int h8, int w8, const float* init, int64_t sb, int64_t st, int64_t sc, hipStream_t s);
// corr[p] = f1[slot s1 of p] f2[slot s2 of p]^T / sqrt(D) for the P pairs; kPairSlots: f1 and f2 are [P][N][D]
int launch_corr(const float* f1, const float* f2, int P, int N, int D, float* corr, hipStream_t s, SlotMap s1 = kPairSlots, SlotMap s2 = kPairSlots);
int launch_corr_pool(const float* in, int64_t maps, int h, int w, float* out, hipStream_t s);
int launch_corr_lookup(const CorrLookupParams& p, int planes, hipStream_t s);
// avg_pool2d(2, stride 2), floor, of an NHWC map [P][h][w][C] -> [P][h / 2][w / 2][C] (C a multiple of 4, 16-byte aligned maps)
// `is`: map j of the output pools the input map at slot `is` of j (kPairSlots: the input is [P] maps in order)
int launch_fmap_pool(const float* in, int64_t P, int h, int w, int C, float* out, hipStream_t s, SlotMap is = kPairSlots);
// launch_corr_lookup's features from the feature maps themselves: every tap's correlation is computed when it is looked up (fp32 FMA, fixed order)
int launch_corr_lookup_on_the_fly(const CorrOnTheFlyParams& p, int planes, hipStream_t s);
int launch_motion_finish(float* x, const float* coords, int64_t M, int h8, int w8, hipStream_t s);
int launch_gru_update(float* h, const float* zr, const float* q, int64_t M, hipStream_t s);
int launch_flow_update(float* coords, const float* delta, int ld, int64_t M, hipStream_t s);
int launch_convex_upsample(const ConvexUpParams& p, hipStream_t s);
int launch_flow_low(const float* coords, int P, int h8, int w8, float* out, hipStream_t s);
// forward_interpolate (raft/utils.py:28-56) of P planar fields [2][h8][w8] (rows contiguous; field p at flow + p * stride_p, its channel c at + c * stride_c)
// -> out [P][2][h8][w8] contiguous: every target takes the valid source that lands nearest to it (double arithmetic, lowest index among equals; zeros
// when none is valid).  Brute force, N^2 distances per field: h8 * w8 <= 65536.  out must not overlap flow.
int launch_forward_interpolate(const float* flow, int64_t stride_p, int64_t stride_c, int P, int h8, int w8, float* out, hipStream_t s);
// The output head (raft_model.py:152-159, 257-267; output_dim = 1).  launch_head_project: value[m] = bias[0] + sum_c w[c] * relu(hidden[m * ld + c]) over
// the 256 channels of output_block.0's result, fp32, one wave per low-resolution pixel; launch_convex_upsample with C = 1 then upsamples that planar map.
constexpr int kHeadHidden = 256;
int launch_head_project(const float* hidden, int ld, const float* w, const float* bias, int64_t M, float* value, hipStream_t s);
// CorrBlock built from two feature maps [P][h8 * w8][256] and indexed at coords [P * h8 * w8][2]: the pyramid (allocated and freed inside), then the lookup
// as fp32 `out` [M][324], or (out == nullptr) as convc1's Kpad = 384 operand A in the layout of `planes`.  Synchronises the stream.
// s1 / s2: where pair p's maps lie in fmap1 / fmap2 (kPairSlots: one map per pair, as above).
int raft_corr_lookup_run(const float* fmap1, const float* fmap2, const float* coords, int P, int h8, int w8, float* out, bf16* A, int planes, hipStream_t s,
                         SlotMap s1 = kPairSlots, SlotMap s2 = kPairSlots);
// The same result from AlternateCorrBlock's form: what is allocated and freed inside is fmap2's three poolings, not a correlation volume.  Synchronises the stream.
int raft_corr_lookup_on_the_fly_run(const float* fmap1, const float* fmap2, const float* coords, int P, int h8, int w8, float* out, bf16* A, int planes,
                                    hipStream_t s);

}  // namespace cwm
