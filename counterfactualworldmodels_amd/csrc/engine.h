// Shared host-side machinery of the model handles behind the C ABI: packed weights, state-dict slots,
// activation workspace, timed launches, batch lanes and the transformer Block sequence.  Used by model.hip
// (plain VMAE predictor), conj_model.hip (conjoined predictors) and raft_model.hip (RAFT).
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/cwm_hip.h"
#include "common.h"
#include "kernels.h"

namespace cwm {

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

struct LinearW {
    bf16* w = nullptr;     // fast mode:   [Npad][Kpad]   bf16(weight)
    bf16* w_il = nullptr;  // parity mode: [Npad][2*Kpad] hi/lo interleaved per 32-k block (common.h a_pos)
    int64_t plane = 0;
    int N = 0, K = 0, Npad = 0, Kpad = 0;
    float* bias = nullptr;  // [Npad] (zero-filled) or nullptr when the layer has no bias
};

struct BlockW {
    float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
    LinearW qkv, proj, fc1, fc2;
};

enum SlotKind { SLOT_MATRIX, SLOT_VECTOR, SLOT_IGNORED };

struct Slot {
    SlotKind kind = SLOT_VECTOR;
    std::vector<int64_t> shape;
    LinearW* lin = nullptr;  // SLOT_MATRIX
    float* dst = nullptr;    // SLOT_VECTOR (device)
    int repeat = 1;          // SLOT_VECTOR: number of consecutive copies written at dst
    int64_t numel = 0;
    bool loaded = false;
    bool optional = false;  // missing_weights does not count it (the handle that set it checks for itself where the tensor is needed)
};

struct EventPair {
    hipEvent_t a, b;
    double flops;
    int sub;  // kernel class the launch is also booked under (0: none)
};

struct KernelTimer {
    bool enabled = false;
    std::vector<EventPair> pool;
    size_t used = 0;
    cwm_kernel_stats acc = {0, 0.0, 0.0};
};

// Activation buffers of one token stream (bf16 planes are [2][rows][width], plane stride set per use).
struct StreamBuffers {
    bf16 *hbuf = nullptr, *gbuf = nullptr, *qbuf = nullptr, *kbuf = nullptr, *vbuf = nullptr;
    float* qkv_f32 = nullptr;  // only for streams whose head_dim != 64 (small-sequence attention path)
};

// One token stream (patch / tubelet embed -> encoder -> encoder_to_decoder -> decoder -> head): the plain VMAE predictor is one of them (no padding, no null
// tokens), a conjoined predictor two.  StreamW is what creation fixes (dims and weights), StreamWs the stream's workspace pointers.
struct StreamW {
    int enc_dim = 0, dec_dim = 0, enc_heads = 0, dec_heads = 0, n_tok = 0, max_pad = 0, out_dim = 0, embed_k = 0, embed_kpad = 0;
    std::vector<BlockW> enc, dec;
    LinearW embed, e2d, head;
    float *enc_norm_g = nullptr, *enc_norm_b = nullptr, *dec_norm_g = nullptr, *dec_norm_b = nullptr;
    float *mask_token = nullptr, *null_enc = nullptr;
    float *pos_enc_ext = nullptr, *pos_dec_ext = nullptr;  // [n_tok + max_pad][D]; pad rows: 0 (enc) / null_token_dec (dec)
    int n_slots() const { return n_tok + max_pad; }
};

// Every buffer is batch-major, so a lane that starts at batch element b0 owns the slice behind the capacity of b0 elements: a lane works on its own copy of
// this struct (for_each_stream_buffer), next to a reference to the StreamW.
struct StreamWs {
    uint8_t* ext_mask = nullptr;  // (a stream that takes the caller's mask as it is leaves it unused: one byte per token)
    int* perm = nullptr;
    bf16* tokens_in = nullptr;
    float *x_enc = nullptr, *x_dec = nullptr;
    StreamBuffers sb;
};

// THE layout of a stream's workspace: visit(pointer, elements per batch element) for every buffer.  Every size is linear in the batch size, so the same
// statement serves the allocation (WsAlloc: per_b * batch capacity elements) and a lane's view (WsShift: pointer += per_b * b0).  vcap = the visible rows per
// sample the workspace holds -- its CAPACITY (the handle's ws_nvis / ws_vmain / ws_vctx), not a call's count --; small = the stream keeps qkv in fp32
// (run_block_small) instead of the three bf16 buffers.
template <typename Visit>
int for_each_stream_buffer(const StreamW& S, StreamWs& w, int vcap, int mlp_ratio, bool small, Visit&& visit) {
    const size_t rows_e = (size_t)vcap, rows_d = (size_t)S.n_slots();
    const size_t act = std::max(rows_e * S.enc_dim, rows_d * S.dec_dim);
    int rc;
    if ((rc = visit(w.ext_mask, rows_d)) || (rc = visit(w.perm, rows_d)) || (rc = visit(w.tokens_in, 2 * rows_e * S.embed_kpad)) ||
        (rc = visit(w.x_enc, rows_e * S.enc_dim)) || (rc = visit(w.x_dec, rows_d * S.dec_dim)) || (rc = visit(w.sb.hbuf, 2 * act)) ||
        (rc = visit(w.sb.gbuf, 2 * act * mlp_ratio)))
        return rc;
    if (small) return visit(w.sb.qkv_f32, 3 * act);
    if ((rc = visit(w.sb.qbuf, 2 * act)) || (rc = visit(w.sb.kbuf, 2 * act))) return rc;
    return visit(w.sb.vbuf, 2 * act);
}

// Encoder rows (batch elements x visible tokens) each half of a batch must keep for the forward to run as two batch lanes (cwm_forward,
// cwm_conj_forward).  Measured (tools/lane_threshold.py, round 4): ViT-B/8 batch 8 / 10 / 14 (3168 / 3960 / 5544 rows per half) -6 / -7.5 / -10 % with
// two lanes, batch 6 (2376) +3 %; ViT-L/4 batch 2 (3168) -7 %.  (Rounds 1-3 used 6000: batch >= 16.)
constexpr int kMinLaneRows = 3000;  // (Tuning.min_lane_rows overrides it per model: tools/lane_threshold.py)
// The IMU-conditioned model (its lanes carry a context stream each: four queues): batch 2 / 3 / 4 / 6 are 5.3 / 4.3 / 2.5 / 2.8 % SLOWER on two lanes,
// batch 8 / 12 / 16 2.3 / 1.4 / 1.0 % faster (3172 visible rows per sample; rounds 1-3 split from batch 4)
constexpr int kMinLaneRowsConj = 12000;

// The streams and events of a forward that runs as batch lanes: lane 0 is the caller's stream, lanes 1 .. n - 1 non-blocking streams of the model, created on
// first use.  fork() makes them wait for what the caller's stream holds so far, join() makes the caller's stream wait for them.  The caller decides the lane
// count and the batch split, issues its launches stage by stage over stream(l, ...), and joins even after a failed launch: the caller's stream must not run
// ahead of work already queued on a lane.
struct Lanes {
    static constexpr int kMax = 4;
    hipStream_t streams[kMax - 1] = {};
    hipEvent_t ev_fork = nullptr, ev_join[kMax - 1] = {};
    int forked = 1;  // lanes between fork() and join()
    ~Lanes();
    int fork(hipStream_t caller, int n_lanes);
    hipStream_t stream(int l, hipStream_t caller) const { return l == 0 ? caller : streams[l - 1]; }
    int join(hipStream_t caller);
};

struct Engine {
    int device = 0;
    int overlapped = 0;  // 1 while a forward call runs two batch lanes (passed to the GEMM kernel choice)
    Tuning tune = thread_tuning();  // this model's execution options (cwm_model_set_option); every launch of the model carries a pointer to it
    float ln_eps = 1e-6f;
    std::map<std::string, Slot> slots;
    uint64_t loads = 0;  // load_weight calls that changed a stored tensor (not those into an ignored slot): a handle that derives data from its slots compares it
    std::vector<void*> allocs;     // weights etc., freed on destroy
    std::vector<void*> ws_allocs;  // workspace, re-allocated when it has to grow
    uint64_t ws_bytes = 0;         // bytes asked of alloc() for the workspace held now (free_workspace resets it)
    KernelTimer timers[CWM_KCLASS_COUNT];
    struct SplitKWs {
        float* slabs;
        unsigned* counts;
        uint64_t last_use;  // launch counter at the last split launch on the stream: the eviction order
    };
    uint64_t splitk_clock = 0;
    static constexpr size_t kMaxSplitKStreams = 8;
    std::map<hipStream_t, SplitKWs> splitk_ws;  // one split-K workspace per stream that has launched a split GEMM (batch lanes run concurrently); created lazily, capped
    // Decoder block 0 of the plain VMAE predictor, mask-token rows: LN1 and the Q/K/V projection of mask_token + pos_dec[p] depend on the weights and the token
    // position p only -- not on the sample, the input or the call -- so they are kept as a table of n_tok rows per arithmetic mode ([fast, parity]) in the
    // Q / K / V element format: [q hi(, q lo), k hi(, k lo), v hi(, v lo)] planes of [heads][n_tok][64].  Built lazily on the forward's stream by the same
    // LayerNorm kernel and GEMM launch path as the rows of a forward (rows are independent in both: the same bits); stale after any load_weight.
    struct Dec0Table {
        bf16* qkv = nullptr;
        uint64_t loads = 0;  // Engine::loads when it was built
        bool built = false;
    };
    Dec0Table dec0_tab[2];

    ~Engine();
    int alloc(void** p, size_t bytes, bool zero, bool workspace);
    template <typename T>
    int ws(T** p, size_t count) {
        void* v = nullptr;
        if (int rc = alloc(&v, count * sizeof(T), true, true)) return rc;
        *p = (T*)v;
        return 0;
    }
    int free_workspace();

    int make_linear(LinearW& L, int N, int K, bool bias);
    int make_vec(float** v, int n);
    void add_matrix_slot(const std::string& key, LinearW* L, std::vector<int64_t> shape);
    void add_vec_slot(const std::string& key, float* dst, std::vector<int64_t> shape, int repeat = 1);
    void add_ignored_slot(const std::string& key, std::vector<int64_t> shape);
    int make_block(BlockW& b, const std::string& pre, int D, int hidden);
    int make_sinusoid(float** dst, int n_pos, int d, int extra_rows = 0);      // VideoMAE/utils.py:251-268 (float64 host)
    int make_pos_embedding_f32(float** dst, int n_pos, int d, int extra_rows = 0);  // transformer.py:37-52 (float32)
    // weights and state-dict slots of one stream under the key prefix `pre` (S's dims, n_tok, max_pad and out_dim are set by the caller)
    int make_stream(StreamW& S, const std::string& pre, int embed_k, std::vector<int64_t> embed_shape, int depth_e, int depth_d, int mlp_ratio,
                    bool sinusoid_f64, bool null_tokens);

    int load_weight(const char* key, const float* data, int on_device, const int64_t* shape, int ndim);
    int missing_weights(char* buf, int buflen);
    int require_weights(const char* fn);                            // CWM_ERR_INVALID naming the first tensor that was never loaded
    int set_option(const char* fn, const char* key, int value);  // cwm_model_set_option / cwm_conj_set_option

    int run_gemm(const GemmParams& p, int planes, hipStream_t s, bool book = true);  // book = false: not counted by the kernel timers
    int attach_splitk_workspace(GemmParams& p, hipStream_t s);  // this stream's entry of splitk_ws, created or evicted as needed
    int run_attention(const AttnParams& p, int planes, hipStream_t s);
    // the HBM-bound edge kernels, booked by class with their algorithmic bytes (cwm_hip.h CWM_KCLASS_*)
    int run_layernorm(const LayerNormParams& p, int planes, hipStream_t s);
    int run_patch_gather(const PatchGatherParams& p, int planes, hipStream_t s);
    int run_index_gather(const PatchGatherParams& p, const uint8_t* mask, int n_vis, int* perm, int* rank, int* err_rows, int planes, hipStream_t s,
                         int n_vis_min = 0, int* counts = nullptr);  // (n_vis_min > 0: ragged batches, kernels.h launch_index_gather)
    int run_fill_mask_tokens(float* x_full, const float* mask_token, const float* pos, const int* perm, int B, int Nt, int n_vis, int D, hipStream_t s,
                             const int* counts = nullptr, int n_vis_min = 0);  // (counts: ragged batches, kernels.h launch_fill_mask_tokens)
    int run_unembed(const UnembedParams& p, hipStream_t s);
    // `launch()` between an event pair of class `kclass` (no events unless the class is enabled); work = FLOPs or bytes
    template <typename F>
    int timed(int kclass, double work, hipStream_t s, F&& launch) {
        EventPair* e = nullptr;
        if (int rc = timer_begin(kclass, work, s, &e)) return rc;
        if (int rc = launch()) return rc;
        return timer_end(e, s);
    }
    int timer_begin(int kclass, double work, hipStream_t s, EventPair** out);
    int timer_end(EventPair* e, hipStream_t s);
    // the launches every forward is made of: LayerNorm of `rows` contiguous rows into the GEMM A-operand layout, and y = A W^T + bias in fp32 (+ resid), in
    // the A-operand layout (what the MFMA cross attention reads its token fragments from), or through GELU in the A-operand layout
    int layernorm_to(const float* x, int rows, int D, const float* g, const float* b, bf16* out, int planes, hipStream_t s) {
        return run_layernorm(layernorm_rows(x, D, D, g, b, ln_eps, rows, out, D), planes, s);
    }
    int linear_f32(const bf16* A, int rows, int K, const LinearW& L, float* C, const float* resid, int planes, hipStream_t s);
    int linear_operand(const bf16* A, int rows, int K, const LinearW& L, bf16* out, int planes, hipStream_t s);
    int linear_gelu(const bf16* A, int rows, int K, const LinearW& L, bf16* out, int planes, hipStream_t s);
    // x += fc2(gelu(fc1(LN x))) on x[B*n_tok, D] (in place): the second half of a Block and of each side of a cross block.  n_keep: see run_block
    int run_mlp(const float* ln_g, const float* ln_b, const LinearW& fc1, const LinearW& fc2, float* x, int B, int n_tok, int D, int planes, StreamBuffers& sb,
                hipStream_t s, int n_keep = 0);
    // Block.forward (VideoMAE/utils.py:146-153) on a residual stream x[B*n_tok, D] (in place), head_dim 64
    // key_len (device, [B]; nullptr: all n_tok): the keys sample b attends to -- the encoder blocks of a ragged batch (AttnParams.key_len)
    // tab_rows (with tab_vis, tab_perm; nullptr: off): decoder block 0 of a rectangular batch -- rows [tab_vis, n_tok) of every sample are mask tokens, whose
    // Q / K / V rows are copied from the table (dec0_table) at the positions tab_perm[b][j]; LN1 and the Q/K/V GEMM run over the first tab_vis rows only
    int run_block(const BlockW& w, float* x, int B, int n_tok, int D, int H, int planes, StreamBuffers& sb, hipStream_t s, int n_keep = 0,
                  const int* key_len = nullptr, const bf16* tab_rows = nullptr, int tab_vis = 0, const int* tab_perm = nullptr);
    // The table of this mode, (re)built on stream s when it is missing or a weight was loaded since; x_tmp [n_tok][dec_dim] fp32, h_tmp [2][n_tok][dec_dim] bf16 and
    // perm_tmp [n_tok] are scratch of the caller (workspace buffers nothing on s or behind it still needs)
    int dec0_table(const StreamW& S, int planes, float* x_tmp, bf16* h_tmp, int* perm_tmp, hipStream_t s, const bf16** tab);
    // same for short sequences with any head_dim (fp32 VALU attention): the IMU context stream
    int run_block_small(const BlockW& w, float* x, int B, int n_tok, int D, int H, int planes, StreamBuffers& sb, hipStream_t s);
    // the pieces of a stream's forward around its blocks, over B samples of n_vis visible rows each (w: the lane's view)
    int embed_stream(const StreamW& S, const StreamWs& w, int B, int n_vis, int planes, hipStream_t s);
    // counts (device, [B]; nullptr: every sample has n_vis): sample b has counts[b] in [n_vis_min, n_vis] encoder rows, mask tokens from there on
    int to_decoder(const StreamW& S, const StreamWs& w, int B, int n_vis, int planes, hipStream_t s, const int* counts = nullptr, int n_vis_min = 0);
    // out[B][n_out][head.N] = head(norm(x_dec[:, -n_out:]))
    int head_rows(const StreamW& S, const StreamWs& w, int B, int n_out, float* out, int planes, hipStream_t s);

    int timing_enable(int kclass, int enable);
    int timing_collect(int kclass, cwm_kernel_stats* out);
};

// The versioned argument structs of the forward entry points (`struct_size` first): the caller's struct may end before fields a later version appended, so
// copy what it has into a zeroed one (the rest reads as "not requested").  `min_size`: the end of the last field of the first version; the upper bound
// catches a struct without the field.  `fn` names the entry point, whose struct is `<fn>_args`.
template <typename Args>
int copy_args(Args& dst, const Args* src, size_t min_size, const char* fn, const char* note = "") {
    CWM_REQUIRE(src->struct_size >= min_size && src->struct_size <= 4096, "%s: args->struct_size = %u is not a %s_args (set it to sizeof(%s_args)%s)", fn,
                src->struct_size, fn, fn, note);
    memset(&dst, 0, sizeof(dst));
    memcpy(&dst, src, std::min<size_t>(src->struct_size, sizeof(dst)));
    return 0;
}

// The two visitors of a workspace layout (for_each_stream_buffer): allocate every buffer for `batch` elements, or move every pointer behind b0 elements.
struct WsAlloc {
    Engine& E;
    size_t batch;
    template <typename T>
    int operator()(T*& p, size_t per_b) const { return E.ws(&p, per_b * batch); }
};
struct WsShift {
    size_t b0;
    template <typename T>
    int operator()(T*& p, size_t per_b) const {
        p += per_b * b0;
        return 0;
    }
};

GemmParams gemm_base(const bf16* A, int lda, const LinearW& L, int M, int planes);
// The Q/K/V projection of B samples' first n_in of n_tok rows (A: [B * n_in][D], D = L.N / 3) with its per-head scatter.  Decoder block 0's table is built by the
// same statement as a forward's rows (Engine::dec0_table, Engine::run_block): the two must stay bit-equal.
inline GemmParams qkv_gemm(const bf16* A, const LinearW& L, int B, int n_in, int n_tok, int H, bf16* q, bf16* k, bf16* v, int64_t qk_plane, int planes) {
    const int D = L.N / 3;
    GemmParams g = gemm_base(A, D, L, B * n_in, planes);
    set_qkv_epilogue(g, n_in, n_tok, D, D / H, q, k, v, qk_plane);
    return g;
}

// fp32 [N][K] -> bf16 [Npad][Kpad] (hi only) and [Npad][2*Kpad] (hi/lo interleaved), zero padded
int launch_pack_weight(const float* src, int N, int K, bf16* hi, bf16* il, int Npad, int Kpad, hipStream_t stream);

// ---- what the stand-alone entry points (model.hip) and the development ones (dev.hip) share ----
// The arithmetic mode of an entry point `fn` as the number of bf16 planes its operands have (fast: 1, parity: 2)
static inline int mode_planes(const char* fn, int mode, int* planes) {
    CWM_REQUIRE(mode == CWM_MODE_FAST || mode == CWM_MODE_PARITY, "%s: bad mode", fn);
    *planes = mode == CWM_MODE_PARITY ? 2 : 1;
    return 0;
}
// Device buffers of one call, freed when it returns.  They allocate per call: not for hot loops.
struct Scratch {
    std::vector<void*> ptrs;
    ~Scratch() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    template <typename T>
    T* get(size_t count) {
        void* p = nullptr;
        if (hipMalloc(&p, count * sizeof(T) + 16) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return (T*)p;
    }
    // Zeroed ON THE STREAM that uses the buffer.  (hipMemset runs on the null stream, which a non-blocking stream does not wait for, and while the null stream
    // is busy it returns before the fill has landed: the call then read what the block last held -- the error word or the bias of an earlier call -- and the
    // fill could land on top of what the call had written; tests/test_stream_order_gpu.py protocol B)
    template <typename T>
    T* get_zeroed(size_t count, hipStream_t s) {
        T* p = get<T>(count);
        if (p && hipMemsetAsync(p, 0, count * sizeof(T), s) != hipSuccess) return nullptr;
        return p;
    }
};
// fp32 a [M][K], w [N][K], bias [N] (or nullptr) as a GEMM reads them in the mode of `planes`: A rows in the operand layout with K zero-padded to Kp =
// round_up(K, 64), W packed by launch_pack_weight to Np = round_up(N, 256) rows, bias [Np] zero beyond N.  The buffers are `sc`'s (model.hip).
struct LinearOperands {
    bf16 *A, *W;
    float* bias;
    int Kp, Np;
};
int stage_linear_operands(Scratch& sc, const char* who, const float* a, const float* w, const float* bias, int M, int N, int K, int planes, hipStream_t s,
                          LinearOperands* out);
// qkv [B, N, 3, H, 64] fp32 -> Q (times scale), K, V [B * H, N, 64], hi plane and lo plane (qk_plane elements further) whatever the mode (model.hip)
int launch_qkv_scatter(const float* qkv, int B, int N, int H, float scale, bf16* q, bf16* k, bf16* v, int64_t qk_plane, hipStream_t s);
// Attention on qkv [B, N, 3, H, 64] fp32 with this thread's options (model.hip): Q / K / V scattered into `sc`'s buffers, then one launch_attention that writes
// O into o_dst in the operand layout (rows of ldo columns; nullptr: a buffer of `sc`, rows of H * 64).  key_len: AttnParams.key_len or nullptr; q_off / n_q: the
// query window (0, 0: all rows).  *o_out = where O went.  Nothing is synchronised.
int attention_from_qkv(Scratch& sc, const char* who, const float* qkv, const int* key_len, bf16* o_dst, int ldo, int B, int N, int H, int q_off, int n_q, int planes,
                       hipStream_t s, bf16** o_out);
// mask -> permutation -> rank -> un-embed of y into out, frames x at strides (sb, sc, st); n_vis_min > 0: rows of n_vis_min .. n_vis visible tokens, y row 0 =
// decoder row n_vis_min (a ragged batch).  Synchronises; CWM_ERR_MASK with the text of the case when a row's count is off (model.hip)
int unembed_from_mask(const char* who, const float* y, const float* x, int64_t sb, int64_t sc, int64_t st, const uint8_t* mask, int B, int T, int C, int H, int W, int P,
                      int n_vis_min, int n_vis, float* out, hipStream_t s);
// Reads err[0] back on s (synchronising): CWM_ERR_MASK with the text of the case (n_vis_min > 0: a ragged batch's range) when it is set
int check_mask_err(const int* err, int n_vis_min, int n_vis, hipStream_t s);

}  // namespace cwm
