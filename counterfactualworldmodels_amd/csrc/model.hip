// Model handle, weight packing, workspace and forward orchestration behind the C ABI (include/cwm_hip.h).
// Restates the control flow of `PretrainVisionTransformer.forward` (cwm/models/VideoMAE/vmae.py:539-560),
// `PretrainVisionTransformerEncoder.forward_features` (:152-173), `...Decoder.forward` (:246-255) and
// `Block.forward` (cwm/models/VideoMAE/utils.py:146-153) as a fixed sequence of HIP kernel launches
// on the caller's stream.
#include <stddef.h>

#include "engine.h"

using namespace cwm;

// The workspace of a forward: the token stream's buffers + what only this model has.  Every buffer is batch-major, so the lane that starts at batch
// element b0 owns the slice behind the capacity of b0 elements (lane_ws).
struct ModelWs {
    StreamWs st;
    int* rank = nullptr;  // inverse permutation, for the un-embed
    int* err = nullptr;   // one word per batch row (index_gather_kernel writes every row's, every call: no memset)
    int* counts = nullptr;  // ragged batches (cwm_model_set_ragged): visible tokens per batch row, written by the index prologue (behind `err` in its allocation)
};

struct cwm_model {
    Engine eng;
    cwm_config cfg;
    StreamW st;  // the model is ONE token stream without padding (max_pad = 0, no null tokens)
    // workspace (grown on demand)
    int ws_batch = 0, ws_nvis = 0;
    ModelWs ws;
    // batch lanes (cwm_model_set_lanes): a batch whose slices keep >= kMinLaneRows encoder rows each runs as up to `lanes` slices, the first on the
    // caller's stream and the others on streams of `lane_set`, joined by events before cwm_forward returns control of the stream
    int lanes = 2;
    // cwm_model_set_ragged: 0 = every row of a call has args->n_vis visible tokens; > 0 = between this many and args->n_vis
    int ragged_min = 0;
    static constexpr int kMaxLanes = Lanes::kMax;
    Lanes lane_set;
};

namespace {

// the workspace layout (engine.h for_each_stream_buffer): the stream's buffers for n_vis_cap visible rows per sample, and the inverse permutation
template <typename Visit>
int for_each_buffer(const cwm_model* m, ModelWs& w, int n_vis_cap, Visit&& visit) {
    if (int rc = for_each_stream_buffer(m->st, w.st, n_vis_cap, m->cfg.mlp_ratio, false, visit)) return rc;
    return visit(w.rank, (size_t)m->st.n_tok);
}

int ensure_workspace(cwm_model* m, int B, int n_vis) {
    if (B <= m->ws_batch && n_vis <= m->ws_nvis && m->ws_batch > 0) return 0;
    Engine& E = m->eng;
    const int Bc = std::max(B, m->ws_batch), Nv = std::max(n_vis, m->ws_nvis);
    m->ws_batch = 0;  // (nothing is usable until all of it is there again)
    int rc;
    if ((rc = E.free_workspace()) || (rc = for_each_buffer(m, m->ws, Nv, WsAlloc{E, (size_t)Bc}))) return rc;
    // `err` is the one buffer that is not linear in the batch size (B + 4 words, and as many again for the rows' visible counts), so it is not part of the
    // layout: allocated here, sliced in lane_ws
    if ((rc = E.ws(&m->ws.err, (size_t)2 * Bc + 8))) return rc;
    m->ws.counts = m->ws.err + Bc + 4;
    m->ws_batch = Bc;
    m->ws_nvis = Nv;
    // (the zero fills above ran on the null stream; the lane streams are non-blocking and would not wait for them)
    CWM_HIP_CHECK(hipDeviceSynchronize());
    return 0;
}

// the view of the lane that starts at batch element b0: offsets at the workspace's capacity (ws_nvis), whatever the call's n_vis
ModelWs lane_ws(const cwm_model* m, int b0) {
    ModelWs w = m->ws;
    (void)for_each_buffer(m, w, m->ws_nvis, WsShift{(size_t)b0});
    w.err += b0;
    w.counts += b0;
    return w;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int cwm_model_create(const cwm_config* cfg, cwm_model** out) {
    CWM_REQUIRE(cfg && out, "cwm_model_create: null argument");
    const cwm_config& c = *cfg;
    CWM_REQUIRE(c.patch > 0 && c.img_h % c.patch == 0 && c.img_w % c.patch == 0, "image size (%d,%d) must be divisible by patch size %d",
                c.img_h, c.img_w, c.patch);
    CWM_REQUIRE(c.patch % 4 == 0 && c.img_w % 4 == 0, "patch size must be a multiple of 4");
    CWM_REQUIRE(c.enc_heads > 0 && c.dec_heads > 0 && c.enc_dim == 64 * c.enc_heads && c.dec_dim == 64 * c.dec_heads,
                "this build supports head_dim 64 only (enc %d/%d, dec %d/%d)", c.enc_dim, c.enc_heads, c.dec_dim, c.dec_heads);
    CWM_REQUIRE(c.enc_dim <= 1024 && c.dec_dim <= 1024 && c.enc_dim % 64 == 0 && c.dec_dim % 64 == 0, "embed dims must be multiples of 64, <= 1024");
    CWM_REQUIRE(c.in_chans == 3 && c.num_frames >= 1 && c.mlp_ratio >= 1 && c.enc_depth >= 1 && c.dec_depth >= 1, "unsupported config");
    cwm_model* m = new cwm_model();
    m->cfg = c;
    Engine& E = m->eng;
    E.ln_eps = c.ln_eps;
    CWM_HIP_CHECK(hipGetDevice(&E.device));
    StreamW& S = m->st;
    S.enc_dim = c.enc_dim; S.dec_dim = c.dec_dim; S.enc_heads = c.enc_heads; S.dec_heads = c.dec_heads;
    S.n_tok = (c.img_h / c.patch) * (c.img_w / c.patch) * c.num_frames; S.out_dim = c.in_chans * c.patch * c.patch;
    // (the float64 sinusoid tables: vmae.py:75, :366)
    const int rc = E.make_stream(S, "", c.in_chans * c.patch * c.patch, {c.enc_dim, c.in_chans, 1, c.patch, c.patch}, c.enc_depth, c.dec_depth, c.mlp_ratio,
                                 true, false);
    if (rc) {
        cwm_model_destroy(m);
        return rc;
    }
    *out = m;
    return CWM_OK;
}

extern "C" void cwm_model_destroy(cwm_model* m) { delete m; }

extern "C" int cwm_model_load_weight(cwm_model* m, const char* key, const float* data, int on_device, const int64_t* shape, int ndim) {
    CWM_REQUIRE(m, "cwm_model_load_weight: null model");
    return m->eng.load_weight(key, data, on_device, shape, ndim);
}

extern "C" int cwm_model_missing_weights(cwm_model* m, char* buf, int buflen) { return m->eng.missing_weights(buf, buflen); }

// (Rounds 2-3 carried a form with every LayerNorm folded into the GEMMs around it -- parity-tested, measured slower: the 4 bytes / element
// a producer GEMM then adds to its store-bound epilogue cost more than the LayerNorm launch they replace, DESIGN.md section 4.6 -- never the
// default and removed in round 4.)

// One lane: batch elements [b0, b0 + B) of the call, on stream s, in the workspace slice lw.
// Stages [stage_lo, stage_hi) of the lane's launch sequence: 0 = mask -> permutation, patch gather + embed; 1 .. Le = encoder blocks;
// Le + 1 = encoder norm + encoder_to_decoder + mask tokens; Le + 2 .. Le + 1 + Ld = decoder blocks; Le + Ld + 2 = norm + head + un-embed.
// (cwm_forward issues stage by stage over all lanes, so that after a host synchronisation every lane's queue starts filling at once
// instead of lane 1 waiting behind lane 0's ~136 launches.)
// dec0_tab (nullptr: off): the mask-token rows of decoder block 0's Q / K / V come from this table (Engine::dec0_table) instead of LN1 and the GEMM
static int forward_lane(cwm_model* m, const cwm_forward_args* a, int b0, int B, ModelWs lw, hipStream_t s, int stage_lo, int stage_hi, const bf16* dec0_tab) {
    const cwm_config& c = m->cfg;
    const StreamW& S = m->st;
    StreamWs& w = lw.st;
    // ragged batch (cwm_model_set_ragged): Nv is the cap of the rows' visible counts, which the index prologue leaves in lw.counts; the encoder runs Nv
    // rows per sample of which sample b attends to its first counts[b]; the decoder's output rows are the last Nt - ragged_min of every sample
    const int rg_min = m->ragged_min;
    const int* counts = rg_min > 0 ? lw.counts : nullptr;
    const int Nt = S.n_tok, Nv = a->n_vis, Nm = Nt - (rg_min > 0 ? rg_min : Nv);
    const int Nret = Nm > 0 ? Nm : Nt;
    Engine& E = m->eng;
    const int planes = a->mode == CWM_MODE_PARITY ? 2 : 1;
    const float* x_in = a->x_dev + (int64_t)b0 * a->x_stride_b;
    const uint8_t* mask_in = a->mask_dev + (size_t)b0 * Nt;
    float* y_tokens = a->y_tokens_dev + (size_t)b0 * Nret * S.out_dim;
    int rc;
    auto in_range = [&](int st) { return st >= stage_lo && st < stage_hi; };
    const int st_e2d = c.enc_depth + 1, st_head = c.enc_depth + c.dec_depth + 2;

    if (in_range(0)) {
    // a1-a3: mask -> permutation (+ its inverse for the un-embed, + the per-row check of the visible count), frame load (+normalise) and
    // tubelet patch gather of the visible tokens in ONE launch (elementwise.hip index_gather_kernel); then the patch-embed GEMM with bias
    // and positional-table add in the epilogue
    PatchGatherParams pg;
    memset(&pg, 0, sizeof(pg));
    pg.x = x_in; pg.sb = a->x_stride_b; pg.sc = a->x_stride_c; pg.st = a->x_stride_t; pg.normalize = a->normalize;
    pg.C = c.in_chans; pg.H = c.img_h; pg.W = c.img_w; pg.P = c.patch; pg.perm = w.perm; pg.Nt = Nt; pg.n_rows = Nv; pg.B = B;
    pg.out = w.tokens_in; pg.out_plane = (int64_t)B * Nv * S.embed_kpad; pg.ld = S.embed_kpad;
    if (E.tune.index_fused) {
        if ((rc = E.run_index_gather(pg, mask_in, Nv, w.perm, a->y_video_dev ? lw.rank : nullptr, lw.err, planes, s, rg_min, lw.counts))) return rc;
    } else {  // the four launches of rounds 1-4 (A/B and the bitwise cross-check of the fused kernel)
        CWM_HIP_CHECK(hipMemsetAsync(lw.err, 0, (size_t)B * sizeof(int), s));
        if ((rc = launch_mask_to_perm(mask_in, B, Nt, Nv, w.perm, lw.err, s, rg_min, lw.counts))) return rc;
        if ((rc = E.run_patch_gather(pg, planes, s))) return rc;
        if (a->y_video_dev && (rc = launch_perm_to_rank(w.perm, lw.rank, B, Nt, s))) return rc;
    }
    if ((rc = E.embed_stream(S, w, B, Nv, planes, s))) return rc;
    }

    // a4-a6: encoder blocks over the visible tokens
    for (int i = 0; i < c.enc_depth; ++i)
        if (in_range(1 + i) && (rc = E.run_block(S.enc[i], w.x_enc, B, Nv, S.enc_dim, S.enc_heads, planes, w.sb, s, 0, counts))) return rc;

    // a7: encoder.norm, encoder_to_decoder (no bias); a8: + pos[vis] written straight into x_full rows [0,Nv), mask tokens behind them
    if (in_range(st_e2d) && (rc = E.to_decoder(S, w, B, Nv, planes, s, counts, rg_min))) return rc;

    // a9: decoder blocks over the full token set, norm + head on the last Nm tokens
    // (the last block only has to produce the Nm rows the head reads: option "prune_last_block" = 0 runs it in full)
    const bool pruned = Nm > 0 && E.tune.prune_last_block;
    for (int i = 0; i < c.dec_depth; ++i) {
        const int keep = (i == c.dec_depth - 1 && pruned) ? Nm : 0;
        const bf16* tab = i == 0 ? dec0_tab : nullptr;
        if (in_range(st_e2d + 1 + i) && (rc = E.run_block(S.dec[i], w.x_dec, B, Nt, S.dec_dim, S.dec_heads, planes, w.sb, s, keep, nullptr, tab, Nv, w.perm))) return rc;
    }
    if (!in_range(st_head)) return CWM_OK;
    if ((rc = E.head_rows(S, w, B, Nret, y_tokens, planes, s))) return rc;

    // a11: patch un-embed scatter
    if (a->y_video_dev) {
        const float* xr = a->xraw_dev ? a->xraw_dev + (int64_t)b0 * a->x_stride_b : x_in;
        UnembedParams u;  // (lw.rank: written by the index prologue of stage 0)
        memset(&u, 0, sizeof(u));
        u.y = y_tokens; u.x = xr; u.sb = a->x_stride_b; u.sc = a->x_stride_c; u.st = a->x_stride_t;
        u.mask = mask_in; u.rank = lw.rank; u.B = B; u.T = c.num_frames; u.C = c.in_chans; u.H = c.img_h; u.W = c.img_w;
        // (ragged batch: y row j of every sample is decoder row ragged_min + j, whatever the sample's own count -- and `rank` is the decoder row)
        u.P = c.patch; u.n_vis = Nt - Nm; u.Nm = Nm;
        u.out = a->y_video_dev + (size_t)b0 * c.num_frames * c.in_chans * c.img_h * c.img_w;
        if ((rc = E.run_unembed(u, s))) return rc;
    }
    return CWM_OK;
}

extern "C" int cwm_forward(cwm_model* m, const cwm_forward_args* a_in) {
    CWM_REQUIRE(m && a_in, "cwm_forward: null argument");
    // (the upper bound of struct_size catches a caller built against the 0.5 header, which had no such field: the low half of its x_dev pointer lands there)
    cwm_forward_args a_copy;
    if (int rc = copy_args(a_copy, a_in, offsetof(cwm_forward_args, stream) + sizeof(void*), "cwm_forward", "; callers built against the 0.5 header must be rebuilt"))
        return rc;
    const cwm_forward_args* a = &a_copy;
    if (int rc = cwm_require_device(m->eng.device, "cwm_forward")) return rc;
    CWM_REQUIRE(a->x_dev && a->mask_dev && a->y_tokens_dev, "cwm_forward: x_dev, mask_dev and y_tokens_dev are required");
    CWM_REQUIRE(a->mode == CWM_MODE_FAST || a->mode == CWM_MODE_PARITY, "cwm_forward: bad mode %d", a->mode);
    const cwm_config& c = m->cfg;
    const int B = a->batch, Nt = m->st.n_tok, Nv = a->n_vis, Nm = Nt - Nv;
    CWM_REQUIRE(B > 0, "cwm_forward: batch must be positive");
    CWM_REQUIRE(m->ragged_min <= Nv, "cwm_forward: the handle takes rows of at least %d visible tokens (cwm_model_set_ragged), more than the call's cap n_vis = %d",
                m->ragged_min, Nv);
    CWM_REQUIRE(Nv > 0 && Nm >= 0, "cwm_forward: need 0 < n_vis (%d) <= num tokens (%d)", Nv, Nt);
    // nothing masked: the reference decoder then returns head(norm(x)) for ALL tokens (vmae.py:250-253), and its wrapper cannot
    // compose a video from that (prediction.py:252-254 would assign Nt rows to an empty selection)
    CWM_REQUIRE(Nm > 0 || !a->y_video_dev, "cwm_forward: no token is masked, there is no predicted patch to un-embed");
    CWM_REQUIRE(!a->y_video_dev || a->xraw_dev || a->normalize, "cwm_forward: y_video_dev needs the raw frames (xraw_dev) when normalize=0");
    if (int rc = m->eng.require_weights("cwm_forward")) return rc;
    if (int rc = ensure_workspace(m, B, Nv)) return rc;
    hipStream_t s = (hipStream_t)a->stream;
    // Decoder block 0's mask-token rows from the per-position table (option "mask_token_tables"; a rectangular batch with masked tokens): looked up -- after a weight
    // load, rebuilt -- on the caller's stream before the lanes fork, in the first lane's workspace, which stage 0 then overwrites
    const bf16* dec0_tab = nullptr;
    if (m->eng.tune.mask_token_tables && Nm > 0 && m->ragged_min == 0)
        if (int rc = m->eng.dec0_table(m->st, a->mode == CWM_MODE_PARITY ? 2 : 1, m->ws.st.x_dec, m->ws.st.sb.hbuf, m->ws.st.perm, s, &dec0_tab)) return rc;

    // Batch lanes: between two dependent kernels the queue idles ~6 us (x 136 kernels = 5 % of a batch-32 step) and every kernel ends in a
    // partially filled round of workgroups; further, independent slices of the batch on other queues fill both.
    const int min_rows = m->eng.tune.min_lane_rows > 0 ? m->eng.tune.min_lane_rows : kMinLaneRows;
    int n_lanes = 1;
    while (n_lanes < m->lanes && n_lanes < B && (int64_t)(B / (n_lanes + 1)) * Nv >= min_rows) ++n_lanes;
    int first[cwm_model::kMaxLanes + 1];
    for (int l = 0; l <= n_lanes; ++l) first[l] = (int)(((int64_t)B * l + n_lanes - 1) / n_lanes);  // lane l owns batch elements [first[l], first[l+1])
    if (int rc = m->lane_set.fork(s, n_lanes)) return rc;
    m->eng.overlapped = n_lanes >= 2;
    int rc = 0;
    // launch order: stage by stage (one transformer block at a time) over all lanes, so that every lane's queue starts filling at once
    const int n_stages = c.enc_depth + c.dec_depth + 3;
    for (int st = 0; st < n_stages && !rc; ++st)
        for (int l = 0; l < n_lanes && !rc; ++l)
            rc = forward_lane(m, a, first[l], first[l + 1] - first[l], lane_ws(m, first[l]), m->lane_set.stream(l, s), st, st + 1, dec0_tab);
    m->eng.overlapped = 0;
    if (int jrc = m->lane_set.join(s)) return jrc;  // (even after a failed launch)
    if (rc) return rc;

    if (a->check) {
        std::vector<int> herr((size_t)B, 0);
        CWM_HIP_CHECK(hipMemcpyAsync(herr.data(), m->ws.err, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
        CWM_HIP_CHECK(hipStreamSynchronize(s));
        if (std::any_of(herr.begin(), herr.end(), [](int e) { return e != 0; })) {
            if (m->ragged_min > 0)
                cwm_set_error("mask rows do not all have between %d (cwm_model_set_ragged) and n_vis=%d visible tokens", m->ragged_min, Nv);
            else
                cwm_set_error("mask rows do not all have n_vis=%d visible tokens (shape '[%d, -1, %d]' is invalid for the gathered input)", Nv, B, c.enc_dim);
            return CWM_ERR_MASK;
        }
    }
    return CWM_OK;
}

extern "C" int cwm_model_set_lanes(cwm_model* m, int lanes) {
    CWM_REQUIRE(m && lanes >= 1 && lanes <= cwm_model::kMaxLanes, "cwm_model_set_lanes: lanes must be 1 .. %d", cwm_model::kMaxLanes);
    m->lanes = lanes;
    return CWM_OK;
}

extern "C" int cwm_model_set_ragged(cwm_model* m, int n_vis_min) {
    CWM_REQUIRE(m && n_vis_min >= 0 && n_vis_min <= m->st.n_tok, "cwm_model_set_ragged: n_vis_min must be 0 (rectangular batches) or a visible count up to %d",
                m ? m->st.n_tok : 0);
    m->ragged_min = n_vis_min;
    return CWM_OK;
}

extern "C" int cwm_model_set_option(cwm_model* m, const char* key, int value) {
    CWM_REQUIRE(m && key, "cwm_model_set_option: null argument");
    return m->eng.set_option("cwm_model_set_option", key, value);
}

extern "C" int cwm_timing_enable(cwm_model* m, int kclass, int enable) {
    CWM_REQUIRE(m, "cwm_timing_enable: null model");
    return m->eng.timing_enable(kclass, enable);
}

extern "C" int cwm_timing_collect(cwm_model* m, int kclass, cwm_kernel_stats* out) {
    CWM_REQUIRE(m, "cwm_timing_collect: null model");
    return m->eng.timing_collect(kclass, out);
}

// ---------------------------------------------------------------------------------------------
// stand-alone kernel entry points (tests).  They allocate scratch per call: not for hot loops.
// ---------------------------------------------------------------------------------------------
namespace {
// fp32 [rows][K] -> GEMM A-operand layout of the given mode (common.h a_pos), K zero-padded to Kpad
template <int PLANES>
__global__ void pad_split_rows_kernel(const float* src, int rows, int K, bf16* out, int Kpad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * Kpad) return;
    const int r = (int)(i / Kpad), k = (int)(i - (int64_t)r * Kpad);
    const float v = k < K ? src[(size_t)r * K + k] : 0.f;
    store_operand<PLANES>(out, r, Kpad, k, v);
}

// qkv [B,N,3,H,64] fp32 -> Q (scaled), K, V [B*H,N,64]
__global__ void qkv_scatter_kernel(const float* qkv, int B, int N, int H, float scale, bf16* q, bf16* k, bf16* v_out, int64_t qk_plane) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int D = H * 64;
    if (i >= (int64_t)B * N * 3 * D) return;
    const int c = (int)(i % (3 * D));
    const int64_t row = i / (3 * D);
    const int b = (int)(row / N), n = (int)(row - (int64_t)b * N);
    const int which = c / D, cc = c - which * D, h = cc / 64, d = cc - h * 64;
    float v = qkv[i];
    if (which == 0) v *= scale;
    bf16 hi, lo;
    split_bf16(v, hi, lo);
    bf16* dst = which == 0 ? q : which == 1 ? k : v_out;
    const size_t o = ((size_t)(b * H + h) * N + n) * 64 + d;
    dst[o] = hi;
    dst[o + qk_plane] = lo;
}

// GEMM A-operand layout (row length ld_in, a multiple of 32) -> fp32 [rows][ld]
// key_len (with bad and N; nullptr: every row): the rows are [B][N], of which the first key_len[b] of every batch row were written; the others, and every row when
// key_len_check_kernel flagged a length in bad[0], are left as the caller passed them
template <int PLANES>
__global__ void merge_planes_kernel(const bf16* in, float* out, int rows, int ld, int ld_in, const int* key_len, const int* bad, int N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * ld) return;
    const int r = (int)(i / ld), c = (int)(i - (int64_t)r * ld);
    if (key_len && (bad[0] || r % N >= key_len[r / N])) return;
    const bf16* s = in + a_pos<PLANES>(r, ld_in, c);
    out[i] = (float)s[0] + (PLANES == 2 ? (float)s[kLoOffset] : 0.f);
}

// cwm_attention_ragged: bad[0] = 1 when a row's key count is outside [1, N]
__global__ void key_len_check_kernel(const int* key_len, int B, int N, int* bad) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && (key_len[b] < 1 || key_len[b] > N)) bad[0] = 1;
}
}  // namespace

int cwm::stage_linear_operands(Scratch& sc, const char* who, const float* a, const float* w, const float* bias, int M, int N, int K, int planes, hipStream_t s,
                               LinearOperands* out) {
    const int Kp = round_up(K, 64), Np = round_up(N, 256);
    out->Kp = Kp;
    out->Np = Np;
    out->A = sc.get<bf16>((size_t)2 * M * Kp);
    out->W = sc.get<bf16>((size_t)2 * Np * Kp);
    out->bias = sc.get_zeroed<float>(Np, s);
    CWM_REQUIRE(out->A && out->W && out->bias, "%s: out of device memory", who);
    const unsigned gridA = (unsigned)(((int64_t)M * Kp + 255) / 256);
    dispatch_int<1, 2>(planes == 2 ? 2 : 1, [&](auto pl) { hipLaunchKernelGGL(pad_split_rows_kernel<pl.value>, dim3(gridA), dim3(256), 0, s, a, M, K, out->A, Kp); });
    if (int rc = launch_pack_weight(w, N, K, planes == 1 ? out->W : nullptr, planes == 2 ? out->W : nullptr, Np, Kp, s)) return rc;
    if (bias) CWM_HIP_CHECK(hipMemcpyAsync(out->bias, bias, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

int cwm::launch_qkv_scatter(const float* qkv, int B, int N, int H, float scale, bf16* q, bf16* k, bf16* v, int64_t qk_plane, hipStream_t s) {
    const int64_t total = (int64_t)B * N * 3 * H * 64;
    hipLaunchKernelGGL(qkv_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, qkv, B, N, H, scale, q, k, v, qk_plane);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int cwm_split_bf16(const float* x_dev, int64_t n, void* hi_dev, void* lo_dev, void* stream) {
    CWM_REQUIRE(x_dev && hi_dev && n >= 0, "cwm_split_bf16: bad argument");
    return launch_split_bf16(x_dev, n, (bf16*)hi_dev, (bf16*)lo_dev, (hipStream_t)stream);
}

extern "C" int cwm_linear(const float* a_dev, const float* w_dev, const float* bias_dev, const float* resid_dev, float* c_dev, int M,
                          int N, int K, int gelu, int mode, void* stream) {
    CWM_REQUIRE(a_dev && w_dev && c_dev && M > 0 && N > 0 && K > 0, "cwm_linear: bad argument");
    int planes;
    if (int rc = mode_planes("cwm_linear", mode, &planes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    Scratch sc;
    LinearOperands op;
    if (int rc = stage_linear_operands(sc, "cwm_linear", a_dev, w_dev, bias_dev, M, N, K, planes, s, &op)) return rc;
    const int ldg = round_up(N, 32);  // operand-layout rows are whole [32 hi | 32 lo] blocks
    bf16* G = gelu ? sc.get<bf16>((size_t)2 * M * ldg) : nullptr;
    CWM_REQUIRE(!gelu || G, "cwm_linear: out of device memory");
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = op.A; p.lda = op.Kp; p.W = op.W;
    p.M = M; p.N = N; p.K = op.Kp; p.bias = op.bias;
    if (gelu) {
        p.epi = EPI_BF16_GELU; p.out_hi = G; p.ldo = ldg;
    } else {
        p.epi = EPI_F32; p.C = c_dev; p.ldc = N; p.resid = resid_dev; p.ldr = N;
    }
    p.tune = &thread_tuning();
    if (int rc = launch_gemm(p, planes, s)) return rc;
    if (gelu) {
        const unsigned gridG = (unsigned)(((int64_t)M * N + 255) / 256);
        dispatch_int<1, 2>(planes, [&](auto pl) {
            hipLaunchKernelGGL(merge_planes_kernel<pl.value>, dim3(gridG), dim3(256), 0, s, G, c_dev, M, N, ldg, (const int*)nullptr, (const int*)nullptr, 0);
        });
    }
    CWM_HIP_CHECK(hipStreamSynchronize(s));
    return CWM_OK;
}

int cwm::attention_from_qkv(Scratch& sc, const char* who, const float* qkv, const int* key_len, bf16* o_dst, int ldo, int B, int N, int H, int q_off, int n_q, int planes,
                            hipStream_t s, bf16** o_out) {
    const int64_t qk_plane = (int64_t)B * N * H * 64, o_plane = (int64_t)B * (n_q ? n_q : N) * ldo;
    bf16* q = sc.get<bf16>(2 * qk_plane);
    bf16* k = sc.get<bf16>(2 * qk_plane);
    bf16* v = sc.get<bf16>(2 * qk_plane);
    bf16* o = o_dst ? o_dst : sc.get<bf16>(2 * o_plane);
    CWM_REQUIRE(q && k && v && o, "%s: out of device memory", who);
    if (int rc = launch_qkv_scatter(qkv, B, N, H, 0.125f, q, k, v, qk_plane, s)) return rc;
    AttnParams a = attn_dense(q, k, v, qk_plane, o, o_plane, ldo, B, H, N);
    a.q_off = q_off; a.n_q = n_q;
    a.key_len = key_len;
    a.tune = &thread_tuning();
    *o_out = o;
    return launch_attention(a, planes, s);
}

// cwm_attention, and with a key count per batch row (AttnParams.key_len) cwm_attention_ragged: what a predictor needs to run rows with different numbers of visible
// tokens as one batch, where the reference equalises the counts first (RectangularizeMasks, prediction.py:421) because its gather reshapes to one count (vmae.py:167)
static int attention_entry(const char* who, const float* qkv_dev, const int32_t* key_len_dev, float* o_dev, int B, int N, int H, int mode, void* stream) {
    int planes;
    if (int rc = mode_planes(who, mode, &planes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int D = H * 64;
    Scratch sc;
    int* bad = nullptr;
    if (key_len_dev) {
        bad = sc.get_zeroed<int>(4, s);
        CWM_REQUIRE(bad, "%s: out of device memory", who);
        hipLaunchKernelGGL(key_len_check_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, key_len_dev, B, N, bad);
    }
    bf16* o;
    if (int rc = attention_from_qkv(sc, who, qkv_dev, key_len_dev, nullptr, D, B, N, H, 0, 0, planes, s, &o)) return rc;
    dispatch_int<1, 2>(planes, [&](auto pl) {
        hipLaunchKernelGGL(merge_planes_kernel<pl.value>, dim3((unsigned)(((int64_t)B * N * D + 255) / 256)), dim3(256), 0, s, o, o_dev, B * N, D, D, key_len_dev, bad, N);
    });
    int hbad = 0;
    if (bad) CWM_HIP_CHECK(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    CWM_HIP_CHECK(hipStreamSynchronize(s));
    if (hbad) {
        cwm_set_error("%s: a key count is outside [1, N = %d]; o_dev was not written", who, N);
        return CWM_ERR_INVALID;
    }
    return CWM_OK;
}

extern "C" int cwm_attention(const float* qkv_dev, float* o_dev, int B, int N, int H, int mode, void* stream) {
    CWM_REQUIRE(qkv_dev && o_dev && B > 0 && N > 0 && H > 0, "cwm_attention: bad argument");
    return attention_entry("cwm_attention", qkv_dev, nullptr, o_dev, B, N, H, mode, stream);
}

extern "C" int cwm_attention_ragged(const float* qkv_dev, const int32_t* key_len_dev, float* o_dev, int B, int N, int H, int mode, void* stream) {
    CWM_REQUIRE(qkv_dev && key_len_dev && o_dev && B > 0 && N > 0 && H > 0, "cwm_attention_ragged: bad argument");
    return attention_entry("cwm_attention_ragged", qkv_dev, key_len_dev, o_dev, B, N, H, mode, stream);
}

extern "C" int cwm_layernorm(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* y_dev, int rows, int D, float eps,
                             void* stream) {
    CWM_REQUIRE(x_dev && gamma_dev && beta_dev && y_dev && rows > 0, "cwm_layernorm: bad argument");
    hipStream_t s = (hipStream_t)stream;
    Scratch sc;
    const int ldo = round_up(D, 32);  // operand-layout rows are whole [32 hi | 32 lo] blocks
    bf16* tmp = sc.get<bf16>((size_t)2 * rows * ldo);
    CWM_REQUIRE(tmp, "cwm_layernorm: out of device memory");
    LayerNormParams ln = layernorm_rows(x_dev, D, D, gamma_dev, beta_dev, eps, rows, tmp, ldo);
    ln.out_f32 = y_dev;
    if (int rc = launch_layernorm(ln, 2, s)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize(s));
    return CWM_OK;
}

int cwm::check_mask_err(const int* err, int n_vis_min, int n_vis, hipStream_t s) {
    int herr = 0;
    CWM_HIP_CHECK(hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, s));
    CWM_HIP_CHECK(hipStreamSynchronize(s));
    if (herr) {
        if (n_vis_min > 0)
            cwm_set_error("mask rows do not all have between %d and n_vis=%d visible tokens", n_vis_min, n_vis);
        else
            cwm_set_error("mask rows do not all have n_vis=%d visible tokens", n_vis);
        return CWM_ERR_MASK;
    }
    return CWM_OK;
}

extern "C" int cwm_mask_to_perm(const uint8_t* mask_dev, int B, int Nt, int n_vis, int32_t* perm_dev, void* stream) {
    CWM_REQUIRE(mask_dev && perm_dev && B > 0 && Nt > 0, "cwm_mask_to_perm: bad argument");
    hipStream_t s = (hipStream_t)stream;
    Scratch sc;
    int* err = sc.get_zeroed<int>(4, s);
    CWM_REQUIRE(err, "cwm_mask_to_perm: out of device memory");
    if (int rc = launch_mask_to_perm(mask_dev, B, Nt, n_vis, perm_dev, err, s)) return rc;
    return check_mask_err(err, 0, n_vis, s);
}

int cwm::unembed_from_mask(const char* who, const float* y, const float* x, int64_t sb, int64_t sc, int64_t st, const uint8_t* mask, int B, int T, int C, int H, int W,
                           int P, int n_vis_min, int n_vis, float* out, hipStream_t s) {
    const int Nt = T * (H / P) * (W / P);
    Scratch tmp;
    int* perm = tmp.get<int>((size_t)B * Nt);
    int* rank = tmp.get<int>((size_t)B * Nt);
    int* err = tmp.get_zeroed<int>(4, s);
    int* counts = n_vis_min > 0 ? tmp.get<int>((size_t)B) : nullptr;
    CWM_REQUIRE(perm && rank && err && (counts || n_vis_min == 0), "%s: out of device memory", who);
    int rc;
    if ((rc = launch_mask_to_perm(mask, B, Nt, n_vis, perm, err, s, n_vis_min, counts))) return rc;
    if ((rc = launch_perm_to_rank(perm, rank, B, Nt, s))) return rc;
    const int y0 = n_vis_min > 0 ? n_vis_min : n_vis;  // the decoder row of y row 0
    UnembedParams u = {};
    u.y = y; u.x = x; u.sb = sb; u.st = st; u.sc = sc;
    u.mask = mask; u.rank = rank; u.B = B; u.T = T; u.C = C; u.H = H; u.W = W; u.P = P; u.n_vis = y0; u.Nm = Nt - y0; u.out = out;
    if ((rc = launch_unembed(u, s))) return rc;
    return check_mask_err(err, n_vis_min, n_vis, s);
}

extern "C" int cwm_unembed(const float* y_tokens_dev, const float* x_dev, const uint8_t* mask_dev, int B, int T, int C, int H, int W, int P,
                           int n_vis, float* out_dev, void* stream) {
    CWM_REQUIRE(y_tokens_dev && x_dev && mask_dev && out_dev, "cwm_unembed: null argument");
    CWM_REQUIRE(P > 0 && H % P == 0 && W % P == 0, "cwm_unembed: image size must be divisible by the patch size");
    return unembed_from_mask("cwm_unembed", y_tokens_dev, x_dev, (int64_t)T * C * H * W, (int64_t)H * W, (int64_t)C * H * W, mask_dev, B, T, C, H, W, P, 0, n_vis, out_dev,
                             (hipStream_t)stream);
}

extern "C" int cwm_mask_row_counts(const uint8_t* mask_dev, int B, int Nt, int32_t* counts_dev, void* stream) {
    CWM_REQUIRE(mask_dev && counts_dev && B > 0 && Nt > 0, "cwm_mask_row_counts: bad argument");
    return launch_mask_row_counts(mask_dev, B, Nt, counts_dev, (hipStream_t)stream);
}

extern "C" int cwm_mask_flip_picks(uint8_t* mask_dev, int B, int Nt, const int32_t* table_dev, int n_rows, void* stream) {
    CWM_REQUIRE(mask_dev && table_dev && B > 0 && Nt > 0 && n_rows >= 0 && n_rows <= B, "cwm_mask_flip_picks: bad argument");
    return launch_mask_flip_picks(mask_dev, B, Nt, table_dev, n_rows, (hipStream_t)stream);
}

extern "C" int cwm_prompt_table_expand(const int32_t* table_dev, int S, int T, int grid_h, int grid_w, int frame, uint8_t* active_dev, uint8_t* passive_dev,
                                       int32_t* shifts_dev, void* stream) {
    CWM_REQUIRE(table_dev && active_dev && passive_dev && shifts_dev, "cwm_prompt_table_expand: null argument");
    CWM_REQUIRE(S > 0 && T >= 2 && grid_h > 0 && grid_w > 0 && frame >= 1 && frame < T, "cwm_prompt_table_expand: bad sizes (S %d, T %d, grid %d x %d, frame %d)", S, T, grid_h, grid_w, frame);
    return launch_prompt_table_expand(table_dev, S, grid_h, grid_w, T, frame, active_dev, passive_dev, shifts_dev, (hipStream_t)stream);
}

extern "C" int cwm_shift_prompts(const float* x_dev, int B, int T, int C, int H, int W, int P, int frame, int S, int fix_passive,
                                 const uint8_t* active_dev, const uint8_t* masks_dev, const int32_t* shifts_dev, float* x_out_dev,
                                 uint8_t* mask_out_dev, void* stream) {
    CWM_REQUIRE(active_dev && masks_dev && shifts_dev && (x_out_dev || mask_out_dev) && (x_dev || !x_out_dev), "cwm_shift_prompts: null argument");
    CWM_REQUIRE(B > 0 && S > 0 && T > 0 && C > 0 && P > 0, "cwm_shift_prompts: bad sizes");
    ShiftPromptParams p;
    memset(&p, 0, sizeof(p));
    p.x = x_dev; p.B = B; p.S = S; p.T = T; p.C = C; p.H = H; p.W = W; p.P = P; p.frame = frame; p.fix_passive = fix_passive;
    p.active = active_dev; p.masks = masks_dev; p.shifts = shifts_dev; p.x_out = x_out_dev; p.mask_out = mask_out_dev;
    return launch_shift_prompts(p, (hipStream_t)stream);
}

extern "C" int cwm_multi_shift_prompts(const float* x_dev, int B, int T, int C, int H, int W, int P, int frame, int S, int K, int fix_passive,
                                       const uint8_t* points_dev, const uint8_t* masks_dev, int mask_steps, const int32_t* shifts_dev, int max_abs_shift,
                                       float* x_out_dev, uint8_t* mask_out_dev, void* stream) {
    CWM_REQUIRE(points_dev && shifts_dev && (x_dev || !x_out_dev), "cwm_multi_shift_prompts: null argument");
    CWM_REQUIRE(x_out_dev || mask_out_dev, "cwm_multi_shift_prompts: null outputs (x_out_dev and mask_out_dev are both NULL)");
    CWM_REQUIRE(B > 0 && S > 0 && T > 0 && C > 0 && P > 0 && H > 0 && W > 0, "cwm_multi_shift_prompts: bad sizes");
    CWM_REQUIRE(max_abs_shift >= 0 && max_abs_shift < (H < W ? H : W), "cwm_multi_shift_prompts: shifts up to %d px, need |s| < min(H=%d, W=%d)", max_abs_shift, H, W);
    MultiShiftParams p;
    memset(&p, 0, sizeof(p));
    p.x = x_dev; p.B = B; p.S = S; p.K = K; p.T = T; p.C = C; p.H = H; p.W = W; p.P = P; p.frame = frame; p.fix_passive = fix_passive;
    p.points = points_dev; p.masks = masks_dev; p.mask_steps = masks_dev ? mask_steps : 0; p.shifts = shifts_dev;
    p.x_out = x_out_dev; p.mask_out = mask_out_dev;
    return launch_multi_shift_prompts(p, (hipStream_t)stream);
}

