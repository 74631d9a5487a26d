// IMU-conditioned conjoined padded predictor behind the C ABI (BASELINE configs[4]).
// Restates `ConjoinedPaddedVisionTransformer.forward` for `imu400_base_4x4patch_2frames_1tube`
// (cwm/models/VideoMAE/conjoined_vmae.py:889-1011, 852-887, 1230-1243): two token streams (RGB "main",
// IMU "context"), null-token padding (:49-165), cross-attention blocks BEFORE encoder blocks 0,3,6,9 and
// AFTER every decoder block (:543-576, :688-720; cwm/models/transformer.py:253-378, 442-583).
#include <stddef.h>

#include "engine.h"

using namespace cwm;

namespace {

struct CrossW {
    float *n1_g, *n1_b, *n1s_g, *n1s_b, *n2_g, *n2_b, *n2s_g, *n2s_b;
    LinearW qk, qk_src, v, v_src, proj, proj_src, mlp_t0, mlp_t2, mlp_s0, mlp_s2;
};

// workspace shared by the cross blocks of a lane (batch-major, like a stream's)
struct CrossWs {
    float *qk = nullptr, *v = nullptr, *qk_src = nullptr, *v_src = nullptr, *scores_t = nullptr, *cross_partial = nullptr;
    bf16 *ybuf = nullptr, *ysbuf = nullptr;
};

}  // namespace

struct cwm_conj_model {
    Engine eng;
    cwm_conj_config cfg;
    cwm_conj_variant var;  // cwm_conj_create_ex; cwm_conj_create: padded, no dummy token, frames
    StreamW main, ctx;
    float* dummy = nullptr;  // context_stream.encoder.dummy_token [ctx_in_chans][ctx_tubelet] (var.ctx_dummy_token)
    // var.ctx_dummy_token: the call's IMU [B][C][L] + dummy as [B][C][L + tubelet] and its mask + the visible dummy as [B][n + 1]
    float* ctx_stage = nullptr;
    uint8_t* ctx_mask_stage = nullptr;
    std::vector<CrossW> enc_cross, dec_cross;
    // workspace (grown on demand)
    int ws_batch = 0, ws_vmain = 0, ws_vctx = 0;
    StreamWs main_ws, ctx_ws;
    CrossWs cross_ws;
    int* err = nullptr;  // one word per lane
    // batch lanes (cwm_conj_set_lanes; see cwm_model in model.hip)
    int lanes = 2;
    Lanes lane_set;
    // the context (IMU) stream of every lane runs its blocks on a stream of its own between two cross blocks (conj_forward_lane)
    hipStream_t ctx_stream[2] = {nullptr, nullptr};
    hipEvent_t ev_ctx[2] = {nullptr, nullptr}, ev_main[2] = {nullptr, nullptr};
    hipEvent_t ev_cross[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};  // run_cross
    ~cwm_conj_model() {
        for (int i = 0; i < 2; ++i) {
            if (ctx_stream[i]) (void)hipStreamDestroy(ctx_stream[i]);
            if (ev_ctx[i]) (void)hipEventDestroy(ev_ctx[i]);
            if (ev_main[i]) (void)hipEventDestroy(ev_main[i]);
            for (int k = 0; k < 4; ++k)
                if (ev_cross[i][k]) (void)hipEventDestroy(ev_cross[i][k]);
        }
    }
};

namespace {

// One lane's view of the workspace: the slice of every batch-major buffer that lies behind the capacity of the b0 batch elements of the
// lanes before it (the weights are the model's: m->main, m->ctx).
struct ConjLane {
    cwm_conj_model* m;
    StreamWs main, ctx;
    CrossWs cross;
    int* err;
    bool have_prev = false;  // a cross block of this forward has used the projection buffers (run_cross); carried from stage to stage
};

// scratch of the context-side partials: the larger of the two kernel forms' needs (conj_kernels.hip / conj_attention.hip)
size_t cross_partial_floats(int B, int heads, int M, int head_dim) {
    return std::max(cross_attention_partial_floats(B, heads, M, head_dim), cross_attention_mfma_partial_floats(B, heads, M, head_dim));
}

// The layout of the cross blocks' workspace, in elements per batch element (engine.h for_each_stream_buffer has the two streams').
template <typename Visit>
int for_each_cross_buffer(const cwm_conj_model* m, CrossWs& w, Visit&& visit) {
    const size_t N = m->main.n_slots(), M = m->ctx.n_slots(), Dmax = std::max(m->main.enc_dim, m->main.dec_dim), heads = m->cfg.cross_heads;
    int rc;
    if ((rc = visit(w.qk, N * 2 * Dmax)) || (rc = visit(w.v, N * Dmax)) || (rc = visit(w.qk_src, M * 2 * Dmax)) || (rc = visit(w.v_src, M * Dmax)) ||
        (rc = visit(w.scores_t, N * heads * M)) || (rc = visit(w.cross_partial, cross_partial_floats(1, (int)heads, (int)M, (int)(Dmax / heads)))) ||
        (rc = visit(w.ybuf, 2 * N * Dmax)))
        return rc;
    return visit(w.ysbuf, 2 * M * Dmax);
}

// every batch-major buffer of the model: both streams at their visible-row capacities, and the cross blocks'
template <typename Visit>
int for_each_buffer(const cwm_conj_model* m, StreamWs& main, StreamWs& ctx, CrossWs& cross, int vmain_cap, int vctx_cap, Visit&& visit) {
    int rc;
    if ((rc = for_each_stream_buffer(m->main, main, vmain_cap, m->cfg.main.mlp_ratio, false, visit)) ||
        (rc = for_each_stream_buffer(m->ctx, ctx, vctx_cap, m->cfg.main.mlp_ratio, true, visit)))
        return rc;
    return for_each_cross_buffer(m, cross, visit);
}

// offsets at the workspace's capacities (ws_vmain, ws_vctx), whatever the call's counts
ConjLane conj_lane(cwm_conj_model* m, int lane, int b0) {
    ConjLane L{m, m->main_ws, m->ctx_ws, m->cross_ws, m->err + lane};
    (void)for_each_buffer(m, L.main, L.ctx, L.cross, m->ws_vmain, m->ws_vctx, WsShift{(size_t)b0});
    return L;
}

}  // namespace

namespace {

int make_cross(Engine& E, CrossW& C, const std::string& pre, int ci, int cs, int ratio) {
    int rc;
    float** vecs[8] = {&C.n1_g, &C.n1_b, &C.n1s_g, &C.n1s_b, &C.n2_g, &C.n2_b, &C.n2s_g, &C.n2s_b};
    const int dims[8] = {ci, ci, cs, cs, ci, ci, cs, cs};
    const char* names[8] = {"norm1_cross.weight", "norm1_cross.bias", "norm1_src_cross.weight", "norm1_src_cross.bias",
                            "norm2.weight", "norm2.bias", "norm2_src.weight", "norm2_src.bias"};
    for (int i = 0; i < 8; ++i) {
        if ((rc = E.make_vec(vecs[i], dims[i]))) return rc;
        E.add_vec_slot(pre + names[i], *vecs[i], {dims[i]});
    }
    const int D = ci;
    if ((rc = E.make_linear(C.qk, 2 * D, ci, false)) || (rc = E.make_linear(C.qk_src, 2 * D, cs, false)) || (rc = E.make_linear(C.v, D, ci, false)) ||
        (rc = E.make_linear(C.v_src, D, cs, false)) || (rc = E.make_linear(C.proj, ci, D, true)) || (rc = E.make_linear(C.proj_src, cs, D, true)) ||
        (rc = E.make_linear(C.mlp_t0, ratio * ci, ci, true)) || (rc = E.make_linear(C.mlp_t2, ci, ratio * ci, true)) ||
        (rc = E.make_linear(C.mlp_s0, ratio * cs, cs, true)) || (rc = E.make_linear(C.mlp_s2, cs, ratio * cs, true)))
        return rc;
    E.add_matrix_slot(pre + "cross_attention.qk.weight", &C.qk, {2 * D, ci});
    E.add_matrix_slot(pre + "cross_attention.qk_src.weight", &C.qk_src, {2 * D, cs});
    E.add_matrix_slot(pre + "cross_attention.v.weight", &C.v, {D, ci});
    E.add_matrix_slot(pre + "cross_attention.v_src.weight", &C.v_src, {D, cs});
    E.add_matrix_slot(pre + "cross_attention.projection.weight", &C.proj, {ci, D});
    E.add_vec_slot(pre + "cross_attention.projection.bias", C.proj.bias, {ci});
    E.add_matrix_slot(pre + "cross_attention.projection_src.weight", &C.proj_src, {cs, D});
    E.add_vec_slot(pre + "cross_attention.projection_src.bias", C.proj_src.bias, {cs});
    E.add_matrix_slot(pre + "mlp.trg.layers.0.weight", &C.mlp_t0, {ratio * ci, ci});
    E.add_vec_slot(pre + "mlp.trg.layers.0.bias", C.mlp_t0.bias, {ratio * ci});
    E.add_matrix_slot(pre + "mlp.trg.layers.2.weight", &C.mlp_t2, {ci, ratio * ci});
    E.add_vec_slot(pre + "mlp.trg.layers.2.bias", C.mlp_t2.bias, {ci});
    E.add_matrix_slot(pre + "mlp.src.layers.0.weight", &C.mlp_s0, {ratio * cs, cs});
    E.add_vec_slot(pre + "mlp.src.layers.0.bias", C.mlp_s0.bias, {ratio * cs});
    E.add_matrix_slot(pre + "mlp.src.layers.2.weight", &C.mlp_s2, {cs, ratio * cs});
    E.add_vec_slot(pre + "mlp.src.layers.2.bias", C.mlp_s2.bias, {cs});
    return 0;
}

int ensure_workspace(cwm_conj_model* m, int B, int vmain, int vctx) {
    if (m->ws_batch > 0 && B <= m->ws_batch && vmain <= m->ws_vmain && vctx <= m->ws_vctx) return 0;
    Engine& E = m->eng;
    const int Bc = std::max(B, m->ws_batch), vm = std::max(vmain, m->ws_vmain), vc = std::max(vctx, m->ws_vctx);
    m->ws_batch = 0;  // (nothing is usable until all of it is there again)
    int rc;
    if ((rc = E.free_workspace()) || (rc = for_each_buffer(m, m->main_ws, m->ctx_ws, m->cross_ws, vm, vc, WsAlloc{E, (size_t)Bc}))) return rc;
    // `err` is not linear in the batch size (one word per lane: 4 words, lane l at err + l), so it is not part of the layout; nor are the staging
    // buffers of the whole call's context input, which no lane owns a slice of (the lanes read them as they read the caller's inputs)
    if ((rc = E.ws(&m->err, 4))) return rc;
    if (m->var.ctx_dummy_token &&
        ((rc = E.ws(&m->ctx_stage, (size_t)Bc * m->cfg.ctx_in_chans * (m->cfg.ctx_seq_len + m->cfg.ctx_tubelet))) || (rc = E.ws(&m->ctx_mask_stage, (size_t)Bc * m->ctx.n_tok))))
        return rc;
    m->ws_batch = Bc;
    m->ws_vmain = vm;
    m->ws_vctx = vc;
    // (the zero fills above ran on the null stream; the lane streams are non-blocking and would not wait for them)
    CWM_HIP_CHECK(hipDeviceSynchronize());
    return 0;
}

// CrossAttentionTransformerBlock.forward (transformer.py:559-583) with with_self_attention=False.
//
// s = the lane's stream (RGB side), sc = the lane's context stream (== s: everything in order on one stream).  With two streams and the
// MFMA kernels the block runs as two chains that meet once:
//     s :  LN(x) -> qk, v projections ---+--> role A (y = softmax_M . v_src) -> x += proj(y) -> LN2 -> MLP_trg
//     sc:  LN(src) -> qk_src, v_src -----+--> role B + combine (y_src = softmax_N . v) -> src += proj_src(y_src) -> LN2 -> MLP_src
// (+: each stream waits for the other one's projections).  The two roles stream disjoint halves of the RGB-side projections and run
// concurrently; the ~10 tiny context-side launches leave the lane's stream.  ev[0..3] = {s projections done, sc projections done, role A
// done, role B done}: the last two guard the projection buffers against the NEXT cross block of the lane (role B reads qk / v that the
// next block's projections on s overwrite, role A reads qk_src / v_src that the next block overwrites on sc).
int run_cross(ConjLane& L, const CrossW& C, float* x, int N, int ci, float* src, int M, int cs, int B, int planes, hipStream_t s, hipStream_t sc,
              hipEvent_t* ev, bool& have_prev) {
    cwm_conj_model* m = L.m;
    Engine& E = m->eng;
    const int D = ci, heads = m->cfg.cross_heads, hd = D / heads;
    const int rows = B * N, rows_s = B * M;
    int rc;
    // main-stream projections: operand layout (bf16 hi [, lo] planes, the same 4 bytes per element as fp32) for the MFMA kernel
    const bool mfma = E.tune.conj_attn && cross_attention_mfma_ok(hd, M) && cross_attention_mfma_fits(B, N, heads, hd) && (2 * D) % 32 == 0;
    const bool two = sc != s && mfma;
    if (sc != s && !two) {  // VALU fallback: one chain on s, bracketed by the context stream
        CWM_HIP_CHECK(hipEventRecord(ev[1], sc));
        CWM_HIP_CHECK(hipStreamWaitEvent(s, ev[1], 0));
    }
    hipStream_t const t = two ? sc : s;  // where the context side runs
    if (two && have_prev) {
        CWM_HIP_CHECK(hipStreamWaitEvent(s, ev[3], 0));  // the previous block's role B has read qk / v
        CWM_HIP_CHECK(hipStreamWaitEvent(sc, ev[2], 0));  // ... its role A has read qk_src / v_src
    }
    if ((rc = E.layernorm_to(x, rows, ci, C.n1_g, C.n1_b, L.main.sb.hbuf, planes, s))) return rc;
    if (mfma) {
        if ((rc = E.linear_operand(L.main.sb.hbuf, rows, ci, C.qk, reinterpret_cast<bf16*>(L.cross.qk), planes, s))) return rc;
        if ((rc = E.linear_operand(L.main.sb.hbuf, rows, ci, C.v, reinterpret_cast<bf16*>(L.cross.v), planes, s))) return rc;
    } else {
        if ((rc = E.linear_f32(L.main.sb.hbuf, rows, ci, C.qk, L.cross.qk, nullptr, planes, s))) return rc;
        if ((rc = E.linear_f32(L.main.sb.hbuf, rows, ci, C.v, L.cross.v, nullptr, planes, s))) return rc;
    }
    if ((rc = E.layernorm_to(src, rows_s, cs, C.n1s_g, C.n1s_b, L.ctx.sb.hbuf, planes, t))) return rc;
    if ((rc = E.linear_f32(L.ctx.sb.hbuf, rows_s, cs, C.qk_src, L.cross.qk_src, nullptr, planes, t))) return rc;
    if ((rc = E.linear_f32(L.ctx.sb.hbuf, rows_s, cs, C.v_src, L.cross.v_src, nullptr, planes, t))) return rc;
    if (two) {
        CWM_HIP_CHECK(hipEventRecord(ev[0], s));
        CWM_HIP_CHECK(hipEventRecord(ev[1], sc));
        CWM_HIP_CHECK(hipStreamWaitEvent(sc, ev[0], 0));
        CWM_HIP_CHECK(hipStreamWaitEvent(s, ev[1], 0));
    }
    CrossAttnParams ca;
    memset(&ca, 0, sizeof(ca));
    ca.qk = L.cross.qk; ca.v = L.cross.v; ca.qk_op = reinterpret_cast<const bf16*>(L.cross.qk); ca.v_op = reinterpret_cast<const bf16*>(L.cross.v); ca.qk_src = L.cross.qk_src; ca.v_src = L.cross.v_src; ca.B = B; ca.N = N; ca.M = M; ca.heads = heads; ca.head_dim = hd;
    ca.scale = 1.0f / sqrtf((float)hd);
    ca.y = L.cross.ybuf; ca.y_plane = (int64_t)rows * D; ca.y_src = L.cross.ysbuf; ca.y_src_plane = (int64_t)rows_s * D; ca.scores_t = L.cross.scores_t; ca.partial = L.cross.cross_partial;
    if (two) {
        if ((rc = launch_cross_attention_mfma_roles(ca, planes, s, sc, 1))) return rc;
        CWM_HIP_CHECK(hipEventRecord(ev[2], s));
        if ((rc = launch_cross_attention_mfma_roles(ca, planes, s, sc, 2))) return rc;
        CWM_HIP_CHECK(hipEventRecord(ev[3], sc));
        have_prev = true;
    } else {
        // both directions: 2 x (scores 2 N M hd + P.V 2 N M hd) FLOP per head
        if ((rc = E.timed(CWM_KCLASS_CROSS_ATTN, 8.0 * (double)B * heads * N * M * hd, s,
                          [&] { return mfma ? launch_cross_attention_mfma(ca, planes, s) : launch_cross_attention(ca, planes, s); })))
            return rc;
    }
    if ((rc = E.linear_f32(L.cross.ybuf, rows, D, C.proj, x, x, planes, s))) return rc;          // x += proj(y) + b
    if ((rc = E.run_mlp(C.n2_g, C.n2_b, C.mlp_t0, C.mlp_t2, x, B, N, ci, planes, L.main.sb, s))) return rc;
    if ((rc = E.linear_f32(L.cross.ysbuf, rows_s, D, C.proj_src, src, src, planes, t))) return rc;
    if ((rc = E.run_mlp(C.n2s_g, C.n2s_b, C.mlp_s0, C.mlp_s2, src, B, M, cs, planes, L.ctx.sb, t))) return rc;
    if (sc != s && !two) {  // VALU fallback: the context stream continues behind the whole block
        CWM_HIP_CHECK(hipEventRecord(ev[0], s));
        CWM_HIP_CHECK(hipStreamWaitEvent(sc, ev[0], 0));
    }
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int cwm_conj_create(const cwm_conj_config* cfg, cwm_conj_model** out) { return cwm_conj_create_ex(cfg, nullptr, out); }

extern "C" int cwm_conj_create_ex(const cwm_conj_config* cfg, const cwm_conj_variant* variant, cwm_conj_model** out) {
    CWM_REQUIRE(cfg && out, "cwm_conj_create: null argument");
    const cwm_conj_config& c = *cfg;
    const cwm_config& mc = c.main;
    cwm_conj_variant v;
    memset(&v, 0, sizeof(v));
    v.padded = 1;
    if (variant) {
        CWM_REQUIRE(variant->struct_size >= offsetof(cwm_conj_variant, padded) + sizeof(int32_t) && variant->struct_size <= 4096,
                    "cwm_conj_create_ex: variant->struct_size = %u is not a cwm_conj_variant", variant->struct_size);
        memcpy(&v, variant, std::min<size_t>(variant->struct_size, sizeof(v)));
    }
    v.struct_size = sizeof(v);
    CWM_REQUIRE(v.padded == 0 || v.padded == 1, "cwm_conj_create_ex: padded must be 0 or 1");
    CWM_REQUIRE(v.ctx_dummy_token == 0 || v.ctx_dummy_token == 1, "cwm_conj_create_ex: ctx_dummy_token must be 0 or 1");
    CWM_REQUIRE(v.main_input == CWM_CONJ_INPUT_FRAMES || v.main_input == CWM_CONJ_INPUT_FLOWBACK_RGB01, "cwm_conj_create_ex: unknown main_input %d", v.main_input);
    // the two models the reference ships: the padded IMU-conditioned predictor and the unpadded flow -> IMU predictor (a padded
    // model with the dummy token would put null_token_dec after the dummy's position row, which the reference never defines)
    CWM_REQUIRE((v.padded && !v.ctx_dummy_token && v.main_input == CWM_CONJ_INPUT_FRAMES) ||
                    (!v.padded && v.ctx_dummy_token && v.main_input == CWM_CONJ_INPUT_FLOWBACK_RGB01),
                "cwm_conj_create_ex: supported variants are {padded, no dummy token, frames} and {unpadded, dummy token, flowback_rgb01}");
    CWM_REQUIRE(v.padded || (c.main_max_pad == 0 && c.ctx_max_pad == 0), "cwm_conj_create_ex: an unpadded model needs main_max_pad = ctx_max_pad = 0");
    CWM_REQUIRE(v.main_input != CWM_CONJ_INPUT_FLOWBACK_RGB01 || (mc.in_chans == 7 && mc.num_frames == 1),
                "cwm_conj_create_ex: the flowback_rgb01 input needs main.in_chans = 7 and main.num_frames = 1");
    const int ctx_tokens = c.ctx_tubelet > 0 ? c.ctx_seq_len / c.ctx_tubelet + v.ctx_dummy_token : 0;
    CWM_REQUIRE(mc.patch > 0 && mc.patch % 4 == 0 && mc.img_h % mc.patch == 0 && mc.img_w % mc.patch == 0 && mc.img_w % 4 == 0, "bad image/patch size");
    CWM_REQUIRE(mc.enc_dim == 64 * mc.enc_heads && mc.dec_dim == 64 * mc.dec_heads, "main stream needs head_dim 64");
    CWM_REQUIRE(mc.enc_dim % 128 == 0 && mc.dec_dim % 128 == 0 && mc.enc_dim <= 1024, "main stream widths must be multiples of 128");
    CWM_REQUIRE(c.ctx_tubelet > 0 && c.ctx_seq_len % c.ctx_tubelet == 0 && ctx_tokens + c.ctx_max_pad <= 64, "context stream: at most 64 tokens incl. padding");
    CWM_REQUIRE(c.ctx_enc_dim % c.ctx_enc_heads == 0 && c.ctx_dec_dim % c.ctx_dec_heads == 0 && c.ctx_enc_dim / c.ctx_enc_heads <= 64 &&
                    c.ctx_dec_dim / c.ctx_dec_heads <= 64, "context stream head_dim must be <= 64");
    CWM_REQUIRE(c.ctx_enc_dim % 16 == 0 && c.ctx_dec_dim % 16 == 0 && c.ctx_enc_dim <= 1024, "context widths must be multiples of 16");
    CWM_REQUIRE(c.cross_heads > 0 && mc.enc_dim / c.cross_heads <= 192 && mc.enc_dim % c.cross_heads == 0 && mc.dec_dim % c.cross_heads == 0, "cross attention head_dim must be <= 192");
    CWM_REQUIRE(c.n_enc_cross >= 0 && c.n_enc_cross <= 16 && c.n_dec_cross >= 0 && c.n_dec_cross <= 16, "too many conjoining blocks");
    cwm_conj_model* m = new cwm_conj_model();
    m->cfg = c;
    m->var = v;
    Engine& E = m->eng;
    E.ln_eps = mc.ln_eps;
    CWM_HIP_CHECK(hipGetDevice(&E.device));
    StreamW& A = m->main;
    A.enc_dim = mc.enc_dim; A.dec_dim = mc.dec_dim; A.enc_heads = mc.enc_heads; A.dec_heads = mc.dec_heads;
    A.n_tok = (mc.img_h / mc.patch) * (mc.img_w / mc.patch) * mc.num_frames; A.max_pad = c.main_max_pad; A.out_dim = mc.in_chans * mc.patch * mc.patch;
    StreamW& S = m->ctx;
    S.enc_dim = c.ctx_enc_dim; S.dec_dim = c.ctx_dec_dim; S.enc_heads = c.ctx_enc_heads; S.dec_heads = c.ctx_dec_heads;
    S.n_tok = ctx_tokens; S.max_pad = c.ctx_max_pad; S.out_dim = c.ctx_in_chans * c.ctx_tubelet;
    int rc = 0;
    do {
        if ((rc = E.make_stream(A, "main_stream.", mc.in_chans * mc.patch * mc.patch, {mc.enc_dim, mc.in_chans, 1, mc.patch, mc.patch}, mc.enc_depth,
                              mc.dec_depth, mc.mlp_ratio, true, v.padded)))
            break;
        if ((rc = E.make_stream(S, "context_stream.", c.ctx_in_chans * c.ctx_tubelet, {c.ctx_enc_dim, c.ctx_in_chans, c.ctx_tubelet, 1, 1}, mc.enc_depth,
                              mc.dec_depth, mc.mlp_ratio, false, v.padded)))
            break;
        if (v.ctx_dummy_token) {  // ImuEncoder.dummy_token, registered between context_stream.mask_token and the patch embed
            if ((rc = E.make_vec(&m->dummy, c.ctx_in_chans * c.ctx_tubelet))) break;
            E.add_vec_slot("context_stream.encoder.dummy_token", m->dummy, {1, c.ctx_in_chans, c.ctx_tubelet, 1, 1});
        }
        // loaded from the checkpoints but never used on this path (vmae.py:368-369)
        E.add_ignored_slot("context_stream.pos_embed_encoder.weight", {c.ctx_dec_dim, 2 * c.ctx_dec_dim});
        E.add_ignored_slot("context_stream.pos_embed_encoder.bias", {c.ctx_dec_dim});
        m->enc_cross.resize(c.n_enc_cross);
        m->dec_cross.resize(c.n_dec_cross);
        for (int i = 0; i < c.n_enc_cross && !rc; ++i) {
            const std::string k = std::to_string(c.enc_cross[i]);
            rc = make_cross(E, m->enc_cross[i], "encoder_conjoining_blocks." + k + "-" + k + ".", mc.enc_dim, c.ctx_enc_dim, c.cross_mlp_ratio);
        }
        for (int i = 0; i < c.n_dec_cross && !rc; ++i) {
            const std::string k = std::to_string(c.dec_cross[i]);
            rc = make_cross(E, m->dec_cross[i], "decoder_conjoining_blocks." + k + "-" + k + ".", mc.dec_dim, c.ctx_dec_dim, c.cross_mlp_ratio);
        }
    } while (0);
    if (rc) {
        delete m;
        return rc;
    }
    *out = m;
    return CWM_OK;
}

extern "C" void cwm_conj_destroy(cwm_conj_model* m) { delete m; }

extern "C" int cwm_conj_load_weight(cwm_conj_model* m, const char* key, const float* data, int on_device, const int64_t* shape, int ndim) {
    CWM_REQUIRE(m, "cwm_conj_load_weight: null model");
    return m->eng.load_weight(key, data, on_device, shape, ndim);
}

extern "C" int cwm_conj_missing_weights(cwm_conj_model* m, char* buf, int buflen) { return m->eng.missing_weights(buf, buflen); }

// One lane: batch elements [b0, b0 + B) of the call on stream s.
//
// The context (IMU) stream is a chain of ~300 tiny launches (25 / 50 tokens per sample: 5-15 us each, latency-bound) that only meets
// the RGB stream in the 8 cross blocks.  It runs on a stream of its own (sc), so that the chain hides under the RGB stream's kernels
// instead of extending the lane by ~4 %; inside a cross block the two streams exchange their projections once (run_cross).
// (Not while kernel timers are on: those want every launch alone on the chip.)
// Stages [stage_lo, stage_hi) of the lane's launch sequence: 0 = masks + tokenisation + embedding of both streams; 1 .. Le = encoder step i (the cross block in front of
// block i, then block i of both streams); Le + 1 = the two to_decoder steps; Le + 2 .. Le + 1 + Ld = decoder step i; Le + Ld + 2 = outputs.  cwm_conj_forward issues stage by
// stage over the lanes, as cwm_forward does: a forward is ~1000 launches per lane, and a host that issues lane 0 to its end first starts lane 1 that much later -- 1.5 ms of
// 61 normally, but 22 ms under rocprofv3 (whose launches cost ~20 us each: the lanes of the round-4 trace overlapped for half of their time only).  Measured without the
// profiler: no difference (61.2 ms per step either way; this model's step is the sum of its kernels -- 62.6 ms of kernel time in the one-lane trace).
static int conj_forward_lane(ConjLane& L, const cwm_conj_forward_args* a, int b0, int B, hipStream_t s, int lane, int stage_lo, int stage_hi) {
    cwm_conj_model* m = L.m;
    const cwm_conj_config& c = m->cfg;
    const cwm_config& mc = c.main;
    const StreamW &A = m->main, &S = m->ctx;
    StreamWs &Aw = L.main, &Sw = L.ctx;
    const int vm = a->n_vis_max, vc = a->n_vis_ctx_max;
    const int Nx = A.n_slots(), Mx = S.n_slots();
    const int n_out = Nx - vm;
    Engine& E = m->eng;
    const int planes = a->mode == CWM_MODE_PARITY ? 2 : 1;
    const float* x_in = a->x_dev + (int64_t)b0 * a->x_stride_b;
    const uint8_t* mask_in = a->mask_dev + (size_t)b0 * A.n_tok;
    const int ctx_len = S.n_tok * c.ctx_tubelet;  // (+ the dummy's samples: a->ctx_dev is then the engine's staging buffer)
    const float* ctx_in = a->ctx_dev + (size_t)b0 * c.ctx_in_chans * ctx_len;
    const uint8_t* ctx_mask_in = a->ctx_mask_dev + (size_t)b0 * S.n_tok;
    float* y_tokens = a->y_tokens_dev ? a->y_tokens_dev + (size_t)b0 * n_out * A.out_dim : nullptr;
    int rc;
    bool side = E.tune.conj_ctx_stream != 0;  // (0 keeps the context stream's blocks on the lane's own stream)
    for (int k = 0; k < CWM_KCLASS_COUNT; ++k) side = side && !E.timers[k].enabled;
    if (side && !m->ctx_stream[lane]) {
        CWM_HIP_CHECK(hipStreamCreateWithFlags(&m->ctx_stream[lane], hipStreamNonBlocking));
        CWM_HIP_CHECK(hipEventCreateWithFlags(&m->ev_ctx[lane], hipEventDisableTiming));
        CWM_HIP_CHECK(hipEventCreateWithFlags(&m->ev_main[lane], hipEventDisableTiming));
        for (int k = 0; k < 4; ++k) CWM_HIP_CHECK(hipEventCreateWithFlags(&m->ev_cross[lane][k], hipEventDisableTiming));
    }
    bool& have_prev = L.have_prev;
    auto in_range = [&](int st) { return st >= stage_lo && st < stage_hi; };
    const int st_todec = mc.enc_depth + 1, st_out = mc.enc_depth + mc.dec_depth + 2;
    hipStream_t sc = side ? m->ctx_stream[lane] : s;
    // main -> ctx: the context stream may continue once everything queued on s so far is done; ctx -> main likewise
    auto ctx_follows_main = [&]() -> int {
        if (!side) return 0;
        CWM_HIP_CHECK(hipEventRecord(m->ev_main[lane], s));
        CWM_HIP_CHECK(hipStreamWaitEvent(sc, m->ev_main[lane], 0));
        return 0;
    };
    auto main_follows_ctx = [&]() -> int {
        if (!side) return 0;
        CWM_HIP_CHECK(hipEventRecord(m->ev_ctx[lane], sc));
        CWM_HIP_CHECK(hipStreamWaitEvent(s, m->ev_ctx[lane], 0));
        return 0;
    };

    if (in_range(0)) {
    have_prev = false;
    // a13: padded masks -> permutations [visible slots ascending | masked slots ascending] over n_tok + max_pad slots
    CWM_HIP_CHECK(hipMemsetAsync(L.err, 0, sizeof(int), s));
    if ((rc = launch_pad_mask(mask_in, B, A.n_tok, A.max_pad, vm, Aw.ext_mask, s))) return rc;
    if ((rc = launch_mask_to_perm(Aw.ext_mask, B, Nx, vm, Aw.perm, L.err, s))) return rc;
    if ((rc = launch_pad_mask(ctx_mask_in, B, S.n_tok, S.max_pad, vc, Sw.ext_mask, s))) return rc;
    if ((rc = launch_mask_to_perm(Sw.ext_mask, B, Mx, vc, Sw.perm, L.err, s))) return rc;

    // a2/a14: tokenise both streams (visible slots only)
    if (m->var.main_input == CWM_CONJ_INPUT_FLOWBACK_RGB01) {
        FlowRgbGatherParams fg;
        memset(&fg, 0, sizeof(fg));
        fg.fwd = a->flow_fwd_dev + b0 * a->flow_fwd_stride_b; fg.f_sb = a->flow_fwd_stride_b; fg.f_sc = a->flow_fwd_stride_c;
        fg.bwd = a->flow_bwd_dev + b0 * a->flow_bwd_stride_b; fg.b_sb = a->flow_bwd_stride_b; fg.b_sc = a->flow_bwd_stride_c;
        fg.x = x_in; fg.sb = a->x_stride_b; fg.sc = a->x_stride_c; fg.normalize = a->normalize;
        fg.H = mc.img_h; fg.W = mc.img_w; fg.P = mc.patch; fg.perm = Aw.perm; fg.Nt = A.n_tok; fg.perm_stride = Nx; fg.n_rows = vm; fg.B = B;
        fg.out = Aw.tokens_in; fg.out_plane = (int64_t)B * vm * A.embed_kpad; fg.ld = A.embed_kpad;
        if ((rc = E.timed(CWM_KCLASS_PATCH_GATHER, (double)B * vm * 7 * mc.patch * mc.patch * (4.0 + 2.0 * planes), s,
                          [&] { return launch_flow_rgb_gather(fg, planes, s); })))
            return rc;
    } else {
        PatchGatherParams pg;
        memset(&pg, 0, sizeof(pg));
        pg.x = x_in; pg.sb = a->x_stride_b; pg.sc = a->x_stride_c; pg.st = a->x_stride_t; pg.normalize = a->normalize;
        pg.C = mc.in_chans; pg.H = mc.img_h; pg.W = mc.img_w; pg.P = mc.patch; pg.perm = Aw.perm; pg.Nt = A.n_tok; pg.perm_stride = Nx; pg.n_rows = vm; pg.B = B;
        pg.out = Aw.tokens_in; pg.out_plane = (int64_t)B * vm * A.embed_kpad; pg.ld = A.embed_kpad;
        if ((rc = E.run_patch_gather(pg, planes, s))) return rc;
    }
    if ((rc = E.embed_stream(A, Aw, B, vm, planes, s))) return rc;
    ImuGatherParams ig;
    memset(&ig, 0, sizeof(ig));
    ig.imu = ctx_in; ig.B = B; ig.C = c.ctx_in_chans; ig.L = ctx_len; ig.tubelet = c.ctx_tubelet; ig.perm = Sw.perm; ig.perm_stride = Mx;
    ig.n_rows = vc; ig.n_real = S.n_tok; ig.out = Sw.tokens_in; ig.out_plane = (int64_t)B * vc * S.embed_kpad; ig.ld = S.embed_kpad;
    if ((rc = launch_imu_gather(ig, planes, s))) return rc;
    if ((rc = E.embed_stream(S, Sw, B, vc, planes, s))) return rc;
    if ((rc = ctx_follows_main())) return rc;
    }

    // encoder: cross block BEFORE the self-attention blocks listed in enc_cross (forward_encoder_blocks :543-576)
    for (int i = 0; i < mc.enc_depth; ++i) {
        if (!in_range(1 + i)) continue;
        for (int k = 0; k < c.n_enc_cross; ++k)
            if (c.enc_cross[k] == i &&
                (rc = run_cross(L, m->enc_cross[k], Aw.x_enc, vm, A.enc_dim, Sw.x_enc, vc, S.enc_dim, B, planes, s, sc, m->ev_cross[lane], have_prev)))
                return rc;
        if ((rc = E.run_block(A.enc[i], Aw.x_enc, B, vm, A.enc_dim, A.enc_heads, planes, Aw.sb, s))) return rc;
        if ((rc = E.run_block_small(S.enc[i], Sw.x_enc, B, vc, S.enc_dim, S.enc_heads, planes, Sw.sb, sc))) return rc;
    }
    if (in_range(st_todec) && ((rc = E.to_decoder(A, Aw, B, vm, planes, s)) || (rc = E.to_decoder(S, Sw, B, vc, planes, sc)))) return rc;

    // decoder: cross block AFTER the blocks listed in dec_cross (forward_decoder_blocks :688-720)
    for (int i = 0; i < mc.dec_depth; ++i) {
        if (!in_range(st_todec + 1 + i)) continue;
        if ((rc = E.run_block(A.dec[i], Aw.x_dec, B, Nx, A.dec_dim, A.dec_heads, planes, Aw.sb, s))) return rc;
        if ((rc = E.run_block_small(S.dec[i], Sw.x_dec, B, Mx, S.dec_dim, S.dec_heads, planes, Sw.sb, sc))) return rc;
        for (int k = 0; k < c.n_dec_cross; ++k)
            if (c.dec_cross[k] == i &&
                (rc = run_cross(L, m->dec_cross[k], Aw.x_dec, Nx, A.dec_dim, Sw.x_dec, Mx, S.dec_dim, B, planes, s, sc, m->ev_cross[lane], have_prev)))
                return rc;
    }
    if (!in_range(st_out)) return CWM_OK;
    // context output (forward(..., output_context=True), conjoined_decode :990-1002): head_ctx(norm_ctx(x_c[:, -n_out_c:])) * ~null_mask_ctx
    if (a->y_ctx_tokens_dev) {
        const int n_out_c = Mx - vc;
        float* y_ctx = a->y_ctx_tokens_dev + (size_t)b0 * n_out_c * S.out_dim;
        if ((rc = E.head_rows(S, Sw, B, n_out_c, y_ctx, planes, sc))) return rc;
        if ((rc = launch_zero_pad_out_rows(y_ctx, Sw.perm, B, Mx, vc, n_out_c, S.n_tok, S.out_dim, sc))) return rc;
    }
    if ((rc = main_follows_ctx())) return rc;  // the call's stream semantics cover the context stream's work too

    // main output: head(norm(x[:, -n_out:])) * ~null_mask   (conjoined_decode :984-1002); the flow -> IMU model may skip it
    if (!y_tokens || n_out == 0) return CWM_OK;
    if ((rc = E.head_rows(A, Aw, B, n_out, y_tokens, planes, s))) return rc;
    return launch_zero_pad_out_rows(y_tokens, Aw.perm, B, Nx, vm, n_out, A.n_tok, A.out_dim, s);
}

extern "C" int cwm_conj_forward(cwm_conj_model* m, const cwm_conj_forward_args* a_in) {
    CWM_REQUIRE(m && a_in, "cwm_conj_forward: null argument");
    cwm_conj_forward_args a_copy;
    if (int rc = copy_args(a_copy, a_in, offsetof(cwm_conj_forward_args, stream) + sizeof(void*), "cwm_conj_forward")) return rc;
    const cwm_conj_forward_args* a = &a_copy;
    if (int rc = cwm_require_device(m->eng.device, "cwm_conj_forward")) return rc;
    const bool flowback = m->var.main_input == CWM_CONJ_INPUT_FLOWBACK_RGB01;
    CWM_REQUIRE(a->x_dev && a->mask_dev && a->ctx_dev && a->ctx_mask_dev && (a->y_tokens_dev || flowback),
                "cwm_conj_forward: x, mask, context, context mask and y are required");
    CWM_REQUIRE(!flowback || (a->flow_fwd_dev && a->flow_bwd_dev), "cwm_conj_forward: the flowback_rgb01 input needs flow_fwd_dev and flow_bwd_dev");
    CWM_REQUIRE(a->y_tokens_dev || a->y_ctx_tokens_dev, "cwm_conj_forward: no output requested");
    CWM_REQUIRE(a->mode == CWM_MODE_FAST || a->mode == CWM_MODE_PARITY, "cwm_conj_forward: bad mode %d", a->mode);
    const int B = a->batch, vm = a->n_vis_max, vc = a->n_vis_ctx_max;
    const int Nx = m->main.n_slots();
    // (unpadded: a fully visible main stream is allowed when only the context output is asked for -- the decoder then has Nm = 0)
    CWM_REQUIRE(B > 0 && vm > 0 && (vm < Nx || (!m->var.padded && !(a->y_tokens_dev && vm == Nx))) && vc > 0 && vc <= m->ctx.n_tok,
                "cwm_conj_forward: bad batch / visible counts (%d, %d, %d)", B, vm, vc);
    if (int rc = m->eng.require_weights("cwm_conj_forward")) return rc;
    if (int rc = ensure_workspace(m, B, vm, vc)) return rc;
    hipStream_t s = (hipStream_t)a->stream;
    if (m->var.ctx_dummy_token) {  // the lanes read the IMU and its mask with the dummy token appended, from the engine's staging buffers
        const cwm_conj_config& c = m->cfg;
        if (int rc = launch_imu_append_dummy(a->ctx_dev, a->ctx_mask_dev, m->dummy, B, c.ctx_in_chans, c.ctx_seq_len, c.ctx_tubelet, m->ctx.n_tok - 1, m->ctx_stage,
                                             m->ctx_mask_stage, s))
            return rc;
        a_copy.ctx_dev = m->ctx_stage;
        a_copy.ctx_mask_dev = m->ctx_mask_stage;
    }

    // two lanes as in cwm_forward (model.hip): the halves share n_vis_max / n_vis_ctx_max, so the padded layout of every row is unchanged
    const bool two = m->lanes >= 2 && B >= 2 && (int64_t)(B / 2) * vm >= (m->eng.tune.min_lane_rows > 0 ? m->eng.tune.min_lane_rows : kMinLaneRowsConj);
    const int B0 = two ? (B + 1) / 2 : B;
    if (int rc = m->lane_set.fork(s, two ? 2 : 1)) return rc;
    ConjLane lanes[2] = {conj_lane(m, 0, 0), conj_lane(m, 1, two ? B0 : 0)};
    m->eng.overlapped = two;
    int rc = 0;
    // launch order: stage by stage over the lanes (conj_forward_lane), so that both queues fill at the same pace
    const int n_stages = m->cfg.main.enc_depth + m->cfg.main.dec_depth + 3;
    for (int st = 0; st < n_stages && !rc; ++st) {
        rc = conj_forward_lane(lanes[0], a, 0, B0, s, 0, st, st + 1);
        if (two && !rc) rc = conj_forward_lane(lanes[1], a, B0, B - B0, m->lane_set.stream(1, s), 1, st, st + 1);
    }
    m->eng.overlapped = 0;
    if (int jrc = m->lane_set.join(s)) return jrc;  // (even after a failed launch)
    if (rc) return rc;

    if (a->check) {
        int herr[2] = {0, 0};
        CWM_HIP_CHECK(hipMemcpyAsync(herr, m->err, (two ? 2 : 1) * sizeof(int), hipMemcpyDeviceToHost, s));
        CWM_HIP_CHECK(hipStreamSynchronize(s));
        if ((herr[0] || herr[1]) && !m->var.padded) {
            cwm_set_error("unpadded model: every row needs exactly n_vis_max visible main tokens and n_vis_ctx_max visible context tokens");
            return CWM_ERR_INVALID;
        }
        if (herr[0] || herr[1]) {
            cwm_set_error("n_vis_max / n_vis_ctx_max do not match the masks (a row has more visible tokens, or the padding budget is exceeded)");
            return CWM_ERR_MASK;
        }
    }
    return CWM_OK;
}

extern "C" int cwm_conj_set_option(cwm_conj_model* m, const char* key, int value) {
    CWM_REQUIRE(m && key, "cwm_conj_set_option: null argument");
    return m->eng.set_option("cwm_conj_set_option", key, value);
}

extern "C" int cwm_conj_set_lanes(cwm_conj_model* m, int lanes) {
    CWM_REQUIRE(m && (lanes == 1 || lanes == 2), "cwm_conj_set_lanes: lanes must be 1 or 2");
    m->lanes = lanes;
    return CWM_OK;
}

extern "C" int cwm_conj_timing_enable(cwm_conj_model* m, int kclass, int enable) {
    CWM_REQUIRE(m, "cwm_conj_timing_enable: null model");
    return m->eng.timing_enable(kclass, enable);
}

extern "C" int cwm_conj_timing_collect(cwm_conj_model* m, int kclass, cwm_kernel_stats* out) {
    CWM_REQUIRE(m, "cwm_conj_timing_collect: null model");
    return m->eng.timing_collect(kclass, out);
}
