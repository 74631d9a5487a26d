// Development library (libcwm_hip_dev.so = every object of libcwm_hip.so + this file; include/cwm_hip_dev.h): the switches, per-shape tile
// overrides, micro-benchmarks on random operands and profiling queries that tools/ and the bitwise cross-checks of the test suite use.  None of
// it is linked into the production library.  cwm_debug_set changes THIS THREAD's copy of the execution options (kernels.h thread_tuning):
// the stand-alone entry points called on the thread afterwards use it, model handles created on the thread afterwards start from it; a model
// that already exists is changed through cwm_model_set_option / cwm_conj_set_option, which the production library has too.
#include <atomic>
#include <map>
#include <mutex>
#include <tuple>

#include "../../include/cwm_hip_dev.h"
#include "engine.h"
#include "flow_view.h"

using namespace cwm;

void cwm_set_pretend_device(int d);  // engine.hip

namespace {
__global__ void fill_random_bf16_kernel(bf16* dst, int64_t n, unsigned seed, float scale) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned x = (unsigned)i * 2654435761u + seed;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    dst[i] = (bf16)(((float)(x & 0xFFFF) / 32768.0f - 1.0f) * scale);
}
__global__ void fill_random_f32_kernel(float* dst, int64_t n, unsigned seed, float scale) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned x = (unsigned)i * 2654435761u + seed;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    dst[i] = ((float)(x & 0xFFFF) / 32768.0f - 1.0f) * scale;
}
void fill_bf16(bf16* d, int64_t n, unsigned seed, float scale) {
    hipLaunchKernelGGL(fill_random_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d, n, seed, scale);
}
void fill_f32(float* d, int64_t n, unsigned seed, float scale) {
    hipLaunchKernelGGL(fill_random_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d, n, seed, scale);
}
// *avg_us = the mean time of `iters` calls of launch() on `stream` after 3 warm-up calls; the two events are destroyed on every path
template <typename F>
int time_launches(int iters, hipStream_t stream, F&& launch, double* avg_us) {
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } ev;
    CWM_HIP_CHECK(hipEventCreate(&ev.e0));
    CWM_HIP_CHECK(hipEventCreate(&ev.e1));
    for (int i = 0; i < 3; ++i)
        if (int rc = launch()) return rc;
    CWM_HIP_CHECK(hipEventRecord(ev.e0, stream));
    for (int i = 0; i < iters; ++i)
        if (int rc = launch()) return rc;
    CWM_HIP_CHECK(hipEventRecord(ev.e1, stream));
    CWM_HIP_CHECK(hipEventSynchronize(ev.e1));
    float ms = 0.f;
    CWM_HIP_CHECK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *avg_us = 1e3 * ms / iters;
    return CWM_OK;
}
}  // namespace


extern "C" int cwm_debug_set(const char* key, int value) {
    CWM_REQUIRE(key, "cwm_debug_set: null key");
    if (!strcmp(key, "gemm_prof")) return gemm_prof_dump();            // query (profiling builds)
    if (!strcmp(key, "attn_prof")) return attention_pipe_prof(value);  // query (profiling builds)
    if (!strcmp(key, "pretend_device")) {  // the device index this thread's wrong-device checks see (-1: the real one): tests on a one-GPU box
        cwm_set_pretend_device(value);
        return CWM_OK;
    }
    CWM_REQUIRE(tuning_set(thread_tuning(), key, value) == 0, "cwm_debug_set: unknown key %s", key);
    return CWM_OK;
}

extern "C" int cwm_debug_get(const char* key, int* value) {
    CWM_REQUIRE(key && value, "cwm_debug_get: null argument");
    CWM_REQUIRE(tuning_get(thread_tuning(), key, value) == 0, "cwm_debug_get: unknown key %s", key);
    return CWM_OK;
}

// Per-shape overrides of the tile choice (the tuning hook behind tools/autotune_step.py).  All configurations give bit-identical results
// (tests/test_kernels_gpu.py; a split-K launch on 128x128 tiles up to the order of its fp32 sum), so an override can only change the speed.
// The table is process-wide; it reaches a launch through Tuning.tile_hook, which the first override installs in this thread's options (models
// created afterwards inherit it).
namespace {
struct TileKey {
    int M, N, K, epi, ovl;
    bool operator<(const TileKey& o) const { return std::tie(M, N, K, epi, ovl) < std::tie(o.M, o.N, o.K, o.epi, o.ovl); }
};
std::mutex g_tile_mu;
std::map<TileKey, int> g_tile_overrides;
std::atomic<int> g_tile_override_count{0};
int tile_hook(int M, int N, int K, int epi, int overlapped) {
    if (g_tile_override_count.load(std::memory_order_relaxed) == 0) return 0;
    std::lock_guard<std::mutex> lock(g_tile_mu);
    auto it = g_tile_overrides.find(TileKey{M, N, K, epi, overlapped ? 1 : 0});
    return it == g_tile_overrides.end() ? 0 : it->second;
}
}  // namespace

extern "C" int cwm_gemm_tile_override(int M, int N, int K, int epi, int overlapped, int cfg) {
    thread_tuning().tile_hook = tile_hook;
    std::lock_guard<std::mutex> lock(g_tile_mu);
    if (M <= 0) {
        g_tile_overrides.clear();
    } else if (cfg == 0) {
        g_tile_overrides.erase(TileKey{M, N, K, epi, overlapped ? 1 : 0});
    } else {
        CWM_REQUIRE(cfg == 1 || cfg == 4 || cfg == 6, "cwm_gemm_tile_override: unknown tile configuration %d", cfg);
        g_tile_overrides[TileKey{M, N, K, epi, overlapped ? 1 : 0}] = cfg;
    }
    g_tile_override_count.store((int)g_tile_overrides.size());
    return 0;
}

// What gemm_plan decides for a launch of this shape under this thread's options: nothing is launched and no device is needed.
extern "C" int cwm_dev_gemm_plan(int M, int N, int K, int epi, int mode, int overlapped, int forced_cfg, int cus, cwm_dev_gemm_plan_out* out) {
    CWM_REQUIRE(out && epi >= 0 && epi <= 3 && forced_cfg >= 0 && cus >= 0, "cwm_dev_gemm_plan: bad argument");
    int planes;
    if (int rc = mode_planes("cwm_dev_gemm_plan", mode, &planes)) return rc;
    static_assert(CWM_DEV_GEMM_KERNEL_128 == GEMM_KERNEL_128 && CWM_DEV_GEMM_KERNEL_DEEP128 == GEMM_KERNEL_DEEP128 &&
                      CWM_DEV_GEMM_KERNEL_DEEP64 == GEMM_KERNEL_DEEP64 && CWM_DEV_GEMM_KERNEL_8PHASE == GEMM_KERNEL_8PHASE,
                  "cwm_hip_dev.h names the kernels of kernels.h GemmKernel");
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.M = M; p.N = N; p.K = K; p.lda = K; p.epi = epi;
    p.ldc = p.ldr = p.ldo = N;  // dense outputs, as cwm_bench_gemm makes them
    if (epi == EPI_QKV) set_qkv_epilogue(p, M, M, N / 3, 64, nullptr, nullptr, nullptr, 0);  // one sample of M tokens, heads of 64
    p.overlapped = overlapped ? 1 : 0;
    p.tune = &thread_tuning();
    GemmPlan plan;
    if (int rc = gemm_plan(p, planes, forced_cfg, cus ? cus : gemm_cu_count(), &plan)) return rc;
    memset(out, 0, sizeof(*out));
    out->cfg = plan.cfg;
    out->nparts = plan.nparts;
    for (int i = 0; i < plan.nparts; ++i) {
        out->part[i].m_offset = plan.part[i].m_offset;
        out->part[i].M = plan.part[i].M;
        out->part[i].kernel = plan.part[i].kernel;
        out->part[i].splitk = plan.part[i].splitk;
    }
    return CWM_OK;
}

// The forms flow_view.h picks for these flow samples, entry point by entry point: its functions, called as the entry points call them.
extern "C" int cwm_dev_flow_forms(const int64_t* strides, int B, int C, int H, int W, int S, uint64_t flows_addr, uint64_t aux_addr, int normalize_per_sample,
                                  const int64_t* mask_strides, uint64_t mask_addr, int patches_per_frame, cwm_dev_flow_forms_out* out) {
    CWM_REQUIRE(out && mask_strides, "cwm_dev_flow_forms: null pointer");
    static_assert(CWM_DEV_FLOW_REFUSED == FLOW_REFUSED && CWM_DEV_FLOW_FEATURES_VEC4 == FEATURES_VEC4 && CWM_DEV_FLOW_MOTION_TILE == MOTION_TILE &&
                      CWM_DEV_FLOW_MOTION_ROWS16 == MOTION_ROWS16 && CWM_DEV_FLOW_MOTION_ROWS32 == MOTION_ROWS32 && CWM_DEV_FLOW_MOTION_ROWS64 == MOTION_ROWS64 &&
                      CWM_DEV_FLOW_COUNT_PLANES_VEC == COUNT_PLANES_VEC && CWM_DEV_FLOW_COUNT_PACKED == COUNT_PACKED && CWM_DEV_FLOW_COUNT_PACKED_VEC == COUNT_PACKED_VEC &&
                      CWM_DEV_FLOW_FINISH_V4 == FINISH_V4 && CWM_DEV_FLOW_ZERO_PLANES_VEC == ZERO_PLANES_VEC && CWM_DEV_FLOW_ZERO_SCATTER == ZERO_SCATTER &&
                      CWM_DEV_FLOW_FEATURES_SCALAR == FEATURES_SCALAR && CWM_DEV_FLOW_MOTION_STRIDED == MOTION_STRIDED && CWM_DEV_FLOW_COUNT_PLANES == COUNT_PLANES &&
                      CWM_DEV_FLOW_FINISH_V1 == FINISH_V1 && CWM_DEV_FLOW_ZERO_PLANES == ZERO_PLANES && CWM_DEV_FLOW_PACK_TRANSPOSE == PACK_TRANSPOSE,
                  "cwm_hip_dev.h names the forms of flow_view.h FlowForm");
    const float* flows = reinterpret_cast<const float*>((uintptr_t)flows_addr);
    out->features = out->motion = out->count = out->finish = out->zero = out->pack = FLOW_REFUSED;
    FlowView v;
    if (flow_view("cwm_dev_flow_forms", false, flows, strides, B, C, H, W, S, &v) == 0) {
        const FlowLayout l = flow_layout(v, (uintptr_t)aux_addr);
        out->features = flow_features_form(v, l);
        out->motion = flow_motion_form(v, l, normalize_per_sample != 0);
    }
    if (flow_view("cwm_dev_flow_forms", true, flows, strides, B, C, H, W, S, &v) == 0) {
        const FlowLayout l = flow_layout(v, 0);
        out->count = flow_count_form(v, l);
        out->finish = flow_finish_form(S, mask_strides, (uintptr_t)mask_addr, patches_per_frame);
        out->zero = flow_zero_form(v, l);
        out->pack = flow_pack_form(l);
    }
    cwm_set_error("%s", "");  // (a refusal is reported through the -1 fields: the checks' texts do not outlive a call that succeeded)
    return CWM_OK;
}

extern "C" int cwm_bench_gemm(int M, int N, int K, int mode, int epi, int iters, double* avg_us) {
    CWM_REQUIRE(avg_us && M > 0 && N > 0 && K > 0 && iters > 0, "cwm_bench_gemm: bad argument");
    int planes;
    if (int rc = mode_planes("cwm_bench_gemm", mode, &planes)) return rc;
    const int Kp = round_up(K, 64), Np = round_up(N, 256);
    Scratch sc;
    bf16* A = sc.get<bf16>((size_t)2 * M * Kp);
    bf16* W = sc.get<bf16>((size_t)2 * Np * Kp);
    float* bias = sc.get<float>(Np);
    float* Cm = sc.get<float>((size_t)M * N);
    bf16* G = sc.get<bf16>((size_t)2 * M * N + 64 * 1024);
    bf16* G2 = sc.get<bf16>((size_t)2 * M * N + 64 * 1024);
    bf16* G3 = sc.get<bf16>((size_t)2 * M * N + 64 * 1024 * 64);
    CWM_REQUIRE(A && W && bias && Cm && G && G2 && G3, "cwm_bench_gemm: out of device memory");
    fill_bf16(A, (int64_t)2 * M * Kp, 1, 1.0f);
    fill_bf16(W, (int64_t)2 * Np * Kp, 2, 0.05f);
    fill_f32(bias, Np, 3, 0.1f);
    fill_f32(Cm, (int64_t)M * N, 4, 1.0f);
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = A; p.lda = Kp; p.W = W;
    p.M = M; p.N = N; p.K = Kp; p.bias = bias;
    if (epi == 1 || epi == 2) {
        p.epi = epi == 1 ? EPI_BF16_GELU : EPI_BF16; p.out_hi = G; p.ldo = N;
    } else if (epi == 3) {
        CWM_REQUIRE(N % 192 == 0, "cwm_bench_gemm: QKV epilogue needs N = 3*64*heads");
        const int n_tok = 792 <= M && M % 792 == 0 ? 792 : M;
        set_qkv_epilogue(p, n_tok, n_tok, N / 3, 64, G, G2, G3, (int64_t)M * (N / 3));
    } else {
        p.epi = EPI_F32; p.C = Cm; p.ldc = N; p.resid = Cm; p.ldr = N;
    }
    p.tune = &thread_tuning();
    return time_launches(iters, 0, [&] { return launch_gemm(p, planes, 0); }, avg_us);
}

extern "C" int cwm_bench_attention(int B, int H, int N, int mode, int iters, double* avg_us) {
    CWM_REQUIRE(avg_us && B > 0 && H > 0 && N > 0 && iters > 0, "cwm_bench_attention: bad argument");
    int planes;
    if (int rc = mode_planes("cwm_bench_attention", mode, &planes)) return rc;
    const int D = H * 64;
    const int64_t qk_plane = (int64_t)B * N * D;
    Scratch sc;
    bf16* q = sc.get<bf16>(2 * qk_plane);
    bf16* k = sc.get<bf16>(2 * qk_plane);
    bf16* v = sc.get<bf16>(2 * qk_plane);
    bf16* o = sc.get<bf16>(2 * qk_plane);
    CWM_REQUIRE(q && k && v && o, "cwm_bench_attention: out of device memory");
    fill_bf16(q, 2 * qk_plane, 5, 0.5f);
    fill_bf16(k, 2 * qk_plane, 6, 1.0f);
    fill_bf16(v, 2 * qk_plane, 7, 1.0f);
    AttnParams a = attn_dense(q, k, v, qk_plane, o, qk_plane, D, B, H, N);
    a.tune = &thread_tuning();
    return time_launches(iters, 0, [&] { return launch_attention(a, planes, 0); }, avg_us);
}

// ---- RAFT kernels one at a time (tests/test_raft_kernels_gpu.py) ---------------------------------------------------------------------------------
// The launches of raft_model.hip on caller-owned buffers.  A convolution is made of what the model's run_conv / prepare are made of (kernels.h
// set_conv_geometry, pack_conv_parts, conv_gemm) and launched by launch_gemm with this thread's options.
namespace {
ConvSrc conv_src_of(const cwm_dev_conv_src& d) {
    ConvSrc s = {};
    s.p = d.p;
    s.ld = d.ld ? d.ld : d.C;
    s.C = d.C;
    s.stats = d.stats;
    s.relu = d.relu;
    s.gate = d.gate;
    s.gate_ld = d.gate_ld;
    s.coords = d.coords;
    return s;
}
bool conv_src_ok(const cwm_dev_conv_src& d) { return d.C > 0 && (d.coords ? d.C == 2 : d.p != nullptr) && (!d.gate || d.gate_ld >= d.C); }
}  // namespace

extern "C" int cwm_dev_raft_conv(const cwm_dev_raft_conv_args* args) {
    CWM_REQUIRE(args && args->struct_size == sizeof(cwm_dev_raft_conv_args), "cwm_dev_raft_conv: args->struct_size must be sizeof(cwm_dev_raft_conv_args)");
    const cwm_dev_raft_conv_args& a = *args;
    hipStream_t s = (hipStream_t)a.stream;
    int planes;
    if (int rc = mode_planes("cwm_dev_raft_conv", a.mode, &planes)) return rc;
    const bool frames = a.image[0] != nullptr, operand_only = a.flags & CWM_DEV_CONV_OPERAND_ONLY, keep = a.flags & CWM_DEV_CONV_KEEP_OPERAND;
    CWM_REQUIRE(!(operand_only && keep), "cwm_dev_raft_conv: flags ask for the operand only and for no operand");
    CWM_REQUIRE(a.n_img > 0 && a.H > 0 && a.W > 0 && a.kh > 0 && a.kw > 0 && a.stride > 0 && a.pad_h >= 0 && a.pad_w >= 0, "cwm_dev_raft_conv: bad geometry");
    Im2colParams ip = {};
    if (frames) {
        CWM_REQUIRE(a.image[1] && a.P > 0 && a.ppg > 0 && a.P % a.ppg == 0 && a.img0 >= 0 && a.img0 + a.n_img <= 2 * a.P,
                    "cwm_dev_raft_conv: images [%d, %d) of 2 x %d pairs (%d per group)", a.img0, a.img0 + a.n_img, a.P, a.ppg);
        ip.src[0].C = 3;
        ip.nsrc = 1;
        for (int f = 0; f < 2; ++f) {
            ip.image.base[f] = a.image[f];
            ip.image.sb[f] = a.image_sb[f];
            ip.image.st[f] = a.image_st[f];
            ip.image.sc[f] = a.image_sc[f];
        }
        ip.image.P = a.P;
        ip.image.ppg = a.ppg;
        ip.image.scale = a.scale;
        ip.img0 = a.img0;
    } else {
        CWM_REQUIRE((a.nsrc == 1 || a.nsrc == 2) && conv_src_ok(a.src[0]) && (a.nsrc == 1 || conv_src_ok(a.src[1])), "cwm_dev_raft_conv: bad source");
        ip.nsrc = a.nsrc;
        for (int i = 0; i < a.nsrc; ++i) ip.src[i] = conv_src_of(a.src[i]);
    }
    const int cin = ip.src[0].C + (ip.nsrc > 1 ? ip.src[1].C : 0), K = a.kh * a.kw * cin, Kpad = round_up(K, 64);
    set_conv_geometry(ip, a.n_img, a.H, a.W, a.kh, a.kw, a.stride, a.pad_h, a.pad_w, Kpad);
    ip.c_lo = a.c_lo;
    ip.c_hi = a.c_hi;
    CWM_REQUIRE(a.H + 2 * a.pad_h >= a.kh && a.W + 2 * a.pad_w >= a.kw, "cwm_dev_raft_conv: the kernel is larger than the padded input");
    CWM_REQUIRE(a.c_hi <= a.c_lo || (a.A && a.c_lo >= 0 && a.c_hi <= cin), "cwm_dev_raft_conv: a partial rewrite [%d, %d) of %d channels needs the caller's A",
                a.c_lo, a.c_hi, cin);
    CWM_REQUIRE(a.A || !(operand_only || keep), "cwm_dev_raft_conv: flags = %d needs the caller's A", a.flags);
    const int64_t M = (int64_t)a.n_img * ip.OH * ip.OW;
    CWM_REQUIRE(M * Kpad * planes < (1ll << 32), "cwm_dev_raft_conv: operand too large");
    Scratch sc;
    bf16* A = (bf16*)a.A;
    if (!A) {
        A = sc.get<bf16>((size_t)M * Kpad * planes);
        CWM_REQUIRE(A, "cwm_dev_raft_conv: out of device memory");
    }
    ip.A = A;
    if (!keep)
        if (int rc = launch_im2col(ip, planes, s)) return rc;
    if (!operand_only) {
        CWM_REQUIRE(a.nparts == 1 || a.nparts == 2, "cwm_dev_raft_conv: nparts = %d", a.nparts);
        int n = 0;
        ConvPartW parts[2];
        for (int i = 0; i < a.nparts; ++i) {
            const cwm_dev_conv_part& p = a.part[i];
            CWM_REQUIRE(p.w && p.b && p.n > 0 && (!p.bn_gamma || (p.bn_beta && p.bn_mean && p.bn_var)), "cwm_dev_raft_conv: bad weight part %d", i);
            parts[i] = ConvPartW{p.w, p.b, p.bn_gamma, p.bn_beta, p.bn_mean, p.bn_var, p.n};
            n += p.n;
        }
        // the model's LinearW (engine.hip make_linear): N = the output channels rounded up to 16, zero rows / bias beyond them
        const int N = round_up(n, 16), Npad = round_up(N, 256);
        CWM_REQUIRE(a.out && a.col0 >= 0 && a.ldc >= a.col0 + N, "cwm_dev_raft_conv: columns [%d, %d) do not fit rows of %d", a.col0, a.col0 + N, a.ldc);
        const size_t plane = (size_t)Npad * Kpad;
        bf16* w_hi = sc.get<bf16>(plane);
        bf16* w_il = sc.get<bf16>(2 * plane);
        float* bias = sc.get<float>(Npad);
        CWM_REQUIRE(w_hi && w_il && bias, "cwm_dev_raft_conv: out of device memory");
        CWM_HIP_CHECK(hipMemsetAsync(w_hi, 0, plane * sizeof(bf16), s));
        CWM_HIP_CHECK(hipMemsetAsync(w_il, 0, 2 * plane * sizeof(bf16), s));
        CWM_HIP_CHECK(hipMemsetAsync(bias, 0, (size_t)Npad * sizeof(float), s));
        if (int rc = pack_conv_parts(parts, a.nparts, a.bn_eps, cin, a.kh, a.kw, Kpad, w_il, w_hi, bias, s)) return rc;
        GemmParams g = conv_gemm(A, planes == 2 ? w_il : w_hi, bias, (int)M, N, Kpad, a.out + a.col0, a.ldc);
        g.tune = &thread_tuning();
        if (int rc = launch_gemm(g, planes, s)) return rc;
    }
    CWM_HIP_CHECK(hipStreamSynchronize(s));
    return CWM_OK;
}

extern "C" int cwm_dev_raft_corr_lookup_operand(const float* fmap1_dev, const float* fmap2_dev, const float* coords_dev, int P, int h8, int w8, int mode,
                                                void* A_dev, void* stream) {
    CWM_REQUIRE(fmap1_dev && fmap2_dev && coords_dev && A_dev && P > 0 && h8 >= 8 && w8 >= 8, "cwm_dev_raft_corr_lookup_operand: bad argument");
    int planes;
    if (int rc = mode_planes("cwm_dev_raft_corr_lookup_operand", mode, &planes)) return rc;
    return raft_corr_lookup_run(fmap1_dev, fmap2_dev, coords_dev, P, h8, w8, nullptr, (bf16*)A_dev, planes, (hipStream_t)stream);
}

extern "C" int cwm_dev_raft_corr_lookup_on_the_fly_operand(const float* fmap1_dev, const float* fmap2_dev, const float* coords_dev, int P, int h8, int w8,
                                                           int mode, void* A_dev, void* stream) {
    CWM_REQUIRE(fmap1_dev && fmap2_dev && coords_dev && A_dev && P > 0 && h8 >= 8 && w8 >= 8, "cwm_dev_raft_corr_lookup_on_the_fly_operand: bad argument");
    int planes;
    if (int rc = mode_planes("cwm_dev_raft_corr_lookup_on_the_fly_operand", mode, &planes)) return rc;
    return raft_corr_lookup_on_the_fly_run(fmap1_dev, fmap2_dev, coords_dev, P, h8, w8, nullptr, (bf16*)A_dev, planes, (hipStream_t)stream);
}

extern "C" int cwm_dev_raft_instnorm_stats(const float* x_dev, int n_img, int HW, int C, float eps, float* stats_dev, void* stream) {
    CWM_REQUIRE(x_dev && stats_dev && n_img > 0 && HW > 0 && C > 0, "cwm_dev_raft_instnorm_stats: bad argument");
    Scratch sc;
    double* work = sc.get<double>((size_t)2 * n_img * kInstNormMaxChunks * C);
    CWM_REQUIRE(work, "cwm_dev_raft_instnorm_stats: out of device memory");
    if (int rc = launch_instnorm_stats(x_dev, n_img, HW, C, eps, stats_dev, work, (hipStream_t)stream)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return CWM_OK;
}

extern "C" int cwm_dev_raft_residual_join(const cwm_dev_conv_src* X, const cwm_dev_conv_src* Y, int n_img, int HW, float* out_dev, void* stream) {
    CWM_REQUIRE(X && Y && out_dev && n_img > 0 && HW > 0 && X->p && Y->p && X->C == Y->C && Y->C > 0 && !X->coords && !Y->coords && !X->gate && !Y->gate,
                "cwm_dev_raft_residual_join: bad argument");
    if (int rc = launch_residual_join(conv_src_of(*X), conv_src_of(*Y), n_img, HW, out_dev, (hipStream_t)stream)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return CWM_OK;
}

extern "C" int cwm_dev_raft_cnet_split(const float* cn_dev, int64_t M, float* h_dev, float* x_dev, void* stream) {
    CWM_REQUIRE(cn_dev && h_dev && x_dev && M > 0, "cwm_dev_raft_cnet_split: bad argument");
    if (int rc = launch_cnet_split(cn_dev, M, h_dev, x_dev, (hipStream_t)stream)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return CWM_OK;
}

// ---- frames shared between the pairs of a RAFT forward (tests/test_raft_share_cpu.py, tests/test_raft_share_kernels_gpu.py) ----
extern "C" int cwm_dev_raft_frame_slots(const cwm_raft_forward_args* args, int share, int* slot1, int* slot2, int* cslot, int* n_fnet, int* n_cnet) {
    CWM_REQUIRE(args && slot1 && slot2 && cslot && n_fnet && n_cnet, "cwm_dev_raft_frame_slots: null argument");
    cwm_raft_forward_args a;
    if (int rc = copy_args(a, args, offsetof(cwm_raft_forward_args, stream) + sizeof(void*), "cwm_dev_raft_frame_slots")) return rc;
    CWM_REQUIRE(a.batch >= 1 && a.pairs >= 0 && (share == 0 || share == 1), "cwm_dev_raft_frame_slots: batch = %d, pairs = %d, share = %d", a.batch, a.pairs,
                share);
    const int ppg = a.pairs > 0 ? a.pairs : 1;
    const float* const imgs[2] = {a.image1_dev, a.image2_dev};
    const int64_t sb[2] = {a.image1_stride_b, a.image2_stride_b}, st[2] = {a.image1_stride_t, a.image2_stride_t},
                  sc[2] = {a.image1_stride_c, a.image2_stride_c};
    const FramePlan fp = raft_frame_plan(a.batch, ppg, imgs, sb, st, sc, share != 0);
    for (int p = 0; p < a.batch * ppg; ++p) {
        slot1[p] = (int)(fp.base1 + slot_at(fp.s1, p));
        slot2[p] = (int)(fp.base2 + slot_at(fp.s2, p));
        cslot[p] = (int)slot_at(fp.sc, p);
    }
    *n_fnet = fp.n_fnet;
    *n_cnet = fp.n_cnet;
    return CWM_OK;
}

extern "C" int cwm_dev_raft_corr_lookup_slots(const float* fmap1_dev, const float* fmap2_dev, const float* coords_dev, int P, int ppg, int h8, int w8, int64_t s1b,
                                              int64_t s1t, int64_t s2b, int64_t s2t, float* out_dev, void* stream) {
    CWM_REQUIRE(fmap1_dev && fmap2_dev && coords_dev && out_dev && P > 0 && ppg > 0 && P % ppg == 0 && h8 >= 8 && w8 >= 8 && s1b >= 0 && s1t >= 0 && s2b >= 0 &&
                    s2t >= 0,
                "cwm_dev_raft_corr_lookup_slots: bad argument");
    return raft_corr_lookup_run(fmap1_dev, fmap2_dev, coords_dev, P, h8, w8, out_dev, nullptr, 2, (hipStream_t)stream, SlotMap{ppg, s1b, s1t},
                                SlotMap{ppg, s2b, s2t});
}

extern "C" int cwm_dev_raft_fmap_pool_slots(const float* in_dev, int n_out, int nt, int64_t in_sb, int64_t in_st, int h, int w, int C, float* out_dev,
                                            void* stream) {
    CWM_REQUIRE(in_dev && out_dev && n_out > 0 && nt > 0 && in_sb >= 0 && in_st >= 0 && h >= 2 && w >= 2 && C > 0, "cwm_dev_raft_fmap_pool_slots: bad argument");
    if (int rc = launch_fmap_pool(in_dev, n_out, h, w, C, out_dev, (hipStream_t)stream, SlotMap{nt, in_sb, in_st})) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return CWM_OK;
}

extern "C" int cwm_dev_raft_corr_lookup_on_the_fly_slots(const float* fmap1_dev, const float* const* fmap2_levels_dev, const float* coords_dev, int P, int ppg,
                                                         int h8, int w8, int64_t s1b, int64_t s1t, int64_t s2b, int64_t s2t, int64_t s2pb, int64_t s2pt,
                                                         float* out_dev, void* stream) {
    CWM_REQUIRE(fmap1_dev && fmap2_levels_dev && coords_dev && out_dev && P > 0 && ppg > 0 && P % ppg == 0 && h8 >= 8 && w8 >= 8 && s1b >= 0 && s1t >= 0 &&
                    s2b >= 0 && s2t >= 0 && s2pb >= 0 && s2pt >= 0,
                "cwm_dev_raft_corr_lookup_on_the_fly_slots: bad argument");
    CorrOnTheFlyParams lp = {};
    lp.fmap1 = fmap1_dev;
    lp.coords = coords_dev;
    lp.hw8 = (int64_t)h8 * w8;
    lp.M = P * lp.hw8;
    lp.Kpad = 384;
    lp.out = out_dev;
    lp.out_ld = 324;
    lp.ppg = ppg;
    lp.s1b = s1b;
    lp.s1t = s1t;
    for (int l = 0; l < 4; ++l) {
        CWM_REQUIRE(fmap2_levels_dev[l], "cwm_dev_raft_corr_lookup_on_the_fly_slots: level %d is null", l);
        lp.fmap2[l] = fmap2_levels_dev[l];
        lp.h[l] = h8 >> l;
        lp.w[l] = w8 >> l;
        lp.s2b[l] = l ? s2pb : s2b;
        lp.s2t[l] = l ? s2pt : s2t;
    }
    if (int rc = launch_corr_lookup_on_the_fly(lp, 2, (hipStream_t)stream)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return CWM_OK;
}

extern "C" int cwm_dev_raft_cnet_split_slots(const float* cn_dev, int64_t M, int64_t hw8, int ppg, int64_t sb, int64_t st, float* h_dev, float* x_dev,
                                             void* stream) {
    CWM_REQUIRE(cn_dev && h_dev && x_dev && M > 0 && hw8 > 0 && M % hw8 == 0 && ppg > 0 && (M / hw8) % ppg == 0 && sb >= 0 && st >= 0,
                "cwm_dev_raft_cnet_split_slots: bad argument");
    if (int rc = launch_cnet_split(cn_dev, M, h_dev, x_dev, (hipStream_t)stream, hw8, SlotMap{ppg, sb, st})) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return CWM_OK;
}

extern "C" int cwm_dev_raft_motion_finish(float* x_dev, const float* coords_dev, int64_t M, int h8, int w8, void* stream) {
    CWM_REQUIRE(x_dev && coords_dev && M > 0 && h8 > 0 && w8 > 0, "cwm_dev_raft_motion_finish: bad argument");
    if (int rc = launch_motion_finish(x_dev, coords_dev, M, h8, w8, (hipStream_t)stream)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return CWM_OK;
}

extern "C" int cwm_dev_raft_gru_update(float* h_dev, const float* zr_dev, const float* q_dev, int64_t M, void* stream) {
    CWM_REQUIRE(h_dev && zr_dev && q_dev && M > 0, "cwm_dev_raft_gru_update: bad argument");
    if (int rc = launch_gru_update(h_dev, zr_dev, q_dev, M, (hipStream_t)stream)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return CWM_OK;
}

extern "C" int cwm_dev_raft_flow_update(float* coords_dev, const float* delta_dev, int ld, int64_t M, void* stream) {
    CWM_REQUIRE(coords_dev && delta_dev && ld >= 2 && M > 0, "cwm_dev_raft_flow_update: bad argument");
    if (int rc = launch_flow_update(coords_dev, delta_dev, ld, M, (hipStream_t)stream)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return CWM_OK;
}

// ---- the operand gathers one launch at a time (tests/test_gather_kernels_gpu.py) ----
// ragged: cwm_dev_gather_ragged's call (INDEX / INDEX_UNFUSED with the launch forms of a ragged batch: n_vis_min and counts go to the launchers as they are; the
// entry point refuses a least count of 0, which the launchers take for a rectangular batch)
static int dev_gather(const cwm_dev_gather_args* args, bool ragged, int n_vis_min, int* counts) {
    CWM_REQUIRE(args && args->struct_size == sizeof(cwm_dev_gather_args), "cwm_dev_gather: args->struct_size must be sizeof(cwm_dev_gather_args)");
    const cwm_dev_gather_args& a = *args;
    CWM_REQUIRE(!ragged || a.kind == CWM_DEV_GATHER_INDEX || a.kind == CWM_DEV_GATHER_INDEX_UNFUSED, "cwm_dev_gather_ragged: kind %d has no ragged form", a.kind);
    hipStream_t s = (hipStream_t)a.stream;
    int planes;
    if (int rc = mode_planes("cwm_dev_gather", a.mode, &planes)) return rc;
    CWM_REQUIRE(a.out && a.x && a.B > 0 && a.n_rows > 0 && a.Nt > 0 && a.ld > 0 && a.ld % (planes == 2 ? 32 : 4) == 0,
                "cwm_dev_gather: bad argument (rows of ld = %d need a multiple of 32 in parity mode, of 4 in fast mode)", a.ld);
    const int L = a.perm_stride ? a.perm_stride : a.Nt;
    CWM_REQUIRE(L >= a.Nt && a.n_rows <= L, "cwm_dev_gather: %d rows per sample of a %d-slot permutation over %d tokens", a.n_rows, L, a.Nt);
    int rc = 0;
    if (a.kind == CWM_DEV_GATHER_IMU) {
        CWM_REQUIRE(a.perm && a.C > 0 && a.tubelet > 0 && a.C * a.tubelet <= a.ld && (int64_t)a.Nt * a.tubelet <= a.L, "cwm_dev_gather: bad IMU geometry");
        ImuGatherParams g;
        memset(&g, 0, sizeof(g));
        g.imu = a.x;
        g.B = a.B, g.C = a.C, g.L = a.L, g.tubelet = a.tubelet;
        g.perm = a.perm, g.perm_stride = L, g.n_rows = a.n_rows, g.n_real = a.Nt;
        g.out = (bf16*)a.out, g.ld = a.ld;
        rc = launch_imu_gather(g, planes, s);
    } else {
        CWM_REQUIRE(a.P > 0 && a.P % 4 == 0 && a.H > 0 && a.W > 0 && a.H % a.P == 0 && a.W % a.P == 0, "cwm_dev_gather: bad frame geometry");
        const int n = (a.H / a.P) * (a.W / a.P);
        CWM_REQUIRE(((uintptr_t)a.x & 15) == 0 && a.sb % 4 == 0 && a.sc % 4 == 0 && a.st % 4 == 0, "cwm_dev_gather: frames must be 16-byte aligned, strides multiples of 4");
        if (a.kind == CWM_DEV_GATHER_FLOW_RGB) {
            CWM_REQUIRE(a.perm && a.Nt == n, "cwm_dev_gather: the flow-RGB gather has one frame of %d tokens", n);
            FlowRgbGatherParams g;
            memset(&g, 0, sizeof(g));
            g.fwd = a.fwd, g.bwd = a.bwd, g.f_sb = a.f_sb, g.f_sc = a.f_sc, g.b_sb = a.b_sb, g.b_sc = a.b_sc;
            g.x = a.x, g.sb = a.sb, g.sc = a.sc;
            g.normalize = a.normalize, g.H = a.H, g.W = a.W, g.P = a.P;
            g.perm = a.perm, g.Nt = a.Nt, g.n_rows = a.n_rows, g.perm_stride = L, g.B = a.B;
            g.out = (bf16*)a.out, g.ld = a.ld;
            rc = launch_flow_rgb_gather(g, planes, s);
        } else {
            CWM_REQUIRE(a.C > 0 && a.Nt % n == 0, "cwm_dev_gather: %d tokens are no whole number of %d-token frames", a.Nt, n);
            PatchGatherParams g;
            memset(&g, 0, sizeof(g));
            g.x = a.x, g.sb = a.sb, g.sc = a.sc, g.st = a.st;
            g.normalize = a.normalize, g.C = a.C, g.H = a.H, g.W = a.W, g.P = a.P;
            g.perm = a.perm, g.Nt = a.Nt, g.n_rows = a.n_rows, g.perm_stride = a.perm_stride, g.B = a.B;
            g.out = (bf16*)a.out, g.ld = a.ld;
            if (a.kind == CWM_DEV_GATHER_PATCH) {
                CWM_REQUIRE(a.perm, "cwm_dev_gather: the patch gather reads perm");
                rc = launch_patch_gather(g, planes, s);
            } else if (a.kind == CWM_DEV_GATHER_INDEX) {
                CWM_REQUIRE(a.mask && a.perm && a.err_rows, "cwm_dev_gather: the index gather needs mask, perm and err_rows");
                rc = launch_index_gather(g, a.mask, a.n_vis, a.perm, a.rank, a.err_rows, planes, s, n_vis_min, counts);
            } else if (a.kind == CWM_DEV_GATHER_INDEX_UNFUSED) {
                CWM_REQUIRE(a.mask && a.perm && a.rank && a.err_rows, "cwm_dev_gather: the unfused index prologue needs mask, perm, rank and err_rows");
                CWM_HIP_CHECK(hipMemsetAsync(a.err_rows, 0, (size_t)a.B * sizeof(int), s));
                CWM_REQUIRE(!ragged || n_vis_min != 0, "mask_to_perm (ragged): bad argument");
                if ((rc = launch_mask_to_perm(a.mask, a.B, L, a.n_vis, a.perm, a.err_rows, s, n_vis_min, counts))) return rc;
                if ((rc = launch_patch_gather(g, planes, s))) return rc;
                rc = launch_perm_to_rank(a.perm, a.rank, a.B, L, s);
            } else {
                CWM_REQUIRE(false, "cwm_dev_gather: unknown kind %d", a.kind);
            }
        }
    }
    if (rc) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize(s));
    return CWM_OK;
}

extern "C" int cwm_dev_gather(const cwm_dev_gather_args* args) { return dev_gather(args, false, 0, nullptr); }

extern "C" int cwm_dev_gather_ragged(const cwm_dev_gather_args* args, int n_vis_min, int32_t* counts_dev) { return dev_gather(args, true, n_vis_min, counts_dev); }

// ---- the conjoined predictor's attention and padding kernels one call at a time (tests/test_conj_kernels_gpu.py) ----
namespace {
// fp32 [rows][K] -> the operand layout the MFMA cross attention reads its main-stream projections in (what Engine::linear_operand writes in a forward)
template <int PLANES>
__global__ void stage_operand_kernel(const float* src, int64_t rows, int K, bf16* out) {  // K a multiple of 4
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= rows * K) return;
    const int64_t r = i / K;
    store_operand4<PLANES>(out, r, K, (int)(i - r * K), *reinterpret_cast<const f32x4*>(src + i));
}
int stage_operand(const float* src, int64_t rows, int K, bf16* out, int planes, hipStream_t s) {
    const unsigned grid = (unsigned)((rows * K / 4 + 255) / 256);
    dispatch_int<1, 2>(planes == 2 ? 2 : 1, [&](auto pl) { hipLaunchKernelGGL(stage_operand_kernel<pl.value>, dim3(grid), dim3(256), 0, s, src, rows, K, out); });
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" int cwm_dev_conj_cross_attention(const cwm_dev_conj_cross_attention_args* args) {
    CWM_REQUIRE(args && args->struct_size == sizeof(cwm_dev_conj_cross_attention_args),
                "cwm_dev_conj_cross_attention: args->struct_size must be sizeof(cwm_dev_conj_cross_attention_args)");
    const cwm_dev_conj_cross_attention_args& a = *args;
    hipStream_t s = (hipStream_t)a.stream;
    int planes;
    if (int rc = mode_planes("cwm_dev_conj_cross_attention", a.mode, &planes)) return rc;
    CWM_REQUIRE(a.impl == CWM_DEV_CONJ_VALU || a.impl == CWM_DEV_CONJ_MFMA, "cwm_dev_conj_cross_attention: unknown impl %d", a.impl);
    const bool mfma = a.impl == CWM_DEV_CONJ_MFMA;
    CWM_REQUIRE(a.roles >= 1 && a.roles <= 3 && (mfma || a.roles == 3), "cwm_dev_conj_cross_attention: roles = %d (MFMA: 1, 2 or 3; VALU: 3)", a.roles);
    CWM_REQUIRE(a.qk && a.v && a.qk_src && a.v_src && a.y && a.y_src, "cwm_dev_conj_cross_attention: null argument");
    CWM_REQUIRE(a.B > 0 && a.N > 0 && a.M > 0 && a.heads > 0 && a.head_dim > 0 && (int64_t)a.B * a.N * 4 * a.heads * a.head_dim < (1ll << 31),
                "cwm_dev_conj_cross_attention: bad geometry");
    const int D = a.heads * a.head_dim;
    CWM_REQUIRE(D % 32 == 0, "cwm_dev_conj_cross_attention: operand rows of %d columns (need a multiple of 32)", D);
    if (mfma) {
        CWM_REQUIRE(cross_attention_mfma_ok(a.head_dim, a.M), "cwm_dev_conj_cross_attention: the MFMA form has no kernel for head_dim %d, M %d", a.head_dim, a.M);
        CWM_REQUIRE(cross_attention_mfma_fits(a.B, a.N, a.heads, a.head_dim), "cwm_dev_conj_cross_attention: too large for the MFMA form's 32-bit offsets");
    } else {
        CWM_REQUIRE(cross_attention_ok(a.M, a.head_dim), "cwm_dev_conj_cross_attention: the VALU form refuses M %d, head_dim %d (%zu bytes of LDS)", a.M, a.head_dim,
                    cross_attention_lds_bytes(a.M, a.head_dim));
    }
    const int64_t rows = (int64_t)a.B * a.N;
    Scratch sc;
    CrossAttnParams p;
    memset(&p, 0, sizeof(p));
    p.qk = a.qk, p.v = a.v, p.qk_src = a.qk_src, p.v_src = a.v_src;
    p.B = a.B, p.N = a.N, p.M = a.M, p.heads = a.heads, p.head_dim = a.head_dim, p.scale = a.scale;
    p.y = (bf16*)a.y, p.y_plane = rows * D, p.y_src = (bf16*)a.y_src, p.y_src_plane = (int64_t)a.B * a.M * D;
    int rc;
    if (mfma) {
        bf16* qk_op = sc.get<bf16>((size_t)rows * 2 * D * planes);
        bf16* v_op = sc.get<bf16>((size_t)rows * D * planes);
        p.partial = sc.get<float>(cross_attention_mfma_partial_floats(a.B, a.heads, a.M, a.head_dim));
        CWM_REQUIRE(qk_op && v_op && p.partial, "cwm_dev_conj_cross_attention: out of device memory");
        if ((rc = stage_operand(a.qk, rows, 2 * D, qk_op, planes, s)) || (rc = stage_operand(a.v, rows, D, v_op, planes, s))) return rc;
        p.qk_op = qk_op, p.v_op = v_op;
        if ((rc = launch_cross_attention_mfma_roles(p, planes, s, s, a.roles))) return rc;
    } else {
        p.scores_t = sc.get<float>((size_t)a.B * a.heads * a.M * a.N);
        p.partial = sc.get<float>(cross_attention_partial_floats(a.B, a.heads, a.M, a.head_dim));
        CWM_REQUIRE(p.scores_t && p.partial, "cwm_dev_conj_cross_attention: out of device memory");
        if ((rc = launch_cross_attention(p, planes, s))) return rc;
    }
    CWM_HIP_CHECK(hipStreamSynchronize(s));
    return CWM_OK;
}

extern "C" int cwm_dev_conj_small_attention(const cwm_dev_conj_small_attention_args* args) {
    CWM_REQUIRE(args && args->struct_size == sizeof(cwm_dev_conj_small_attention_args),
                "cwm_dev_conj_small_attention: args->struct_size must be sizeof(cwm_dev_conj_small_attention_args)");
    const cwm_dev_conj_small_attention_args& a = *args;
    hipStream_t s = (hipStream_t)a.stream;
    int planes;
    if (int rc = mode_planes("cwm_dev_conj_small_attention", a.mode, &planes)) return rc;
    CWM_REQUIRE(a.impl == CWM_DEV_CONJ_VALU || a.impl == CWM_DEV_CONJ_MFMA, "cwm_dev_conj_small_attention: unknown impl %d", a.impl);
    CWM_REQUIRE(a.qkv && a.o && a.B > 0 && a.heads > 0, "cwm_dev_conj_small_attention: bad argument");
    CWM_REQUIRE(a.n_tok > 0 && a.n_tok <= 64 && a.head_dim > 0 && a.head_dim <= 64, "cwm_dev_conj_small_attention: needs n_tok <= 64 and head_dim <= 64 (got %d, %d)",
                a.n_tok, a.head_dim);
    CWM_REQUIRE(a.impl == CWM_DEV_CONJ_VALU || small_attention_mfma_ok(a.n_tok, a.head_dim), "cwm_dev_conj_small_attention: the MFMA form needs head_dim 32 (got %d)",
                a.head_dim);
    const int D = a.heads * a.head_dim;
    CWM_REQUIRE(D % 4 == 0 && a.ldo % 32 == 0 && a.ldo >= D, "cwm_dev_conj_small_attention: %d columns in operand rows of ldo = %d (a multiple of 32)", D, a.ldo);
    SmallAttnParams p;
    memset(&p, 0, sizeof(p));
    p.qkv = a.qkv;
    p.B = a.B, p.n_tok = a.n_tok, p.heads = a.heads, p.head_dim = a.head_dim;
    p.o = (bf16*)a.o, p.o_plane = (int64_t)a.B * a.n_tok * a.ldo, p.ldo = a.ldo;
    if (int rc = a.impl == CWM_DEV_CONJ_MFMA ? launch_small_attention_mfma(p, planes, s) : launch_small_attention(p, planes, s)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize(s));
    return CWM_OK;
}

extern "C" int cwm_dev_conj_pad(const cwm_dev_conj_pad_args* args) {
    CWM_REQUIRE(args && args->struct_size == sizeof(cwm_dev_conj_pad_args), "cwm_dev_conj_pad: args->struct_size must be sizeof(cwm_dev_conj_pad_args)");
    const cwm_dev_conj_pad_args& a = *args;
    hipStream_t s = (hipStream_t)a.stream;
    CWM_REQUIRE(a.B > 0, "cwm_dev_conj_pad: bad batch");
    int rc = 0;
    if (a.kind == CWM_DEV_CONJ_PAD_MASK) {
        CWM_REQUIRE(a.mask && a.ext_mask && a.N > 0 && a.P >= 0 && a.vmax >= 0, "cwm_dev_conj_pad: bad pad-mask argument");
        rc = launch_pad_mask(a.mask, a.B, a.N, a.P, a.vmax, a.ext_mask, s);
    } else if (a.kind == CWM_DEV_CONJ_FIX_PAD_ROWS) {
        CWM_REQUIRE(a.x && a.perm && a.token && a.n_rows > 0 && a.D > 0 && a.perm_stride >= a.n_rows && a.n_real >= 0, "cwm_dev_conj_pad: bad fix-pad-rows argument");
        rc = launch_fix_pad_rows(a.x, a.perm, a.B, a.perm_stride, a.n_rows, a.n_real, a.D, a.token, s);
    } else if (a.kind == CWM_DEV_CONJ_ZERO_PAD_OUT_ROWS) {
        CWM_REQUIRE(a.x && a.perm && a.n_rows > 0 && a.D > 0 && a.n_vis >= 0 && a.perm_stride >= a.n_vis + a.n_rows && a.n_real >= 0,
                    "cwm_dev_conj_pad: bad zero-pad-out-rows argument");
        rc = launch_zero_pad_out_rows(a.x, a.perm, a.B, a.perm_stride, a.n_vis, a.n_rows, a.n_real, a.D, s);
    } else if (a.kind == CWM_DEV_CONJ_IMU_APPEND_DUMMY) {
        CWM_REQUIRE(a.imu && a.mask && a.dummy && a.out && a.ext_mask && a.C > 0 && a.L > 0 && a.T > 0 && a.N > 0, "cwm_dev_conj_pad: bad append-dummy argument");
        rc = launch_imu_append_dummy(a.imu, a.mask, a.dummy, a.B, a.C, a.L, a.T, a.N, a.out, a.ext_mask, s);
    } else {
        CWM_REQUIRE(false, "cwm_dev_conj_pad: unknown kind %d", a.kind);
    }
    if (rc) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize(s));
    return CWM_OK;
}

// ---- the ViT engine's own launch forms one at a time (tests/test_engine_kernels_gpu.py) ----
// The parameters engine.hip builds for its row-mapped GEMMs (residual_gemm, embed_stream, to_decoder), the Q/K/V scatter and the pruned block's query
// window, LayerNorm on mapped rows (run_mlp, head_rows) and the mask-token fill, each as one launch on the caller's buffers.
extern "C" int cwm_dev_gemm(const cwm_dev_gemm_args* args) {
    CWM_REQUIRE(args && args->struct_size == sizeof(cwm_dev_gemm_args), "cwm_dev_gemm: args->struct_size must be sizeof(cwm_dev_gemm_args)");
    const cwm_dev_gemm_args& a = *args;
    hipStream_t s = (hipStream_t)a.stream;
    int planes;
    if (int rc = mode_planes("cwm_dev_gemm", a.mode, &planes)) return rc;
    CWM_REQUIRE(a.a && a.w && a.M > 0 && a.N > 0 && a.K > 0 && a.epi >= EPI_F32 && a.epi <= EPI_QKV, "cwm_dev_gemm: bad argument");
    CWM_REQUIRE(a.rows_in >= 0 && a.out_row_offset >= 0 && (a.rows_in > 0 || (!a.resid_rowmap && a.out_row_offset == 0)),
                "cwm_dev_gemm: a row map or row offset needs rows_in > 0");
    if (a.rows_in > 0) {
        CWM_REQUIRE(a.M % a.rows_in == 0 && a.rows_in + a.out_row_offset <= a.rows_out, "cwm_dev_gemm: %d rows as samples of %d rows at offset %d of %d", a.M,
                    a.rows_in, a.out_row_offset, a.rows_out);
        CWM_REQUIRE(!a.resid_rowmap || a.map_stride >= a.rows_in, "cwm_dev_gemm: a residual row map of %d entries per sample for %d rows", a.map_stride, a.rows_in);
    }
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.M = a.M; p.N = a.N; p.K = p.lda = round_up(a.K, 64);
    p.epi = a.epi;
    p.rows_in = a.rows_in; p.rows_out = a.rows_out; p.out_row_offset = a.out_row_offset; p.map_stride = a.map_stride; p.resid_rowmap = a.resid_rowmap;
    if (a.epi == EPI_F32) {
        CWM_REQUIRE(a.C && a.ldc >= a.N && (!a.resid || a.ldr >= a.N), "cwm_dev_gemm: the fp32 output needs C and rows of at least N columns");
        CWM_REQUIRE(!a.resid_rowmap || a.resid, "cwm_dev_gemm: a residual row map without a residual");
        p.C = a.C; p.ldc = a.ldc; p.resid = a.resid; p.ldr = a.ldr;
    } else if (a.epi == EPI_QKV) {
        CWM_REQUIRE(a.q_out && a.k_out && a.v_out && a.heads > 0 && a.head_dim > 0 && a.n_tok > 0 && a.N == 3 * a.heads * a.head_dim &&
                        (a.rows_in > 0 ? a.rows_in <= a.n_tok : a.M % a.n_tok == 0),
                    "cwm_dev_gemm: the Q/K/V scatter needs the three outputs, N = 3 * heads * head_dim and whole samples of n_tok rows (or of their first rows_in)");
        // (samples of rows_in <= n_tok rows each own n_tok output rows)
        CWM_REQUIRE(planes == 1 || a.qk_plane >= (int64_t)(a.rows_in > 0 ? a.M / a.rows_in : a.M / a.n_tok) * a.n_tok * a.heads * a.head_dim,
                    "cwm_dev_gemm: the lo plane would overlap the hi plane");
        p.q_out = (bf16*)a.q_out; p.k_out = (bf16*)a.k_out; p.v_out = (bf16*)a.v_out; p.qk_plane = a.qk_plane;
        p.qkv_dim = a.heads * a.head_dim; p.heads = a.heads; p.head_dim = a.head_dim; p.n_tok = a.n_tok; p.q_scale = a.q_scale;
    } else {
        CWM_REQUIRE(a.out && a.ldo >= a.N, "cwm_dev_gemm: the operand output needs out and rows of at least N columns");
        p.out_hi = (bf16*)a.out; p.ldo = a.ldo;
    }
    p.tune = &thread_tuning();
    GemmPlan plan;
    if (int rc = gemm_plan(p, planes, 0, gemm_cu_count(), &plan)) return rc;  // the launcher's own refusals, before anything is staged
    if (a.plan_forms) a.plan_forms[0] = plan.staged, a.plan_forms[1] = plan.direct;
    Scratch sc;
    LinearOperands op;
    if (int rc = stage_linear_operands(sc, "cwm_dev_gemm", a.a, a.w, a.bias, a.M, a.N, a.K, planes, s, &op)) return rc;
    p.A = op.A; p.W = op.W;
    p.bias = a.bias ? op.bias : nullptr;
    if (int rc = launch_gemm(p, planes, s)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize(s));
    return CWM_OK;
}

static int dev_attention(const cwm_dev_attention_args* args, const int* key_len) {
    CWM_REQUIRE(args && args->struct_size == sizeof(cwm_dev_attention_args), "cwm_dev_attention: args->struct_size must be sizeof(cwm_dev_attention_args)");
    const cwm_dev_attention_args& a = *args;
    // (launch_attention refuses this too, but only after the Q/K/V scatter below has been launched)
    CWM_REQUIRE(!key_len || a.n_q == 0, "cwm_dev_attention: per-row key counts (key_len) go with queries over all rows (n_q = 0), got n_q = %d", a.n_q);
    hipStream_t s = (hipStream_t)a.stream;
    int planes;
    if (int rc = mode_planes("cwm_dev_attention", a.mode, &planes)) return rc;
    CWM_REQUIRE(a.qkv && a.o && a.B > 0 && a.N > 0 && a.H > 0, "cwm_dev_attention: bad argument");
    CWM_REQUIRE(a.q_off >= 0 && a.n_q >= 0 && a.q_off + a.n_q <= a.N && (a.n_q > 0 || a.q_off == 0), "cwm_dev_attention: query rows [%d, %d) of %d tokens", a.q_off,
                a.q_off + a.n_q, a.N);
    const int D = a.H * 64;
    CWM_REQUIRE(a.ldo >= D && a.ldo % (planes == 2 ? 32 : 4) == 0, "cwm_dev_attention: %d columns in operand rows of ldo = %d (a multiple of 32 in parity mode, of 4 in fast mode)",
                D, a.ldo);
    Scratch sc;
    bf16* o;
    if (int rc = attention_from_qkv(sc, "cwm_dev_attention", a.qkv, key_len, (bf16*)a.o, a.ldo, a.B, a.N, a.H, a.q_off, a.n_q, planes, s, &o)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize(s));
    return CWM_OK;
}

extern "C" int cwm_dev_attention(const cwm_dev_attention_args* args) { return dev_attention(args, nullptr); }

extern "C" int cwm_dev_attention_ragged(const cwm_dev_attention_args* args, const int32_t* key_len_dev) {
    CWM_REQUIRE(key_len_dev, "cwm_dev_attention_ragged: null key_len_dev");
    return dev_attention(args, key_len_dev);
}

extern "C" int cwm_dev_layernorm(const cwm_dev_layernorm_args* args) {
    CWM_REQUIRE(args && args->struct_size == sizeof(cwm_dev_layernorm_args), "cwm_dev_layernorm: args->struct_size must be sizeof(cwm_dev_layernorm_args)");
    const cwm_dev_layernorm_args& a = *args;
    hipStream_t s = (hipStream_t)a.stream;
    int planes;
    if (int rc = mode_planes("cwm_dev_layernorm", a.mode, &planes)) return rc;
    CWM_REQUIRE(a.x && a.gamma && a.beta && a.out && a.rows > 0 && a.D > 0 && a.ldx >= a.D, "cwm_dev_layernorm: bad argument");
    CWM_REQUIRE(a.rows_out_per_b >= 0 && a.in_offset >= 0 &&
                    (a.rows_out_per_b == 0 ? a.in_offset == 0 : a.rows % a.rows_out_per_b == 0 && a.in_offset + a.rows_out_per_b <= a.rows_in_per_b),
                "cwm_dev_layernorm: %d rows as samples of %d rows at offset %d of %d", a.rows, a.rows_out_per_b, a.in_offset, a.rows_in_per_b);
    LayerNormParams ln = layernorm_rows(a.x, a.ldx, a.D, a.gamma, a.beta, a.eps, a.rows, (bf16*)a.out, a.ldo, a.rows_out_per_b, a.rows_in_per_b, a.in_offset);
    ln.out_f32 = a.out_f32;
    if (int rc = launch_layernorm(ln, planes, s)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize(s));
    return CWM_OK;
}

extern "C" int cwm_dev_fill_mask_tokens(float* x_full_dev, const float* mask_token_dev, const float* pos_dev, const int32_t* perm_dev, int B, int Nt, int n_vis,
                                        int D, void* stream) {
    CWM_REQUIRE(x_full_dev && mask_token_dev && pos_dev && perm_dev && B > 0 && D > 0 && n_vis >= 0 && n_vis <= Nt, "cwm_dev_fill_mask_tokens: bad argument");
    if (int rc = launch_fill_mask_tokens(x_full_dev, mask_token_dev, pos_dev, perm_dev, B, Nt, n_vis, D, (hipStream_t)stream)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return CWM_OK;
}

extern "C" int cwm_dev_fill_mask_tokens_ragged(float* x_full_dev, const float* mask_token_dev, const float* pos_dev, const int32_t* perm_dev,
                                               const int32_t* counts_dev, int B, int Nt, int n_vis_min, int D, void* stream) {
    CWM_REQUIRE(x_full_dev && mask_token_dev && pos_dev && perm_dev && B > 0 && Nt > 0 && D > 0, "cwm_dev_fill_mask_tokens_ragged: bad argument");
    CWM_REQUIRE(counts_dev && n_vis_min > 0, "fill_mask_tokens (ragged): bad argument");  // (the launcher would take a call without them for a rectangular batch)
    if (int rc = launch_fill_mask_tokens(x_full_dev, mask_token_dev, pos_dev, perm_dev, B, Nt, n_vis_min, D, (hipStream_t)stream, counts_dev, n_vis_min)) return rc;
    CWM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return CWM_OK;
}

// cwm_unembed with the engine's strided frames (model.hip forward_lane: x_stride_b / _c / _t of the caller's tensor): mask -> perm -> rank -> launch_unembed
// n_vis_min > 0: the ragged batch's form (forward_lane) -- rows of n_vis_min .. n_vis visible tokens, y rows = decoder rows n_vis_min ..
static int dev_unembed(const float* y_tokens_dev, const float* x_dev, int64_t x_stride_b, int64_t x_stride_c, int64_t x_stride_t, const uint8_t* mask_dev, int B, int T,
                       int C, int H, int W, int P, int n_vis_min, int n_vis, float* out_dev, void* stream) {
    CWM_REQUIRE(y_tokens_dev && x_dev && mask_dev && out_dev && B > 0 && T > 0 && C > 0 && H > 0 && W > 0, "cwm_dev_unembed: bad argument");
    CWM_REQUIRE(P > 0 && H % P == 0 && W % P == 0, "cwm_dev_unembed: image size must be divisible by the patch size");
    CWM_REQUIRE(x_stride_c >= (int64_t)H * W && x_stride_t >= 0 && x_stride_b >= 0, "cwm_dev_unembed: channel planes of %d x %d pixels at a stride of %lld", H, W,
                (long long)x_stride_c);
    const int Nt = T * (H / P) * (W / P);
    CWM_REQUIRE(n_vis >= 0 && n_vis <= Nt, "cwm_dev_unembed: n_vis = %d of %d tokens", n_vis, Nt);
    return unembed_from_mask("cwm_dev_unembed", y_tokens_dev, x_dev, x_stride_b, x_stride_c, x_stride_t, mask_dev, B, T, C, H, W, P, n_vis_min, n_vis, out_dev,
                             (hipStream_t)stream);
}

extern "C" int cwm_dev_unembed(const float* y_tokens_dev, const float* x_dev, int64_t x_stride_b, int64_t x_stride_c, int64_t x_stride_t, const uint8_t* mask_dev,
                               int B, int T, int C, int H, int W, int P, int n_vis, float* out_dev, void* stream) {
    return dev_unembed(y_tokens_dev, x_dev, x_stride_b, x_stride_c, x_stride_t, mask_dev, B, T, C, H, W, P, 0, n_vis, out_dev, stream);
}

extern "C" int cwm_dev_unembed_ragged(const float* y_tokens_dev, const float* x_dev, int64_t x_stride_b, int64_t x_stride_c, int64_t x_stride_t, const uint8_t* mask_dev,
                                      int B, int T, int C, int H, int W, int P, int n_vis_min, int n_vis, float* out_dev, void* stream) {
    CWM_REQUIRE(n_vis_min > 0, "cwm_dev_unembed_ragged: n_vis_min = %d (a ragged batch has a least count > 0)", n_vis_min);
    return dev_unembed(y_tokens_dev, x_dev, x_stride_b, x_stride_c, x_stride_t, mask_dev, B, T, C, H, W, P, n_vis_min, n_vis, out_dev, stream);
}
