// The flow samples [B, C, H, W, S] as flowstats.hip and flowfilter.hip see them: the view an entry point makes once, the facts about its layout and the kernel form every
// entry point launches for it, each stated here and nowhere else.  No HIP call: cwm_dev_flow_forms reads the forms out, tests/test_flow_forms_cpu.py holds them.
#pragma once
#include "../../include/cwm_hip.h"
#include "common.h"

namespace cwm {

// Kernels that address through all five strides take it by value.  The kernels of a contiguous layout (the packed forms: f, sb, sc; the pack kernel: f, sb, ss) take
// those members as arguments, as does flow_filter_count_kernel (see there).
struct FlowView {
    const float* f;  // element (b, c, y, x, s) at f[b sb + c sc + y sh + x sw + s ss]
    int B, C, H, W, S;
    int64_t sb, sc, sh, sw, ss;
};

// the argument checks of every entry point (`who`: its name, for the error text); filter: two channels, a square image, sizes its launch grids hold
static inline int flow_view(const char* who, bool filter, const float* flows, const int64_t* strides, int B, int C, int H, int W, int S, FlowView* v) {
    CWM_REQUIRE(flows && strides, "%s: null pointer", who);
    CWM_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1 && S >= 1, "%s: B=%d, C=%d, H=%d, W=%d, S=%d must be >= 1", who, B, C, H, W, S);
    *v = FlowView{flows, B, C, H, W, S, strides[0], strides[1], strides[2], strides[3], strides[4]};
    if (!filter) return 0;
    CWM_REQUIRE(C == 2, "%s: flow samples have C=2 channels, got C=%d", who, C);
    CWM_REQUIRE(H == W, "%s: H=%d != W=%d (the patch grid is inferred from a square image, sampling.py:186)", who, H, W);
    CWM_REQUIRE((int64_t)H * W <= (1 << 30) && S <= 65535 && B <= 65535, "%s: H W=%lld, S=%d or B=%d beyond the launch grid", who, (long long)H * W, S, B);
    return 0;
}

// A 16-byte access is safe where every stride its kernel multiplies and every address it starts from is a multiple of four floats: the forms below name them.
struct FlowLayout {
    bool packed;        // sample axis innermost, (H, W, S) contiguous (`.contiguous()`, `torch.cat(.., -1)`): a channel plane is ONE array of H W S floats
    bool planes;        // every (b, c, s) plane is H W contiguous floats
    bool sample_outer;  // planes, and a sample's C planes adjacent: the `_batch_to_samples` view of the flow model's [(b s), 1, C, H, W] output
    bool sb4, sc4, sh4, sw4, ss4;  // the stride is a multiple of four floats
    bool f16, aux16, has_aux;      // the base pointer / the entry point's other address (output, work buffer) is 16-byte aligned; that address is not null
};
static inline FlowLayout flow_layout(const FlowView& v, uintptr_t aux) {
    FlowLayout l;
    l.packed = v.ss == 1 && v.sw == v.S && v.sh == (int64_t)v.W * v.S;
    l.planes = v.sw == 1 && v.sh == v.W;
    l.sample_outer = l.planes && v.sc == (int64_t)v.H * v.W;
    l.sb4 = v.sb % 4 == 0, l.sc4 = v.sc % 4 == 0, l.sh4 = v.sh % 4 == 0, l.sw4 = v.sw % 4 == 0, l.ss4 = v.ss % 4 == 0;
    l.f16 = ((uintptr_t)v.f & 15) == 0, l.aux16 = (aux & 15) == 0, l.has_aux = aux != 0;
    return l;
}

// pixels per workgroup of the packed layout's tiles: the tile of magnitudes stays <= 34 KB, and at S = 24 a quarter as many workgroups hit the S range atomics
// (784 workgroups x 24 samples on 48 addresses were the whole 24-us launch)
static inline int mag_tile_pix(int S) { return S <= 32 ? 256 : S <= 64 ? 128 : 64; }
constexpr int kSumTilePix = 64;  // the motion map's sum pass (the range pass wants few workgroups -- fewer atomics --, the sum pass many)
static inline size_t motion_range_lds(int S) { return (size_t)mag_tile_pix(S) * (S + 1) * sizeof(float); }
static inline size_t motion_sum_lds(int S) { return ((size_t)kSumTilePix * (S + 1) + 2 * (size_t)S) * sizeof(float); }

// The forms; the values are include/cwm_hip_dev.h's CWM_DEV_FLOW_*.
enum FlowForm {
    FLOW_REFUSED = -1,
    FEATURES_SCALAR = 0, FEATURES_VEC4, MOTION_STRIDED = 0, MOTION_TILE, MOTION_ROWS16, MOTION_ROWS32, MOTION_ROWS64,
    COUNT_PLANES = 0, COUNT_PLANES_VEC, COUNT_PACKED, COUNT_PACKED_VEC, FINISH_V1 = 0, FINISH_V4,
    ZERO_PLANES = 0, ZERO_PLANES_VEC, ZERO_SCATTER, PACK_TRANSPOSE = 0,
    VOTE_STRIDED = 0, VOTE_PLANES_VEC, VOTE_PACKED,  // (cwm_segment_step; not read out by cwm_dev_flow_forms)
};

// cwm_flow_features (aux: the output): four samples per thread
static inline FlowForm flow_features_form(const FlowView& v, const FlowLayout& l) {
    return v.ss == 1 && v.S % 4 == 0 && l.f16 && l.aux16 && l.sb4 && l.sc4 && l.sh4 && l.sw4 ? FEATURES_VEC4 : FEATURES_SCALAR;
}
// cwm_flow_motion_sum (aux: the work buffer of per-sample normalisation).  Packed: the rows form where S = 64, 128 or 256 k, else the LDS tile while it fits; else strided.
static inline FlowForm flow_motion_form(const FlowView& v, const FlowLayout& l, bool normalize_per_sample) {
    if (normalize_per_sample && !l.has_aux) return FLOW_REFUSED;
    const FlowForm rows = v.S == 64 ? MOTION_ROWS16 : v.S == 128 ? MOTION_ROWS32 : v.S % 256 == 0 ? MOTION_ROWS64 : MOTION_STRIDED;
    if (!l.packed) return MOTION_STRIDED;
    if (rows != MOTION_STRIDED && l.sb4 && l.sc4 && l.f16 && (!normalize_per_sample || l.aux16)) return rows;
    return motion_range_lds(v.S) <= 150 * 1024 && motion_sum_lds(v.S) <= 150 * 1024 ? MOTION_TILE : MOTION_STRIDED;
}
// cwm_flow_filter_stats, the counting pass (packed: 2 S counters in LDS; any other strides take the scalar form of the planes kernel) ...
static inline FlowForm flow_count_form(const FlowView& v, const FlowLayout& l) {
    const bool base4 = l.f16 && l.sb4 && l.sc4;
    if (l.packed && v.S <= 8192) return base4 && v.S % 4 == 0 ? COUNT_PACKED_VEC : COUNT_PACKED;
    return l.planes && (v.H * v.W) % 4 == 0 && base4 && l.ss4 ? COUNT_PLANES_VEC : COUNT_PLANES;
}
// ... and its finish: the mask bytes of four samples as one 32-bit load (mask [B, 2 hw, S] bytes with strides (b, patch, s); the kernel reads frame 2, from row hw)
static inline FlowForm flow_finish_form(int S, const int64_t* mask_strides, uintptr_t mask, int hw) {
    const uintptr_t frame2 = mask + (uintptr_t)((int64_t)hw * mask_strides[1]);
    return mask_strides[2] == 1 && S % 4 == 0 && mask_strides[0] % 4 == 0 && mask_strides[1] % 4 == 0 && (frame2 & 3) == 0 ? FINISH_V4 : FINISH_V1;
}
// cwm_flow_filter_apply (scatter: the list of rejected samples, S entries, in LDS)
static inline FlowForm flow_zero_form(const FlowView& v, const FlowLayout& l) {
    if (l.planes) return (v.H * v.W) % 4 == 0 && l.f16 && l.sb4 && l.sc4 && l.ss4 ? ZERO_PLANES_VEC : ZERO_PLANES;
    return v.S <= 8192 ? ZERO_SCATTER : FLOW_REFUSED;
}
static inline FlowForm flow_pack_form(const FlowLayout& l) { return l.sample_outer ? PACK_TRANSPOSE : FLOW_REFUSED; }
// cwm_segment_step, the vote pass (aux: the votes, [B][H W] bytes).  Packed: a tile of 64 pixels x S samples per workgroup, read as consecutive floats.  Planes (the
// sample-outermost view among them): four pixels per thread as 16-byte loads and one 4-byte store of their votes, where the addresses allow it.  Everything else, and
// planes that do not, takes the one-pixel-per-thread form through all five strides -- still coalesced on planes, where adjacent threads read adjacent floats.
constexpr int kVoteTilePix = 64;
static inline FlowForm flow_vote_form(const FlowView& v, const FlowLayout& l) {
    if (l.packed && v.S > 1) return VOTE_PACKED;
    return l.planes && (v.H * v.W) % 4 == 0 && l.f16 && l.sb4 && l.sc4 && l.ss4 && l.aux16 ? VOTE_PLANES_VEC : VOTE_STRIDED;
}

// ---- the magnitude: TWO forms, because hipcc rounds them differently and an ulp would move patch_mag or a threshold decision.  The statistics sum v v
// over the channels from zero; T = float, or f32x4: four adjacent elements as one 16-byte load (f + c sc stays workgroup-uniform where `off` carries the lane's part).
template <class T>
__device__ __forceinline__ T flow_mag_sq(const float* f, int64_t sc, int C, int64_t off = 0) {
    T a{};
    for (int c = 0; c < C; ++c) {
        const T v = *reinterpret_cast<const T*>(f + c * sc + off);
        a += v * v;
    }
    return a;
}
__device__ __forceinline__ float flow_mag2(float a, float c) { return sqrtf(a * a + c * c); }

}  // namespace cwm
