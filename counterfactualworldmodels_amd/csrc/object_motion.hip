// Per-object motion and occlusion order (cwm_object_motion): one pass over the slot map of frame A, the flow from A to the other frame and -- where given -- the
// codes of cwm_flow_consistency and the other frame's slot map, into one table per row and slot: pixel counts by class, the integer sums a least-squares affine
// fit needs, the fit itself (translation, 2 x 2 matrix, centroid, flow variance) and a 65 x 65 table of who was hidden behind whom.  Slot 0, everything that is
// no object, is summed like any other: its model is the camera's own motion.  No counterpart in the reference, whose README lists read-outs of this kind as
// coming ("using counterfactuals to estimate other scene properties").
//
// The definition (this is the contract; include/cwm_hip.h repeats it for callers).  Rows r = b T + t, b < B, t < T.  Every input plane is H W contiguous elements
// at base + b strides[0] + t strides[1] (elements; the flow has a third stride for its channel, 0 horizontal and 1 vertical), so a [B,T,H,W] buffer, a [:, :-1] or
// [:, 1:] slice of one and a plain [B,H,W] (T = 1) are read in place.  labels: the slot map of frame A; flow: from A to the other frame, on A's grid, in pixels;
// code (may be NULL): what cwm_flow_consistency wrote for this flow; other (may be NULL): the slot map of the other frame.  Per row and pixel (x, y):
//   1 slot     l = labels[y][x], or 0 if that is above 64
//   2 target   (u, v) = flow[:, y, x]; USABLE iff both are finite and |u| <= 4096 and |v| <= 4096; fx = (float)x + u, fy = (float)y + v (one fp32 add each);
//              INSIDE iff fx >= 0 && fx <= W-1 && fy >= 0 && fy <= H-1, in fp32 and before anything is converted: step 1 of cwm_flow_consistency
//   3 class    k = 2 if the vector is not usable or the pixel not inside; otherwise 1 if code is given and code[y][x] != 0; otherwise 0.  counts[l][k] += 1 (int32;
//              counts[l][3] stays 0)
//   4 sums     k = 0 only: qu = (int)rintf(u * 256.0f), qv likewise -- the multiply is exact, |q| <= 2^20, the flow is held in 1/256 px.  sums[l][0..13] (int64)
//              += 1, x, y, x x, x y, y y, qu, qv, x qu, y qu, x qv, y qv, qu qu, qv qv; entries 14 and 15 stay 0.  x, y < 2^16 (H W <= 2^18 and both are multiples
//              of 4), so over the at most 2^18 pixels of a row sum x x <= 2^50, sum x qu <= 2^54 and sum qu qu <= 2^58: nothing wraps
//   5 occluder k = 1 only, and only with other: m = other[(int)rintf(fy)][(int)rintf(fx)], or 0 if that is above 64; occ[l][m] += 1 (int32 [65][65]).  The row is
//              the slot that was hidden, the column what stands there in the other frame; the index is in range because the pixel is inside; the diagonal is
//              counted too (a flow that is wrong on the object itself)
//   6 model    per row and slot, after all pixels, twelve float64 values.  Every operator is ONE correctly rounded binary64 operation, evaluated as parenthesised:
//              no fused multiply-add, no reciprocal; a sum enters through a round-to-nearest int64 -> double conversion.  n = (double)N, N = sums[l][0]:
//                mx = (Sx/n)  my = (Sy/n)  mu = (Su/n)  mv = (Sv/n)
//                cxx = ((Sxx/n) - (mx mx))  cxy = ((Sxy/n) - (mx my))  cyy = ((Syy/n) - (my my))
//                cxu = ((Sxu/n) - (mx mu))  cyu = ((Syu/n) - (my mu))  cxv = ((Sxv/n) - (mx mv))  cyv = ((Syv/n) - (my mv))
//                det = ((cxx cyy) - (cxy cxy))
//                tu = (mu 2^-8)  tv = (mv 2^-8)  var_u = (((Suu/n) - (mu mu)) 2^-16)  var_v = (((Svv/n) - (mv mv)) 2^-16)
//                a11 = ((((cxu cyy) - (cyu cxy)) / det) 2^-8)  a12 = ((((cyu cxx) - (cxu cxy)) / det) 2^-8)  a21, a22: the same with cxv, cyv
//              model[l] = (valid, tu, tv, a11, a12, a21, a22, mx, my, var_u, var_v, 0): the predicted flow of a pixel of the object is t + A ((x, y) - (mx, my)).
//              valid = 0 and all twelve 0 if N < min_pixels; valid = 2 if N >= min_affine and det >= min_det; otherwise valid = 1 and A = 0 (a NaN det cannot
//              occur; the comparison is written so that one would give 1)
// Outputs: sums int64 [R][65][16], counts int32 [R][65][4], model float64 [R][65][12], occ int32 [R][65][65] (given iff other is given).
//
// Two kernels behind the memsets of the three integer tables, all on base.stream.  What was chosen, and why:
//   accumulate  grid (chunks of 1024 pixels, R), 256 threads.  A thread owns 4 consecutive pixels of an image row: a 16-byte load of u and of v, 4-byte loads of the
//               label and code bytes (narrow loads where an address or a stride is not aligned; the host picks the instantiation).  The workgroup's tables live
//               in LDS: 65 x 14 int64, 65 x 4 int32 and (with other) 65 x 65 int32, 25 KB together; at the end only the non-zero entries go to global memory, as
//               INTEGER atomics into the tables the call zeroed, and the occluder table only from a workgroup that met a class-1 pixel.  Labels are spatially
//               coherent: a lane collapses the runs of its four pixels (the terms with y follow from the others at the end of a run), and the slot of a wave's
//               first lane is summed over the wave -- four DPP steps within the rows of 16 lanes, then lanes 0, 16, 32 and 48 read out; five of the terms fit 32
//               bits over a wave and the counts are packed into one word -- and added by one lane with one set of LDS atomics: a wave whose 64 lanes hold one
//               slot, the common case, is done with that.  The lanes of other slots (a wave across an object's edge, many slots in one wave) and the runs that
//               end inside a lane add per lane.  The occluder look-up is a byte gather per class-1 pixel (rare; the map is at most 256 KB) and one LDS atomic.
//               What was measured on the way: a workgroup is one wave per SIMD and nothing hides its latency, so 4096 pixels per workgroup in
//               four steps took 17 - 26 us at 224 x 224 where 1024 pixels take 8 - 12 us; with six __shfl_xor steps per word in place of the DPP steps the
//               former took 48 us; summing a second and a third slot of a wave the same way was not faster than letting their lanes add
//   finalise    one thread per (row, slot): step 6 on the finished sums
// Integer atomics give the same bits in any order: two calls on the same inputs give the same bits.  There is no workspace.  No content of a device buffer moves
// an address beyond what the geometry allows: label bytes are tested against 64 before they index a table, and the occluder's source is tested in fp32 before it
// is converted.
#include <cstring>

#include "../../include/cwm_hip.h"
#include "common.h"
#include "wave_sum.h"

#pragma clang fp contract(off)  // (file scope: a*b-c stays a multiply and a subtraction, in fp32 and in binary64)

namespace cwm {

namespace {

constexpr int kMotSlots = 64;
constexpr int kMotSide = kMotSlots + 1;  // slots 0 .. 64
constexpr int kMotTerms = 14, kMotSumStride = 16, kMotModel = 12;
constexpr int kMotMaxPixels = 1 << 18;
constexpr int kMotThreads = 256;
constexpr int kMotGroupPixels = 4 * kMotThreads;  // 4 pixels per thread

struct MotParams {
    const uint8_t *labels, *code, *other;
    const float* flow;
    int64_t ls0, ls1, fs0, fs1, fs2, cs0, cs1, os0, os1;
    int R, T, H, W;
    int min_pixels, min_affine;
    double min_det;
    unsigned long long* sums;
    int *counts, *occ;
    double* model;
};

// what a lane has gathered for one slot: the class counts packed 10 bits each (at most 4 per lane, 256 per wave) and the 14 terms of step 4, the five that stay
// below 2^31 over a whole wave in 32 bits
struct MotAcc {
    int cls;
    int n, sx, sy, su, sv;
    long long sxx, sxy, syy, sxu, syu, sxv, syv, suu, svv;
};

__device__ __forceinline__ void mot_clear(MotAcc& a) {
    a.cls = 0, a.n = 0, a.sx = 0, a.sy = 0, a.su = 0, a.sv = 0;
    a.sxx = 0, a.sxy = 0, a.syy = 0, a.sxu = 0, a.syu = 0, a.sxv = 0, a.syv = 0, a.suu = 0, a.svv = 0;
}

// the four pixels of a lane lie in one image row, so the terms with y follow from the others when a run ends
__device__ __forceinline__ void mot_close_run(MotAcc& a, int y) {
    a.sy = a.n * y;
    a.sxy = (long long)y * a.sx, a.syy = (long long)y * y * a.n, a.syu = (long long)y * a.su, a.syv = (long long)y * a.sv;
}

__device__ __forceinline__ void mot_lds_add(unsigned long long* q, long long v) { atomicAdd(q, (unsigned long long)v); }

// one set of LDS atomics for slot l; zero terms are not issued
__device__ __forceinline__ void mot_flush(const MotAcc& a, int l, unsigned long long* sum_s, int* cnt_s) {
    if (a.cls & 0x3ff) atomicAdd(&cnt_s[4 * l], a.cls & 0x3ff);
    if ((a.cls >> 10) & 0x3ff) atomicAdd(&cnt_s[4 * l + 1], (a.cls >> 10) & 0x3ff);
    if (a.cls >> 20) atomicAdd(&cnt_s[4 * l + 2], a.cls >> 20);
    if (a.n) {
        unsigned long long* s = sum_s + kMotTerms * l;
        mot_lds_add(s + 0, a.n), mot_lds_add(s + 1, a.sx), mot_lds_add(s + 2, a.sy);
        mot_lds_add(s + 3, a.sxx), mot_lds_add(s + 4, a.sxy), mot_lds_add(s + 5, a.syy);
        if (a.su) mot_lds_add(s + 6, a.su);
        if (a.sv) mot_lds_add(s + 7, a.sv);
        if (a.sxu) mot_lds_add(s + 8, a.sxu);
        if (a.syu) mot_lds_add(s + 9, a.syu);
        if (a.sxv) mot_lds_add(s + 10, a.sxv);
        if (a.syv) mot_lds_add(s + 11, a.syv);
        if (a.suu) mot_lds_add(s + 12, a.suu);
        if (a.svv) mot_lds_add(s + 13, a.svv);
    }
}

template <bool kVec>
__device__ __forceinline__ void mot_load4(const float* q, float (&f)[4]) {
    if (kVec) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        f[0] = t.x, f[1] = t.y, f[2] = t.z, f[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = q[i];
    }
}
template <bool kVec>
__device__ __forceinline__ unsigned mot_load4(const uint8_t* q) {
    if (kVec) return *reinterpret_cast<const unsigned*>(q);
    return (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | ((unsigned)q[3] << 24);
}

// grid (chunks of 1024 pixels, R).  kVec: the flow planes of every row are 16-byte aligned and the byte planes 4-byte aligned (the host decides)
template <bool kVec>
__global__ __launch_bounds__(kMotThreads) void object_motion_accumulate_kernel(const MotParams p) {
    __shared__ unsigned long long sum_s[kMotSide * kMotTerms];
    __shared__ int cnt_s[kMotSide * 4];
    __shared__ int occ_s[kMotSide * kMotSide];
    __shared__ int occ_used_s;  // (most workgroups meet no class-1 pixel and have nothing of occ_s to add)
    const int r = blockIdx.y, tid = threadIdx.x, W = p.W, H = p.H, quads = (H * W) >> 2;
    const int b = r / p.T, t = r - b * p.T;
    for (int e = tid; e < kMotSide * kMotTerms; e += kMotThreads) sum_s[e] = 0;
    for (int e = tid; e < kMotSide * 4; e += kMotThreads) cnt_s[e] = 0;
    if (p.other) {
        for (int e = tid; e < kMotSide * kMotSide; e += kMotThreads) occ_s[e] = 0;
        if (tid == 0) occ_used_s = 0;
    }
    __syncthreads();
    const uint8_t* lab = p.labels + b * p.ls0 + t * p.ls1;
    const float* fu = p.flow + b * p.fs0 + t * p.fs1;
    const float* fv = fu + p.fs2;
    const uint8_t* cod = p.code ? p.code + b * p.cs0 + t * p.cs1 : nullptr;
    const uint8_t* oth = p.other ? p.other + b * p.os0 + t * p.os1 : nullptr;
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    const int g = blockIdx.x * kMotThreads + tid;  // the group of 4 pixels; consecutive over the lanes of a wave
    const bool live = g < quads;
    if (__any(live)) {  // (wave-uniform; a wave past the plane has nothing to add)
        const int pix = live ? 4 * g : 0;
        const int y = pix / W, x0 = pix - y * W;  // W is a multiple of 4: the four pixels lie in one image row
        unsigned lw = 0, cw = 0;
        float u[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            lw = mot_load4<kVec>(lab + pix);
            mot_load4<kVec>(fu + pix, u);
            mot_load4<kVec>(fv + pix, v);
            if (cod) cw = mot_load4<kVec>(cod + pix);
        }
        int l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s = (int)((lw >> (8 * j)) & 0xffu);
            l[j] = s <= kMotSlots ? s : 0;
        }
        MotAcc a;
        mot_clear(a);
        int cur = l[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (l[j] != cur) {  // a run of the lane ends inside its four pixels (an object's edge): the lane adds it on its own
                mot_close_run(a, y);
                mot_flush(a, cur, sum_s, cnt_s);
                mot_clear(a);
                cur = l[j];
            }
            const int x = x0 + j;
            const bool usable = fabsf(u[j]) <= 4096.f && fabsf(v[j]) <= 4096.f;  // (false for a NaN and for an inf)
            const float fx = (float)x + u[j], fy = (float)y + v[j];
            const bool inside = fx >= 0.f && fx <= xmax && fy >= 0.f && fy <= ymax;
            const int k = !(usable && inside) ? 2 : (((cw >> (8 * j)) & 0xffu) ? 1 : 0);
            if (live) a.cls += 1 << (10 * k);
            if (live && k == 0) {
                const int qu = (int)rintf(u[j] * 256.0f), qv = (int)rintf(v[j] * 256.0f);
                a.n += 1, a.sx += x, a.su += qu, a.sv += qv;
                a.sxx += (long long)x * x, a.sxu += (long long)x * qu, a.sxv += (long long)x * qv;
                a.suu += (long long)qu * qu, a.svv += (long long)qv * qv;
            }
            if (live && k == 1 && oth) {  // (inside: 0 <= rintf(fx) <= W-1 and 0 <= rintf(fy) <= H-1)
                const int s = (int)oth[(int)rintf(fy) * W + (int)rintf(fx)];
                atomicAdd(&occ_s[kMotSide * l[j] + (s <= kMotSlots ? s : 0)], 1);
                occ_used_s = 1;
            }
        }
        mot_close_run(a, y);
        // every lane now holds (cur, a), its last run.  The slot of the wave's first lane (it holds the lowest group: it is live whenever a lane of the wave is) is
        // summed over the wave -- every lane takes part, a lane of another slot or past the plane with zeros -- and added by one lane: a wave of one slot, the
        // common case, is done with that.  The lanes of other slots (a wave across an object's edge, or many slots in one wave) add per lane
        const int slot = __shfl(cur, 0, 64);
        const bool mine = live && cur == slot;
        MotAcc w;
        mot_clear(w);
        if (mine) w = a;
        w.cls = wave_sum(w.cls);
        w.n = wave_sum(w.n);
        if (w.n) {  // (uniform after the sum)
            w.sx = wave_sum(w.sx), w.sy = wave_sum(w.sy), w.su = wave_sum(w.su), w.sv = wave_sum(w.sv);
            w.sxx = wave_sum(w.sxx), w.sxy = wave_sum(w.sxy), w.syy = wave_sum(w.syy);
            w.sxu = wave_sum(w.sxu), w.syu = wave_sum(w.syu), w.sxv = wave_sum(w.sxv), w.syv = wave_sum(w.syv);
            w.suu = wave_sum(w.suu), w.svv = wave_sum(w.svv);
        }
        if ((tid & 63) == 0) mot_flush(w, slot, sum_s, cnt_s);
        if (live && !mine) mot_flush(a, cur, sum_s, cnt_s);
    }
    __syncthreads();
    unsigned long long* gs = p.sums + (size_t)r * kMotSide * kMotSumStride;
    for (int e = tid; e < kMotSide * kMotTerms; e += kMotThreads) {
        const unsigned long long s = sum_s[e];
        if (s) atomicAdd(&gs[(e / kMotTerms) * kMotSumStride + e % kMotTerms], s);
    }
    int* gc = p.counts + (size_t)r * kMotSide * 4;
    for (int e = tid; e < kMotSide * 4; e += kMotThreads) {
        const int c = cnt_s[e];
        if (c) atomicAdd(&gc[e], c);
    }
    if (p.other && occ_used_s) {
        int* go = p.occ + (size_t)r * kMotSide * kMotSide;
        for (int e = tid; e < kMotSide * kMotSide; e += kMotThreads) {
            const int c = occ_s[e];
            if (c) atomicAdd(&go[e], c);
        }
    }
}

// one thread per (row, slot): step 6.  Every line is one binary64 operation (the file is compiled without contraction)
__global__ __launch_bounds__(kMotThreads) void object_motion_finalise_kernel(const MotParams p) {
    const int e = blockIdx.x * kMotThreads + threadIdx.x;
    if (e >= p.R * kMotSide) return;
    const long long* S = reinterpret_cast<const long long*>(p.sums) + (size_t)e * kMotSumStride;
    double* m = p.model + (size_t)e * kMotModel;
    const long long N = S[0];
    double out[kMotModel];
#pragma unroll
    for (int i = 0; i < kMotModel; ++i) out[i] = 0.0;
    if (N >= (long long)p.min_pixels) {
        const double n = (double)N;
        const double mx = (double)S[1] / n, my = (double)S[2] / n, mu = (double)S[6] / n, mv = (double)S[7] / n;
        const double cxx = ((double)S[3] / n) - (mx * mx), cxy = ((double)S[4] / n) - (mx * my), cyy = ((double)S[5] / n) - (my * my);
        const double cxu = ((double)S[8] / n) - (mx * mu), cyu = ((double)S[9] / n) - (my * mu);
        const double cxv = ((double)S[10] / n) - (mx * mv), cyv = ((double)S[11] / n) - (my * mv);
        const double det = (cxx * cyy) - (cxy * cxy);
        const double scale = 0.00390625, scale2 = 0.0000152587890625;  // 2^-8, 2^-16
        const bool affine = N >= (long long)p.min_affine && det >= p.min_det;  // (a NaN det compares false)
        out[0] = affine ? 2.0 : 1.0;
        out[1] = mu * scale, out[2] = mv * scale;
        if (affine) {
            out[3] = (((cxu * cyy) - (cyu * cxy)) / det) * scale;
            out[4] = (((cyu * cxx) - (cxu * cxy)) / det) * scale;
            out[5] = (((cxv * cyy) - (cyv * cxy)) / det) * scale;
            out[6] = (((cyv * cxx) - (cxv * cxy)) / det) * scale;
        }
        out[7] = mx, out[8] = my;
        out[9] = (((double)S[12] / n) - (mu * mu)) * scale2;
        out[10] = (((double)S[13] / n) - (mv * mv)) * scale2;
    }
#pragma unroll
    for (int i = 0; i < kMotModel; ++i) m[i] = out[i];
}

}  // namespace

}  // namespace cwm

using namespace cwm;

extern "C" int cwm_object_motion(const cwm_object_motion_args* a) {
    CWM_REQUIRE(a && a->struct_size == sizeof(cwm_object_motion_args), "cwm_object_motion: args->struct_size must be sizeof(cwm_object_motion_args)");
    const cwm_patch_error_args& g = a->base;
    CWM_REQUIRE(g.batch >= 1 && g.batch <= 65535, "cwm_object_motion: base.batch = %d, 1 .. 65535", g.batch);
    CWM_REQUIRE(g.T >= 1 && (int64_t)g.batch * g.T <= 65535, "cwm_object_motion: base.T = %d: at least 1, and base.batch base.T at most 65535 rows", g.T);
    CWM_REQUIRE(g.H > 0 && g.H % 4 == 0, "cwm_object_motion: base.H = %d must be a positive multiple of 4", g.H);
    CWM_REQUIRE(g.W > 0 && g.W % 4 == 0, "cwm_object_motion: base.W = %d must be a positive multiple of 4", g.W);
    CWM_REQUIRE((int64_t)g.H * g.W <= kMotMaxPixels, "cwm_object_motion: base.H base.W = %lld pixels, at most %d", (long long)g.H * g.W, kMotMaxPixels);
    CWM_REQUIRE(a->labels_dev, "cwm_object_motion: labels_dev is NULL");
    CWM_REQUIRE(a->flow_dev, "cwm_object_motion: flow_dev is NULL");
    CWM_REQUIRE(a->labels_strides[0] >= 0 && a->labels_strides[1] >= 0, "cwm_object_motion: labels_strides = (%lld, %lld) must not be negative",
                (long long)a->labels_strides[0], (long long)a->labels_strides[1]);
    CWM_REQUIRE(a->flow_strides[0] >= 0 && a->flow_strides[1] >= 0 && a->flow_strides[2] >= 0,
                "cwm_object_motion: flow_strides = (%lld, %lld, %lld) must not be negative", (long long)a->flow_strides[0], (long long)a->flow_strides[1],
                (long long)a->flow_strides[2]);
    CWM_REQUIRE(!a->code_dev || (a->code_strides[0] >= 0 && a->code_strides[1] >= 0), "cwm_object_motion: code_strides = (%lld, %lld) must not be negative",
                (long long)a->code_strides[0], (long long)a->code_strides[1]);
    CWM_REQUIRE(!a->other_dev || (a->other_strides[0] >= 0 && a->other_strides[1] >= 0), "cwm_object_motion: other_strides = (%lld, %lld) must not be negative",
                (long long)a->other_strides[0], (long long)a->other_strides[1]);
    CWM_REQUIRE(a->min_pixels >= 1, "cwm_object_motion: min_pixels = %d, at least 1", a->min_pixels);
    CWM_REQUIRE(a->min_affine >= 3, "cwm_object_motion: min_affine = %d, at least 3", a->min_affine);
    CWM_REQUIRE(a->min_det > 0.0 && a->min_det <= 1.7976931348623157e308, "cwm_object_motion: min_det = %g must be finite and positive", a->min_det);
    CWM_REQUIRE(a->sums_dev, "cwm_object_motion: sums_dev is NULL");
    CWM_REQUIRE(a->counts_dev, "cwm_object_motion: counts_dev is NULL");
    CWM_REQUIRE(a->model_dev, "cwm_object_motion: model_dev is NULL");
    CWM_REQUIRE(!a->occ_dev || a->other_dev, "cwm_object_motion: occ_dev is given without other_dev");
    CWM_REQUIRE(a->occ_dev || !a->other_dev, "cwm_object_motion: other_dev is given without occ_dev");
    MotParams p;
    memset(&p, 0, sizeof(p));
    p.labels = a->labels_dev, p.ls0 = a->labels_strides[0], p.ls1 = a->labels_strides[1];
    p.flow = a->flow_dev, p.fs0 = a->flow_strides[0], p.fs1 = a->flow_strides[1], p.fs2 = a->flow_strides[2];
    p.code = a->code_dev, p.cs0 = a->code_strides[0], p.cs1 = a->code_strides[1];
    p.other = a->other_dev, p.os0 = a->other_strides[0], p.os1 = a->other_strides[1];
    p.R = g.batch * g.T, p.T = g.T, p.H = g.H, p.W = g.W;
    p.min_pixels = a->min_pixels, p.min_affine = a->min_affine, p.min_det = a->min_det;
    p.sums = reinterpret_cast<unsigned long long*>(a->sums_dev), p.counts = a->counts_dev, p.occ = a->occ_dev, p.model = a->model_dev;
    hipStream_t stream = (hipStream_t)g.stream;
    // the tables the workgroups add into
    CWM_HIP_CHECK(hipMemsetAsync(p.sums, 0, (size_t)p.R * kMotSide * kMotSumStride * sizeof(long long), stream));
    CWM_HIP_CHECK(hipMemsetAsync(p.counts, 0, (size_t)p.R * kMotSide * 4 * sizeof(int), stream));
    if (p.occ) CWM_HIP_CHECK(hipMemsetAsync(p.occ, 0, (size_t)p.R * kMotSide * kMotSide * sizeof(int), stream));
    // wide loads need every plane on its alignment: the base on it and the strides (elements) multiples of 4 (H W % 16 == 0 does the rest)
    const auto misaligned = [](const void* q, uintptr_t mask, int64_t s0, int64_t s1, int64_t s2) {
        return ((reinterpret_cast<uintptr_t>(q) & mask) | (uintptr_t)((s0 | s1 | s2) & 3)) != 0;
    };
    const bool vec = !misaligned(p.labels, 3, p.ls0, p.ls1, 0) && !misaligned(p.flow, 15, p.fs0, p.fs1, p.fs2) && !misaligned(p.code, 3, p.cs0, p.cs1, 0);
    const dim3 grid((unsigned)((p.H * p.W + kMotGroupPixels - 1) / kMotGroupPixels), (unsigned)p.R), block(kMotThreads);
    if (vec) hipLaunchKernelGGL((object_motion_accumulate_kernel<true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((object_motion_accumulate_kernel<false>), grid, block, 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(object_motion_finalise_kernel, dim3((unsigned)((p.R * kMotSide + kMotThreads - 1) / kMotThreads)), block, 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}
