// The flow-sample filter on the device: which of the S counterfactual flow samples does `sample_counterfactual_motion_map` keep?
//
// Replaces (cwm/models/sampling.py):
//   FlowSampleFilter.compute_flow_magnitude    :163-205  norm over the channels ([B,H,W,S] materialised), a permuted bilinear resize of ALL of it to the patch
//                                                        grid, the mean over the active patches of frame 2
//   FlowSampleFilter.filter_by_patch_magnitude :207-215  patch_mag < flow_magnitude_threshold
//   FlowSampleFilter.filter_by_flow_area       :217-228  count(|flow| > flow_magnitude_threshold) / (H W) > flow_area_threshold
//   FlowSampleFilter.filter_by_num_corners     :230-250  #corner pixels over the threshold >= num_corners_threshold
//   FlowSampleFilter.forward                   :252-286  the OR of the enabled tests; rejected samples are zeroed in place through an expanded boolean mask
//
// cwm_flow_filter_stats: a streaming pass reads every flow element once and counts, per (b, s), the pixels (and corner pixels) whose magnitude exceeds the
// threshold -- integer counts, so block partials are combined with integer atomics and the result does not depend on the order.  The patch mean needs the
// bilinearly resized magnitude at the ACTIVE patches only: the finish kernel scans the mask of frame 2 and evaluates the four taps of each active patch (8
// floats per active patch, out of 2 H W per sample), adds them in a FIXED order (64 contiguous chunks of the patch axis, in patch order inside a chunk, chunks in
// order) and writes patch_mag, the decision and nothing else.  Two launches on the same input give the same bits, whatever the layout of the flows.
// cwm_flow_filter_apply writes zeros over the rejected samples and reads no flow element; cwm_flow_filter_pack transposes the sample-outermost batch into the
// packed [B,2,H,W,S] tensor the reference returns (`.contiguous()`), writing zeros for rejected samples without reading them.
//
// Layouts and which form a launch takes: flow_view.h.  "planes" are read with 16-byte loads along the pixels, "packed" along the samples, anything else 4 bytes at a time.
#include <cmath>

#include "../../include/cwm_hip.h"
#include "common.h"
#include "flow_view.h"
#include "kernels.h"

namespace cwm {

constexpr int kFiltPixPerBlock = 4096;  // planes form: 256 threads x 16 pixels
constexpr int kFinRows = 64;            // finish: the patch axis is cut into 64 contiguous chunks; chunk partials are added in chunk order

// how many of the reference's four corner reads (top-left, top-right, bottom-left, bottom-right) land on pixel e
__device__ __forceinline__ int corner_hits(int e, int W, int HW) { return (e == 0) + (e == W - 1) + (e == HW - W) + (e == HW - 1); }

__device__ __forceinline__ void block_add2(int cnt, int cor, int* __restrict__ area, int* __restrict__ corner) {
    __shared__ int red[2][4];
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
        cor += __shfl_xor(cor, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = cnt;
        red[1][threadIdx.x >> 6] = cor;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int a = red[0][0] + red[0][1] + red[0][2] + red[0][3], c = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        if (a) atomicAdd(area, a);
        if (c) atomicAdd(corner, c);
    }
}

// one (b, s) per blockIdx.(z, y), kFiltPixPerBlock pixels per blockIdx.x.  VEC: contiguous, 16-byte aligned planes of a multiple of 4 pixels.
// (Not on a FlowView: from a struct hipcc vectorises the scalar loop eight wide instead of two, 107 registers instead of 28.)
template <int VEC>
__global__ __launch_bounds__(256) void flow_filter_count_kernel(const float* __restrict__ f, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int64_t ss, int H,
                                                                int W, int S, float thr, int* __restrict__ area, int* __restrict__ corner) {
    const int s = blockIdx.y, b = blockIdx.z, HW = H * W;
    const float* u = f + b * sb + s * ss;
    const float* v = u + sc;
    const int e0 = blockIdx.x * kFiltPixPerBlock, e1 = min(e0 + kFiltPixPerBlock, HW);
    int cnt = 0, cor = 0;
    if (VEC) {
        for (int e = e0 + 4 * (int)threadIdx.x; e < e1; e += 1024) {  // e % 4 == 0 and HW % 4 == 0: e + 3 < e1
            const float4 a = *reinterpret_cast<const float4*>(u + e), c = *reinterpret_cast<const float4*>(v + e);
            const float m[4] = {flow_mag2(a.x, c.x), flow_mag2(a.y, c.y), flow_mag2(a.z, c.z), flow_mag2(a.w, c.w)};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (m[k] > thr) {
                    ++cnt;
                    cor += corner_hits(e + k, W, HW);
                }
        }
    } else {
        for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {
            const int y = e / W, x = e - y * W;
            const int64_t off = (int64_t)y * sh + (int64_t)x * sw;
            if (flow_mag2(u[off], v[off]) > thr) {
                ++cnt;
                cor += corner_hits(e, W, HW);
            }
        }
    }
    block_add2(cnt, cor, area + (size_t)b * S + s, corner + (size_t)b * S + s);
}

// packed layout: a workgroup takes tile_pix consecutive pixels = tile_pix * S consecutive floats per channel; per-sample counts in LDS (integer atomics), then one
// global atomic per (workgroup, sample with a non-zero count).  VEC: S % 4 == 0 (a 16-byte load = 4 samples of one pixel), aligned base and strides.
template <int VEC>
__global__ __launch_bounds__(256) void flow_filter_count_packed_kernel(const float* __restrict__ f, int64_t sb, int64_t sc, int HW, int W, int S, int tile_pix,
                                                                       float thr, int* __restrict__ area, int* __restrict__ corner) {
    extern __shared__ int cnt[];  // [S] area, [S] corners
    const int b = blockIdx.y, pix0 = blockIdx.x * tile_pix;
    const int npix = min(tile_pix, HW - pix0), n = npix * S;
    for (int s = threadIdx.x; s < 2 * S; s += blockDim.x) cnt[s] = 0;
    __syncthreads();
    const float* u = f + b * sb + (int64_t)pix0 * S;
    const float* v = u + sc;
    if (VEC) {
        for (int e = 4 * (int)threadIdx.x; e < n; e += 1024) {  // n % 4 == 0
            const float4 a = *reinterpret_cast<const float4*>(u + e), c = *reinterpret_cast<const float4*>(v + e);
            const float m[4] = {flow_mag2(a.x, c.x), flow_mag2(a.y, c.y), flow_mag2(a.z, c.z), flow_mag2(a.w, c.w)};
            if (m[0] > thr || m[1] > thr || m[2] > thr || m[3] > thr) {
                const int p = e / S, s = e - p * S, ch = corner_hits(pix0 + p, W, HW);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (m[k] > thr) {
                        atomicAdd(&cnt[s + k], 1);
                        if (ch) atomicAdd(&cnt[S + s + k], ch);
                    }
            }
        }
    } else {
        for (int e = threadIdx.x; e < n; e += 256) {
            if (flow_mag2(u[e], v[e]) > thr) {
                const int p = e / S, s = e - p * S, ch = corner_hits(pix0 + p, W, HW);
                atomicAdd(&cnt[s], 1);
                if (ch) atomicAdd(&cnt[S + s], ch);
            }
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
        if (cnt[s]) atomicAdd(&area[(size_t)b * S + s], cnt[s]);
        if (cnt[S + s]) atomicAdd(&corner[(size_t)b * S + s], cnt[S + s]);
    }
}

// F.interpolate(size=[h, w], mode='bilinear', align_corners=False, antialias=False) of the magnitude, at patch p of one sample (fs = its channel-0 plane)
__device__ __forceinline__ void bilinear_axis(int dst, int in, int out, int& i0, int& i1, float& l1) {
    const float src = fmaxf(((float)dst + 0.5f) * ((float)in / (float)out) - 0.5f, 0.f);
    i0 = min((int)src, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}

__device__ float patch_tap(const FlowView& fv, const float* __restrict__ fs, int h, int w, int p) {
    const int dy = p / w, dx = p - dy * w;
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_axis(dy, fv.H, h, y0, y1, ly);
    bilinear_axis(dx, fv.W, w, x0, x1, lx);
    auto mag_at = [&](int64_t off) { return flow_mag2(fs[off], fs[off + fv.sc]); };
    const float m00 = mag_at(y0 * fv.sh + x0 * fv.sw), m01 = mag_at(y0 * fv.sh + x1 * fv.sw);
    const float m10 = mag_at(y1 * fv.sh + x0 * fv.sw), m11 = mag_at(y1 * fv.sh + x1 * fv.sw);
    return (1.f - ly) * ((1.f - lx) * m00 + lx * m01) + ly * ((1.f - lx) * m10 + lx * m11);
}

// patch_mag and the decision.  A workgroup owns 64 consecutive samples of one b; V = 4: a lane reads the mask bytes of 4 samples as one 32-bit load (the mask's sample
// axis is contiguous and S % 4 == 0).  Row slot r (0 .. 63) covers patches [r chunk, (r + 1) chunk) in order; the 64 partials of a sample are then added in slot order:
// the same additions whatever V is.
template <int V>
__global__ __launch_bounds__(1024) void flow_filter_finish_kernel(const FlowView fv, const uint8_t* __restrict__ act, int64_t ab, int64_t ap, int64_t as, int h, int w,
                                                                  int methods, float thr, float area_thr, float corner_thr, const int* __restrict__ area,
                                                                  const int* __restrict__ corner, float* __restrict__ patch_mag, uint8_t* __restrict__ reject) {
    __shared__ float part[kFinRows][64];
    __shared__ int npart[kFinRows][64];
    constexpr int LPR = 64 / V;      // lanes per row slot
    constexpr int RPS = 1024 / LPR;  // row slots per sweep
    const int b = blockIdx.y, s0 = blockIdx.x * 64, hw = h * w, chunk = (hw + kFinRows - 1) / kFinRows, S = fv.S;
    const int l = threadIdx.x % LPR, sl = V * l, s = s0 + sl;
    const uint8_t* ab2 = act + b * ab + (int64_t)hw * ap;  // frame 2
    const float* fb = fv.f + b * fv.sb;
    for (int r = threadIdx.x / LPR; r < kFinRows; r += RPS) {
        float acc[V];
        int n[V];
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0.f, n[k] = 0;
        const int p1 = min((r + 1) * chunk, hw);
        if (s < S) {  // V == 4: S % 4 == 0, so s + 3 < S too
            for (int p = r * chunk; p < p1; p += 4) {
                unsigned m[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    m[j] = 0xFFFFFFFFu;
                    if (p + j < p1) {
                        if (V == 4) m[j] = *reinterpret_cast<const unsigned*>(ab2 + (int64_t)(p + j) * ap + s);
                        else m[j] = ab2[(int64_t)(p + j) * ap + (int64_t)s * as];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int k = 0; k < V; ++k)
                        if (((m[j] >> (8 * k)) & 0xFFu) == 0u) {
                            acc[k] += patch_tap(fv, fb + (int64_t)(s + k) * fv.ss, h, w, p + j);
                            ++n[k];
                        }
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            part[r][sl + k] = acc[k];
            npart[r][sl + k] = n[k];
        }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= 64 || s0 + t >= S) return;
    float sum = 0.f;
    int n = 0;
    for (int r = 0; r < kFinRows; ++r) {
        sum += part[r][t];
        n += npart[r][t];
    }
    const size_t i = (size_t)b * S + s0 + t;
    const float pm = sum / ((float)n + 1e-12f);  // sampling.py:203: an empty active set gives 0 / 1e-12
    patch_mag[i] = pm;
    bool rej = false;  // NaN compares false everywhere, as in torch
    if (methods & CWM_FLOW_FILTER_PATCH_MAGNITUDE) rej |= pm < thr;
    if (methods & CWM_FLOW_FILTER_FLOW_AREA) rej |= (float)area[i] / (float)(fv.H * fv.W) > area_thr;
    if (methods & CWM_FLOW_FILTER_NUM_CORNERS) rej |= (float)corner[i] >= corner_thr;
    reject[i] = rej ? 1 : 0;
}

// zero the rejected samples, planes form: a rejected (b, s, c) plane is one contiguous block; workgroups of kept samples leave at once.  VEC as above.
template <int VEC>
__global__ __launch_bounds__(256) void flow_filter_zero_planes_kernel(const FlowView fv, const uint8_t* __restrict__ reject) {
    const int s = blockIdx.y, b = blockIdx.z, HW = fv.H * fv.W;
    if (!reject[(size_t)b * fv.S + s]) return;
    float* u = const_cast<float*>(fv.f) + b * fv.sb + s * fv.ss;  // (cwm_flow_filter_apply's flows are not const)
    const int e0 = blockIdx.x * kFiltPixPerBlock, e1 = min(e0 + kFiltPixPerBlock, HW);
    for (int c = 0; c < 2; ++c, u += fv.sc) {
        if (VEC)
            for (int e = e0 + 4 * (int)threadIdx.x; e < e1; e += 1024) *reinterpret_cast<float4*>(u + e) = make_float4(0.f, 0.f, 0.f, 0.f);
        else
            for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) u[e] = 0.f;
    }
}

// any other layout (the packed one included): a workgroup lists the rejected samples of its b, then writes one zero per (channel, pixel of its tile, rejected
// sample), the rejected samples innermost (neighbours in the packed layout).  Kept samples are neither read nor written.
__global__ __launch_bounds__(256) void flow_filter_zero_scatter_kernel(const FlowView fv, int tile_pix, const uint8_t* __restrict__ reject) {
    extern __shared__ int rej_list[];  // [S]
    __shared__ int n_rej;
    const int b = blockIdx.y, pix0 = blockIdx.x * tile_pix, W = fv.W, HW = fv.H * W, S = fv.S;
    if (threadIdx.x == 0) {  // (in sample order: the writes of neighbouring lanes then go to increasing addresses)
        int n = 0;
        for (int s = 0; s < S; ++s)
            if (reject[(size_t)b * S + s]) rej_list[n++] = s;
        n_rej = n;
    }
    __syncthreads();
    const int nr = n_rej, npix = min(tile_pix, HW - pix0);
    if (nr == 0) return;
    float* fb = const_cast<float*>(fv.f) + b * fv.sb;
    const int64_t total = (int64_t)npix * nr;
    for (int64_t i = threadIdx.x; i < total; i += blockDim.x) {
        const int pl = (int)(i / nr), e = pix0 + pl, y = e / W, x = e - y * W;
        const int64_t off = (int64_t)y * fv.sh + (int64_t)x * fv.sw + (int64_t)rej_list[(int)(i - (int64_t)pl * nr)] * fv.ss;
        fb[off] = 0.f;
        fb[off + fv.sc] = 0.f;
    }
}

// planes -> packed: out[b][n][s] = reject[b][s] ? 0 : in[b][s][n], n over the 2 H W floats of a sample (contiguous), 64 x 64 tiles through LDS
__global__ __launch_bounds__(256) void flow_filter_pack_kernel(const float* __restrict__ f, int64_t sb, int64_t ss, int N, int S, const uint8_t* __restrict__ reject,
                                                               float* __restrict__ out) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z, s0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
    for (int k = row; k < 64; k += 4) {
        const int s = s0 + k, n = n0 + lane;
        float v = 0.f;
        if (s < S && n < N && !reject[(size_t)b * S + s]) v = f[b * sb + s * ss + n];
        tile[k][lane] = v;
    }
    __syncthreads();
    for (int k = row; k < 64; k += 4) {
        const int n = n0 + k, s = s0 + lane;
        if (n < N && s < S) out[((size_t)b * N + n) * S + s] = tile[lane][k];
    }
}

}  // namespace cwm

using namespace cwm;

extern "C" int cwm_flow_filter_stats(const float* flows_dev, const int64_t* strides, int B, int C, int H, int W, int S, const uint8_t* active_dev,
                                     const int64_t* active_strides, int Np, int methods, float flow_magnitude_threshold, float flow_area_threshold,
                                     float num_corners_threshold, float* patch_mag_dev, int32_t* area_count_dev, int32_t* corner_count_dev, uint8_t* reject_dev,
                                     void* stream) {
    FlowView v;
    if (int rc = flow_view("cwm_flow_filter_stats", true, flows_dev, strides, B, C, H, W, S, &v)) return rc;
    CWM_REQUIRE(active_dev && active_strides && patch_mag_dev && area_count_dev && corner_count_dev && reject_dev, "cwm_flow_filter_stats: null pointer");
    CWM_REQUIRE(Np >= 2 && Np % 2 == 0, "cwm_flow_filter_stats: Np=%d must be the (even) patch count of two frames", Np);
    const int h = (int)std::sqrt((double)(Np / 2));  // sampling.py:188: h = w = int((Np / 2) ** 0.5)
    CWM_REQUIRE(2 * h * h == Np, "cwm_flow_filter_stats: Np=%d is not 2 h w for a square patch grid", Np);
    CWM_REQUIRE((methods & ~(CWM_FLOW_FILTER_PATCH_MAGNITUDE | CWM_FLOW_FILTER_FLOW_AREA | CWM_FLOW_FILTER_NUM_CORNERS)) == 0,
                "cwm_flow_filter_stats: unknown bits in methods=0x%x", methods);
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    CWM_HIP_CHECK(hipMemsetAsync(area_count_dev, 0, (size_t)B * S * sizeof(int32_t), st));
    CWM_HIP_CHECK(hipMemsetAsync(corner_count_dev, 0, (size_t)B * S * sizeof(int32_t), st));
    const FlowForm count = flow_count_form(v, flow_layout(v, 0));
    if (count == COUNT_PACKED || count == COUNT_PACKED_VEC) {
        const int tile = mag_tile_pix(S);
        const dim3 grid((unsigned)((HW + tile - 1) / tile), (unsigned)B);
        dispatch_int<0, 1>(count == COUNT_PACKED_VEC, [&](auto vec) {
            hipLaunchKernelGGL(flow_filter_count_packed_kernel<vec.value>, grid, dim3(256), (size_t)2 * S * sizeof(int), st, v.f, v.sb, v.sc, HW, W, S, tile,
                               flow_magnitude_threshold, area_count_dev, corner_count_dev);
        });
    } else {
        const dim3 grid((unsigned)((HW + kFiltPixPerBlock - 1) / kFiltPixPerBlock), (unsigned)S, (unsigned)B);
        dispatch_int<0, 1>(count == COUNT_PLANES_VEC, [&](auto vec) {
            hipLaunchKernelGGL(flow_filter_count_kernel<vec.value>, grid, dim3(256), 0, st, v.f, v.sb, v.sc, v.sh, v.sw, v.ss, H, W, S, flow_magnitude_threshold,
                               area_count_dev, corner_count_dev);
        });
    }
    CWM_HIP_CHECK(hipGetLastError());
    dispatch_int<1, 4>(flow_finish_form(S, active_strides, (uintptr_t)active_dev, h * h) == FINISH_V4 ? 4 : 1, [&](auto V) {
        hipLaunchKernelGGL(flow_filter_finish_kernel<V.value>, dim3((unsigned)((S + 63) / 64), (unsigned)B), dim3(1024), 0, st, v, active_dev, active_strides[0], active_strides[1],
                           active_strides[2], h, h, methods, flow_magnitude_threshold, flow_area_threshold, num_corners_threshold, area_count_dev, corner_count_dev, patch_mag_dev,
                           reject_dev);
    });
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int cwm_flow_filter_apply(float* flows_dev, const int64_t* strides, int B, int C, int H, int W, int S, const uint8_t* reject_dev, void* stream) {
    FlowView v;
    if (int rc = flow_view("cwm_flow_filter_apply", true, flows_dev, strides, B, C, H, W, S, &v)) return rc;
    CWM_REQUIRE(reject_dev, "cwm_flow_filter_apply: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, tile = 256;
    const FlowForm zero = flow_zero_form(v, flow_layout(v, 0));
    CWM_REQUIRE(zero != FLOW_REFUSED, "cwm_flow_filter_apply: S=%d > 8192 in a layout whose (H, W) planes are not contiguous", S);
    const dim3 grid((unsigned)((HW + kFiltPixPerBlock - 1) / kFiltPixPerBlock), (unsigned)S, (unsigned)B);  // (planes)
    if (zero == ZERO_SCATTER)
        hipLaunchKernelGGL(flow_filter_zero_scatter_kernel, dim3((unsigned)((HW + tile - 1) / tile), (unsigned)B), dim3(256), (size_t)S * sizeof(int), st, v, tile, reject_dev);
    else
        dispatch_int<0, 1>(zero == ZERO_PLANES_VEC, [&](auto vec) { hipLaunchKernelGGL(flow_filter_zero_planes_kernel<vec.value>, grid, dim3(256), 0, st, v, reject_dev); });
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int cwm_flow_filter_pack(const float* flows_dev, const int64_t* strides, int B, int C, int H, int W, int S, const uint8_t* reject_dev, float* out_dev,
                                    void* stream) {
    FlowView v;
    if (int rc = flow_view("cwm_flow_filter_pack", true, flows_dev, strides, B, C, H, W, S, &v)) return rc;
    CWM_REQUIRE(reject_dev && out_dev, "cwm_flow_filter_pack: null pointer");
    CWM_REQUIRE(flow_pack_form(flow_layout(v, 0)) != FLOW_REFUSED,
                "cwm_flow_filter_pack: every sample must be one contiguous [2,H,W] block (the sample-outermost view of the flow model's output)");
    hipLaunchKernelGGL(flow_filter_pack_kernel, dim3((unsigned)((2 * H * W + 63) / 64), (unsigned)((S + 63) / 64), (unsigned)B), dim3(256), 0, (hipStream_t)stream, v.f, v.sb,
                       v.ss, 2 * H * W, S, reject_dev, out_dev);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}
