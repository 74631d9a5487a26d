// Token read-outs: small per-patch answers straight from predicted tokens, without the predicted video -- the patch-error map (cwm_patch_error), the response
// of a perturbation (cwm_token_response) and the error-guided reveal step on top of the map (cwm_unmask_step; its selection kernel: unmask.hip).  None takes a
// model handle.  What they share is stated once here: the geometry and its check (PatchGrid, kernels.h), the y row of every patch of a patch row, the
// per-item partials in LDS and their fixed-order fold.
#include "common.h"
#include "kernels.h"
#include "../../include/cwm_hip.h"
#include <cstring>

namespace cwm {

PatchGrid patch_grid_of(const cwm_patch_error_args& a) {
    PatchGrid g = {a.batch, a.T, a.C, a.H, a.W, a.P, a.n_vis, 0, a.frame};
    if (g.P > 0 && g.T > 0 && g.H > 0 && g.W > 0) g.Nm = g.T * (g.H / g.P) * (g.W / g.P) - g.n_vis;  // (check_patch_grid checks the sizes themselves)
    return g;
}

int check_patch_grid(const char* who, const PatchGrid& g, unsigned needs) {
    CWM_REQUIRE(g.B > 0 && g.T > 0, "%sbatch = %d and T = %d must be positive", who, g.B, g.T);
    CWM_REQUIRE(g.P == 4 || g.P == 8 || g.P == 16, "%sP = %d, patches of 4, 8 or 16 pixels", who, g.P);
    CWM_REQUIRE(g.H > 0 && g.H % g.P == 0, "%sH = %d is no positive multiple of P = %d", who, g.H, g.P);
    CWM_REQUIRE(g.W > 0 && g.W % g.P == 0, "%sW = %d is no positive multiple of P = %d", who, g.W, g.P);
    if (needs & kGridChannels) CWM_REQUIRE(g.C >= 1 && g.C <= 8, "%sC = %d, 1 .. 8", who, g.C);
    if (needs & kGridTokens) {
        const int64_t Nt = (int64_t)g.T * (g.H / g.P) * (g.W / g.P);
        CWM_REQUIRE(g.n_vis >= 0 && g.n_vis <= Nt && g.Nm == Nt - g.n_vis, "%sn_vis = %d, Nm = %d of %lld tokens", who, g.n_vis, g.Nm, (long long)Nt);
    }
    if (needs & (kGridFrame | kGridFrameEach)) {
        const bool each = needs & kGridFrameEach;
        CWM_REQUIRE(g.frame >= (each ? -1 : 0) && g.frame < g.T, "%sframe = %d of %d (%s)", who, g.frame, g.T, each ? "-1: each" : "one frame, 0 .. T-1");
    }
    return 0;
}

namespace {

// ---------------------------------------------------------------------------------------------
// One workgroup of 256 lanes reads one patch row i of one frame: P image rows of W pixels.  An item is 4 horizontally adjacent pixels of one image row, ALL
// channels: consecutive lanes read consecutive 16 bytes of an image row and consecutive 16 C bytes of a token of y.  The front of the dynamic LDS is
// part [P][W / 4] (one partial sum per item) | yrow [gw] (y row of patch j, -1 = visible) | cnt [4] (per wave); a kernel's own tail follows.
// ---------------------------------------------------------------------------------------------
struct PatchRowLds {
    float* part;
    int *yrow, *cnt;
    float* tail;
};
__device__ __forceinline__ PatchRowLds patch_row_lds(float* lds, int items, int gw) {
    int* yrow = reinterpret_cast<int*>(lds + items);
    return {lds, yrow, yrow + gw, reinterpret_cast<float*>(yrow + gw + 4)};
}
size_t patch_row_lds_bytes(const PatchGrid& g) { return ((size_t)g.P * (g.W / 4) + g.W / g.P + 4) * sizeof(float); }

// The y row of a masked token is its rank among the row's masked tokens: the mask bytes in front of the patch row (tau0 of them) are counted here -- an integer
// sum, any order -- and each of the gw patches adds those in front of it.  Whatever the mask holds, the row read lies in [0, Nm); with Nm = 0 there is no y
// and every patch counts as visible.  Ends with a barrier: yrow is complete.
__device__ __forceinline__ void patch_row_yrows(const uint8_t* mrow, int tau0, int gw, int Nm, const PatchRowLds& l) {
    int c0 = 0;
    for (int k = threadIdx.x; k < tau0; k += 256) c0 += mrow[k] != 0;
#pragma unroll
    for (int o = 32; o; o >>= 1) c0 += __shfl_down(c0, o, 64);
    if ((threadIdx.x & 63) == 0) l.cnt[threadIdx.x >> 6] = c0;
    __syncthreads();
    if ((int)threadIdx.x < gw) {
        int rk = l.cnt[0] + l.cnt[1] + l.cnt[2] + l.cnt[3];
        for (int k = 0; k < (int)threadIdx.x; ++k) rk += mrow[tau0 + k] != 0;
        l.yrow[threadIdx.x] = (mrow[tau0 + threadIdx.x] != 0 && Nm > 0) ? min(rk, Nm - 1) : -1;
    }
    __syncthreads();
}

// the mean over patch j of the items' partials, summed from LDS in (ph, k) order by one lane
__device__ __forceinline__ float patch_row_value(const float* part, int w4, int P, int j) {
    const int q = P / 4;
    float s = 0.f;
    for (int ph = 0; ph < P; ++ph)
        for (int k = 0; k < q; ++k) s += part[ph * w4 + j * q + k];
    return s / (float)(P * P);
}

template <bool A16>
__device__ __forceinline__ float4 pe_load4(const float* p) {
    if (A16) return *reinterpret_cast<const float4*>(p);
    const Float4A4 v = *reinterpret_cast<const Float4A4*>(p);
    return make_float4(v.v[0], v.v[1], v.v[2], v.v[3]);
}

__device__ __forceinline__ float pe_sq4(float s, const float4& a, const float4& b) {
    const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
    s += d0 * d0;
    s += d1 * d1;
    s += d2 * d2;
    s += d3 * d3;
    return s;
}

bool off16(const void* q) { return ((uintptr_t)q & 15) != 0; }

// ---------------------------------------------------------------------------------------------
// Per-patch prediction error straight from the predicted tokens: `get_error_on_target_region` (prediction.py:553-574) = `_get_error` (:324-329; MSELoss
// summed over the channels) of `pred_patches_to_video` (:245-259) against the target frames, avg_pool3d over each patch, times the region, averaged --
// without the predicted video.  map[b][t][i][j] = (1 / P^2) sum over the pixels of patch (i, j) and the channels of (pred_f - target_t)^2, where pred_f is
// frame f = `frame` (or t: frame < 0) of that video: y at the masked patches of frame f, x at its visible ones.
//
// One workgroup per (b, t, patch row i).  Every float sum has a fixed order: an item's 4 C squares in sequence, the items of a patch as patch_row_value.
// FAST: C == 3 and every pointer and stride on the 16-byte grid (three aligned 16-byte loads of a token's 12 floats, transposed in registers as unembed3_kernel does)
// ---------------------------------------------------------------------------------------------
template <bool FAST>
__global__ __launch_bounds__(256) void patch_error_map_kernel(const PatchErrorParams p, float* map) {
    extern __shared__ __align__(16) float pe_lds[];
    const PatchGrid& g = p.g;
    const int gw = g.W / g.P, gh = g.H / g.P, n = gh * gw, Nt = g.T * n;
    const int w4 = g.W / 4, items = g.P * w4;
    const PatchRowLds l = patch_row_lds(pe_lds, items, gw);
    int r = blockIdx.x;
    const int i = r % gh; r /= gh;
    const int t = r % g.T;
    const int b = r / g.T;
    const int f = g.frame < 0 ? t : g.frame;
    patch_row_yrows(p.mask + (size_t)b * Nt, f * n + i * gw, gw, g.Nm, l);
    const float* xb = p.x + b * p.sb + f * p.st;
    const float* tg = p.target ? p.target + b * p.tb + t * p.tt : p.x + b * p.sb + t * p.st;
    const int64_t tc = p.target ? p.tc : p.sc;
    const bool same = xb == tg && tc == p.sc;  // the target IS the frame the visible patches come from: their error is exactly 0, nothing to read
    const int PPC = g.P * g.P * g.C;
    for (int it = threadIdx.x; it < items; it += 256) {
        const int ph = it / w4, x0 = (it - ph * w4) * 4;
        const int jr = l.yrow[x0 / g.P];
        const int64_t off = (int64_t)(i * g.P + ph) * g.W + x0;
        float s = 0.f;
        if (jr >= 0) {
            const float* yp = p.y + ((size_t)b * g.Nm + jr) * PPC + (ph * g.P + (x0 % g.P)) * g.C;
            if (FAST) {
                const float4* y4 = reinterpret_cast<const float4*>(yp);
                const float4 a = y4[0], bb = y4[1], c = y4[2];  // px0 (r g b) px1 (r | g b) px2 (r g | b) px3 (r g b)
                s = pe_sq4(s, make_float4(a.x, a.w, bb.z, c.y), pe_load4<true>(tg + off));
                s = pe_sq4(s, make_float4(a.y, bb.x, bb.w, c.z), pe_load4<true>(tg + off + tc));
                s = pe_sq4(s, make_float4(a.z, bb.y, c.x, c.w), pe_load4<true>(tg + off + 2 * tc));
            } else {
                for (int c = 0; c < g.C; ++c)
                    s = pe_sq4(s, make_float4(yp[c], yp[g.C + c], yp[2 * g.C + c], yp[3 * g.C + c]), pe_load4<false>(tg + off + c * tc));
            }
        } else if (!same) {
            for (int c = 0; c < g.C; ++c) s = pe_sq4(s, pe_load4<FAST>(xb + off + c * p.sc), pe_load4<FAST>(tg + off + c * tc));
        }
        l.part[it] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < gw) map[(((size_t)b * g.T + t) * gh + i) * gw + threadIdx.x] = patch_row_value(l.part, w4, g.P, threadIdx.x);
}

// mean[b] = sum(map * region) / max(sum(region), 1) (prediction.py:570-573): one workgroup per batch row, lane k sums elements k, k + 256, ... in order, then
// a halving tree over LDS -- the same order on every call
__global__ __launch_bounds__(256) void patch_error_mean_kernel(const float* map, const float* region, int n_el, float* mean) {
    __shared__ float num[256], den[256];
    const int b = blockIdx.x;
    float sn = 0.f, sd = 0.f;
    for (int k = threadIdx.x; k < n_el; k += 256) {
        const float rg = region ? region[(size_t)b * n_el + k] : 1.f;
        sn += map[(size_t)b * n_el + k] * rg;
        sd += rg;
    }
    num[threadIdx.x] = sn;
    den[threadIdx.x] = sd;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if ((int)threadIdx.x < o) {
            num[threadIdx.x] += num[threadIdx.x + o];
            den[threadIdx.x] += den[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) mean[b] = num[0] / fmaxf(den[0], 1.f);
}

// ---------------------------------------------------------------------------------------------
// Response of a perturbation straight from two sets of predicted tokens (cwm_token_response): r[b][Y][X] = sum_c (y - y_ref)^2 over frame `frame`, 0 where
// the frame's patch is visible (both predictions copy the same input pixel there); the per-patch mean of r, its first maximum (torch.argmax: a NaN is the
// maximum, the first NaN wins), its sum and its centroid -- neither predicted video is built, and one location per row is all that leaves the device.
//
// One workgroup per (b, patch row i).  Every float sum has a fixed order: a pixel's C squares in channel order from 0.f; a lane's pixels in ascending pixel
// index; the 256 lanes by a halving tree over LDS; the H / P workgroups of a row in index order by one lane of token_response_fold_kernel.  The maximum is
// taken with its index (lower index among equal values), so the order it is folded in does not matter.
// ---------------------------------------------------------------------------------------------
// does candidate a = (value, pixel index) come before b as torch.argmax sees them?
__device__ __forceinline__ bool tr_better(float va, int ia, float vb, int ib) {
    const bool an = va != va, bn = vb != vb;
    if (an || bn) return an && (!bn || ia < ib);
    return va > vb || (va == vb && ia < ib);
}

constexpr int kTokenResponsePartial = 8;  // floats per workgroup partial: peak, its pixel index (int bits), mass, sum r Y, sum r X, 3 unused

// FAST: C == 3 and every pointer and the reference's row stride on the 16-byte grid
template <bool FAST>
__global__ __launch_bounds__(256) void token_response_kernel(const TokenResponseParams p) {
    extern __shared__ __align__(16) float tr_lds[];  // (all of the kernel's LDS: nothing static in front of the dynamic region)
    const PatchGrid& g = p.g;
    const int gw = g.W / g.P, gh = g.H / g.P, n = gh * gw, Nt = g.T * n;
    const int w4 = g.W / 4, items = g.P * w4;
    const PatchRowLds l = patch_row_lds(tr_lds, items, gw);
    float* red_v = l.tail;                                 // [256] each: the lanes' partials (peak, its index, mass, sum r Y, sum r X)
    int* red_i = reinterpret_cast<int*>(red_v + 256);
    float *red_m = red_v + 512, *red_y = red_v + 768, *red_x = red_v + 1024;
    const int i = blockIdx.x % gh, b = blockIdx.x / gh;
    patch_row_yrows(p.mask + (size_t)b * Nt, g.frame * n + i * gw, gw, g.Nm, l);  // (Nm = 0: no tokens, the response is 0 everywhere)
    const int PPC = g.P * g.P * g.C;
    const bool reduce = p.scratch != nullptr;
    float bv = -1.f, sm = 0.f, sy = 0.f, sx = 0.f;  // (-1, INT_MAX): behind every pixel, whose response is >= 0 or NaN
    int bi = 0x7fffffff;
    for (int it = threadIdx.x; it < items; it += 256) {
        const int ph = it / w4, x0 = (it - ph * w4) * 4;
        const int jr = l.yrow[x0 / g.P];
        const int Y = i * g.P + ph;
        float r[4] = {0.f, 0.f, 0.f, 0.f};
        float s = 0.f;
        if (jr >= 0) {
            const size_t tok = (size_t)jr * PPC + (ph * g.P + (x0 % g.P)) * g.C;
            const float* yp = p.y + (size_t)b * g.Nm * PPC + tok;
            const float* rp = p.y_ref + (int64_t)b * p.ref_sb + tok;
            if (FAST) {
                const float4* y4 = reinterpret_cast<const float4*>(yp);
                const float4* r4 = reinterpret_cast<const float4*>(rp);
                const float4 a = y4[0], bb = y4[1], c = y4[2];  // px0 (r g b) px1 (r | g b) px2 (r g | b) px3 (r g b)
                const float4 ra = r4[0], rb = r4[1], rc = r4[2];
                const float d[4][3] = {{a.x - ra.x, a.y - ra.y, a.z - ra.z}, {a.w - ra.w, bb.x - rb.x, bb.y - rb.y},
                                       {bb.z - rb.z, bb.w - rb.w, c.x - rc.x}, {c.y - rc.y, c.z - rc.z, c.w - rc.w}};
#pragma unroll
                for (int px = 0; px < 4; ++px)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) r[px] += d[px][ch] * d[px][ch];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                    for (int px = 0; px < 4; ++px) s += d[px][ch] * d[px][ch];
            } else {
#pragma unroll
                for (int px = 0; px < 4; ++px)
                    for (int ch = 0; ch < g.C; ++ch) {
                        const float dd = yp[px * g.C + ch] - rp[px * g.C + ch];
                        r[px] += dd * dd;
                    }
                for (int ch = 0; ch < g.C; ++ch)
                    s = pe_sq4(s, make_float4(yp[ch], yp[g.C + ch], yp[2 * g.C + ch], yp[3 * g.C + ch]),
                               make_float4(rp[ch], rp[g.C + ch], rp[2 * g.C + ch], rp[3 * g.C + ch]));
            }
        }
        l.part[it] = s;
        if (p.pixel_map) {
            float* dst = p.pixel_map + ((size_t)b * g.H + Y) * g.W + x0;
            if (FAST) {
                *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
            } else {
#pragma unroll
                for (int px = 0; px < 4; ++px) dst[px] = r[px];
            }
        }
        if (reduce) {
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                const int idx = Y * g.W + x0 + px;
                if (tr_better(r[px], idx, bv, bi)) { bv = r[px]; bi = idx; }
                sm += r[px];
                sy += r[px] * (float)Y;
                sx += r[px] * (float)(x0 + px);
            }
        }
    }
    __syncthreads();
    if (p.map && (int)threadIdx.x < gw) p.map[((size_t)b * gh + i) * gw + threadIdx.x] = patch_row_value(l.part, w4, g.P, threadIdx.x);
    if (!reduce) return;  // (uniform: a kernel argument)
    red_v[threadIdx.x] = bv; red_i[threadIdx.x] = bi;
    red_m[threadIdx.x] = sm; red_y[threadIdx.x] = sy; red_x[threadIdx.x] = sx;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const int u = threadIdx.x, v = threadIdx.x + o;
            if (tr_better(red_v[v], red_i[v], red_v[u], red_i[u])) { red_v[u] = red_v[v]; red_i[u] = red_i[v]; }
            red_m[u] += red_m[v];
            red_y[u] += red_y[v];
            red_x[u] += red_x[v];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float* out = p.scratch + ((size_t)b * gh + i) * kTokenResponsePartial;
        out[0] = red_v[0];
        out[1] = __int_as_float(red_i[0]);
        out[2] = red_m[0];
        out[3] = red_y[0];
        out[4] = red_x[0];
    }
}

// one lane per row: the row's H / P partials in index order
__global__ __launch_bounds__(64) void token_response_fold_kernel(const float* partials, int B, int gh, int W, int* peak_index, float* stats) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float* in = partials + (size_t)b * gh * kTokenResponsePartial;
    float bv = -1.f, sm = 0.f, sy = 0.f, sx = 0.f;
    int bi = 0x7fffffff;
    for (int i = 0; i < gh; ++i, in += kTokenResponsePartial) {
        const float v = in[0];
        const int idx = __float_as_int(in[1]);
        if (tr_better(v, idx, bv, bi)) { bv = v; bi = idx; }
        sm += in[2];
        sy += in[3];
        sx += in[4];
    }
    if (peak_index) peak_index[b] = bi;
    if (stats) {
        const bool empty = sm == 0.f;  // nothing to weigh the positions with: the peak's own
        stats[b * 4 + 0] = bv;
        stats[b * 4 + 1] = sm;
        stats[b * 4 + 2] = empty ? (float)(bi / W) : sy / sm;
        stats[b * 4 + 3] = empty ? (float)(bi % W) : sx / sm;
    }
}

PatchErrorParams patch_error_params(const cwm_patch_error_args& a) {
    PatchErrorParams p;
    memset(&p, 0, sizeof(p));
    p.y = a.y_tokens_dev;
    p.x = a.x_dev; p.sb = a.x_stride_b; p.st = a.x_stride_t; p.sc = a.x_stride_c;
    p.target = a.target_dev; p.tb = a.target_stride_b; p.tt = a.target_stride_t; p.tc = a.target_stride_c;
    p.mask = a.mask_dev; p.region = a.region_dev;
    p.g = patch_grid_of(a);
    p.map = a.map_dev; p.mean = a.mean_dev; p.scratch = a.scratch_dev;
    return p;
}

}  // namespace

int launch_patch_error(const PatchErrorParams& p, hipStream_t stream) {
    const PatchGrid& g = p.g;
    CWM_REQUIRE(p.x && p.mask, "patch_error: x_dev and mask_dev are required");
    if (int rc = check_patch_grid("patch_error: ", g, kGridChannels | kGridTokens | kGridFrameEach)) return rc;
    CWM_REQUIRE(p.y || g.Nm == 0, "patch_error: the predicted tokens are required when a token is masked");
    CWM_REQUIRE(p.sb >= 0 && p.st >= 0 && p.sc >= (int64_t)g.H * g.W && (!p.target || (p.tb >= 0 && p.tt >= 0 && p.tc >= (int64_t)g.H * g.W)),
                "patch_error: channel planes of %d x %d pixels need a stride of at least that, batch and frame strides >= 0", g.H, g.W);
    CWM_REQUIRE(p.map || p.mean, "patch_error: neither output requested");
    float* map = p.map ? p.map : p.scratch;
    CWM_REQUIRE(map, "patch_error: the mean alone needs scratch for the map ([B][T][H / P][W / P] floats)");
    const int gh = g.H / g.P, gw = g.W / g.P;
    const size_t lds = patch_row_lds_bytes(g);
    CWM_REQUIRE(gw <= 256 && lds <= 48 * 1024 && (int64_t)g.B * g.T * gh < (1ll << 31), "patch_error: image or batch too large (%d patches per row, %d rows)", gw, g.B * g.T * gh);
    const dim3 grid((unsigned)(g.B * g.T * gh));
    const bool fast = g.C == 3 && !off16(p.y) && !off16(p.x) && !off16(p.target) && p.sb % 4 == 0 && p.st % 4 == 0 && p.sc % 4 == 0 &&
                      (!p.target || (p.tb % 4 == 0 && p.tt % 4 == 0 && p.tc % 4 == 0));
    if (fast)
        hipLaunchKernelGGL(patch_error_map_kernel<true>, grid, dim3(256), lds, stream, p, map);
    else
        hipLaunchKernelGGL(patch_error_map_kernel<false>, grid, dim3(256), lds, stream, p, map);
    CWM_HIP_CHECK(hipGetLastError());
    if (p.mean) {
        hipLaunchKernelGGL(patch_error_mean_kernel, dim3((unsigned)g.B), dim3(256), 0, stream, map, p.region, g.T * gh * gw, p.mean);
        CWM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

int launch_token_response(const TokenResponseParams& p, hipStream_t stream) {
    const PatchGrid& g = p.g;
    CWM_REQUIRE(p.mask, "token_response: mask_dev is required");
    if (int rc = check_patch_grid("token_response: ", g, kGridChannels | kGridTokens | kGridFrame)) return rc;
    CWM_REQUIRE((p.y && p.y_ref) || g.Nm == 0, "token_response: y_tokens_dev and y_ref_dev are required when a token is masked");
    CWM_REQUIRE(p.ref_sb >= 0, "token_response: y_ref_stride_b = %lld must not be negative", (long long)p.ref_sb);
    CWM_REQUIRE(p.map || p.pixel_map || p.peak_index || p.stats, "token_response: no output requested");
    const bool reduce = p.peak_index || p.stats;
    CWM_REQUIRE(!reduce || p.scratch, "token_response: peak_index_dev and stats_dev need scratch for the per-workgroup partials ([B][H / P][8] floats)");
    const int gh = g.H / g.P, gw = g.W / g.P;
    const size_t lds = patch_row_lds_bytes(g) + 5 * 256 * sizeof(float);  // (the tail: the five [256] reduction arrays)
    CWM_REQUIRE(gw <= 256 && lds <= 48 * 1024 && (int64_t)g.B * gh < (1ll << 31) && (int64_t)g.H * g.W < (1ll << 31),
                "token_response: image or batch too large (%d patches per row, %lld workgroups)", gw, (long long)g.B * gh);
    TokenResponseParams q = p;
    if (!reduce) q.scratch = nullptr;  // (the kernel reduces when it has somewhere to put the partials)
    const bool fast = g.C == 3 && !off16(p.y) && !off16(p.y_ref) && !off16(p.pixel_map) && p.ref_sb % 4 == 0;
    const dim3 grid((unsigned)(g.B * gh));
    if (fast)
        hipLaunchKernelGGL(token_response_kernel<true>, grid, dim3(256), lds, stream, q);
    else
        hipLaunchKernelGGL(token_response_kernel<false>, grid, dim3(256), lds, stream, q);
    CWM_HIP_CHECK(hipGetLastError());
    if (reduce) {
        hipLaunchKernelGGL(token_response_fold_kernel, dim3((unsigned)((g.B + 63) / 64)), dim3(64), 0, stream, (const float*)q.scratch, g.B, gh, g.W, p.peak_index, p.stats);
        CWM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace cwm

using namespace cwm;

extern "C" int cwm_patch_error(const cwm_patch_error_args* a) {
    CWM_REQUIRE(a && a->struct_size == sizeof(cwm_patch_error_args), "cwm_patch_error: args->struct_size must be sizeof(cwm_patch_error_args)");
    return launch_patch_error(patch_error_params(*a), (hipStream_t)a->stream);
}

extern "C" int cwm_unmask_step(const cwm_unmask_step_args* a) {
    CWM_REQUIRE(a && a->struct_size == sizeof(cwm_unmask_step_args), "cwm_unmask_step: args->struct_size must be sizeof(cwm_unmask_step_args)");
    const cwm_patch_error_args& g = a->base;
    CWM_REQUIRE(g.mask_dev, "cwm_unmask_step: base.mask_dev is required");
    PatchErrorParams p = patch_error_params(g);
    if (int rc = check_patch_grid("cwm_unmask_step: base.", p.g, 0)) return rc;  // (what the selection reads; with a reveal the error map's launcher checks the rest)
    CWM_REQUIRE(a->mode == 0 || a->mode == 1, "cwm_unmask_step: mode = %d (0 top, 1 race)", a->mode);
    UnmaskStepParams u;
    memset(&u, 0, sizeof(u));
    u.mask = g.mask_dev;
    u.B = g.batch; u.T = g.T; u.gh = g.H / g.P; u.gw = g.W / g.P; u.frame = a->frame;
    u.k = a->num_reveal; u.race = a->mode; u.self_mask = a->self_mask != 0;
    u.threshold = a->threshold_dev; u.e = a->e_dev;
    u.mask_out = a->mask_out_dev; u.picks = a->picks_dev; u.dist = a->dist_dev; u.frontier = a->frontier_dev;
    if (u.k <= 0) {  // nothing to reveal: the distance and the frontier alone
        u.mask_out = nullptr;
        u.picks = nullptr;
        return launch_unmask_select(u, (hipStream_t)g.stream);
    }
    // Everything that can refuse is checked before the first launch: the selection's own arguments here (with a stand-in for the map), the error map's by its launcher.
    CWM_REQUIRE(g.x_dev, "cwm_unmask_step: x_dev is required when a cell is revealed");
    CWM_REQUIRE(g.map_dev || g.scratch_dev, "cwm_unmask_step: base.map_dev or base.scratch_dev ([B, T, H/P, W/P] floats) is required: the selection reads the error map from it");
    if (!p.map && !p.mean) p.map = p.scratch;
    u.map = p.map ? p.map : p.scratch;
    u.region = g.region_dev;
    int rc;
    if ((rc = check_unmask_select(u))) return rc;
    if ((rc = launch_patch_error(p, (hipStream_t)g.stream))) return rc;
    return launch_unmask_select(u, (hipStream_t)g.stream);
}

extern "C" int cwm_token_response(const cwm_token_response_args* a) {
    CWM_REQUIRE(a && a->struct_size == sizeof(cwm_token_response_args), "cwm_token_response: args->struct_size must be sizeof(cwm_token_response_args)");
    const cwm_patch_error_args& g = a->base;
    TokenResponseParams p;
    memset(&p, 0, sizeof(p));
    p.y = g.y_tokens_dev; p.y_ref = a->y_ref_dev; p.ref_sb = a->y_ref_stride_b;
    p.mask = g.mask_dev;
    p.g = patch_grid_of(g);
    p.map = g.map_dev; p.pixel_map = a->pixel_map_dev; p.peak_index = a->peak_index_dev; p.stats = a->stats_dev; p.scratch = g.scratch_dev;
    return launch_token_response(p, (hipStream_t)g.stream);
}
