// RAFT-large optical flow (cwm/models/raft): the kernels around the convolution GEMMs.  Activations are fp32 NHWC; a convolution is an
// explicit im2col into the GEMM's A operand (common.h a_pos: split-bf16 hi/lo in parity mode, one bf16 plane in fast mode; K order
// (ky, kx, c), zero padded to Kpad) and one launch_gemm with the EPI_F32 epilogue.  Activation functions, normalisations and the GRU's r*h are applied where an operand is read, never as a pass of
// their own, except the residual join of the encoders and the GRU state update.  Below the kernels: launch_flat, the one launch of every grid-stride kernel
// here; the three statements a convolution launch is made of (set_conv_geometry, pack_conv_parts, conv_gemm), shared by raft_model.hip and dev.hip; and the
// launchers.  One convex-upsampling kernel serves the flow (2 channels, read from the coordinates) and the output head's map (1 channel, planar).
// The correlation lookup has two kernels behind one contract: corr_lookup_kernel samples the all-pairs pyramid, corr_lookup_on_the_fly_kernel computes the
// correlation of every tap it needs from the feature maps (no pyramid); both take taps and weights from lookup_tap.
#include <math.h>

#include <algorithm>

#include "kernels.h"

namespace cwm {

namespace {

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// value of channel c of one source at pixel `pix` (of image `img`, spatial position (y, x))
__device__ __forceinline__ float src_value(const ConvSrc& s, int64_t pix, int img, int y, int x, int c) {
    if (s.coords) return s.coords[pix * 2 + c] - (float)(c ? y : x);  // flow = coords1 - coords0
    float v = s.p[pix * s.ld + c];
    if (s.stats) {
        const float2 st = reinterpret_cast<const float2*>(s.stats)[(int64_t)img * s.C + c];
        v = (v - st.x) * st.y;
    }
    if (s.relu) v = fmaxf(v, 0.f);
    if (s.gate) v = v * sigmoidf_(s.gate[pix * s.gate_ld + c]);
    return v;
}

// One thread per 8 consecutive k of one row: they lie in one [32 hi | 32 lo] block of the parity layout, so the thread ends with one
// 16-byte store per plane.  (K order (ky, kx, c): the 8 channels of a thread come from at most two taps.)  PLANES == 1 (fast mode): the
// same values rounded once to bf16 into the row-major one-plane layout, one 16-byte store per thread, consecutive threads consecutive.
template <int PLANES>
__global__ void im2col_kernel(const Im2colParams p) {
    const int Ctot = p.src[0].C + (p.nsrc > 1 ? p.src[1].C : 0);
    const int K = p.kh * p.kw * Ctot;
    const int kg = p.Kpad >> 3, ohw = p.OH * p.OW;
    const int total = p.n_img * ohw * kg;
    const bool partial = p.c_hi > p.c_lo;
    for (int gi = blockIdx.x * blockDim.x + threadIdx.x; gi < total; gi += gridDim.x * blockDim.x) {
        const int m = gi / kg, kb = (gi - m * kg) << 3;
        if (partial && kb >= K) continue;
        int tap = kb / Ctot, c = kb - tap * Ctot;
        if (partial && (c < p.c_lo || c >= p.c_hi)) continue;  // channel ranges are multiples of 8: a group is wholly in or out
        const int img = m / ohw, r = m - img * ohw;
        const int oy = r / p.OW, ox = r - oy * p.OW;
        bf16x8 hv, lv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = 0.f;
            if (kb + j < K) {
                const int ky = tap / p.kw, kx = tap - ky * p.kw;
                const int y = oy * p.stride - p.pad_h + ky, x = ox * p.stride - p.pad_w + kx;
                if (y >= 0 && y < p.H && x >= 0 && x < p.W) {
                    if (p.image.base[0]) {  // the input frames: NCHW (any batch / time / channel strides), scaled 2 * (x * scale / 255) - 1
                        const ImageSrc& I = p.image;
                        const int ii = p.img0 + img;
                        const int which = ii / I.P, pr = ii - which * I.P;
                        const int g = pr / I.ppg, t = pr - g * I.ppg;
                        const float xv = I.base[which][g * I.sb[which] + t * I.st[which] + c * I.sc[which] + (int64_t)y * p.W + x];
                        float sv = xv * I.scale;
                        sv = sv / 255.f;
                        v = 2.f * sv - 1.f;
                    } else {
                        const int64_t pix = ((int64_t)img * p.H + y) * p.W + x;
                        v = c < p.src[0].C ? src_value(p.src[0], pix, img, y, x, c) : src_value(p.src[1], pix, img, y, x, c - p.src[0].C);
                    }
                }
            }
            split_bf16_at<PLANES>(v, hv, lv, j);
            if (++c == Ctot) {
                c = 0;
                ++tap;
            }
        }
        store_operand_split<PLANES>(p.A, m, p.Kpad, kb, hv, lv);
    }
}

// InstanceNorm2d statistics (no affine, biased variance) per image and channel over H*W: partial sums of x and x^2 in double over
// pixel chunks (grid: image x 64-channel group x chunk), then one thread per (image, channel) adds the chunks in order (deterministic)
__global__ void __launch_bounds__(512) instnorm_partial_kernel(const float* x, int HW, int C, int chunk, double2* part) {
    __shared__ double2 red[8][64];
    const int img = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6, ch = blockIdx.z;
    const float* base = x + (int64_t)img * HW * C;
    const int p0 = ch * chunk, p1 = min(HW, p0 + chunk);
    double s = 0.0, q = 0.0;
    if (c < C)
        for (int pp = p0 + g; pp < p1; pp += 8) {
            const double v = (double)base[(int64_t)pp * C + c];
            s += v;
            q += v * v;
        }
    red[g][threadIdx.x & 63] = make_double2(s, q);
    __syncthreads();
    if (g == 0 && c < C) {
        double2 t = red[0][threadIdx.x];
        for (int j = 1; j < 8; ++j) {
            t.x += red[j][threadIdx.x].x;
            t.y += red[j][threadIdx.x].y;
        }
        part[((int64_t)img * gridDim.z + ch) * C + c] = t;
    }
}

__global__ void instnorm_finish_kernel(const double2* part, int n_img, int HW, int C, int nchunk, float eps, float2* stats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img * C) return;
    const int img = i / C, c = i - img * C;
    double s = 0.0, q = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) {
        const double2 t = part[((int64_t)img * nchunk + ch) * C + c];
        s += t.x;
        q += t.y;
    }
    const double mean = s / HW, var = fmax(q / HW - mean * mean, 0.0);
    stats[i] = make_float2((float)mean, (float)(1.0 / sqrt(var + (double)eps)));
}

// ResidualBlock.forward's last line: out = relu(X + relu(norm2(y)))  (X: the block input, or norm3(downsample(x)))
__global__ void residual_join_kernel(const ConvSrc X, const ConvSrc Y, int64_t total, int HW, float* out) {
    const int C = Y.C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i / C;
        const int c = (int)(i - pix * C), img = (int)(pix / HW);
        const float a = src_value(X, pix, img, 0, 0, c), b = src_value(Y, pix, img, 0, 0, c);
        out[i] = fmaxf(a + b, 0.f);
    }
}

// the slot of pair pr under `sm` (kernels.h SlotMap)
__device__ __forceinline__ int64_t slot_of(const SlotMap& sm, int64_t pr) {
    const int64_t g = pr / sm.ppg;
    return g * sm.sb + (pr - g * sm.ppg) * sm.st;
}

// cnet output -> h = tanh(net) [M][128], x[:, 0:128] = relu(inp)  (x row stride 256), per pair; the context map [hw8][256] of pair pr is the one at
// slot `cs` of pr in cn (pairs that share their first frame share it)
__global__ void cnet_split_kernel(const float* cn, int64_t M, float* h, float* x, int64_t hw8, SlotMap cs) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M * 128; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i >> 7;
        const int c = (int)(i & 127);
        const int64_t pr = m / hw8;
        const float* src = cn + ((slot_of(cs, pr) - pr) * hw8 + m) * 256;
        h[i] = tanhf(src[c]);
        x[m * 256 + c] = fmaxf(src[128 + c], 0.f);
    }
}

__global__ void coords_init_kernel(float* coords, int64_t M, int h8, int w8) {
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(m % ((int64_t)h8 * w8));
        coords[2 * m] = (float)(r % w8);
        coords[2 * m + 1] = (float)(r / w8);
    }
}

// The warm start (raft_model.py:241-242): coords1 = grid + flow_init.  Element (c, y, x) of pair pr = (g, t) of the planar init field is at
// init[g * sb + t * st + c * sc + y * w8 + x] (a stride of 0 shares one field); one thread per low-resolution pixel, one float2 store of (x, y).
__global__ void coords_init_flow_kernel(float* coords, int64_t M, int h8, int w8, int ppg, const float* init, int64_t sb, int64_t st, int64_t sc) {
    const int64_t hw = (int64_t)h8 * w8;
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
        const int pr = (int)(m / hw), r = (int)(m - (int64_t)pr * hw);
        const int g = pr / ppg, t = pr - g * ppg;
        const float* f = init + g * sb + t * st + r;
        reinterpret_cast<float2*>(coords)[m] = make_float2((float)(r % w8) + f[0], (float)(r / w8) + f[sc]);
    }
}

// corr[p][i][j] = <f1[slot s1 of p][i], f2[slot s2 of p][j]> / sqrt(256), fp32 FMA (CorrBlock.corr); 64 x 64 tiles, 4 x 4 per thread
__global__ void __launch_bounds__(256) corr_kernel(const float* f1, const float* f2, int N, int D, float scale, float* corr, SlotMap s1, SlotMap s2) {
    __shared__ float As[16][64 + 4];
    __shared__ float Bs[16][64 + 4];
    const int p = blockIdx.z, i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const float* a = f1 + slot_of(s1, p) * N * D;
    const float* b = f2 + slot_of(s2, p) * N * D;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int lr = threadIdx.x >> 2, lk = (threadIdx.x & 3) * 4;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < D; k0 += 16) {
        const int ia = min(i0 + lr, N - 1), jb = min(j0 + lr, N - 1);
        const float4 va = *reinterpret_cast<const float4*>(a + (int64_t)ia * D + k0 + lk);
        const float4 vb = *reinterpret_cast<const float4*>(b + (int64_t)jb * D + k0 + lk);
        As[lk + 0][lr] = va.x; As[lk + 1][lr] = va.y; As[lk + 2][lr] = va.z; As[lk + 3][lr] = va.w;
        Bs[lk + 0][lr] = vb.x; Bs[lk + 1][lr] = vb.y; Bs[lk + 2][lr] = vb.z; Bs[lk + 3][lr] = vb.w;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            float av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                av[u] = As[kk][ty * 4 + u];
                bv[u] = Bs[kk][tx * 4 + u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(av[u], bv[v], acc[u][v]);
        }
        __syncthreads();
    }
    for (int u = 0; u < 4; ++u) {
        const int i = i0 + ty * 4 + u;
        if (i >= N) continue;
        for (int v = 0; v < 4; ++v) {
            const int j = j0 + tx * 4 + v;
            if (j < N) corr[((int64_t)p * N + i) * N + j] = acc[u][v] * scale;
        }
    }
}

// avg_pool2d(2, stride 2) of every [h][w] map (floor): the next pyramid level
__global__ void corr_pool_kernel(const float* in, int64_t maps, int h, int w, float* out, int oh, int ow) {
    const int64_t total = maps * oh * ow;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / ((int64_t)oh * ow);
        const int q = (int)(i - r * oh * ow), y = q / ow, x = q - y * ow;
        const float* s = in + r * h * w + (int64_t)(2 * y) * w + 2 * x;
        float acc = s[0];
        acc += s[1];
        acc += s[w];
        acc += s[w + 1];
        out[i] = acc / 4.f;
    }
}

// One axis of a lookup sample: coordinate c (level 0) displaced by d pixels on level l, whose side is `side` -> the left / upper tap i0 and the weight w of
// the tap after it.  The pixel coordinate is what grid_sample(align_corners=True) recovers from bilinear_sampler's normalisation, roundings included, so
// the two lookup kernels below take their taps and weights from one expression.
__device__ __forceinline__ void lookup_tap(float c, int l, int side, int d, int& i0, float& w) {
    const float cx = c / (float)(1 << l) + (float)d;
    const float gx = 2.f * cx / (float)(side - 1) - 1.f;
    const float ix = (gx + 1.f) * (0.5f * (float)(side - 1));
    const float fx = floorf(ix);
    i0 = (int)fx;
    w = ix - fx;
}

// CorrBlock.__call__: feature l*81 + a*9 + b of row m samples level l at (x + a - 4, y + b - 4) (the meshgrid(dy, dx) order), bilinear with
// zero padding as grid_sample(align_corners=True) after bilinear_sampler's normalisation; written as convc1's A operand (Kpad 384) in the
// layout of PLANES, or as fp32 (p.out)
template <int PLANES>
__global__ void corr_lookup_kernel(const CorrLookupParams p) {
    const int64_t total = p.M * (int64_t)p.Kpad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / p.Kpad;
        const int f = (int)(i - m * p.Kpad);
        float v = 0.f;
        if (f < p.levels * 81) {
            const int l = f / 81, a = (f - l * 81) / 9, b = f % 9;
            const int H = p.h[l], W = p.w[l];
            int x0, y0;
            float wx, wy;
            lookup_tap(p.coords[2 * m], l, W, a - 4, x0, wx);
            lookup_tap(p.coords[2 * m + 1], l, H, b - 4, y0, wy);
            const float* map = p.pyr[l] + m * (int64_t)H * W;
            auto at = [&](int yy, int xx) { return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? map[(int64_t)yy * W + xx] : 0.f; };
            v = at(y0, x0) * ((1.f - wx) * (1.f - wy)) + at(y0, x0 + 1) * (wx * (1.f - wy)) + at(y0 + 1, x0) * ((1.f - wx) * wy) +
                at(y0 + 1, x0 + 1) * (wx * wy);
        } else if (p.out) {
            continue;
        }
        if (p.out) p.out[m * p.out_ld + f] = v;
        else store_operand<PLANES>(p.A, m, p.Kpad, f, v);
    }
}

// avg_pool2d(2, stride 2), floor, of an NHWC feature map [P][h][w][C] -> [P][h / 2][w / 2][C]: the next level of fmap2 for the on-the-fly lookup
// (AlternateCorrBlock.__init__, corr.py:63-73).  Four channels per thread; the four pixels are added in corr_pool_kernel's order.  Output map j pools
// the input map at slot `is` of j.
__global__ void fmap_pool_kernel(const float* in, int64_t P, int h, int w, int C, float* out, int oh, int ow, SlotMap is) {
    const int c4n = C >> 2;
    const int64_t total = P * oh * ow * c4n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i / c4n;
        const int c4 = (int)(i - pix * c4n);
        const int64_t pr = pix / ((int64_t)oh * ow);
        const int q = (int)(pix - pr * oh * ow), y = q / ow, x = q - y * ow;
        const float4* s = reinterpret_cast<const float4*>(in + ((slot_of(is, pr) * h + 2 * y) * w + 2 * x) * C) + c4;
        const float4 a = s[0], b = s[c4n], c = s[(int64_t)w * c4n], d = s[(int64_t)w * c4n + c4n];
        float4 acc = a;
        acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w;
        acc.x += c.x; acc.y += c.y; acc.z += c.z; acc.w += c.w;
        acc.x += d.x; acc.y += d.y; acc.z += d.z; acc.w += d.w;
        reinterpret_cast<float4*>(out)[i] = make_float4(acc.x / 4.f, acc.y / 4.f, acc.z / 4.f, acc.w / 4.f);
    }
}

// AlternateCorrBlock.__call__ (corr.py:75-91) under corr_lookup_kernel's contract: the same features of the same taps and weights (lookup_tap), each
// tap's correlation computed here, <fmap1[m], fmap2_l[tap]> / 16 with fmap2_l the l times pooled fmap2 (pooling is linear: the pooled correlation of
// CorrBlock up to summation order).  One workgroup per row m, wave l on level l:
//   1. The nine displacements of an axis share their fraction, so their taps are i0 + a and i0 + a + 1 with one i0 -- or, when the pixel coordinate lies
//      within an ulp of an integer, with i0 and i0 - 1 mixed: the taps of a level fall into a window of 10 x 10 integer positions at
//      (xbase, ybase) = the smallest tap - displacement of each axis, 11 (kOtfWin) along an axis in the mixed case: its extent is the largest tap + 2.
//   2. The wave computes the 256-long dot product of every position in the intersection of that window and the level: eight lanes per position, 32
//      channels per lane as eight 16-byte loads (the eight lanes of a group read 128 contiguous bytes), fp32 FMA in channel order, then the DPP sum of
//      the group: a fixed order, no atomics.  A position outside the level is neither read nor stored: the blend takes it as 0, as the zero padding does.
//   3. The 324 features (and the K padding) are blended from the window in LDS by all 256 threads, with corr_lookup_kernel's expression.
constexpr int kOtfWin = 11;
constexpr int kOtfFar = 1 << 24;  // taps are clamped to +-kOtfFar: far outside every level either way, and differences of taps stay in range
template <int PLANES>
__global__ void __launch_bounds__(256) corr_lookup_on_the_fly_kernel(const CorrOnTheFlyParams p) {
    __shared__ float dots[4][kOtfWin * kOtfWin];
    __shared__ int tap_i[4][2][9];  // [level][x, y][displacement]: the first tap, relative to the window's origin
    __shared__ float tap_w[4][2][9];
    __shared__ int base[4][2];
    const int lane = threadIdx.x & (kWave - 1), l = threadIdx.x / kWave;
    const int grp = lane >> 3, sub = lane & 7;
    const int H = p.h[l], W = p.w[l];
    for (int64_t m = xcd_remap(blockIdx.x, gridDim.x); m < p.M; m += gridDim.x) {
        const float2 c = reinterpret_cast<const float2*>(p.coords)[m];
        const int a = lane % 9;  // lanes 0 .. 8 hold the nine displacements
        int x0, y0;
        float wx, wy;
        lookup_tap(c.x, l, W, a - 4, x0, wx);
        lookup_tap(c.y, l, H, a - 4, y0, wy);
        x0 = max(-kOtfFar, min(kOtfFar, x0));
        y0 = max(-kOtfFar, min(kOtfFar, y0));
        const int xr = x0 - a, yr = y0 - a;
        int xbase = __shfl(xr, 0, kWave), ybase = __shfl(yr, 0, kWave), xlast = __shfl(x0, 0, kWave), ylast = __shfl(y0, 0, kWave);
#pragma unroll
        for (int j = 1; j < 9; ++j) {
            xbase = min(xbase, __shfl(xr, j, kWave));
            ybase = min(ybase, __shfl(yr, j, kWave));
            xlast = max(xlast, __shfl(x0, j, kWave));
            ylast = max(ylast, __shfl(y0, j, kWave));
        }
        // the part of the window that taps reach (the largest tap and the one after it) and that lies in the level: columns [qx0, qx0 + nx), rows [qy0, qy0 + ny)
        const int qx0 = min(kOtfWin, max(0, -xbase)), qy0 = min(kOtfWin, max(0, -ybase));
        const int nx = max(0, min(min(kOtfWin, xlast - xbase + 2), W - xbase) - qx0), ny = max(0, min(min(kOtfWin, ylast - ybase + 2), H - ybase) - qy0);
        if (lane < 9) {
            tap_i[l][0][lane] = x0 - xbase;
            tap_w[l][0][lane] = wx;
            tap_i[l][1][lane] = y0 - ybase;
            tap_w[l][1][lane] = wy;
        }
        if (lane == 0) {
            base[l][0] = xbase;
            base[l][1] = ybase;
        }
        // the two maps of this row's pair: one per pair in pair order, or (p.ppg > 0) where the strides of the forward's shared frames put them
        const int64_t pr = m / p.hw8;
        int64_t m1 = m, slot2 = pr;
        if (p.ppg > 0) {
            const int64_t g = pr / p.ppg, t = pr - g * p.ppg;
            m1 = (g * p.s1b + t * p.s1t - pr) * p.hw8 + m;
            slot2 = g * p.s2b[l] + t * p.s2t[l];
        }
        const float4* f1 = reinterpret_cast<const float4*>(p.fmap1 + m1 * 256) + sub;
        float4 q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = f1[8 * i];
        const float* lvl = p.fmap2[l] + slot2 * H * W * 256;
        const int n = nx * ny;
        int qy = grp / max(nx, 1), qx = grp - qy * nx;  // position qi = s * 8 + grp of the nx x ny rectangle, kept as (qx, qy)
        for (int s = 0; s * 8 < n; ++s) {
            const int qi = s * 8 + grp;
            float acc = 0.f;
            if (qi < n) {
                const float4* r = reinterpret_cast<const float4*>(lvl + ((int64_t)(ybase + qy0 + qy) * W + xbase + qx0 + qx) * 256) + sub;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float4 v = r[8 * i];
                    acc = fmaf(q[i].x, v.x, acc);
                    acc = fmaf(q[i].y, v.y, acc);
                    acc = fmaf(q[i].z, v.z, acc);
                    acc = fmaf(q[i].w, v.w, acc);
                }
            }
            acc = group8_sum(acc);
            if (sub == 0 && qi < n) dots[l][(qy0 + qy) * kOtfWin + qx0 + qx] = acc * 0.0625f;  // / sqrt(256)
            for (qx += 8; qx >= nx && qy < ny; ++qy) qx -= nx;
        }
        __syncthreads();
        for (int f = threadIdx.x; f < p.Kpad; f += blockDim.x) {
            float v = 0.f;
            if (f < 4 * 81) {
                const int fl = f / 81, fa = (f - fl * 81) / 9, fb = f % 9;
                const int Hl = p.h[fl], Wl = p.w[fl];
                const int tx = tap_i[fl][0][fa], ty = tap_i[fl][1][fb];
                const int X0 = base[fl][0] + tx, Y0 = base[fl][1] + ty;
                // (a tap beyond the window can only come from a coordinate too large to have a fraction: it is outside the level, and not read)
                const int jx = max(0, min(kOtfWin - 2, tx)), jy = max(0, min(kOtfWin - 2, ty));
                const float ux = tap_w[fl][0][fa], uy = tap_w[fl][1][fb];
                const float* d = dots[fl];
                auto at = [&](int dy, int dx) {
                    const int yy = Y0 + dy, xx = X0 + dx;
                    return (yy >= 0 && yy < Hl && xx >= 0 && xx < Wl) ? d[(jy + dy) * kOtfWin + jx + dx] : 0.f;
                };
                v = at(0, 0) * ((1.f - ux) * (1.f - uy)) + at(0, 1) * (ux * (1.f - uy)) + at(1, 0) * ((1.f - ux) * uy) + at(1, 1) * (ux * uy);
            } else if (p.out) {
                continue;
            }
            if (p.out) p.out[m * p.out_ld + f] = v;
            else store_operand<PLANES>(p.A, m, p.Kpad, f, v);
        }
        __syncthreads();  // the window is free for the next row
    }
}

// BasicMotionEncoder's output: x[:, 128:254] = relu(conv(...)), x[:, 254:256] = flow
__global__ void motion_finish_kernel(float* x, const float* coords, int64_t M, int h8, int w8) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M * 128; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i >> 7;
        const int c = (int)(i & 127);
        float* d = x + m * 256 + 128 + c;
        if (c < 126) {
            *d = fmaxf(*d, 0.f);
        } else {
            const int r = (int)(m % ((int64_t)h8 * w8));
            *d = coords[2 * m + (c - 126)] - (float)(c == 126 ? r % w8 : r / w8);
        }
    }
}

// SepConvGRU state update: h = (1 - z) h + z tanh(q), z = sigmoid(zr[:, :128])
__global__ void gru_update_kernel(float* h, const float* zr, const float* q, int64_t M) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M * 128; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i >> 7;
        const int c = (int)(i & 127);
        const float z = sigmoidf_(zr[m * 256 + c]);
        const float qq = tanhf(q[i]);
        h[i] = (1.f - z) * h[i] + z * qq;
    }
}

__global__ void flow_update_kernel(float* coords, const float* delta, int ld, int64_t M) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * M; i += (int64_t)gridDim.x * blockDim.x)
        coords[i] = coords[i] + delta[(i >> 1) * ld + (i & 1)];
}

// RAFT.upsample_flow of a C-channel field v: out[c, 8y+i, 8x+j] = sum_k softmax_k(mask[k*64 + i*8 + j]) * 8 v[c, y+ky-1, x+kx-1] (k = 3ky + kx, zero
// padding).  v is the flow coords - (x, y) (p.coords, C = 2) or the planar p.value; one output pixel (all C channels) per thread.
template <int C>
__global__ void convex_upsample_kernel(const ConvexUpParams p) {
    const int H = 8 * p.h8, W = 8 * p.w8;
    const int64_t total = (int64_t)p.P * H * W, hw = (int64_t)p.h8 * p.w8;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int pr = (int)(i / ((int64_t)H * W));
        const int q = (int)(i - (int64_t)pr * H * W), Y = q / W, X = q - Y * W;
        const int y = Y >> 3, x = X >> 3, sub = (Y & 7) * 8 + (X & 7);
        const int64_t pix = ((int64_t)pr * p.h8 + y) * p.w8 + x;
        const float* mk = p.mask + pix * p.mask_ld + sub;
        float e[9], mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            e[k] = mk[k * 64] * p.mask_scale;
            mx = fmaxf(mx, e[k]);
        }
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            e[k] = expf(e[k] - mx);
            s += e[k];
        }
        float o[C] = {};
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
            float f[C] = {};
            if (yy >= 0 && yy < p.h8 && xx >= 0 && xx < p.w8) {
                const int64_t r = (int64_t)yy * p.w8 + xx;
#pragma unroll
                for (int c = 0; c < C; ++c)
                    f[c] = 8.f * (C == 2 && p.coords ? p.coords[2 * (pr * hw + r) + c] - (float)(c ? yy : xx) : p.value[((int64_t)pr * C + c) * hw + r]);
            }
            const float w = e[k] / s;
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] += w * f[c];
        }
        const int g = pr / p.ppg, t = pr - g * p.ppg;
        float* dst = p.out + g * p.out_sb + t * p.out_st + (int64_t)Y * W + X;
#pragma unroll
        for (int c = 0; c < C; ++c) dst[c * p.out_sc] = o[c];
    }
}

// flow_low[p][c][y][x] = coords1 - coords0 (the two-image call's first output)
__global__ void flow_low_kernel(const float* coords, int P, int h8, int w8, float* out) {
    const int64_t n = (int64_t)P * h8 * w8;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i >> 1;
        const int c = (int)(i & 1);
        const int pr = (int)(m / ((int64_t)h8 * w8)), r = (int)(m - (int64_t)pr * h8 * w8);
        out[((int64_t)pr * 2 + c) * h8 * w8 + r] = coords[i] - (float)(c ? r / w8 : r % w8);
    }
}

// forward_interpolate (raft/utils.py:28-56): carry a flow along itself.  Source pixel i = (y0, x0) of pair blockIdx.x / bpp lands at (x0 + dx[i], y0 + dy[i]),
// in double, where the sums are exact; target g takes both channels of the valid source with the smallest squared distance, the lowest i among equals
// (ascending scan, replaced on `<` only), zeros when no source is valid.  One target per thread; the sources pass through LDS in chunks of
// kFinterpChunk landing points, every lane reading the same address (a broadcast).  An invalid source (landing outside the open rectangle
// (0, w8) x (0, h8), or a NaN / infinite component) is staged as (+inf, +inf): its distance is +inf, which is never < the best, +inf at the start.
// Products and the sum are separately rounded (no fma): the order of near-equal distances is that of the same expression in numpy.
constexpr int kFinterpThreads = 256, kFinterpChunk = 1024;
__global__ void __launch_bounds__(kFinterpThreads) forward_interpolate_kernel(const float* flow, int64_t stride_p, int64_t stride_c, int bpp, int h8, int w8,
                                                                             float* out) {
#pragma clang fp contract(off)
    __shared__ double2 land[kFinterpChunk];
    const int N = h8 * w8;
    const int pr = blockIdx.x / bpp, tgt = (blockIdx.x - pr * bpp) * kFinterpThreads + threadIdx.x;
    const float* dx = flow + pr * stride_p;
    const float* dy = dx + stride_c;
    const double gx = (double)(tgt % w8), gy = (double)(tgt / w8);
    double best = INFINITY;
    int best_i = -1;
    for (int base = 0; base < N; base += kFinterpChunk) {
        const int cnt = min(kFinterpChunk, N - base);
        __syncthreads();  // the previous chunk has been read
        for (int j = threadIdx.x; j < cnt; j += kFinterpThreads) {
            const int i = base + j;
            const double x1 = (double)(i % w8) + (double)dx[i], y1 = (double)(i / w8) + (double)dy[i];
            const bool valid = x1 > 0.0 && x1 < (double)w8 && y1 > 0.0 && y1 < (double)h8;
            land[j] = valid ? make_double2(x1, y1) : make_double2(INFINITY, INFINITY);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const double2 s = land[j];
            const double ex = gx - s.x, ey = gy - s.y;
            const double d = ex * ex + ey * ey;
            if (d < best) {
                best = d;
                best_i = base + j;
            }
        }
    }
    if (tgt < N) {
        float* o = out + (int64_t)pr * 2 * N + tgt;
        o[0] = best_i < 0 ? 0.f : dx[best_i];
        o[N] = best_i < 0 ? 0.f : dy[best_i];
    }
}

// output_block.2 on relu(output_block.0(net)): one wave per low-resolution pixel, four consecutive channels per lane (one 16-byte load of the
// row and of the weight each), the 256 products summed in fp32 by the wave butterfly.
__global__ void __launch_bounds__(256) head_project_kernel(const float* hidden, int ld, const float* w, const float* bias, int64_t M, float* value) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wpb = blockDim.x / kWave;
    const float4 wv = reinterpret_cast<const float4*>(w)[lane];
    const float b = bias[0];
    for (int64_t m = (int64_t)blockIdx.x * wpb + threadIdx.x / kWave; m < M; m += (int64_t)gridDim.x * wpb) {
        const float4 v = *reinterpret_cast<const float4*>(hidden + m * ld + 4 * lane);
        float acc = fmaxf(v.x, 0.f) * wv.x;
        acc = fmaf(fmaxf(v.y, 0.f), wv.y, acc);
        acc = fmaf(fmaxf(v.z, 0.f), wv.z, acc);
        acc = fmaf(fmaxf(v.w, 0.f), wv.w, acc);
        acc = wave_sum(acc);
        if (lane == 0) value[m] = acc + b;
    }
}

// Convolution weights [N][C][kh][kw] -> rows row0 .. row0 + N of the GEMM's W operand in K order (ky, kx, c), zero padded to Kpad, in both layouts
// (il: parity, hi: fast); an eval-mode batch norm after the convolution is folded in: w * gamma / sqrt(var + eps), (b - mean) * gamma / sqrt(var + eps) + beta
__global__ void pack_conv_kernel(const float* w, const float* gamma, const float* var, float eps, int N, int C, int kh, int kw, int Kpad, int row0,
                                 bf16* il, bf16* hi) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * Kpad) return;
    const int n = (int)(i / Kpad), k = (int)(i - (int64_t)n * Kpad);
    float v = 0.f;
    if (k < kh * kw * C) {
        const int tap = k / C, c = k - tap * C, ky = tap / kw, kx = tap - ky * kw;
        v = w[(((int64_t)n * C + c) * kh + ky) * kw + kx];
        if (gamma) v = v * (gamma[n] / sqrtf(var[n] + eps));
    }
    store_operand<2>(il, row0 + n, Kpad, k, v);
    store_operand<1>(hi, row0 + n, Kpad, k, v);  // the fast plane: the folded weight rounded once (the parity hi plane is the same (bf16)v)
}

__global__ void pack_bias_kernel(const float* b, const float* gamma, const float* beta, const float* mean, const float* var, float eps, int N,
                                 float* dst) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    dst[n] = gamma ? (b[n] - mean[n]) * (gamma[n] / sqrtf(var[n] + eps)) + beta[n] : b[n];
}

unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 1 << 20); }

// the launch of every grid-stride kernel over n elements: 256 threads, one element per thread up to 2^20 workgroups
template <typename Kernel, typename... Args>
int launch_flat(Kernel kernel, int64_t n, hipStream_t s, Args... args) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(n)), dim3(256), 0, s, args...);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_pack_conv(const float* w, const float* b, const float* gamma, const float* beta, const float* mean, const float* var, float eps, int n, int cin,
                     int kh, int kw, int Kpad, int row0, bf16* w_il, bf16* w_hi, float* bias, hipStream_t s) {
    const int64_t total = (int64_t)n * Kpad;
    hipLaunchKernelGGL(pack_conv_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, gamma, var, eps, n, cin, kh, kw, Kpad, row0, w_il, w_hi);
    hipLaunchKernelGGL(pack_bias_kernel, dim3((n + 255) / 256), dim3(256), 0, s, b, gamma, beta, mean, var, eps, n, bias + row0);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

void set_conv_geometry(Im2colParams& ip, int n_img, int H, int W, int kh, int kw, int stride, int pad_h, int pad_w, int Kpad) {
    ip.n_img = n_img;
    ip.H = H;
    ip.W = W;
    ip.kh = kh;
    ip.kw = kw;
    ip.stride = stride;
    ip.pad_h = pad_h;
    ip.pad_w = pad_w;
    ip.OH = (H + 2 * pad_h - kh) / stride + 1;
    ip.OW = (W + 2 * pad_w - kw) / stride + 1;
    ip.Kpad = Kpad;
}

int pack_conv_parts(const ConvPartW* parts, int nparts, float eps, int cin, int kh, int kw, int Kpad, bf16* w_il, bf16* w_hi, float* bias, hipStream_t s) {
    int row0 = 0;
    for (int i = 0; i < nparts; ++i) {
        const ConvPartW& p = parts[i];
        if (int rc = launch_pack_conv(p.w, p.b, p.gamma, p.beta, p.mean, p.var, eps, p.n, cin, kh, kw, Kpad, row0, w_il, w_hi, bias, s)) return rc;
        row0 += p.n;
    }
    return 0;
}

GemmParams conv_gemm(const bf16* A, const bf16* W, const float* bias, int M, int N, int Kpad, float* C, int ldc) {
    GemmParams g = {};
    g.A = A;
    g.lda = Kpad;
    g.W = W;
    g.M = M;
    g.N = N;
    g.K = Kpad;
    g.bias = bias;
    g.epi = EPI_F32;
    g.C = C;
    g.ldc = ldc;
    return g;
}

int launch_im2col(const Im2colParams& p, int planes, hipStream_t s) {
    CWM_REQUIRE(p.Kpad % 64 == 0 && (p.c_hi <= p.c_lo || (p.c_lo % 8 == 0 && p.c_hi % 8 == 0)), "im2col: Kpad = %d, channel range [%d, %d)", p.Kpad,
                p.c_lo, p.c_hi);
    const int64_t total = (int64_t)p.n_img * p.OH * p.OW * (p.Kpad / 8);
    CWM_REQUIRE(total < (1ll << 31), "im2col: %lld groups exceed 32-bit indexing", (long long)total);
    hipLaunchKernelGGL(planes == 2 ? im2col_kernel<2> : im2col_kernel<1>, dim3(grid_for(total)), dim3(256), 0, s, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

int instnorm_chunks(int HW) { return std::min(kInstNormMaxChunks, (HW + 1023) / 1024); }

int launch_instnorm_stats(const float* x, int n_img, int HW, int C, float eps, float* stats, double* work, hipStream_t s) {
    const int nch = instnorm_chunks(HW), chunk = (HW + nch - 1) / nch;
    hipLaunchKernelGGL(instnorm_partial_kernel, dim3(n_img, (C + 63) / 64, nch), dim3(512), 0, s, x, HW, C, chunk, (double2*)work);
    hipLaunchKernelGGL(instnorm_finish_kernel, dim3((n_img * C + 255) / 256), dim3(256), 0, s, (const double2*)work, n_img, HW, C, nch, eps,
                       (float2*)stats);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_residual_join(const ConvSrc& X, const ConvSrc& Y, int n_img, int HW, float* out, hipStream_t s) {
    const int64_t total = (int64_t)n_img * HW * Y.C;
    return launch_flat(residual_join_kernel, total, s, X, Y, total, HW, out);
}

int launch_cnet_split(const float* cn, int64_t M, float* h, float* x, hipStream_t s, int64_t hw8, SlotMap cs) {
    CWM_REQUIRE(hw8 > 0 && M % hw8 == 0 && cs.ppg > 0, "cnet_split: %lld rows are not whole maps of %lld", (long long)M, (long long)hw8);
    return launch_flat(cnet_split_kernel, M * 128, s, cn, M, h, x, hw8, cs);
}

int launch_coords_init(float* coords, int64_t M, int h8, int w8, hipStream_t s) { return launch_flat(coords_init_kernel, M, s, coords, M, h8, w8); }

int launch_coords_init_flow(float* coords, int P, int ppg, int h8, int w8, const float* init, int64_t sb, int64_t st, int64_t sc, hipStream_t s) {
    const int64_t M = (int64_t)P * h8 * w8;
    return launch_flat(coords_init_flow_kernel, M, s, coords, M, h8, w8, ppg, init, sb, st, sc);
}

int launch_corr(const float* f1, const float* f2, int P, int N, int D, float* corr, hipStream_t s, SlotMap s1, SlotMap s2) {
    CWM_REQUIRE(D % 16 == 0 && s1.ppg > 0 && s2.ppg > 0, "corr: feature width %d must be a multiple of 16", D);
    hipLaunchKernelGGL(corr_kernel, dim3((N + 63) / 64, (N + 63) / 64, P), dim3(256), 0, s, f1, f2, N, D, 1.f / sqrtf((float)D), corr, s1, s2);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_corr_pool(const float* in, int64_t maps, int h, int w, float* out, hipStream_t s) {
    const int oh = h / 2, ow = w / 2;
    return launch_flat(corr_pool_kernel, maps * oh * ow, s, in, maps, h, w, out, oh, ow);
}

int launch_corr_lookup(const CorrLookupParams& p, int planes, hipStream_t s) {
    return launch_flat(planes == 2 ? corr_lookup_kernel<2> : corr_lookup_kernel<1>, p.M * p.Kpad, s, p);
}

int launch_fmap_pool(const float* in, int64_t P, int h, int w, int C, float* out, hipStream_t s, SlotMap is) {
    CWM_REQUIRE(C % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0 && is.ppg > 0, "fmap_pool: %d channels in 16-byte aligned maps are required", C);
    const int oh = h / 2, ow = w / 2;
    return launch_flat(fmap_pool_kernel, P * oh * ow * (C / 4), s, in, P, h, w, C, out, oh, ow, is);
}

int launch_corr_lookup_on_the_fly(const CorrOnTheFlyParams& p, int planes, hipStream_t s) {
    bool aligned = ((uintptr_t)p.fmap1 & 15) == 0 && ((uintptr_t)p.coords & 7) == 0;
    for (const float* f : p.fmap2) aligned = aligned && ((uintptr_t)f & 15) == 0;
    CWM_REQUIRE(aligned && p.M > 0 && p.hw8 > 0 && p.M % p.hw8 == 0 && p.ppg >= 0, "corr_lookup_on_the_fly: 16-byte aligned feature maps and whole pairs are required");
    // one workgroup of four waves (one per level) per row
    hipLaunchKernelGGL(planes == 2 ? corr_lookup_on_the_fly_kernel<2> : corr_lookup_on_the_fly_kernel<1>, dim3((unsigned)std::min<int64_t>(p.M, 1 << 20)),
                       dim3(4 * kWave), 0, s, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_motion_finish(float* x, const float* coords, int64_t M, int h8, int w8, hipStream_t s) {
    return launch_flat(motion_finish_kernel, M * 128, s, x, coords, M, h8, w8);
}

int launch_gru_update(float* h, const float* zr, const float* q, int64_t M, hipStream_t s) { return launch_flat(gru_update_kernel, M * 128, s, h, zr, q, M); }

int launch_flow_update(float* coords, const float* delta, int ld, int64_t M, hipStream_t s) {
    return launch_flat(flow_update_kernel, 2 * M, s, coords, delta, ld, M);
}

ConvexUpParams convex_up_params(int C, const float* coords, const float* value, const float* mask, float mask_scale, int P, int ppg, int h8, int w8, float* out,
                                int64_t out_sb, int64_t out_st, int64_t out_sc) {
    ConvexUpParams p = {};
    p.coords = coords;
    p.value = value;
    p.mask = mask;
    p.mask_ld = 576;
    p.mask_scale = mask_scale;
    p.C = C;
    p.P = P;
    p.ppg = ppg;
    p.h8 = h8;
    p.w8 = w8;
    p.out = out;
    p.out_sb = out_sb;
    p.out_st = out_st;
    p.out_sc = out_sc;
    return p;
}

int launch_convex_upsample(const ConvexUpParams& p, hipStream_t s) {
    return launch_flat(p.C == 2 ? convex_upsample_kernel<2> : convex_upsample_kernel<1>, (int64_t)p.P * 64 * p.h8 * p.w8, s, p);
}

int launch_flow_low(const float* coords, int P, int h8, int w8, float* out, hipStream_t s) {
    return launch_flat(flow_low_kernel, (int64_t)2 * P * h8 * w8, s, coords, P, h8, w8, out);
}

int launch_forward_interpolate(const float* flow, int64_t stride_p, int64_t stride_c, int P, int h8, int w8, float* out, hipStream_t s) {
    CWM_REQUIRE(flow && out && P >= 1 && h8 >= 1 && w8 >= 1, "forward_interpolate: bad argument (P = %d, grid %d x %d)", P, h8, w8);
    const int64_t N = (int64_t)h8 * w8;
    CWM_REQUIRE(N <= 65536, "forward_interpolate: a grid of %d x %d = %lld pixels exceeds 65536 (every target scans every source: the cost is N^2)", h8, w8,
                (long long)N);
    const int64_t bpp = (N + kFinterpThreads - 1) / kFinterpThreads;
    CWM_REQUIRE(P * bpp < (1ll << 31) && 2 * P * N < (1ll << 31), "forward_interpolate: %d fields of %lld pixels exceed 32-bit indexing", P, (long long)N);
    // what is read: rows [0, N) of channels 0, 1 of fields 0 .. P - 1 (strides of either sign); what is written: [P][2][N]
    const int64_t lo = std::min<int64_t>(0, (P - 1) * stride_p) + std::min<int64_t>(0, stride_c);
    const int64_t hi = std::max<int64_t>(0, (P - 1) * stride_p) + std::max<int64_t>(0, stride_c) + N;
    const intptr_t f = (intptr_t)flow, o = (intptr_t)out, fsz = sizeof(float);
    CWM_REQUIRE(o + 2 * P * N * fsz <= f + lo * fsz || f + hi * fsz <= o, "forward_interpolate: out overlaps flow (every target reads other pixels' sources)");
    hipLaunchKernelGGL(forward_interpolate_kernel, dim3((unsigned)(P * bpp)), dim3(kFinterpThreads), 0, s, flow, stride_p, stride_c, (int)bpp, h8, w8, out);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_head_project(const float* hidden, int ld,const float* w, const float* bias, int64_t M, float* value, hipStream_t s) {
    CWM_REQUIRE(ld >= kHeadHidden && ld % 4 == 0 && ((uintptr_t)hidden & 15) == 0 && ((uintptr_t)w & 15) == 0,
                "head_project: rows of %d floats and 16-byte aligned operands are required (ld = %d)", kHeadHidden, ld);
    hipLaunchKernelGGL(head_project_kernel, dim3(grid_for(M * kWave)), dim3(256), 0, s, hidden, ld, w, bias, M, value);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace cwm
