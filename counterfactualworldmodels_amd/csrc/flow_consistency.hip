// Forward-backward flow consistency (cwm_flow_consistency): whether a flow vector can be believed.  The flow a of grid A is followed to the other frame, the
// other frame's flow o is sampled there, and the round trip is held against a threshold that grows with the motion.  Out come a code per pixel (0 consistent,
// 1 inconsistent: occluded or wrong, 2 the target lies outside the frame), the residual, the flow with NaN written where it failed -- which cwm_segment_track
// reads as "falls outside" --, the failing fraction per P x P cell and the three counts per row.  No counterpart in the reference.
//
// The definition (this is the contract; include/cwm_hip.h repeats it for callers).  a[b] and o[b] are flows [2][H][W], pixel (b, c, y, x) at
// base[b strides[0] + c strides[1] + y W + x], channel 0 horizontal and channel 1 vertical, in pixels; a lives on its own grid A and points to the other frame,
// o lives on the other frame's grid and points back.  Every arithmetic step is ONE correctly rounded fp32 operation in the stated order: nothing is contracted
// into a fused multiply-add.  Per row b and pixel (y, x) of grid A, (u, v) = a[:, y, x]:
//   1 target   fx = (float)x + u, fy = (float)y + v; INSIDE iff fx >= 0 && fx <= W-1 && fy >= 0 && fy <= H-1, in fp32 and before anything is converted to an
//              integer (NaN, inf and huge flows are outside).  Outside: code = 2, res = +inf, and nothing of o is read
//   2 sample   x0f = floorf(fx), wx = fx - x0f, ix0 = (int)x0f, ix1 = min(ix0 + 1, W-1); the same in y.  Per channel c of o, with o00 = o[c][iy0][ix0],
//              o01 = o[c][iy0][ix1], o10 = o[c][iy1][ix0], o11 = o[c][iy1][ix1]: top = o00 + wx (o01 - o00), bot = o10 + wx (o11 - o10),
//              s_c = top + wy (bot - top).  (The clamp: a target exactly on the last column or row is inside and reads nothing beyond the plane)
//   3 residual ru = u + s_0, rv = v + s_1, res = ru ru + rv rv; mag = (u u + v v) + (s_0 s_0 + s_1 s_1); thr = alpha mag + beta
//   4 decision code = 0 iff res <= thr (equality is consistent), otherwise 1: a NaN anywhere (a NaN or inf sample of o) compares false and gives 1.
//              res_out = res if res == res, else +inf
//   5 masked   m[:, y, x] = a[:, y, x] where code == 0; elsewhere both channels are the quiet NaN 0x7fc00000
//   6 cells    cell[i][j] = (the number of the cell's P P pixels with code != 0) / (float)(P P): an integer count and one exact division
//   7 stats    [b][4]: the numbers of pixels with code 0, code 1 and code 2, then 0
// both = 1: the same call also produces everything with the roles of a and o exchanged, as direction d = 1 of a leading dimension D = 2.
//
// One kernel, behind one memset of the stats when they are asked for.  What was chosen, and why:
//   a thread owns 4 consecutive pixels of a row: float4 loads of u and v where the planes of both flows are 16-byte aligned in every row (narrow loads
//   otherwise; the host picks one of four instantiations from the addresses and strides), the 4 x 4 x 2 taps of o as 32 independent gathers through the
//   caches (a plane is at most 1 MB; latency, not bandwidth), one 4-byte store of codes, 16-byte stores of res and of the two masked planes (narrow stores
//   where the caller's buffer is not aligned).
//   a workgroup of 256 threads owns a tile of 16 rows x 64 columns, which holds whole cells for every P (edge tiles are partial, and H and W are multiples of
//   P): the 4 pixels of a thread lie in one cell, the cell counts are LDS integer adds and are written once -- no global atomics, no workspace.
//   direction d is grid dimension z and exchanges the two pointer sets.
//   stats: shuffles over the wave, one LDS add per wave, then three global INTEGER atomics per workgroup into the output itself, which the call zeroes on the
//   stream first: the same bits in any order.
// No content of a device buffer moves an address: the target is tested in fp32 before it is converted, so every tap index lies in [0, H W).
#include <cstring>

#include "../../include/cwm_hip.h"
#include "common.h"

#pragma clang fp contract(off)  // (file scope: the helpers and the kernel below; a*b+c stays a multiply and an add)

namespace cwm {

namespace {

constexpr int kConsMaxPixels = 1 << 18;
constexpr int kConsThreads = 256;
constexpr int kConsTileH = 16, kConsTileW = 64;  // whole cells for P = 4, 8, 16
constexpr int kConsMaxCells = (kConsTileH / 4) * (kConsTileW / 4);
static_assert(kConsTileH * (kConsTileW / 4) == kConsThreads, "a thread per 4 pixels of the tile");

struct ConsParams {
    const float *a, *o;  // direction 1 exchanges them
    int64_t as0, as1, os0, os1;
    int B, H, W, P;
    float alpha, beta;
    uint8_t* code;
    float *res, *masked, *cell;
    int* stats;
};

template <bool kVec>
__device__ __forceinline__ void cons_load4(const float* q, float (&f)[4]) {
    if (kVec) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        f[0] = t.x, f[1] = t.y, f[2] = t.z, f[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = q[i];
    }
}
template <bool kVec>
__device__ __forceinline__ void cons_store4(float* q, const float (&f)[4]) {
    if (kVec) {
        *reinterpret_cast<float4*>(q) = make_float4(f[0], f[1], f[2], f[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = f[i];
    }
}

// grid (tiles of 16 x 64 pixels, B, D).  kVecIn: all four input planes of every row are 16-byte aligned; kVecOut: so are the outputs given (the host decides:
// with a run-time test in the kernel the compiler merges the two forms into the narrow one)
template <bool kVecIn, bool kVecOut>
__global__ __launch_bounds__(kConsThreads) void flow_consistency_kernel(const ConsParams p) {
    __shared__ int cell_s[kConsMaxCells];
    __shared__ int stat_s[2];
    const int d = blockIdx.z, b = blockIdx.y, tid = threadIdx.x, W = p.W, H = p.H, HW = H * W;
    const int tiles_x = (W + kConsTileW - 1) / kConsTileW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int ly = tid >> 4, lx = 4 * (tid & 15);
    const int y = ty * kConsTileH + ly, x0 = tx * kConsTileW + lx;
    if (tid < kConsMaxCells) cell_s[tid] = 0;
    if (tid < 2) stat_s[tid] = 0;
    __syncthreads();
    int n1 = 0, n2 = 0;
    if (y < H && x0 < W) {  // (W is a multiple of 4: the thread's four pixels are in or out together)
        const float* au = (d ? p.o : p.a) + (int64_t)b * (d ? p.os0 : p.as0);
        const float* av = au + (d ? p.os1 : p.as1);
        const float* ou = (d ? p.a : p.o) + (int64_t)b * (d ? p.as0 : p.os0);
        const float* ov = ou + (d ? p.as1 : p.os1);
        const int pix = y * W + x0;
        float u[4], v[4];
        cons_load4<kVecIn>(au + pix, u);
        cons_load4<kVecIn>(av + pix, v);
        const float xmax = (float)(W - 1), ymax = (float)(H - 1);
        bool inside[4];
        int at[4][4];  // the four taps: (iy0, ix0), (iy0, ix1), (iy1, ix0), (iy1, ix1)
        float wx[4], wy[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float fx = (float)(x0 + j) + u[j], fy = (float)y + v[j];
            inside[j] = fx >= 0.f && fx <= xmax && fy >= 0.f && fy <= ymax;
            const float x0f = floorf(fx), y0f = floorf(fy);
            wx[j] = fx - x0f, wy[j] = fy - y0f;
            const int ix0 = inside[j] ? (int)x0f : 0, iy0 = inside[j] ? (int)y0f : 0;  // (converted only after the fp32 test)
            const int ix1 = min(ix0 + 1, W - 1), iy1 = min(iy0 + 1, H - 1);
            at[j][0] = iy0 * W + ix0, at[j][1] = iy0 * W + ix1, at[j][2] = iy1 * W + ix0, at[j][3] = iy1 * W + ix1;
        }
        float tu[4][4], tv[4][4];  // 32 independent gathers; an outside pixel reads nothing
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int k = 0; k < 4; ++k) tu[j][k] = inside[j] ? ou[at[j][k]] : 0.f, tv[j][k] = inside[j] ? ov[at[j][k]] : 0.f;
        }
        const float inf = __int_as_float(0x7f800000), qnan = __int_as_float(0x7fc00000);
        float res[4], mu[4], mv[4];
        unsigned codes = 0;
        int bad = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float topu = tu[j][0] + wx[j] * (tu[j][1] - tu[j][0]), botu = tu[j][2] + wx[j] * (tu[j][3] - tu[j][2]);
            const float topv = tv[j][0] + wx[j] * (tv[j][1] - tv[j][0]), botv = tv[j][2] + wx[j] * (tv[j][3] - tv[j][2]);
            const float s0 = topu + wy[j] * (botu - topu), s1 = topv + wy[j] * (botv - topv);
            const float ru = u[j] + s0, rv = v[j] + s1;
            const float r = ru * ru + rv * rv;
            const float mag = (u[j] * u[j] + v[j] * v[j]) + (s0 * s0 + s1 * s1);
            const float thr = p.alpha * mag + p.beta;
            const int code = !inside[j] ? 2 : (r <= thr ? 0 : 1);
            res[j] = (inside[j] && r == r) ? r : inf;
            mu[j] = code == 0 ? u[j] : qnan, mv[j] = code == 0 ? v[j] : qnan;
            codes |= (unsigned)code << (8 * j);
            n1 += code == 1, n2 += code == 2, bad += code != 0;
        }
        const size_t plane = ((size_t)d * p.B + b) * HW;
        if (p.code) {
            uint8_t* q = p.code + plane + pix;
            if (kVecOut) {
                *reinterpret_cast<unsigned*>(q) = codes;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j] = (uint8_t)(codes >> (8 * j));
            }
        }
        if (p.res) cons_store4<kVecOut>(p.res + plane + pix, res);
        if (p.masked) {
            cons_store4<kVecOut>(p.masked + 2 * plane + pix, mu);
            cons_store4<kVecOut>(p.masked + 2 * plane + HW + pix, mv);
        }
        if (p.cell && bad) atomicAdd(&cell_s[(ly / p.P) * (kConsTileW / p.P) + lx / p.P], bad);
    }
    if (p.stats) {  // (every lane takes part in the shuffles)
        int packed = n1 | (n2 << 16);  // at most 1024 each per workgroup
#pragma unroll
        for (int s = 32; s; s >>= 1) packed += __shfl_xor(packed, s, 64);
        if ((tid & 63) == 0 && packed) atomicAdd(&stat_s[0], packed & 0xffff), atomicAdd(&stat_s[1], packed >> 16);
    }
    __syncthreads();
    if (p.cell) {
        const int per_row = kConsTileW / p.P, n_cells = (kConsTileH / p.P) * per_row;
        if (tid < n_cells) {
            const int ci = tid / per_row, cj = tid - ci * per_row;
            const int gh = H / p.P, gw = W / p.P, gy = ty * (kConsTileH / p.P) + ci, gx = tx * per_row + cj;
            if (gy < gh && gx < gw) p.cell[(((size_t)d * p.B + b) * gh + gy) * gw + gx] = __fdiv_rn((float)cell_s[tid], (float)(p.P * p.P));
        }
    }
    if (p.stats && tid == 0) {
        const int n_pix = min(kConsTileH, H - ty * kConsTileH) * min(kConsTileW, W - tx * kConsTileW);
        int* st = p.stats + 4 * ((size_t)d * p.B + b);
        const int c1 = stat_s[0], c2 = stat_s[1];
        if (n_pix - c1 - c2) atomicAdd(&st[0], n_pix - c1 - c2);
        if (c1) atomicAdd(&st[1], c1);
        if (c2) atomicAdd(&st[2], c2);
    }
}

}  // namespace

}  // namespace cwm

using namespace cwm;

extern "C" int cwm_flow_consistency(const cwm_flow_consistency_args* a) {
    CWM_REQUIRE(a && a->struct_size == sizeof(cwm_flow_consistency_args),
                "cwm_flow_consistency: args->struct_size must be sizeof(cwm_flow_consistency_args)");
    const cwm_patch_error_args& g = a->base;
    CWM_REQUIRE(g.batch >= 1 && g.batch <= 65535, "cwm_flow_consistency: base.batch = %d, 1 .. 65535", g.batch);
    CWM_REQUIRE(g.H > 0 && g.H % 4 == 0, "cwm_flow_consistency: base.H = %d must be a positive multiple of 4", g.H);
    CWM_REQUIRE(g.W > 0 && g.W % 4 == 0, "cwm_flow_consistency: base.W = %d must be a positive multiple of 4", g.W);
    CWM_REQUIRE((int64_t)g.H * g.W <= kConsMaxPixels, "cwm_flow_consistency: base.H base.W = %lld pixels, at most %d", (long long)g.H * g.W, kConsMaxPixels);
    CWM_REQUIRE(a->a_dev, "cwm_flow_consistency: a_dev is NULL");
    CWM_REQUIRE(a->o_dev, "cwm_flow_consistency: o_dev is NULL");
    CWM_REQUIRE(a->a_strides[0] >= 0 && a->a_strides[1] >= 0, "cwm_flow_consistency: a_strides = (%lld, %lld) must not be negative", (long long)a->a_strides[0],
                (long long)a->a_strides[1]);
    CWM_REQUIRE(a->o_strides[0] >= 0 && a->o_strides[1] >= 0, "cwm_flow_consistency: o_strides = (%lld, %lld) must not be negative", (long long)a->o_strides[0],
                (long long)a->o_strides[1]);
    CWM_REQUIRE(a->alpha >= 0.f && a->alpha <= 3.4028234664e38f, "cwm_flow_consistency: alpha = %g must be finite and not negative", (double)a->alpha);
    CWM_REQUIRE(a->beta >= 0.f && a->beta <= 3.4028234664e38f, "cwm_flow_consistency: beta = %g must be finite and not negative", (double)a->beta);
    CWM_REQUIRE(a->both == 0 || a->both == 1, "cwm_flow_consistency: both = %d, 0 or 1", a->both);
    CWM_REQUIRE(a->code_dev || a->res_dev || a->masked_dev || a->cell_dev || a->stats_dev, "cwm_flow_consistency: no output requested");
    if (a->cell_dev) {
        CWM_REQUIRE(g.P == 4 || g.P == 8 || g.P == 16, "cwm_flow_consistency: base.P = %d with cell_dev: 4, 8 or 16", g.P);
        CWM_REQUIRE(g.H % g.P == 0 && g.W % g.P == 0, "cwm_flow_consistency: base.H = %d and base.W = %d must be multiples of base.P = %d with cell_dev", g.H, g.W,
                    g.P);
    }
    ConsParams p;
    memset(&p, 0, sizeof(p));
    p.a = a->a_dev, p.as0 = a->a_strides[0], p.as1 = a->a_strides[1], p.o = a->o_dev, p.os0 = a->o_strides[0], p.os1 = a->o_strides[1];
    p.B = g.batch, p.H = g.H, p.W = g.W, p.P = a->cell_dev ? g.P : 4;
    p.alpha = a->alpha, p.beta = a->beta;
    p.code = a->code_dev, p.res = a->res_dev, p.masked = a->masked_dev, p.cell = a->cell_dev, p.stats = a->stats_dev;
    const int D = a->both ? 2 : 1;
    hipStream_t stream = (hipStream_t)g.stream;
    if (p.stats) CWM_HIP_CHECK(hipMemsetAsync(p.stats, 0, (size_t)D * p.B * 4 * sizeof(int), stream));  // the table the workgroups add into
    const unsigned tiles = (unsigned)(((p.W + kConsTileW - 1) / kConsTileW) * ((p.H + kConsTileH - 1) / kConsTileH));
    // 16-byte accesses need the base on a 16-byte address and the strides (elements) multiples of 4: every plane of every row is then aligned (H W % 16 == 0)
    const auto misaligned = [](const void* q, int64_t s0, int64_t s1) {
        return ((reinterpret_cast<uintptr_t>(q) & 15) | (uintptr_t)(s0 & 3) | (uintptr_t)(s1 & 3)) != 0;
    };
    const bool vec_in = !misaligned(p.a, p.as0, p.as1) && !misaligned(p.o, p.os0, p.os1);
    const bool vec_out = !misaligned(p.res, 0, 0) && !misaligned(p.masked, 0, 0) && (reinterpret_cast<uintptr_t>(p.code) & 3) == 0;
    const dim3 grid(tiles, (unsigned)p.B, (unsigned)D), block(kConsThreads);
    if (vec_in && vec_out) hipLaunchKernelGGL((flow_consistency_kernel<true, true>), grid, block, 0, stream, p);
    else if (vec_in) hipLaunchKernelGGL((flow_consistency_kernel<true, false>), grid, block, 0, stream, p);
    else if (vec_out) hipLaunchKernelGGL((flow_consistency_kernel<false, true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((flow_consistency_kernel<false, false>), grid, block, 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}
