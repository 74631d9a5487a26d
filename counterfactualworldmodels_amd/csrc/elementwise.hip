// HBM-bound edge kernels of the VMAE predictor path (gfx950): LayerNorm, mask -> token permutation
// (bit-exact index op), frame load + imagenet-normalise + tubelet patch gather, decoder mask-token
// fill, patch un-embed scatter, fp32 -> bf16 (hi, lo) split.
#include "common.h"
#include "kernels.h"
#include <algorithm>

namespace cwm {

// ---------------------------------------------------------------------------------------------
// LayerNorm (eps 1e-6, affine) -> bf16 hi(/lo) planes.  Reference: nn.LayerNorm call sites
// VideoMAE/utils.py:148-149 (norm1/norm2), vmae.py:172 (encoder.norm), :251 (decoder.norm on the
// last Nm tokens).  One wave per row, row kept in registers (16-byte loads and stores), two-pass mean/variance in fp32.
// ---------------------------------------------------------------------------------------------
template <int PLANES>
__global__ __launch_bounds__(256) void layernorm_kernel(const LayerNormParams p) {
    constexpr int MAXI = 2;  // D <= 1024: lane l owns elements 8 l + 512 i .. + 7 (two 16-byte loads; ONE 16-byte store per plane: round 4 --
                             // 8-byte stores ran at 0.55-0.7 of the 16-byte rate, MI355X_MICROARCH.md; 8 consecutive k never straddle a
                             // 32-k [hi | lo] block)
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.rows) return;
    int in_row = r;
    if (p.rows_out_per_b > 0) {
        const int b = r / p.rows_out_per_b;
        in_row = b * p.rows_in_per_b + p.in_offset + (r - b * p.rows_out_per_b);
    }
    const float* x = p.x + (size_t)in_row * p.ldx;
    f32x4 v[MAXI][2];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
        const int idx = lane * 8 + i * 512;
        if (idx < p.D) {
            v[i][0] = *reinterpret_cast<const f32x4*>(x + idx);
            v[i][1] = *reinterpret_cast<const f32x4*>(x + idx + 4);
            s += ((v[i][0][0] + v[i][0][1]) + (v[i][0][2] + v[i][0][3])) + ((v[i][1][0] + v[i][1][1]) + (v[i][1][2] + v[i][1][3]));
        } else {
            v[i][0] = v[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    const float mean = wave_sum_dpp(s) / (float)p.D;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
        const int idx = lane * 8 + i * 512;
        if (idx < p.D) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = v[i][h][e] - mean;
                    sq += a * a;
                }
        }
    }
    const float rstd = rsqrtf(wave_sum_dpp(sq) / (float)p.D + p.eps);
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
        const int idx = lane * 8 + i * 512;
        if (idx < p.D) {
            f32x4 y[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x4 g = *reinterpret_cast<const f32x4*>(p.gamma + idx + 4 * h);
                const f32x4 be = *reinterpret_cast<const f32x4*>(p.beta + idx + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) y[h][e] = (v[i][h][e] - mean) * rstd * g[e] + be[e];
                if (p.out_f32) *reinterpret_cast<f32x4*>(p.out_f32 + (size_t)r * p.D + idx + 4 * h) = y[h];
            }
            store_operand8<PLANES>(p.out, r, p.ldo, idx, y[0], y[1]);
        }
    }
}

int launch_layernorm(const LayerNormParams& p, int planes, hipStream_t stream) {
    CWM_REQUIRE(p.D % 8 == 0 && p.D <= 1024, "layernorm: D=%d must be a multiple of 8 and <= 1024", p.D);
    CWM_REQUIRE(p.ldx % 4 == 0 && p.ldo % 8 == 0, "layernorm: row strides must be multiples of 4 (input) / 8 (output)");
    // (a_pos puts column c of a split row at 64 (c / 32) + c % 32, its lo half 32 further: the last block of a row whose ldo is no multiple of 32 would reach
    // into the next row -- D = 40 in rows of ldo = 40 wrote the lo half of columns 32..39 of row r over the hi half of columns 16..23 of row r + 1)
    CWM_REQUIRE(p.ldo >= p.D && (planes == 1 || p.ldo % 32 == 0),
                "layernorm: %d columns in output rows of ldo=%d (split-bf16 rows are whole [32 hi | 32 lo] blocks: a multiple of 32)", p.D, p.ldo);
    const int blocks = (p.rows + 3) / 4;
    dispatch_int<2, 1>(planes == 1 ? 1 : 2, [&](auto pl) { hipLaunchKernelGGL(layernorm_kernel<pl.value>, dim3(blocks), dim3(256), 0, stream, p); });
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// mask -> permutation.  Reference: `x[~mask].reshape(B,-1,C)` (vmae.py:167) and the decoder order
// `cat([vis, masked])` (vmae.py:555-557): visible tokens in ascending token index, then masked
// tokens in ascending token index.  Integer-exact; one workgroup per sample, block-wide scan.
// ---------------------------------------------------------------------------------------------
// Exclusive prefix of `count` over the 256 threads of a workgroup, in thread order, and the workgroup's total: an inclusive shuffle scan per
// wave, the four wave totals through LDS (`wave_tot`, 4 ints), ONE __syncthreads (which callers may rely on for their own LDS writes).
__device__ __forceinline__ int block_exclusive_scan256(int count, int* wave_tot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = count;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int before = incl - count;
    for (int w = 0; w < wave; ++w) before += wave_tot[w];
    total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    return before;
}

// Ragged batches (n_vis_min > 0): a row may have n_vis_min .. n_vis visible tokens, and its count goes to counts[b].
__global__ __launch_bounds__(256) void mask_to_perm_kernel(const uint8_t* mask, int Nt, int n_vis, int* perm, int* err, int n_vis_min, int* counts) {
    __shared__ int wave_tot[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const uint8_t* m = mask + (size_t)b * Nt;
    const int per = (Nt + 255) / 256;
    const int lo = min(t * per, Nt), hi = min(lo + per, Nt);
    int c = 0;
    for (int i = lo; i < hi; ++i) c += (m[i] == 0);
    int tv;
    int vis_before = block_exclusive_scan256(c, wave_tot, tv);
    if (t == 0 && (n_vis_min > 0 ? (tv < n_vis_min || tv > n_vis) : tv != n_vis)) atomicExch(err, 1);
    if (t == 0 && counts) counts[b] = tv;
    int* pr = perm + (size_t)b * Nt;
    for (int i = lo; i < hi; ++i) {
        if (m[i] == 0) {
            pr[vis_before] = i;
            ++vis_before;
        } else {
            pr[tv + (i - vis_before)] = i;
        }
    }
}

int launch_mask_to_perm(const uint8_t* mask, int B, int Nt, int n_vis, int* perm, int* err, hipStream_t stream, int n_vis_min, int* counts) {
    CWM_REQUIRE(n_vis_min == 0 || (n_vis_min > 0 && n_vis_min <= n_vis && counts), "mask_to_perm (ragged): bad argument");
    hipLaunchKernelGGL(mask_to_perm_kernel, dim3(B), dim3(256), 0, stream, mask, Nt, n_vis, perm, err, n_vis_min, counts);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void perm_to_rank_kernel(const int* perm, int* rank, int Nt, int total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int b = i / Nt;
    rank[(size_t)b * Nt + perm[i]] = i - b * Nt;
}

int launch_perm_to_rank(const int* perm, int* rank, int B, int Nt, hipStream_t stream) {
    const int total = B * Nt;
    hipLaunchKernelGGL(perm_to_rank_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, perm, rank, Nt, total);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Frame load + imagenet normalise + tubelet patch gather (im2col of the visible tokens only).
// Reference: `_preprocess` + `imagenet_normalize` (prediction.py:304-312, utils.py:15-21) and the
// Conv3d patch embed (VideoMAE/utils.py:174-197), whose GEMM is done by gemm.hip on this matrix.
// The reference embeds all Nt tokens and gathers afterwards (vmae.py:155-167); the embed is
// per-token, so gathering first is identical and skips the masked half of frame 2.
// One thread per (row, c, ph): reads P contiguous pixels, writes P contiguous bf16.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void imagenet_mean_std(int c, float& mean, float& stdv) {
    mean = (c == 0) ? 0.485f : (c == 1) ? 0.456f : 0.406f;
    stdv = (c == 0) ? 0.229f : (c == 1) ? 0.224f : 0.225f;
}

// The body of every tubelet gather, one (row, channel, patch row) item: P contiguous pixels at `src` -> columns kbase .. kbase + P - 1 of
// operand row `row`, as (a - shift) / div when `arith`, as they are otherwise.  A pad slot (the null token of a padded predictor: no pixels
// behind it) reads nothing and writes exact zeros.
template <int PLANES>
__device__ __forceinline__ void gather_item(const float* src, bool pad_slot, bool arith, float shift, float div, bf16* out, int64_t row, int ld, int kbase, int P) {
    for (int pw = 0; pw < P; pw += 4) {
        const f32x4 v = pad_slot ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(src + pw);
        bf16x4 hv, lv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = v[e];
            if (arith && !pad_slot) a = (a - shift) / div;
            split_bf16_at<PLANES>(a, hv, lv, e);
        }
        store_operand_split<PLANES>(out, row, ld, kbase + pw, hv, lv);
    }
}

// Item `rem` = (channel, patch row) of token `tau` of sample b -> operand row `row`; item 0 also zeroes the row's K padding (K = C*P*P up to ld)
template <int PLANES>
__device__ __forceinline__ void patch_gather_item(const PatchGatherParams& p, int b, int64_t row, int rem, int tau) {
    const int c = rem / p.P, ph = rem - c * p.P;
    const bool pad_slot = tau >= p.Nt;
    const int tt = pad_slot ? 0 : tau;
    const int gw = p.W / p.P;
    const int n = (p.H / p.P) * gw;
    const int t = tt / n, hw = tt - t * n;
    const int hy = hw / gw, wx = hw - hy * gw;
    const float* src = p.x + b * p.sb + c * p.sc + t * p.st + (int64_t)(hy * p.P + ph) * p.W + wx * p.P;
    float mean, stdv;
    imagenet_mean_std(c, mean, stdv);
    gather_item<PLANES>(src, pad_slot, p.normalize != 0, mean, stdv, p.out, row, p.ld, c * p.P * p.P + ph * p.P, p.P);
    if (rem == 0) zero_operand_tail<PLANES>(p.out, row, p.ld, p.C * p.P * p.P);
}

template <int PLANES>
__global__ __launch_bounds__(256) void patch_gather_kernel(const PatchGatherParams p) {
    const int per_row = p.C * p.P;
    const int64_t total = (int64_t)p.B * p.n_rows * per_row;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int row = (int)(gid / per_row);
    const int rem = (int)(gid - (int64_t)row * per_row);
    const int b = row / p.n_rows, i = row - b * p.n_rows;
    patch_gather_item<PLANES>(p, b, row, rem, p.perm[(size_t)b * (p.perm_stride ? p.perm_stride : p.Nt) + i]);
}

int launch_patch_gather(const PatchGatherParams& p, int planes, hipStream_t stream) {
    CWM_REQUIRE(p.P % 4 == 0 && p.W % 4 == 0, "patch_gather: patch size and width must be multiples of 4");
    CWM_REQUIRE(p.C == 3 || !p.normalize, "patch_gather: imagenet normalisation needs 3 channels");
    CWM_REQUIRE(p.ld >= p.C * p.P * p.P && p.ld % 4 == 0, "patch_gather: bad ld");
    const int64_t total = (int64_t)p.B * p.n_rows * p.C * p.P;
    const int blocks = (int)((total + 255) / 256);
    dispatch_int<2, 1>(planes == 1 ? 1 : 2, [&](auto pl) { hipLaunchKernelGGL(patch_gather_kernel<pl.value>, dim3(blocks), dim3(256), 0, stream, p); });
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Flow + RGB tubelet gather of the flow -> IMU predictor: `FlowBackRGB01` (preprocessor.py:208-277, 356) followed by the
// Conv3d patch embed's im2col, for the visible tokens only.  The reference concatenates
//     [fwd / (W/2, H/2), bwd / (W/2, H/2), imagenet_normalize(frame 1)]
// into a [B,7,1,H,W] tensor and embeds it; here the 7 channels are read from their three sources directly.
// One thread per (row, c, ph) as patch_gather_kernel: P contiguous pixels as float4 loads, P contiguous bf16 stores.
// ---------------------------------------------------------------------------------------------
template <int PLANES>
__global__ __launch_bounds__(256) void flow_rgb_gather_kernel(const FlowRgbGatherParams p) {
    constexpr int C = 7;
    const int per_row = C * p.P;
    const int64_t total = (int64_t)p.B * p.n_rows * per_row;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int row = (int)(gid / per_row);
    const int rem = (int)(gid - (int64_t)row * per_row);
    const int c = rem / p.P, ph = rem - c * p.P;
    const int b = row / p.n_rows, i = row - b * p.n_rows;
    const int tau = p.perm[(size_t)b * p.perm_stride + i];
    const bool pad_slot = tau >= p.Nt;
    const int gw = p.W / p.P;
    const int hy = pad_slot ? 0 : tau / gw, wx = pad_slot ? 0 : tau - (tau / gw) * gw;
    const int64_t pix = (int64_t)(hy * p.P + ph) * p.W + wx * p.P;
    const float* src;
    float div = 1.f, shift = 0.f;
    if (c < 4) {  // flow / (size / 2), size = (W, H) per (x, y) channel (_normalize_flow, preprocessor.py:254-266)
        src = (c < 2 ? p.fwd + b * p.f_sb + (c & 1) * p.f_sc : p.bwd + b * p.b_sb + (c & 1) * p.b_sc) + pix;
        div = 0.5f * (float)((c & 1) ? p.H : p.W);
    } else {
        src = p.x + b * p.sb + (c - 4) * p.sc + pix;
        if (p.normalize) imagenet_mean_std(c - 4, shift, div);
    }
    gather_item<PLANES>(src, pad_slot, true, shift, div, p.out, row, p.ld, c * p.P * p.P + ph * p.P, p.P);
    if (rem == 0) zero_operand_tail<PLANES>(p.out, row, p.ld, C * p.P * p.P);
}

int launch_flow_rgb_gather(const FlowRgbGatherParams& p, int planes, hipStream_t stream) {
    CWM_REQUIRE(p.P % 4 == 0 && p.W % 4 == 0 && p.H % p.P == 0 && p.W % p.P == 0, "flow_rgb_gather: patch size and width must be multiples of 4");
    CWM_REQUIRE(p.ld >= 7 * p.P * p.P && p.ld % 4 == 0, "flow_rgb_gather: bad ld");
    CWM_REQUIRE(p.perm_stride >= p.n_rows && p.Nt == (p.H / p.P) * (p.W / p.P), "flow_rgb_gather: bad token counts");
    const float* ptrs[3] = {p.fwd, p.bwd, p.x};
    const int64_t strides[6] = {p.f_sb, p.f_sc, p.b_sb, p.b_sc, p.sb, p.sc};
    for (const float* q : ptrs) CWM_REQUIRE(q && ((uintptr_t)q & 15) == 0, "flow_rgb_gather: flow and frame pointers must be 16-byte aligned");
    for (int64_t st : strides) CWM_REQUIRE(st % 4 == 0, "flow_rgb_gather: batch / channel strides must be multiples of 4 elements");
    const int64_t total = (int64_t)p.B * p.n_rows * 7 * p.P;
    const int blocks = (int)((total + 255) / 256);
    if (blocks == 0) return 0;
    dispatch_int<2, 1>(planes == 1 ? 1 : 2, [&](auto pl) { hipLaunchKernelGGL(flow_rgb_gather_kernel<pl.value>, dim3(blocks), dim3(256), 0, stream, p); });
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// The index prologue of a forward in ONE launch (round 5): mask -> permutation (visible tokens ascending, then masked ascending:
// vmae.py:167, :555-557), its inverse `rank` (what the un-embed scatter reads, prediction.py:252-259), the per-row check of the visible
// count (the reference's reshape failure at vmae.py:167) and the patch gather above.  Until round 4 these were four dependent launches
// (memset of the error word, mask_to_perm, patch_gather, and perm_to_rank before the un-embed) of 4 - 12 us each with the platform's ~6 us
// between dependent kernels: ~25 us of the 1.86-ms batch-1 forward.  grid = (workgroups per sample, B).  Every workgroup of a sample
// scans the sample's mask row itself (1.5 - 6 KB from L2, a wave-shuffle prefix sum) into an LDS table {i-th visible token -> token index}
// and gathers its share of the visible rows from it; workgroup 0 of the sample also writes perm / rank / the row check.  Integer-exact.
// ---------------------------------------------------------------------------------------------
template <int PLANES>
__global__ __launch_bounds__(256) void index_gather_kernel(const PatchGatherParams p, const uint8_t* __restrict__ mask, int n_vis, int* __restrict__ perm_out,
                                                           int* __restrict__ rank_out, int* __restrict__ err_rows, int n_vis_min, int* __restrict__ counts) {
    extern __shared__ int vis_tab[];  // [n_rows]
    __shared__ int wave_tot[4];
    const int b = blockIdx.y, t = threadIdx.x;
    const int L = p.perm_stride ? p.perm_stride : p.Nt;  // mask row length (padded predictors: real tokens + pad slots)
    const uint8_t* m = mask + (size_t)b * L;
    // perm / rank of the sample are written by ALL of its workgroups (every one has the whole scan anyway): thread slice t belongs to workgroup t mod nw.
    // Until round 5 workgroup 0 wrote all L entries alone: 25 dependent rounds of scattered 4-byte stores on the critical path of the launch.
    const int nw = min((int)gridDim.x, 256);
    const bool writer = (t % nw) == (int)blockIdx.x;
    int* pr = perm_out + (size_t)b * L;
    int* rk = rank_out ? rank_out + (size_t)b * L : nullptr;
    // Is token i visible?  Rows of whole 16-byte groups: the thread's slice of the mask row -- 16 or 32 consecutive bytes -- comes in with one or two
    // 16-byte loads and STAYS in registers for the second pass (round 6.  Round 5: (L + 255) / 256 = 25 single-byte loads per thread at a 25-byte
    // lane stride, twice; on the long rows of ViT-L/4 -- L = 6272 -- that scan, repeated by each of the sample's ~150 workgroups, was most of the
    // launch: 27 - 34 us for 10 MB, now 20 - 23.)  Other rows (test-sized grids): the byte loop, the mask read twice.
    const bool vec = (L & 15) == 0 && L <= 256 * 32 && ((uintptr_t)mask & 15) == 0;
    const int per = !vec ? (L + 255) / 256 : L <= 256 * 16 ? 16 : 32;
    const int lo = min(t * per, L), hi = min(lo + per, L);
    u32x4 w0 = u32x4{0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u}, w1 = w0;  // (past the row: "masked", never counted)
    int c = 0;
    if (vec) {
        if (lo < L) w0 = *reinterpret_cast<const u32x4*>(m + lo);
        if (per == 32 && lo + 16 < L) w1 = *reinterpret_cast<const u32x4*>(m + lo + 16);
        auto zero_bytes = [](unsigned x) {  // number of bytes of x that are 0 (any non-zero byte = masked, as `m[i] == 0` reads it)
            const unsigned y = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
            return __popc(~(y | x | 0x7F7F7F7Fu));
        };
#pragma unroll
        for (int q = 0; q < 4; ++q) c += zero_bytes(w0[q]) + zero_bytes(w1[q]);
    } else {
        for (int i = lo; i < hi; ++i) c += (m[i] == 0);
    }
    int total_vis;
    int v = block_exclusive_scan256(c, wave_tot, total_vis);
    auto emit = [&](int i, bool visible) {
        if (visible) {
            if (v < p.n_rows) vis_tab[v] = i;
            if (writer) {
                pr[v] = i;
                if (rk) rk[i] = v;
            }
            ++v;
        } else if (writer) {
            const int pos = total_vis + (i - v);
            pr[pos] = i;
            if (rk) rk[i] = pos;
        }
    };
    if (vec) {
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            if (k < hi - lo) {
                const unsigned word = k < 16 ? w0[(k >> 2) & 3] : w1[(k >> 2) & 3];
                emit(lo + k, ((word >> (8 * (k & 3))) & 0xFFu) == 0);
            }
        }
    } else {
        for (int i = lo; i < hi; ++i) emit(i, m[i] == 0);
    }
    // (ragged batches, n_vis_min > 0: n_vis is the cap; the rows of a sample behind its count are gathered as pad slots -- zeros -- and are padding
    // all through the encoder)
    if (blockIdx.x == 0 && t == 0) {
        err_rows[b] = (n_vis_min > 0 ? (total_vis < n_vis_min || total_vis > n_vis) : total_vis != n_vis) ? 1 : 0;
        if (counts) counts[b] = total_vis;
    }
    __syncthreads();

    const int per_row = p.C * p.P;
    const int total = p.n_rows * per_row;
    for (int gid = blockIdx.x * 256 + t; gid < total; gid += gridDim.x * 256) {
        const int i = gid / per_row;
        // (a row with too few visible tokens is reported through err_rows: its missing rows read nothing)
        patch_gather_item<PLANES>(p, b, (int64_t)b * p.n_rows + i, gid - i * per_row, i < total_vis ? vis_tab[i] : p.Nt);
    }
}

int launch_index_gather(const PatchGatherParams& p, const uint8_t* mask, int n_vis, int* perm, int* rank, int* err_rows, int planes, hipStream_t stream,
                        int n_vis_min, int* counts) {
    CWM_REQUIRE(n_vis_min == 0 || (n_vis_min > 0 && n_vis_min <= n_vis && counts), "index_gather: ragged rows need 0 < n_vis_min <= n_vis and a count array");
    CWM_REQUIRE(p.P % 4 == 0 && p.W % 4 == 0, "index_gather: patch size and width must be multiples of 4");
    CWM_REQUIRE(p.C == 3 || !p.normalize, "index_gather: imagenet normalisation needs 3 channels");
    CWM_REQUIRE(p.ld >= p.C * p.P * p.P && p.ld % 4 == 0, "index_gather: bad ld");
    CWM_REQUIRE(mask && perm && err_rows && p.n_rows > 0 && p.n_rows <= 12000, "index_gather: bad argument (rows per sample: %d)", p.n_rows);
    // one gather item per thread.  (Capping the grid at one resident round of the chip -- every workgroup pays the mask scan once -- and letting the
    // grid-strided loop run twice measured SLOWER at batch 32: 28.6 against 22.2 us; the scan hides under the other workgroups' loads.)
    const int per_sample = (p.n_rows * p.C * p.P + 255) / 256;
    const dim3 grid((unsigned)per_sample, (unsigned)p.B);
    const size_t smem = (size_t)p.n_rows * sizeof(int);
    dispatch_int<2, 1>(planes == 1 ? 1 : 2, [&](auto pl) {
        hipLaunchKernelGGL(index_gather_kernel<pl.value>, grid, dim3(256), smem, stream, p, mask, n_vis, perm, rank, err_rows, n_vis_min, counts);
    });
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// decoder input, masked half: x_full[b][n_vis + j] = mask_token + pos[perm[b][n_vis + j]]
// (vmae.py:556-557).  The visible half is written by the encoder_to_decoder GEMM epilogue.
// ---------------------------------------------------------------------------------------------
// EIGHT rows per thread, all loads (perm -> positional row) issued
// before the first store.  One row per thread ran as ~4.6 rounds of short-lived waves, each a dependent perm -> pos -> store
// chain: 2.9 TB/s of stores (13.1 us for 38 MB, ViT-B/8 batch 32); with independent chains per thread the launch is one round.
__global__ __launch_bounds__(256) void fill_mask_tokens4_kernel(float* x_full, const float* mask_token, const float* pos, const int* perm, int Nt,
                                                                 int n_vis, int D, int64_t rows, int64_t rows_q) {
    const int d4 = D / 4;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= rows_q * d4) return;
    const int64_t r0 = gid / d4;
    const int c4 = (int)(gid - r0 * d4);
    const int nm = Nt - n_vis;
    const float4 mt = *reinterpret_cast<const float4*>(mask_token + c4 * 4);
    constexpr int R = 8;  // rows per thread: the whole launch is resident at once (no second, nearly empty round of waves)
    size_t orow[R];
    int tau[R];
    bool live[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int64_t row = r0 + i * rows_q;
        live[i] = row < rows;
        const int64_t rr = live[i] ? row : 0;
        const int b = (int)(rr / nm), j = (int)(rr - (int64_t)b * nm);
        orow[i] = (size_t)b * Nt + n_vis + j;
        tau[i] = perm[orow[i]];
    }
    float4 pe[R];
#pragma unroll
    for (int i = 0; i < R; ++i) pe[i] = *reinterpret_cast<const float4*>(pos + (size_t)tau[i] * D + c4 * 4);
#pragma unroll
    for (int i = 0; i < R; ++i)
        if (live[i]) *reinterpret_cast<float4*>(x_full + orow[i] * D + c4 * 4) = make_float4(mt.x + pe[i].x, mt.y + pe[i].y, mt.z + pe[i].z, mt.w + pe[i].w);
}

// Ragged batches: sample b has counts[b] (>= n_vis_min) visible tokens, so its mask tokens are rows [counts[b], Nt).  The encoder_to_decoder GEMM
// before this launch wrote rows [0, cap) of every sample, padding rows [counts[b], cap) included: those are overwritten here.  One thread per four
// columns of a row of [n_vis_min, Nt); rows below the sample's count are left alone.
__global__ __launch_bounds__(256) void fill_mask_tokens_ragged_kernel(float* x_full, const float* mask_token, const float* pos, const int* perm,
                                                                      const int* counts, int Nt, int n_vis_min, int D, int64_t total) {
    const int d4 = D / 4;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int64_t row = gid / d4;
    const int c4 = (int)(gid - row * d4);
    const int nm = Nt - n_vis_min;
    const int b = (int)(row / nm), j = n_vis_min + (int)(row - (int64_t)b * nm);
    if (j < counts[b]) return;
    const size_t orow = (size_t)b * Nt + j;
    const float4 mt = *reinterpret_cast<const float4*>(mask_token + c4 * 4);
    const float4 pe = *reinterpret_cast<const float4*>(pos + (size_t)perm[orow] * D + c4 * 4);
    *reinterpret_cast<float4*>(x_full + orow * D + c4 * 4) = make_float4(mt.x + pe.x, mt.y + pe.y, mt.z + pe.z, mt.w + pe.w);
}

int launch_fill_mask_tokens(float* x_full, const float* mask_token, const float* pos, const int* perm, int B, int Nt, int n_vis, int D, hipStream_t stream,
                            const int* counts, int n_vis_min) {
    if (counts || n_vis_min > 0) {
        CWM_REQUIRE(D % 4 == 0 && counts && n_vis_min > 0 && n_vis_min <= Nt, "fill_mask_tokens (ragged): bad argument");
        const int64_t total = (int64_t)B * (Nt - n_vis_min) * (D / 4);
        if (total == 0) return 0;
        hipLaunchKernelGGL(fill_mask_tokens_ragged_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x_full, mask_token, pos, perm, counts, Nt,
                           n_vis_min, D, total);
        CWM_HIP_CHECK(hipGetLastError());
        return 0;
    }
    CWM_REQUIRE(D % 4 == 0, "fill_mask_tokens: D must be a multiple of 4");
    const int64_t rows = (int64_t)B * (Nt - n_vis), rows_q = (rows + 7) / 8;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(fill_mask_tokens4_kernel, dim3((unsigned)((rows_q * (D / 4) + 255) / 256)), dim3(256), 0, stream, x_full, mask_token, pos, perm, Nt,
                       n_vis, D, rows, rows_q);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// decoder block 0, masked half of Q / K / V: LN1 and the Q/K/V projection of mask_token + pos[p] depend on the weights and p only, so they come from a
// table of Nt rows (engine.hip Engine::dec0_table) instead of the GEMM.  A (sample, masked row) is `cpr` = 3 * planes * H * 8 chunks of 16 bytes: chunk c =
// ((which * planes + pl) * H + h) * 8 + e is elements 8 e .. 8 e + 7 of head h in plane pl of Q / K / V.  FOUR rows per thread, the permutation entries and
// then the table chunks all requested before the first store (as fill_mask_tokens4_kernel); consecutive lanes copy consecutive chunks, whole 128-byte head rows.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dec0_gather_kernel(const bf16* tab, const int* perm, bf16* q, bf16* k, bf16* v, int64_t qk_plane, int Nt, int n_vis, int H,
                                                          int planes, int64_t rows, int64_t rows_q) {
    const int cpr = 3 * planes * H * 8;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= rows_q * cpr) return;
    const int64_t r0 = gid / cpr;
    const int c = (int)(gid - r0 * cpr);
    const int e = c & 7, h = (c >> 3) % H, wp = (c >> 3) / H;  // wp = which * planes + pl
    const int which = wp / planes, pl = wp - which * planes;
    const int nm = Nt - n_vis;
    const bf16* src = tab + ((size_t)wp * H + h) * Nt * 64 + e * 8;
    bf16* dst = (which == 0 ? q : which == 1 ? k : v) + (size_t)pl * qk_plane + e * 8;
    constexpr int R = 4;
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    size_t orow[R];
    int tau[R];
    bool live[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int64_t row = r0 + i * rows_q;
        live[i] = row < rows;
        const int64_t rr = live[i] ? row : 0;
        const int b = (int)(rr / nm), j = n_vis + (int)(rr - (int64_t)b * nm);
        orow[i] = ((size_t)b * H + h) * Nt + j;
        tau[i] = perm[(size_t)b * Nt + j];
    }
    u32x4 val[R];
#pragma unroll
    for (int i = 0; i < R; ++i) val[i] = *reinterpret_cast<const u32x4*>(src + (size_t)min(max(tau[i], 0), Nt - 1) * 64);
#pragma unroll
    for (int i = 0; i < R; ++i)
        if (live[i]) *reinterpret_cast<u32x4*>(dst + orow[i] * 64) = val[i];
}

int launch_dec0_gather(const bf16* tab, const int* perm, bf16* q, bf16* k, bf16* v, int64_t qk_plane, int B, int Nt, int n_vis, int H, int planes, hipStream_t stream) {
    CWM_REQUIRE(tab && perm && q && k && v && B > 0 && H > 0 && n_vis >= 0 && n_vis <= Nt && (planes == 1 || planes == 2) && qk_plane % 8 == 0,
                "dec0_gather: bad argument");
    const int64_t rows = (int64_t)B * (Nt - n_vis), rows_q = (rows + 3) / 4;
    if (rows == 0) return 0;
    const int64_t total = rows_q * 3 * planes * H * 8;
    hipLaunchKernelGGL(dec0_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, tab, perm, q, k, v, qk_plane, Nt, n_vis, H, planes, rows, rows_q);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void iota_kernel(int* perm, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) perm[i] = i;
}

int launch_iota(int* perm, int n, hipStream_t stream) {
    CWM_REQUIRE(perm && n > 0, "iota: bad argument");
    hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, perm, n);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Patch un-embed scatter.  Reference: `pred_patches_to_video` (prediction.py:245-259) with
// `Patchify` (patches.py:74,98-102): feature index f = (ph*P + pw)*C + c; visible patches take the
// RAW (un-normalised) wrapper input.  One thread per 4 horizontally adjacent output pixels.
// ---------------------------------------------------------------------------------------------
// (the generic kernel below is the form for everything unembed3_kernel refuses: it moves Float4A4, common.h)
__global__ __launch_bounds__(256) void unembed_kernel(const UnembedParams p) {
    const int w4 = p.W / 4;
    const int64_t total = (int64_t)p.B * p.T * p.C * p.H * w4;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    int64_t r = gid;
    const int x4 = (int)(r % w4); r /= w4;
    const int y = (int)(r % p.H); r /= p.H;
    const int c = (int)(r % p.C); r /= p.C;
    const int t = (int)(r % p.T);
    const int b = (int)(r / p.T);
    const int x0 = x4 * 4;
    const int gw = p.W / p.P;
    const int n = (p.H / p.P) * gw;
    const int Nt = p.T * n;
    const int tau = t * n + (y / p.P) * gw + (x0 / p.P);
    Float4A4 o;
    if (p.mask[(size_t)b * Nt + tau]) {
        // (a row with fewer visible tokens than n_vis -- reported through the prologue's err, but this launch is already queued by then -- has masked tokens
        // of rank < n_vis: they read y row 0 instead of rows in front of the sample's, which for sample 0 lie in front of the buffer)
        const int j = max(p.rank[(size_t)b * Nt + tau] - p.n_vis, 0);
        const float* yp = p.y + ((size_t)b * p.Nm + j) * (p.P * p.P * p.C) + ((y % p.P) * p.P + (x0 % p.P)) * p.C + c;
        o = Float4A4{{yp[0], yp[p.C], yp[2 * p.C], yp[3 * p.C]}};
    } else {
        o = *reinterpret_cast<const Float4A4*>(p.x + b * p.sb + t * p.st + c * p.sc + (int64_t)y * p.W + x0);
    }
    *reinterpret_cast<Float4A4*>(p.out + ((((size_t)b * p.T + t) * p.C + c) * p.H + y) * p.W + x0) = o;
}

// C == 3 (every predictor of the path): one thread per 4 horizontally adjacent pixels of ALL THREE channels.  A masked patch row is
// 4 px x 3 channels = 12 consecutive floats of the token (feature order (ph pw c), c fastest): three aligned 16-byte loads, transposed
// in registers, three 16-byte stores (one per channel plane).  The one-channel form above reads the same 48 bytes from three threads
// of three different waves with 4-byte loads at a 12-byte stride: 3.0 TB/s (25.7 us for 77 MB at ViT-B/8 batch 32).
__global__ __launch_bounds__(256) void unembed3_kernel(const UnembedParams p) {
    const int w4 = p.W / 4, hh = p.H / 2;  // two image rows (y, y + H/2) per thread: six independent 16-byte loads in flight
    const int64_t total = (int64_t)p.B * p.T * hh * w4;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    int64_t r = gid;
    const int x4 = (int)(r % w4); r /= w4;
    const int y0 = (int)(r % hh); r /= hh;
    const int t = (int)(r % p.T);
    const int b = (int)(r / p.T);
    const int x0 = x4 * 4;
    const int gw = p.W / p.P;
    const int n = (p.H / p.P) * gw;
    const int Nt = p.T * n;
    float4 o[2][3];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int y = y0 + k * hh;
        const int tau = t * n + (y / p.P) * gw + (x0 / p.P);
        if (p.mask[(size_t)b * Nt + tau]) {
            const int j = max(p.rank[(size_t)b * Nt + tau] - p.n_vis, 0);  // (< 0: a row that err reports -- see unembed_kernel)
            const float4* yp = reinterpret_cast<const float4*>(p.y + ((size_t)b * p.Nm + j) * (p.P * p.P * 3) + ((y % p.P) * p.P + (x0 % p.P)) * 3);
            const float4 a = yp[0], bb = yp[1], c = yp[2];  // px0 (r g b) px1 (r | g b) px2 (r g | b) px3 (r g b)
            o[k][0] = make_float4(a.x, a.w, bb.z, c.y);
            o[k][1] = make_float4(a.y, bb.x, bb.w, c.z);
            o[k][2] = make_float4(a.z, bb.y, c.x, c.w);
        } else {
            const float* src = p.x + b * p.sb + t * p.st + (int64_t)y * p.W + x0;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[k][c] = *reinterpret_cast<const float4*>(src + c * p.sc);
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float* dst = p.out + (((size_t)b * p.T + t) * 3 * p.H + y0 + k * hh) * p.W + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {  // (the predicted video is the call's result: written once, streaming stores)
            const f32x4 v = f32x4{o[k][c].x, o[k][c].y, o[k][c].z, o[k][c].w};
            __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(dst + (size_t)c * p.H * p.W));
        }
    }
}

int launch_unembed(const UnembedParams& p, hipStream_t stream) {
    CWM_REQUIRE(p.P % 4 == 0 && p.W % 4 == 0, "unembed: patch size and width must be multiples of 4");
    if (p.C == 3 && p.H % 2 == 0 && (((uintptr_t)p.y | (uintptr_t)p.out | (uintptr_t)p.x) & 15) == 0 && (p.sc % 4 == 0) && (p.sb % 4 == 0) && (p.st % 4 == 0)) {
        const int64_t total3 = (int64_t)p.B * p.T * (p.H / 2) * (p.W / 4);
        hipLaunchKernelGGL(unembed3_kernel, dim3((unsigned)((total3 + 255) / 256)), dim3(256), 0, stream, p);
        CWM_HIP_CHECK(hipGetLastError());
        return 0;
    }
    const int64_t total = (int64_t)p.B * p.T * p.C * p.H * (p.W / 4);
    hipLaunchKernelGGL(unembed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Motion-counterfactual prompt construction, vectorised over all B*S prompts.
// Reference: the per-sample Python loop of `create_motion_counterfactuals` (segmentation.py:324-338)
// calling `PatchPerturbation.forward` + `ShiftPatchesAndMask.perturb` (perturbation.py:99-113,
// 245-289) on a static movie (`make_static_movie`, prediction.py:731-739).  For prompt i = b*S+s:
//   frame `frame`: the destination patch (pi,pj) of every active patch (pi-dy, pj-dx) receives the
//   active patch's pixels; everything else is the (static) input.  Pure copies: bit-exact.
//   mask_out = (active ? masks : 1) & (shifted perturbation mask), destinations out of frame vanish.
// fix_passive: 0 = the movie as given; 1 = every frame := frame 0 (`make_static_movie`); 2 = `MakeStatic` (perturbation.py:120-145)
// applied before the shift: only the patches that `masks` leaves visible are replaced by their frame-0 pixels.
// ---------------------------------------------------------------------------------------------
// One thread = 4 horizontally adjacent pixels of FOUR consecutive image rows (y = 4 yq .. 4 yq + 3: one patch row block, P is a multiple of 4), so the
// source decision -- which patch, which frame -- is taken once for four independent 16-byte loads and stores.  (Until round 5: one 16-byte store per thread
// behind six integer divisions and a dependent mask byte load; profiles/r6_bench_prompt_build*.json.)  The prompts are written once and read once by the
// predictor's gather: streaming (non-temporal) stores.
__global__ __launch_bounds__(256) void shift_prompts_x_kernel(const ShiftPromptParams p) {
    const int w4 = p.W / 4, h4 = p.H / 4;
    const int64_t total = (int64_t)p.B * p.S * p.T * p.C * h4 * w4;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    int64_t r = gid;
    const int x4 = (int)(r % w4); r /= w4;
    const int yq = (int)(r % h4); r /= h4;
    const int c = (int)(r % p.C); r /= p.C;
    const int t = (int)(r % p.T);
    const int i = (int)(r / p.T);
    const int b = i / p.S;
    const int x0 = x4 * 4, y = yq * 4;
    int ft = p.fix_passive == 1 ? 0 : t;
    int sy = y, sx = x0;
    const int gw = p.W / p.P, gh = p.H / p.P, n = gh * gw;
    if (t == p.frame) {
        const int dy = p.shifts[2 * i], dx = p.shifts[2 * i + 1];
        const int pi = y / p.P - dy, pj = x0 / p.P - dx;
        if (pi >= 0 && pi < gh && pj >= 0 && pj < gw && p.active[(size_t)i * p.T * n + (size_t)p.frame * n + pi * gw + pj] == 0) {
            sy = y - dy * p.P;
            sx = x0 - dx * p.P;
        }
    }
    if (p.fix_passive == 2) {  // MakeStatic (perturbation.py:120-145): the patches `masks` leaves visible take their frame-0 pixels
        if (p.masks[(size_t)i * p.T * n + (size_t)t * n + (sy / p.P) * gw + sx / p.P] == 0) ft = 0;
    }
    const float* src = p.x + ((((size_t)b * p.T + ft) * p.C + c) * p.H + sy) * p.W + sx;
    float* dst = p.x_out + ((((size_t)i * p.T + t) * p.C + c) * p.H + y) * p.W + x0;
    f32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const f32x4*>(src + (size_t)k * p.W);
#pragma unroll
    for (int k = 0; k < 4; ++k) __builtin_nontemporal_store(v[k], reinterpret_cast<f32x4*>(dst + (size_t)k * p.W));
}

__global__ __launch_bounds__(256) void shift_prompts_mask_kernel(const ShiftPromptParams p) {
    const int gw = p.W / p.P, gh = p.H / p.P, n = gh * gw, Nt = p.T * n;
    const int64_t total = (int64_t)p.B * p.S * Nt;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int i = (int)(gid / Nt), tau = (int)(gid - (int64_t)i * Nt);
    const int t = tau / n, hw = tau - t * n;
    const uint8_t act = p.active[gid];
    const uint8_t m1 = act ? p.masks[gid] : 1;
    uint8_t mp = act;
    if (t == p.frame) {
        const int dy = p.shifts[2 * i], dx = p.shifts[2 * i + 1];
        const int pi = hw / gw - dy, pj = hw % gw - dx;
        mp = (pi >= 0 && pi < gh && pj >= 0 && pj < gw) ? p.active[(size_t)i * Nt + (size_t)t * n + pi * gw + pj] : 1;
    }
    p.mask_out[gid] = (m1 && mp) ? 1 : 0;
}

// The prompt table of the counterfactual batch (BASELINE configs[3]; interface.py:370-377: one active patch of frame `frame` per prompt, moved by (dy, dx)
// patches, nothing passive) -> the dense operands of the kernels above: passive[i] = "frame 0 visible, every later frame masked", active[i] = passive[i] with the
// prompt's patch cleared, shifts[i] = (dy, dx).  One launch instead of the ten tensor operations that built them on rank 0's critical path (dist.py prompt_hooks).
// A table cell outside the grid (h outside [0, gh) or w outside [0, gw)) clears nothing: its linear index h gw + w would name another cell, or another frame.
__global__ __launch_bounds__(256) void prompt_table_expand_kernel(const int* __restrict__ table, int S, int gh, int gw, int T, int frame, uint8_t* __restrict__ active,
                                                                  uint8_t* __restrict__ passive, int* __restrict__ shifts) {
    const int n = gh * gw;
    const int Nt = T * n;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)S * Nt) return;
    const int i = (int)(gid / Nt), tau = (int)(gid - (int64_t)i * Nt);
    const int h = table[4 * i], w = table[4 * i + 1];
    const uint8_t pas = tau >= n ? 1 : 0;
    passive[gid] = pas;
    const bool in_grid = h >= 0 && h < gh && w >= 0 && w < gw;
    active[gid] = (in_grid && tau == frame * n + h * gw + w) ? 0 : pas;
    if (tau < 2) shifts[2 * i + tau] = table[4 * i + 2 + tau];
}

int launch_prompt_table_expand(const int* table, int S, int gh, int gw, int T, int frame, uint8_t* active, uint8_t* passive, int* shifts, hipStream_t stream) {
    const int64_t total = (int64_t)S * T * gh * gw;
    hipLaunchKernelGGL(prompt_table_expand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, table, S, gh, gw, T, frame, active, passive, shifts);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_shift_prompts(const ShiftPromptParams& p, hipStream_t stream) {
    CWM_REQUIRE(p.P % 4 == 0 && p.W % 4 == 0 && p.H % p.P == 0 && p.W % p.P == 0, "shift_prompts: bad patch/image size");
    CWM_REQUIRE(p.frame >= 0 && p.frame < p.T, "shift_prompts: frame out of range");
    CWM_REQUIRE(p.fix_passive >= 0 && p.fix_passive <= 2, "shift_prompts: fix_passive must be 0, 1 or 2");
    CWM_REQUIRE(p.H % 4 == 0, "shift_prompts: the image height must be a multiple of 4");
    const int64_t tx = (int64_t)p.B * p.S * p.T * p.C * (p.H / 4) * (p.W / 4);
    const int64_t tm = (int64_t)p.B * p.S * p.T * (p.H / p.P) * (p.W / p.P);
    // either output may be absent: the sharded loop builds the masks of ALL prompts on rank 0 (the rectangulariser is the one cross-row step) but frames only for
    // the rows a rank predicts (dist.py)
    if (p.x_out) hipLaunchKernelGGL(shift_prompts_x_kernel, dim3((unsigned)((tx + 255) / 256)), dim3(256), 0, stream, p);
    if (p.mask_out) hipLaunchKernelGGL(shift_prompts_mask_kernel, dim3((unsigned)((tm + 255) / 256)), dim3(256), 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Multi-shift prompts: K steps per prompt, step k moving its own set of patches of frame `frame` by its own PIXEL shift (sy_k, sx_k).
// Reference: `MultiShiftPatchesAndMask.forward` (perturbation.py:644-779) = K rounds of `ShiftPatchesAndMask.perturb` in fractional mode
// (:245-289: pad, centre-crop, patchify and blend the whole frame per step, per sample).  Step k leaves a destination patch (pi, pj) holding the
// pixels at (y - sy_k, x - sx_k) of the frame as step k-1 left it whenever the source cell (pi - my_k, pj - mx_k) is one of its points
// (my = sy / P truncated toward zero: the mask moves by whole patches only), zeros where that leaves the image; so an output pixel is found by
// walking the steps BACKWARDS from its own position.  Pure copies and zeros: bit-exact.  Semantics in full: include/cwm_hip.h.
// ---------------------------------------------------------------------------------------------
// Steps k .. 0 for one pixel at (cy, cx), which is inside the image; false once the position has left the image (the pixel is 0).  Every table read is
// behind the grid test, and a step is taken only from a cell inside the grid, which bounds |s| by (grid + 1) P: no overflow whatever the table holds.
__device__ __forceinline__ bool multi_shift_walk(const uint8_t* __restrict__ pts, const int* __restrict__ sh, int k, int Nt, int P, int gh, int gw, int H, int W,
                                                 int& cy, int& cx) {
    for (; k >= 0; --k) {
        const int sy = sh[2 * k], sx = sh[2 * k + 1];
        const int pi = cy / P - sy / P, pj = cx / P - sx / P;  // (C division truncates toward zero: sign(s) (|s| // P))
        if (pi >= 0 && pi < gh && pj >= 0 && pj < gw && pts[(size_t)k * Nt + pi * gw + pj]) {
            cy -= sy;
            cx -= sx;
            if (cy < 0 || cy >= H || cx < 0 || cx >= W) return false;
        }
    }
    return true;
}

// One thread = 4 horizontally adjacent pixels of one image row, all C channels (the walk does not depend on the channel).  The four pixels share ONE walk
// while they sit 4-aligned inside one patch: then they take the same decisions, and a step whose sx is a multiple of 4 keeps them so (16-byte loads).
// The first step that breaks this -- sx not a multiple of 4, or P not a multiple of 4 and the group straddling two patches -- splits the group into four
// walks over the remaining steps and dword loads.  Rows whose sx are all multiples of 4 never split; frames other than `frame` are plain copies.
// Stores are whole 16-byte groups of the output row either way, streaming like the single-shift kernel's.
__global__ __launch_bounds__(256) void multi_shift_prompts_x_kernel(const MultiShiftParams p) {
    const int w4 = p.W / 4;
    const int64_t total = (int64_t)p.B * p.S * p.T * p.H * w4;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    int64_t r = gid;
    const int x0 = (int)(r % w4) * 4; r /= w4;
    const int y = (int)(r % p.H); r /= p.H;
    const int t = (int)(r % p.T);
    const int i = (int)(r / p.T);
    const int b = i / p.S;
    const int ft = p.fix_passive == 1 ? 0 : t;
    const int H = p.H, W = p.W, P = p.P;
    const size_t plane = (size_t)H * W;
    const float* __restrict__ src = p.x + ((size_t)b * p.T + ft) * p.C * plane;
    float* __restrict__ dst = p.x_out + ((size_t)i * p.T + t) * p.C * plane + (size_t)y * W + x0;
    int cy = y, cx = x0, k = -1;
    bool split = false, alive = true;
    const int gw = W / P, gh = H / P, n = gh * gw, Nt = p.T * n;
    const uint8_t* __restrict__ pts = p.points + (size_t)i * p.K * Nt + (size_t)p.frame * n;  // step k of frame `frame` at pts + k Nt
    const int* __restrict__ sh = p.shifts + (size_t)i * p.K * 2;
    if (t == p.frame) {
        for (k = p.K - 1; k >= 0; --k) {
            if (cx % P + 3 >= P) { split = true; break; }  // (P % 4 != 0 only) step k is still to be taken, per pixel
            const int sy = sh[2 * k], sx = sh[2 * k + 1];
            const int pi = cy / P - sy / P, pj = cx / P - sx / P;
            if (pi >= 0 && pi < gh && pj >= 0 && pj < gw && pts[(size_t)k * Nt + pi * gw + pj]) {
                cy -= sy;
                cx -= sx;
                if (sx & 3) { split = true; --k; break; }  // taken by all four, but they are no longer one aligned group
                if (cy < 0 || cy >= H || cx < 0 || cx >= W) { alive = false; break; }  // (W % 4 == 0: all four inside or all four outside)
            }
        }
    }
    if (!split) {
        const float* s = src + (alive ? (size_t)cy * W + cx : 0);
        for (int c0 = 0; c0 < p.C; c0 += 4) {
            f32x4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                v[j] = (alive && c0 + j < p.C) ? *reinterpret_cast<const f32x4*>(s + (size_t)(c0 + j) * plane) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c0 + j < p.C) __builtin_nontemporal_store(v[j], reinterpret_cast<f32x4*>(dst + (size_t)(c0 + j) * plane));
        }
        return;
    }
    int off[4];  // source offset inside a channel plane, -1 = outside the image (constant padding: 0)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int py = cy, px = cx + j;
        const bool ok = py >= 0 && py < H && px >= 0 && px < W && multi_shift_walk(pts, sh, k, Nt, P, gh, gw, H, W, py, px);
        off[j] = ok ? py * W + px : -1;
    }
    for (int c = 0; c < p.C; ++c) {
        const float* s = src + (size_t)c * plane;
        f32x4 v;
        v.x = off[0] >= 0 ? s[off[0]] : 0.f;
        v.y = off[1] >= 0 ? s[off[1]] : 0.f;
        v.z = off[2] >= 0 ? s[off[2]] : 0.f;
        v.w = off[3] >= 0 ? s[off[3]] : 0.f;
        __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(dst + (size_t)c * plane));
    }
}

// mask_out = AND_k step_k; step_k = (M_k | A_k) & shifted_k with base masks, shifted_k without (the reference's `_has_base_mask`, perturbation.py:697-714,
// 774-778), shifted_k = !A_k moved by (my_k, mx_k) patches in frame `frame` (cells whose source is outside the grid are masked), !A_k elsewhere.
__global__ __launch_bounds__(256) void multi_shift_prompts_mask_kernel(const MultiShiftParams p) {
    const int gw = p.W / p.P, gh = p.H / p.P, n = gh * gw, Nt = p.T * n;
    const int64_t total = (int64_t)p.B * p.S * Nt;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int i = (int)(gid / Nt), tau = (int)(gid - (int64_t)i * Nt);
    const int t = tau / n, hw = tau - t * n;
    const uint8_t* __restrict__ pts = p.points + (size_t)i * p.K * Nt;
    const int* __restrict__ sh = p.shifts + (size_t)i * p.K * 2;
    uint8_t out = 1;
    for (int k = 0; k < p.K; ++k) {
        const uint8_t a = pts[(size_t)k * Nt + tau] != 0;
        uint8_t shifted = !a;
        if (t == p.frame) {
            const int pi = hw / gw - sh[2 * k] / p.P, pj = hw % gw - sh[2 * k + 1] / p.P;
            shifted = (pi >= 0 && pi < gh && pj >= 0 && pj < gw) ? (pts[(size_t)k * Nt + (size_t)t * n + pi * gw + pj] == 0) : 1;
        }
        uint8_t step = shifted;
        if (p.masks) {
            const uint8_t m = p.masks[((size_t)i * p.mask_steps + (p.mask_steps == 1 ? 0 : k)) * Nt + tau] != 0;
            step = (m | a) & shifted;
        }
        out &= step;
    }
    p.mask_out[gid] = out;
}

int launch_multi_shift_prompts(const MultiShiftParams& p, hipStream_t stream) {
    CWM_REQUIRE(p.K >= 1 && p.K <= kMultiShiftMaxSteps, "multi_shift_prompts: K=%d steps, need 1 <= K <= %d", p.K, kMultiShiftMaxSteps);
    CWM_REQUIRE(p.P > 0 && p.W % 4 == 0 && p.H % p.P == 0 && p.W % p.P == 0,
                "multi_shift_prompts: bad patch/image size (H=%d W=%d P=%d: W must be a multiple of 4, H and W multiples of P)", p.H, p.W, p.P);
    CWM_REQUIRE(p.frame >= 0 && p.frame < p.T, "multi_shift_prompts: frame out of range");
    CWM_REQUIRE(p.fix_passive == 0 || p.fix_passive == 1, "multi_shift_prompts: fix_passive must be 0 or 1");
    CWM_REQUIRE(!p.masks || p.mask_steps == 1 || p.mask_steps == p.K, "multi_shift_prompts: mask_steps=%d, need 1 or K=%d", p.mask_steps, p.K);
    CWM_REQUIRE((((uintptr_t)p.x | (uintptr_t)p.x_out) & 15) == 0, "multi_shift_prompts: the frames must be 16-byte aligned");
    const int64_t tx = (int64_t)p.B * p.S * p.T * p.H * (p.W / 4);
    const int64_t tm = (int64_t)p.B * p.S * p.T * (p.H / p.P) * (p.W / p.P);
    if (p.x_out) hipLaunchKernelGGL(multi_shift_prompts_x_kernel, dim3((unsigned)((tx + 255) / 256)), dim3(256), 0, stream, p);
    if (p.mask_out) hipLaunchKernelGGL(multi_shift_prompts_mask_kernel, dim3((unsigned)((tm + 255) / 256)), dim3(256), 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// `RectangularizeMasks` on device masks (masking.py:90-132) without reading the masks back: the host needs only the per-row COUNTS to decide
// the target and to draw the reference's `torch.randperm(#candidates)[:surplus]` per changed row (the draws depend on the counts alone); the
// picks -- "the k-th masked (or visible) token of row r in ascending order" -- come back as a small table and are applied here, every pick of a
// row against the row as it was BEFORE any of them (the reference indexes one `torch.where` list per row).  Integer-exact.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_row_counts_kernel(const uint8_t* __restrict__ mask, int Nt, int* __restrict__ counts) {
    __shared__ int red[4];
    const uint8_t* m = mask + (size_t)blockIdx.x * Nt;
    int c = 0;
    for (int i = threadIdx.x; i < Nt; i += 256) c += (m[i] != 0);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// table: [R | rows[R] | offsets[R + 1] | to_value[R] | picks[offsets[R]]]; one workgroup per changed row.  A table row whose index is outside [0, B) names no
// row of the mask: its workgroup leaves (the whole workgroup, before the first barrier) and the other rows get their picks.
constexpr int kFlipMaxTokens = 16384;
__global__ __launch_bounds__(256) void mask_flip_picks_kernel(uint8_t* __restrict__ mask, int B, int Nt, const int* __restrict__ table) {
    __shared__ unsigned bits[kFlipMaxTokens / 32];
    __shared__ int wave_tot[4];
    const int R = table[0], r = blockIdx.x, t = threadIdx.x;
    const int row = table[1 + r], p0 = table[1 + R + r], p1 = table[1 + R + r + 1], to = table[2 + 2 * R + r];
    const int* picks = table + 2 + 3 * R;
    if (row < 0 || row >= B) return;
    uint8_t* m = mask + (size_t)row * Nt;
    for (int i = t; i < (Nt + 31) / 32; i += 256) bits[i] = 0u;
    __syncthreads();
    for (int q = p0 + t; q < p1; q += 256) {
        const int k = picks[q];
        if (k >= 0 && k < Nt) atomicOr(&bits[k >> 5], 1u << (k & 31));
    }
    const int per = (Nt + 255) / 256;
    const int lo = min(t * per, Nt), hi = min(lo + per, Nt);
    int c = 0;
    for (int i = lo; i < hi; ++i) c += ((m[i] != 0) != (to != 0));  // candidates: tokens whose state is not `to` yet
    int total;
    int v = block_exclusive_scan256(c, wave_tot, total);  // (its barrier also completes the bitmap)
    for (int i = lo; i < hi; ++i) {
        if ((m[i] != 0) != (to != 0)) {
            if (bits[v >> 5] & (1u << (v & 31))) m[i] = (uint8_t)(to ? 1 : 0);
            ++v;
        }
    }
}

int launch_mask_row_counts(const uint8_t* mask, int B, int Nt, int* counts, hipStream_t stream) {
    hipLaunchKernelGGL(mask_row_counts_kernel, dim3((unsigned)B), dim3(256), 0, stream, mask, Nt, counts);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_mask_flip_picks(uint8_t* mask, int B, int Nt, const int* table, int n_rows, hipStream_t stream) {
    CWM_REQUIRE(Nt <= kFlipMaxTokens, "mask_flip_picks: rows of %d tokens exceed the %d-token pick bitmap", Nt, kFlipMaxTokens);
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(mask_flip_picks_kernel, dim3((unsigned)n_rows), dim3(256), 0, stream, mask, B, Nt, table);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
__global__ void split_bf16_kernel(const float* x, int64_t n, bf16* hi, bf16* lo) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bf16 h, l;
    split_bf16(x[i], h, l);
    hi[i] = h;
    if (lo) lo[i] = l;
}

int launch_split_bf16(const float* x, int64_t n, bf16* hi, bf16* lo, hipStream_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, n, hi, lo);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace cwm
