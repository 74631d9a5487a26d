// Device-side helpers shared by the five attention translation units (attention.hip, attention_tail.h, attention_pipe.hip and the
// cross / context attention of conj_attention.hip): workgroup placement, LDS tile images, the hardware transpose read, and the
// building blocks of the one dataflow they all run -- S^T on 32x32x16 MFMAs, lane-local softmax, accumulator-as-operand P V, output
// in the GEMM A-operand layout -- each written once.  The hand-scheduled slots of attention_pipe.hip place single MFMAs between
// sched_barriers and deliberately do not use the MFMA helpers.  Not part of the C ABI.
#pragma once
#include "common.h"
#include "kernels.h"
#include <type_traits>

namespace cwm {

// Query tile / (batch, head) of work item L (dispatch order) of nqb x nbh items of `rows` query rows each.  Speed only -- the mapping
// is a bijection, any placement is correct:
//  * all query tiles of one (batch, head) go to ONE XCD (workgroups are dealt round-robin over the 8 XCDs by their linear id), so its
//    K / V tiles are fetched into one L2 instead of up to eight (ViT-B/8 encoder: 7 tiles per head, 405 KB of K / V per head)
//  * inside an XCD the ragged last query tile of every head (N = 792: 24 of 128 rows, one active wave) is dispatched after all full
//    tiles, so that those light workgroups fill the tail of the launch instead of being spread through it
__device__ __forceinline__ void attn_tile_of_item(int L, int nqb, int nbh, int nq, int rows, bool remap, int& qt, int& bh) {
    qt = L % nqb;
    bh = L / nqb;
    if (nbh % 8 != 0 || !remap) return;
    const int xcd = L & 7, idx = L >> 3, per = nbh >> 3;
    const int light = (nqb > 1 && (nq - (nqb - 1) * rows) * 2 <= rows) ? 1 : 0;  // last tile at most half full
    const int heavy = nqb - light;
    if (idx < per * heavy) {
        bh = xcd * per + idx / heavy;
        qt = idx - (idx / heavy) * heavy;
    } else {
        bh = xcd * per + (idx - per * heavy);
        qt = nqb - 1;
    }
}
// (the same for a 2-D grid of (nqb, nbh) workgroups: linear id = dispatch order)
__device__ __forceinline__ void attn_tile_of_block(int nq, int rows, bool remap, int& qt, int& bh) {
    attn_tile_of_item(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, gridDim.y, nq, rows, remap, qt, bh);
}

__device__ __forceinline__ int lds_off128(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
// V tile image: key row of 128 bytes, 16-byte chunk c (8 d) stored at c ^ 4 on key rows with bit 1 set
__device__ __forceinline__ int lds_off_v(int row, int chunk) { return row * 128 + ((chunk ^ (((row >> 1) & 1) << 2)) << 4); }

typedef __attribute__((ext_vector_type(4))) short s16x4;
__device__ __forceinline__ bf16x4 lds_read_tr16(const char* ptr) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)ptr);
    return __builtin_bit_cast(bf16x4, v);
}
// the two transposed reads (keys +0..3, +8..11) of a V^T fragment as one A operand
__device__ __forceinline__ bf16x8 join_halves(const bf16x4 (&h)[2]) { return __builtin_shufflevector(h[0], h[1], 0, 1, 2, 3, 4, 5, 6, 7); }

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
// ds_read_b64_tr_b16 as inline asm (attention.hip / attention_pipe.hip, the P V phase); OFF = immediate byte offset
template <int OFF>
__device__ __forceinline__ u32x2 lds_read_tr16_asm(unsigned addr) {
    u32x2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
// all V^T fragments of k-step KS: [d-block][plane][half]
template <int KS, int PLANES>
__device__ __forceinline__ void lds_read_v_step(u32x2 (&dst)[2][PLANES][2], unsigned va0, unsigned va1) {
    constexpr int T = 64 * 64 * 2;
    dst[0][0][0] = lds_read_tr16_asm<KS * 2048>(va0);
    dst[0][0][1] = lds_read_tr16_asm<KS * 2048 + 1024>(va0);
    if constexpr (PLANES == 2) {
        dst[0][PLANES - 1][0] = lds_read_tr16_asm<KS * 2048 + T>(va0);
        dst[0][PLANES - 1][1] = lds_read_tr16_asm<KS * 2048 + T + 1024>(va0);
    }
    dst[1][0][0] = lds_read_tr16_asm<KS * 2048>(va1);
    dst[1][0][1] = lds_read_tr16_asm<KS * 2048 + 1024>(va1);
    if constexpr (PLANES == 2) {
        dst[1][PLANES - 1][0] = lds_read_tr16_asm<KS * 2048 + T>(va1);
        dst[1][PLANES - 1][1] = lds_read_tr16_asm<KS * 2048 + T + 1024>(va1);
    }
}

// s_waitcnt lgkmcnt(N) for fragments requested by lds_read_v_step.  The registers are operands of the wait: hipcc treats the
// output of the asm read as available at once, and without the dependency it is free to schedule a consumer (an MFMA) above
// a bare s_waitcnt statement -- which goes unnoticed as long as the LDS answers quickly (one workgroup per CU) and reads stale
// registers when it does not.
template <int N, int PLANES>
__device__ __forceinline__ void lds_wait_v_step(u32x2 (&v)[2][PLANES][2]) {
    if constexpr (PLANES == 2)
        asm volatile("s_waitcnt lgkmcnt(%8)"
                     : "+v"(v[0][0][0]), "+v"(v[0][0][1]), "+v"(v[0][1][0]), "+v"(v[0][1][1]), "+v"(v[1][0][0]), "+v"(v[1][0][1]), "+v"(v[1][1][0]), "+v"(v[1][1][1])
                     : "n"(N)
                     : "memory");
    else
        asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(v[0][0][0]), "+v"(v[0][0][1]), "+v"(v[1][0][0]), "+v"(v[1][0][1]) : "n"(N) : "memory");
}

// max over the lane pair (l, l ^ 32) -- the two key halves of a query in the 32x32 accumulator layout -- with one v_permlane32_swap
// (__shfl_xor would be a ds_bpermute round trip through the LDS queue plus five VALU instructions of index arithmetic)
__device__ __forceinline__ float max_lane_xor32(float x) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}

// the other half of the pair: sum over (l, l ^ 32)
__device__ __forceinline__ float sum_lane_xor32(float x) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}

// ---- building blocks of the shared dataflow (lane = (column qcol = lane & 31, half hh = lane >> 5) of a 32x32 accumulator) ----

// acc += a . b with split-bf16 operands: lo*hi, hi*lo, hi*hi, ALWAYS in this order (the order is what makes attention_kernel and
// attention_pipe_kernel bit-identical); PLANES == 1: hi*hi only -- callers pass index [PLANES - 1] for the lo operands, so the
// one-plane form names no second register.
template <int PLANES>
__device__ __forceinline__ void mfma_split(f32x16& acc, const bf16x8& a_hi, const bf16x8& a_lo, const bf16x8& b_hi, const bf16x8& b_lo) {
    if constexpr (PLANES == 2) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b_hi, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_lo, acc, 0, 0, 0);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_hi, acc, 0, 0, 0);
}

// P^T fragment (B operand) of k-step ks of a 32-key block: the accumulator's own elements 8 ks .. 8 ks + 7 as bf16 hi [, lo]
template <int PLANES>
__device__ __forceinline__ void p_fragments(const f32x16& s, int ks, bf16x8& ph, bf16x8& plo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) split_bf16_at<PLANES>(s[8 * ks + j], ph, plo, j);
}

// row (of 32) that accumulator element r holds in lane half hh
__device__ __forceinline__ int acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
// rows row0 + acc_row at or past `limit` (keys past the sequence end, padded context tokens) leave the softmax: -inf
__device__ __forceinline__ void mask_rows_from(f32x16& s, int row0, int hh, int limit) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (row0 + acc_row(r, hh) >= limit) s[r] = -INFINITY;
}

// One 32-wide d block of O^T (acc * mul) to columns col0 .. col0 + 31 of row `row` in the GEMM A-operand layout (common.h a_pos)
template <int PLANES>
__device__ __forceinline__ void store_o_block(bf16* o, int64_t row, int ld, int col0, const f32x16& acc, float mul, int hh) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        bf16x4 hi4, lo4;
#pragma unroll
        for (int e = 0; e < 4; ++e) split_bf16_at<PLANES>(acc[4 * g + e] * mul, hi4, lo4, e);
        store_operand_split<PLANES>(o, row, ld, col0 + 8 * g + 4 * hh, hi4, lo4);
    }
}

// Q fragments (B operand of S^T) of the head_dim-64 kernels from head-major Q: the lane holds Q[qrow][16 s + 8 hh + 0..7]
template <int PLANES>
__device__ __forceinline__ void load_q_fragments(bf16x8 (&qf)[PLANES][4], const bf16* Qb, int64_t qk_plane, int qrow, int hh) {
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl)
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[pl][s] = *reinterpret_cast<const bf16x8*>(Qb + (size_t)pl * qk_plane + (size_t)qrow * 64 + s * 16 + hh * 8);
}

// V^T (A operand of O^T) by transposed reads of a [key][64 d] image (lds_off_v): this lane's byte offset for d block db.
// 16-lane group g = lane >> 4 reads the block {keys 4 (g >> 1) + 0..3 (+ 16 ks, + 8 for the second half of the fragment)} x
// {d = 32 db + 16 (g & 1) + 0..15}: lane 4 q + pc of the group supplies the address of key row q, d columns 4 pc .. 4 pc + 3, and
// lane i receives d column i (= 32 db + lane % 32) with key q in element q.  Key offsets 16 ks + 8 half are multiples of 4, so the
// swizzle bit is (q >> 1) & 1 and they are plain immediates (2048 ks + 1024 half bytes); the two db blocks differ by the swizzled
// chunk bit -> one base register each.
__device__ __forceinline__ int v_tr_offset(int lane, int db) {
    const int g = lane >> 4, q = (lane >> 2) & 3, pc = lane & 3;
    return lds_off_v(4 * (g >> 1) + q, db * 4 + (g & 1) * 2 + (pc >> 1)) + (pc & 1) * 8;
}

// Register staging of 64-key K / V tiles, global -> registers -> swizzled LDS images, by a workgroup of 256 threads (attention_kernel:
// one tile in flight; attention_tail_block: NT = 2, a pass stages two).  512 16-byte chunks per tile and plane (row = key, 8 chunks
// of 8 d), 2 per thread.  An LDS stage is K planes, then V planes.
template <int PLANES, int NT>
struct KvStage {
    static constexpr int TILE_BYTES = 64 * 64 * 2;
    int row[2], chunk[2], koff[2], voff[2];
    u32x4 rk[NT][PLANES][2], rv[NT][PLANES][2];
    __device__ __forceinline__ void init(int tid) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * 256;
            row[i] = idx >> 3;
            chunk[i] = idx & 7;
            koff[i] = lds_off128(row[i], chunk[i]);
            voff[i] = lds_off_v(row[i], chunk[i]);
        }
    }
    // key tile kt of an N-key sequence into register set t
    __device__ __forceinline__ void load(int t, const bf16* Kb, const bf16* Vb, int64_t qk_plane, int kt, int N) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            // keys past the sequence end re-read the last row: finite values, and P is exactly 0 there
            const size_t off = (size_t)min(kt * 64 + row[i], N - 1) * 64 + chunk[i] * 8;
#pragma unroll
            for (int pl = 0; pl < PLANES; ++pl) {
                rk[t][pl][i] = *reinterpret_cast<const u32x4*>(Kb + (size_t)pl * qk_plane + off);
                rv[t][pl][i] = *reinterpret_cast<const u32x4*>(Vb + (size_t)pl * qk_plane + off);
            }
        }
    }
    // register set t into the LDS stage at `stage`
    __device__ __forceinline__ void store(int t, char* stage) const {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int pl = 0; pl < PLANES; ++pl) {
                *reinterpret_cast<u32x4*>(stage + pl * TILE_BYTES + koff[i]) = rk[t][pl][i];
                *reinterpret_cast<u32x4*>(stage + (PLANES + pl) * TILE_BYTES + voff[i]) = rv[t][pl][i];
            }
    }
};

}  // namespace cwm
