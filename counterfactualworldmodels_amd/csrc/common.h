// Shared device/host helpers for the CDNA4 (gfx950) VMAE predictor kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace cwm {

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
// NB: use this native vector (not HIP's struct uint4) for register-staged tiles: arrays of the HIP
// struct types are not promoted to registers by hipcc and end up in scratch.
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
// Four floats at an address that is only 4-byte aligned: what the generic un-embed and read-out kernels move (C != 3, a pointer off the 16-byte grid, strides
// that are no multiple of 4), so their groups of four pixels may start at any float.
struct __attribute__((packed, aligned(4))) Float4A4 {
    float v[4];
};

constexpr int kWave = 64;

// Split an fp32 value into bf16 hi + bf16 lo (hi + lo carries ~16 significand bits).
__device__ __forceinline__ void split_bf16(float v, bf16& hi, bf16& lo) {
    hi = (bf16)v;
    lo = (bf16)(v - (float)hi);
}

// GEMM A/W operand layout.  PLANES == 1 ("fast"): plain [rows][ld] bf16.  PLANES == 2 ("parity"): ONE buffer
// [rows][2*ld] with the hi and lo planes interleaved per 32-element k block -- [32 hi | 32 lo] = one 128-byte
// line -- so that the GEMM's LDS-DMA requests are full cache lines in both modes (64-byte half-line requests
// measured ~1.5x slower per byte).  a_pos() is the position of the hi element; the lo element is 32 further.
template <int PLANES>
__device__ __forceinline__ size_t a_pos(int64_t row, int ld, int col) {
    if constexpr (PLANES == 1) return (size_t)row * ld + col;
    else return (size_t)row * 2 * ld + ((col >> 5) << 6) + (col & 31);
}
constexpr int kLoOffset = 32;

// ---- operand WRITERS: the one place that knows where the lo plane lies.  Producers write through these, readers through a_pos. ----

// Register-only split, element j of a hi / lo vector pair.  PLANES == 1 neither computes nor names `lo`: the one-plane kernels keep
// their register counts (the same point as mfma_split, attention_device.h).
template <int PLANES, class V>
__device__ __forceinline__ void split_bf16_at(float v, V& hi, V& lo, int j) {
    const bf16 h = (bf16)v;
    hi[j] = h;
    if constexpr (PLANES == 2) lo[j] = (bf16)(v - (float)h);
}
// ... of 4 values, and of 8 (two f32x4: elements 0-3, 4-7)
template <int PLANES>
__device__ __forceinline__ void split_bf16v(const f32x4& v, bf16x4& hi, bf16x4& lo) {
#pragma unroll
    for (int e = 0; e < 4; ++e) split_bf16_at<PLANES>(v[e], hi, lo, e);
}
template <int PLANES>
__device__ __forceinline__ void split_bf16v(const f32x4& v0, const f32x4& v1, bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int e = 0; e < 4; ++e) split_bf16_at<PLANES>(v0[e], hi, lo, e);
#pragma unroll
    for (int e = 0; e < 4; ++e) split_bf16_at<PLANES>(v1[e], hi, lo, 4 + e);
}

// An already split group (V = bf16, bf16x4, bf16x8) to columns k .. of `row`: one store per plane.  k is a multiple of the group's
// width, so the group never straddles a 32-k [hi | lo] block.
template <int PLANES, class V>
__device__ __forceinline__ void store_operand_split(bf16* A, int64_t row, int ld, int k, const V& hi, const V& lo) {
    bf16* d = A + a_pos<PLANES>(row, ld, k);
    *reinterpret_cast<V*>(d) = hi;
    if constexpr (PLANES == 2) *reinterpret_cast<V*>(d + kLoOffset) = lo;
}

template <int PLANES>
__device__ __forceinline__ void store_operand(bf16* A, int64_t row, int ld, int k, float v) {
    const bf16 h = (bf16)v;
    bf16 l;
    if constexpr (PLANES == 2) l = (bf16)(v - (float)h);
    store_operand_split<PLANES>(A, row, ld, k, h, l);
}
template <int PLANES>
__device__ __forceinline__ void store_operand4(bf16* A, int64_t row, int ld, int k, const f32x4& v) {
    bf16x4 hi, lo;
    split_bf16v<PLANES>(v, hi, lo);
    store_operand_split<PLANES>(A, row, ld, k, hi, lo);
}
template <int PLANES>
__device__ __forceinline__ void store_operand8(bf16* A, int64_t row, int ld, int k, const f32x4& v0, const f32x4& v1) {
    bf16x8 hi, lo;
    split_bf16v<PLANES>(v0, v1, hi, lo);
    store_operand_split<PLANES>(A, row, ld, k, hi, lo);
}
// zeros in columns k_from .. ld - 1 of `row` (the K padding of a producer whose K is not a multiple of the GEMM's k tile)
template <int PLANES>
__device__ __forceinline__ void zero_operand_tail(bf16* A, int64_t row, int ld, int k_from) {
    for (int k = k_from; k < ld; ++k) store_operand_split<PLANES>(A, row, ld, k, (bf16)0.f, (bf16)0.f);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The same butterfly without the LDS: DPP inside a row of 16 lanes (xor 1, xor 2, then mirrors of quad- / half-row-uniform values),
// v_permlane16_swap / v_permlane32_swap across rows (gfx950).  __shfl_xor is a ds_bpermute round trip per step -- six dependent LDS
// latencies per reduction.  Every lane gets the sum; the order of the additions differs from wave_sum (fp32 rounding).
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, true));  // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, true));  // row_mirror
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// Sum over each aligned group of 8 consecutive lanes (every lane of the group gets the total): DPP only, no LDS round trip.
__device__ __forceinline__ float group8_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, true));  // row_half_mirror
    return v;
}

// A run-time value as a template argument: calls fn(std::integral_constant<int, N>{}) for the N of the list that equals n (launch sites: `K<q.value>`).
// Returns false, having called nothing, when n is not in the list.  Call sites pass a bool or a `? :` over the listed values, so that cannot happen there; a site
// that passes anything else must check the result.  (The compiler emits the kernels a generic lambda instantiates in the REVERSE of the list's order; the launch
// sites list the values so that each object file keeps the order its kernels had under the `if (planes == 1) K<1> else K<2>` pairs they replaced.)
template <int... Ns, class F>
static inline bool dispatch_int(int n, F&& fn) {
    return ((n == Ns && (fn(std::integral_constant<int, Ns>{}), true)) || ...);
}

// XCD-aware bijective remap of a linear workgroup id (guide §5.5 T1): blocks b and b+8 share an
// XCD under round-robin dispatch, so give every XCD a contiguous chunk of the logical tile order.
// Speed only; any placement is correct.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int nx = 8;
    int q = nwg / nx, r = nwg % nx;
    int xcd = bid % nx, idx = bid / nx;
    int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

}  // namespace cwm

// ---- host-side error plumbing (C ABI never throws) ------------------------------------------
void cwm_set_error(const char* fmt, ...);
// hipFuncAttributeMaxDynamicSharedMemorySize for a kernel, once per (device, kernel): the attribute is per device, so a process-wide
// "done" flag would leave a second device without it (engine.hip; thread-safe).  Returns 0 or CWM_ERR_HIP.
int cwm_set_max_lds(const void* kernel, int bytes);

// A handle (model, communicator) belongs to the HIP device that was current when it was created: its weights, workspace, streams and RCCL
// communicator live there, and a launch from another current device would run on the wrong GPU without any error.  0 when the calling thread's
// current device is `handle_device`, else CWM_ERR_INVALID with a message naming `what` (engine.hip).
int cwm_require_device(int handle_device, const char* what);

#define CWM_HIP_CHECK(expr)                                                                  \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            cwm_set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return -2;                                                                       \
        }                                                                                    \
    } while (0)

#define CWM_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            cwm_set_error(__VA_ARGS__);   \
            return -1;                    \
        }                                 \
    } while (0)
