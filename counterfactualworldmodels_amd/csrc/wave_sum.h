// The sum of a value over the 64 lanes of a wave, in every lane, for the table kernels that add one slot per wave before they touch LDS (object_motion.hip,
// object_response.hip).  No HIP call.
#pragma once
#include "common.h"

namespace cwm {

// The sum of v over the 64 lanes of a wave, in every lane (it is wave-uniform); EVERY lane of the wave must call it.  Four DPP steps leave each lane with the sum
// of its row of 16 lanes -- the neighbour of its pair, of its quad, the mirrored half row, the mirrored row --, and the four rows are read out of lanes 0, 16, 32
// and 48.  (Six dependent __shfl_xor steps per word are a ds_bpermute round trip each, for 24 words: cwm_object_motion's kernel took twice as long with them.)
template <int kCtrl>
__device__ __forceinline__ int wave_dpp(int v) {
    return __builtin_amdgcn_update_dpp(0, v, kCtrl, 0xf, 0xf, false);
}
constexpr int kDppQuadXor1 = 0xB1, kDppQuadXor2 = 0x4E, kDppRowHalfMirror = 0x141, kDppRowMirror = 0x140;  // quad_perm:[1,0,3,2], quad_perm:[2,3,0,1]
__device__ __forceinline__ int wave_sum(int v) {
    v += wave_dpp<kDppQuadXor1>(v);
    v += wave_dpp<kDppQuadXor2>(v);
    v += wave_dpp<kDppRowHalfMirror>(v);
    v += wave_dpp<kDppRowMirror>(v);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}
template <int kCtrl>
__device__ __forceinline__ long long wave_dpp64(long long v) {
    const unsigned lo = (unsigned)wave_dpp<kCtrl>((int)(unsigned)v), hi = (unsigned)wave_dpp<kCtrl>((int)(unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ long long wave_lane64(long long v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), lane);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ long long wave_sum(long long v) {
    v += wave_dpp64<kDppQuadXor1>(v);
    v += wave_dpp64<kDppQuadXor2>(v);
    v += wave_dpp64<kDppRowHalfMirror>(v);
    v += wave_dpp64<kDppRowMirror>(v);
    return wave_lane64(v, 0) + wave_lane64(v, 16) + wave_lane64(v, 32) + wave_lane64(v, 48);
}

}  // namespace cwm
