// The ordering rule of the device selections (cwm_unmask_step, cwm_segment_step, cwm_segment_merge, cwm_seed_select), stated once: cells are ranked by (class, key descending with a NaN above every
// number and -0 equal to +0, index ascending), packed into one 64-bit rank word, and k rounds of arg-max over a workgroup of kSelThreads threads take the first k.
// Fixed order, no atomics.  Cell c belongs to thread c % kSelThreads.
#pragma once
#include "common.h"

namespace cwm {

constexpr int kSelThreads = 256;
constexpr int kSelMaxCells = 4096;  // the index takes the low 12 bits of a rank word

// Orders fp32 keys as torch.sort(descending=True) does: a NaN above every number, -0 equal to +0.
__device__ __forceinline__ unsigned um_order(float v) {
    if (v != v) return 0xFFFFFFFFu;
    if (v == 0.f) v = 0.f;
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long um_max64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// The rank word of cell c (cls >= 1; 0 is "not a candidate"), and the cell of a winning word (-1: none left).
__device__ __forceinline__ unsigned long long um_rank(int cls, float key, int c) {
    return ((unsigned long long)cls << 44) | ((unsigned long long)um_order(key) << 12) | (unsigned long long)(kSelMaxCells - 1 - c);
}
__device__ __forceinline__ int um_rank_cell(unsigned long long win) { return win ? kSelMaxCells - 1 - (int)(win & (kSelMaxCells - 1)) : -1; }

// The maximum of v over the workgroup, in every thread: xor shuffles within a wave, one LDS exchange between the four waves.  `xch` has 4 slots and may be
// reused after the call returns only behind another barrier (the callers alternate two sets).
__device__ __forceinline__ unsigned long long um_block_max(unsigned long long v, unsigned long long* xch) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = um_max64(v, (unsigned long long)__shfl_xor((long long)v, o, 64));
    if ((threadIdx.x & 63) == 0) xch[threadIdx.x >> 6] = v;
    __syncthreads();
    return um_max64(um_max64(xch[0], xch[1]), um_max64(xch[2], xch[3]));
}

// k rounds of arg-max over the rank words comp[0 .. n): `best` is the maximum over the thread's own cells on entry.  A round is xor shuffles and one LDS
// exchange (round r uses xch[(r + 1) & 1]); on_pick(r, cell) runs in EVERY thread (cell -1: no candidate is left), then the thread that owns the pick
// clears its word and scans its cells again.
template <class OnPick>
__device__ __forceinline__ void um_select_rounds(unsigned long long* comp, int n, int k, unsigned long long best, unsigned long long (*xch)[4], OnPick on_pick) {
    const int tid = threadIdx.x;
    for (int r = 0; r < k; ++r) {
        const int cell = um_rank_cell(um_block_max(best, xch[(r + 1) & 1]));
        on_pick(r, cell);
        if (cell >= 0 && (cell & (kSelThreads - 1)) == tid) {
            comp[cell] = 0;
            best = 0;
            for (int c = tid; c < n; c += kSelThreads) best = um_max64(best, comp[c]);
        }
    }
}

// The same rounds where a pick removes more than itself (cwm_seed_select: every candidate within a window of the pick): removes(cell, c) says whether the pick
// `cell` takes candidate c out; it must hold for c == cell.  In every round each thread clears its own cells, and a thread that cleared anything scans its cells
// again.  removes() must depend on the geometry alone, so that the loop reads and writes comp[0 .. n) whatever the words hold.
template <class OnPick, class Removes>
__device__ __forceinline__ void um_select_rounds_removing(unsigned long long* comp, int n, int k, unsigned long long best, unsigned long long (*xch)[4], OnPick on_pick,
                                                          Removes removes) {
    const int tid = threadIdx.x;
    for (int r = 0; r < k; ++r) {
        const int cell = um_rank_cell(um_block_max(best, xch[(r + 1) & 1]));
        on_pick(r, cell);
        if (cell < 0) continue;
        bool cleared = false;
        for (int c = tid; c < n; c += kSelThreads)
            if (comp[c] && removes(cell, c)) comp[c] = 0, cleared = true;
        if (cleared) {
            best = 0;
            for (int c = tid; c < n; c += kSelThreads) best = um_max64(best, comp[c]);
        }
    }
}

}  // namespace cwm
