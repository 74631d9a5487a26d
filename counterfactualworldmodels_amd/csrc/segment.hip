// Spelke-object segmentation, one step (cwm_segment_step): which pixels move with a seed point in the S counterfactual flows of a movie, the connected region of
// them that hangs on the seed's patch, how much of every patch it covers, and which patches the next round of counterfactuals moves (inside the region) and pins
// (in the ring just outside it).  No counterpart in the reference: its README names the use and lists "Iterative algorithms for segmenting Spelke objects" as coming.
//
// The definition (this is the contract; include/cwm_hip.h repeats it for callers).  Flows f[b][c][y][x][s] by five element strides, c = 0 the x-displacement u and
// c = 1 the y-displacement v; seeds[b] = (y, x); patch size P, gh = H / P, gw = W / P, n = gh gw; directions dirs[s] = (dy, dx), optional.  Per row b, in this order:
//   1 magnitude   m_s(p) = flow_mag2(u, v) of flow_view.h, the filter's form
//   2 seed cell   (y, x) clamped into the image; c0 = (y / P) gw + x / P
//   3 seed ref    ref_s = (the sum of m_s over the P P pixels of cell c0 in row-major order, from 0.f, plain fp32 adds by ONE thread) / (float)(P P).  The fixed order
//                 is the point: no tree
//   4 valid       s is valid iff ref_s >= min_seed_mag (a NaN is not valid); n_valid = their number
//   5 votes       p votes in a valid s iff m_s(p) >= fmaxf(abs_thresh, rel_thresh * ref_s) and, with dirs, u dx + v dy >= (cos_min * m_s(p)) * sqrtf(dx dx + dy dy);
//                 a NaN compares false; votes[p] = the number of samples in which p votes (a byte: S <= 255)
//   6 candidates  need = max(1, (int)ceilf(vote_frac * (float)n_valid)); candidate[p] = n_valid > 0 && votes[p] >= need
//   7 segment     the union of the 4-connected components of `candidate` that hold a candidate pixel of cell c0; empty when the cell has none; seed_hit = 0 / 1
//   8 cover       cover[cell] = (#segment pixels of the cell) / (float)(P P), exact for P = 4, 8, 16
//   9 stats       (n_valid, area, n_candidates, seed_hit)
//  10 selection   (k_active > 0)  inside = cover >= inside_frac; touched = cover > 0; ring = !touched and a touched cell within Chebyshev distance ring_radius.
//                 Order: select_order.h (the higher key first, a NaN above every number, -0 equal to +0, the lower index first); keys[b][0] ranks the active picks,
//                 keys[b][1] the passive ones, no keys = all 0 = index order.  Active: c0 first and always, then the first k_active - 1 inside cells other than
//                 c0.  Passive: the first k_passive ring cells.  active_out / passive_out [B][2 n]: frame 0 all 0, frame 1 all 1 with the picks of their kind
//                 cleared (cwm_prompt_table_expand's convention); picks [B][k_active + k_passive] = n + cell, -1 for a slot that found no cell
//  11 init step   no flows: an empty segment, so active_out holds c0 alone and passive_out nothing
//
// Three passes.  segment_ref_kernel: one thread per (b, s).  segment_vote_*: many workgroups stream the flows once (the form: flow_view.h flow_vote_form) and write
// the vote bytes -- counts are summed per pixel inside a thread or through LDS bytes, no atomics.  segment_component_kernel: one workgroup per row; the candidate and
// the reached bitmaps live in LDS as bit rows of ceil(W / 32) words, propagation works on whole words.  No table content moves an address: the seed is clamped, every
// other index comes from the thread index and the geometry.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/cwm_hip.h"
#include "common.h"
#include "flow_view.h"
#include "kernels.h"
#include "select_order.h"

namespace cwm {

namespace {

constexpr int kVoteThreads = 256;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// ref_s, or a NaN where sample s is not valid
__global__ __launch_bounds__(64) void segment_ref_kernel(const float* __restrict__ f, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int64_t ss, int B, int H, int W,
                                                        int S, int P, const int* __restrict__ seeds, float min_seed_mag, float* __restrict__ seed_ref) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B * S) return;
    const int b = i / S, s = i - b * S;
    const int y0 = clampi(seeds[2 * b], 0, H - 1) / P * P, x0 = clampi(seeds[2 * b + 1], 0, W - 1) / P * P;
    const float* u = f + b * sb + s * ss;
    float sum = 0.f;
    for (int r = 0; r < P; ++r)
        for (int c = 0; c < P; ++c) {
            const int64_t off = (int64_t)(y0 + r) * sh + (int64_t)(x0 + c) * sw;
            sum += flow_mag2(u[off], u[off + sc]);
        }
    const float ref = sum / (float)(P * P);
    seed_ref[i] = ref >= min_seed_mag ? ref : __int_as_float(0x7fc00000);
}

// The per-sample tables of a vote workgroup: the magnitude threshold (a NaN for a sample that is not valid: nothing compares >= NaN, so it gets no vote) and the direction
struct VoteTables {
    float thr[kSegmentMaxSamples + 1], dx[kSegmentMaxSamples + 1], dy[kSegmentMaxSamples + 1], dn[kSegmentMaxSamples + 1];
};
__device__ __forceinline__ void vote_tables(VoteTables& t, const float* __restrict__ ref, const float* __restrict__ dirs, int S, float abs_thresh, float rel_thresh) {
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
        const float r = ref[s];
        t.thr[s] = r == r ? fmaxf(abs_thresh, rel_thresh * r) : r;
        const float dy = dirs ? dirs[2 * s] : 0.f, dx = dirs ? dirs[2 * s + 1] : 0.f;
        t.dy[s] = dy, t.dx[s] = dx, t.dn[s] = sqrtf(dx * dx + dy * dy);
    }
    __syncthreads();
}
template <bool DIRS>
__device__ __forceinline__ int vote_of(const VoteTables& t, int s, float u, float v, float cos_min) {
    const float m = flow_mag2(u, v);
    bool ok = m >= t.thr[s];
    if (DIRS) ok = ok && (u * t.dx[s] + v * t.dy[s] >= (cos_min * m) * t.dn[s]);
    return ok ? 1 : 0;
}

// one pixel per thread through all five strides (coalesced where sw == 1: adjacent threads, adjacent floats)
template <bool DIRS>
__global__ __launch_bounds__(kVoteThreads) void segment_vote_strided_kernel(const float* __restrict__ f, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int64_t ss,
                                                                            int HW, int W, int S, const float* __restrict__ seed_ref, const float* __restrict__ dirs,
                                                                            float abs_thresh, float rel_thresh, float cos_min, uint8_t* __restrict__ votes) {
    __shared__ VoteTables t;
    const int b = blockIdx.y;
    vote_tables(t, seed_ref + (size_t)b * S, dirs, S, abs_thresh, rel_thresh);
    const int e = blockIdx.x * kVoteThreads + threadIdx.x;
    if (e >= HW) return;
    const int y = e / W, x = e - y * W;
    const float* u = f + b * sb + (int64_t)y * sh + (int64_t)x * sw;
    int cnt = 0;
    for (int s = 0; s < S; ++s) cnt += vote_of<DIRS>(t, s, u[s * ss], u[s * ss + sc], cos_min);
    votes[(size_t)b * HW + e] = (uint8_t)cnt;
}

// contiguous 16-byte aligned planes of a multiple of 4 pixels: four pixels per thread, their votes as one 4-byte store
template <bool DIRS>
__global__ __launch_bounds__(kVoteThreads) void segment_vote_planes_kernel(const float* __restrict__ f, int64_t sb, int64_t sc, int64_t ss, int HW, int S,
                                                                           const float* __restrict__ seed_ref, const float* __restrict__ dirs, float abs_thresh,
                                                                           float rel_thresh, float cos_min, uint8_t* __restrict__ votes) {
    __shared__ VoteTables t;
    const int b = blockIdx.y;
    vote_tables(t, seed_ref + (size_t)b * S, dirs, S, abs_thresh, rel_thresh);
    const int e = 4 * (blockIdx.x * kVoteThreads + (int)threadIdx.x);
    if (e >= HW) return;  // HW % 4 == 0: e + 3 < HW
    const float* u = f + b * sb + e;
    unsigned cnt = 0;  // four byte counters (S <= 255: no carry between them)
    for (int s = 0; s < S; ++s) {
        const float4 a = *reinterpret_cast<const float4*>(u + s * ss), c = *reinterpret_cast<const float4*>(u + s * ss + sc);
        cnt += (unsigned)vote_of<DIRS>(t, s, a.x, c.x, cos_min) | ((unsigned)vote_of<DIRS>(t, s, a.y, c.y, cos_min) << 8) |
               ((unsigned)vote_of<DIRS>(t, s, a.z, c.z, cos_min) << 16) | ((unsigned)vote_of<DIRS>(t, s, a.w, c.w, cos_min) << 24);
    }
    *reinterpret_cast<unsigned*>(votes + (size_t)b * HW + e) = cnt;
}

// packed layout: a workgroup takes kVoteTilePix consecutive pixels = that many times S consecutive floats per channel; a vote is a byte in LDS, four threads add up
// the S bytes of a pixel (integers: no order to fix)
template <bool DIRS>
__global__ __launch_bounds__(kVoteThreads) void segment_vote_packed_kernel(const float* __restrict__ f, int64_t sb, int64_t sc, int HW, int S,
                                                                           const float* __restrict__ seed_ref, const float* __restrict__ dirs, float abs_thresh,
                                                                           float rel_thresh, float cos_min, uint8_t* __restrict__ votes) {
    __shared__ VoteTables t;
    __shared__ unsigned char flag[kVoteTilePix * kSegmentMaxSamples];
    const int b = blockIdx.y, pix0 = blockIdx.x * kVoteTilePix;
    vote_tables(t, seed_ref + (size_t)b * S, dirs, S, abs_thresh, rel_thresh);
    const int npix = min(kVoteTilePix, HW - pix0), n = npix * S;
    const float* u = f + b * sb + (int64_t)pix0 * S;
    for (int e = threadIdx.x; e < n; e += kVoteThreads) flag[e] = (unsigned char)vote_of<DIRS>(t, e % S, u[e], u[e + sc], cos_min);
    __syncthreads();
    const int pix = threadIdx.x >> 2, part = threadIdx.x & 3;  // kVoteThreads / 4 == kVoteTilePix
    int cnt = 0;
    if (pix < npix)
        for (int s = part; s < S; s += 4) cnt += flag[pix * S + s];
    cnt += __shfl_xor(cnt, 1, 64);
    cnt += __shfl_xor(cnt, 2, 64);
    if (part == 0 && pix < npix) votes[(size_t)b * HW + pix0 + pix] = (uint8_t)cnt;
}
static_assert(kVoteThreads == 4 * kVoteTilePix, "four threads per pixel of a packed tile");

// Spreads the reached bits r (a subset of c) along the runs of set bits of c inside one word, both ways: five doubling shift-or steps per direction.
__device__ __forceinline__ unsigned fill_word(unsigned r, unsigned c) {
    unsigned up = r, m = c;
    up |= m & (up << 1), m &= m << 1;
    up |= m & (up << 2), m &= m << 2;
    up |= m & (up << 4), m &= m << 4;
    up |= m & (up << 8), m &= m << 8;
    up |= m & (up << 16);
    unsigned dn = r;
    m = c;
    dn |= m & (dn >> 1), m &= m >> 1;
    dn |= m & (dn >> 2), m &= m >> 2;
    dn |= m & (dn >> 4), m &= m >> 4;
    dn |= m & (dn >> 8), m &= m >> 8;
    dn |= m & (dn >> 16);
    return up | dn;
}

// One workgroup per row b.  Dynamic LDS: the candidate and the reached bitmap (`words` 32-bit words each, bit x & 31 of word y wpr + x / 32 is pixel (y, x); the
// unused high bits of a row's last word stay 0), and after the coverage is counted the rank words of the selection in the same bytes.
__global__ __launch_bounds__(kSelThreads) void segment_component_kernel(const SegmentStepParams p, int wpr, int words) {
    extern __shared__ unsigned long long seg_lds[];
    __shared__ unsigned short cnt[kSelMaxCells];  // segment pixels of a cell
    __shared__ unsigned char rowt[kSelMaxCells];  // a touched cell within the radius in the cell's grid row
    __shared__ unsigned char sel[kSelMaxCells];   // bit 0: an active pick, bit 1: a passive pick
    __shared__ unsigned long long xch[2][4];
    __shared__ int red[2][4];
    volatile unsigned* cand = reinterpret_cast<unsigned*>(seg_lds);
    volatile unsigned* reach = cand + words;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int H = p.H, W = p.W, P = p.P, HW = H * W, gw = W / P, gh = H / P, n = gh * gw;
    const bool init = p.f == nullptr;

    int valid = 0;
    if (!init && tid < p.S) {  // S <= 255 < kSelThreads
        const float r = p.seed_ref[(size_t)b * p.S + tid];
        valid = r == r;
    }
    const int n_valid = __syncthreads_count(valid);
    const float nf = ceilf(p.vote_frac * (float)n_valid);
    const int need = nf >= 256.f ? 256 : nf >= 1.f ? (int)nf : 1;  // max(1, (int)nf), kept inside what a byte can reach

    const int sy = clampi(p.seeds[2 * b], 0, H - 1), sx = clampi(p.seeds[2 * b + 1], 0, W - 1);
    const int y0 = sy / P * P, x0 = sx / P * P, c0 = (sy / P) * gw + sx / P;
    const unsigned cell_bits = (1u << P) - 1u;  // P <= 16; 32 % P == 0: the P bits of a cell's row lie in one word

    // candidates: 64 pixels of the padded rows per wave and step, their bits as one ballot
    const uint8_t* vrow = p.votes ? p.votes + (size_t)b * HW : nullptr;
    const int row_bits = wpr * 32, total = words * 32;
    for (int base = 0; base < total; base += kSelThreads) {
        const int e = base + tid, y = e / row_bits, x = e - y * row_bits;
        const bool c = !init && n_valid > 0 && e < total && x < W && (int)vrow[y * W + x] >= need;
        const unsigned long long bits = __ballot(c);
        if ((tid & 63) == 0) {
            const int wi = e >> 5;
            if (wi < words) cand[wi] = (unsigned)bits;
            if (wi + 1 < words) cand[wi + 1] = (unsigned)(bits >> 32);
        }
    }
    if (init && p.votes)
        for (int e = tid; e < HW; e += kSelThreads) p.votes[(size_t)b * HW + e] = 0;
    __syncthreads();
    int hit = 0;
    for (int wi = tid; wi < words; wi += kSelThreads) {
        const int y = wi / wpr, wx = wi - y * wpr;
        unsigned r = 0;
        if (y >= y0 && y < y0 + P && wx == (x0 >> 5)) r = cand[wi] & (cell_bits << (x0 & 31));
        reach[wi] = r;
        hit |= r != 0;
    }
    const int seed_hit = __syncthreads_or(hit) ? 1 : 0;

    // Propagation.  A visit gives a word the reached bits of the words above and below and the edge bits of its row neighbours, masked by the candidates, and
    // fills inside the word; a sweep visits every word.  Words are updated in place while other threads read them: `reach` only ever gains bits, each a bit of the component (it is derived
    // from reached neighbours through candidates), so whichever value a reader sees the sweeps end at the same fixed point, the component itself.
    // BOUND: a sweep that changes anything sets at least one of the H W bits and none is ever cleared, so at most H W sweeps change something and sweep H W + 1
    // at the latest reports no change.  The loop runs at most H W + 1 times whatever the votes hold; a correct sweep never reaches the cap.
    // A thread owns runs of `rows` vertically adjacent words of one word column and walks each run down and then up, so that a sweep carries reached bits through
    // a whole run (and, within a word, along a whole row of it); between runs and between columns they travel one word per sweep.
    if (seed_hit) {
        const unsigned cap = (unsigned)HW + 1u;
        const int rows = (words + kSelThreads - 1) / kSelThreads, runs = (H + rows - 1) / rows, tasks = runs * wpr;
        auto visit = [&](int y, int wx) -> int {
            const int wi = y * wpr + wx;
            const unsigned c = cand[wi];
            if (!c) return 0;
            const unsigned r = reach[wi];
            unsigned nw = r;
            if (y > 0) nw |= reach[wi - wpr];
            if (y < H - 1) nw |= reach[wi + wpr];
            if (wx > 0) nw |= reach[wi - 1] >> 31;
            if (wx < wpr - 1) nw |= reach[wi + 1] << 31;
            nw = fill_word(nw & c, c);
            if (nw == r) return 0;
            reach[wi] = nw;
            return 1;
        };
        for (unsigned it = 0; it < cap; ++it) {
            int changed = 0;
            for (int t = tid; t < tasks; t += kSelThreads) {
                const int wx = t / runs, ya = (t - wx * runs) * rows, yb = min(ya + rows, H);
                for (int y = ya; y < yb; ++y) changed |= visit(y, wx);
                for (int y = yb - 2; y >= ya; --y) changed |= visit(y, wx);
            }
            if (!__syncthreads_or(changed)) break;
        }
    }

    int area = 0, ncand = 0;
    for (int wi = tid; wi < words; wi += kSelThreads) {
        area += __popc(reach[wi]);
        ncand += __popc(cand[wi]);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        area += __shfl_xor(area, o, 64);
        ncand += __shfl_xor(ncand, o, 64);
    }
    if ((tid & 63) == 0) red[0][tid >> 6] = area, red[1][tid >> 6] = ncand;
    if (p.segment)
        for (int e = tid; e < HW; e += kSelThreads) {
            const int y = e / W, x = e - y * W;
            p.segment[(size_t)b * HW + e] = (uint8_t)((reach[y * wpr + (x >> 5)] >> (x & 31)) & 1u);
        }
    for (int c = tid; c < n; c += kSelThreads) {
        const int cy = c / gw, cx = c - cy * gw, px = cx * P;
        int k = 0;
        for (int r = 0; r < P; ++r) k += __popc((reach[(cy * P + r) * wpr + (px >> 5)] >> (px & 31)) & cell_bits);
        cnt[c] = (unsigned short)k;
        if (p.cover) p.cover[(size_t)b * n + c] = (float)k / (float)(P * P);
    }
    __syncthreads();  // cnt and red are complete; nobody reads the bitmaps any more
    if (tid == 0 && p.stats) {
        int* st = p.stats + 4 * (size_t)b;
        st[0] = n_valid, st[1] = red[0][0] + red[0][1] + red[0][2] + red[0][3], st[2] = red[1][0] + red[1][1] + red[1][2] + red[1][3], st[3] = seed_hit;
    }
    if (p.k_active <= 0) return;

    // ---- selection ----
    unsigned long long* comp = seg_lds;  // the rank words, over the bitmaps
    const int R = min(p.ring_radius, max(gh, gw)), K = p.k_active + p.k_passive;
    const float pp = (float)(P * P);
    for (int c = tid; c < n; c += kSelThreads) {
        const int cy = c / gw, cx = c - cy * gw;
        int t = 0;
        for (int x = max(cx - R, 0); x <= min(cx + R, gw - 1); ++x) t |= cnt[cy * gw + x] != 0;
        rowt[c] = (unsigned char)t;
        sel[c] = 0;
    }
    const float* key_a = p.keys ? p.keys + (size_t)b * 2 * n : nullptr;
    const float* key_p = key_a ? key_a + n : nullptr;
    unsigned long long best = 0;
    for (int c = tid; c < n; c += kSelThreads) {
        const bool inside = (float)cnt[c] / pp >= p.inside_frac;
        const unsigned long long w = inside && c != c0 ? um_rank(1, key_a ? key_a[c] : 0.f, c) : 0ull;
        comp[c] = w;
        best = um_max64(best, w);
    }
    if (tid == (c0 & (kSelThreads - 1))) sel[c0] = 1;
    if (tid == 0 && p.picks) p.picks[(size_t)b * K] = n + c0;
    um_select_rounds(comp, n, p.k_active - 1, best, xch, [&](int r, int cell) {
        if (tid == 0 && p.picks) p.picks[(size_t)b * K + 1 + r] = cell < 0 ? -1 : n + cell;
        if (cell >= 0 && (cell & (kSelThreads - 1)) == tid) sel[cell] |= 1;
    });
    __syncthreads();  // rowt is complete (its writers passed this barrier) and xch is free again
    best = 0;
    for (int c = tid; c < n; c += kSelThreads) {
        const int cy = c / gw, cx = c - cy * gw;
        int t = 0;
        for (int y = max(cy - R, 0); y <= min(cy + R, gh - 1); ++y) t |= rowt[y * gw + cx];
        const unsigned long long w = t && cnt[c] == 0 ? um_rank(1, key_p ? key_p[c] : 0.f, c) : 0ull;
        comp[c] = w;
        best = um_max64(best, w);
    }
    um_select_rounds(comp, n, p.k_passive, best, xch, [&](int r, int cell) {
        if (tid == 0 && p.picks) p.picks[(size_t)b * K + p.k_active + r] = cell < 0 ? -1 : n + cell;
        if (cell >= 0 && (cell & (kSelThreads - 1)) == tid) sel[cell] |= 2;
    });
    __syncthreads();
    for (int k = tid; k < 2 * n; k += kSelThreads) {
        const unsigned char s = k < n ? 3 : sel[k - n];
        if (p.active_out) p.active_out[(size_t)b * 2 * n + k] = k < n ? 0 : (s & 1 ? 0 : 1);
        if (p.passive_out) p.passive_out[(size_t)b * 2 * n + k] = k < n ? 0 : (s & 2 ? 0 : 1);
    }
}

int words_per_row(int W) { return (W + 31) / 32; }

template <bool DIRS>
int launch_votes(const SegmentStepParams& p, const FlowView& v, FlowForm form, hipStream_t stream) {
    const int HW = p.H * p.W;
    if (form == VOTE_PACKED)
        hipLaunchKernelGGL(segment_vote_packed_kernel<DIRS>, dim3((unsigned)((HW + kVoteTilePix - 1) / kVoteTilePix), (unsigned)p.B), dim3(kVoteThreads), 0, stream, v.f, v.sb,
                           v.sc, HW, p.S, p.seed_ref, p.dirs, p.abs_thresh, p.rel_thresh, p.cos_min, p.votes);
    else if (form == VOTE_PLANES_VEC)
        hipLaunchKernelGGL(segment_vote_planes_kernel<DIRS>, dim3((unsigned)((HW / 4 + kVoteThreads - 1) / kVoteThreads), (unsigned)p.B), dim3(kVoteThreads), 0, stream, v.f,
                           v.sb, v.sc, v.ss, HW, p.S, p.seed_ref, p.dirs, p.abs_thresh, p.rel_thresh, p.cos_min, p.votes);
    else
        hipLaunchKernelGGL(segment_vote_strided_kernel<DIRS>, dim3((unsigned)((HW + kVoteThreads - 1) / kVoteThreads), (unsigned)p.B), dim3(kVoteThreads), 0, stream, v.f,
                           v.sb, v.sc, v.sh, v.sw, v.ss, HW, p.W, p.S, p.seed_ref, p.dirs, p.abs_thresh, p.rel_thresh, p.cos_min, p.votes);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

int check_segment_step(const SegmentStepParams& p) {
    const PatchGrid g = {p.B, 2, 0, p.H, p.W, p.P, 0, 0, 0};  // (B, T, H, W and P are all it reads; the entry point has checked base.T = 2)
    if (int rc = check_patch_grid("cwm_segment_step: base.", g, 0)) return rc;
    CWM_REQUIRE(p.B <= 65535, "cwm_segment_step: base.batch = %d, 1 .. 65535", p.B);
    CWM_REQUIRE((int64_t)p.H * p.W <= kSegmentMaxPixels, "cwm_segment_step: base.H base.W = %lld pixels, at most %d", (long long)p.H * p.W, kSegmentMaxPixels);
    CWM_REQUIRE((int64_t)p.H * words_per_row(p.W) <= kSegmentMaxWords, "cwm_segment_step: base.H = %d rows of %d words (base.W = %d), at most %d words of bit rows", p.H,
                words_per_row(p.W), p.W, kSegmentMaxWords);
    CWM_REQUIRE((p.H / p.P) * (p.W / p.P) <= kSelMaxCells, "cwm_segment_step: n = %d patches per frame, at most %d", (p.H / p.P) * (p.W / p.P), kSelMaxCells);
    CWM_REQUIRE(p.seeds, "cwm_segment_step: seeds_dev is required");
    if (p.f) {
        CWM_REQUIRE(p.S >= 1 && p.S <= kSegmentMaxSamples, "cwm_segment_step: S = %d, 1 .. %d (votes are bytes)", p.S, kSegmentMaxSamples);
        CWM_REQUIRE(p.votes, "cwm_segment_step: votes_dev is required when flows are given (the component pass reads it)");
        CWM_REQUIRE(p.seed_ref, "cwm_segment_step: seed_ref_dev is required when flows are given (the vote pass reads it)");
    } else {
        CWM_REQUIRE(p.S == 0, "cwm_segment_step: S = %d without flows_dev (the init step has S = 0)", p.S);
    }
    CWM_REQUIRE(p.k_active >= 0 && p.k_active <= kSegmentMaxPicks, "cwm_segment_step: k_active = %d, 0 .. %d", p.k_active, kSegmentMaxPicks);
    CWM_REQUIRE(p.k_passive >= 0 && p.k_passive <= kSegmentMaxPicks, "cwm_segment_step: k_passive = %d, 0 .. %d", p.k_passive, kSegmentMaxPicks);
    CWM_REQUIRE(p.ring_radius >= 1, "cwm_segment_step: ring_radius = %d, at least 1", p.ring_radius);
    CWM_REQUIRE(p.vote_frac == p.vote_frac, "cwm_segment_step: vote_frac is a NaN");
    return 0;
}

int launch_segment_step(const SegmentStepParams& p, hipStream_t stream) {
    if (int rc = check_segment_step(p)) return rc;
    const int wpr = words_per_row(p.W), words = p.H * wpr, n = (p.H / p.P) * (p.W / p.P);
    FlowView v{};
    FlowForm form = VOTE_STRIDED;
    if (p.f) {
        const int64_t st[5] = {p.sb, p.sc, p.sh, p.sw, p.ss};
        if (int rc = flow_view("cwm_segment_step", false, p.f, st, p.B, 2, p.H, p.W, p.S, &v)) return rc;
        form = flow_vote_form(v, flow_layout(v, (uintptr_t)p.votes));
    }
    const size_t lds = std::max((size_t)2 * words * sizeof(unsigned), (size_t)n * sizeof(unsigned long long));
    if (int rc = cwm_set_max_lds((const void*)segment_component_kernel, 2 * kSegmentMaxWords * (int)sizeof(unsigned))) return rc;
    if (p.f) {
        hipLaunchKernelGGL(segment_ref_kernel, dim3((unsigned)((p.B * p.S + 63) / 64)), dim3(64), 0, stream, v.f, v.sb, v.sc, v.sh, v.sw, v.ss, p.B, p.H, p.W, p.S, p.P,
                           p.seeds, p.min_seed_mag, p.seed_ref);
        CWM_HIP_CHECK(hipGetLastError());
        if (int rc = p.dirs ? launch_votes<true>(p, v, form, stream) : launch_votes<false>(p, v, form, stream)) return rc;
    }
    hipLaunchKernelGGL(segment_component_kernel, dim3((unsigned)p.B), dim3(kSelThreads), lds, stream, p, wpr, words);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace cwm

using namespace cwm;

extern "C" int cwm_segment_step(const cwm_segment_step_args* a) {
    CWM_REQUIRE(a && a->struct_size == sizeof(cwm_segment_step_args), "cwm_segment_step: args->struct_size must be sizeof(cwm_segment_step_args)");
    const cwm_patch_error_args& g = a->base;
    CWM_REQUIRE(g.T == 2, "cwm_segment_step: base.T = %d (two frames: the masks are [B, 2 n])", g.T);
    CWM_REQUIRE(!a->flows_dev || a->C == 2, "cwm_segment_step: flow samples have C = 2 channels, got C = %d", a->C);
    SegmentStepParams p;
    memset(&p, 0, sizeof(p));
    p.f = a->flows_dev;
    p.sb = a->flow_strides[0], p.sc = a->flow_strides[1], p.sh = a->flow_strides[2], p.sw = a->flow_strides[3], p.ss = a->flow_strides[4];
    p.B = g.batch, p.H = g.H, p.W = g.W, p.S = a->S, p.P = g.P;
    p.seeds = a->seeds_dev, p.dirs = a->dirs_dev;
    p.min_seed_mag = a->min_seed_mag, p.abs_thresh = a->abs_thresh, p.rel_thresh = a->rel_thresh, p.vote_frac = a->vote_frac, p.cos_min = a->cos_min;
    p.inside_frac = a->inside_frac;
    p.k_active = a->k_active, p.k_passive = a->k_passive, p.ring_radius = a->ring_radius;
    p.keys = a->keys_dev;
    p.seed_ref = a->seed_ref_dev, p.votes = a->votes_dev, p.segment = a->segment_dev, p.cover = a->cover_dev, p.stats = a->stats_dev, p.picks = a->picks_dev;
    p.active_out = a->active_out_dev, p.passive_out = a->passive_out_dev;
    return launch_segment_step(p, (hipStream_t)g.stream);
}
