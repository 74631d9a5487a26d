// Seed selection (cwm_seed_select): a score map -- a keypoint map, a movability map, the patch distribution of the scene loop -- becomes at most K well-spaced
// seed pixels per row: the strongest peaks first, or an exponential race in proportion to the map, both under non-maximum suppression and both excluding the
// neighbourhood of earlier seeds.  No counterpart in the reference, whose `sample_patches_from_energy` and `sample_and_visualize_keypoints` only ever sample.
//
// The definition (this is the contract; include/cwm_hip.h repeats it for callers).  Map: pixels [B,H,W] by a batch and a row stride, or cells [B,gh,gw]; patch
// size P, gh = H / P, gw = W / P, n = gh gw, cell c = i gw + j; free[b][c] bytes (none: all free); e[b][c] (given: race mode); prior[b][q] cells of earlier seeds;
// K, r = radius (Chebyshev, in cells), peaks_only, abs_thresh, rel_thresh.  Per row b, in this order:
//   1 pool        pixels form: v[c] = the maximum over the P P pixels of cell c, NaN pixels ignored; the seed pixel of c is the first pixel in row-major order that
//                 attains it (-0 and +0 are equal; v is that pixel's own value); a cell whose pixels are all NaN has v = NaN.
//                 cells form: v[c] = map[c]; the seed pixel is the cell's centre (i P + P/2, j P + P/2)
//   2 row maximum m = the maximum of v over the non-NaN cells of the row, free or not; a row without one has no candidates
//   3 threshold   t = abs_thresh if rel_thresh <= 0, else max(abs_thresh, rel_thresh * m): one fp32 multiply and one compare per test
//   4 peak        c is a peak iff v[c] is not a NaN and its word (um_order(v[c]), the lower index higher) is the maximum of the words of the non-NaN cells within
//                 Chebyshev distance r, free or not, the window clipped at the border: a plateau has exactly one peak per window, its lowest index
//   5 candidates  c is free, v[c] is not a NaN, v[c] >= t, c is a peak (with peaks_only), and no prior cell lies within Chebyshev distance r of c (r = 0: the
//                 prior cells themselves are excluded); prior entries outside 0 .. n-1 are ignored
//   6 key         v[c]; in race mode max(v[c], 0) / e[b][c], one correctly rounded division
//   7 selection   K rounds: the candidate that is first in the order of select_order.h (the higher key first, a NaN above every number, -0 equal to +0, the lower
//                 index first) is picked, then every candidate within Chebyshev distance r of it, itself included, is removed.  A round that finds no
//                 candidate is a dead slot: seed (-1, -1), cell -1, value 0
//   8 stats       (free non-NaN cells, candidates after step 5, picks made, 0)
//
// Two kernels on base.stream.  What was chosen, and why:
//   pool      grid (bands of cells, cell rows, B).  A cell belongs to P P / 4 adjacent lanes of ONE wave (4, 16 or 64: every P divides a wave), lane l of a cell
//             reads the 16 bytes at pixel row l / (P / 4), item l % (P / 4): the lanes of a wave read whole 64 .. 256-byte runs of an image row.  A lane folds its four pixels
//             in address order into a word (um_order(value), 255 - offset in the cell), the lanes of the cell fold theirs by xor shuffles: the word holds the
//             offset, so its maximum is the first pixel in row-major order whatever the lane layout.  The value travels with the word (so -0 stays -0).  One
//             workgroup per row of the batch would read a 224 x 224 map through one CU; this form has (gw / cells per group) gh B workgroups and no loop.
//             A map whose address or strides are not multiples of 16 bytes takes four scalar loads per lane in the same layout.  Every cell of the workspace is
//             written: the call does not depend on what work_dev holds on entry.  The cells form skips the pass
//   select    one workgroup of kSelThreads per row; v (16 KB), the rank words (32 KB) and the seed offsets (4 KB) in static LDS.  The peak test is a separable
//             windowed maximum of the rank words: a row pass into registers (a thread owns 16 cells), written back in place behind a barrier, then a column pass:
//             O(r) per cell and pass.  The rounds are um_select_rounds_removing (select_order.h): every thread clears its own cells in the picked window and
//             scans its cells again only if it cleared one.
// Loop bounds come from the geometry alone.  The only index taken from a table is the picked cell of a round, decoded from a rank word this kernel wrote for a
// cell below n, and the prior cells, which are tested against 0 .. n-1 and only ever compared: no map content moves an address.
#include <cstring>

#include "../../include/cwm_hip.h"
#include "common.h"
#include "kernels.h"
#include "select_order.h"

namespace cwm {

namespace {

constexpr int kCellsPerThread = kSelMaxCells / kSelThreads;
static_assert(kCellsPerThread * kSelThreads == kSelMaxCells && kCellsPerThread <= 32, "a thread's cells are one bit each of a 32-bit mask");

size_t seed_align16(size_t v) { return (v + 15) & ~(size_t)15; }
bool seed_sizes_ok(int B, int H, int W, int P) {
    if (!(P == 4 || P == 8 || P == 16) || B < 1 || B > 65535 || H <= 0 || W <= 0 || H % P || W % P) return false;
    return (int64_t)H * W <= kSeedMaxPixels && (H / P) * (W / P) <= kSelMaxCells;
}

// um_order of a number, undone (-0 comes back as +0)
__device__ __forceinline__ float seed_unorder(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }

// grid (ceil(gw / (256 / L)), gh, B), L = P P / 4 lanes per cell
template <int P>
__global__ __launch_bounds__(kSelThreads) void seed_pool_kernel(const float* __restrict__ map, int64_t sb, int64_t sr, int gw, int vec, float* __restrict__ pooled,
                                                                uint8_t* __restrict__ offset) {
    constexpr int Q = P / 4, L = P * Q, kCells = kSelThreads / L;
    static_assert(64 % L == 0, "the lanes of a cell lie in one wave");
    const int tid = threadIdx.x, l = tid % L, py = l / Q, q = l % Q;
    const int j = blockIdx.x * kCells + tid / L, i = blockIdx.y, b = blockIdx.z;
    unsigned long long word = 0;  // 0: no number yet
    float best = 0.f;
    if (j < gw) {
        const float* src = map + (int64_t)b * sb + (int64_t)(i * P + py) * sr + (j * P + 4 * q);
        float v[4];
        if (vec) {
            const float4 f = *reinterpret_cast<const float4*>(src);
            v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = src[u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (v[u] != v[u]) continue;
            const unsigned long long w = ((unsigned long long)um_order(v[u]) << 8) | (unsigned long long)(255 - (py * P + 4 * q + u));
            if (w > word) word = w, best = v[u];
        }
    }
#pragma unroll
    for (int o = L / 2; o; o >>= 1) {  // (every lane of the wave takes part; a cell past the grid holds 0 in all its lanes)
        const unsigned long long w = (unsigned long long)__shfl_xor((long long)word, o, 64);
        const float f = __shfl_xor(best, o, 64);
        if (w > word) word = w, best = f;
    }
    if (l == 0 && j < gw) {
        const size_t c = ((size_t)b * gridDim.y + i) * gw + j;
        pooled[c] = word ? best : __uint_as_float(0x7FC00000u);
        offset[c] = word ? (uint8_t)(255 - (int)(word & 255u)) : (uint8_t)0;
    }
}

// one workgroup per row
__global__ __launch_bounds__(kSelThreads) void seed_select_kernel(const SeedSelectParams p) {
    __shared__ unsigned long long comp[kSelMaxCells];  // rank words: of every non-NaN cell for the peak test, then of the candidates
    __shared__ float val[kSelMaxCells];
    __shared__ unsigned char off[kSelMaxCells];
    __shared__ unsigned long long xch[2][4];
    __shared__ int pri[kSeedMaxPrior];
    __shared__ int cnt[2][4];
    const int gw = p.W / p.P, gh = p.H / p.P, n = gh * gw, r = p.radius, P = p.P;
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)b * n;
    const float* vrow = (p.cells ? p.map : p.w_pooled) + row;
    if (tid < kSeedMaxPrior) {
        const int c = tid < p.n_prior ? p.prior[(size_t)b * p.n_prior + tid] : -1;
        pri[tid] = (c >= 0 && c < n) ? c : -1;
    }
    unsigned long long top = 0;
    for (int c = tid; c < n; c += kSelThreads) {
        const float v = vrow[c];
        val[c] = v;
        off[c] = p.cells ? (unsigned char)0 : p.w_offset[row + c];
        if (p.pooled) p.pooled[row + c] = v;
        const unsigned long long w = v != v ? 0ull : um_rank(1, v, c);
        comp[c] = w;
        top = um_max64(top, w);
    }
    top = um_block_max(top, xch[0]);  // (its barrier also orders comp, val, off and pri for every thread)
    const bool has = top != 0;
    const float m = seed_unorder((unsigned)(top >> 12));
    const float t = p.rel_thresh > 0.f ? fmaxf(p.abs_thresh, __fmul_rn(p.rel_thresh, m)) : p.abs_thresh;

    unsigned peak = 0;  // bit i: the thread's cell tid + i kSelThreads is a peak
    if (p.peaks || p.peaks_only) {
        unsigned long long rowmax[kCellsPerThread];
#pragma unroll
        for (int i = 0; i < kCellsPerThread; ++i) {
            const int c = tid + i * kSelThreads;
            unsigned long long mx = 0;
            if (c < n) {
                const int y = c / gw, x = c - y * gw;
                for (int xx = max(x - r, 0); xx <= min(x + r, gw - 1); ++xx) mx = um_max64(mx, comp[y * gw + xx]);
            }
            rowmax[i] = mx;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kCellsPerThread; ++i) {
            const int c = tid + i * kSelThreads;
            if (c < n) comp[c] = rowmax[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kCellsPerThread; ++i) {
            const int c = tid + i * kSelThreads;
            if (c < n) {
                const int y = c / gw, x = c - y * gw;
                unsigned long long mx = 0;
                for (int yy = max(y - r, 0); yy <= min(y + r, gh - 1); ++yy) mx = um_max64(mx, comp[yy * gw + x]);
                const float v = val[c];
                const bool is_peak = v == v && mx == um_rank(1, v, c);
                if (is_peak) peak |= 1u << i;
                if (p.peaks) p.peaks[row + c] = is_peak ? 1 : 0;
            }
        }
        __syncthreads();  // the words of the window maxima have been read: comp takes the candidates' words
    }

    int n_free = 0, n_cand = 0;
    unsigned long long best = 0;
#pragma unroll
    for (int i = 0; i < kCellsPerThread; ++i) {
        const int c = tid + i * kSelThreads;
        if (c >= n) continue;
        const float v = val[c];
        const bool number = v == v, is_free = !p.free || p.free[row + c] != 0;
        n_free += number && is_free;
        bool cand = has && number && is_free && v >= t && (!p.peaks_only || ((peak >> i) & 1u));
        if (cand) {
            const int y = c / gw, x = c - y * gw;
            for (int q = 0; q < p.n_prior; ++q) {
                const int pc = pri[q];
                if (pc < 0) continue;
                const int py = pc / gw, px = pc - py * gw;
                if (abs(y - py) <= r && abs(x - px) <= r) cand = false;
            }
        }
        unsigned long long w = 0;
        if (cand) {
            const float key = p.e ? __fdiv_rn(fmaxf(v, 0.f), p.e[row + c]) : v;
            w = um_rank(1, key, c);
        }
        n_cand += cand;
        comp[c] = w;
        best = um_max64(best, w);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) n_free += __shfl_xor(n_free, o, 64), n_cand += __shfl_xor(n_cand, o, 64);
    if ((tid & 63) == 0) cnt[0][tid >> 6] = n_free, cnt[1][tid >> 6] = n_cand;  // (read by thread 0 behind the barriers of the rounds; K >= 1)

    int n_picks = 0;
    um_select_rounds_removing(
        comp, n, p.K, best, xch,
        [&](int rd, int cell) {
            if (tid != 0) return;
            const size_t slot = (size_t)b * p.K + rd;
            if (p.picks) p.picks[slot] = cell;
            if (p.values) p.values[slot] = cell < 0 ? 0.f : val[cell];
            if (p.seeds) {
                int y = -1, x = -1;
                if (cell >= 0) {
                    const int ci = cell / gw, cj = cell - ci * gw, o = off[cell];
                    y = ci * P + (p.cells ? P / 2 : o / P), x = cj * P + (p.cells ? P / 2 : o % P);
                }
                p.seeds[2 * slot] = y, p.seeds[2 * slot + 1] = x;
            }
            n_picks += cell >= 0;
        },
        [&](int cell, int c) {
            const int cy = cell / gw, cx = cell - cy * gw, y = c / gw, x = c - y * gw;
            return abs(y - cy) <= r && abs(x - cx) <= r;
        });
    if (tid == 0 && p.stats) {
        int* st = p.stats + 4 * (size_t)b;
        st[0] = cnt[0][0] + cnt[0][1] + cnt[0][2] + cnt[0][3], st[1] = cnt[1][0] + cnt[1][1] + cnt[1][2] + cnt[1][3], st[2] = n_picks, st[3] = 0;
    }
}

}  // namespace

int launch_seed_pool(const SeedSelectParams& p, hipStream_t stream) {
    const int gw = p.W / p.P, gh = p.H / p.P, per_group = kSelThreads / (p.P * p.P / 4);
    const int vec = (reinterpret_cast<uintptr_t>(p.map) & 15) == 0 && p.sb % 4 == 0 && p.sr % 4 == 0;
    const dim3 grid((unsigned)((gw + per_group - 1) / per_group), (unsigned)gh, (unsigned)p.B), block(kSelThreads);
    if (p.P == 4)
        hipLaunchKernelGGL(seed_pool_kernel<4>, grid, block, 0, stream, p.map, p.sb, p.sr, gw, vec, p.w_pooled, p.w_offset);
    else if (p.P == 8)
        hipLaunchKernelGGL(seed_pool_kernel<8>, grid, block, 0, stream, p.map, p.sb, p.sr, gw, vec, p.w_pooled, p.w_offset);
    else
        hipLaunchKernelGGL(seed_pool_kernel<16>, grid, block, 0, stream, p.map, p.sb, p.sr, gw, vec, p.w_pooled, p.w_offset);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_seed_select(const SeedSelectParams& p, hipStream_t stream) {
    if (!p.cells)
        if (int rc = launch_seed_pool(p, stream)) return rc;
    hipLaunchKernelGGL(seed_select_kernel, dim3((unsigned)p.B), dim3(kSelThreads), 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace cwm

using namespace cwm;

extern "C" size_t cwm_seed_select_work_bytes(int B, int H, int W, int P) {
    if (!seed_sizes_ok(B, H, W, P)) return 0;
    const size_t cells = (size_t)B * (H / P) * (W / P);
    return seed_align16(cells * sizeof(float)) + seed_align16(cells);
}

extern "C" int cwm_seed_select(const cwm_seed_select_args* a) {
    CWM_REQUIRE(a && a->struct_size == sizeof(cwm_seed_select_args), "cwm_seed_select: args->struct_size must be sizeof(cwm_seed_select_args)");
    const cwm_patch_error_args& g = a->base;
    const PatchGrid grid = {g.batch, 1, 0, g.H, g.W, g.P, 0, 0, 0};
    if (int rc = check_patch_grid("cwm_seed_select: base.", grid, 0)) return rc;
    CWM_REQUIRE(g.batch <= 65535, "cwm_seed_select: base.batch = %d, 1 .. 65535", g.batch);
    CWM_REQUIRE((int64_t)g.H * g.W <= kSeedMaxPixels, "cwm_seed_select: base.H base.W = %lld pixels, at most %d", (long long)g.H * g.W, kSeedMaxPixels);
    const int n = (g.H / g.P) * (g.W / g.P);
    CWM_REQUIRE(n <= kSelMaxCells, "cwm_seed_select: n = %d patches per frame, at most %d", n, kSelMaxCells);
    CWM_REQUIRE(a->map_dev, "cwm_seed_select: map_dev is required");
    CWM_REQUIRE(a->cells == 0 || a->cells == 1, "cwm_seed_select: cells = %d, 0 (a pixel map) or 1 (one value per cell)", a->cells);
    CWM_REQUIRE(a->K >= 1 && a->K <= kSeedMaxPicks, "cwm_seed_select: K = %d, 1 .. %d", a->K, kSeedMaxPicks);
    CWM_REQUIRE(a->radius >= 0 && a->radius <= kSeedMaxRadius, "cwm_seed_select: radius = %d, 0 .. %d", a->radius, kSeedMaxRadius);
    CWM_REQUIRE(a->n_prior >= 0 && a->n_prior <= kSeedMaxPrior, "cwm_seed_select: n_prior = %d, 0 .. %d", a->n_prior, kSeedMaxPrior);
    CWM_REQUIRE(a->n_prior == 0 || a->prior_dev, "cwm_seed_select: prior_dev is required with n_prior = %d", a->n_prior);
    CWM_REQUIRE(a->peaks_only == 0 || a->peaks_only == 1, "cwm_seed_select: peaks_only = %d, 0 or 1", a->peaks_only);
    CWM_REQUIRE(a->abs_thresh == a->abs_thresh, "cwm_seed_select: abs_thresh must not be a NaN (-inf disables it)");
    CWM_REQUIRE(a->rel_thresh - a->rel_thresh == 0.f, "cwm_seed_select: rel_thresh must be finite (<= 0 disables it)");
    CWM_REQUIRE(a->seeds_dev || a->cells_dev || a->values_dev || a->pooled_dev || a->peaks_dev || a->stats_dev, "cwm_seed_select: no output requested");
    SeedSelectParams p;
    memset(&p, 0, sizeof(p));
    if (!a->cells) {
        CWM_REQUIRE(a->map_strides[0] >= 0 && a->map_strides[1] >= g.W, "cwm_seed_select: map_strides = (%lld, %lld): a batch stride that is not negative and a row stride of at least W",
                    (long long)a->map_strides[0], (long long)a->map_strides[1]);
        CWM_REQUIRE(a->work_dev && (reinterpret_cast<uintptr_t>(a->work_dev) & 15) == 0, "cwm_seed_select: work_dev = %p must be a 16-byte aligned device address", a->work_dev);
        const size_t need = cwm_seed_select_work_bytes(g.batch, g.H, g.W, g.P);
        CWM_REQUIRE(a->work_bytes >= need, "cwm_seed_select: work_bytes = %llu, cwm_seed_select_work_bytes gives %llu", (unsigned long long)a->work_bytes,
                    (unsigned long long)need);
        p.sb = a->map_strides[0], p.sr = a->map_strides[1];
        p.w_pooled = static_cast<float*>(a->work_dev);
        p.w_offset = static_cast<uint8_t*>(a->work_dev) + seed_align16((size_t)g.batch * n * sizeof(float));
    }
    p.map = a->map_dev, p.cells = a->cells;
    p.B = g.batch, p.H = g.H, p.W = g.W, p.P = g.P;
    p.free = a->free_dev, p.e = a->e_dev, p.prior = a->n_prior ? a->prior_dev : nullptr;
    p.n_prior = a->n_prior, p.K = a->K, p.radius = a->radius, p.peaks_only = a->peaks_only;
    p.abs_thresh = a->abs_thresh, p.rel_thresh = a->rel_thresh;
    p.seeds = a->seeds_dev, p.picks = a->cells_dev, p.values = a->values_dev, p.pooled = a->pooled_dev, p.peaks = a->peaks_dev, p.stats = a->stats_dev;
    return launch_seed_select(p, (hipStream_t)g.stream);
}
