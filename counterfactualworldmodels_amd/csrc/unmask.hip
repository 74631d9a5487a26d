// Frontier unmasking (cwm_unmask_step): the L-inf distance transform of a frame's mask grid, the frontier it defines, and the reveal of the k highest-keyed
// masked cells of every batch row -- all of one row's state in the LDS of one workgroup.
#include "common.h"
#include "kernels.h"
#include "select_order.h"
#include <climits>

namespace cwm {

namespace {

constexpr int kThreads = kSelThreads;
static_assert(kUnmaskMaxCells == kSelMaxCells, "the rank word keeps the cell index in 12 bits");
constexpr unsigned kNoGap = 0xFFFFu;  // no visible cell in the column (a real gap is below h <= 1365)

}  // namespace

// ---------------------------------------------------------------------------------------------
// Reference: `patch_distance_transform` cwm/models/masking.py:32-56, `patches_adjacent_to_visible` :58-71 (the integer-radius branch: d <= threshold).
// One workgroup per batch row b, frame f of its mask: n = gh gw <= 4096 cells.
//
// Distance.  With sy = (gh-1)/2, sx = (gw-1)/2 the reference takes d(p) = min_v max(|py-vy| / sy, |px-vx| / sx) over the visible cells v, every quotient
// rounded to fp32.  Rounding is monotone, so d(p) is the rounded quotient of the smallest rational, and that rational is found in integers: a column pass
// gives g(y, x') = the vertical gap from row y to the nearest visible cell of column x', a row pass K(y, x) = min_x' max(g sx, |x-x'| sy) -- the numerator
// over the common denominator sy sx.  d = float(K) / float(sy sx): K and sy sx are exact in fp32 (< 2^24) and the division is correctly rounded, which is
// the reference's float(a) / float(sy) or float(b) / float(sx) of the same rational.  No visible cell: d = 0 everywhere.  self_mask: the visible cells
// get the grid's maximum (an integer maximum of K, then the one division).
//
// Selection.  A masked cell's key is err = map[b][f][cell] (times region[b][f][cell]) or, in race mode, max(err, 0) / e[b][cell] with a NaN err kept; the
// cells are ranked by (frontier before the other masked cells, key descending with NaN first and -0 == +0, index ascending) packed into one 64-bit word,
// and k rounds of arg-max take the first k.  A round is a scan of the thread's own cells (only by the thread that owned the last pick), xor shuffles and
// one LDS exchange.  Fixed order, no atomics.  Every index is computed from the thread index and the geometry: no mask content moves an address.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void unmask_select_kernel(const UnmaskStepParams p) {
    __shared__ unsigned long long comp[kUnmaskMaxCells];  // rank word of a cell; 0: visible, or picked
    __shared__ unsigned short gap[kUnmaskMaxCells];
    __shared__ unsigned char m[kUnmaskMaxCells];          // the frame's mask bytes, picks cleared as they are made
    __shared__ unsigned long long xch[2][4];
    const int gw = p.gw, gh = p.gh, n = gh * gw;
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t Nt = (size_t)p.T * n;
    const uint8_t* mrow = p.mask + b * Nt + (size_t)p.frame * n;
    for (int c = tid; c < n; c += kThreads) m[c] = mrow[c];
    __syncthreads();
    for (int c = tid; c < n; c += kThreads) {
        const int y = c / gw, x = c - y * gw;
        int g = kNoGap;
        for (int vy = 0; vy < gh; ++vy)
            if (m[vy * gw + x] == 0) g = min(g, abs(y - vy));
        gap[c] = (unsigned short)g;
    }
    __syncthreads();
    const int sy = (gh - 1) / 2, sx = (gw - 1) / 2;
    const float den = (float)(sy * sx);
    const float thr = p.threshold ? p.threshold[0] : -1.f;
    unsigned long long kmax = 0;
    for (int c = tid; c < n; c += kThreads) {
        const int y = c / gw, x = c - y * gw;
        int K = INT_MAX;
        for (int vx = 0; vx < gw; ++vx) {
            const int g = gap[y * gw + vx];
            if (g != (int)kNoGap) K = min(K, max(g * sx, abs(x - vx) * sy));
        }
        if (K == INT_MAX) K = 0;  // a grid without a visible cell
        comp[c] = (unsigned long long)K;
        kmax = um_max64(kmax, (unsigned long long)K);
    }
    kmax = um_block_max(kmax, xch[0]);  // (its barrier also orders comp for nobody yet: every thread reads back its own cells only)
    const float dmax = __fdiv_rn((float)(int)kmax, den);
    const float* erow = p.map ? p.map + ((size_t)b * p.T + p.frame) * n : nullptr;
    const float* rrow = p.region ? p.region + ((size_t)b * p.T + p.frame) * n : nullptr;
    unsigned long long best = 0;
    for (int c = tid; c < n; c += kThreads) {
        const float d = __fdiv_rn((float)(int)comp[c], den);
        const bool masked = m[c] != 0;
        const bool front = masked && (thr < 0.f || d <= thr);
        if (p.dist) p.dist[(size_t)b * n + c] = (!masked && p.self_mask) ? dmax : d;
        if (p.frontier) p.frontier[(size_t)b * n + c] = front ? 1 : 0;
        unsigned long long w = 0;
        if (masked && p.k > 0) {
            float key = erow[c];
            if (rrow) key = key * rrow[c];
            if (p.race) key = key != key ? key : __fdiv_rn(fmaxf(key, 0.f), p.e[(size_t)b * n + c]);
            w = um_rank(front ? 2 : 1, key, c);
        }
        comp[c] = w;
        best = um_max64(best, w);
    }
    um_select_rounds(comp, n, p.k, best, xch, [&](int r, int cell) {
        if (tid == 0 && p.picks) p.picks[(size_t)b * p.k + r] = cell < 0 ? -1 : p.frame * n + cell;
        if (cell >= 0 && (cell & (kThreads - 1)) == tid) m[cell] = 0;  // the owner clears the cell
    });
    if (p.mask_out) {
        __syncthreads();
        const uint8_t* src = p.mask + b * Nt;
        uint8_t* dst = p.mask_out + b * Nt;
        const size_t f0 = (size_t)p.frame * n;
        for (size_t k = tid; k < Nt; k += kThreads) dst[k] = (k >= f0 && k < f0 + n) ? m[k - f0] : src[k];
    }
}

int check_unmask_select(const UnmaskStepParams& p) {
    CWM_REQUIRE(p.mask && p.B > 0 && p.T > 0, "unmask_step: mask_dev, a positive batch and T are required");
    CWM_REQUIRE(p.gh >= 3 && p.gw >= 3, "unmask_step: a grid of at least 3 x 3 patches (the reference divides by (h-1)//2 and (w-1)//2), got %d x %d", p.gh, p.gw);
    CWM_REQUIRE((int64_t)p.gh * p.gw <= kUnmaskMaxCells, "unmask_step: at most %d patches per frame, got %d x %d", kUnmaskMaxCells, p.gh, p.gw);
    CWM_REQUIRE(p.frame >= 0 && p.frame < p.T, "unmask_step: frame = %d of %d (one frame, 0 .. T-1)", p.frame, p.T);
    CWM_REQUIRE(p.k >= 0 && p.k <= kUnmaskMaxReveal, "unmask_step: num_reveal = %d, 0 .. %d", p.k, kUnmaskMaxReveal);
    CWM_REQUIRE(p.k == 0 || p.map, "unmask_step: the error map is required when a cell is revealed");
    CWM_REQUIRE(p.k == 0 || !p.race || p.e, "unmask_step: race mode needs e_dev ([B, n] exponential draws)");
    CWM_REQUIRE(p.dist || p.frontier || (p.k > 0 && (p.picks || p.mask_out)), "unmask_step: no output requested");
    if (p.mask_out) {
        const size_t bytes = (size_t)p.B * p.T * p.gh * p.gw;
        const uintptr_t a = (uintptr_t)p.mask, o = (uintptr_t)p.mask_out;
        CWM_REQUIRE(o + bytes <= a || a + bytes <= o, "unmask_step: mask_out_dev must not alias base.mask_dev");
    }
    return 0;
}

int launch_unmask_select(const UnmaskStepParams& p, hipStream_t stream) {
    if (int rc = check_unmask_select(p)) return rc;
    hipLaunchKernelGGL(unmask_select_kernel, dim3((unsigned)p.B), dim3(kThreads), 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace cwm
