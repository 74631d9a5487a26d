// Motion parallax (cwm_parallax): from S flow samples of a scene under S different motions of the viewer to a per-pixel parallax map -- how far the pixel moves
// along a reference motion, as a multiple of it, the median over the samples -- and a per-slot histogram of it with its order statistics: a depth cue for every
// pixel and every slot, where object_motion's occlusion order speaks only about pairs of objects that cross.  No counterpart in the reference, whose README
// lists "using counterfactuals to estimate other scene properties" as coming.
//
// The definition is the comment of cwm_parallax in include/cwm_hip.h: seven numbered steps, each an integer operation or ONE correctly rounded binary64 (at the
// very end binary32) operation; this file is compiled without contraction.  What is particular to the kernels:
//   reference   grid (chunks of 1024 pixels, S, R), 256 threads, 4 consecutive pixels of one image row per thread, only without dirs_dev.  The sums of qu, qv
//               and 1 over the usable pixels (of ref_slot) are added over the wave (wave_sum.h; a lane holds at most 2^22, a wave 2^28), by one lane per wave into
//               LDS and by three threads as INTEGER atomics into ref_dev, which holds (SU, SV, N, 0) as int64 until the finalise pass turns the row into
//               (mu, mv, den, live).  Two instantiations, chosen by the host: 16-byte loads of u and v (and 4-byte label loads) where the view has contiguous
//               planes on their alignment -- the `_batch_to_samples` view of the flow model's output --, a scalar form through all five strides otherwise
//   pixels      grid (chunks of kThreads pixels, R).  A thread owns ONE pixel: its S projections are a column of an LDS array [kCap][kThreads] of doubles (lane
//               i reads bank pair i whatever the row: no conflict), because a per-thread array indexed by a run-time value would live in scratch.  Four pixels
//               per thread would need four such columns; adjacent lanes read adjacent floats instead, a wave one 256-byte line per load on contiguous planes,
//               and the same code walks any other strides.  (kThreads, kCap) = (256, 8), (256, 16), (128, 32), (64, 64) by S: at most 32 KB of LDS.  The order
//               statistics come from ranking by counting: the rank of sample s is the number of t with p_t < p_s or (p_t == p_s and t < s) -- the stable
//               order of the definition --, four candidates at a time in registers (compile-time indices) against one LDS read per t.  A sample that does not
//               count is stored as a NaN, which no comparison counts.  The across values take the same column in a second pass over the (cached) flows.
//               The histogram of the slot of the workgroup's first pixel is gathered in LDS (1 KB) and flushed once; pixels of other slots add to memory
//               directly.  Every count reaches hist_dev / slot_tab_dev as an INTEGER atomic
//   finalise    grid (R, 17), 256 threads: block (r, 0) turns ref_dev's row into doubles; wave w of block (r, y) owns slot 4 y + w: lane i loads bins 4 i .. 4 i + 3
//               with one 16-byte load, an inclusive scan over the lanes gives the cumulative counts, and the lane whose range holds an order statistic writes
//               its bin
// Integer atomics give the same bits in any order: two calls on the same inputs give the same bits.  No content of a device buffer moves an address beyond what
// the geometry allows: a label byte is tested against 64 before it indexes a table, a bin is clamped as a double before it is converted.
#include <cstring>

#include "../../include/cwm_hip.h"
#include "common.h"
#include "flow_view.h"
#include "wave_sum.h"

#pragma clang fp contract(off)

namespace cwm {

namespace {

constexpr int kParSlots = 64;
constexpr int kParSide = kParSlots + 1;  // slots 0 .. 64
constexpr int kParBins = 256;
constexpr int kParTerms = 8;
constexpr int kParMaxPixels = 1 << 18;
constexpr int kParMaxSamples = 64;
constexpr long long kParMaxRefQ = 1 << 21;
constexpr int kParRefThreads = 256;
constexpr int kParRefGroupPixels = 4 * kParRefThreads;  // 4 pixels per thread
constexpr int kParFinThreads = 256;
constexpr int kParFinBlocks = (kParSide + 3) / 4;  // a wave per slot

struct ParParams {
    const float* flows;
    int64_t sb, sc, sh, sw, ss;
    const int* dirs;
    const uint8_t* labels;
    int64_t ls;
    int R, H, W, S;
    int ref_slot, min_pixels, min_samples;
    double min_den;
    float *par, *spread, *off;
    uint8_t* cnt;
    double* ref;
    int* hist;
    int* slot_tab;
};

// step 1 and 2 for one flow vector
__device__ __forceinline__ bool par_quantise(float u, float v, int& qu, int& qv) {
    const bool usable = fabsf(u) <= 4096.f && fabsf(v) <= 4096.f;  // (false for a NaN and for an inf)
    qu = usable ? (int)rintf(u * 256.0f) : 0, qv = usable ? (int)rintf(v * 256.0f) : 0;
    return usable;
}

// step 3 for (r, s), from dirs or from the sums the reference kernel left in ref_dev
__device__ __forceinline__ bool par_reference(const ParParams& p, int r, int s, double& mu, double& mv, double& den) {
    long long N;
    if (p.dirs) {
        mu = (double)(256LL * p.dirs[2 * s + 1]), mv = (double)(256LL * p.dirs[2 * s]);
        N = (long long)p.H * p.W;
    } else {
        const long long* t = reinterpret_cast<const long long*>(p.ref) + ((size_t)r * p.S + s) * 4;
        const long long SU = t[0], SV = t[1];
        N = t[2];
        mu = N ? (double)SU / (double)N : 0.0, mv = N ? (double)SV / (double)N : 0.0;
    }
    const double uu = mu * mu, vv = mv * mv;
    den = uu + vv;
    return N >= (long long)p.min_pixels && den >= p.min_den;
}

// grid (chunks of 1024 pixels, S, R).  kVec: contiguous planes, the flow planes of every (row, channel, sample) 16-byte aligned and the label planes 4-byte
// aligned (the host decides)
template <bool kVec>
__global__ __launch_bounds__(kParRefThreads) void parallax_reference_kernel(const ParParams p) {
    __shared__ unsigned long long sum_s[3];
    const int s = blockIdx.y, r = blockIdx.z, tid = threadIdx.x, W = p.W, quads = (p.H * W) >> 2;
    if (tid < 3) sum_s[tid] = 0;
    __syncthreads();
    const bool by_slot = p.ref_slot >= 0;  // (the host has seen to it that labels are there)
    const uint8_t* lab = p.labels + r * p.ls;
    const float* fu = p.flows + r * p.sb + s * p.ss;
    const float* fv = fu + p.sc;
    const int g = blockIdx.x * kParRefThreads + tid;  // the group of 4 pixels
    int su = 0, sv = 0, n = 0;
    if (g < quads) {
        const int pix = 4 * g;
        unsigned lw = 0;
        float u[4], v[4];
        if (kVec) {
            if (by_slot) lw = *reinterpret_cast<const unsigned*>(lab + pix);
            const float4 tu = *reinterpret_cast<const float4*>(fu + pix), tv = *reinterpret_cast<const float4*>(fv + pix);
            u[0] = tu.x, u[1] = tu.y, u[2] = tu.z, u[3] = tu.w;
            v[0] = tv.x, v[1] = tv.y, v[2] = tv.z, v[3] = tv.w;
        } else {
            const int y = pix / W, x0 = pix - y * W;  // W is a multiple of 4: the four pixels lie in one image row
            const int64_t o = y * p.sh + x0 * p.sw;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (by_slot) lw |= (unsigned)lab[pix + j] << (8 * j);
                u[j] = fu[o + j * p.sw], v[j] = fv[o + j * p.sw];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = (int)((lw >> (8 * j)) & 0xffu);
            const int l = q <= kParSlots ? q : 0;
            int qu, qv;
            const bool usable = par_quantise(u[j], v[j], qu, qv);
            if (usable && (!by_slot || l == p.ref_slot)) su += qu, sv += qv, n += 1;
        }
    }
    su = wave_sum(su), sv = wave_sum(sv), n = wave_sum(n);  // (every lane takes part, one past the plane with zeros)
    if ((tid & 63) == 0 && n) {
        atomicAdd(&sum_s[0], (unsigned long long)(long long)su);
        atomicAdd(&sum_s[1], (unsigned long long)(long long)sv);
        atomicAdd(&sum_s[2], (unsigned long long)n);
    }
    __syncthreads();
    if (tid < 3) {
        const unsigned long long t = sum_s[tid];
        if (t) atomicAdd(reinterpret_cast<unsigned long long*>(p.ref) + ((size_t)r * p.S + s) * 4 + tid, t);
    }
}

// The order statistics of the column `col` (S entries, kThreads doubles apart; a NaN does not count; n >= 1 of them count): the entries of rank (n-1)/4, (n-1)/2
// and 3(n-1)/4 in the stable ascending order.  The ranks are a permutation of 0 .. n-1, so each is found exactly once
template <int kThreads>
__device__ __forceinline__ void par_select(const double* col, int S, int n, double& q1, double& med, double& q3) {
    const int k1 = (n - 1) / 4, k2 = (n - 1) / 2, k3 = (3 * (n - 1)) / 4;
    for (int s0 = 0; s0 < S; s0 += 4) {
        double a[4];
        int rk[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = s0 + j < S ? col[(s0 + j) * kThreads] : __builtin_nan("");
            rk[j] = 0;
        }
        for (int t = 0; t < S; ++t) {
            const double pt = col[t * kThreads];
#pragma unroll
            for (int j = 0; j < 4; ++j) rk[j] += (pt < a[j] || (pt == a[j] && t < s0 + j)) ? 1 : 0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (a[j] == a[j]) {
                if (rk[j] == k1) q1 = a[j];
                if (rk[j] == k2) med = a[j];
                if (rk[j] == k3) q3 = a[j];
            }
        }
    }
}

// grid (chunks of kThreads pixels, R); S <= kCap
template <int kThreads, int kCap>
__global__ __launch_bounds__(kThreads) void parallax_pixel_kernel(const ParParams p) {
    __shared__ double buf_s[kCap * kThreads];
    __shared__ double ref_s[kCap * 3];  // (mu, mv, den); den = 0 for a sample that is not live (a live one has den >= min_ref_q^2 >= 1)
    __shared__ int hist_s[kParBins + 1];  // the workgroup's first slot: its bins, then its pixels without a parallax
    const int r = blockIdx.y, tid = threadIdx.x, S = p.S, HW = p.H * p.W;
    for (int e = tid; e <= kParBins; e += kThreads) hist_s[e] = 0;
    if (tid < S) {  // (S <= 64 <= kThreads)
        double mu, mv, den;
        const bool live = par_reference(p, r, tid, mu, mv, den);
        ref_s[3 * tid] = mu, ref_s[3 * tid + 1] = mv, ref_s[3 * tid + 2] = live ? den : 0.0;
    }
    __syncthreads();
    const int first = blockIdx.x * kThreads;  // (inside the plane: the grid is ceil(H W / kThreads))
    const int pix = first + tid;
    const bool inside = pix < HW;
    const int pc = inside ? pix : first;  // a thread past the plane walks the first pixel again and writes nothing
    const int y = pc / p.W, x = pc - y * p.W;
    const float* fu = p.flows + r * p.sb + y * p.sh + x * p.sw;
    const float* fv = fu + p.sc;
    int l = 0, slot0 = 0;
    if (p.labels) {
        const uint8_t* lab = p.labels + r * p.ls;
        const int q = lab[pc], q0 = lab[first];
        l = q <= kParSlots ? q : 0, slot0 = q0 <= kParSlots ? q0 : 0;
    }
    double* col = buf_s + tid;
    const double nan = __builtin_nan("");
    int n = 0;
    for (int s = 0; s < S; ++s) {  // steps 1, 2 and 4: along
        int qu, qv;
        const bool usable = par_quantise(fu[s * p.ss], fv[s * p.ss], qu, qv);
        const double mu = ref_s[3 * s], mv = ref_s[3 * s + 1], den = ref_s[3 * s + 2];
        double val = nan;
        if (usable && den > 0.0) {
            const double a = (double)qu * mu, b = (double)qv * mv;
            val = (a + b) / den;
            n += 1;
        }
        col[s * kThreads] = val;
    }
    const bool good = n >= p.min_samples;  // (min_samples >= 1)
    double q1 = 0.0, med = 0.0, q3 = 0.0, cmed = 0.0;
    if (good) par_select<kThreads>(col, S, n, q1, med, q3);
    if (p.off && good) {  // across: the same column once more
        for (int s = 0; s < S; ++s) {
            int qu, qv;
            const bool usable = par_quantise(fu[s * p.ss], fv[s * p.ss], qu, qv);
            const double mu = ref_s[3 * s], mv = ref_s[3 * s + 1], den = ref_s[3 * s + 2];
            double val = nan;
            if (usable && den > 0.0) {
                const double a = (double)qu * mv, b = (double)qv * mu;
                val = fabs(a - b) / den;
            }
            col[s * kThreads] = val;
        }
        double c1, c3;
        par_select<kThreads>(col, S, n, c1, cmed, c3);
    }
    if (inside) {
        const size_t o = (size_t)r * HW + pix;
        const float fnan = __builtin_nanf("");
        p.par[o] = good ? (float)med : fnan;
        if (p.spread) p.spread[o] = good ? (float)(q3 - q1) : fnan;
        if (p.off) p.off[o] = good ? (float)cmed : fnan;
        if (p.cnt) p.cnt[o] = (uint8_t)n;
        if (p.labels) {  // step 6
            double b = floor(med * 32.0) + 128.0;
            b = b < 0.0 ? 0.0 : (b > 255.0 ? 255.0 : b);
            const int bin = good ? (int)b : kParBins;
            if (l == slot0) atomicAdd(&hist_s[bin], 1);
            else if (good) atomicAdd(&p.hist[((size_t)r * kParSide + l) * kParBins + bin], 1);
            else atomicAdd(&p.slot_tab[((size_t)r * kParSide + l) * kParTerms + 1], 1);
        }
    }
    __syncthreads();
    if (p.labels) {
        for (int e = tid; e <= kParBins; e += kThreads) {
            const int t = hist_s[e];
            if (!t) continue;
            if (e < kParBins) atomicAdd(&p.hist[((size_t)r * kParSide + slot0) * kParBins + e], t);
            else atomicAdd(&p.slot_tab[((size_t)r * kParSide + slot0) * kParTerms + 1], t);
        }
    }
}

// the bin of the order statistic k, if this lane's four bins (c0 .. c3, cumulative counts `below` before and `upto` after them) hold it: step 7
__device__ __forceinline__ void par_bin_of(int k, int lane, int below, int upto, int c0, int c1, int c2, int* out) {
    if (k < below || k >= upto) return;
    int b = 4 * lane, cum = below + c0;
    if (cum <= k) {
        b += 1, cum += c1;
        if (cum <= k) {
            b += 1, cum += c2;
            if (cum <= k) b += 1;
        }
    }
    *out = b;
}

// grid (R, 17), 256 threads
__global__ __launch_bounds__(kParFinThreads) void parallax_finalise_kernel(const ParParams p) {
    const int r = blockIdx.x, tid = threadIdx.x;
    if (blockIdx.y == 0 && tid < p.S) {  // a thread reads the sums of its own sample before it writes over them
        double mu, mv, den;
        const bool live = par_reference(p, r, tid, mu, mv, den);
        double* o = p.ref + ((size_t)r * p.S + tid) * 4;
        o[0] = mu, o[1] = mv, o[2] = den, o[3] = live ? 1.0 : 0.0;
    }
    if (!p.labels) return;
    const int l = blockIdx.y * 4 + (tid >> 6), lane = tid & 63;
    if (l >= kParSide) return;  // (a whole wave)
    const int4 h = *reinterpret_cast<const int4*>(p.hist + ((size_t)r * kParSide + l) * kParBins + 4 * lane);
    const int tot = h.x + h.y + h.z + h.w;
    int upto = tot;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(upto, d, 64);
        if (lane >= d) upto += t;
    }
    const int below = upto - tot, n = __shfl(upto, 63, 64);
    int* out = p.slot_tab + ((size_t)r * kParSide + l) * kParTerms;  // (entry 1 holds what the pixels added, entry 7 the zero of the memset)
    if (n == 0) {
        if (lane < 5) out[2 + lane] = -1;
        if (lane == 5) out[0] = 0;
        return;
    }
    par_bin_of((n - 1) / 2, lane, below, upto, h.x, h.y, h.z, out + 2);
    par_bin_of((n - 1) / 4, lane, below, upto, h.x, h.y, h.z, out + 3);
    par_bin_of((3 * (n - 1)) / 4, lane, below, upto, h.x, h.y, h.z, out + 4);
    const unsigned long long some = __ballot(tot > 0);  // (not zero: n > 0)
    if (lane == __builtin_ctzll(some)) out[5] = 4 * lane + (h.x ? 0 : h.y ? 1 : h.z ? 2 : 3);
    if (lane == 63 - __builtin_clzll(some)) out[6] = 4 * lane + (h.w ? 3 : h.z ? 2 : h.y ? 1 : 0);
    if (lane == 0) out[0] = n;
}

template <int kThreads, int kCap>
void launch_pixels(const ParParams& p, hipStream_t stream) {
    const dim3 grid((unsigned)((p.H * p.W + kThreads - 1) / kThreads), (unsigned)p.R);
    hipLaunchKernelGGL((parallax_pixel_kernel<kThreads, kCap>), grid, dim3(kThreads), 0, stream, p);
}

}  // namespace

}  // namespace cwm

using namespace cwm;

extern "C" int cwm_parallax(const cwm_parallax_args* a) {
    CWM_REQUIRE(a && a->struct_size == sizeof(cwm_parallax_args), "cwm_parallax: args->struct_size must be sizeof(cwm_parallax_args)");
    const cwm_patch_error_args& g = a->base;
    CWM_REQUIRE(g.batch >= 1 && g.batch <= 65535, "cwm_parallax: base.batch = %d, 1 .. 65535", g.batch);
    CWM_REQUIRE(g.H > 0 && g.H % 4 == 0, "cwm_parallax: base.H = %d must be a positive multiple of 4", g.H);
    CWM_REQUIRE(g.W > 0 && g.W % 4 == 0, "cwm_parallax: base.W = %d must be a positive multiple of 4", g.W);
    CWM_REQUIRE((int64_t)g.H * g.W <= kParMaxPixels, "cwm_parallax: base.H base.W = %lld pixels, at most %d", (long long)g.H * g.W, kParMaxPixels);
    CWM_REQUIRE(a->S >= 1 && a->S <= kParMaxSamples, "cwm_parallax: S = %d samples, 1 .. %d", a->S, kParMaxSamples);
    CWM_REQUIRE(a->flows_dev, "cwm_parallax: flows_dev is NULL");
    for (int i = 0; i < 5; ++i)
        CWM_REQUIRE(a->flow_strides[i] >= 0, "cwm_parallax: flow_strides[%d] = %lld must not be negative", i, (long long)a->flow_strides[i]);
    CWM_REQUIRE(a->labels_stride >= 0, "cwm_parallax: labels_stride = %lld must not be negative", (long long)a->labels_stride);
    CWM_REQUIRE(a->ref_slot >= -1 && a->ref_slot <= kParSlots, "cwm_parallax: ref_slot = %d, -1 or 0 .. %d", a->ref_slot, kParSlots);
    CWM_REQUIRE(a->ref_slot < 0 || a->labels_dev, "cwm_parallax: ref_slot = %d needs labels_dev", a->ref_slot);
    CWM_REQUIRE(a->min_pixels >= 1, "cwm_parallax: min_pixels = %d, at least 1", a->min_pixels);
    CWM_REQUIRE(a->min_ref_q >= 1 && a->min_ref_q <= kParMaxRefQ, "cwm_parallax: min_ref_q = %lld, 1 .. %lld", (long long)a->min_ref_q, kParMaxRefQ);
    CWM_REQUIRE(a->min_samples >= 1 && a->min_samples <= a->S, "cwm_parallax: min_samples = %d, 1 .. S = %d", a->min_samples, a->S);
    CWM_REQUIRE(a->par_dev, "cwm_parallax: par_dev is NULL");
    CWM_REQUIRE(a->ref_dev && (reinterpret_cast<uintptr_t>(a->ref_dev) & 7) == 0, "cwm_parallax: ref_dev must not be NULL and must be 8-byte aligned");
    if (a->labels_dev) {
        CWM_REQUIRE(a->hist_dev && (reinterpret_cast<uintptr_t>(a->hist_dev) & 15) == 0, "cwm_parallax: hist_dev must not be NULL with labels_dev and must be 16-byte aligned");
        CWM_REQUIRE(a->slot_tab_dev, "cwm_parallax: slot_tab_dev is NULL with labels_dev");
    }
    ParParams p;
    memset(&p, 0, sizeof(p));
    p.flows = a->flows_dev, p.sb = a->flow_strides[0], p.sc = a->flow_strides[1], p.sh = a->flow_strides[2], p.sw = a->flow_strides[3], p.ss = a->flow_strides[4];
    p.dirs = a->dirs_dev, p.labels = a->labels_dev, p.ls = a->labels_stride;
    p.R = g.batch, p.H = g.H, p.W = g.W, p.S = a->S;
    p.ref_slot = a->ref_slot, p.min_pixels = a->min_pixels, p.min_samples = a->min_samples;
    p.min_den = (double)a->min_ref_q * (double)a->min_ref_q;  // (exact: at most 2^42)
    p.par = a->par_dev, p.spread = a->spread_dev, p.off = a->off_dev, p.cnt = a->cnt_dev, p.ref = a->ref_dev;
    p.hist = p.labels ? a->hist_dev : nullptr, p.slot_tab = p.labels ? a->slot_tab_dev : nullptr;
    hipStream_t stream = (hipStream_t)g.stream;
    // the tables the workgroups add into
    if (p.labels) {
        CWM_HIP_CHECK(hipMemsetAsync(p.hist, 0, (size_t)p.R * kParSide * kParBins * sizeof(int), stream));
        CWM_HIP_CHECK(hipMemsetAsync(p.slot_tab, 0, (size_t)p.R * kParSide * kParTerms * sizeof(int), stream));
    }
    if (!p.dirs) {
        CWM_HIP_CHECK(hipMemsetAsync(p.ref, 0, (size_t)p.R * p.S * 4 * sizeof(double), stream));
        // wide loads: contiguous planes, every plane of the flow on 16 bytes and, where they are read, every label plane on 4 (H W % 16 == 0 does the rest)
        const FlowView view{p.flows, p.R, 2, p.H, p.W, p.S, p.sb, p.sc, p.sh, p.sw, p.ss};
        const FlowLayout lay = flow_layout(view, 0);
        const bool lab4 = p.ref_slot < 0 || ((reinterpret_cast<uintptr_t>(p.labels) & 3) == 0 && (p.ls & 3) == 0);
        const bool vec = lay.planes && lay.f16 && lay.sb4 && lay.sc4 && lay.ss4 && lab4;
        const dim3 grid((unsigned)((p.H * p.W + kParRefGroupPixels - 1) / kParRefGroupPixels), (unsigned)p.S, (unsigned)p.R), block(kParRefThreads);
        if (vec) hipLaunchKernelGGL((parallax_reference_kernel<true>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((parallax_reference_kernel<false>), grid, block, 0, stream, p);
        CWM_HIP_CHECK(hipGetLastError());
    }
    if (p.S <= 8) launch_pixels<256, 8>(p, stream);
    else if (p.S <= 16) launch_pixels<256, 16>(p, stream);
    else if (p.S <= 32) launch_pixels<128, 32>(p, stream);
    else launch_pixels<64, 64>(p, stream);
    CWM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(parallax_finalise_kernel, dim3((unsigned)p.R, (unsigned)kParFinBlocks), dim3(kParFinThreads), 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}
