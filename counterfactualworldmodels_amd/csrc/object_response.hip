// Object interactions (cwm_object_response): which slots of a slot map move when one of them is pushed.  The input is what the counterfactual driver gives for K
// pushed objects per scene -- S flow samples per push -- and the output is, per push, one small table per sample and slot (pixel counts, how many moved, the
// integer flow sums) and, over the samples in which the pushed object itself moved, per slot the share of pushes in which it moved too, its mean displacement
// along the push and its gain against the pushed object.  No counterpart in the reference, whose README describes the motion covariance this reads out at the
// level of objects ("objects adjacent to one another tend to move together, as some motion counterfactuals include collisions between them").
//
// The definition (this is the contract; include/cwm_hip.h repeats it for callers).  Rows r = b K + k, b < B = base.batch, k < K = base.T.  flows: element
// (r, c, y, x, s) at flows_dev[r st[0] + c st[1] + y st[2] + x st[3] + s st[4]], c = 0 horizontal, 1 vertical, in pixels; labels: the slot map of (b, k), H W
// contiguous bytes at labels_dev + b ls[0] + k ls[1] (ls[1] = 0: all pushes of a scene read one map); pushed int32 [R]; dirs int32 [S,2] (dy, dx) in pixels or
// NULL.  Every step is an integer operation or ONE correctly rounded binary64 operation as parenthesised.  Per row r, sample s and pixel (x, y):
//   1 slot     l = labels[y][x], or 0 if that is above 64
//   2 usable   (u, v) = flows[r, :, y, x, s]; usable iff |u| <= 4096 and |v| <= 4096 (false for a NaN and an inf).  Not usable: tab[r][s][l][7] += 1, nothing else
//   3 quantise qu = (int)rintf(u * 256.0f), qv likewise (the multiply is exact); q2 = (int64)qu qu + (int64)qv qv; moved = q2 >= min_q2, an integer comparison
//   4 table    tab[r][s][l][0..6] += 1, moved, qu, qv, moved ? qu : 0, moved ? qv : 0, q2.  |q| <= 2^20 and H W <= 2^18: every sum stays below 2^59
// Then per row, with a = pushed[r] and n_l(s), m_l(s), su_l(s), sv_l(s) = entries 0 .. 3 of tab[r][s][l]:
//   5 valid    sample s is valid iff a is in 1 .. 64, n_a(s) >= min_pixels and ((double)m_a(s) / (double)n_a(s)) >= self_frac: the pushed object itself moved.
//              valid[r][s] = 0 / 1; n_valid = their number
//   6 agg      per slot l over the valid samples: N_l = sum n_l(s), M_l = sum m_l(s), A_l = sum (su_l(s) dx_s + sv_l(s) dy_s) (0 without dirs; |d| <= 4096 keeps it
//              below 2^59), V_l = the number of valid s with n_l(s) > 0 and ((double)m_l(s) / (double)n_l(s)) >= move_frac.  agg[r][l] = (N, M, A, V)
//   7 coupling c0 = ((double)V_l / (double)n_valid), 0 if n_valid = 0; c1 = ((double)M_l / (double)N_l), 0 if N_l = 0; c2 = (((double)A_l / (double)N_l) 2^-8), 0 if
//              N_l = 0; c3 = (((double)A_l / (double)N_l) / ((double)A_a / (double)N_a)), 0 if N_l = 0, N_a = 0 or A_a = 0.  Slot 0 is a row like any other
//   8 stats    (n_valid, a or 0 for a dead row, n_a(0) + tab[r][0][a][7] -- the area of the pushed slot; 0 for a dead row --, 0)
// Outputs: tab int64 [R][S][65][8], valid uint8 [R][S], agg int64 [R][65][4], coupling float64 [R][65][4], stats int32 [R][4].
//
// Two kernels behind one memset of tab, all on base.stream:
//   accumulate  grid (chunks of 1024 pixels, S, R), 256 threads, 4 consecutive pixels of one image row per thread, the shape of object_motion_accumulate_kernel:
//               the 65 x 8 int64 table of the workgroup lives in LDS (4.2 KB); a lane collapses the label runs of its four pixels; the slot of the wave's first
//               lane is summed over the wave (wave_sum.h: the three counts packed into one word, the four flow sums in 32 bits, q2 in 64) and added by one lane
//               with one set of LDS atomics; lanes of other slots and runs that end inside a lane add per lane.  At the end the non-zero entries go to tab as
//               INTEGER atomics.  Two instantiations, chosen by the host: 16-byte loads of u and v and 4-byte label loads where the view has contiguous planes
//               (st[3] = 1, st[2] = W) and every base and stride is on its alignment (flow_view.h's flow_layout: the `_batch_to_samples` view of the flow
//               model's output is one of these); a scalar form through all five strides for everything else (a packed [.., S]-innermost tensor, planes off
//               their alignment)
//   finalise    one workgroup per row: a thread per sample decides step 5, then thread l < 65 owns slot l and loops over the S samples for steps 6 - 8.  (With
//               step 5 inside that loop the call took 138 us at S = 64 and 8 rows, with it in front 113 us; the loop is still a chain of cache round trips,
//               6 us at S = 8 and 34 - 48 us at S = 64: DESIGN.md 8.28)
// Integer atomics give the same bits in any order: two calls on the same inputs give the same bits.  There is no workspace.  No content of a device buffer moves
// an address beyond what the geometry allows: a label byte is tested against 64 before it indexes a table, pushed[r] against 1 .. 64 before it does.
#include <cstring>

#include "../../include/cwm_hip.h"
#include "common.h"
#include "flow_view.h"
#include "wave_sum.h"

#pragma clang fp contract(off)

namespace cwm {

namespace {

constexpr int kRespSlots = 64;
constexpr int kRespSide = kRespSlots + 1;  // slots 0 .. 64
constexpr int kRespTerms = 8;
constexpr int kRespMaxPixels = 1 << 18;
constexpr int kRespMaxSamples = 255;
constexpr int kRespThreads = 256;
constexpr int kRespGroupPixels = 4 * kRespThreads;  // 4 pixels per thread
constexpr int kRespFinThreads = 256;  // (more than kRespMaxSamples and than kRespSide)

struct RespParams {
    const float* flows;
    int64_t sb, sc, sh, sw, ss;
    const uint8_t* labels;
    int64_t ls0, ls1;
    const int* pushed;
    const int* dirs;
    int R, K, H, W, S;
    long long min_q2;
    int min_pixels;
    double self_frac, move_frac;
    unsigned long long* tab;
    uint8_t* valid;
    long long* agg;
    double* coupling;
    int* stats;
};

// what a lane has gathered for one slot: the counts (usable, moved, not usable) packed 10 bits each -- at most 4 per lane, 256 per wave --, the flow sums (at
// most 2^22 per lane, 2^28 per wave) and the sum of q2 (at most 2^43 per lane)
struct RespAcc {
    int cls;
    int su, sv, mu, mv;
    long long q2;
};

__device__ __forceinline__ void resp_clear(RespAcc& a) { a.cls = 0, a.su = 0, a.sv = 0, a.mu = 0, a.mv = 0, a.q2 = 0; }

__device__ __forceinline__ void resp_lds_add(unsigned long long* q, long long v) { atomicAdd(q, (unsigned long long)v); }

// one set of LDS atomics for slot l; zero terms are not issued
__device__ __forceinline__ void resp_flush(const RespAcc& a, int l, unsigned long long* tab_s) {
    unsigned long long* t = tab_s + kRespTerms * l;
    const int n = a.cls & 0x3ff, m = (a.cls >> 10) & 0x3ff, bad = a.cls >> 20;
    if (n) resp_lds_add(t + 0, n);
    if (m) resp_lds_add(t + 1, m);
    if (a.su) resp_lds_add(t + 2, a.su);
    if (a.sv) resp_lds_add(t + 3, a.sv);
    if (a.mu) resp_lds_add(t + 4, a.mu);
    if (a.mv) resp_lds_add(t + 5, a.mv);
    if (a.q2) resp_lds_add(t + 6, a.q2);
    if (bad) resp_lds_add(t + 7, bad);
}

// grid (chunks of 1024 pixels, S, R).  kVec: contiguous planes, the flow planes of every (row, channel, sample) 16-byte aligned and the label planes 4-byte
// aligned (the host decides)
template <bool kVec>
__global__ __launch_bounds__(kRespThreads) void object_response_accumulate_kernel(const RespParams p) {
    __shared__ unsigned long long tab_s[kRespSide * kRespTerms];
    const int s = blockIdx.y, r = blockIdx.z, tid = threadIdx.x, W = p.W, quads = (p.H * W) >> 2;
    const int b = r / p.K, k = r - b * p.K;
    for (int e = tid; e < kRespSide * kRespTerms; e += kRespThreads) tab_s[e] = 0;
    __syncthreads();
    const uint8_t* lab = p.labels + b * p.ls0 + k * p.ls1;
    const float* fu = p.flows + r * p.sb + s * p.ss;
    const float* fv = fu + p.sc;
    const int g = blockIdx.x * kRespThreads + tid;  // the group of 4 pixels; consecutive over the lanes of a wave
    const bool live = g < quads;
    if (__any(live)) {  // (wave-uniform; a wave past the plane has nothing to add)
        const int pix = live ? 4 * g : 0;
        unsigned lw = 0;
        float u[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            if (kVec) {
                lw = *reinterpret_cast<const unsigned*>(lab + pix);
                const float4 tu = *reinterpret_cast<const float4*>(fu + pix), tv = *reinterpret_cast<const float4*>(fv + pix);
                u[0] = tu.x, u[1] = tu.y, u[2] = tu.z, u[3] = tu.w;
                v[0] = tv.x, v[1] = tv.y, v[2] = tv.z, v[3] = tv.w;
            } else {
                const int y = pix / W, x0 = pix - y * W;  // W is a multiple of 4: the four pixels lie in one image row
                const int64_t o = y * p.sh + x0 * p.sw;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    lw |= (unsigned)lab[pix + j] << (8 * j);
                    u[j] = fu[o + j * p.sw], v[j] = fv[o + j * p.sw];
                }
            }
        }
        int l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = (int)((lw >> (8 * j)) & 0xffu);
            l[j] = q <= kRespSlots ? q : 0;
        }
        RespAcc a;
        resp_clear(a);
        int cur = l[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (l[j] != cur) {  // a run of the lane ends inside its four pixels (an object's edge): the lane adds it on its own
                resp_flush(a, cur, tab_s);
                resp_clear(a);
                cur = l[j];
            }
            const bool usable = fabsf(u[j]) <= 4096.f && fabsf(v[j]) <= 4096.f;  // (false for a NaN and for an inf)
            if (live && !usable) a.cls += 1 << 20;
            if (live && usable) {
                const int qu = (int)rintf(u[j] * 256.0f), qv = (int)rintf(v[j] * 256.0f);
                const long long q2 = (long long)qu * qu + (long long)qv * qv;
                const bool moved = q2 >= p.min_q2;
                a.cls += moved ? 1 + (1 << 10) : 1;
                a.su += qu, a.sv += qv, a.q2 += q2;
                if (moved) a.mu += qu, a.mv += qv;
            }
        }
        // every lane now holds (cur, a), its last run.  The slot of the wave's first lane (it holds the lowest group: it is live whenever a lane of the wave is) is
        // summed over the wave -- every lane takes part, a lane of another slot or past the plane with zeros -- and added by one lane; the others add per lane
        const int slot = __shfl(cur, 0, 64);
        const bool mine = live && cur == slot;
        RespAcc w;
        resp_clear(w);
        if (mine) w = a;
        w.cls = wave_sum(w.cls);
        if (w.cls & 0x3ff) {  // (uniform after the sum; without a usable pixel the flow sums are zero)
            w.su = wave_sum(w.su), w.sv = wave_sum(w.sv), w.mu = wave_sum(w.mu), w.mv = wave_sum(w.mv);
            w.q2 = wave_sum(w.q2);
        }
        if ((tid & 63) == 0) resp_flush(w, slot, tab_s);
        if (live && !mine) resp_flush(a, cur, tab_s);
    }
    __syncthreads();
    unsigned long long* gt = p.tab + ((size_t)r * p.S + s) * (kRespSide * kRespTerms);
    for (int e = tid; e < kRespSide * kRespTerms; e += kRespThreads) {
        const unsigned long long t = tab_s[e];
        if (t) atomicAdd(&gt[e], t);
    }
}

// grid (R), 256 threads: thread s < S decides sample s, then thread l < 65 owns slot l.  Every line is one binary64 operation (the file is compiled without
// contraction)
__global__ __launch_bounds__(kRespFinThreads) void object_response_finalise_kernel(const RespParams p) {
    const int r = blockIdx.x, l = threadIdx.x, S = p.S;
    const int pushed = p.pushed[r];
    const bool alive = pushed >= 1 && pushed <= kRespSlots;
    const int a = alive ? pushed : 0;  // (a dead row reads slot 0's entries and uses none of them)
    const long long* T = reinterpret_cast<const long long*>(p.tab) + (size_t)r * S * (kRespSide * kRespTerms);
    __shared__ int valid_s[kRespFinThreads];
    __shared__ long long pushed_s[2];
    if (l < S) {  // step 5, a thread per sample (S <= 255 < kRespFinThreads)
        const long long* ta = T + ((size_t)l * kRespSide + a) * kRespTerms;
        const long long na = ta[0], ma = ta[1];
        const bool valid = alive && na >= (long long)p.min_pixels && ((double)ma / (double)na) >= p.self_frac;  // (min_pixels >= 1: na > 0 where it divides)
        valid_s[l] = valid;
        p.valid[(size_t)r * S + l] = valid ? 1 : 0;
    }
    __syncthreads();
    long long N = 0, M = 0, A = 0, V = 0;
    int n_valid = 0;
    if (l < kRespSide) {  // step 6, a thread per slot: the loads of a sample do not wait for the sample before it
#pragma unroll 4
        for (int s = 0; s < S; ++s) {
            const long long* tl = T + ((size_t)s * kRespSide + l) * kRespTerms;
            const long long n = tl[0], m = tl[1], su = tl[2], sv = tl[3];
            const long long dy = p.dirs ? (long long)p.dirs[2 * s] : 0, dx = p.dirs ? (long long)p.dirs[2 * s + 1] : 0;
            if (!valid_s[s]) continue;
            n_valid += 1;
            N += n, M += m;
            A += su * dx + sv * dy;
            if (n > 0 && ((double)m / (double)n) >= p.move_frac) V += 1;
        }
        if (l == a) pushed_s[0] = N, pushed_s[1] = A;  // (a dead row leaves slot 0's here, and all of its sums are zero)
    }
    __syncthreads();
    if (l >= kRespSide) return;
    const long long Na = pushed_s[0], Aa = pushed_s[1];
    long long* g = p.agg + ((size_t)r * kRespSide + l) * 4;
    g[0] = N, g[1] = M, g[2] = A, g[3] = V;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    if (n_valid > 0) c0 = (double)V / (double)n_valid;
    if (N != 0) {
        const double mean = (double)A / (double)N;
        c1 = (double)M / (double)N;
        c2 = mean * 0.00390625;  // 2^-8
        if (Na != 0 && Aa != 0) c3 = mean / ((double)Aa / (double)Na);
    }
    double* c = p.coupling + ((size_t)r * kRespSide + l) * 4;
    c[0] = c0, c[1] = c1, c[2] = c2, c[3] = c3;
    if (l == 0) {
        const long long* t0 = T + (size_t)a * kRespTerms;
        int* st = p.stats + (size_t)r * 4;
        st[0] = n_valid, st[1] = a, st[2] = alive ? (int)(t0[0] + t0[7]) : 0, st[3] = 0;
    }
}

}  // namespace

}  // namespace cwm

using namespace cwm;

extern "C" int cwm_object_response(const cwm_object_response_args* a) {
    CWM_REQUIRE(a && a->struct_size == sizeof(cwm_object_response_args), "cwm_object_response: args->struct_size must be sizeof(cwm_object_response_args)");
    const cwm_patch_error_args& g = a->base;
    CWM_REQUIRE(g.batch >= 1 && g.batch <= 65535, "cwm_object_response: base.batch = %d, 1 .. 65535", g.batch);
    CWM_REQUIRE(g.T >= 1 && (int64_t)g.batch * g.T <= 65535, "cwm_object_response: base.T = %d: at least 1, and base.batch base.T at most 65535 rows", g.T);
    CWM_REQUIRE(g.H > 0 && g.H % 4 == 0, "cwm_object_response: base.H = %d must be a positive multiple of 4", g.H);
    CWM_REQUIRE(g.W > 0 && g.W % 4 == 0, "cwm_object_response: base.W = %d must be a positive multiple of 4", g.W);
    CWM_REQUIRE((int64_t)g.H * g.W <= kRespMaxPixels, "cwm_object_response: base.H base.W = %lld pixels, at most %d", (long long)g.H * g.W, kRespMaxPixels);
    CWM_REQUIRE(a->S >= 1 && a->S <= kRespMaxSamples, "cwm_object_response: S = %d samples, 1 .. %d", a->S, kRespMaxSamples);
    CWM_REQUIRE(a->flows_dev, "cwm_object_response: flows_dev is NULL");
    for (int i = 0; i < 5; ++i)
        CWM_REQUIRE(a->flow_strides[i] >= 0, "cwm_object_response: flow_strides[%d] = %lld must not be negative", i, (long long)a->flow_strides[i]);
    CWM_REQUIRE(a->labels_dev, "cwm_object_response: labels_dev is NULL");
    CWM_REQUIRE(a->labels_strides[0] >= 0 && a->labels_strides[1] >= 0, "cwm_object_response: labels_strides = (%lld, %lld) must not be negative",
                (long long)a->labels_strides[0], (long long)a->labels_strides[1]);
    CWM_REQUIRE(a->pushed_dev, "cwm_object_response: pushed_dev is NULL");
    CWM_REQUIRE(a->min_q2 >= 0, "cwm_object_response: min_q2 = %lld must not be negative", (long long)a->min_q2);
    CWM_REQUIRE(a->min_pixels >= 1, "cwm_object_response: min_pixels = %d, at least 1", a->min_pixels);
    CWM_REQUIRE(a->self_frac >= 0.0 && a->self_frac <= 1.0, "cwm_object_response: self_frac = %g must lie in [0, 1]", a->self_frac);  // (false for a NaN)
    CWM_REQUIRE(a->move_frac >= 0.0 && a->move_frac <= 1.0, "cwm_object_response: move_frac = %g must lie in [0, 1]", a->move_frac);
    CWM_REQUIRE(a->tab_dev, "cwm_object_response: tab_dev is NULL");
    CWM_REQUIRE(a->valid_dev, "cwm_object_response: valid_dev is NULL");
    CWM_REQUIRE(a->agg_dev, "cwm_object_response: agg_dev is NULL");
    CWM_REQUIRE(a->coupling_dev, "cwm_object_response: coupling_dev is NULL");
    CWM_REQUIRE(a->stats_dev, "cwm_object_response: stats_dev is NULL");
    RespParams p;
    memset(&p, 0, sizeof(p));
    p.flows = a->flows_dev, p.sb = a->flow_strides[0], p.sc = a->flow_strides[1], p.sh = a->flow_strides[2], p.sw = a->flow_strides[3], p.ss = a->flow_strides[4];
    p.labels = a->labels_dev, p.ls0 = a->labels_strides[0], p.ls1 = a->labels_strides[1];
    p.pushed = a->pushed_dev, p.dirs = a->dirs_dev;
    p.R = g.batch * g.T, p.K = g.T, p.H = g.H, p.W = g.W, p.S = a->S;
    p.min_q2 = a->min_q2, p.min_pixels = a->min_pixels, p.self_frac = a->self_frac, p.move_frac = a->move_frac;
    p.tab = reinterpret_cast<unsigned long long*>(a->tab_dev), p.valid = a->valid_dev, p.agg = reinterpret_cast<long long*>(a->agg_dev);
    p.coupling = a->coupling_dev, p.stats = a->stats_dev;
    hipStream_t stream = (hipStream_t)g.stream;
    // the tables the workgroups add into
    CWM_HIP_CHECK(hipMemsetAsync(p.tab, 0, (size_t)p.R * p.S * kRespSide * kRespTerms * sizeof(long long), stream));
    // wide loads: contiguous planes, every plane of the flow on 16 bytes and every label plane on 4 (H W % 16 == 0 does the rest)
    const FlowView view{p.flows, p.R, 2, p.H, p.W, p.S, p.sb, p.sc, p.sh, p.sw, p.ss};
    const FlowLayout lay = flow_layout(view, 0);
    const bool vec = lay.planes && lay.f16 && lay.sb4 && lay.sc4 && lay.ss4 && (reinterpret_cast<uintptr_t>(p.labels) & 3) == 0 && ((p.ls0 | p.ls1) & 3) == 0;
    const dim3 grid((unsigned)((p.H * p.W + kRespGroupPixels - 1) / kRespGroupPixels), (unsigned)p.S, (unsigned)p.R), block(kRespThreads);
    if (vec) hipLaunchKernelGGL((object_response_accumulate_kernel<true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((object_response_accumulate_kernel<false>), grid, block, 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(object_response_finalise_kernel, dim3((unsigned)p.R), dim3(kRespFinThreads), 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}
