// Point tracks through a movie (cwm_point_track): where K query points per row go over T frames, and when they are hidden.  A point follows the forward flow of
// its pair while it stands on the object it started on and the flow can be believed (usable, inside, and -- given the backward flow -- consistent by the test of
// cwm_flow_consistency); otherwise it coasts on the affine motion model of its object (cwm_object_motion) or, without one, on its last believed flow vector, and
// is picked up again when it stands on its object once more.  No counterpart in the reference.
//
// The definition (this is the contract; include/cwm_hip.h repeats it for callers).  Strides are in elements, H x W planes are contiguous, slices of larger buffers
// are read in place.  fwd [B,T-1,2,H,W] fp32 in PAIR order: entry t is the flow from frame t to frame t+1 on frame t's grid, channel 0 horizontal; bwd (may be
// NULL) the same shape in pair order: entry t is the flow from frame t+1 back to frame t on frame t+1's grid; labels (may be NULL) [B,T,H,W] uint8 slot maps, a
// byte above 64 reads as 0; model (may be NULL, needs labels) [B,T,65,12] float64, the rows (valid, tu, tv, a11, a12, a21, a22, mx, my, ..) that cwm_object_motion
// writes: entry t describes the pair (t, t+1) in the slots of frame t; points [B,K,2] fp32 (x, y) in pixels; start (may be NULL: 0) [B,K] int32, the frame a
// point begins in.  Every fp32 step below is ONE correctly rounded fp32 operation in the stated order and every float64 step one binary64 operation: nothing is
// contracted into a fused multiply-add.  Per row b and point k, with s = start[b][k]; state is 0 visible, 1 hidden and coasting, 2 left the frame (terminal),
// 3 lost: hidden for more than max_coast consecutive frames (terminal), 255 not started yet.  A terminal or not-started entry writes xy = the quiet NaN
// 0x7fc00000 (both coordinates) and under = 0.  A start outside 0 .. T-1 gives a point that is never started: 255 in every frame, owner 0.  p_s = points[b][k],
// last = (0, 0), run = 0.  For t = s .. T-1, until a terminal state (which then holds to the last frame):
//   1 inside   p = (px, py) is INSIDE iff px >= 0 && px <= W-1 && py >= 0 && py <= H-1, in fp32 and before anything is converted (a NaN or inf point is
//              outside).  Outside: state 2 from this frame on
//   2 under    under_t = labels[t][(int)rintf(py)][(int)rintf(px)], or 0 if that is above 64, or 0 without labels.  owner = under_s (0 if p_s is outside)
//   3 hidden   with labels hidden_t = (under_t != owner); without, hidden_t = (t > s and the step into frame t was a coast).  run = hidden_t ? run + 1 : 0;
//              run > max_coast: state 3 from this frame on.  Otherwise state_t = hidden_t ? 1 : 0, xy_t = p, and for t < T-1 the point steps:
//   4 flow     tried iff under_t == owner (always without labels).  a_c = the bilinear sample of fwd[t] channel c at p by step 2 of cwm_flow_consistency:
//              x0f = floorf(px), wx = px - x0f, ix0 = (int)x0f, ix1 = min(ix0 + 1, W-1), the same in y; top = o00 + wx (o01 - o00), bot = o10 + wx (o11 - o10),
//              a_c = top + wy (bot - top).  USABLE iff |a_0| <= 4096 && |a_1| <= 4096 (false for a NaN).  q = (px + a_0, py + a_1).  Usable and q not INSIDE: the
//              point leaves, p_{t+1} = q (step 1 makes that state 2).  Usable, q inside and bwd given: o_c = the same sample of bwd[t] at q; ru = a_0 + o_0,
//              rv = a_1 + o_1, res = ru ru + rv rv; mag = (a_0 a_0 + a_1 a_1) + (o_0 o_0 + o_1 o_1); thr = alpha mag + beta (steps 3 and 4 there).  BELIEVED iff
//              usable, q inside and (no bwd or res <= thr).  Believed: p_{t+1} = q, last = a
//   5 coast    when the flow step was not tried, or tried and neither believed nor leaving.  c = last.  With model and m = model[b][t][owner], m.valid >= 1 (false
//              for a NaN): dx = (double)px - mx, dy = (double)py - my; e0 = a11 dx, e1 = a12 dy, cu = e0 + e1, cu = tu + cu; e0 = a21 dx, e1 = a22 dy,
//              cv = e0 + e1, cv = tv + cv; f = ((float)cu, (float)cv) (round to nearest); c = f if both are finite (valid == 1 has a zero matrix: the same
//              lines serve both values).  p_{t+1} = (px + c_0, py + c_1); the step into t+1 counts as a coast
// Outputs, frame-major: xy [B,T,K,2] fp32, state [B,T,K] uint8, under [B,T,K] uint8 (under_t; 0 for terminal and not-started entries), owner [B,K] uint8.
//
// One kernel, one launch per call; a thread owns a point and walks its frames.  What was chosen, and why:
//   the work of a point is a chain: per frame the label byte, then the eight taps of fwd (independent of each other), then the eight taps of bwd at a place
//   that depends on the first eight, then -- rarely -- nine doubles of the model.  Nothing of frame t+1 can be asked for before frame t is done, so a wave waits
//   for two to three cache round trips per frame and nothing but other waves hides them: the kernel wants as many waves in flight as the points give, spread
//   over as many CUs as possible.  Hence ONE point per thread and workgroups of ONE wave (64 threads): K = 784 is 13 workgroups on 13 CUs where 256 threads
//   would put it on 4, and K = 50176 is 784 waves per row, three per CU.  A thread holds a dozen live values: registers limit nothing.
//   the planes (at most 1 MB each, 200 KB at 224 x 224) sit in L2; the taps are 4-byte gathers, the two taps of an image row adjacent.
//   stores are frame-major: the 64 points of a wave write 512 contiguous bytes of xy and 64 contiguous bytes of state and of under per frame.
//   points and start are read once, with 4-byte loads: no alignment beyond that of their element type is asked for.
// Only vector stores, no atomics, no LDS, no workspace, nothing read back.  No content of a device buffer moves an address before it has been range-tested: a
// point is tested in fp32 before it is converted, so every tap and the label index lie in [0, H W); a label byte is tested against 64 before it indexes the model.
#include <cstring>

#include "../../include/cwm_hip.h"
#include "common.h"

#pragma clang fp contract(off)  // (file scope: a*b+c stays a multiply and an add, in fp32 and in binary64)

namespace cwm {

namespace {

constexpr int kPtSlots = 64;
constexpr int kPtModel = 12;  // doubles per slot of the model table
constexpr int kPtMaxPixels = 1 << 18;
constexpr int kPtMaxFrames = 4096, kPtMaxPoints = 65536;
#ifndef CWM_PT_THREADS
#define CWM_PT_THREADS 64  // one wave: see above (a side build with -DCWM_PT_THREADS=256 is how the other choice was measured)
#endif
constexpr int kPtThreads = CWM_PT_THREADS;

struct PtParams {
    const float *fwd, *bwd, *points;
    const uint8_t* labels;
    const double* model;
    const int* start;
    int64_t fs0, fs1, fs2, bs0, bs1, bs2, ls0, ls1, ms0, ms1;
    int T, H, W, K, max_coast;
    float alpha, beta;
    float* xy;
    uint8_t *state, *under, *owner;
};

__device__ __forceinline__ bool pt_inside(float x, float y, float xmax, float ymax) { return x >= 0.f && x <= xmax && y >= 0.f && y <= ymax; }

// both channels of a flow at an INSIDE point: eight independent gathers, then step 2 of cwm_flow_consistency
__device__ __forceinline__ void pt_sample(const float* cu, const float* cv, float px, float py, int W, int H, float& s0, float& s1) {
    const float x0f = floorf(px), y0f = floorf(py);
    const float wx = px - x0f, wy = py - y0f;
    const int ix0 = (int)x0f, iy0 = (int)y0f;  // (the caller tested the point in fp32)
    const int ix1 = min(ix0 + 1, W - 1), iy1 = min(iy0 + 1, H - 1);
    const int i00 = iy0 * W + ix0, i01 = iy0 * W + ix1, i10 = iy1 * W + ix0, i11 = iy1 * W + ix1;
    const float u00 = cu[i00], u01 = cu[i01], u10 = cu[i10], u11 = cu[i11];
    const float v00 = cv[i00], v01 = cv[i01], v10 = cv[i10], v11 = cv[i11];
    const float topu = u00 + wx * (u01 - u00), botu = u10 + wx * (u11 - u10);
    const float topv = v00 + wx * (v01 - v00), botv = v10 + wx * (v11 - v10);
    s0 = topu + wy * (botu - topu), s1 = topv + wy * (botv - topv);
}

// grid (chunks of 64 points, B)
__global__ __launch_bounds__(kPtThreads) void point_track_kernel(const PtParams p) {
    const int k = blockIdx.x * kPtThreads + threadIdx.x, b = blockIdx.y;
    if (k >= p.K) return;
    const int T = p.T, H = p.H, W = p.W, K = p.K;
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    const float qnan = __int_as_float(0x7fc00000), fmax = 3.4028234664e38f;
    const size_t bk = (size_t)b * K + k;
    const int s = p.start ? p.start[bk] : 0;
    const bool started = s >= 0 && s < T;
    float px = p.points[2 * bk], py = p.points[2 * bk + 1];
    float l0 = 0.f, l1 = 0.f;
    int run = 0, owner = 0, term = 0;
    bool coasted = false;
    const float* fwd = p.fwd + b * p.fs0;
    const float* bwd = p.bwd ? p.bwd + b * p.bs0 : nullptr;
    const uint8_t* lab = p.labels ? p.labels + b * p.ls0 : nullptr;
    const double* mod = p.model ? p.model + b * p.ms0 : nullptr;
    size_t o = (size_t)b * T * K + k;
    for (int t = 0; t < T; ++t, o += K) {
        int st = 255, un = 0;
        float ox = qnan, oy = qnan;
        if (started && t >= s) {
            if (!term && !pt_inside(px, py, xmax, ymax)) term = 2;  // 1 inside
            if (!term) {
                if (lab) {  // 2 under (inside: 0 <= rintf(px) <= W-1 and 0 <= rintf(py) <= H-1)
                    const int v = (int)lab[t * p.ls1 + (int)rintf(py) * W + (int)rintf(px)];
                    un = v <= kPtSlots ? v : 0;
                }
                if (t == s) owner = un;
                const bool hidden = lab ? un != owner : coasted;  // 3 hidden (coasted is false at t == s)
                run = hidden ? run + 1 : 0;
                if (run > p.max_coast) term = 3;
                else st = hidden ? 1 : 0, ox = px, oy = py;
            }
            if (term) st = term, un = 0;
        }
        p.xy[2 * o] = ox, p.xy[2 * o + 1] = oy;
        p.state[o] = (uint8_t)st;
        p.under[o] = (uint8_t)un;
        if (st > 1 || t == T - 1) continue;
        bool moved = false;
        if (un == owner) {  // 4 flow
            const float* fu = fwd + t * p.fs1;
            float a0, a1;
            pt_sample(fu, fu + p.fs2, px, py, W, H, a0, a1);
            const bool usable = fabsf(a0) <= 4096.f && fabsf(a1) <= 4096.f;  // (false for a NaN and for an inf)
            const float qx = px + a0, qy = py + a1;
            if (usable) {
                bool ok = true;
                if (pt_inside(qx, qy, xmax, ymax)) {
                    if (bwd) {
                        const float* bu = bwd + t * p.bs1;
                        float o0, o1;
                        pt_sample(bu, bu + p.bs2, qx, qy, W, H, o0, o1);
                        const float ru = a0 + o0, rv = a1 + o1;
                        const float res = ru * ru + rv * rv;
                        const float mag = (a0 * a0 + a1 * a1) + (o0 * o0 + o1 * o1);
                        const float thr = p.alpha * mag + p.beta;
                        ok = res <= thr;  // (a NaN compares false)
                    }
                    if (ok) l0 = a0, l1 = a1;  // believed
                }  // (else the point leaves: the next frame's step 1 ends it)
                if (ok) px = qx, py = qy, moved = true, coasted = false;
            }
        }
        if (!moved) {  // 5 coast
            float c0 = l0, c1 = l1;
            if (mod) {
                const double* m = mod + t * p.ms1 + owner * kPtModel;  // (owner <= 64)
                if (m[0] >= 1.0) {  // (false for a NaN)
                    const double dx = (double)px - m[7], dy = (double)py - m[8];
                    double e0 = m[3] * dx, e1 = m[4] * dy;
                    double cu = e0 + e1;
                    cu = m[1] + cu;
                    e0 = m[5] * dx, e1 = m[6] * dy;
                    double cv = e0 + e1;
                    cv = m[2] + cv;
                    const float f0 = (float)cu, f1 = (float)cv;
                    if (fabsf(f0) <= fmax && fabsf(f1) <= fmax) c0 = f0, c1 = f1;  // (false for a NaN and for an inf)
                }
            }
            px = px + c0, py = py + c1, coasted = true;
        }
    }
    p.owner[bk] = (uint8_t)owner;
}

}  // namespace

}  // namespace cwm

using namespace cwm;

extern "C" int cwm_point_track(const cwm_point_track_args* a) {
    CWM_REQUIRE(a && a->struct_size == sizeof(cwm_point_track_args), "cwm_point_track: args->struct_size must be sizeof(cwm_point_track_args)");
    const cwm_patch_error_args& g = a->base;
    CWM_REQUIRE(g.batch >= 1 && g.batch <= 65535, "cwm_point_track: base.batch = %d, 1 .. 65535", g.batch);
    CWM_REQUIRE(g.T >= 2 && g.T <= kPtMaxFrames, "cwm_point_track: base.T = %d frames, 2 .. %d", g.T, kPtMaxFrames);
    CWM_REQUIRE(g.H > 0 && g.W > 0, "cwm_point_track: base.H = %d and base.W = %d must be positive", g.H, g.W);
    CWM_REQUIRE((int64_t)g.H * g.W <= kPtMaxPixels, "cwm_point_track: base.H base.W = %lld pixels, at most %d", (long long)g.H * g.W, kPtMaxPixels);
    CWM_REQUIRE(a->K >= 1 && a->K <= kPtMaxPoints, "cwm_point_track: K = %d points, 1 .. %d", a->K, kPtMaxPoints);
    CWM_REQUIRE(a->max_coast >= 0, "cwm_point_track: max_coast = %d must not be negative", a->max_coast);
    CWM_REQUIRE(a->fwd_dev, "cwm_point_track: fwd_dev is NULL");
    CWM_REQUIRE(a->fwd_strides[0] >= 0 && a->fwd_strides[1] >= 0 && a->fwd_strides[2] >= 0,
                "cwm_point_track: fwd_strides = (%lld, %lld, %lld) must not be negative", (long long)a->fwd_strides[0], (long long)a->fwd_strides[1],
                (long long)a->fwd_strides[2]);
    CWM_REQUIRE(!a->bwd_dev || (a->bwd_strides[0] >= 0 && a->bwd_strides[1] >= 0 && a->bwd_strides[2] >= 0),
                "cwm_point_track: bwd_strides = (%lld, %lld, %lld) must not be negative", (long long)a->bwd_strides[0], (long long)a->bwd_strides[1],
                (long long)a->bwd_strides[2]);
    CWM_REQUIRE(a->alpha >= 0.f && a->alpha <= 3.4028234664e38f, "cwm_point_track: alpha = %g must be finite and not negative", (double)a->alpha);
    CWM_REQUIRE(a->beta >= 0.f && a->beta <= 3.4028234664e38f, "cwm_point_track: beta = %g must be finite and not negative", (double)a->beta);
    CWM_REQUIRE(!a->labels_dev || (a->labels_strides[0] >= 0 && a->labels_strides[1] >= 0), "cwm_point_track: labels_strides = (%lld, %lld) must not be negative",
                (long long)a->labels_strides[0], (long long)a->labels_strides[1]);
    CWM_REQUIRE(!a->model_dev || a->labels_dev, "cwm_point_track: model_dev is given without labels_dev");
    CWM_REQUIRE(!a->model_dev || (a->model_strides[0] >= 0 && a->model_strides[1] >= 0), "cwm_point_track: model_strides = (%lld, %lld) must not be negative",
                (long long)a->model_strides[0], (long long)a->model_strides[1]);
    CWM_REQUIRE((reinterpret_cast<uintptr_t>(a->model_dev) & 7) == 0, "cwm_point_track: model_dev must be 8-byte aligned");
    CWM_REQUIRE(a->points_dev, "cwm_point_track: points_dev is NULL");
    CWM_REQUIRE((reinterpret_cast<uintptr_t>(a->points_dev) & 3) == 0 && (reinterpret_cast<uintptr_t>(a->start_dev) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(a->fwd_dev) & 3) == 0 && (reinterpret_cast<uintptr_t>(a->bwd_dev) & 3) == 0,
                "cwm_point_track: points_dev, start_dev, fwd_dev and bwd_dev must be 4-byte aligned");
    CWM_REQUIRE(a->xy_dev, "cwm_point_track: xy_dev is NULL");
    CWM_REQUIRE((reinterpret_cast<uintptr_t>(a->xy_dev) & 3) == 0, "cwm_point_track: xy_dev must be 4-byte aligned");
    CWM_REQUIRE(a->state_dev, "cwm_point_track: state_dev is NULL");
    CWM_REQUIRE(a->under_dev, "cwm_point_track: under_dev is NULL");
    CWM_REQUIRE(a->owner_dev, "cwm_point_track: owner_dev is NULL");
    PtParams p;
    memset(&p, 0, sizeof(p));
    p.fwd = a->fwd_dev, p.fs0 = a->fwd_strides[0], p.fs1 = a->fwd_strides[1], p.fs2 = a->fwd_strides[2];
    p.bwd = a->bwd_dev, p.bs0 = a->bwd_strides[0], p.bs1 = a->bwd_strides[1], p.bs2 = a->bwd_strides[2];
    p.labels = a->labels_dev, p.ls0 = a->labels_strides[0], p.ls1 = a->labels_strides[1];
    p.model = a->model_dev, p.ms0 = a->model_strides[0], p.ms1 = a->model_strides[1];
    p.points = a->points_dev, p.start = a->start_dev;
    p.T = g.T, p.H = g.H, p.W = g.W, p.K = a->K, p.max_coast = a->max_coast;
    p.alpha = a->alpha, p.beta = a->beta;
    p.xy = a->xy_dev, p.state = a->state_dev, p.under = a->under_dev, p.owner = a->owner_dev;
    const dim3 grid((unsigned)((p.K + kPtThreads - 1) / kPtThreads), (unsigned)g.batch), block(kPtThreads);
    hipLaunchKernelGGL(point_track_kernel, grid, block, 0, (hipStream_t)g.stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}
