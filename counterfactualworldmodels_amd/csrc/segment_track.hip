// Scene segments through a movie (cwm_segment_track): the previous frame's track map is warped onto this frame by the backward flow, its overlaps with this
// frame's label map (what cwm_segment_merge wrote) are counted, tracks and labels are linked one to one, unlinked tracks coast or end, unlinked labels are born
// into free slots, and the result is painted -- one call per frame, nothing read back.  No counterpart in the reference, whose README lists the segmentation
// algorithm itself as coming.
//
// The definition (this is the contract; include/cwm_hip.h repeats it for callers).  There are 64 track SLOTS, numbered 1 .. 64.  Per row b, in this order:
//   0 inputs   prev[b]: the H W contiguous bytes at prev_dev + b prev_stride, the previous frame's track map (0: none, 1 .. 64: a slot); NULL: no previous frame.
//              cur[b]: the same with cur_stride, this frame's label map (0: none, 1 .. 64: a label); NULL: no segmentation for this frame, the call only
//              propagates.  flow: pixel (b, c, y, x) at flow_dev[b flow_strides[0] + c flow_strides[1] + y W + x], channel 0 horizontal and channel 1 vertical,
//              in pixels, FROM THIS FRAME TO THE PREVIOUS ONE, on this frame's grid; NULL: zero motion.  State in: track_id_in[b][64] (0: the slot is free,
//              otherwise its persistent id), age_in[b][64], next_id_in[b]; all three NULL: every slot free, next_id 1.  A prev or cur byte above 64 counts as 0;
//              a prev slot whose track_id_in is 0 counts as 0.  A slot is LIVE iff its track_id_in is not 0
//   1 warp     fx = (float)x + u, fy = (float)y + v (one fp32 add each); rx = rintf(fx), ry = rintf(fy) (half to even); the source is inside iff
//              rx >= 0 && rx <= W-1 && ry >= 0 && ry <= H-1 in fp32 (a NaN or an inf is outside); w(y,x) = prev[(int)ry][(int)rx] inside, else 0
//   2 table    n[c][p] = the number of pixels with cur == c and w == p, c and p in 0 .. 64; area_cur[c] = sum_p n[c][p]; area_w[p] = sum_c n[c][p]
//   3 link     (c >= 1, p >= 1) is a candidate iff n[c][p] >= max(1, min_inter) and (float)n[c][p] > iou_thresh * (float)(area_cur[c] + area_w[p] - n[c][p])
//              (one fp32 multiply and one compare; every integer is at most 2^19 and exact in fp32; a NaN threshold compares false).  Up to 64 rounds in the
//              order of select_order.h: key (float)n[c][p], the higher first, ties to the lower index (c-1) 64 + (p-1).  The winner is linked, slot_of[c] = p,
//              and every candidate that shares its c or its p is removed
//   4 coast    a live slot p that no pair linked COASTS iff carry && area_w[p] > 0 && age_in[p] + 1 <= max_age: it keeps its id, age_out = age_in + 1.  Otherwise
//              it ENDS: track_id_out = 0, age_out = 0.  A linked slot keeps its id and gets age 0
//   5 births   the unlinked labels c >= 1 with area_cur[c] >= max(1, min_area), in ascending c, each take the lowest slot that was free on entry or ended in
//              step 4 and that no earlier birth took; id = the running next_id, counting up from next_id_in (32-bit wrap-around), age 0.  Without a free slot
//              the label is dropped, slot_of[c] = 0; unlinked labels below min_area are dropped too.  next_id_out = next_id_in + the number of births
//   6 paint    out(y,x) = slot_of[cur(y,x)] where that is > 0; elsewhere w(y,x) if that slot coasts; elsewhere 0
//   7 read-outs per slot s over the pixels of out with value s: area[b][64]; bbox[b][64][4] = (y0, x0, y1, x1) inclusive, (0, 0, -1, -1) for an empty slot;
//              moments[b][64][2] int64 = (sum y, sum x)
//   8 tables   slot_of_cur[b][64]: entry c-1 = the slot of label c or 0; linked_cur[b][64]: entry p-1 = the label linked to slot p or 0; table[b][65][65] = n;
//              warped[b][H][W] = w
//   9 stats    [b][8]: linked, born, coasting, ended, dropped labels (area_cur >= 1 and no slot), live slots out (track_id_out != 0), labelled pixels of out, 0
// The state buffers in and out are separate and may not alias; out_dev may not overlap prev_dev or cur_dev.
//
// Four kernels behind one memset, all on base.stream.  What was chosen, and why:
//   count    a thread owns 16 consecutive pixels: one 16-byte load of cur, float4 loads of u and v (planes that are not 16-byte aligned take narrow loads, as the
//            merge's pack kernel does), 16 byte gathers of prev (the map is at most 256 KB: latency, not bandwidth), one 16-byte store of w into the workspace.
//            The pair counts go into a 65 x 65 int table in LDS.  Most pixels are the pair (0, 0) and neighbours mostly share a pair: a thread collapses the
//            runs of its 16 pixels first, the (0, 0) count stays in a register and is summed over the wave by shuffles -- otherwise the pass serialises on
//            one LDS address.  Then one global INTEGER atomic per non-zero entry and workgroup into the table the call zeroed
//   link     one workgroup of kSelThreads per row: table and margins in LDS, the 4096 pair words through um_select_rounds_removing (select_order.h); steps 4 and 5
//            on one wave, the lowest free slots by ballots and popcounts; writes the state, the tables and two 65-entry look-up tables for the paint pass
//   paint    16 pixels per thread, the look-up tables in LDS, 16-byte stores of out (byte stores when the row is not 16-byte aligned).  Area, bbox (integer
//            maxima of H - y, W - x, y + 1, x + 1: zero is "none", so one memset serves) and moments (64-bit integer adds) go through LDS with the same run
//            collapsing, then one global integer atomic per slot and workgroup
//   finish   one wave per row: area, bbox, moments, stats
// Integer atomics give the same bits in any order: two calls on the same inputs give the same bits, and the call does not depend on what work_dev holds on entry.
// No content of a device buffer moves an address beyond what the geometry allows: label and slot bytes are tested against 64 before they index a table, the
// warp source is tested in fp32 before it is converted, and ids, ages and next_id are only ever compared and copied.
#include <cstring>

#include "../../include/cwm_hip.h"
#include "common.h"
#include "select_order.h"

namespace cwm {

namespace {

constexpr int kTrackSlots = 64;
constexpr int kTrackSide = kTrackSlots + 1;          // labels and slots 0 .. 64
constexpr int kTrackPairs = kTrackSide * kTrackSide;  // 4225
constexpr int kTrackMaxPixels = 1 << 18;
constexpr int kTrackThreads = 256;
constexpr int kTrackLut = 80;                         // bytes per look-up table in the workspace (65 used)
static_assert(kTrackSlots * kTrackSlots == kSelMaxCells, "one rank word per (label, slot) pair");

struct TrackParams {
    const uint8_t *prev, *cur;
    int64_t prev_stride, cur_stride;
    const float* flow;
    int64_t fs0, fs1;
    const int *id_in, *age_in, *next_in;
    int B, H, W;
    float iou_thresh;
    int min_inter, min_area, max_age, carry;
    // workspace
    unsigned long long* w_mom;  // [B][64][2], zeroed by the call
    int* w_table;               // [B][65 65], zeroed by the call
    int* w_area;                // [B][64], zeroed by the call
    int* w_bbox;                // [B][64][4] maxima of (H - y, W - x, y + 1, x + 1), zeroed by the call
    uint8_t* w_lut;             // [B][2][kTrackLut]: slot_of[c], then p where slot p coasts
    int* w_meta;                // [B][8]: linked, born, coasting, ended, dropped, live out
    uint8_t* w_warp;            // [B][H W]
    // outputs
    uint8_t* out;
    int64_t out_stride;
    int *id_out, *age_out, *next_out, *area, *bbox;
    long long* moments;
    int *slot_of_cur, *linked_cur, *table;
    uint8_t* warped;
    int* stats;
};

struct TrackLayout {
    size_t mom, table, area, bbox, zero_bytes, lut, meta, warp, total;  // byte offsets; mom, lut, meta, warp are multiples of 16
};
size_t track_align16(size_t v) { return (v + 15) & ~(size_t)15; }
TrackLayout track_layout(int B, int HW) {
    TrackLayout l;
    l.mom = 0;  // (the 64-bit table first: what follows needs 4-byte alignment only, and one memset clears all four)
    l.table = (size_t)B * kTrackSlots * 2 * sizeof(unsigned long long);
    l.area = l.table + (size_t)B * kTrackPairs * sizeof(int);
    l.bbox = l.area + (size_t)B * kTrackSlots * sizeof(int);
    l.zero_bytes = l.bbox + (size_t)B * kTrackSlots * 4 * sizeof(int);
    l.lut = track_align16(l.zero_bytes);
    l.meta = track_align16(l.lut + (size_t)B * 2 * kTrackLut);
    l.warp = track_align16(l.meta + (size_t)B * 8 * sizeof(int));
    l.total = track_align16(l.warp + (size_t)B * HW);
    return l;
}
bool track_sizes_ok(int B, int H, int W) {
    return B >= 1 && B <= 65535 && H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0 && (int64_t)H * W <= kTrackMaxPixels;
}

// 16 bytes of a plane, by one 16-byte load where the plane allows it
__device__ __forceinline__ void track_load16(const uint8_t* q, bool vec, unsigned (&w)[4]) {
    if (vec) {
        const uint4 v = *reinterpret_cast<const uint4*>(q);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = (unsigned)q[4 * i] | ((unsigned)q[4 * i + 1] << 8) | ((unsigned)q[4 * i + 2] << 16) | ((unsigned)q[4 * i + 3] << 24);
    }
}
__device__ __forceinline__ void track_store16(uint8_t* q, bool vec, const unsigned (&w)[4]) {
    if (vec) {
        *reinterpret_cast<uint4*>(q) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) q[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}
__device__ __forceinline__ void track_load_flow16(const float* q, bool vec, float (&f)[16]) {
    if (vec) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 v = reinterpret_cast<const float4*>(q)[i];
            f[4 * i] = v.x, f[4 * i + 1] = v.y, f[4 * i + 2] = v.z, f[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) f[i] = q[i];
    }
}
__device__ __forceinline__ int track_byte(const unsigned (&w)[4], int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 0xffu); }

// grid (groups of 16 pixels / 256, B)
__global__ __launch_bounds__(kTrackThreads) void track_count_kernel(const TrackParams p) {
    __shared__ int tab[kTrackPairs];
    __shared__ unsigned long long live_s;
    const int b = blockIdx.y, tid = threadIdx.x, W = p.W, HW = p.H * W;
    for (int e = tid; e < kTrackPairs; e += kTrackThreads) tab[e] = 0;
    if (tid < 64) {
        const unsigned long long m = __ballot(p.prev && p.id_in && p.id_in[(size_t)b * kTrackSlots + tid] != 0);
        if (tid == 0) live_s = m;
    }
    __syncthreads();
    const unsigned long long live = live_s;
    const int g = blockIdx.x * kTrackThreads + tid;
    int zero = 0;  // the thread's pixels of the pair (0, 0)
    if (g < (HW >> 4)) {  // H W % 16 == 0
        const int pix = 16 * g;
        unsigned cw[4] = {0, 0, 0, 0}, ww[4] = {0, 0, 0, 0};
        if (p.cur) {
            const uint8_t* plane = p.cur + (int64_t)b * p.cur_stride;
            track_load16(plane + pix, (reinterpret_cast<uintptr_t>(plane) & 15) == 0, cw);
        }
        if (live) {  // (no live slot, or no previous frame: w is 0 everywhere)
            const uint8_t* prev = p.prev + (int64_t)b * p.prev_stride;
            float u[16], v[16];
            if (p.flow) {
                const float* fu = p.flow + (int64_t)b * p.fs0;
                const float* fv = fu + p.fs1;
                const bool vec = ((reinterpret_cast<uintptr_t>(fu) | reinterpret_cast<uintptr_t>(fv)) & 15) == 0;
                track_load_flow16(fu + pix, vec, u);
                track_load_flow16(fv + pix, vec, v);
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) u[i] = 0.f, v[i] = 0.f;
            }
            const float xmax = (float)(W - 1), ymax = (float)(p.H - 1);
            int src[16];  // the source pixel, -1 outside: the 16 gathers are independent loads
#pragma unroll
            for (int q = 0; q < 4; ++q) {  // four pixels from a multiple of 4: one image row (W is a multiple of 4)
                const int y = (pix + 4 * q) / W, x0 = (pix + 4 * q) - y * W;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float rx = rintf(__fadd_rn((float)(x0 + j), u[4 * q + j])), ry = rintf(__fadd_rn((float)y, v[4 * q + j]));
                    const bool inside = rx >= 0.f && rx <= xmax && ry >= 0.f && ry <= ymax;
                    src[4 * q + j] = inside ? (int)ry * W + (int)rx : -1;
                }
            }
            int got[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) got[i] = src[i] >= 0 ? (int)prev[src[i]] : 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int s = got[i];
                const bool ok = s >= 1 && s <= kTrackSlots && ((live >> ((s - 1) & 63)) & 1ull);
                ww[i >> 2] |= ok ? (unsigned)s << (8 * (i & 3)) : 0u;
            }
        }
        track_store16(p.w_warp + (size_t)b * HW + pix, true, ww);
        int last = 0, cnt = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = track_byte(cw, i), key = (c <= kTrackSlots ? c : 0) * kTrackSide + track_byte(ww, i);
            if (key == last) {
                ++cnt;
            } else {
                if (last == 0) zero += cnt;
                else atomicAdd(&tab[last], cnt);
                last = key, cnt = 1;
            }
        }
        if (last == 0) zero += cnt;
        else atomicAdd(&tab[last], cnt);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) zero += __shfl_xor(zero, o, 64);  // (every lane takes part)
    if ((tid & 63) == 0 && zero) atomicAdd(&tab[0], zero);
    __syncthreads();
    int* dst = p.w_table + (size_t)b * kTrackPairs;
    for (int e = tid; e < kTrackPairs; e += kTrackThreads)
        if (tab[e]) atomicAdd(&dst[e], tab[e]);
}

// one workgroup per row
__global__ __launch_bounds__(kSelThreads) void track_link_kernel(const TrackParams p) {
    __shared__ unsigned long long comp[kSelMaxCells];
    __shared__ int tab[kTrackPairs];
    __shared__ int area_cur[kTrackSide], area_w[kTrackSide], slot_of[kTrackSide], linked[kTrackSide];
    __shared__ int by_rank[kTrackSlots];
    __shared__ unsigned long long xch[2][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int* src = p.w_table + (size_t)b * kTrackPairs;
    for (int e = tid; e < kTrackPairs; e += kSelThreads) {
        const int n = src[e];
        tab[e] = n;
        if (p.table) p.table[(size_t)b * kTrackPairs + e] = n;
    }
    if (tid < kTrackSide) slot_of[tid] = 0, linked[tid] = 0;
    __syncthreads();
    if (tid < kTrackSide) {
        int s = 0;
        for (int q = 0; q < kTrackSide; ++q) s += tab[tid * kTrackSide + q];
        area_cur[tid] = s;
    } else if (tid >= 128 && tid < 128 + kTrackSide) {
        const int q = tid - 128;
        int s = 0;
        for (int c = 0; c < kTrackSide; ++c) s += tab[c * kTrackSide + q];
        area_w[q] = s;
    }
    __syncthreads();
    const int need = p.min_inter > 1 ? p.min_inter : 1;
    unsigned long long best = 0;
    for (int i = tid; i < kSelMaxCells; i += kSelThreads) {
        const int c = (i >> 6) + 1, q = (i & 63) + 1, n = tab[c * kTrackSide + q];
        const bool cand = n >= need && (float)n > __fmul_rn(p.iou_thresh, (float)(area_cur[c] + area_w[q] - n));
        const unsigned long long w = cand ? um_rank(1, (float)n, i) : 0ull;
        comp[i] = w;
        best = um_max64(best, w);
    }
    um_select_rounds_removing(
        comp, kSelMaxCells, kTrackSlots, best, xch,
        [&](int, int cell) {
            if (tid == 0 && cell >= 0) slot_of[(cell >> 6) + 1] = (cell & 63) + 1, linked[(cell & 63) + 1] = (cell >> 6) + 1;
        },
        [&](int cell, int c) { return (cell >> 6) == (c >> 6) || (cell & 63) == (c & 63); });
    __syncthreads();

    // steps 4 and 5 on one wave: lane l is slot l + 1, and label l + 1
    const int lane = tid;
    const bool wave0 = tid < 64;
    int id = 0, age = 0, next = 1, n_want = 0, free_rank = 0, n_born = 0;
    bool is_linked = false, coast = false, ended = false, is_free = false;
    if (wave0) {
        const size_t at = (size_t)b * kTrackSlots + lane;
        if (p.id_in) id = p.id_in[at], age = p.age_in[at], next = p.next_in[b];
        const bool is_live = id != 0;
        is_linked = linked[lane + 1] > 0;  // (only live slots appear in w, so a linked slot is live)
        coast = is_live && !is_linked && p.carry && area_w[lane + 1] > 0 && age <= p.max_age - 1;
        ended = is_live && !is_linked && !coast;
        is_free = !is_live || ended;
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned long long free_mask = __ballot(is_free);
        free_rank = __popcll(free_mask & below);
        const bool wants = slot_of[lane + 1] == 0 && area_cur[lane + 1] >= (p.min_area > 1 ? p.min_area : 1);
        const unsigned long long want_mask = __ballot(wants);
        n_want = __popcll(want_mask);
        if (wants) by_rank[__popcll(want_mask & below)] = lane + 1;
        n_born = min(n_want, __popcll(free_mask));
    }
    __syncthreads();
    int id_o = 0, age_o = 0;
    bool born = false;
    if (wave0) {
        born = is_free && free_rank < n_want;
        if (born) slot_of[by_rank[free_rank]] = lane + 1;
        id_o = (is_linked || coast) ? id : born ? (int)((unsigned)next + (unsigned)free_rank) : 0;
        age_o = coast ? age + 1 : 0;
        const size_t at = (size_t)b * kTrackSlots + lane;
        if (p.id_out) p.id_out[at] = id_o;
        if (p.age_out) p.age_out[at] = age_o;
        if (lane == 0 && p.next_out) p.next_out[b] = (int)((unsigned)next + (unsigned)n_born);
        if (p.linked_cur) p.linked_cur[at] = linked[lane + 1];
    }
    __syncthreads();
    if (wave0) {
        const size_t at = (size_t)b * kTrackSlots + lane;
        const int s = slot_of[lane + 1];
        if (p.slot_of_cur) p.slot_of_cur[at] = s;
        uint8_t* lut = p.w_lut + (size_t)b * 2 * kTrackLut;
        lut[lane + 1] = (uint8_t)s;
        lut[kTrackLut + lane + 1] = coast ? (uint8_t)(lane + 1) : (uint8_t)0;
        if (lane == 0) lut[0] = 0, lut[kTrackLut] = 0;
        const int n_linked = __popcll(__ballot(is_linked)), n_coast = __popcll(__ballot(coast)), n_ended = __popcll(__ballot(ended));
        const int n_dropped = __popcll(__ballot(area_cur[lane + 1] >= 1 && s == 0)), n_live = __popcll(__ballot(id_o != 0));
        if (lane == 0) {
            int* meta = p.w_meta + 8 * (size_t)b;
            meta[0] = n_linked, meta[1] = n_born, meta[2] = n_coast, meta[3] = n_ended, meta[4] = n_dropped, meta[5] = n_live, meta[6] = 0, meta[7] = 0;
        }
    }
}

// grid (groups of 16 pixels / 256, B)
__global__ __launch_bounds__(kTrackThreads) void track_paint_kernel(const TrackParams p) {
    __shared__ unsigned long long mom[kTrackSlots][2];
    __shared__ int area[kTrackSlots];
    __shared__ int box[kTrackSlots][4];
    __shared__ uint8_t lut_cur[kTrackLut], lut_coast[kTrackLut];
    const int b = blockIdx.y, tid = threadIdx.x, W = p.W, H = p.H, HW = H * W;
    if (tid < kTrackSlots) {
        mom[tid][0] = 0, mom[tid][1] = 0, area[tid] = 0;
        box[tid][0] = 0, box[tid][1] = 0, box[tid][2] = 0, box[tid][3] = 0;
    }
    if (tid < kTrackLut) {
        const uint8_t* lut = p.w_lut + (size_t)b * 2 * kTrackLut;
        lut_cur[tid] = tid < kTrackSide ? min((int)lut[tid], kTrackSlots) : 0;
        lut_coast[tid] = tid < kTrackSide ? min((int)lut[kTrackLut + tid], kTrackSlots) : 0;
    }
    __syncthreads();
    const int g = blockIdx.x * kTrackThreads + tid;
    if (g < (HW >> 4)) {
        const int pix = 16 * g;
        unsigned cw[4] = {0, 0, 0, 0}, ww[4], ow[4] = {0, 0, 0, 0};
        if (p.cur) {
            const uint8_t* plane = p.cur + (int64_t)b * p.cur_stride;
            track_load16(plane + pix, (reinterpret_cast<uintptr_t>(plane) & 15) == 0, cw);
        }
        track_load16(p.w_warp + (size_t)b * HW + pix, true, ww);
        // a run: consecutive pixels of one slot (in one thread's 16; they may cross image rows)
        int last = 0, cnt = 0, sy = 0, sx = 0, y0 = 0, y1 = 0, x0 = 0, x1 = 0;
        auto flush = [&]() {
            if (last == 0) return;
            const int s = last - 1;
            atomicAdd(&area[s], cnt);
            atomicMax(&box[s][0], H - y0), atomicMax(&box[s][1], W - x0), atomicMax(&box[s][2], y1 + 1), atomicMax(&box[s][3], x1 + 1);
            atomicAdd(&mom[s][0], (unsigned long long)sy), atomicAdd(&mom[s][1], (unsigned long long)sx);
        };
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int y = (pix + 4 * q) / W, xq = (pix + 4 * q) - y * W;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = 4 * q + j, x = xq + j;
                const int c = track_byte(cw, i), wv = min(track_byte(ww, i), kTrackSlots);
                const int sc = c <= kTrackSlots ? (int)lut_cur[c] : 0;
                const int o = sc > 0 ? sc : (int)lut_coast[wv];
                ow[q] |= (unsigned)o << (8 * j);
                if (o == last) {
                    ++cnt, sy += y, sx += x;
                    y0 = min(y0, y), y1 = max(y1, y), x0 = min(x0, x), x1 = max(x1, x);
                } else {
                    flush();
                    last = o, cnt = 1, sy = y, sx = x, y0 = y1 = y, x0 = x1 = x;
                }
            }
        }
        flush();
        if (p.out) {
            uint8_t* row = p.out + (int64_t)b * p.out_stride;
            track_store16(row + pix, (reinterpret_cast<uintptr_t>(row) & 15) == 0, ow);
        }
        if (p.warped) {
            uint8_t* row = p.warped + (size_t)b * HW;
            track_store16(row + pix, (reinterpret_cast<uintptr_t>(row) & 15) == 0, ww);
        }
    }
    __syncthreads();
    if (tid < kTrackSlots && area[tid]) {
        const size_t at = (size_t)b * kTrackSlots + tid;
        atomicAdd(&p.w_area[at], area[tid]);
#pragma unroll
        for (int k = 0; k < 4; ++k) atomicMax(&p.w_bbox[4 * at + k], box[tid][k]);
        atomicAdd(&p.w_mom[2 * at], mom[tid][0]), atomicAdd(&p.w_mom[2 * at + 1], mom[tid][1]);
    }
}

// one wave per row
__global__ __launch_bounds__(64) void track_finish_kernel(const TrackParams p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const size_t at = (size_t)b * kTrackSlots + lane;
    const int a = p.w_area[at];
    if (p.area) p.area[at] = a;
    if (p.bbox) {
        const int* m = p.w_bbox + 4 * at;
        int* o = p.bbox + 4 * at;
        o[0] = a ? p.H - m[0] : 0, o[1] = a ? p.W - m[1] : 0, o[2] = a ? m[2] - 1 : -1, o[3] = a ? m[3] - 1 : -1;
    }
    if (p.moments) p.moments[2 * at] = (long long)p.w_mom[2 * at], p.moments[2 * at + 1] = (long long)p.w_mom[2 * at + 1];
    int sum = a;
#pragma unroll
    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane < 8 && p.stats) {
        const int* meta = p.w_meta + 8 * (size_t)b;
        p.stats[8 * (size_t)b + lane] = lane < 6 ? meta[lane] : lane == 6 ? sum : 0;
    }
}

int launch_segment_track(const TrackParams& q, void* work, hipStream_t stream) {
    TrackParams p = q;
    const int HW = p.H * p.W;
    const TrackLayout l = track_layout(p.B, HW);
    char* w = static_cast<char*>(work);
    p.w_mom = reinterpret_cast<unsigned long long*>(w + l.mom), p.w_table = reinterpret_cast<int*>(w + l.table), p.w_area = reinterpret_cast<int*>(w + l.area);
    p.w_bbox = reinterpret_cast<int*>(w + l.bbox), p.w_lut = reinterpret_cast<uint8_t*>(w + l.lut), p.w_meta = reinterpret_cast<int*>(w + l.meta);
    p.w_warp = reinterpret_cast<uint8_t*>(w + l.warp);
    CWM_HIP_CHECK(hipMemsetAsync(w, 0, l.zero_bytes, stream));  // the four tables the kernels add into
    const dim3 grid((unsigned)((HW / 16 + kTrackThreads - 1) / kTrackThreads), (unsigned)p.B), block(kTrackThreads);
    hipLaunchKernelGGL(track_count_kernel, grid, block, 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(track_link_kernel, dim3((unsigned)p.B), dim3(kSelThreads), 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(track_paint_kernel, grid, block, 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(track_finish_kernel, dim3((unsigned)p.B), dim3(64), 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

}  // namespace cwm

using namespace cwm;

extern "C" size_t cwm_segment_track_work_bytes(int B, int H, int W) { return track_sizes_ok(B, H, W) ? track_layout(B, H * W).total : 0; }

extern "C" int cwm_segment_track(const cwm_segment_track_args* a) {
    CWM_REQUIRE(a && a->struct_size == sizeof(cwm_segment_track_args), "cwm_segment_track: args->struct_size must be sizeof(cwm_segment_track_args)");
    const cwm_patch_error_args& g = a->base;
    CWM_REQUIRE(g.batch >= 1 && g.batch <= 65535, "cwm_segment_track: base.batch = %d, 1 .. 65535", g.batch);
    CWM_REQUIRE(g.H > 0 && g.H % 4 == 0, "cwm_segment_track: base.H = %d must be a positive multiple of 4", g.H);
    CWM_REQUIRE(g.W > 0 && g.W % 4 == 0, "cwm_segment_track: base.W = %d must be a positive multiple of 4", g.W);
    CWM_REQUIRE((int64_t)g.H * g.W <= kTrackMaxPixels, "cwm_segment_track: base.H base.W = %lld pixels, at most %d", (long long)g.H * g.W, kTrackMaxPixels);
    const int64_t HW = (int64_t)g.H * g.W;
    CWM_REQUIRE(a->prev_stride >= 0, "cwm_segment_track: prev_stride = %lld must not be negative", (long long)a->prev_stride);
    CWM_REQUIRE(a->cur_stride >= 0, "cwm_segment_track: cur_stride = %lld must not be negative", (long long)a->cur_stride);
    CWM_REQUIRE(a->flow_strides[0] >= 0 && a->flow_strides[1] >= 0, "cwm_segment_track: flow_strides = (%lld, %lld) must not be negative",
                (long long)a->flow_strides[0], (long long)a->flow_strides[1]);
    const int n_state = (a->track_id_in_dev != nullptr) + (a->age_in_dev != nullptr) + (a->next_id_in_dev != nullptr);
    CWM_REQUIRE(n_state == 0 || n_state == 3, "cwm_segment_track: track_id_in_dev, age_in_dev and next_id_in_dev: all three or none (none: an empty state)");
    CWM_REQUIRE(a->min_inter >= 0, "cwm_segment_track: min_inter = %d must not be negative", a->min_inter);
    CWM_REQUIRE(a->min_area >= 0, "cwm_segment_track: min_area = %d must not be negative", a->min_area);
    CWM_REQUIRE(a->max_age >= 0, "cwm_segment_track: max_age = %d must not be negative", a->max_age);
    CWM_REQUIRE(a->carry == 0 || a->carry == 1, "cwm_segment_track: carry = %d, 0 or 1", a->carry);
    CWM_REQUIRE(!a->out_dev || a->out_stride >= HW, "cwm_segment_track: out_stride = %lld, at least H W = %lld", (long long)a->out_stride, (long long)HW);
    CWM_REQUIRE(a->out_dev || a->track_id_out_dev || a->age_out_dev || a->next_id_out_dev || a->area_dev || a->bbox_dev || a->moments_dev || a->slot_of_cur_dev ||
                    a->linked_cur_dev || a->table_dev || a->warped_dev || a->stats_dev,
                "cwm_segment_track: no output requested");
    CWM_REQUIRE(a->work_dev && (reinterpret_cast<uintptr_t>(a->work_dev) & 15) == 0, "cwm_segment_track: work_dev = %p must be a 16-byte aligned device address", a->work_dev);
    const size_t need = cwm_segment_track_work_bytes(g.batch, g.H, g.W);
    CWM_REQUIRE(a->work_bytes >= need, "cwm_segment_track: work_bytes = %llu, cwm_segment_track_work_bytes gives %llu", (unsigned long long)a->work_bytes,
                (unsigned long long)need);
    TrackParams p;
    memset(&p, 0, sizeof(p));
    p.prev = a->prev_dev, p.prev_stride = a->prev_stride, p.cur = a->cur_dev, p.cur_stride = a->cur_stride;
    p.flow = a->flow_dev, p.fs0 = a->flow_strides[0], p.fs1 = a->flow_strides[1];
    p.id_in = a->track_id_in_dev, p.age_in = a->age_in_dev, p.next_in = a->next_id_in_dev;
    p.B = g.batch, p.H = g.H, p.W = g.W;
    p.iou_thresh = a->iou_thresh, p.min_inter = a->min_inter, p.min_area = a->min_area, p.max_age = a->max_age, p.carry = a->carry;
    p.out = a->out_dev, p.out_stride = a->out_stride, p.id_out = a->track_id_out_dev, p.age_out = a->age_out_dev, p.next_out = a->next_id_out_dev;
    p.area = a->area_dev, p.bbox = a->bbox_dev, p.moments = reinterpret_cast<long long*>(a->moments_dev);
    p.slot_of_cur = a->slot_of_cur_dev, p.linked_cur = a->linked_cur_dev, p.table = a->table_dev, p.warped = a->warped_dev, p.stats = a->stats_dev;
    return launch_segment_track(p, a->work_dev, (hipStream_t)g.stream);
}
