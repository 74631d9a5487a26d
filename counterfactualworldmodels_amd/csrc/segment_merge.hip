// Scene segmentation, the merge (cwm_segment_merge): K candidate segments per row -- what K seeds of cwm_segment_step found -- become one label map.  Duplicates
// and parts are absorbed, segments that are nothing or everything are dropped, overlaps go to the higher-ranked object, and the per-patch coverage says where the
// next seeds belong.  No counterpart in the reference, whose README names the use and lists the algorithm as coming.
//
// The definition (this is the contract; include/cwm_hip.h repeats it for callers).  Candidates seg[b][k][y][x], bytes, nonzero = in; score[b][k] fp32 (none: all 0);
// patch size P, gh = H / P, gw = W / P; min_area, max_area (0: H W); iou_thresh, contain_thresh; absorb 0 / 1.  Per row b, in this order:
//   1 area        area[k] = the number of nonzero pixels of candidate k
//   2 valid       valid[k] = area[k] >= max(1, min_area) && area[k] <= max_area.  An empty segment (a seed that hit nothing) is never valid
//   3 inter       inter[j][k] = the number of pixels in both j and k, all K K pairs, valid or not: symmetric, the diagonal is area
//   4 order       the valid candidates in the order of select_order.h: the higher score first, a NaN above every number, -0 equal to +0, the lower index first
//   5 suppression walk the order.  k is ABSORBED by the first already-kept j, in the order they were kept, for which
//                     (float)inter[j][k] > iou_thresh * (float)(area[j] + area[k] - inter[j][k])   or
//                     (float)inter[j][k] > contain_thresh * (float)min(area[j], area[k])
//                 (one fp32 multiply and one compare each; every integer is at most 2^19 and exact in fp32; a NaN threshold compares false); otherwise k is KEPT and
//                 gets the next label 1, 2, ....  Always the candidates' own segments, never a union: the result does not chain.
//                 owner[k] = k's label if kept, its absorber's label if absorbed, 0 if not valid
//   6 paint       the painting set of label m: its keeper's segment, plus the segments of the candidates it absorbed when `absorb` is set.
//                 labels[p] = the lowest m whose painting set holds p, 0 where there is none: overlaps between kept objects go to the higher-ranked one.
//                 A label's region may end up disconnected (an overlap cut out of it, an absorbed part that does not touch it): there is no clean-up pass
//   7 label_area  label_area[m - 1] = the number of pixels with label m, m = 1 .. K; 0 for labels that do not exist
//   8 cover       cover[cell] = (#pixels of the cell with a label > 0) / (float)(P P), exact for P = 4, 8, 16
//   9 stats       (n_valid, num_labels, #labelled pixels, n_absorbed = n_valid - num_labels)
//
// Five kernels behind one memset, all on base.stream.  What was chosen, and why:
//   pack      a thread reads 16 pixels as one 16-byte load and makes 16 bits of them; two lanes make a word (one shuffle).  The issue's sketch has one pixel per lane and
//             64 per ballot: with 16-byte loads a ballot would collect every 16th pixel, so the bits are gathered inside the thread instead.  Planes that are not
//             16-byte aligned take byte loads.  Writes flat bit words [B][K][ceil(H W / 32)], tail bits zero; nothing later reads the bytes again.  It adds up no
//             popcounts: area is the diagonal of the intersection table, which the next kernel computes anyway
//   inter     a workgroup takes an 8 x 8 tile of (j, k) pairs (upper triangle of tiles only; the mirror is written too) and a chunk of 512 words: 16 word loads feed
//             64 AND + popcounts, so a word is read K / 8 times, not K.  Sums: registers, a 63-shuffle transpose-reduce in the wave, then INTEGER atomics -- LDS across the four waves,
//             global into a table the call zeroed itself.  Integer adds give the same bits in any order; a slab per chunk plus a reduce would cost one more pass
//             for the same bits
//   suppress  one wave per row.  The table moves to LDS; lane k ranks candidate k by counting the greater rank words (select_order.h um_rank); the walk is at most 64
//             steps: lane j tests kept j against k, a ballot and its lowest set bit give the absorber.  Writes owner, area, inter and the painting list in label order
//   paint     one workgroup per patch row (P W pixels, contiguous, a multiple of 16).  A thread owns 16 pixels, walks the painting list and claims bits not yet
//             claimed; label bytes leave as one 16-byte store (byte stores when labels_dev is not 16-byte aligned).  Cells and labels are counted with integer LDS
//             atomics; cover is written from LDS, label areas go to the zeroed table with one integer atomic per label and workgroup
//   finish    one wave per row: label_area and stats
// No content of a device table moves an address beyond what the geometry allows: scores only order lane indices 0 .. K-1, and the painting list is read back
// clamped into [0, K).  The call does not depend on what work_dev holds on entry.
#include <cstring>

#include "../../include/cwm_hip.h"
#include "common.h"
#include "kernels.h"
#include "select_order.h"

namespace cwm {

namespace {

constexpr int kMergeMaxK = 64;
constexpr int kMergeMaxPixels = 1 << 18;
constexpr int kMergeThreads = 256;
constexpr int kTile = 8;                         // candidates per side of a pair tile
constexpr int kChunkWords = 2 * kMergeThreads;   // words of a plane per intersection workgroup
constexpr int kPaintBatch = 8;                   // list entries whose words a paint thread loads together (divides kMergeMaxK)

struct MergeParams {
    const uint8_t* segs;
    int64_t sb, sk;
    const float* scores;
    int B, K, H, W, P;
    int min_area, max_area;
    float iou_thresh, contain_thresh;
    int absorb;
    // workspace
    int* w_inter;        // [B][K][K], zeroed by the call
    int* w_label_area;   // [B][K], zeroed by the call
    int* w_meta;         // [B][4]: n_list, num_labels, n_valid
    int* w_list;         // [B][K]: candidate | label << 8, in label order
    unsigned* w_bits;    // [B][K][Wn]
    // outputs
    uint8_t* labels;
    int *owner, *area, *label_area, *inter;
    float* cover;
    int* stats;
};

struct MergeLayout {
    size_t inter, label_area, meta, list, bits, total;  // byte offsets, each a multiple of 16
};
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
int words_of(int HW) { return (HW + 31) / 32; }
MergeLayout merge_layout(int B, int K, int HW) {
    MergeLayout l;
    l.inter = 0;
    l.label_area = (size_t)B * K * K * sizeof(int);  // (directly behind inter: one memset clears both)
    l.meta = align16(l.label_area + (size_t)B * K * sizeof(int));
    l.list = align16(l.meta + (size_t)B * 4 * sizeof(int));
    l.bits = align16(l.list + (size_t)B * K * sizeof(int));
    l.total = align16(l.bits + (size_t)B * K * words_of(HW) * sizeof(unsigned));
    return l;
}
bool merge_sizes_ok(int B, int K, int H, int W) {
    return B >= 1 && B <= 65535 && K >= 1 && K <= kMergeMaxK && H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0 && (int64_t)H * W <= kMergeMaxPixels;
}

// grid (groups of 16 pixels / 256, K, B)
__global__ __launch_bounds__(kMergeThreads) void merge_pack_kernel(const uint8_t* __restrict__ segs, int64_t sb, int64_t sk, int K, int HW, int Wn,
                                                                   unsigned* __restrict__ bits) {
    const int k = blockIdx.y, b = blockIdx.z;
    const int g = blockIdx.x * kMergeThreads + (int)threadIdx.x, groups = HW >> 4;  // HW % 16 == 0
    const uint8_t* plane = segs + (int64_t)b * sb + (int64_t)k * sk;
    unsigned m = 0;
    if (g < groups) {
        const uint8_t* q = plane + 16 * (size_t)g;
        if ((reinterpret_cast<uintptr_t>(plane) & 15) == 0) {
            const uint4 v = *reinterpret_cast<const uint4*>(q);
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) m |= ((w[i] >> (8 * j)) & 0xffu) ? 1u << (4 * i + j) : 0u;
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) m |= q[i] ? 1u << i : 0u;
        }
    }
    const unsigned other = (unsigned)__shfl_xor((int)m, 1, 64);  // every lane takes part; a group past the plane holds 0: the tail bits of the last word
    if ((g & 1) == 0 && g < groups) bits[((size_t)b * K + k) * Wn + (g >> 1)] = m | (other << 16);
}

// grid (chunks of kChunkWords words, upper-triangle tiles, B)
__global__ __launch_bounds__(kMergeThreads) void merge_inter_kernel(const unsigned* __restrict__ bits, int K, int Wn, int* __restrict__ inter) {
    __shared__ int red[kTile * kTile];
    const int b = blockIdx.z, tid = threadIdx.x, T = (K + kTile - 1) / kTile;
    int tj = 0, t = blockIdx.y;  // tile t of the upper triangle, row by row: (0,0) (0,1) .. (0,T-1) (1,1) ..
    while (t >= T - tj) t -= T - tj, ++tj;
    const int tk = tj + t;
    const int j0 = tj * kTile, k0 = tk * kTile;
    if (tid < kTile * kTile) red[tid] = 0;
    __syncthreads();
    int acc[kTile * kTile];  // pair (i, j) of the tile at i kTile + j
#pragma unroll
    for (int e = 0; e < kTile * kTile; ++e) acc[e] = 0;
    const unsigned* base = bits + (size_t)b * K * Wn;
    const int w0 = blockIdx.x * kChunkWords;
    for (int w = w0 + tid; w < min(w0 + kChunkWords, Wn); w += kMergeThreads) {
        unsigned a[kTile], c[kTile];
#pragma unroll
        for (int i = 0; i < kTile; ++i) {
            a[i] = j0 + i < K ? base[(size_t)(j0 + i) * Wn + w] : 0u;
            c[i] = k0 + i < K ? base[(size_t)(k0 + i) * Wn + w] : 0u;
        }
#pragma unroll
        for (int i = 0; i < kTile; ++i)
#pragma unroll
            for (int j = 0; j < kTile; ++j) acc[i * kTile + j] += __popc(a[i] & c[j]);
    }
    // 64 sums over the 64 lanes of a wave in 63 shuffles: at offset o a lane keeps the half of its values that its bit o selects and hands the other half to
    // lane ^ o, so that after the six steps lane l holds the wave's sum of pair l.  Every index is a compile-time constant (the loops are unrolled)
    static_assert(kTile * kTile == 64, "one pair per lane");
    const int lane = tid & 63;
#pragma unroll
    for (int half = 32; half; half >>= 1) {
        const bool up = lane & half;
#pragma unroll
        for (int e = 0; e < half; ++e) {
            const int keep = up ? acc[e + half] : acc[e], send = up ? acc[e] : acc[e + half];
            acc[e] = keep + __shfl_xor(send, half, 64);
        }
    }
    atomicAdd(&red[lane], acc[0]);  // the four waves
    __syncthreads();
    if (tid < kTile * kTile) {
        const int j = j0 + tid / kTile, k = k0 + tid % kTile;
        if (j < K && k < K) {
            int* row = inter + (size_t)b * K * K;
            atomicAdd(&row[j * K + k], red[tid]);
            if (tj != tk) atomicAdd(&row[k * K + j], red[tid]);  // (a diagonal tile holds both (j, k) and (k, j) itself)
        }
    }
}

// one wave per row
__global__ __launch_bounds__(64) void merge_suppress_kernel(const MergeParams p) {
    __shared__ int tab[kMergeMaxK * kMergeMaxK];
    __shared__ int ord[kMergeMaxK];
    const int b = blockIdx.x, lane = threadIdx.x, K = p.K;
    const int* src = p.w_inter + (size_t)b * K * K;
#pragma unroll 16
    for (int e = lane; e < K * K; e += 64) tab[e] = src[e];  // (nothing but loads and LDS stores: the loads of a batch are in flight together)
    __syncthreads();
    if (p.inter)
        for (int e = lane; e < K * K; e += 64) p.inter[(size_t)b * K * K + e] = tab[e];
    const bool mine = lane < K;
    const int area = mine ? tab[lane * K + lane] : 0;
    const int lo = p.min_area > 1 ? p.min_area : 1, hi = p.max_area > 0 ? p.max_area : p.H * p.W;
    const bool valid = mine && area >= lo && area <= hi;
    const unsigned long long word = valid ? um_rank(1, p.scores ? p.scores[(size_t)b * K + lane] : 0.f, lane) : 0ull;
    int pos = 0;
    for (int j = 0; j < 64; ++j) pos += (unsigned long long)__shfl((long long)word, j, 64) > word;
    if (valid) ord[pos] = lane;  // the rank words of valid candidates differ (their low bits hold the index): pos is a permutation of 0 .. n_valid-1
    const int n_valid = __popcll(__ballot(valid));
    __syncthreads();

    int kept = 0;                  // lane l < nkept: the candidate with label l + 1
    int karea = 0;
    int owner = 0, nkept = 0;
    for (int r = 0; r < n_valid; ++r) {
        const int k = ord[r] & (kMergeMaxK - 1);
        const int ak = tab[k * K + k];
        bool hit = false;
        if (lane < nkept) {
            const int I = tab[kept * K + k];
            hit = (float)I > p.iou_thresh * (float)(karea + ak - I) || (float)I > p.contain_thresh * (float)min(karea, ak);
        }
        const unsigned long long hits = __ballot(hit);
        if (hits) {
            const int j = __ffsll((long long)hits) - 1;
            if (lane == k) owner = j + 1;
        } else {
            if (lane == nkept) kept = k, karea = ak;
            if (lane == k) owner = nkept + 1;
            ++nkept;
        }
    }
    // which label paints candidate `lane`: its owner when it is kept, or absorbed with `absorb` set
    unsigned long long keepers = 0;
    for (int l = 0; l < nkept; ++l) keepers |= 1ull << __shfl(kept, l, 64);
    const bool paints = valid && owner > 0 && (p.absorb || ((keepers >> lane) & 1ull));
    const int key = paints ? owner * 64 + lane : 1 << 30;
    int at = 0;
    for (int j = 0; j < 64; ++j) at += __shfl(key, j, 64) < key;
    if (paints) p.w_list[(size_t)b * K + at] = lane | (owner << 8);
    const int n_list = __popcll(__ballot(paints));
    if (mine) {
        if (p.owner) p.owner[(size_t)b * K + lane] = owner;
        if (p.area) p.area[(size_t)b * K + lane] = area;
    }
    if (lane == 0) {
        int* meta = p.w_meta + 4 * (size_t)b;
        meta[0] = n_list, meta[1] = nkept, meta[2] = n_valid, meta[3] = 0;
    }
}

// grid (gh, B): one workgroup per patch row
__global__ __launch_bounds__(kMergeThreads) void merge_paint_kernel(const MergeParams p, int Wn) {
    __shared__ int cnt[kSelMaxCells];  // labelled pixels of the gw cells of the patch row
    __shared__ int la[kMergeMaxK];
    __shared__ int list[kMergeMaxK];
    const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, K = p.K, W = p.W, P = p.P, gw = W / P;
    const int n_list = min(max(p.w_meta[4 * (size_t)b], 0), K);
    for (int c = tid; c < gw; c += kMergeThreads) cnt[c] = 0;
    if (tid < kMergeMaxK) {
        la[tid] = 0;
        list[tid] = tid < n_list ? p.w_list[(size_t)b * K + tid] : 0;
    }
    __syncthreads();
    const int pix_row0 = i * P * W, groups = (P * W) >> 4;
    const unsigned* bits = p.w_bits + (size_t)b * K * Wn;
    uint8_t* out = p.labels ? p.labels + (size_t)b * p.H * W : nullptr;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (int g = tid; g < groups; g += kMergeThreads) {
        const int pix = pix_row0 + 16 * g, word = pix >> 5, sh = pix & 16;
        unsigned claimed = 0, o[4] = {0, 0, 0, 0};
        for (int e0 = 0; e0 < n_list && claimed != 0xffffu; e0 += kPaintBatch) {
            unsigned got[kPaintBatch];  // the words of a batch of list entries are loaded together, not one dependent load per entry (measured: no slower, no faster)
#pragma unroll
            for (int u = 0; u < kPaintBatch; ++u)
                got[u] = e0 + u < n_list ? (bits[(size_t)min(list[e0 + u] & 0xff, K - 1) * Wn + word] >> sh) & 0xffffu : 0u;
#pragma unroll
            for (int u = 0; u < kPaintBatch; ++u) {
                const unsigned claim = got[u] & ~claimed;
                if (!claim) continue;
                const int label = min(max(list[min(e0 + u, kMergeMaxK - 1)] >> 8, 1), K);
                claimed |= claim;
                atomicAdd(&la[label - 1], __popc(claim));
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned nib = (claim >> (4 * q)) & 0xfu;
                    o[q] |= ((nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21)) * (unsigned)label;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // four pixels from a multiple of 4: one image row, one cell (P and W are multiples of 4)
            const int c = __popc((claimed >> (4 * q)) & 0xfu);
            if (c) atomicAdd(&cnt[((pix + 4 * q) % W) / P], c);
        }
        if (out) {
            if (vec) {
                *reinterpret_cast<uint4*>(out + pix) = make_uint4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int q = 0; q < 16; ++q) out[pix + q] = (uint8_t)(o[q >> 2] >> (8 * (q & 3)));
            }
        }
    }
    __syncthreads();
    if (p.cover)
        for (int c = tid; c < gw; c += kMergeThreads) p.cover[((size_t)b * gridDim.x + i) * gw + c] = (float)cnt[c] / (float)(P * P);
    if (tid < K && la[tid]) atomicAdd(&p.w_label_area[(size_t)b * K + tid], la[tid]);
}

// one wave per row
__global__ __launch_bounds__(64) void merge_finish_kernel(const MergeParams p) {
    const int b = blockIdx.x, lane = threadIdx.x, K = p.K;
    const int v = lane < K ? p.w_label_area[(size_t)b * K + lane] : 0;
    if (lane < K && p.label_area) p.label_area[(size_t)b * K + lane] = v;
    int sum = v;
#pragma unroll
    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0 && p.stats) {
        const int* meta = p.w_meta + 4 * (size_t)b;
        int* st = p.stats + 4 * (size_t)b;
        st[0] = meta[2], st[1] = meta[1], st[2] = sum, st[3] = meta[2] - meta[1];
    }
}

int launch_segment_merge(const MergeParams& q, void* work, hipStream_t stream) {
    MergeParams p = q;
    const int HW = p.H * p.W, Wn = words_of(HW);
    const MergeLayout l = merge_layout(p.B, p.K, HW);
    char* w = static_cast<char*>(work);
    p.w_inter = reinterpret_cast<int*>(w + l.inter), p.w_label_area = reinterpret_cast<int*>(w + l.label_area);
    p.w_meta = reinterpret_cast<int*>(w + l.meta), p.w_list = reinterpret_cast<int*>(w + l.list), p.w_bits = reinterpret_cast<unsigned*>(w + l.bits);
    CWM_HIP_CHECK(hipMemsetAsync(w, 0, l.label_area + (size_t)p.B * p.K * sizeof(int), stream));  // the two tables the kernels add into
    const int groups = HW / 16, T = (p.K + kTile - 1) / kTile;
    hipLaunchKernelGGL(merge_pack_kernel, dim3((unsigned)((groups + kMergeThreads - 1) / kMergeThreads), (unsigned)p.K, (unsigned)p.B), dim3(kMergeThreads), 0, stream,
                       p.segs, p.sb, p.sk, p.K, HW, Wn, p.w_bits);
    CWM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(merge_inter_kernel, dim3((unsigned)((Wn + kChunkWords - 1) / kChunkWords), (unsigned)(T * (T + 1) / 2), (unsigned)p.B), dim3(kMergeThreads), 0,
                       stream, p.w_bits, p.K, Wn, p.w_inter);
    CWM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(merge_suppress_kernel, dim3((unsigned)p.B), dim3(64), 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(merge_paint_kernel, dim3((unsigned)(p.H / p.P), (unsigned)p.B), dim3(kMergeThreads), 0, stream, p, Wn);
    CWM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(merge_finish_kernel, dim3((unsigned)p.B), dim3(64), 0, stream, p);
    CWM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

}  // namespace cwm

using namespace cwm;

extern "C" size_t cwm_segment_merge_work_bytes(int B, int K, int H, int W) {
    return merge_sizes_ok(B, K, H, W) ? merge_layout(B, K, H * W).total : 0;
}

extern "C" int cwm_segment_merge(const cwm_segment_merge_args* a) {
    CWM_REQUIRE(a && a->struct_size == sizeof(cwm_segment_merge_args), "cwm_segment_merge: args->struct_size must be sizeof(cwm_segment_merge_args)");
    const cwm_patch_error_args& g = a->base;
    CWM_REQUIRE(g.T == 2, "cwm_segment_merge: base.T = %d (two frames, as cwm_segment_step)", g.T);
    const PatchGrid grid = {g.batch, 2, 0, g.H, g.W, g.P, 0, 0, 0};
    if (int rc = check_patch_grid("cwm_segment_merge: base.", grid, 0)) return rc;
    CWM_REQUIRE(g.batch <= 65535, "cwm_segment_merge: base.batch = %d, 1 .. 65535", g.batch);
    CWM_REQUIRE((int64_t)g.H * g.W <= kMergeMaxPixels, "cwm_segment_merge: base.H base.W = %lld pixels, at most %d", (long long)g.H * g.W, kMergeMaxPixels);
    CWM_REQUIRE((g.H / g.P) * (g.W / g.P) <= kSelMaxCells, "cwm_segment_merge: n = %d patches per frame, at most %d", (g.H / g.P) * (g.W / g.P), kSelMaxCells);
    CWM_REQUIRE(a->K >= 1 && a->K <= kMergeMaxK, "cwm_segment_merge: K = %d, 1 .. %d", a->K, kMergeMaxK);
    CWM_REQUIRE(a->segs_dev, "cwm_segment_merge: segs_dev is required");
    CWM_REQUIRE(a->seg_strides[0] >= 0 && a->seg_strides[1] >= 0, "cwm_segment_merge: seg_strides = (%lld, %lld) must not be negative", (long long)a->seg_strides[0],
                (long long)a->seg_strides[1]);
    CWM_REQUIRE(a->min_area >= 0, "cwm_segment_merge: min_area = %d must not be negative", a->min_area);
    CWM_REQUIRE(a->max_area >= 0, "cwm_segment_merge: max_area = %d must not be negative (0: H W)", a->max_area);
    CWM_REQUIRE(a->absorb == 0 || a->absorb == 1, "cwm_segment_merge: absorb = %d, 0 or 1", a->absorb);
    CWM_REQUIRE(a->work_dev && (reinterpret_cast<uintptr_t>(a->work_dev) & 15) == 0, "cwm_segment_merge: work_dev = %p must be a 16-byte aligned device address", a->work_dev);
    const size_t need = cwm_segment_merge_work_bytes(g.batch, a->K, g.H, g.W);
    CWM_REQUIRE(a->work_bytes >= need, "cwm_segment_merge: work_bytes = %llu, cwm_segment_merge_work_bytes gives %llu", (unsigned long long)a->work_bytes,
                (unsigned long long)need);
    MergeParams p;
    memset(&p, 0, sizeof(p));
    p.segs = a->segs_dev, p.sb = a->seg_strides[0], p.sk = a->seg_strides[1], p.scores = a->scores_dev;
    p.B = g.batch, p.K = a->K, p.H = g.H, p.W = g.W, p.P = g.P;
    p.min_area = a->min_area, p.max_area = a->max_area, p.iou_thresh = a->iou_thresh, p.contain_thresh = a->contain_thresh, p.absorb = a->absorb;
    p.labels = a->labels_dev, p.owner = a->owner_dev, p.area = a->area_dev, p.label_area = a->label_area_dev, p.inter = a->inter_dev, p.cover = a->cover_dev;
    p.stats = a->stats_dev;
    return launch_segment_merge(p, a->work_dev, (hipStream_t)g.stream);
}
