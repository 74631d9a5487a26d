// RAFT-large optical flow behind the C ABI (include/cwm_hip.h cwm_raft_*): cwm/models/raft/raft_model.py:103-300 in its inference
// configuration -- BasicEncoder fnet (instance norm) and cnet (eval batch norm, folded into the convolutions at load), 4-level all-pairs
// correlation of radius 4, BasicUpdateBlock with SepConvGRU, convex upsampling.  Every convolution is an im2col (raft_kernels.hip) and a
// GEMM on launch_gemm whose fp32 epilogue writes straight into a channel slice of an NHWC buffer.  The call chooses the arithmetic of these
// convolutions (cwm_raft_forward_args.mode): parity (split-bf16 operands, planes = 2) or fast (one bf16 plane per operand, planes = 1);
// everything between them -- norm statistics, residual join, correlation, lookup, coordinates, GRU update, upsampling -- is fp32 in both.  The mask head and
// the upsampling run once, after the last iteration (the reference computes them every iteration and returns the last), unless a call asks for
// every iteration's prediction (cwm_raft_forward_ex: flow_iters_dev / head_iters_dev; the same entry point takes the warm start, flow_init_dev).  So does the optional
// output head (raft_model.py:152-159, output_dim = 1: the keypoint predictor): output_block.0 as one more 3x3 convolution, then the 256 -> 1
// projection as a kernel of its own and the convex upsampling kernel once more, on one channel (raft_kernels.hip).
// The state dict lives in the engine's slot table (engine.h Slot: the raw fp32 tensors as vector slots, num_batches_tracked ignored; the head's keys and
// num_batches_tracked optional); prepare() packs the convolutions from it when Engine::loads has moved.  What a convolution launch is made of (geometry,
// packing of the weight parts, GEMM params) is stated once in raft_kernels.hip, for this file and for dev.hip's cwm_dev_raft_conv; the correlation pyramid
// once here (build_pyramid), for the forward and the stand-alone lookup.  A handle may instead compute the correlations at lookup time
// (cwm_raft_set_corr, AlternateCorrBlock of raft/corr.py:63-91): build_fmap_levels pools fmap2 three times in place of the pyramid, and the lookup of
// every iteration is corr_lookup_on_the_fly_kernel; nothing else of the forward changes.  A handle may also run the encoders once per distinct frame of a
// call (cwm_raft_set_share_frames): raft_frame_plan reads what repeats off the two image sources' strides, the encoders run over the plan's frames, and the
// consumers of their maps (correlation, fmap2's poolings, the on-the-fly lookup, the context split) find each pair's maps by slot (kernels.h FramePlan, SlotMap).
#include <stddef.h>

#include "engine.h"

using namespace cwm;

namespace {

constexpr int kMaxPlanes = 2;  // the im2col workspaces hold the parity layout, so one handle serves both modes
constexpr int kFeat = 256;  // fnet output width
constexpr int kLookupKpad = 384;  // 4 levels x 81 = 324 correlation features, padded to the GEMM's K granule
constexpr int kMaxEncImages = 32;  // images per encoder pass (bounds the im2col buffer: 29 MB per 224^2 image)

struct ConvPart {
    std::string w, b, bn;  // weight / bias keys; bn: prefix of the batch norm folded into this convolution ("" = none)
    int n = 0;             // output channels
};

struct RaftConv {
    LinearW L;  // N = output channels of all parts rounded up to 16 (zero rows / bias beyond), K = kh * kw * cin
    int cin = 0, kh = 1, kw = 1, stride = 1, pad_h = 0, pad_w = 0;
    std::vector<ConvPart> parts;
};

struct Block {
    RaftConv c1, c2, down;
    bool has_down = false;
};

struct Encoder {
    bool instance = false;
    RaftConv conv1, conv2;
    Block blocks[6];
};

// the output head's state-dict keys, in the reference's order
const char* const kHeadKeys[4] = {"output_block.0.weight", "output_block.0.bias", "output_block.2.weight", "output_block.2.bias"};

ConvSrc src_of(const float* p, int C, const float* stats = nullptr, int relu = 0, int ld = 0) {
    ConvSrc s = {};
    s.p = p;
    s.C = C;
    s.ld = ld ? ld : C;
    s.stats = stats;
    s.relu = relu;
    return s;
}

}  // namespace

struct cwm_raft_model {
    Engine eng;  // its slot table holds the raw fp32 tensors of the state dict (Slot::dst), from which prepare() packs the convolutions
    std::vector<RaftConv*> convs;
    uint64_t packed_at = ~0ull;  // eng.loads when the convolutions were last packed
    Encoder fnet, cnet;
    RaftConv convc1, convc2, convf1, convf2, conv, zr[2], q[2], fh1, fh2, mask0, mask2, out0;
    int corr = CWM_RAFT_CORR_ALL_PAIRS;  // cwm_raft_set_corr
    int share = 0;                       // cwm_raft_set_share_frames
    int last_fnet = 0, last_cnet = 0;    // cwm_raft_encoder_images: what the last forward's plan ran through each encoder
    // workspace (cached by shape, by `corr` and by the frame counts of the plan: pairs, fnet frames, cnet frames, distinct image2 frames)
    int ws_P = 0, ws_nf = 0, ws_nc = 0, ws_n2 = 0, ws_H = 0, ws_W = 0, ws_corr = CWM_RAFT_CORR_ALL_PAIRS;
    float *enc_act[4] = {nullptr, nullptr, nullptr, nullptr}, *enc_stats[4] = {nullptr, nullptr, nullptr, nullptr};
    bf16* enc_A = nullptr;
    double* enc_norm_work = nullptr;
    float *fmap = nullptr, *cn = nullptr, *pyr[4] = {nullptr, nullptr, nullptr, nullptr};
    float* f2lvl[4] = {nullptr, nullptr, nullptr, nullptr};  // on-the-fly correlation: fmap2 pooled to levels 1 .. 3 (level 0 is fmap's second half) in place of pyr
    bf16 *corrA = nullptr, *updA = nullptr;
    float *c1 = nullptr, *cf = nullptr, *f1 = nullptr, *x = nullptr, *h = nullptr, *zrb = nullptr, *qb = nullptr, *fh = nullptr, *d = nullptr,
          *coords = nullptr, *mask = nullptr;
};

namespace {

const Slot& slot(cwm_raft_model* m, const std::string& key) { return m->eng.slots.at(key); }

void add_bn(cwm_raft_model* m, const std::string& pre, int c) {
    for (const char* p : {"weight", "bias", "running_mean", "running_var"}) m->eng.add_vec_slot(pre + "." + p, nullptr, {c});
    m->eng.add_ignored_slot(pre + ".num_batches_tracked", {});
    m->eng.slots[pre + ".num_batches_tracked"].optional = true;
}

int make_conv(cwm_raft_model* m, RaftConv& cv, std::vector<ConvPart> parts, int cin, int kh, int kw, int stride, int pad_h, int pad_w) {
    cv.cin = cin;
    cv.kh = kh;
    cv.kw = kw;
    cv.stride = stride;
    cv.pad_h = pad_h;
    cv.pad_w = pad_w;
    cv.parts = parts;
    int n = 0;
    for (auto& p : parts) {
        m->eng.add_vec_slot(p.w, nullptr, {p.n, cin, kh, kw});
        m->eng.add_vec_slot(p.b, nullptr, {p.n});
        n += p.n;
    }
    m->convs.push_back(&cv);
    return m->eng.make_linear(cv.L, round_up(n, 16), kh * kw * cin, true);
}

int make_encoder(cwm_raft_model* m, Encoder& e, const std::string& pre, bool instance, int out_dim) {
    e.instance = instance;
    auto bn = [&](const std::string& name, int c) -> std::string {
        if (instance) return "";
        add_bn(m, pre + name, c);
        return pre + name;
    };
    const std::string n1 = bn("norm1", 64);
    int rc;
    if ((rc = make_conv(m, e.conv1, {{pre + "conv1.weight", pre + "conv1.bias", n1, 64}}, 3, 7, 7, 2, 3, 3))) return rc;
    int cin = 64, bi = 0;
    const int dims[3] = {64, 96, 128};
    for (int li = 0; li < 3; ++li)
        for (int j = 0; j < 2; ++j, ++bi) {
            Block& B = e.blocks[bi];
            const std::string b = pre + "layer" + std::to_string(li + 1) + "." + std::to_string(j) + ".";
            const std::string bl = "layer" + std::to_string(li + 1) + "." + std::to_string(j) + ".";
            const int dim = dims[li], stride = (li > 0 && j == 0) ? 2 : 1;
            const std::string bn1 = bn(bl + "norm1", dim), bn2 = bn(bl + "norm2", dim);
            if ((rc = make_conv(m, B.c1, {{b + "conv1.weight", b + "conv1.bias", bn1, dim}}, cin, 3, 3, stride, 1, 1))) return rc;
            if ((rc = make_conv(m, B.c2, {{b + "conv2.weight", b + "conv2.bias", bn2, dim}}, dim, 3, 3, 1, 1, 1))) return rc;
            if (stride != 1) {
                B.has_down = true;
                bn(bl + "norm3", dim);  // the same module as downsample.1 (listed twice in the state dict); downsample.1 is what load_state_dict keeps
                const std::string bn3 = bn(bl + "downsample.1", dim);
                if ((rc = make_conv(m, B.down, {{b + "downsample.0.weight", b + "downsample.0.bias", bn3, dim}}, cin, 1, 1, 2, 0, 0))) return rc;
            }
            cin = dim;
        }
    return make_conv(m, e.conv2, {{pre + "conv2.weight", pre + "conv2.bias", "", out_dim}}, 128, 1, 1, 1, 0, 0);
}

// Packs every convolution whose weights are loaded (the caller has checked that none but the optional ones is missing), when a load has changed one
int prepare(cwm_raft_model* m) {
    if (m->packed_at == m->eng.loads) return 0;
    for (RaftConv* cv : m->convs) {
        if (!slot(m, cv->parts[0].w).loaded || !slot(m, cv->parts[0].b).loaded) continue;  // output_block.0 of a model without the head
        std::vector<ConvPartW> parts;
        for (auto& p : cv->parts) {
            ConvPartW w = {slot(m, p.w).dst, slot(m, p.b).dst, nullptr, nullptr, nullptr, nullptr, p.n};
            if (!p.bn.empty()) {
                w.gamma = slot(m, p.bn + ".weight").dst;
                w.beta = slot(m, p.bn + ".bias").dst;
                w.mean = slot(m, p.bn + ".running_mean").dst;
                w.var = slot(m, p.bn + ".running_var").dst;
            }
            parts.push_back(w);
        }
        if (int rc = pack_conv_parts(parts.data(), (int)parts.size(), 1e-5f, cv->cin, cv->kh, cv->kw, cv->L.Kpad, cv->L.w_il, cv->L.w, cv->L.bias, 0)) return rc;
    }
    CWM_HIP_CHECK(hipGetLastError());
    CWM_HIP_CHECK(hipDeviceSynchronize());
    m->packed_at = m->eng.loads;
    return 0;
}

// side of pyramid level l (avg_pool2d(2, stride 2), floor, l times)
int level_sides(int s, int l) { return s >> l; }

// P pairs whose encoders run on nf (fnet) and nc (cnet) frames, n2 of them distinct second images: 2 P, P and P unless the forward shares frames
int ensure_workspace(cwm_raft_model* m, int P, int nf, int nc, int n2, int H, int W) {
    if (m->ws_P >= P && m->ws_nf >= nf && m->ws_nc >= nc && m->ws_n2 >= n2 && m->ws_H == H && m->ws_W == W && m->ws_corr == m->corr) return 0;
    Engine& E = m->eng;
    if (int rc = E.free_workspace()) return rc;
    m->ws_P = 0;
    const int64_t hw2 = (int64_t)(H / 2) * (W / 2), hw8 = (int64_t)(H / 8) * (W / 8), M = P * hw8;
    const int64_t n = std::min(std::max(nf, nc), kMaxEncImages);
    int rc = 0;
    for (int i = 0; i < 4 && !rc; ++i) rc = E.ws(&m->enc_act[i], (size_t)(n * hw2 * 64));
    for (int i = 0; i < 4 && !rc; ++i) rc = E.ws(&m->enc_stats[i], (size_t)(n * 128 * 2));
    if (rc || (rc = E.ws(&m->enc_A, (size_t)(n * hw2 * 576 * kMaxPlanes))) || (rc = E.ws(&m->enc_norm_work, (size_t)(2 * n * kInstNormMaxChunks * 128))))
        return rc;
    if ((rc = E.ws(&m->fmap, (size_t)(nf * hw8 * kFeat))) || (rc = E.ws(&m->cn, (size_t)(nc * hw8 * 256)))) return rc;
    for (int l = 0; l < 4; ++l) m->pyr[l] = m->f2lvl[l] = nullptr;
    for (int l = 0; l < 4 && !rc; ++l) {
        const int64_t hw = (int64_t)level_sides(H / 8, l) * level_sides(W / 8, l);
        if (m->corr == CWM_RAFT_CORR_ALL_PAIRS) rc = E.ws(&m->pyr[l], (size_t)(M * hw));
        else if (l > 0) rc = E.ws(&m->f2lvl[l], (size_t)(n2 * hw * kFeat));
    }
    if (rc || (rc = E.ws(&m->corrA, (size_t)(M * kLookupKpad * kMaxPlanes))) || (rc = E.ws(&m->updA, (size_t)(M * 2304 * kMaxPlanes)))) return rc;
    if ((rc = E.ws(&m->c1, (size_t)(M * 256))) || (rc = E.ws(&m->cf, (size_t)(M * 256))) || (rc = E.ws(&m->f1, (size_t)(M * 128))) ||
        (rc = E.ws(&m->x, (size_t)(M * 256))) || (rc = E.ws(&m->h, (size_t)(M * 128))) || (rc = E.ws(&m->zrb, (size_t)(M * 256))) ||
        (rc = E.ws(&m->qb, (size_t)(M * 128))) || (rc = E.ws(&m->fh, (size_t)(M * 256))) || (rc = E.ws(&m->d, (size_t)(M * 16))) ||
        (rc = E.ws(&m->coords, (size_t)(M * 2))) || (rc = E.ws(&m->mask, (size_t)(M * 576))))
        return rc;
    m->ws_P = P;
    m->ws_nf = nf;
    m->ws_nc = nc;
    m->ws_n2 = n2;
    m->ws_H = H;
    m->ws_W = W;
    m->ws_corr = m->corr;
    return 0;
}

// one convolution: im2col of `ip` (its sources, image and channel range already set) into A, then the GEMM into C (row stride ldc), both in
// the operand layout of `planes`
int run_conv(cwm_raft_model* m, const RaftConv& cv, Im2colParams ip, int n_img, int H, int W, bf16* A, float* C, int ldc, int planes, hipStream_t s,
             bool skip_im2col = false) {
    set_conv_geometry(ip, n_img, H, W, cv.kh, cv.kw, cv.stride, cv.pad_h, cv.pad_w, cv.L.Kpad);
    ip.A = A;
    if (!skip_im2col)
        if (int rc = launch_im2col(ip, planes, s)) return rc;
    return m->eng.run_gemm(conv_gemm(A, planes == 2 ? cv.L.w_il : cv.L.w, cv.L.bias, n_img * ip.OH * ip.OW, cv.L.N, cv.L.Kpad, C, ldc), planes, s);
}

Im2colParams im2col_of(const ConvSrc& a, const ConvSrc* b = nullptr) {
    Im2colParams ip = {};
    ip.src[0] = a;
    ip.nsrc = 1;
    if (b) {
        ip.src[1] = *b;
        ip.nsrc = 2;
    }
    return ip;
}

// BasicEncoder.forward (extractor.py:160-192) on images [img0, img0 + n) of `image`; output [n][H/8 * W/8][out width] at `out`.  `runs` (a forward that
// shares frames): the images are frames [img0, img0 + n) of the `nruns` runs laid end to end instead; conv1's operand is then written run by run (one
// im2col launch per run the pass touches, at that run's rows of A) and multiplied once.
int run_encoder(cwm_raft_model* m, const Encoder& e, const ImageSrc& image, int img0, int n, int H, int W, float* out, int planes, hipStream_t s,
                const FrameRun* runs = nullptr, int nruns = 0) {
    int rc;
    float** act = m->enc_act;
    float** st = m->enc_stats;
    const float eps = 1e-5f;
    // conv1 7x7/2 -> norm1 -> relu
    Im2colParams ip = im2col_of(src_of(nullptr, 3));
    ip.image = image;
    ip.img0 = img0;
    if (runs) {
        int first = 0;  // the first frame of run r
        for (int r = 0; r < nruns; first += runs[r].n, ++r) {
            const int lo = std::max(img0, first), hi = std::min(img0 + n, first + runs[r].n);
            if (lo >= hi) continue;
            Im2colParams iq = ip;
            iq.image = ImageSrc{{runs[r].base, runs[r].base}, {runs[r].sb, runs[r].sb}, {runs[r].st, runs[r].st}, {runs[r].sc, runs[r].sc}, runs[r].n, runs[r].nt,
                                image.scale};
            iq.img0 = lo - first;
            set_conv_geometry(iq, hi - lo, H, W, e.conv1.kh, e.conv1.kw, e.conv1.stride, e.conv1.pad_h, e.conv1.pad_w, e.conv1.L.Kpad);
            iq.A = m->enc_A + (size_t)(lo - img0) * iq.OH * iq.OW * e.conv1.L.Kpad * planes;
            if ((rc = launch_im2col(iq, planes, s))) return rc;
        }
    }
    if ((rc = run_conv(m, e.conv1, ip, n, H, W, m->enc_A, act[0], 64, planes, s, runs != nullptr))) return rc;
    int h = H / 2, w = W / 2, C = 64;
    if (e.instance && (rc = launch_instnorm_stats(act[0], n, h * w, C, eps, st[0], m->enc_norm_work, s))) return rc;
    ConvSrc a = src_of(act[0], C, e.instance ? st[0] : nullptr, 1);
    for (int bi = 0; bi < 6; ++bi) {
        const Block& B = e.blocks[bi];
        const int dim = B.c1.L.N, stride = B.c1.stride;
        const int oh = (h - 1) / stride + 1, ow = (w - 1) / stride + 1;
        // y = relu(norm1(conv1(x))); y = relu(norm2(conv2(y)))
        if ((rc = run_conv(m, B.c1, im2col_of(a), n, h, w, m->enc_A, act[1], dim, planes, s))) return rc;
        if (e.instance && (rc = launch_instnorm_stats(act[1], n, oh * ow, dim, eps, st[1], m->enc_norm_work, s))) return rc;
        if ((rc = run_conv(m, B.c2, im2col_of(src_of(act[1], dim, e.instance ? st[1] : nullptr, 1)), n, oh, ow, m->enc_A, act[2], dim, planes, s))) return rc;
        if (e.instance && (rc = launch_instnorm_stats(act[2], n, oh * ow, dim, eps, st[2], m->enc_norm_work, s))) return rc;
        ConvSrc X = a;
        if (B.has_down) {  // x = norm3(downsample(x))
            if ((rc = run_conv(m, B.down, im2col_of(a), n, h, w, m->enc_A, act[3], dim, planes, s))) return rc;
            if (e.instance && (rc = launch_instnorm_stats(act[3], n, oh * ow, dim, eps, st[3], m->enc_norm_work, s))) return rc;
            X = src_of(act[3], dim, e.instance ? st[3] : nullptr, 0);
        }
        // relu(x + y), in place over the block input (an element is read and written by the same thread)
        if ((rc = launch_residual_join(X, src_of(act[2], dim, e.instance ? st[2] : nullptr, 1), n, oh * ow, act[0], s))) return rc;
        a = src_of(act[0], dim);
        h = oh;
        w = ow;
        C = dim;
    }
    return run_conv(m, e.conv2, im2col_of(a), n, h, w, m->enc_A, out, e.conv2.L.N, planes, s);
}

// CorrBlock.__init__ and the params of its lookups: the all-pairs correlation of two feature maps [P][h8 * w8][256] into pyr[0], its three poolings into
// pyr[1 .. 3] (level l: [M][h8 >> l][w8 >> l]), and `lp` over them at `coords`; the destination (A, or out / out_ld) is the caller's.  s1 / s2: where
// pair p's maps lie in fmap1 / fmap2 (kPairSlots: one per pair); the pyramid is per pair either way.
int build_pyramid(const float* fmap1, const float* fmap2, const float* coords, int P, int h8, int w8, float* const* pyr, CorrLookupParams& lp, hipStream_t s,
                  SlotMap s1 = kPairSlots, SlotMap s2 = kPairSlots) {
    const int64_t M = (int64_t)P * h8 * w8;
    lp = CorrLookupParams{};
    lp.levels = 4;
    lp.coords = coords;
    lp.M = M;
    lp.Kpad = kLookupKpad;
    if (int rc = launch_corr(fmap1, fmap2, P, h8 * w8, kFeat, pyr[0], s, s1, s2)) return rc;
    for (int l = 0; l < 4; ++l) {
        lp.pyr[l] = pyr[l];
        lp.h[l] = level_sides(h8, l);
        lp.w[l] = level_sides(w8, l);
        if (l > 0)
            if (int rc = launch_corr_pool(pyr[l - 1], M, lp.h[l - 1], lp.w[l - 1], pyr[l], s)) return rc;
    }
    return 0;
}

// AlternateCorrBlock.__init__ (corr.py:63-73) and the params of its lookups: fmap2 [P][h8][w8][256] pooled into lvl[1 .. 3] (level l: [P][h8 >> l][w8 >> l][256];
// level 0 is fmap2 itself), and `lp` over them and fmap1 at `coords`; the destination is the caller's.  `fp` (a forward that shares frames): fmap1 and
// fmap2 are the plan's, every distinct second image is pooled once (fp->n2 maps per level) and the lookup finds each pair's maps by the plan's slots.
int build_fmap_levels(const float* fmap1, const float* fmap2, const float* coords, int P, int h8, int w8, float* const* lvl, CorrOnTheFlyParams& lp,
                      hipStream_t s, const FramePlan* fp = nullptr) {
    lp = CorrOnTheFlyParams{};
    if (fp) {
        lp.ppg = fp->s1.ppg;
        lp.s1b = fp->s1.sb;
        lp.s1t = fp->s1.st;
        for (int l = 0; l < 4; ++l) {
            lp.s2b[l] = l ? fp->s2p.sb : fp->s2.sb;
            lp.s2t[l] = l ? fp->s2p.st : fp->s2.st;
        }
    }
    lp.fmap1 = fmap1;
    lp.coords = coords;
    lp.hw8 = (int64_t)h8 * w8;
    lp.M = P * lp.hw8;
    lp.Kpad = kLookupKpad;
    for (int l = 0; l < 4; ++l) {
        lp.fmap2[l] = l ? lvl[l] : fmap2;
        lp.h[l] = level_sides(h8, l);
        lp.w[l] = level_sides(w8, l);
        if (l > 0)
            if (int rc = launch_fmap_pool(lp.fmap2[l - 1], fp ? fp->n2 : P, lp.h[l - 1], lp.w[l - 1], kFeat, lvl[l], s, fp && l == 1 ? fp->pool : kPairSlots))
                return rc;
    }
    return 0;
}

// What cwm_raft_forward_ex adds to a forward; all null: the plain forward of cwm_raft_forward, launch for launch.
struct ForwardExtras {
    const float* init = nullptr;  // flow_init: coords1 = grid + init
    int64_t init_sb = 0, init_st = 0, init_sc = 0;
    float* flow_iters = nullptr;  // flow_up of iteration i at + i * flow_iters_si, addressed inside with the flow strides of the call
    int64_t flow_iters_si = 0;
    float* head_iters = nullptr;  // the upsampled output_block(net) of iteration i, likewise with the head strides
    int64_t head_iters_si = 0;
};

int forward(cwm_raft_model* m, const cwm_raft_forward_args& a, const ForwardExtras& ex) {
    hipStream_t s = (hipStream_t)a.stream;
    const int planes = a.mode == CWM_MODE_FAST ? 1 : 2;
    const int ppg = a.pairs > 0 ? a.pairs : 1;
    const int P = a.batch * ppg, H = a.height, W = a.width, h8 = H / 8, w8 = W / 8;
    const int64_t hw8 = (int64_t)h8 * w8, M = P * hw8;
    int rc;
    // the frames the encoders run on: every pair's image1 and image2, or (cwm_raft_set_share_frames) each distinct frame of a recognised pattern once
    const float* const imgs[2] = {a.image1_dev, a.image2_dev};
    const int64_t isb[2] = {a.image1_stride_b, a.image2_stride_b}, ist[2] = {a.image1_stride_t, a.image2_stride_t},
                  isc[2] = {a.image1_stride_c, a.image2_stride_c};
    const FramePlan fp = raft_frame_plan(a.batch, ppg, imgs, isb, ist, isc, m->share != 0);
    if ((rc = prepare(m)) || (rc = ensure_workspace(m, P, fp.n_fnet, fp.n_cnet, fp.n2, H, W))) return rc;
    m->last_fnet = fp.n_fnet;
    m->last_cnet = fp.n_cnet;
    const ImageSrc img = {{a.image1_dev, a.image2_dev},           {a.image1_stride_b, a.image2_stride_b}, {a.image1_stride_t, a.image2_stride_t},
                          {a.image1_stride_c, a.image2_stride_c}, P, ppg, a.input_scale};
    // feature network over image1 and image2 of every pair, or over the plan's frames (instance norm is per image: any grouping gives the same result)
    for (int i0 = 0; i0 < fp.n_fnet; i0 += kMaxEncImages) {
        const int n = std::min(kMaxEncImages, fp.n_fnet - i0);
        if ((rc = run_encoder(m, m->fnet, img, i0, n, H, W, m->fmap + (int64_t)i0 * hw8 * kFeat, planes, s, fp.shared ? fp.frun : nullptr, 2))) return rc;
    }
    // context network over image1, or over the distinct first images
    for (int i0 = 0; i0 < fp.n_cnet; i0 += kMaxEncImages) {
        const int n = std::min(kMaxEncImages, fp.n_cnet - i0);
        if ((rc = run_encoder(m, m->cnet, img, i0, n, H, W, m->cn + (int64_t)i0 * hw8 * 256, planes, s, fp.shared ? &fp.crun : nullptr, 1))) return rc;
    }
    // the GRU state and input are per pair; pairs of one first frame read one context map
    if ((rc = launch_cnet_split(m->cn, M, m->h, m->x, s, hw8, fp.shared ? fp.sc : kPairSlots))) return rc;
    const float* fmap1 = m->fmap + fp.base1 * hw8 * kFeat;
    const float* fmap2 = m->fmap + fp.base2 * hw8 * kFeat;
    // correlation pyramid, or the levels of fmap2 from which the lookup computes its taps (m->ws_corr: what the workspace was planned for)
    const bool on_the_fly = m->ws_corr == CWM_RAFT_CORR_ON_THE_FLY;
    CorrLookupParams lp = {};
    CorrOnTheFlyParams lq = {};
    if (on_the_fly) {
        if ((rc = build_fmap_levels(fmap1, fmap2, m->coords, P, h8, w8, m->f2lvl, lq, s, fp.shared ? &fp : nullptr))) return rc;
        lq.A = m->corrA;
    } else {
        if ((rc = build_pyramid(fmap1, fmap2, m->coords, P, h8, w8, m->pyr, lp, s, fp.shared ? fp.s1 : kPairSlots, fp.shared ? fp.s2 : kPairSlots))) return rc;
        lp.A = m->corrA;
    }
    if (ex.init) {
        if ((rc = launch_coords_init_flow(m->coords, P, ppg, h8, w8, ex.init, ex.init_sb, ex.init_st, ex.init_sc, s))) return rc;
    } else if ((rc = launch_coords_init(m->coords, M, h8, w8, s))) {
        return rc;
    }
    ConvSrc flow_src = {};
    flow_src.C = 2;
    flow_src.coords = m->coords;
    const bool per_iter = ex.flow_iters || ex.head_iters;
    // mask = 0.25 * mask.2(relu(mask.0(net))) (when `with_mask`), then the convex upsampling of the current flow to `flow_out` and / or of
    // output_block(net) to `head_out` (either may be null), both addressed with the strides of the call; `flow_low`: coords1 - coords0, contiguous
    auto outputs = [&](float* flow_out, float* head_out, float* flow_low, bool with_mask) -> int {
        int rc;
        if (with_mask) {
            // `fh` is free once the flow head's second convolution has read it
            if ((rc = run_conv(m, m->mask0, im2col_of(src_of(m->h, 128)), P, h8, w8, m->updA, m->fh, 256, planes, s))) return rc;
            if ((rc = run_conv(m, m->mask2, im2col_of(src_of(m->fh, 256, nullptr, 1)), P, h8, w8, m->updA, m->mask, 576, planes, s))) return rc;
        }
        if (flow_out) {
            const ConvexUpParams up =
                convex_up_params(2, m->coords, nullptr, m->mask, 0.25f, P, ppg, h8, w8, flow_out, a.flow_stride_b, a.flow_stride_t, a.flow_stride_c);
            if ((rc = launch_convex_upsample(up, s))) return rc;
        }
        if (flow_low && (rc = launch_flow_low(m->coords, P, h8, w8, flow_low, s))) return rc;
        if (head_out) {
            // out = output_block.2(relu(output_block.0(net))), upsampled with the same mask in place of the flow (raft_model.py:257-267).  `fh` is free
            // once mask.2 has read it, and `d` (the flow head's delta) once this iteration's flow update has: the projected map goes there.
            if ((rc = run_conv(m, m->out0, im2col_of(src_of(m->h, 128)), P, h8, w8, m->updA, m->fh, 256, planes, s))) return rc;
            if ((rc = launch_head_project(m->fh, 256, slot(m, kHeadKeys[2]).dst, slot(m, kHeadKeys[3]).dst, M, m->d, s))) return rc;
            const ConvexUpParams up = convex_up_params(1, nullptr, m->d, m->mask, 0.25f, P, ppg, h8, w8, head_out, a.head_stride_b, a.head_stride_t, 0);
            if ((rc = launch_convex_upsample(up, s))) return rc;
        }
        return 0;
    };
    for (int it = 0; it < a.iters; ++it) {
        // BasicMotionEncoder
        if ((rc = on_the_fly ? launch_corr_lookup_on_the_fly(lq, planes, s) : launch_corr_lookup(lp, planes, s))) return rc;
        if ((rc = run_conv(m, m->convc1, Im2colParams{}, P, h8, w8, m->corrA, m->c1, 256, planes, s, true))) return rc;
        if ((rc = run_conv(m, m->convc2, im2col_of(src_of(m->c1, 256, nullptr, 1)), P, h8, w8, m->updA, m->cf, 256, planes, s))) return rc;
        if ((rc = run_conv(m, m->convf1, im2col_of(flow_src), P, h8, w8, m->updA, m->f1, 128, planes, s))) return rc;
        if ((rc = run_conv(m, m->convf2, im2col_of(src_of(m->f1, 128, nullptr, 1)), P, h8, w8, m->updA, m->cf + 192, 256, planes, s))) return rc;
        if ((rc = run_conv(m, m->conv, im2col_of(src_of(m->cf, 256, nullptr, 1)), P, h8, w8, m->updA, m->x + 128, 256, planes, s))) return rc;
        if ((rc = launch_motion_finish(m->x, m->coords, M, h8, w8, s))) return rc;
        // SepConvGRU: (1,5) then (5,1)
        for (int pass = 0; pass < 2; ++pass) {
            const ConvSrc xs = src_of(m->x, 256);
            if ((rc = run_conv(m, m->zr[pass], im2col_of(src_of(m->h, 128), &xs), P, h8, w8, m->updA, m->zrb, 256, planes, s))) return rc;
            ConvSrc rh = src_of(m->h, 128);
            rh.gate = m->zrb + 128;
            rh.gate_ld = 256;
            Im2colParams iq = im2col_of(rh, &xs);
            iq.c_lo = 0;
            iq.c_hi = 128;  // only the h channels change: the x half of every tap is still in A
            if ((rc = run_conv(m, m->q[pass], iq, P, h8, w8, m->updA, m->qb, 128, planes, s))) return rc;
            if ((rc = launch_gru_update(m->h, m->zrb, m->qb, M, s))) return rc;
        }
        // FlowHead; coords1 += delta
        if ((rc = run_conv(m, m->fh1, im2col_of(src_of(m->h, 128)), P, h8, w8, m->updA, m->fh, 256, planes, s))) return rc;
        if ((rc = run_conv(m, m->fh2, im2col_of(src_of(m->fh, 256, nullptr, 1)), P, h8, w8, m->updA, m->d, 16, planes, s))) return rc;
        if ((rc = launch_flow_update(m->coords, m->d, 16, M, s))) return rc;
        // the per-iteration outputs (raft_model.py:257-269 keeps every iteration's flow_up): the mask head and the upsampling of this iteration's state
        if (per_iter && (rc = outputs(ex.flow_iters ? ex.flow_iters + it * ex.flow_iters_si : nullptr,
                                      ex.head_iters ? ex.head_iters + it * ex.head_iters_si : nullptr, nullptr, true)))
            return rc;
    }
    // Without per-iteration outputs the mask head and the upsampling run once, here, after the last iteration.  With them `mask` already holds the
    // last iteration's mask: the final outputs read it.
    return outputs(a.flow_dev, a.head_dev, a.flow_low_dev, !per_iter && (a.flow_dev || a.head_dev));
}

}  // namespace

extern "C" int cwm_raft_create(cwm_raft_model** out) {
    CWM_REQUIRE(out, "cwm_raft_create: null argument");
    cwm_raft_model* m = new cwm_raft_model();
    CWM_HIP_CHECK(hipGetDevice(&m->eng.device));
    int rc = 0;
    do {
        if ((rc = make_encoder(m, m->fnet, "fnet.", true, kFeat)) || (rc = make_encoder(m, m->cnet, "cnet.", false, 256))) break;
        const std::string u = "update_block.";
        auto part = [&](const std::string& name, int n) { return ConvPart{u + name + ".weight", u + name + ".bias", "", n}; };
        if ((rc = make_conv(m, m->convc1, {part("encoder.convc1", 256)}, 324, 1, 1, 1, 0, 0)) ||
            (rc = make_conv(m, m->convc2, {part("encoder.convc2", 192)}, 256, 3, 3, 1, 1, 1)) ||
            (rc = make_conv(m, m->convf1, {part("encoder.convf1", 128)}, 2, 7, 7, 1, 3, 3)) ||
            (rc = make_conv(m, m->convf2, {part("encoder.convf2", 64)}, 128, 3, 3, 1, 1, 1)) ||
            (rc = make_conv(m, m->conv, {part("encoder.conv", 126)}, 256, 3, 3, 1, 1, 1)))
            break;
        // z and r share their input: one GEMM with the two weights stacked (z: columns 0-127, r: 128-255)
        if ((rc = make_conv(m, m->zr[0], {part("gru.convz1", 128), part("gru.convr1", 128)}, 384, 1, 5, 1, 0, 2)) ||
            (rc = make_conv(m, m->q[0], {part("gru.convq1", 128)}, 384, 1, 5, 1, 0, 2)) ||
            (rc = make_conv(m, m->zr[1], {part("gru.convz2", 128), part("gru.convr2", 128)}, 384, 5, 1, 1, 2, 0)) ||
            (rc = make_conv(m, m->q[1], {part("gru.convq2", 128)}, 384, 5, 1, 1, 2, 0)))
            break;
        if ((rc = make_conv(m, m->fh1, {part("flow_head.conv1", 256)}, 128, 3, 3, 1, 1, 1)) ||
            (rc = make_conv(m, m->fh2, {part("flow_head.conv2", 2)}, 256, 3, 3, 1, 1, 1)) ||
            (rc = make_conv(m, m->mask0, {part("mask.0", 256)}, 128, 3, 3, 1, 1, 1)) ||
            (rc = make_conv(m, m->mask2, {part("mask.2", 576)}, 256, 1, 1, 1, 0, 0)))
            break;
        if ((rc = make_conv(m, m->out0, {ConvPart{kHeadKeys[0], kHeadKeys[1], "", kHeadHidden}}, 128, 3, 3, 1, 1, 1))) break;
        m->eng.add_vec_slot(kHeadKeys[2], nullptr, {1, kHeadHidden, 1, 1});
        m->eng.add_vec_slot(kHeadKeys[3], nullptr, {1});
        for (const char* k : kHeadKeys) m->eng.slots[k].optional = true;  // loaded only by models with the output head, which a forward that asks for it checks
        for (auto& kv : m->eng.slots)  // the raw fp32 tensors (registered above without a buffer): every vector slot's destination
            if (kv.second.kind == SLOT_VECTOR && (rc = m->eng.make_vec(&kv.second.dst, (int)kv.second.numel))) break;
    } while (0);
    if (rc) {
        delete m;
        return rc;
    }
    *out = m;
    return CWM_OK;
}

extern "C" void cwm_raft_destroy(cwm_raft_model* m) { delete m; }

extern "C" int cwm_raft_load_weight(cwm_raft_model* m, const char* key, const float* data, int on_device, const int64_t* shape, int ndim) {
    CWM_REQUIRE(m && key && data && (shape || ndim == 0), "cwm_raft_load_weight: null argument");
    if (int rc = cwm_require_device(m->eng.device, "cwm_raft_load_weight")) return rc;
    static const int64_t no_shape = 0;  // a 0-dimensional tensor (num_batches_tracked) may come with a null shape
    return m->eng.load_weight(key, data, on_device, shape ? shape : &no_shape, ndim);
}

extern "C" int cwm_raft_missing_weights(cwm_raft_model* m, char* buf, int buflen) { return m->eng.missing_weights(buf, buflen); }

namespace {

// The checks and the forward body that cwm_raft_forward and cwm_raft_forward_ex share; `fn`: the entry point named in the messages, `plain`: it is
// cwm_raft_forward (the messages then do not speak of the ex struct's fields).
int checked_forward(cwm_raft_model* m, const cwm_raft_forward_args* args, const ForwardExtras& ex, const char* fn, bool plain) {
    // a caller built against the 0.10.0 header (the struct ended at `stream`) or the 0.10.1 one (at `head_stride_c`) passes that size: the fields
    // appended since read as zero (no head; mode 0 = parity)
    cwm_raft_forward_args a_copy;
    if (int rc = copy_args(a_copy, args, offsetof(cwm_raft_forward_args, stream) + sizeof(void*), "cwm_raft_forward",
                           plain ? "" : "; this is cwm_raft_forward_ex_args.base.struct_size"))
        return rc;
    const cwm_raft_forward_args& a = a_copy;
    if (int rc = cwm_require_device(m->eng.device, fn)) return rc;
    CWM_REQUIRE(a.image1_dev && a.image2_dev, "%s: image1 and image2 are required", fn);
    CWM_REQUIRE(a.flow_dev || a.head_dev || ex.flow_iters || ex.head_iters,
                "%s: no output requested: one of flow / head%s is required", fn, plain ? "" : " / flow_iters / head_iters");
    CWM_REQUIRE(a.batch >= 1 && a.pairs >= 0, "%s: batch = %d, pairs = %d", fn, a.batch, a.pairs);
    CWM_REQUIRE(a.height > 0 && a.width > 0 && a.height % 8 == 0 && a.width % 8 == 0, "%s: H = %d and W = %d must be multiples of 8", fn, a.height,
                a.width);
    CWM_REQUIRE(a.height / 8 >= 16 && a.width / 8 >= 16,
                "%s: H / 8 = %d and W / 8 = %d must be at least 16 (the coarsest correlation level would have a side of 1)", fn, a.height / 8,
                a.width / 8);
    CWM_REQUIRE(a.iters >= 1, "%s: iters = %d must be >= 1", fn, a.iters);
    CWM_REQUIRE(a.mode == 0 || a.mode == CWM_MODE_PARITY || a.mode == CWM_MODE_FAST, "%s: mode = %d must be 0 or CWM_MODE_PARITY (parity) or CWM_MODE_FAST",
                fn, a.mode);
    const int planes = a.mode == CWM_MODE_FAST ? 1 : 2;
    const int64_t M = (int64_t)a.batch * std::max(a.pairs, 1) * (a.height / 8) * (a.width / 8);
    CWM_REQUIRE(M * 2304 * planes < (1ll << 32), "%s: batch too large (%lld low-resolution pixels): split it", fn, (long long)M);
    char buf[256];
    const int missing = m->eng.missing_weights(buf, sizeof(buf));
    CWM_REQUIRE(missing == 0, "%s: %d weights missing (first: %s)", fn, missing, buf);
    if (a.head_dev || ex.head_iters)
        for (const char* k : kHeadKeys)
            CWM_REQUIRE(slot(m, k).loaded, "%s: the output head was asked for (%s) but %s is not loaded", fn, a.head_dev ? "head_dev" : "head_iters_dev", k);
    return forward(m, a, ex);
}

}  // namespace

extern "C" int cwm_raft_forward(cwm_raft_model* m, const cwm_raft_forward_args* args) {
    CWM_REQUIRE(m && args, "cwm_raft_forward: null argument");
    return checked_forward(m, args, ForwardExtras(), "cwm_raft_forward", true);
}

extern "C" int cwm_raft_forward_ex(cwm_raft_model* m, const cwm_raft_forward_ex_args* args) {
    CWM_REQUIRE(m && args, "cwm_raft_forward_ex: null argument");
    // the first struct of its name: one size.  (`base` keeps the size rules of cwm_raft_forward_args.)
    CWM_REQUIRE(args->struct_size == sizeof(cwm_raft_forward_ex_args),
                "cwm_raft_forward_ex: args->struct_size = %u is not a cwm_raft_forward_ex_args (set it to sizeof(cwm_raft_forward_ex_args) = %zu)",
                args->struct_size, sizeof(cwm_raft_forward_ex_args));
    ForwardExtras ex;
    ex.init = args->flow_init_dev;
    ex.init_sb = args->flow_init_stride_b;
    ex.init_st = args->flow_init_stride_t;
    ex.init_sc = args->flow_init_stride_c;
    ex.flow_iters = args->flow_iters_dev;
    ex.flow_iters_si = args->flow_iters_stride_i;
    ex.head_iters = args->head_iters_dev;
    ex.head_iters_si = args->head_iters_stride_i;
    return checked_forward(m, &args->base, ex, "cwm_raft_forward_ex", false);
}

extern "C" int cwm_raft_set_corr(cwm_raft_model* m, int corr) {
    CWM_REQUIRE(m, "cwm_raft_set_corr: null argument");
    CWM_REQUIRE(corr == CWM_RAFT_CORR_ALL_PAIRS || corr == CWM_RAFT_CORR_ON_THE_FLY,
                "cwm_raft_set_corr: corr = %d must be CWM_RAFT_CORR_ALL_PAIRS (0) or CWM_RAFT_CORR_ON_THE_FLY (1)", corr);
    m->corr = corr;  // the next forward re-plans the workspace when this differs from what it was planned for
    return CWM_OK;
}

extern "C" int cwm_raft_set_share_frames(cwm_raft_model* m, int on) {
    CWM_REQUIRE(m, "cwm_raft_set_share_frames: null argument");
    CWM_REQUIRE(on == 0 || on == 1, "cwm_raft_set_share_frames: on = %d must be 0 or 1", on);
    m->share = on;  // the next forward plans its frames, and its workspace from their counts
    return CWM_OK;
}

extern "C" int cwm_raft_encoder_images(cwm_raft_model* m, int* fnet_images, int* cnet_images) {
    CWM_REQUIRE(m && fnet_images && cnet_images, "cwm_raft_encoder_images: null argument");
    *fnet_images = m->last_fnet;
    *cnet_images = m->last_cnet;
    return CWM_OK;
}

FramePlan cwm::raft_frame_plan(int batch, int ppg, const float* const img[2], const int64_t sb[2], const int64_t st[2], const int64_t sc[2], bool share) {
    const int P = batch * ppg;
    for (int w = 0; w < 2; ++w) share = share && sb[w] >= 0 && st[w] >= 0 && sc[w] >= 0;
    // a source's own frames: P1 / P2 fold the axis along which its stride is 0
    int nb[2], nt[2];
    SlotMap own[2];
    for (int w = 0; w < 2; ++w) {
        nb[w] = share && sb[w] == 0 && batch > 1 ? 1 : batch;
        nt[w] = share && st[w] == 0 && ppg > 1 ? 1 : ppg;
        own[w] = SlotMap{ppg, nb[w] > 1 ? nt[w] : 0, nt[w] > 1 ? 1 : 0};
    }
    // P3: image2 = image1 + k * stride_t under identical strides
    int k = 2;  // none
    if (share && sb[0] == sb[1] && st[0] == st[1] && sc[0] == sc[1]) {
        const ptrdiff_t d = img[1] - img[0];
        if (d == 0) k = 0;
        else if (ppg > 1 && st[0] > 0 && d == st[0]) k = 1;  // (a single pair per row has no interior frame to share)
        else if (ppg > 1 && st[0] > 0 && d == -st[0]) k = -1;
    }
    FramePlan fp = {};
    for (int w = 0; w < 2; ++w) fp.frun[w] = FrameRun{img[w], sb[w], st[w], sc[w], nb[w] * nt[w], nt[w]};
    fp.crun = fp.frun[0];  // cnet: image1's own frames
    fp.n_cnet = fp.crun.n;
    fp.sc = own[0];
    fp.n2 = nb[1] * nt[1];
    fp.s2p = own[1];
    if (k == 0) {  // one run serves both images
        fp.frun[1].n = 0;
        fp.s1 = fp.s2 = own[0];
    } else if (k == 1 || k == -1) {  // one run of ppg + 1 frames per row, from whichever image comes first in memory
        const int first = k == 1 ? 0 : 1;
        fp.frun[0] = FrameRun{img[first], sb[0], st[0], sc[0], nb[0] * (ppg + 1), ppg + 1};
        fp.frun[1].n = 0;
        fp.s1 = fp.s2 = SlotMap{ppg, nb[0] > 1 ? ppg + 1 : 0, 1};
        (first == 0 ? fp.base2 : fp.base1) = 1;
    } else {  // image1's frames, then image2's
        fp.s1 = own[0];
        fp.s2 = own[1];
        fp.base2 = fp.frun[0].n;
    }
    fp.n_fnet = fp.frun[0].n + fp.frun[1].n;
    fp.pool = SlotMap{nt[1], fp.s2.sb, fp.s2.st};
    fp.shared = k != 2 || fp.n_fnet != 2 * P || fp.n_cnet != P;
    return fp;
}

extern "C" int cwm_raft_workspace_bytes(cwm_raft_model* m, uint64_t* out) {
    CWM_REQUIRE(m && out, "cwm_raft_workspace_bytes: null argument");
    *out = m->eng.ws_bytes;
    return CWM_OK;
}

// ---- stand-alone kernels (kernel tests) -------------------------------------------------------------------------------
int cwm::raft_corr_lookup_run(const float* fmap1_dev, const float* fmap2_dev, const float* coords_dev, int P, int h8, int w8, float* out_dev, bf16* A,
                              int planes, hipStream_t s, SlotMap s1, SlotMap s2) {
    const int64_t M = (int64_t)P * h8 * w8;
    float* pyr[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = 0;
    for (int l = 0; l < 4 && !rc; ++l)
        if (hipMalloc((void**)&pyr[l], (size_t)M * level_sides(h8, l) * level_sides(w8, l) * sizeof(float)) != hipSuccess) {
            cwm_set_error("cwm_raft_corr_lookup: out of device memory");
            rc = CWM_ERR_HIP;
        }
    CorrLookupParams lp = {};
    if (!rc) rc = build_pyramid(fmap1_dev, fmap2_dev, coords_dev, P, h8, w8, pyr, lp, s, s1, s2);
    if (out_dev) {
        lp.out = out_dev;
        lp.out_ld = 324;
    } else {
        lp.A = A;
    }
    if (!rc) rc = launch_corr_lookup(lp, planes, s);  // (fp32 `out`: the operand layout is not used)
    if (hipStreamSynchronize(s) != hipSuccess && !rc) {
        cwm_set_error("cwm_raft_corr_lookup: stream synchronisation failed");
        rc = CWM_ERR_HIP;
    }
    for (float* p : pyr)
        if (p) (void)hipFree(p);
    return rc;
}

extern "C" int cwm_raft_corr_lookup(const float* fmap1_dev, const float* fmap2_dev, const float* coords_dev, int P, int h8, int w8, float* out_dev,
                                    void* stream) {
    CWM_REQUIRE(fmap1_dev && fmap2_dev && coords_dev && out_dev && P > 0 && h8 >= 8 && w8 >= 8, "cwm_raft_corr_lookup: bad argument");
    return raft_corr_lookup_run(fmap1_dev, fmap2_dev, coords_dev, P, h8, w8, out_dev, nullptr, 2, (hipStream_t)stream);
}

int cwm::raft_corr_lookup_on_the_fly_run(const float* fmap1_dev, const float* fmap2_dev, const float* coords_dev, int P, int h8, int w8, float* out_dev, bf16* A,
                                         int planes, hipStream_t s) {
    float* lvl[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = 0;
    for (int l = 1; l < 4 && !rc; ++l)
        if (hipMalloc((void**)&lvl[l], (size_t)P * level_sides(h8, l) * level_sides(w8, l) * kFeat * sizeof(float)) != hipSuccess) {
            cwm_set_error("cwm_raft_corr_lookup_on_the_fly: out of device memory");
            rc = CWM_ERR_HIP;
        }
    CorrOnTheFlyParams lp = {};
    if (!rc) rc = build_fmap_levels(fmap1_dev, fmap2_dev, coords_dev, P, h8, w8, lvl, lp, s);
    if (out_dev) {
        lp.out = out_dev;
        lp.out_ld = 324;
    } else {
        lp.A = A;
    }
    if (!rc) rc = launch_corr_lookup_on_the_fly(lp, planes, s);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) {
        cwm_set_error("cwm_raft_corr_lookup_on_the_fly: stream synchronisation failed");
        rc = CWM_ERR_HIP;
    }
    for (float* p : lvl)
        if (p) (void)hipFree(p);
    return rc;
}

extern "C" int cwm_raft_corr_lookup_on_the_fly(const float* fmap1_dev, const float* fmap2_dev, const float* coords_dev, int P, int h8, int w8, float* out_dev,
                                               void* stream) {
    CWM_REQUIRE(fmap1_dev && fmap2_dev && coords_dev && out_dev && P > 0 && h8 >= 8 && w8 >= 8, "cwm_raft_corr_lookup_on_the_fly: bad argument");
    return raft_corr_lookup_on_the_fly_run(fmap1_dev, fmap2_dev, coords_dev, P, h8, w8, out_dev, nullptr, 2, (hipStream_t)stream);
}

extern "C" int cwm_raft_convex_upsample(const float* flow_dev, const float* mask_dev, int P, int h8, int w8, float* out_dev, void* stream) {
    CWM_REQUIRE(flow_dev && mask_dev && out_dev && P > 0 && h8 > 0 && w8 > 0, "cwm_raft_convex_upsample: bad argument");
    const int64_t plane = (int64_t)64 * h8 * w8;
    return launch_convex_upsample(convex_up_params(2, nullptr, flow_dev, mask_dev, 1.f, P, 1, h8, w8, out_dev, 2 * plane, 0, plane), (hipStream_t)stream);
}

extern "C" int cwm_raft_forward_interpolate(const float* flow_dev, int64_t stride_p, int64_t stride_c, int P, int h8, int w8, float* out_dev, void* stream) {
    CWM_REQUIRE(flow_dev && out_dev, "cwm_raft_forward_interpolate: null pointer");
    return launch_forward_interpolate(flow_dev, stride_p, stride_c, P, h8, w8, out_dev, (hipStream_t)stream);
}

extern "C" int cwm_raft_head_project(const float* hidden_dev, const float* weight_dev, const float* bias_dev, int64_t M, float* value_dev, void* stream) {
    CWM_REQUIRE(hidden_dev && weight_dev && bias_dev && value_dev && M > 0, "cwm_raft_head_project: bad argument");
    return launch_head_project(hidden_dev, kHeadHidden, weight_dev, bias_dev, M, value_dev, (hipStream_t)stream);
}

extern "C" int cwm_raft_convex_upsample1(const float* value_dev, const float* mask_dev, int P, int h8, int w8, float* out_dev, void* stream) {
    CWM_REQUIRE(value_dev && mask_dev && out_dev && P > 0 && h8 > 0 && w8 > 0, "cwm_raft_convex_upsample1: bad argument");
    return launch_convex_upsample(convex_up_params(1, nullptr, value_dev, mask_dev, 1.f, P, 1, h8, w8, out_dev, (int64_t)64 * h8 * w8, 0, 0), (hipStream_t)stream);
}
