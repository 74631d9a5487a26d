"""RAFT's convolution path one kernel at a time (csrc/raft_kernels.hip, the packing and GEMM launches of csrc/raft_model.hip), through the
development library's cwm_dev_raft_* entry points (include/cwm_hip_dev.h), against float64 torch on the CPU built from the same fp32 inputs.

  a. the im2col operand (layout of csrc/common.h a_pos), per source kind  -- the only part tied to an explicit im2col
  b. one convolution per layer family of the model: exact on small integers, numeric on random data, column slices of wider buffers
  c. instance-norm statistics
  d. the pointwise kernels between the convolutions

Nothing of the library appears on a reference side.  Every bound is derived where it is used; none was fitted to a measured error."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from counterfactualworldmodels_amd import _lib
from gpu_utils import NAN_BF16, bits, decode, new_operand  # the operand layout's test helpers
from test_kernels_gpu import TOL  # the project's GEMM bounds (max-abs on O(1) outputs)

pytestmark = pytest.mark.gpu

MODES = {"parity": (_lib.MODE_PARITY, 2), "fast": (_lib.MODE_FAST, 1)}
SENTINEL = 0x7FA5A5A5   # a NaN payload no kernel produces: what the output buffers are pre-filled with
EPS = 1e-5              # the model's instance-norm / batch-norm epsilon
H0, W0, N_IMG = 9, 11, 2  # odd sides, 198 rows (no multiple of any tile), a second image


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.get_dev_lib()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def grid_xy(n_img, H, W):
    """[n_img, H, W, 2] = (x, y) of every pixel"""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys], -1).unsqueeze(0).expand(n_img, H, W, 2).contiguous()


class Src:
    """One convolution source: `x` fp32 [n_img, H, W, ld] on the CPU (channels off .. off + C are read), optional stats [n_img, C, 2], ReLU,
    gate (buffer [n_img, H, W, gate_ld], channels gate_off ..), or a coordinate field [n_img, H, W, 2].  `poison`: the device copy of x is all NaN."""

    def __init__(self, x=None, C=None, off=0, stats=None, relu=False, gate=None, gate_off=0, coords=None, poison=False):
        self.coords, self.stats, self.relu, self.gate, self.gate_off, self.off = coords, stats, relu, gate, gate_off, off
        if coords is not None:
            self.C, self.x = 2, None
            self.coords_d = coords.cuda()
            return
        self.x, self.C = x, (C if C is not None else x.shape[-1])
        self.x_d = torch.full_like(x, float("nan")).cuda() if poison else x.cuda()
        self.stats_d = None if stats is None else stats.cuda()
        self.gate_d = None if gate is None else gate.cuda()

    def fill(self, d):
        if self.coords is not None:
            d.C, d.coords = 2, self.coords_d.data_ptr()
            return
        d.p, d.ld, d.C = self.x_d.data_ptr() + 4 * self.off, self.x.shape[-1], self.C
        d.relu = int(self.relu)
        if self.stats is not None:
            d.stats = self.stats_d.data_ptr()
        if self.gate is not None:
            d.gate, d.gate_ld = self.gate_d.data_ptr() + 4 * self.gate_off, self.gate.shape[-1]

    def value(self):
        """what a consumer reads, float64 [n_img, H, W, C]"""
        if self.coords is not None:
            n, H, W, _ = self.coords.shape
            return self.coords.double() - grid_xy(n, H, W).double()
        v = self.x[..., self.off:self.off + self.C].double()
        if self.stats is not None:
            st = self.stats.double()
            v = (v - st[:, None, None, :, 0]) * st[:, None, None, :, 1]
        if self.relu:
            v = v.clamp(min=0)
        if self.gate is not None:
            v = v * torch.sigmoid(self.gate[..., self.gate_off:self.gate_off + self.C].double())
        return v


class Frames:
    """The encoders' input: x [B, T, 3, H, W]; image1 = x[:, :-1], image2 = x[:, 1:] (non-contiguous views), P = B * (T - 1) pairs, T - 1 per group."""

    def __init__(self, x, scale):
        self.x, self.scale = x, scale
        self.x_d = x.cuda()
        B, T = x.shape[:2]
        self.P, self.ppg = B * (T - 1), T - 1

    def fill(self, a, img0):
        x = self.x
        for f in range(2):
            a.image[f] = self.x_d.data_ptr() + 4 * f * x.stride(1)
            a.image_sb[f], a.image_st[f], a.image_sc[f] = x.stride(0), x.stride(1), x.stride(2)
        a.P, a.ppg, a.scale, a.img0 = self.P, self.ppg, self.scale, img0

    def value(self, img0, n_img):
        """float64 [n_img, H, W, 3]: images img0 .. of [image1 pairs | image2 pairs], scaled as the model sees them"""
        x = self.x.double()
        B, T = x.shape[:2]
        imgs = torch.cat([x[:, :-1].reshape(B * (T - 1), *x.shape[2:]), x[:, 1:].reshape(B * (T - 1), *x.shape[2:])])
        v = 2.0 * (imgs[img0:img0 + n_img] * float(self.scale) / 255.0) - 1.0
        return v.permute(0, 2, 3, 1)


def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad[0] - k[0]) // stride + 1, (W + 2 * pad[1] - k[1]) // stride + 1


def conv_call(dev, mode, n_img, H, W, k, stride, pad, srcs=None, frames=None, img0=0, parts=None, bn=None, out=None, ldc=0, col0=0, A=None, flags=0,
              c_lo=0, c_hi=0):
    """parts: [(w [n, cin, kh, kw], b [n]) ...] device tensors; bn: per part None or (gamma, beta, mean, var) device tensors"""
    a = _lib.new_dev_raft_conv_args()
    if frames is not None:
        frames.fill(a, img0)
    else:
        a.nsrc = len(srcs)
        for i, s in enumerate(srcs):
            s.fill(a.src[i])
    a.n_img, a.H, a.W, a.kh, a.kw, a.stride, a.pad_h, a.pad_w = n_img, H, W, k[0], k[1], stride, pad[0], pad[1]
    for i, (w, b) in enumerate(parts or []):
        p = a.part[i]
        p.w, p.b, p.n = w.data_ptr(), b.data_ptr(), w.shape[0]
        if bn and bn[i] is not None:
            p.bn_gamma, p.bn_beta, p.bn_mean, p.bn_var = (t.data_ptr() for t in bn[i])
    a.nparts, a.bn_eps = len(parts or []), EPS
    if out is not None:
        a.out, a.ldc, a.col0 = out.data_ptr(), ldc, col0
    a.mode, a.c_lo, a.c_hi, a.flags = MODES[mode][0], c_lo, c_hi, flags
    if A is not None:
        a.A = A.data_ptr()
    a.stream = None
    _lib.check(dev.cwm_dev_raft_conv(ctypes.byref(a)), dev)


# ---- a. the operand ----------------------------------------------------------------------------------------------------------------------------
def unfold_rows(v, k, stride, pad):
    """float64 [n, H, W, C] -> the im2col rows [n * OH * OW, kh * kw * C] in K order (ky, kx, c), zero padded at the borders"""
    n, H, W, C = v.shape
    u = F.unfold(v.permute(0, 3, 1, 2), k, padding=pad, stride=stride)  # [n, C * kh * kw, L], channel-major
    L = u.shape[-1]
    return u.view(n, C, k[0] * k[1], L).permute(0, 3, 2, 1).reshape(n * L, k[0] * k[1] * C)


def check_operand(name, A, ref, mode, arithmetic):
    """ref float64 [M, K].  No NaN anywhere; the K .. Kpad tail exactly 0; then
    fast, no arithmetic in the source: bitwise ref rounded once to bf16;
    parity: |hi + lo - ref| <= 2^-16 |ref| (hi is within 2^-9 |v| of v, lo within 2^-9 of the rest);
    sources with arithmetic (stats, gate, frame scaling, fractional coordinates): + 1e-6 max|ref| for the few fp32 roundings of the transform, and in
    fast mode one bf16 ulp, 2^-8 |ref|, in place of bitwise."""
    planes = MODES[mode][1]
    M, K = ref.shape
    Kpad = A.shape[1] // planes
    assert Kpad == (K + 63) // 64 * 64 and A.shape[0] == M
    hi, lo = decode(A, planes, Kpad)
    for p in (hi, lo):
        if p is not None:
            assert not torch.isnan(p.float()).any(), (name, mode, "rows left unwritten")
            assert (bits(p[:, K:]) == 0).all(), (name, mode, "K tail")
    got = hi[:, :K].double() + (lo[:, :K].double() if lo is not None else 0.0)
    err = (got - ref).abs()
    if mode == "fast" and not arithmetic:
        assert torch.equal(bits(hi[:, :K]), bits(ref.float().to(torch.bfloat16))), (name, mode, err.max().item())
        print(f"[operand {name} {mode}] bitwise")
        return got
    rel = 2.0 ** -16 if mode == "parity" else 2.0 ** -8
    bound = rel * ref.abs() + (1e-6 * ref.abs().max().item() if arithmetic else 0.0)
    worst = (err / bound.clamp(min=1e-300)).max().item() if (bound > 0).any() else 0.0
    print(f"[operand {name} {mode}] max-abs {err.max().item():.3e}, worst error / bound {worst:.3f}")
    assert (err <= bound).all(), (name, mode, err.max().item())
    return got


def rand_stats(n_img, C, seed):
    """(mean, rstd) pairs that differ per image"""
    g = gen(seed)
    return torch.stack([0.5 * torch.randn(n_img, C, generator=g), 0.5 + torch.rand(n_img, C, generator=g)], -1).contiguous()


def run_operand(dev, name, mode, srcs, H, W, k, stride, pad, arithmetic, n_img=N_IMG):
    planes = MODES[mode][1]
    oh, ow = out_hw(H, W, k, stride, pad)
    ref = unfold_rows(torch.cat([s.value() for s in srcs], -1), k, stride, pad)
    assert ref.shape[0] == n_img * oh * ow
    A = new_operand(ref.shape[0], (ref.shape[1] + 63) // 64 * 64, planes)
    conv_call(dev, mode, n_img, H, W, k, stride, pad, srcs=srcs, A=A, flags=_lib.DEV_CONV_OPERAND_ONLY)
    check_operand(name, A, ref, mode, arithmetic)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("scale,img0,n_img", [(255.0, 0, 8), (255.0, 3, 4), (1.0, 0, 8), (1.0, 3, 4)])
def test_operand_frames(dev, mode, scale, img0, n_img):
    """7x7 / 2 / 3 over [B = 2, T = 3, 3, 24, 40] frames read through the image1 / image2 views: all 8 images, and 4 from image 3 on (which straddles
    the image1 / image2 boundary and a group boundary).  K = 147, Kpad = 192."""
    x = torch.rand(2, 3, 3, 24, 40, generator=gen(11)) * (255.0 / scale)
    fr = Frames(x, scale)
    k, stride, pad = (7, 7), 2, (3, 3)
    ref = unfold_rows(fr.value(img0, n_img), k, stride, pad)
    assert ref.shape == (n_img * 12 * 20, 147)
    A = new_operand(ref.shape[0], 192, MODES[mode][1])
    conv_call(dev, mode, n_img, 24, 40, k, stride, pad, frames=fr, img0=img0, A=A, flags=_lib.DEV_CONV_OPERAND_ONLY)
    check_operand(f"frames scale {scale:g} img0 {img0}", A, ref, mode, arithmetic=True)


@pytest.mark.parametrize("mode", list(MODES))
def test_operand_plain_and_instance_norm(dev, mode):
    """C = 64, 3x3 / 1 / 1: as stored, ReLU'd, and instance-normalised + ReLU'd with statistics that differ per image"""
    x = torch.randn(N_IMG, H0, W0, 64, generator=gen(12))
    run_operand(dev, "plain", mode, [Src(x)], H0, W0, (3, 3), 1, (1, 1), arithmetic=False)
    run_operand(dev, "relu", mode, [Src(x, relu=True)], H0, W0, (3, 3), 1, (1, 1), arithmetic=False)
    run_operand(dev, "stats+relu", mode, [Src(2 * x + 1, stats=rand_stats(N_IMG, 64, 13), relu=True)], H0, W0, (3, 3), 1, (1, 1), arithmetic=True)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("H,W,k,pad", [(9, 11, (3, 3), (1, 1)), (10, 12, (3, 3), (1, 1)), (9, 11, (1, 1), (0, 0))])
def test_operand_stride_2_output_size(dev, mode, H, W, k, pad):
    x = torch.randn(N_IMG, H, W, 64, generator=gen(14))
    assert out_hw(H, W, k, 2, pad) == (5, 6)
    run_operand(dev, f"stride 2 {H}x{W} k{k[0]}", mode, [Src(x)], H, W, k, 2, pad, arithmetic=False)


@pytest.mark.parametrize("mode", list(MODES))
def test_operand_coordinates(dev, mode):
    """7x7 / 1 / 3 over the flow coords - (x, y): K = 98, Kpad = 128"""
    g = gen(15)
    base = grid_xy(N_IMG, H0, W0)
    whole = base + torch.randint(-4, 5, base.shape, generator=g).float()
    run_operand(dev, "coords integer", mode, [Src(coords=whole)], H0, W0, (7, 7), 1, (3, 3), arithmetic=False)
    frac = base + 3.0 * torch.randn(base.shape, generator=g)
    run_operand(dev, "coords fractional", mode, [Src(coords=frac)], H0, W0, (7, 7), 1, (3, 3), arithmetic=True)


@pytest.mark.parametrize("mode", list(MODES))
def test_operand_channel_slice_of_a_wider_buffer(dev, mode):
    x = torch.randn(N_IMG, H0, W0, 256, generator=gen(16))
    run_operand(dev, "ld 256 C 192", mode, [Src(x, C=192)], H0, W0, (3, 3), 1, (1, 1), arithmetic=False)
    run_operand(dev, "ld 256 C 192 from 64", mode, [Src(x, C=192, off=64)], H0, W0, (3, 3), 1, (1, 1), arithmetic=False)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("k,pad", [((1, 5), (0, 2)), ((5, 1), (2, 0))])
def test_operand_gru_rows_and_partial_rewrite(dev, mode, k, pad):
    """[h (128) | x (256)] rows, Kpad 1920: a full write, then -- as the GRU's q convolution does -- a rewrite of the h channels only, gated by
    sigmoid(r), with the x source pointing at NaNs: the h channels of every tap become h * sigmoid(r), everything else keeps the first call's bits."""
    planes = MODES[mode][1]
    g = gen(17)
    h = torch.randn(N_IMG, H0, W0, 128, generator=g)
    x = torch.randn(N_IMG, H0, W0, 256, generator=g)
    zr = torch.randn(N_IMG, H0, W0, 256, generator=g)
    M = N_IMG * H0 * W0
    A = new_operand(M, 1920, planes)
    full = unfold_rows(torch.cat([Src(h).value(), Src(x).value()], -1), k, 1, pad)
    conv_call(dev, mode, N_IMG, H0, W0, k, 1, pad, srcs=[Src(h), Src(x)], A=A, flags=_lib.DEV_CONV_OPERAND_ONLY)
    check_operand("gru full", A, full, mode, arithmetic=False)
    first = A.clone()
    gated = Src(h, gate=zr, gate_off=128)
    conv_call(dev, mode, N_IMG, H0, W0, k, 1, pad, srcs=[gated, Src(x, poison=True)], A=A, flags=_lib.DEV_CONV_OPERAND_ONLY, c_lo=0, c_hi=128)
    want = unfold_rows(torch.cat([gated.value(), Src(x).value()], -1), k, 1, pad)
    is_h = (torch.arange(1920) % 384) < 128
    got = check_operand("gru gated rewrite", A, want, mode, arithmetic=True)
    assert got.shape == want.shape
    for pa, pb in zip(decode(A, planes, 1920), decode(first, planes, 1920)):
        if pa is not None:
            assert torch.equal(bits(pa[:, ~is_h]), bits(pb[:, ~is_h])), (mode, "x channels changed")
    assert (got[:, is_h] != full[:, is_h]).any()  # the h channels did change: gated where the first call had them plain


@pytest.mark.parametrize("mode", list(MODES))
def test_operand_partial_rewrite_keeps_everything_else(dev, mode):
    """The partial rewrite's contract (kernels.h Im2colParams): only input channels [c_lo, c_hi) of every tap are written; the other channels AND the K
    padding are kept.  Sources of 24 + 16 channels, 3x3: K = 360, Kpad = 384; channels [8, 32) straddle the two sources.  The buffer starts as NaN
    patterns, so every element outside the range must still hold that pattern -- the 24 elements of the K tail included."""
    planes = MODES[mode][1]
    g = gen(18)
    a, b = torch.randn(N_IMG, H0, W0, 24, generator=g), torch.randn(N_IMG, H0, W0, 16, generator=g)
    k, pad = (3, 3), (1, 1)
    ref = unfold_rows(torch.cat([a, b], -1).double(), k, 1, pad)
    A = new_operand(ref.shape[0], 384, planes)
    conv_call(dev, mode, N_IMG, H0, W0, k, 1, pad, srcs=[Src(a), Src(b)], A=A, flags=_lib.DEV_CONV_OPERAND_ONLY, c_lo=8, c_hi=32)
    kk = torch.arange(384)
    inside = (kk < 360) & (kk % 40 >= 8) & (kk % 40 < 32)
    hi, lo = decode(A, planes, 384)
    for p in (hi, lo):
        if p is not None:
            assert (bits(p[:, ~inside]).int() == NAN_BF16).all(), (mode, "written outside [c_lo, c_hi)")
            assert not torch.isnan(p[:, inside].float()).any()
    got = hi[:, inside].double() + (lo[:, inside].double() if lo is not None else 0.0)
    want = ref[:, inside[:360]]
    if mode == "fast":
        assert torch.equal(bits(hi[:, inside]), bits(want.float().to(torch.bfloat16)))
    else:
        assert ((got - want).abs() <= 2.0 ** -16 * want.abs()).all()


def lookup_inputs():
    """the inputs of tests/test_raft_gpu.py::test_corr_lookup_kernel_vs_restatement"""
    g = gen(3)
    P, h, w = 2, 20, 17
    f1 = torch.randn(P, h, w, 256, generator=g).cuda()
    f2 = torch.randn(P, h, w, 256, generator=g).cuda()
    base = torch.stack(torch.meshgrid(torch.arange(w, dtype=torch.float32), torch.arange(h, dtype=torch.float32), indexing="xy"), -1)
    coords = (base.unsqueeze(0) + 9.0 * (torch.rand(P, h, w, 2, generator=g) - 0.5)).cuda()
    coords[0, 0, 0] = torch.tensor([-30.0, 50.0])
    return P, h, w, f1, f2, coords


@pytest.mark.parametrize("mode", list(MODES))
def test_lookup_operand_equals_the_fp32_lookup(dev, mode):
    """The operand-writing form of the correlation lookup (what convc1 reads on every iteration) holds the fp32 form's values (which
    test_corr_lookup_kernel_vs_restatement checks against torch): fast bitwise after one bf16 rounding, parity within 2^-16 |v|; features 324 .. 383 are 0."""
    planes = MODES[mode][1]
    P, h, w, f1, f2, coords = lookup_inputs()
    M = P * h * w
    out = torch.empty(M, 324, device="cuda")
    _lib.check(dev.cwm_raft_corr_lookup(f1.data_ptr(), f2.data_ptr(), coords.data_ptr(), P, h, w, out.data_ptr(), None), dev)
    A = new_operand(M, 384, planes)
    _lib.check(dev.cwm_dev_raft_corr_lookup_operand(f1.data_ptr(), f2.data_ptr(), coords.data_ptr(), P, h, w, MODES[mode][0], A.data_ptr(), None), dev)
    ref = out.cpu().double()
    assert (ref == 0).any() and ref.abs().max() > 1
    check_operand("lookup", A, ref, mode, arithmetic=False)


@pytest.mark.parametrize("mode", list(MODES))
def test_convc1_runs_on_the_lookup_operand_as_it_is(dev, mode):
    """convc1 (324 -> 256, 1x1) has no im2col of its own: the GEMM reads the operand the lookup wrote.  Against the float64 product of the fp32 lookup
    with the weights, within the GEMM's bound (the `src` only tells the channel count; it is not read)."""
    planes = MODES[mode][1]
    P, h, w, f1, f2, coords = lookup_inputs()
    M = P * h * w
    feat = torch.empty(M, 324, device="cuda")
    _lib.check(dev.cwm_raft_corr_lookup(f1.data_ptr(), f2.data_ptr(), coords.data_ptr(), P, h, w, feat.data_ptr(), None), dev)
    A = new_operand(M, 384, planes)
    _lib.check(dev.cwm_dev_raft_corr_lookup_operand(f1.data_ptr(), f2.data_ptr(), coords.data_ptr(), P, h, w, MODES[mode][0], A.data_ptr(), None), dev)
    g = gen(19)
    wt, b = torch.randn(256, 324, 1, 1, generator=g) * 324 ** -0.5, torch.randn(256, generator=g)
    x = feat.cpu()
    ref = F.linear(x.double(), wt.view(256, 324).double(), b.double())
    out = torch.full((M, 256), SENTINEL, dtype=torch.int32, device="cuda")
    conv_call(dev, mode, P, h, w, (1, 1), 1, (0, 0), srcs=[Src(x.view(P, h, w, 324))], parts=[(wt.cuda(), b.cuda())], out=out, ldc=256, A=A,
              flags=_lib.DEV_CONV_KEEP_OPERAND)
    err = (out.cpu().view(torch.float32).double() - ref).abs().max().item()
    bound = TOL[mode] * max(1.0, ref.abs().max().item() / 4)
    print(f"[convc1 on the lookup operand {mode}] max-abs {err:.3e} (bound {bound:.3e}, max|ref| {ref.abs().max().item():.2f})")
    assert err <= bound


# ---- b. one convolution per layer family -------------------------------------------------------------------------------------------------------
# cin: channels per source; n: output channels per weight part; src: "frames", "coords" or per-source flags
FAMILIES = {
    "conv1_7x7s2_frames_bn": dict(src="frames", n=[64], k=(7, 7), stride=2, pad=(3, 3), bn=True, ldc=64),
    "block_3x3": dict(cin=[64], n=[64], k=(3, 3), pad=(1, 1), stats=True, relu=True, ldc=64),
    "block_3x3s2": dict(cin=[64], n=[96], k=(3, 3), stride=2, pad=(1, 1), stats=True, relu=True, ldc=96),
    "downsample_1x1s2_bn": dict(cin=[64], n=[96], k=(1, 1), stride=2, pad=(0, 0), bn=True, ldc=96),
    "encoder_out_1x1": dict(cin=[128], n=[256], k=(1, 1), pad=(0, 0), ldc=256),
    "convf1_7x7_coords": dict(src="coords", n=[128], k=(7, 7), pad=(3, 3), ldc=128),
    "convc2_cols_0_192_of_256": dict(cin=[256], n=[192], k=(3, 3), pad=(1, 1), relu=True, ldc=256),
    "convf2_cols_192_256_of_256": dict(cin=[128], n=[64], k=(3, 3), pad=(1, 1), relu=True, ldc=256, col0=192),
    "conv_126_cols_128_of_256": dict(cin=[256], n=[126], k=(3, 3), pad=(1, 1), relu=True, ldc=256, col0=128),
    "gru_zr_1x5_two_parts": dict(cin=[128, 256], n=[128, 128], k=(1, 5), pad=(0, 2), ldc=256),
    "gru_q_5x1_gated": dict(cin=[128, 256], n=[128], k=(5, 1), pad=(2, 0), gate=True, ldc=128),
    "flow_head_2_of_16": dict(cin=[256], n=[2], k=(3, 3), pad=(1, 1), relu=True, ldc=16),
    "mask2_1x1_576": dict(cin=[256], n=[576], k=(1, 1), pad=(0, 0), relu=True, ldc=576),
}


class ConvCase:
    """Inputs of one family (exact: small integers, no stats / gate / batch norm; else random) and the float64 convolution of them"""

    def __init__(self, name, exact, n_img=N_IMG, seed=100):
        f = FAMILIES[name]
        self.f, self.name, self.n_img = f, name, n_img
        g = gen(seed + sorted(FAMILIES).index(name))
        self.k, self.stride, self.pad = f["k"], f.get("stride", 1), f["pad"]
        self.frames, self.srcs, self.img0 = None, None, 0
        ints = lambda *shape: torch.randint(-4, 5, shape, generator=g).float()  # noqa: E731
        if f.get("src") == "frames":
            # x in steps of 0.5 so that 2 * (x * 255 / 255) - 1 is an integer in [-4, 4]; else frames in [0, 1)
            self.H, self.W, self.img0 = 2 * H0, 2 * W0, 3
            assert n_img == 2
            self.n_img = n_img = 4
            x = (ints(2, 3, 3, self.H, self.W) + 1) / 2 if exact else torch.rand(2, 3, 3, self.H, self.W, generator=g)
            self.frames = Frames(x, 255.0)
            v = self.frames.value(self.img0, n_img)
        elif f.get("src") == "coords":
            self.H, self.W = H0, W0
            base = grid_xy(n_img, H0, W0)
            self.srcs = [Src(coords=base + (ints(*base.shape) if exact else 2.0 * torch.randn(base.shape, generator=g)))]
            v = self.srcs[0].value()
        else:
            self.H, self.W = H0, W0
            self.srcs = []
            for i, c in enumerate(f["cin"]):
                x = ints(n_img, H0, W0, c) if exact else torch.randn(n_img, H0, W0, c, generator=g)
                kw = dict(relu=f.get("relu", False))
                if not exact and f.get("stats"):
                    x, kw["stats"] = 2 * x + 1, rand_stats(n_img, c, seed + 50)
                if not exact and f.get("gate") and i == 0:
                    kw["gate"], kw["gate_off"] = torch.randn(n_img, H0, W0, 256, generator=g), 128
                self.srcs.append(Src(x, **kw))
            v = torch.cat([s.value() for s in self.srcs], -1)
        cin = v.shape[-1]
        K = self.k[0] * self.k[1] * cin
        self.parts, self.bn, ws, bs = [], [], [], []
        for n in f["n"]:
            w = ints(n, cin, *self.k) if exact else torch.randn(n, cin, *self.k, generator=g) * K ** -0.5
            b = ints(n) if exact else torch.randn(n, generator=g)
            w64, b64 = w.double(), b.double()
            if f.get("bn") and not exact:
                gamma, beta = 0.5 + torch.rand(n, generator=g), 0.5 * torch.randn(n, generator=g)
                mean, var = 0.5 * torch.randn(n, generator=g), 0.5 + torch.rand(n, generator=g)
                s = gamma.double() / torch.sqrt(var.double() + float(torch.tensor(EPS, dtype=torch.float32)))
                w64, b64 = w64 * s.view(n, 1, 1, 1), (b64 - mean.double()) * s + beta.double()
                self.bn.append(tuple(t.cuda() for t in (gamma, beta, mean, var)))
            else:
                self.bn.append(None)
            self.parts.append((w.cuda(), b.cuda()))
            ws.append(w64)
            bs.append(b64)
        y = F.conv2d(v.permute(0, 3, 1, 2), torch.cat(ws), torch.cat(bs), stride=self.stride, padding=self.pad)
        self.n = y.shape[1]
        self.n16 = (self.n + 15) // 16 * 16
        self.ref = y.permute(0, 2, 3, 1).reshape(-1, self.n)
        self.ldc, self.col0 = f["ldc"], f.get("col0", 0)
        assert self.ref.shape[0] == self.n_img * (H0 * W0 if self.stride == 1 or self.frames else 5 * 6)

    def new_out(self):
        return torch.full((self.ref.shape[0], self.ldc), SENTINEL, dtype=torch.int32, device="cuda")

    def run(self, dev, mode, out=None):
        out = self.new_out() if out is None else out
        conv_call(dev, mode, self.n_img, self.H, self.W, self.k, self.stride, self.pad, srcs=self.srcs, frames=self.frames, img0=self.img0, parts=self.parts,
                  bn=self.bn, out=out, ldc=self.ldc, col0=self.col0)
        return out

    def check_slice(self, out, before=None):
        """columns outside [col0, col0 + round_up(n, 16)) bitwise untouched, columns n .. round_up(n, 16) exactly 0.0; -> the n result columns"""
        o = out.cpu()
        keep = torch.ones(self.ldc, dtype=torch.bool)
        keep[self.col0:self.col0 + self.n16] = False
        want = torch.full_like(o, SENTINEL) if before is None else before.cpu()
        assert torch.equal(o[:, keep], want[:, keep]), (self.name, "columns outside the slice were written")
        assert (o[:, self.col0 + self.n:self.col0 + self.n16] == 0).all(), (self.name, "padding columns")
        return o[:, self.col0:self.col0 + self.n].contiguous().view(torch.float32)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(FAMILIES))
def test_conv_is_exact_on_small_integers(dev, mode, name):
    """Inputs, weights and biases are integers in [-4, 4] (exact in bf16; every partial sum below 2^24, exact in fp32 in any order): the output is the
    float64 convolution bit for bit in both modes.  A dropped or misplaced tap cannot hide in a rounding bound here.  (The batch-norm fold is not
    exact arithmetic and is left to the numeric test.)"""
    c = ConvCase(name, exact=True)
    got = c.check_slice(c.run(dev, mode))
    assert not torch.isnan(got).any()
    assert torch.equal(got.double(), c.ref), (name, mode, (got.double() - c.ref).abs().max().item())


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(FAMILIES))
def test_conv_matches_float64_on_random_data(dev, mode, name):
    """Random normal inputs, weights scaled K^-0.5, with the family's statistics / gate / batch-norm fold: within the GEMM's own bound,
    TOL[mode] * max(1, max|ref| / 4) as tests/test_kernels_gpu.py::test_linear_matches_torch holds the GEMM to."""
    c = ConvCase(name, exact=False)
    got = c.check_slice(c.run(dev, mode))
    err = (got.double() - c.ref).abs().max().item()
    bound = TOL[mode] * max(1.0, c.ref.abs().max().item() / 4)
    print(f"[conv {name} {mode}] max-abs {err:.3e} (bound {bound:.3e}, max|ref| {c.ref.abs().max().item():.2f})")
    assert err <= bound, (name, mode, err)


@pytest.mark.parametrize("mode", list(MODES))
def test_two_convolutions_share_one_buffer_by_columns(dev, mode):
    """convc2 writes columns 0 .. 191 and convf2 columns 192 .. 255 of one [M][256] buffer (the motion encoder's `cf`): neither touches the other's"""
    a, b = ConvCase("convc2_cols_0_192_of_256", exact=False), ConvCase("convf2_cols_192_256_of_256", exact=False)
    out = a.run(dev, mode)
    ya = a.check_slice(out)
    after_a = out.clone()
    b.run(dev, mode, out=out)
    yb = b.check_slice(out, before=after_a)
    assert torch.equal(out[:, :192].cpu().view(torch.float32), ya)
    for c, y in ((a, ya), (b, yb)):
        assert (y.double() - c.ref).abs().max().item() <= TOL[mode] * max(1.0, c.ref.abs().max().item() / 4)


def run_tiles(dev, c, mode, tiles=(1, 4, 6), debug=0):
    outs = []
    try:
        _lib.check(dev.cwm_debug_set(b"gemm_debug", debug), dev)
        for tile in tiles:
            _lib.check(dev.cwm_debug_set(b"gemm_tile", tile), dev)
            outs.append(c.check_slice(c.run(dev, mode)))  # (the sentinels around the slice are checked under every configuration)
    finally:
        _lib.check(dev.cwm_debug_set(b"gemm_tile", 0), dev)
        _lib.check(dev.cwm_debug_set(b"gemm_debug", 0), dev)
    return outs


@pytest.mark.parametrize("mode", list(MODES))
def test_slice_output_is_the_same_under_every_gemm_tile(dev, mode):
    """128 -> 64 into columns 192 .. 255 of 256 under tile configurations 1, 4 and 6: the same bits, the other columns left alone.  n_img = 56, M = 5544
    rows: the tile configurations apply one product sequence to every accumulator, EXCEPT that a small launch on 128x128 tiles may split K over idle
    CUs (gemm.hip gemm_splitk_parts: min(CUs / tiles, K tiles / 12) >= 3 parts), which re-associates the fp32 sum.  87 row tiles of 64 on 256 CUs leave
    fewer than 3 parts per tile, so no configuration splits here; the next test takes the M = 594 launch that does."""
    c = ConvCase("convf2_cols_192_256_of_256", exact=False, n_img=56)
    assert c.ref.shape[0] >= 512
    outs = run_tiles(dev, c, mode)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert (outs[0].double() - c.ref).abs().max().item() <= TOL[mode] * max(1.0, c.ref.abs().max().item() / 4)


@pytest.mark.parametrize("mode", list(MODES))
def test_slice_output_of_a_split_k_launch(dev, mode):
    """The same slice with M = 6 * 99 = 594 rows: 10 row tiles of 64 and, in parity mode, 36 K tiles -> 3 K parts on the 128x128 configuration.  Without
    the split ("gemm_debug" 32, as the bitwise cross-checks of tests/test_kernels_gpu.py run) the three configurations give the same bits; with it
    the 128x128 result is deterministic, within 2e-5 of them (the re-association of an fp32 sum of O(1) terms; the figure
    test_gemm_deep_ring_and_split_k_small_launches holds the GEMM to), and the sentinels stay intact."""
    c = ConvCase("convf2_cols_192_256_of_256", exact=False, n_img=6)
    assert c.ref.shape[0] >= 512
    outs = run_tiles(dev, c, mode, debug=32)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    split = run_tiles(dev, c, mode, tiles=(1, 1, 4, 6))
    assert torch.equal(split[0], split[1])
    assert torch.equal(split[2], outs[0])   # 256x256 tiles never split K
    assert torch.equal(split[3], split[0])  # no whole round of 256x256 tiles in 594 rows: configuration 6 is all remainder, 128x128 tiles
    d = (split[0] - outs[0]).abs().max().item()
    print(f"[split-K slice {mode}] max-abs vs unsplit {d:.3e}")
    assert d <= (2e-5 if mode == "parity" else 0.0)
    assert (split[0].double() - c.ref).abs().max().item() <= TOL[mode] * max(1.0, c.ref.abs().max().item() / 4)


# ---- c. instance-norm statistics ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 96, 128])
@pytest.mark.parametrize("HW", [323, 5168, 16500])
def test_instnorm_stats(dev, HW, C):
    """HW: one chunk, six ragged chunks, the 16-chunk cap; C = 96 leaves half a channel group idle.  Random channels, channels with mean 100 and std 0.01
    (E[x^2] - mean^2 cancels four digits), one constant channel.  The kernel accumulates in double, so against the float64 two-pass statistics only
    the fp32 cast of the mean (2^-24 |mean|; held to 2^-23) and, for rstd, the conditioning of E[x^2] - mean^2 remain (1e-6 relative)."""
    n_img = 3
    g = gen(1000 + HW + C)
    x = torch.randn(n_img, HW, C, generator=g) * (0.5 + torch.rand(n_img, 1, C, generator=g)) + torch.randn(n_img, 1, C, generator=g)
    x[:, :, 5:9] = 100.0 + 0.01 * torch.randn(n_img, HW, 4, generator=g)
    x[:, :, C - 1] = 1.5
    xd = x.cuda()
    stats = torch.full((n_img, C, 2), float("nan"), device="cuda")
    _lib.check(dev.cwm_dev_raft_instnorm_stats(xd.data_ptr(), n_img, HW, C, EPS, stats.data_ptr(), None), dev)
    got = stats.cpu().double()
    x64 = x.double()
    mean = x64.mean(1)
    var = ((x64 - mean[:, None]) ** 2).mean(1)
    eps64 = float(torch.tensor(EPS, dtype=torch.float32))
    rstd = 1.0 / torch.sqrt(var + eps64)
    e_mean = ((got[..., 0] - mean).abs() / mean.abs()).max().item()
    e_rstd = ((got[..., 1] - rstd).abs() / rstd).max().item()
    print(f"[instnorm HW {HW} C {C}] mean rel {e_mean:.3e} (bound {2.0 ** -23:.3e}), rstd rel {e_rstd:.3e} (bound 1e-6)")
    assert ((got[..., 0] - mean).abs() <= 2.0 ** -23 * mean.abs()).all()
    assert ((got[..., 1] - rstd).abs() <= 1e-6 * rstd).all()
    const = torch.tensor(1.0 / eps64 ** 0.5, dtype=torch.float64).float()
    ulp = torch.nextafter(const, torch.tensor(float("inf"))) - const
    assert ((stats[:, C - 1, 1].cpu() - const).abs() <= ulp).all()


# ---- d. the pointwise kernels ------------------------------------------------------------------------------------------------------------------
M_ROWS = N_IMG * H0 * W0


def close_f32(got, ref):
    """4 * 2^-23 * max(1, |ref|): a few fp32 roundings plus expf / tanhf at <= 2 ulp"""
    err = (got.double() - ref).abs()
    bound = 4 * 2.0 ** -23 * ref.abs().clamp(min=1.0)
    return (err <= bound).all().item(), (err / bound).max().item()


def sentinel_f32(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32).view(torch.float32)


def test_residual_join_in_place(dev):
    """relu(norm(X) + relu(norm(Y))) with per-image statistics on both, written over X as the encoder does"""
    C = 96
    g = gen(21)
    X, Y = Src(2 * torch.randn(N_IMG, H0, W0, C, generator=g) + 1, stats=rand_stats(N_IMG, C, 22)), \
        Src(2 * torch.randn(N_IMG, H0, W0, C, generator=g) - 1, stats=rand_stats(N_IMG, C, 23), relu=True)
    ref = (X.value() + Y.value()).clamp(min=0).reshape(M_ROWS, C)
    dx, dy = _lib.CwmDevConvSrc(), _lib.CwmDevConvSrc()
    X.fill(dx)
    Y.fill(dy)
    _lib.check(dev.cwm_dev_raft_residual_join(ctypes.byref(dx), ctypes.byref(dy), N_IMG, H0 * W0, X.x_d.data_ptr(), None), dev)
    ok, worst = close_f32(X.x_d.cpu().reshape(M_ROWS, C), ref)
    print(f"[residual join] worst error / bound {worst:.3f}")
    assert ok and (ref == 0).any() and (ref > 0).any()
    assert torch.equal(Y.x_d.cpu(), Y.x)


def test_cnet_split(dev):
    cn = 1.5 * torch.randn(M_ROWS, 256, generator=gen(24))
    h, x, cnd = sentinel_f32(M_ROWS, 128).cuda(), sentinel_f32(M_ROWS, 256).cuda(), cn.cuda()
    _lib.check(dev.cwm_dev_raft_cnet_split(cnd.data_ptr(), M_ROWS, h.data_ptr(), x.data_ptr(), None), dev)
    ok, worst = close_f32(h.cpu(), torch.tanh(cn[:, :128].double()))
    print(f"[cnet split] worst error / bound {worst:.3f}")
    assert ok
    x = x.cpu()
    assert torch.equal(x[:, :128], cn[:, 128:].clamp(min=0))  # selection: bitwise
    assert torch.equal(x[:, 128:].contiguous().view(torch.int32), sentinel_f32(M_ROWS, 128).view(torch.int32))


def test_motion_finish(dev):
    g = gen(25)
    x = torch.randn(M_ROWS, 256, generator=g)
    coords = (grid_xy(N_IMG, H0, W0) + 3.0 * torch.randn(N_IMG, H0, W0, 2, generator=g)).reshape(M_ROWS, 2)
    xd, cd = x.cuda(), coords.cuda()
    _lib.check(dev.cwm_dev_raft_motion_finish(xd.data_ptr(), cd.data_ptr(), M_ROWS, H0, W0, None), dev)
    got = xd.cpu()
    assert torch.equal(got[:, :128], x[:, :128])
    assert torch.equal(got[:, 128:254], x[:, 128:254].clamp(min=0))
    flow = (coords.double() - grid_xy(N_IMG, H0, W0).reshape(M_ROWS, 2).double()).float()  # one fp32 subtraction: the exact difference rounded once
    assert torch.equal(got[:, 254:], flow)


def test_gru_update(dev):
    g = gen(26)
    h, zr, q = torch.randn(M_ROWS, 128, generator=g), torch.randn(M_ROWS, 256, generator=g), torch.randn(M_ROWS, 128, generator=g)
    hd, zrd, qd = h.cuda(), zr.cuda(), q.cuda()
    _lib.check(dev.cwm_dev_raft_gru_update(hd.data_ptr(), zrd.data_ptr(), qd.data_ptr(), M_ROWS, None), dev)
    z = torch.sigmoid(zr[:, :128].double())
    ok, worst = close_f32(hd.cpu(), (1 - z) * h.double() + z * torch.tanh(q.double()))
    print(f"[gru update] worst error / bound {worst:.3f}")
    assert ok


def test_flow_update_reads_two_columns_of_16(dev):
    g = gen(27)
    coords = grid_xy(N_IMG, H0, W0).reshape(M_ROWS, 2) + torch.randn(M_ROWS, 2, generator=g)
    delta = torch.full((M_ROWS, 16), float("nan"))
    delta[:, :2] = torch.randn(M_ROWS, 2, generator=g)
    cd, dd = coords.cuda(), delta.cuda()
    _lib.check(dev.cwm_dev_raft_flow_update(cd.data_ptr(), dd.data_ptr(), 16, M_ROWS, None), dev)
    assert torch.equal(cd.cpu(), (coords.double() + delta[:, :2].double()).float())  # one fp32 addition
