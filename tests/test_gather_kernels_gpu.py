"""The operand gathers one launch at a time (csrc/elementwise.hip patch / index / flow-RGB gather, csrc/conj_kernels.hip IMU gather), through the
development library's cwm_dev_gather (include/cwm_hip_dev.h), against torch on the CPU built from the same fp32 inputs.

Every gather writes the GEMM A operand (csrc/common.h a_pos) through the one set of writers of common.h.  The bounds are those of the project's
operand tests (test_raft_kernels_gpu.py, group a):
  sources without arithmetic (normalize = 0, IMU, pad rows, the K tail): bitwise in both modes, hi == bf16(x) and lo == bf16(x - float(hi));
  sources with arithmetic ((a - mean) / std, flow / (size / 2)): |hi + lo - ref| <= 2^-16 |ref| + 1e-6 max|ref| in parity mode,
                                                                  |hi - ref|      <= 2^-8  |ref| + 1e-6 max|ref| in fast mode;
  perm, rank, err_rows: exact.
The operand buffer is pre-filled with a NaN pattern and every element of its ld-wide rows must have been written."""
import ctypes
import functools

import pytest
import torch

from counterfactualworldmodels_amd import _lib
from gpu_utils import bits, decode, new_operand

pytestmark = pytest.mark.gpu

MODES = {"parity": (_lib.MODE_PARITY, 2), "fast": (_lib.MODE_FAST, 1)}
MEAN = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32)  # the kernels' fp32 constants
STD = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.get_dev_lib()


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- references (CPU, computed once per geometry) ------------------------------------------------------------------------------------------------
def strided_frames(B, T, C, H, W, seed):
    """x [B, T, C, H, W] fp32 as a view of a larger buffer: batch, time and channel strides all differ from the contiguous ones"""
    base = torch.randn(B, T + 1, C + 1, H, W, generator=gen(seed))
    return base, base[:, :T, :C]


def tubelets(x, P):
    """[B, T, C, H, W] -> [B, T * gh * gw, C * P * P]: token order (t, hy, wx), K order (c, ph, pw)"""
    B, T, C, H, W = x.shape
    gh, gw = H // P, W // P
    return x.reshape(B, T, C, gh, P, gw, P).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, T * gh * gw, C * P * P)


def perm_rank_of(mask):
    """mask [B, L] (0 = visible) -> perm = [visible ascending | masked ascending], rank = its inverse"""
    B, L = mask.shape
    idx = torch.arange(L)
    perm = torch.stack([torch.cat([idx[mask[b] == 0], idx[mask[b] != 0]]) for b in range(B)]).to(torch.int32)
    rank = torch.empty_like(perm)
    for b in range(B):
        rank[b, perm[b].long()] = torch.arange(L, dtype=torch.int32)
    return perm, rank


def mask_with_counts(B, L, counts, seed, allowed=None):
    """uint8 [B, L], row b with counts[b] visible (0) slots drawn from allowed[b] (default: all L)"""
    g = gen(seed)
    m = torch.ones(B, L, dtype=torch.uint8)
    for b in range(B):
        pool = torch.arange(L) if allowed is None else allowed[b]
        m[b, pool[torch.randperm(len(pool), generator=g)[:counts[b]]]] = 0
    return m


def gather_rows(tok, perm, n_rows, n_real):
    """tok [B, n_real, K] -> (rows [B * n_rows, K], pad [B * n_rows] bool): row (b, i) = token perm[b, i], zeros where that is a pad slot (>= n_real)"""
    B, _, K = tok.shape
    sel = perm[:, :n_rows].long()
    pad = sel >= n_real
    rows = torch.gather(tok, 1, sel.clamp(max=n_real - 1).unsqueeze(-1).expand(B, n_rows, K)).clone()
    rows[pad] = 0
    return rows.reshape(B * n_rows, K), pad.reshape(-1)


def normalized(tok, P):
    """imagenet normalisation of [.., 3 * P * P] tubelets in float64, from the fp32 constants"""
    c = torch.arange(3).repeat_interleave(P * P)
    return (tok.double() - MEAN.double()[c]) / STD.double()[c]


# ---- the call and the check ------------------------------------------------------------------------------------------------------------------------
def gather_call(dev, kind, mode, out, ld, B, n_rows, Nt, perm_stride=0, x=None, frames=None, C=0, P=0, normalize=0, flows=None, imu=None, tubelet=0,
                mask=None, n_vis=0, perm=None, rank=None, err_rows=None, ragged=None, check=True):
    """x: (device buffer, strided CPU view [B, T, C, H, W] of it); flows: two of the same with [B, 2, H, W] views; imu: device [B, C, L].
    ragged = (n_vis_min, counts device tensor or None): through cwm_dev_gather_ragged, n_vis being the cap.  -> the status (raised unless check=False)"""
    a = _lib.new_dev_gather_args()
    a.kind, a.mode, a.normalize = kind, MODES[mode][0], normalize
    if imu is not None:
        a.x, a.C, a.L, a.tubelet = imu.data_ptr(), imu.shape[1], imu.shape[2], tubelet
    else:
        buf, v = x
        a.x = buf.data_ptr() + 4 * v.storage_offset()
        if v.dim() == 5:
            a.sb, a.st, a.sc = v.stride(0), v.stride(1), v.stride(2)
        else:
            a.sb, a.sc = v.stride(0), v.stride(1)
        a.C, a.H, a.W, a.P = C, v.shape[-2], v.shape[-1], P
    if flows is not None:
        (fb, fv), (bb, bv) = flows
        a.fwd, a.f_sb, a.f_sc = fb.data_ptr() + 4 * fv.storage_offset(), fv.stride(0), fv.stride(1)
        a.bwd, a.b_sb, a.b_sc = bb.data_ptr() + 4 * bv.storage_offset(), bv.stride(0), bv.stride(1)
    a.B, a.Nt, a.n_rows, a.perm_stride, a.n_vis = B, Nt, n_rows, perm_stride, n_vis
    for name, t in (("mask", mask), ("perm", perm), ("rank", rank), ("err_rows", err_rows)):
        if t is not None:
            setattr(a, name, t.data_ptr())
    a.out, a.ld, a.stream = out.data_ptr(), ld, None
    if ragged is None:
        rc = dev.cwm_dev_gather(ctypes.byref(a))
    else:
        rc = dev.cwm_dev_gather_ragged(ctypes.byref(a), ragged[0], _lib.ptr(ragged[1]))
    if check:
        _lib.check(rc, dev)
    return rc


def check_operand(name, A, ref, exact, mode, rows=None):
    """ref float64 [M, K]; exact bool [M, K] (or a scalar): the elements whose source has no arithmetic.  Every element of the ld-wide rows written;
    the K tail exactly 0; exact elements bitwise; the others within the bound of the module docstring.  `rows`: check only these rows' values
    (the whole buffer must still have been written)."""
    planes = MODES[mode][1]
    M, K = ref.shape
    Kpad = A.shape[1] // planes
    assert A.shape[0] == M and Kpad >= K
    hi, lo = decode(A, planes, Kpad)
    for p in (hi, lo):
        if p is not None:
            assert not torch.isnan(p.float()).any(), (name, mode, "elements left unwritten")
            assert (bits(p[:, K:]) == 0).all(), (name, mode, "K tail")
    hi, lo = hi[:, :K], (lo[:, :K] if lo is not None else None)
    exact = torch.as_tensor(exact).expand(M, K).clone()
    keep = torch.ones(M, dtype=torch.bool) if rows is None else rows
    exact_k, arith_k = exact & keep[:, None], ~exact & keep[:, None]
    r32 = ref.float()  # (exact sources: ref IS an fp32 input)
    hi_ref = r32.to(torch.bfloat16)
    assert torch.equal(bits(hi)[exact_k], bits(hi_ref)[exact_k]), (name, mode, "hi plane of the sources without arithmetic")
    if lo is not None:
        lo_ref = (r32 - hi_ref.float()).to(torch.bfloat16)
        assert torch.equal(bits(lo)[exact_k], bits(lo_ref)[exact_k]), (name, mode, "lo plane of the sources without arithmetic")
    if arith_k.any():
        got = hi.double() + (lo.double() if lo is not None else 0.0)
        err = (got - ref).abs()
        rel = 2.0 ** -16 if mode == "parity" else 2.0 ** -8
        bound = rel * ref.abs() + 1e-6 * ref[arith_k].abs().max().item()
        print(f"[gather {name} {mode}] max-abs {err[arith_k].max().item():.3e}, worst error / bound {(err / bound)[arith_k].max().item():.3f}")
        assert (err <= bound)[arith_k].all(), (name, mode, err[arith_k].max().item())
    else:
        print(f"[gather {name} {mode}] bitwise")


def run_index(dev, mode, x, C, P, mask, n_vis, Nt, ld, normalize, kind=_lib.DEV_GATHER_INDEX):
    """-> (operand, perm, rank, err_rows) of the index form (or of the three launches it replaced) on mask [B, L]"""
    B, L = mask.shape
    A = new_operand(B * n_vis, ld, MODES[mode][1])
    perm = torch.full((B, L), -1, dtype=torch.int32, device="cuda")
    rank = torch.full((B, L), -1, dtype=torch.int32, device="cuda")
    err = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    gather_call(dev, kind, mode, A, ld, B, n_vis, Nt, perm_stride=(L if L != Nt else 0), x=x, C=C, P=P, normalize=normalize, mask=mask.cuda(), n_vis=n_vis,
                perm=perm, rank=rank, err_rows=err)
    return A, perm.cpu(), rank.cpu(), err.cpu()


# ---- ViT gather: vector mask path (rows of whole 16-byte groups) ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vit_case():
    """P = 8, C = 3, T = 2, 32 x 32 frames (Nt = 32), B = 2, 12 visible of 32"""
    base, x = strided_frames(2, 2, 3, 32, 32, seed=21)
    mask = mask_with_counts(2, 32, [12, 12], seed=22)
    return base.cuda(), x, mask, tubelets(x, 8)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("normalize", [0, 1])
def test_vit_index_gather_vector_mask_path(dev, mode, normalize):
    buf, x, mask, tok = vit_case()
    assert mask.shape[1] % 16 == 0 and not x.is_contiguous()
    A, perm, rank, err = run_index(dev, mode, (buf, x), 3, 8, mask, 12, 32, 192, normalize)
    perm_ref, rank_ref = perm_rank_of(mask)
    assert torch.equal(perm, perm_ref) and torch.equal(rank, rank_ref) and torch.equal(err, torch.zeros(2, dtype=torch.int32))
    rows, _ = gather_rows(tok, perm_ref, 12, 32)
    ref = normalized(rows, 8) if normalize else rows.double()
    check_operand(f"vit normalize {normalize}", A, ref, not normalize, mode)


# ---- ViT gather: byte-loop mask path, K padding, a row with a wrong visible count -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_case():
    """P = 4, 12 x 20 frames (grid 3 x 5, T = 2: Nt = 30, K = 48 in rows of 64), B = 3; row 1 of the mask has 8 visible tokens instead of 10"""
    base, x = strided_frames(3, 2, 3, 12, 20, seed=31)
    mask = mask_with_counts(3, 30, [10, 8, 10], seed=32)
    return base.cuda(), x, mask, tubelets(x, 4)


@pytest.mark.parametrize("mode", list(MODES))
def test_vit_index_gather_byte_path_k_padding_and_bad_row(dev, mode):
    buf, x, mask, tok = small_case()
    assert mask.shape[1] % 16 != 0
    A, perm, rank, err = run_index(dev, mode, (buf, x), 3, 4, mask, 10, 30, 64, 0)
    perm_ref, rank_ref = perm_rank_of(mask)
    assert torch.equal(err, torch.tensor([0, 1, 0], dtype=torch.int32))
    assert torch.equal(perm, perm_ref) and torch.equal(rank, rank_ref)
    rows, _ = gather_rows(tok, perm_ref, 10, 30)
    good = torch.tensor([1, 0, 1], dtype=torch.bool).repeat_interleave(10)  # the flagged sample's rows are written, their values not specified
    check_operand("byte path", A, rows.double(), True, mode, rows=good)


# ---- padded predictor: pad slots among the gathered rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_padded_predictor_pad_slots_are_zero_rows(dev, mode):
    """perm_stride = Nt + 6; sample 0 gathers 7 real tokens and three pad slots (visible slots >= Nt), the others 10 real tokens.  The index form, then the
    patch form on the permutation it wrote: the same bits."""
    buf, x, _, tok = small_case()
    Nt, L, n_vis = 30, 36, 10
    real, pads = torch.arange(Nt), torch.arange(Nt, L)
    m0 = torch.ones(1, L, dtype=torch.uint8)
    g = gen(41)
    m0[0, real[torch.randperm(Nt, generator=g)[:7]]] = 0
    m0[0, pads[torch.randperm(6, generator=g)[:3]]] = 0
    mask = torch.cat([m0, mask_with_counts(2, L, [10, 10], seed=42, allowed=[real, real])])
    A, perm, rank, err = run_index(dev, mode, (buf, x), 3, 4, mask, n_vis, Nt, 64, 1)
    perm_ref, rank_ref = perm_rank_of(mask)
    assert torch.equal(perm, perm_ref) and torch.equal(rank, rank_ref) and torch.equal(err, torch.zeros(3, dtype=torch.int32))
    rows, pad = gather_rows(tok, perm_ref, n_vis, Nt)
    assert pad.sum().item() == 3 and pad[:n_vis].sum().item() == 3
    ref = normalized(rows, 4)
    ref[pad] = 0  # a pad slot is exact zeros (not (0 - mean) / std)
    check_operand("padded", A, ref, pad[:, None], mode)
    planes = MODES[mode][1]
    hi, lo = decode(A, planes, 64)
    for p in (hi, lo):
        if p is not None:
            assert (bits(p[pad]) == 0).all(), (mode, "pad rows")
    A2 = new_operand(3 * n_vis, 64, planes)
    gather_call(dev, _lib.DEV_GATHER_PATCH, mode, A2, 64, 3, n_vis, Nt, perm_stride=L, x=(buf, x), C=3, P=4, normalize=1, perm=perm_ref.cuda())
    assert torch.equal(A2.cpu(), A.cpu())


# ---- flow-RGB gather ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flow_case():
    """P = 4, 16 x 24 (grid 4 x 6: Nt = 24, K = 112 in rows of 128), B = 2; forward flow, backward flow and frame each with strides of its own; 9 rows per
    sample, one of sample 1's a pad slot"""
    H, W, B = 16, 24, 2
    fb = 20.0 * torch.randn(B, 3, H, W, generator=gen(51))
    bb = 20.0 * torch.randn(B + 1, 2, H + 2, W, generator=gen(52))
    xb = torch.rand(B, 4, H, W, generator=gen(53))
    fwd, bwd, x = fb[:, 1:], bb[1:, :, :H], xb[:, :3]
    g = gen(54)
    perm = torch.stack([torch.randperm(26, generator=g) for _ in range(B)]).to(torch.int32)
    perm[0, :9] = torch.randperm(24, generator=g)[:9].to(torch.int32)
    perm[1, :9] = torch.randperm(24, generator=g)[:9].to(torch.int32)
    perm[1, 4] = 25
    return (fb.cuda(), fwd), (bb.cuda(), bwd), (xb.cuda(), x), perm


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("normalize", [0, 1])
def test_flow_rgb_gather(dev, mode, normalize):
    f, b, x, perm = flow_case()
    H, W, P, B, n_rows, Nt = 16, 24, 4, 2, 9, 24
    assert len({f[1].stride(0), b[1].stride(0), x[1].stride(0)}) == 3
    A = new_operand(B * n_rows, 128, MODES[mode][1])
    gather_call(dev, _lib.DEV_GATHER_FLOW_RGB, mode, A, 128, B, n_rows, Nt, perm_stride=26, x=x, C=7, P=P, normalize=normalize, flows=(f, b), perm=perm.cuda())
    size = torch.tensor([W, H, W, H], dtype=torch.float64).repeat_interleave(P * P)  # flow / (size / 2): x channels by W, y channels by H
    flow_tok = tubelets(torch.cat([f[1], b[1]], 1).unsqueeze(1), P).double() / (0.5 * size)
    rgb_tok = tubelets(x[1].unsqueeze(1), P)
    rgb_tok = normalized(rgb_tok, P) if normalize else rgb_tok.double()
    rows, pad = gather_rows(torch.cat([flow_tok, rgb_tok], -1), perm, n_rows, Nt)
    assert pad.sum().item() == 1
    exact = pad[:, None] | (torch.arange(7 * P * P) >= (7 if normalize else 4) * P * P)[None, :]
    check_operand(f"flow-rgb normalize {normalize}", A, rows, exact, mode)


# ---- IMU gather ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_imu_gather(dev, mode):
    """C = 6, tubelet 16, L = 64 (4 tokens, K = 96 in rows of 128), B = 2, 3 rows per sample, one of them a pad slot"""
    B, C, L, tub, Nt, n_rows = 2, 6, 64, 16, 4, 3
    imu = torch.randn(B, C, L, generator=gen(61))
    perm = torch.tensor([[2, 0, 3, 1, 4], [1, 4, 2, 0, 3]], dtype=torch.int32)
    A = new_operand(B * n_rows, 128, MODES[mode][1])
    gather_call(dev, _lib.DEV_GATHER_IMU, mode, A, 128, B, n_rows, Nt, perm_stride=5, imu=imu.cuda(), tubelet=tub, perm=perm.cuda())
    tok = imu.reshape(B, C, Nt, tub).permute(0, 2, 1, 3).reshape(B, Nt, C * tub)  # token l, K order (c, s)
    rows, pad = gather_rows(tok, perm, n_rows, Nt)
    assert pad.sum().item() == 1
    check_operand("imu", A, rows.double(), True, mode)


# ---- the fused index prologue against the launches it replaced -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", ["vector", "byte"])
def test_fused_index_gather_equals_the_three_launches(dev, mode, case):
    """mask_to_perm + patch gather + perm_to_rank on the same inputs: the same bits in perm, rank and the operand"""
    if case == "vector":
        buf, x, mask, _ = vit_case()
        C, P, n_vis, Nt, ld = 3, 8, 12, 32, 192
    else:
        buf, x, mask, _ = small_case()
        mask = mask.clone()
        mask[1] = mask[0].flip(0)  # (the unfused form needs every row's count right)
        C, P, n_vis, Nt, ld = 3, 4, 10, 30, 64
    fused = run_index(dev, mode, (buf, x), C, P, mask, n_vis, Nt, ld, 1)
    unfused = run_index(dev, mode, (buf, x), C, P, mask, n_vis, Nt, ld, 1, kind=_lib.DEV_GATHER_INDEX_UNFUSED)
    for name, a, b in zip(("operand", "perm", "rank"), fused, unfused):
        assert torch.equal(a.cpu(), b.cpu()), (case, mode, name)
    assert not fused[3].any() and unfused[3][0].item() == 0


# ---- long mask rows: the scan across waves, and the 32-byte-per-thread vector path ----------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("H,W", [(80, 104), (160, 208)])
def test_index_gather_long_mask_rows(dev, mode, H, W):
    """P = 4, T = 2, B = 2.  80 x 104: L = 1040, 16 bytes of the mask row per thread, 65 threads hold tokens -- the exclusive prefix of a thread in
    waves 1 .. adds the earlier waves' totals.  160 x 208: L = 4160 > 4096, 32 bytes per thread, 130 threads.  37 visible tokens spread over the whole
    row (and the row's last token among them); perm, rank, err_rows exact, the operand bitwise."""
    P, T, B, n_vis = 4, 2, 2, 37
    Nt = T * (H // P) * (W // P)
    assert Nt % 16 == 0 and Nt in (1040, 4160)
    base, x = strided_frames(B, T, 3, H, W, seed=71)
    mask = mask_with_counts(B, Nt, [n_vis - 1, n_vis - 1], seed=72, allowed=[torch.arange(Nt - 1)] * B)
    mask[:, Nt - 1] = 0
    A, perm, rank, err = run_index(dev, mode, (base.cuda(), x), 3, P, mask, n_vis, Nt, 64, 0)
    perm_ref, rank_ref = perm_rank_of(mask)
    assert (perm_ref[:, :n_vis] >= 64 * (16 if Nt == 1040 else 32)).any(), "no visible token past wave 0"
    assert torch.equal(perm, perm_ref) and torch.equal(rank, rank_ref) and torch.equal(err, torch.zeros(B, dtype=torch.int32))
    rows, _ = gather_rows(tubelets(x, P), perm_ref, n_vis, Nt)
    check_operand(f"long rows L {Nt}", A, rows.double(), True, mode)
