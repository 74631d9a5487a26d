"""The launch forms of a ragged batch one launch at a time, on a real MI355X, through the development library (include/cwm_hip_dev.h
cwm_dev_gather_ragged, cwm_dev_fill_mask_tokens_ragged, cwm_dev_attention_ragged, cwm_dev_unembed_ragged) against tests/ragged_rows_restatement.py
(pinned on the CPU by tests/test_ragged_kernels_cpu.py).

These are index and copy kernels: integers are compared for equality, floats bit for bit, both bf16 planes of an operand.  The exceptions: operand rows
gathered with normalize = 1 (the bound of test_gather_kernels_gpu.check_operand) and ONE attention case that also goes against the float64 softmax.
Every output buffer starts as a sentinel bit pattern between two guards of 64 elements, which must come back untouched; every case first asserts on the
restatement alone that it holds what it is there for (a row at the minimum, at the cap and between; a padding row; a row left alone)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import engine_rows_restatement as R
import ragged_rows_restatement as RR
from counterfactualworldmodels_amd import _lib
from gpu_utils import NAN_BF16, decode, stream
from test_gather_kernels_gpu import MODES, check_operand, gather_call, gen, mask_with_counts, normalized, tubelets
from test_ragged_attention_gpu import DENSE_CASES, SENTINEL as O_SENTINEL, TOL as ATTN_TOL, _bind as bind_ragged, ragged as attention_ragged_f32

pytestmark = pytest.mark.gpu

GUARD = 64
INT_SENT = -0x33333334  # 0xCCCCCCCC
F32_SENT = -12345.75
ERR_INVALID, ERR_MASK = -1, -3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return bind_ragged(_lib.get_dev_lib())


class Guarded:
    """n elements filled with `fill` between two guards of 64 elements filled with `guard`, one allocation; .t is the view the kernel gets"""

    def __init__(self, shape, dtype, fill, guard=None):
        n = 1
        for s in shape:
            n *= s
        self.guard = fill if guard is None else guard
        self.full = torch.full((n + 2 * GUARD,), self.guard, dtype=dtype, device="cuda")
        self.t = self.full[GUARD:GUARD + n].view(*shape)
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        torch.cuda.synchronize()
        f = self.full.cpu()
        return bool((f[:GUARD] == self.guard).all() and (f[-GUARD:] == self.guard).all())


def nonvacuous(counts, lo, cap):
    cs = [int(c) for c in counts]
    return any(c == lo for c in cs), any(c == cap for c in cs), any(lo < c < cap for c in cs)


# ==== the index prologue, fused and unfused =========================================================================================================
# name -> (H, W, P, ld, [(n_vis_min, cap, counts)]): C = 3, T = 2.  Each geometry: a plain band; n_vis_min = 1 with a row of one visible token; cap = Nt with
# a row that masks nothing.  At 4160 tokens B = 2, so the three kinds of row (minimum, cap, between) are spread over the scenarios.
GEOMETRIES = {
    "byte-30": (12, 20, 4, 64, [(7, 12, [7, 12, 9]), (1, 12, [1, 12, 5]), (10, 30, [10, 30, 17])]),        # L % 16 != 0: the byte loop; K = 48 in rows of 64
    "vector-32": (32, 32, 8, 192, [(7, 12, [7, 12, 9]), (1, 12, [1, 12, 5]), (10, 32, [10, 32, 17])]),      # one 16-byte load per thread
    "vector-4160": (160, 208, 4, 64, [(33, 40, [33, 40]), (33, 40, [36, 40]), (1, 40, [1, 37]), (4100, 4160, [4160, 4128])]),  # two loads per thread
}
# rows outside the range: below the minimum, above the cap, all masked; and two rows in range
OUTSIDE = {
    "byte-30": (7, 12, [6, 13, 0, 7, 12]),
    "vector-32": (7, 12, [6, 13, 0, 7, 12]),
    "vector-4160": (33, 40, [32, 36]),
    "vector-4160-above": (33, 40, [36, 41]),
    "vector-4160-empty": (33, 40, [0, 33]),
}


@functools.lru_cache(maxsize=None)
def frames_of(name):
    """(device buffer, strided CPU view, tubelets [B, Nt, K]) for up to 5 samples of a geometry"""
    H, W, P, _, _ = GEOMETRIES[name.split("-above")[0].split("-empty")[0]]
    base = torch.randn(5, 3, 4, H, W, generator=gen(H + W))
    x = base[:, :2, :3]
    assert not x.is_contiguous()
    return base.cuda(), x, tubelets(x, P)


@functools.lru_cache(maxsize=None)
def scenario(name, n_vis_min, cap, counts, seed):
    """mask and the restated prologue of one scenario (CPU, once)"""
    geo = name.split("-above")[0].split("-empty")[0]
    H, W, P, _, _ = GEOMETRIES[geo]
    Nt = 2 * (H // P) * (W // P)
    mask = mask_with_counts(len(counts), Nt, list(counts), seed=seed)
    return (mask,) + RR.index_prologue(mask, n_vis_min, cap)


def run_prologue(dev, kind, mode, name, mask, n_vis_min, cap, normalize, counts_buf=True, check=True):
    geo = name.split("-above")[0].split("-empty")[0]
    H, W, P, ld, _ = GEOMETRIES[geo]
    buf, x, _ = frames_of(geo)
    B, Nt = mask.shape
    planes = MODES[mode][1]
    out = dict(A=Guarded((B * cap, planes * ld), torch.int16, NAN_BF16), perm=Guarded((B, Nt), torch.int32, INT_SENT),
               rank=Guarded((B, Nt), torch.int32, INT_SENT), err=Guarded((B,), torch.int32, INT_SENT), counts=Guarded((B,), torch.int32, INT_SENT))
    rc = gather_call(dev, kind, mode, out["A"].t, ld, B, cap, Nt, x=(buf, x[:B]), C=3, P=P, normalize=normalize, mask=mask.cuda(), n_vis=cap,
                     perm=out["perm"].t, rank=out["rank"].t, err_rows=out["err"].t, ragged=(n_vis_min, out["counts"].t if counts_buf else None), check=check)
    for k, g in out.items():
        assert g.intact(), (name, mode, k, "guard")
    return rc, {k: g.t.cpu() for k, g in out.items()}


def rect_rows(dev, mode, name, perm, cap, normalize):
    """the rectangular patch gather of tokens perm[:, :cap] (all real tokens): what a row in front of a sample's count must equal bit for bit"""
    geo = name.split("-above")[0].split("-empty")[0]
    H, W, P, ld, _ = GEOMETRIES[geo]
    buf, x, _ = frames_of(geo)
    B, Nt = perm.shape
    A = Guarded((B * cap, MODES[mode][1] * ld), torch.int16, NAN_BF16)
    gather_call(dev, _lib.DEV_GATHER_PATCH, mode, A.t, ld, B, cap, Nt, x=(buf, x[:B]), C=3, P=P, normalize=normalize, perm=perm.cuda())
    assert A.intact()
    return A.t.cpu()


def own_rows_mask(counts, cap):
    """[B * cap] bool: operand row (b, i) lies in front of sample b's count"""
    return (torch.arange(cap)[None, :] < torch.as_tensor(counts)[:, None].clamp(max=cap)).reshape(-1)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_index_prologue_ragged(dev, mode, name):
    H, W, P, ld, scenarios = GEOMETRIES[name]
    planes, K = MODES[mode][1], 3 * P * P
    _, _, tok = frames_of(name)
    seen = [False, False, False]
    for si, (lo, cap, counts) in enumerate(scenarios):
        mask, perm, rank, cnt, flags = scenario(name, lo, cap, tuple(counts), 100 + si)
        B, Nt = mask.shape
        assert cnt.tolist() == counts and not flags.any()
        seen = [a or b for a, b in zip(seen, nonvacuous(counts, lo, cap))]
        own = own_rows_mask(counts, cap)
        assert (~own).any(), "no padding row"
        rows, padding = RR.gathered_rows(tok[:B], perm, cnt, cap)
        assert torch.equal(padding.reshape(-1), ~own)
        for normalize in (0, 1):
            rc, fused = run_prologue(dev, _lib.DEV_GATHER_INDEX, mode, name, mask, lo, cap, normalize)
            rc, unfused = run_prologue(dev, _lib.DEV_GATHER_INDEX_UNFUSED, mode, name, mask, lo, cap, normalize)
            rect = rect_rows(dev, mode, name, perm, cap, normalize)
            for form, got in (("fused", fused), ("unfused", unfused)):
                where = (name, mode, si, normalize, form)
                assert torch.equal(got["perm"], perm), where
                assert torch.equal(got["rank"], rank), where
                assert torch.equal(got["counts"], cnt), where
                assert not got["err"].any(), where  # fused: a flag per row; unfused: err[0] and the words the memset cleared
                ref = normalized(rows, P) if normalize else rows.double()
                check_operand("ragged %s %s scenario %d normalize %d" % (name, form, si, normalize), got["A"], ref.reshape(B * cap, K), not normalize, mode, rows=own)
                assert torch.equal(got["A"][own], rect[own]), where + ("rows in front of the count are not the rectangular gather's",)
            assert torch.equal(fused["A"][own], unfused["A"][own])
            assert (fused["A"][~own] == 0).all(), (name, mode, si, normalize, "fused: a padding row is not exact zeros in every plane")
            assert (unfused["A"][~own] != NAN_BF16).all(), (name, mode, si, normalize, "unfused: a padding row was not written")
    assert all(seen), ("the scenarios miss a row at the minimum, at the cap or between", seen)
    if name == "vector-4160":
        assert any(lo == 1 and 1 in c for lo, _, c in scenarios) and any(cap == 4160 and 4160 in c for _, cap, c in scenarios)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["byte-30", "vector-32"])
def test_index_prologue_with_the_minimum_at_nt(dev, mode, name):
    """n_vis_min == cap == Nt: no row masks anything, there is no padding row; perm and rank are the identity and the operand holds every token in order"""
    H, W, P, ld, _ = GEOMETRIES[name]
    Nt = 2 * (H // P) * (W // P)
    mask, perm, rank, cnt, flags = scenario(name, Nt, Nt, (Nt, Nt), 300)
    ident = torch.arange(Nt, dtype=torch.int32).expand(2, Nt)
    assert not mask.any() and torch.equal(perm, ident) and torch.equal(rank, ident) and cnt.tolist() == [Nt, Nt] and not flags.any()
    _, _, tok = frames_of(name)
    rect = rect_rows(dev, mode, name, perm, Nt, 0)
    for kind in (_lib.DEV_GATHER_INDEX, _lib.DEV_GATHER_INDEX_UNFUSED):
        rc, got = run_prologue(dev, kind, mode, name, mask, Nt, Nt, 0)
        assert torch.equal(got["perm"], perm) and torch.equal(got["rank"], rank) and torch.equal(got["counts"], cnt) and not got["err"].any(), (name, mode, kind)
        check_operand("ragged %s n_vis_min = Nt" % name, got["A"], tok[:2].reshape(2 * Nt, -1).double(), True, mode)
        assert torch.equal(got["A"], rect), (name, mode, kind)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(OUTSIDE))
def test_index_prologue_rows_outside_the_range(dev, mode, name):
    lo, cap, counts = OUTSIDE[name]
    mask, perm, rank, cnt, flags = scenario(name, lo, cap, tuple(counts), 200)
    B = len(counts)
    assert cnt.tolist() == counts and flags.tolist() == [int(c < lo or c > cap) for c in counts] and flags.any() and not flags.all()
    if B == 5:
        assert flags.tolist() == [1, 1, 1, 0, 0] and counts[2] == 0
    rc, fused = run_prologue(dev, _lib.DEV_GATHER_INDEX, mode, name, mask, lo, cap, 0)
    rc, unfused = run_prologue(dev, _lib.DEV_GATHER_INDEX_UNFUSED, mode, name, mask, lo, cap, 0)
    assert torch.equal(fused["err"], flags), (name, mode, "the fused form flags exactly the rows outside the range")
    assert unfused["err"][0].item() == 1 and not unfused["err"][1:].any(), (name, mode)
    in_range = own_rows_mask(counts, cap) & (flags == 0).repeat_interleave(cap)
    padding = ~own_rows_mask(counts, cap) & (flags == 0).repeat_interleave(cap)
    assert in_range.any() and padding.any()
    rect = rect_rows(dev, mode, name, perm, cap, 0)
    for form, got in (("fused", fused), ("unfused", unfused)):
        assert torch.equal(got["counts"], cnt), (name, mode, form, "counts is the true count, in range or not")
        assert torch.equal(got["perm"], perm) and torch.equal(got["rank"], rank), (name, mode, form)
        assert torch.equal(got["A"][in_range], rect[in_range]), (name, mode, form, "rows of the samples in range changed")
    assert (fused["A"][padding] == 0).all()


@pytest.mark.parametrize("mode", list(MODES))
def test_index_prologue_refusals_write_nothing(dev, mode):
    name = "byte-30"
    mask = scenario(name, 7, 12, (7, 12, 9), 100)[0]
    fused_k, unfused_k = _lib.DEV_GATHER_INDEX, _lib.DEV_GATHER_INDEX_UNFUSED
    # (kind, n_vis_min, cap, with a count array)
    for kind, lo, cap, with_counts in [(fused_k, 13, 12, True), (unfused_k, 13, 12, True), (fused_k, 7, 12, False), (unfused_k, 7, 12, False), (unfused_k, 0, 12, True),
                                       (unfused_k, -1, 12, True)]:
        rc, got = run_prologue(dev, kind, mode, name, mask, lo, cap, 0, counts_buf=with_counts, check=False)
        where = (mode, kind, lo, cap, with_counts)
        assert rc == ERR_INVALID and dev.cwm_last_error(), where
        assert (got["A"] == NAN_BF16).all() and (got["perm"] == INT_SENT).all() and (got["rank"] == INT_SENT).all() and (got["counts"] == INT_SENT).all(), where
        if kind == fused_k:
            assert (got["err"] == INT_SENT).all(), where
        else:  # the memset of the error words precedes the launch that refuses, as in the model: they are cleared, nothing else
            assert (got["err"] == 0).all(), where
    rc, got = run_prologue(dev, fused_k, mode, name, mask, 7, 12, 0)  # and the entry point works afterwards
    assert rc == 0 and not got["err"].any()


# ==== the mask-token fill ===============================================================================================================================
def run_fill(dev, x0, tok, pos, perm, counts, n_vis_min, D, check=True):
    B, Nt = perm.shape
    x = Guarded((B, Nt, D), torch.float32, F32_SENT)
    x.t.copy_(x0)
    td, pd, permd = tok.cuda(), pos.cuda(), perm.to(torch.int32).cuda()
    cd = torch.as_tensor(counts, dtype=torch.int32).cuda()
    rc = dev.cwm_dev_fill_mask_tokens_ragged(x.t.data_ptr(), td.data_ptr(), pd.data_ptr(), permd.data_ptr(), cd.data_ptr(), B, Nt, n_vis_min, D, stream())
    if check:
        _lib.check(rc, dev)
    assert x.intact()
    return rc, x.t.cpu()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("Nt", [30, 197])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [4, 100, 128, 384])
def test_fill_mask_tokens_ragged(dev, D, B, Nt):
    lo, mid = Nt // 3, Nt // 3 + max(2, Nt // 5)
    scenarios = [[lo, mid, Nt]] if B == 3 else [[lo], [mid], [Nt]]
    g = gen(D + Nt)
    tok, pos = torch.randn(D, generator=g), torch.randn(Nt, D, generator=g)
    x0 = torch.full((B, Nt, D), F32_SENT)
    seen = set()
    for counts in scenarios:
        mask = mask_with_counts(B, Nt, counts, seed=D + Nt + B)
        perm, _, cnt, flags = RR.index_prologue(mask, lo, Nt)
        assert cnt.tolist() == counts and not flags.any()
        seen |= set(counts)
        want = RR.fill_mask_tokens(x0, tok, pos, perm, cnt)
        _, got = run_fill(dev, x0, tok, pos, perm, counts, lo, D)
        assert same_bits(got, want), (D, B, Nt, counts)
        for b, c in enumerate(counts):
            assert (got[b, :c] == F32_SENT).all(), (D, B, Nt, b, "a row in front of the sample's count was written (the band [n_vis_min, count) included)")
            assert same_bits(got[b, c:], tok + pos[perm[b, c:].long()]) and (c == Nt or (got[b, c:] != F32_SENT).all())
    assert seen == {lo, mid, Nt} and lo < mid < Nt  # a row at the minimum, one with a band left alone, one with no write at all
    # all counts at the minimum: the rectangular fill at that n_vis
    mask = mask_with_counts(B, Nt, [lo] * B, seed=D)
    perm = RR.index_prologue(mask, lo, Nt)[0]
    _, got = run_fill(dev, x0, tok, pos, perm, [lo] * B, lo, D)
    rect = Guarded((B, Nt, D), torch.float32, F32_SENT)
    td, pd, permd = tok.cuda(), pos.cuda(), perm.cuda()
    _lib.check(dev.cwm_dev_fill_mask_tokens(rect.t.data_ptr(), td.data_ptr(), pd.data_ptr(), permd.data_ptr(), B, Nt, lo, D, stream()), dev)
    assert rect.intact() and same_bits(got, rect.t.cpu())
    # n_vis_min == Nt: nothing to do
    rc, got = run_fill(dev, x0, tok, pos, perm, [Nt] * B, Nt, D)
    assert rc == 0 and (got == F32_SENT).all()


def test_fill_mask_tokens_ragged_refuses_a_width_that_is_no_multiple_of_4(dev):
    B, Nt, D = 2, 30, 6
    g = gen(6)
    tok, pos = torch.randn(D, generator=g), torch.randn(Nt, D, generator=g)
    perm = RR.index_prologue(mask_with_counts(B, Nt, [10, 12], seed=6), 10, 12)[0]
    rc, got = run_fill(dev, torch.full((B, Nt, D), F32_SENT), tok, pos, perm, [10, 12], 10, D, check=False)
    assert rc == ERR_INVALID and dev.cwm_last_error() and (got == F32_SENT).all()


# ==== attention as the encoder blocks of a ragged batch launch it =====================================================================================
PREFILL = 0x4040  # bf16 3.0 in every plane: "LN1's rows", finite and recognisable


def attention_buffers(B, N, D, ldo, planes):
    hi_pos, lo_pos = R.operand_positions(ldo, planes)
    used = torch.from_numpy(hi_pos[:D] if planes == 1 else np.concatenate([hi_pos[:D], lo_pos[:D]]))
    img = torch.full((B * N, planes * ldo), NAN_BF16, dtype=torch.int16)
    img[:, used] = PREFILL
    o = Guarded((B * N, planes * ldo), torch.int16, NAN_BF16)
    o.t.copy_(img)
    return o, img, used


def run_attention_ragged(dev, mode, qkv_d, lens, B, N, H, ldo, n_q=0, check=True):
    planes, D = MODES[mode][1], 64 * H
    o, img, used = attention_buffers(B, N, D, ldo, planes)
    g = _lib.new_dev_conj_args(_lib.CwmDevAttentionArgs)
    g.mode, g.qkv, g.B, g.N, g.H, g.q_off, g.n_q = MODES[mode][0], qkv_d.data_ptr(), B, N, H, 0, n_q
    g.o, g.ldo, g.stream = o.t.data_ptr(), ldo, stream()
    ld = torch.tensor(lens, dtype=torch.int32).cuda()
    rc = dev.cwm_dev_attention_ragged(ctypes.byref(g), ld.data_ptr())
    if check:
        _lib.check(rc, dev)
    assert o.intact(), (mode, B, N, H, ldo, "guard")
    return rc, o.t.cpu(), img, used


def merged(raw, ldo, planes, D):
    """hi + lo in fp32, as cwm_attention_ragged merges the planes"""
    hi, lo = decode(raw, planes, ldo)
    v = hi[:, :D].float()
    return v + lo[:, :D].float() if planes == 2 else v


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("wide", [0, 64])
@pytest.mark.parametrize("case", range(len(DENSE_CASES)))
def test_engine_form_attention_writes_its_valid_rows_in_place(dev, mode, wide, case):
    (B, N, H), lens = DENSE_CASES[case]
    planes, D = MODES[mode][1], 64 * H
    ldo = D + wide
    assert any(n == N for n in lens) and any(n < N for n in lens)  # a sample written whole, and rows left alone
    qkv = torch.randn(B, N, 3 * D, generator=gen(N + 11))
    qd = qkv.cuda()
    rc, ref = attention_ragged_f32(dev, qkv, lens, H, mode)  # the stand-alone entry point: same kernel, same options, planes merged to fp32
    _lib.check(rc, dev)
    _, raw, img, used = run_attention_ragged(dev, mode, qd, lens, B, N, H, ldo)
    valid = (torch.arange(N)[None, :] < torch.tensor(lens)[:, None]).reshape(-1)
    got = merged(raw, ldo, planes, D)
    assert same_bits(got[valid], ref.reshape(B * N, D)[valid]), (mode, case, ldo, "valid rows are not bitwise the stand-alone result")
    assert (ref.reshape(B * N, D)[~valid] == O_SENTINEL).all()
    assert torch.equal(raw[~valid], img[~valid]), (mode, case, ldo, "a row at or past its sample's length lost the bits it held")
    pad = torch.ones(planes * ldo, dtype=torch.bool)
    pad[used] = False
    assert (raw[:, pad] == NAN_BF16).all(), (mode, case, ldo, "columns outside [0, D) were written")
    assert pad.any() == (wide > 0)
    if case == 0:  # ... and not two copies of one mistake: the dense softmax over the valid keys in float64
        dense = RR.attention_rows(qkv, lens, H).reshape(B * N, D)
        err = (got.double() - dense)[valid].abs().max().item()
        print("engine-form attention %s %s ldo %d: max-abs error against the float64 softmax %.3e" % (mode, (B, N, H), ldo, err))
        assert err <= ATTN_TOL[mode], (mode, err)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", [0, 2])
def test_engine_form_attention_skips_a_sample_whose_length_is_outside_1_to_N(dev, mode, case):
    (B, N, H), lens = DENSE_CASES[case]
    D = 64 * H
    qd = torch.randn(B, N, 3 * D, generator=gen(N + 11)).cuda()
    _, clean, img, _ = run_attention_ragged(dev, mode, qd, lens, B, N, H, D)
    bad = list(lens)
    bad[0], bad[2] = 0, N + 1
    _, raw, _, _ = run_attention_ragged(dev, mode, qd, bad, B, N, H, D)
    raw, clean, img = (t.view(B, N, -1) for t in (raw, clean, img))
    for b in range(B):
        if b in (0, 2):
            assert torch.equal(raw[b], img[b]), (mode, case, b, "a sample with a length outside [1, N] was written")
        else:
            assert torch.equal(raw[b], clean[b]), (mode, case, b)
    assert not torch.equal(clean[0], img[0])


def test_engine_form_attention_refuses_key_len_with_a_query_window(dev):
    B, N, H = 2, 200, 1
    qd = torch.randn(B, N, 192, generator=gen(3)).cuda()
    for mode in MODES:
        rc, raw, img, _ = run_attention_ragged(dev, mode, qd, [N, 50], B, N, H, 64, n_q=100, check=False)
        assert rc == ERR_INVALID and b"key_len" in dev.cwm_last_error()
        assert torch.equal(raw, img)


# ==== the un-embed of a ragged batch ====================================================================================================================
def unembed_inputs(C, strided, counts, lo, seed):
    """24 x 40 frames, P = 8, T = 2 (Nt = 30).  -> x view [B, T, C, H, W] (CPU) of a device buffer, mask, y [B, Nt - lo, P P C] with NaN in front of every
    sample's own predictions, rank"""
    B, T, H, W, P = len(counts), 2, 24, 40, 8
    Nt = T * (H // P) * (W // P)
    g = gen(seed)
    base = torch.rand(B, T, C, H + (2 if strided else 0), W, generator=g)
    x = base[:, :, :, :H]
    mask = mask_with_counts(B, Nt, counts, seed=seed + 1)
    _, rank, cnt, _ = RR.index_prologue(mask, lo, max(counts))
    y = torch.randn(B, Nt - lo, P * P * C, generator=g)
    for b, c in enumerate(cnt.tolist()):
        y[b, :max(c - lo, 0)] = float("nan")
    return base, x, mask, y, rank


def run_unembed_ragged(dev, base, x, mask, y, lo, cap):
    """y: the device tensor (or a view of one) the kernel reads as y_tokens"""
    B, T, C, H, W = x.shape
    bd, md = base.cuda(), mask.cuda()
    sb, st, sc, sh, sw = x.stride()
    assert sw == 1 and sh == W
    out = Guarded((B, T, C, H, W), torch.float32, F32_SENT)
    rc = dev.cwm_dev_unembed_ragged(y.data_ptr(), bd.data_ptr() + 4 * x.storage_offset(), sb, sc, st, md.data_ptr(), B, T, C, H, W, 8, lo, cap,
                                    out.t.data_ptr(), stream())
    assert out.intact()
    return rc, out.t.cpu()


@pytest.mark.parametrize("C,strided", [(3, False), (1, False), (3, True), (1, True)])
def test_unembed_ragged(dev, C, strided):
    lo, cap, counts = 8, 14, [8, 14, 11, 9]
    assert all(nonvacuous(counts, lo, cap))
    base, x, mask, y, rank = unembed_inputs(C, strided, counts, lo, 300 + C)
    assert torch.isnan(y).any() and (x.stride(2) > 24 * 40) == strided
    want = RR.unembed(y, x, mask, rank, lo, 8)
    assert not torch.isnan(want).any()
    yd = y.cuda()
    rc, got = run_unembed_ragged(dev, base, x, mask, yd, lo, cap)
    _lib.check(rc, dev)
    assert not torch.isnan(got).any(), (C, strided, "a y row in front of a sample's own predictions was read")
    assert same_bits(got, want), (C, strided)


@pytest.mark.parametrize("C", [3, 1])
def test_unembed_ragged_reports_a_row_outside_the_range(dev, C):
    """Above the cap: every y row it reads exists.  Below the minimum, in sample 0: the masked tokens of rank < n_vis_min have no y row -- they read row 0,
    never the rows in front of the buffer (here: n_vis_min rows of NaN inside the same allocation, so that no version of the kernel leaves it)."""
    lo, cap = 8, 14
    for counts in ([9, 15, 8, 14], [5, 9, 8, 14], [0, 9, 8, 14]):
        base, x, mask, y, rank = unembed_inputs(C, False, counts, lo, 400 + C)
        B, rows, F = y.shape
        y_full = torch.full((lo + B * rows, F), float("nan"))
        y_full[lo:] = torch.nan_to_num(y, nan=0.5).reshape(B * rows, F)  # (here every row of y itself is finite: only the rows in front of it are NaN)
        yd = y_full.cuda()
        rc, got = run_unembed_ragged(dev, base, x, mask, yd[lo:], lo, cap)
        assert rc == ERR_MASK and b"between 8 and n_vis=14" in dev.cwm_last_error(), (C, counts, rc)
        assert not torch.isnan(got).any() and (got != F32_SENT).all(), (C, counts, "read in front of y_tokens")
        want = RR.unembed(torch.nan_to_num(y, nan=0.5), x, mask, rank.clamp(min=lo), lo, 8)
        good = [b for b, c in enumerate(counts) if lo <= c <= cap]
        assert same_bits(got[good], want[good]), (C, counts, "samples in range changed")
