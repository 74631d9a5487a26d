"""tests/engine_rows_restatement.py (the float64 yardstick of tests/test_engine_kernels_gpu.py) against the model's semantics written the obvious way:
reshape / permute for the Q/K/V scatter, x[:, -Nm:] for the kept rows, F.layer_norm on the slice, F.linear followed by indexed adds for the row maps.
No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import engine_rows_restatement as R


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd64(*shape, g):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def test_map_row_identity_offset_and_map():
    assert R.map_row(7) == (7, 7)
    # three samples of 5 kept rows at the end of 12: row 5 b + i -> 12 b + 7 + i, residual row the same
    assert [R.map_row(m, **R.kept_rows(12, 5)) for m in (0, 4, 5, 14)] == [(7, 7), (11, 11), (19, 19), (35, 35)]
    rowmap = np.array([9, 2, 11, 0, 0, 0, 3, 10, 1, 0, 0, 0])  # two samples, stride 6, three rows each
    assert [R.map_row(m, rows_in=3, rows_out=6, resid_rowmap=rowmap, map_stride=6) for m in range(6)] == [(0, 9), (1, 2), (2, 11), (6, 3), (7, 10), (8, 1)]
    out, res = R.row_maps(6, rows_in=3, rows_out=3, resid_rowmap=rowmap, map_stride=6)
    assert out.tolist() == list(range(6)) and res.tolist() == [9, 2, 11, 3, 10, 1]


@pytest.mark.parametrize("B,n_tok,n_out,N,K", [(3, 19, 7, 16, 24), (2, 8, 1, 32, 8), (1, 10, 5, 16, 16), (2, 6, 6, 16, 8)])
def test_kept_rows_are_the_last_rows_of_every_sample(B, n_tok, n_out, N, K):
    """the pruned block's residual GEMM: x[:, -n_out:] += linear(a) in place, the rows in front of them untouched; wider rows (ldc > N) keep their tail"""
    g = gen(n_tok)
    a, w, b = rnd64(B * n_out, K, g=g), rnd64(N, K, g=g), rnd64(N, g=g)
    x = rnd64(B, n_tok, N + 8, g=g)
    want = x.clone()
    want[:, -n_out:, :N] += F.linear(a, w, b).reshape(B, n_out, N)
    flat = x.reshape(B * n_tok, N + 8)
    got = R.gemm_f32(a, w, b, flat, resid=flat, **R.kept_rows(n_tok, n_out))
    assert torch.equal(got.reshape(B, n_tok, N + 8), want)
    assert torch.equal(got.reshape(B, n_tok, N + 8)[:, :n_tok - n_out], x[:, :n_tok - n_out])


@pytest.mark.parametrize("rows_out_is_stride", [False, True])
def test_residual_row_map_is_an_indexed_add(rows_out_is_stride):
    """embed_stream (rows_out == rows_in) and to_decoder (rows_out = the slot count): out[b][i] = linear(a)[b][i] + table[perm[b][i]], the table extended by pad slots"""
    B, n_vis, n_tok, pad, N, K = 3, 5, 9, 4, 16, 8
    slots = n_tok + pad
    g = gen(3)
    a, w = rnd64(B * n_vis, K, g=g), rnd64(N, K, g=g)
    table = rnd64(slots, N, g=g)
    perm = torch.stack([torch.randperm(slots, generator=g) for _ in range(B)])
    assert (perm[:, :n_vis] >= n_tok).any()  # a pad slot among the visible rows
    rows_out = slots if rows_out_is_stride else n_vis
    C = rnd64(B * rows_out, N, g=g)
    want = C.clone().reshape(B, rows_out, N)
    want[:, :n_vis] = F.linear(a, w).reshape(B, n_vis, N) + table[perm[:, :n_vis]]
    got = R.gemm_f32(a, w, None, C, resid=table, rows_in=n_vis, rows_out=rows_out, resid_rowmap=perm.reshape(-1).numpy(), map_stride=slots)
    assert torch.equal(got.reshape(B, rows_out, N), want)


@pytest.mark.parametrize("B,N,H,hd", [(2, 7, 3, 64), (1, 5, 1, 64), (3, 4, 3, 32), (2, 3, 3, 16)])
def test_qkv_scatter_is_reshape_permute(B, N, H, hd):
    """`qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)` (VideoMAE/utils.py Attention.forward), q scaled"""
    y = rnd64(B * N, 3 * H * hd, g=gen(N))
    q, k, v = y.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    got = R.qkv_scatter(y, B, N, H, hd, 0.125)
    assert torch.equal(got[0], (q * 0.125).reshape(B * H, N, hd))
    assert torch.equal(got[1], k.reshape(B * H, N, hd)) and torch.equal(got[2], v.reshape(B * H, N, hd))
    assert not torch.equal(got[1], got[0] / 0.125)  # (the three thirds are told apart)


@pytest.mark.parametrize("B,N,H,q_off,n_q", [(2, 37, 2, 20, 17), (1, 50, 3, 0, 13), (2, 9, 1, 8, 1), (1, 12, 2, 0, 0)])
def test_attention_window_is_a_row_slice_of_the_full_attention(B, N, H, q_off, n_q):
    qkv = rnd64(B, N, 3 * H * 64, g=gen(N))
    q, k, v = qkv.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    full = (((q * 0.125) @ k.transpose(-2, -1)).softmax(-1) @ v).transpose(1, 2).reshape(B, N, H * 64)
    got = R.attention_window(qkv, H, q_off, n_q)
    n = n_q or N
    assert got.shape == (B, n, H * 64)
    assert (got - full[:, q_off:q_off + n]).abs().max().item() <= 1e-13


@pytest.mark.parametrize("B,n_tok,n_out,D,ldx", [(3, 11, 4, 24, 24), (2, 7, 1, 8, 16), (1, 9, 9, 40, 48)])
def test_layernorm_row_map_is_layer_norm_of_the_slice(B, n_tok, n_out, D, ldx):
    """run_mlp / head_rows: norm(x[:, -n_out:]) (vmae.py: head(norm(x[:, -Nm:])))"""
    g = gen(D)
    x = rnd64(B, n_tok, ldx, g=g) * 3 + 1
    gamma, beta = 1 + 0.1 * rnd64(D, g=g), 0.1 * rnd64(D, g=g)
    want = F.layer_norm(x[:, -n_out:, :D], (D,), gamma, beta, 1e-6).reshape(B * n_out, D)
    got = R.layernorm_rows(x.reshape(B * n_tok, ldx), gamma, beta, 1e-6, D, B * n_out, rows_out_per_b=n_out, rows_in_per_b=n_tok, in_offset=n_tok - n_out)
    assert (got - want).abs().max().item() <= 1e-13
    ident = R.layernorm_rows(x.reshape(B * n_tok, ldx), gamma, beta, 1e-6, D, 5)
    assert (ident - F.layer_norm(x.reshape(B * n_tok, ldx)[:5, :D], (D,), gamma, beta, 1e-6)).abs().max().item() <= 1e-13
    assert [R.layernorm_in_row(r, n_out, n_tok, n_tok - n_out) for r in (0, n_out - 1, n_out)] == [n_tok - n_out, n_tok - 1, 2 * n_tok - n_out]


@pytest.mark.parametrize("B,Nt,n_vis,D", [(2, 9, 4, 8), (1, 5, 0, 4), (2, 6, 6, 4)])
def test_fill_mask_tokens_is_an_indexed_assignment(B, Nt, n_vis, D):
    """vmae.py:556-557: cat([x_vis + pos_vis, mask_token + pos_mask]) -- the masked half"""
    g = gen(Nt)
    x = torch.randn(B, Nt, D, generator=g)
    tok, pos = torch.randn(D, generator=g), torch.randn(Nt + 3, D, generator=g)
    perm = torch.stack([torch.randperm(Nt + 3, generator=g)[:Nt] for _ in range(B)])
    want = x.clone()
    want[:, n_vis:] = tok + pos[perm[:, n_vis:]]
    got = R.fill_mask_tokens(x, tok, pos, perm, n_vis)
    assert got.dtype == torch.float32 and torch.equal(got, want) and torch.equal(got[:, :n_vis], x[:, :n_vis])


def test_split_bf16_is_exact_where_it_must_be():
    """hi + lo reproduces small integers and 16-bit significands exactly, hi rounds to nearest even, lo carries the rest to 2^-17 relative"""
    ints = torch.arange(-300, 301).float()
    hi, lo = R.split_bf16(ints)
    assert torch.equal(hi.float() + lo.float(), ints)
    assert torch.equal(hi[300 - 256:300 + 257].float(), ints[300 - 256:300 + 257]) and (lo[300 - 256:300 + 257].float() == 0).all()
    # ties: 1 + 2^-8 lies halfway between bf16 1 and 1 + 2^-7 -> the even one (1); 1 + 3 * 2^-8 -> 1 + 2^-6
    t = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)])
    hi, lo = R.split_bf16(t)
    assert hi.float().tolist() == [1.0, 1 + 2.0 ** -6, -1.0] and lo.float().tolist() == [2.0 ** -8, -2.0 ** -8, -2.0 ** -8]
    v = torch.randn(4096, generator=gen(1))
    hi, lo = R.split_bf16(v)
    assert ((hi.float() + lo.float() - v).abs() <= v.abs() * 2.0 ** -17).all()
    assert torch.equal(hi, v.to(torch.bfloat16))


@pytest.mark.parametrize("planes", [1, 2])
def test_operand_positions_are_what_the_test_decoder_reads(planes):
    """a_pos as restated here = the layout tests/gpu_utils.py decode() reads (the gather and RAFT kernel tests' reader)"""
    import gpu_utils

    ld = 96
    hi_pos, lo_pos = R.operand_positions(ld, planes)
    row = torch.full((1, planes * ld), -1, dtype=torch.int16)
    row[0, torch.from_numpy(hi_pos)] = torch.arange(ld, dtype=torch.int16)
    if planes == 2:
        row[0, torch.from_numpy(lo_pos)] = torch.arange(ld, dtype=torch.int16) + 1000
        assert hi_pos[40] == 72 and lo_pos[40] == 104  # 64 (c / 32) + c % 32, the lo half 32 further
    hi, lo = gpu_utils.decode(row, planes, ld)
    assert torch.equal(gpu_utils.bits(hi)[0], torch.arange(ld, dtype=torch.int16))
    assert lo is None if planes == 1 else torch.equal(gpu_utils.bits(lo)[0], torch.arange(ld, dtype=torch.int16) + 1000)
