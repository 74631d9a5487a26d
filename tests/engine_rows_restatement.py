"""Plain numpy / torch float64 statements of what the ViT engine's launch forms MEAN -- the row maps of csrc/kernels.h GemmParams and LayerNormParams,
the per-head Q/K/V scatter, the query window of the pruned last decoder block, the mask-token fill, and the split-bf16 operand -- written index by
index from the parameter structs' comments, not from the kernels.  The yardstick of tests/test_engine_kernels_gpu.py;
tests/test_engine_rows_cpu.py pins every function here to the model's semantics written the obvious way (reshape / permute, x[:, -Nm:], F.layer_norm
on the slice, F.linear followed by indexed adds), so the GPU tests do not rest on a reference that is itself wrong."""
import numpy as np
import torch


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------------
def map_row(m, rows_in=0, rows_out=0, out_row_offset=0, resid_rowmap=None, map_stride=0):
    """GemmParams: problem row m -> (output row, residual row).  rows_in == 0: identity.  Else m = b * rows_in + i goes to b * rows_out + i +
    out_row_offset, and its residual row is resid_rowmap[b * map_stride + i] if a map is given, else the output row."""
    if rows_in == 0:
        return m, m
    b, i = divmod(m, rows_in)
    out = b * rows_out + i + out_row_offset
    return out, (int(resid_rowmap[b * map_stride + i]) if resid_rowmap is not None else out)


def row_maps(M, **kw):
    """map_row of every problem row: (out_rows [M], res_rows [M]) as int64 arrays"""
    rows = [map_row(m, **kw) for m in range(M)]
    return np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows], dtype=np.int64)


def kept_rows(n_tok, n_out):
    """the rows a pruned block keeps: the LAST n_out of every sample's n_tok, as the GemmParams fields (rows_in, rows_out, out_row_offset)"""
    return dict(rows_in=n_out, rows_out=n_tok, out_row_offset=n_tok - n_out)


def layernorm_in_row(r, rows_out_per_b=0, rows_in_per_b=0, in_offset=0):
    """LayerNormParams: the input row of output row r"""
    if rows_out_per_b == 0:
        return r
    b, j = divmod(r, rows_out_per_b)
    return b * rows_in_per_b + in_offset + j


# ---- GEMM epilogues, float64 ---------------------------------------------------------------------------------------------------------------------------
def linear64(a, w, bias=None):
    y = a.double() @ w.double().t()
    return y if bias is None else y + bias.double()


def gemm_f32(a, w, bias, C, resid=None, N=None, **rows):
    """EPI_F32 on a float64 copy of the output surface: C [R][ldc] (every row and column the launch does not own keeps its value); resid [*][ldr]
    is read BEFORE anything is written, so resid may be C itself"""
    y = linear64(a, w, bias)
    M, N = y.shape
    out_rows, res_rows = row_maps(M, **rows)
    assert len(set(out_rows.tolist())) == M, "two problem rows share an output row"
    out = C.double().clone()
    if resid is not None:
        y = y + resid.double()[res_rows, :N]
    out[out_rows, :N] = y
    return out


def gelu64(y):
    return 0.5 * y * (1.0 + torch.erf(y / 2.0 ** 0.5))


def qkv_scatter(y, B, n_tok, heads, head_dim, q_scale):
    """EPI_QKV: y [B * n_tok][3 * heads * head_dim], column c = which * D + h * head_dim + d of row (b, tok) -> out[which][(b * heads + h) * n_tok +
    tok][d], Q (which == 0) times q_scale.  Returns (q, k, v), each [B * heads, n_tok, head_dim]"""
    D = heads * head_dim
    out = [torch.empty(B * heads, n_tok, head_dim, dtype=y.dtype) for _ in range(3)]
    for b in range(B):
        for which in range(3):
            for h in range(heads):
                blk = y[b * n_tok:(b + 1) * n_tok, which * D + h * head_dim: which * D + (h + 1) * head_dim]
                out[which][b * heads + h] = blk * q_scale if which == 0 else blk
    return tuple(out)


# ---- attention ------------------------------------------------------------------------------------------------------------------------------------------
def attention_window(qkv, H, q_off=0, n_q=0, q_scale=0.125):
    """qkv [B, N, 3 * H * 64] -> O [B, n_q, H * 64] in float64: queries are rows [q_off, q_off + n_q) of every sample (n_q == 0: all), keys and values
    all N rows; O row b * n_q + (q - q_off), head h in columns 64 h .."""
    B, N, _ = qkv.shape
    n = n_q if n_q else N
    q, k, v = qkv_scatter(qkv.double().reshape(B * N, -1), B, N, H, 64, q_scale)
    q = q[:, q_off:q_off + n]
    p = (q @ k.transpose(-2, -1)).softmax(-1)
    return (p @ v).reshape(B, H, n, 64).permute(0, 2, 1, 3).reshape(B, n, H * 64)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------------------
def layernorm_rows(x, gamma, beta, eps, D, rows, **rowmap):
    """x [R][ldx] -> [rows][D] float64: the LayerNorm (biased variance) over the first D columns of the mapped input rows"""
    src = torch.tensor([layernorm_in_row(r, **rowmap) for r in range(rows)])
    v = x.double()[src, :D]
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    return (v - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


# ---- mask tokens ------------------------------------------------------------------------------------------------------------------------------------------
def fill_mask_tokens(x_full, mask_token, pos, perm, n_vis):
    """x_full [B, Nt, D] fp32: x_full[b][n_vis + j] = mask_token + pos[perm[b][n_vis + j]] (ONE fp32 add); rows < n_vis keep their value"""
    out = x_full.clone()
    B, Nt, _ = x_full.shape
    for b in range(B):
        for r in range(n_vis, Nt):
            out[b, r] = mask_token + pos[int(perm[b, r])]
    return out


# ---- the split-bf16 operand -------------------------------------------------------------------------------------------------------------------------------
def split_bf16(v):
    """fp32 -> (hi, lo) bf16: hi = bf16(v), lo = bf16(v - hi), both round to nearest even (csrc/common.h split_bf16 converts with `(bf16)v`; torch's
    `.to(torch.bfloat16)` rounds the same way -- tests/test_engine_kernels_gpu.py checks that claim against cwm_split_bf16 once).  v - hi is exact in
    fp32 (Sterbenz-like: hi carries the leading 8 bits of v)."""
    v = v.float()
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    return hi, lo


def operand_positions(ld, planes):
    """common.h a_pos: position of column c's hi element within a row of planes * ld bf16, and of its lo element (parity only)"""
    c = np.arange(ld)
    if planes == 1:
        return c, None
    hi = (c // 32) * 64 + c % 32
    return hi, hi + 32
