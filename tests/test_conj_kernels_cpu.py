"""tests/conj_attention_restatement.py (the float64 yardstick of tests/test_conj_kernels_gpu.py) against the oracles that tests/test_conj_oracle.py ties
to the reference's goldens, and the "selection" inputs of the bitwise GPU cases checked on the CPU.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import conj_attention_restatement as R
from oracle import conj_oracle as O
from oracle import vmae_oracle as V


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel_err(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("B,N,M,heads,hd,ci,cs", [(2, 37, 5, 3, 32, 40, 24), (1, 70, 33, 4, 96, 48, 56), (2, 9, 50, 2, 192, 64, 32)])
def test_cross_restatement_equals_the_oracle(B, N, M, heads, hd, ci, cs):
    """projections with random float64 weights outside, the restatement, then projection / projection_src == oracle.conj_oracle.cross_attention"""
    D, g, pre = heads * hd, gen(N), "x."
    W = {pre + k: torch.randn(*shape, generator=g, dtype=torch.float64) * shape[-1] ** -0.5 for k, shape in (
        ("qk.weight", (2 * D, ci)), ("qk_src.weight", (2 * D, cs)), ("v.weight", (D, ci)), ("v_src.weight", (D, cs)), ("projection.weight", (ci, D)),
        ("projection_src.weight", (cs, D)))}
    W[pre + "projection.bias"] = torch.randn(ci, generator=g, dtype=torch.float64)
    W[pre + "projection_src.bias"] = torch.randn(cs, generator=g, dtype=torch.float64)
    x = torch.randn(B, N, ci, generator=g, dtype=torch.float64)
    s = torch.randn(B, M, cs, generator=g, dtype=torch.float64)
    y_ref, ys_ref = O.cross_attention(x, s, W, pre, heads)
    y, ys = R.cross(F.linear(x, W[pre + "qk.weight"]), F.linear(x, W[pre + "v.weight"]), F.linear(s, W[pre + "qk_src.weight"]), F.linear(s, W[pre + "v_src.weight"]),
                    heads, hd ** -0.5)
    assert y.dtype == torch.float64 and ys.dtype == torch.float64
    y = F.linear(y, W[pre + "projection.weight"], W[pre + "projection.bias"])
    ys = F.linear(ys, W[pre + "projection_src.weight"], W[pre + "projection_src.bias"])
    assert rel_err(y, y_ref) <= 1e-12 and rel_err(ys, ys_ref) <= 1e-12


def test_cross_restatement_tells_the_two_halves_and_the_two_sides_apart():
    """a restatement that swapped the halves of a head's slice, or used one softmax for both sides, would not equal itself on swapped inputs"""
    B, N, M, heads, hd = 1, 7, 4, 2, 8
    g = gen(3)
    qk, v = torch.randn(B, N, 2 * heads * hd, generator=g), torch.randn(B, N, heads * hd, generator=g)
    qs, vs = torch.randn(B, M, 2 * heads * hd, generator=g), torch.randn(B, M, heads * hd, generator=g)
    y, ys = R.cross(qk, v, qs, vs, heads, 0.3)
    _, y2 = R.cross(qs, vs, qk, v, heads, 0.3)  # the two streams exchanged WITHOUT exchanging the halves: the other half's softmax
    swap = lambda t: t.reshape(t.shape[0], t.shape[1], heads, 2, hd).flip(3).reshape(t.shape)
    y3, ys3 = R.cross(swap(qs), vs, swap(qk), v, heads, 0.3)  # ... and with the halves exchanged too: the same two results
    assert torch.allclose(ys3, y, atol=1e-14) and torch.allclose(y3, ys, atol=1e-14)
    assert y.shape == (B, N, heads * hd) and ys.shape == (B, M, heads * hd) and y2.shape == y.shape
    assert not torch.allclose(y2, y, atol=1e-3)


@pytest.mark.parametrize("B,n,heads,hd", [(2, 26, 12, 32), (1, 51, 6, 32), (2, 7, 3, 48)])
def test_small_restatement_equals_the_oracle_self_attention(B, n, heads, hd):
    """oracle.vmae_oracle.attention (the self-attention of the context stream's blocks) then the output projection"""
    D, g, pre = heads * hd, gen(n), "a."
    assert not V.PRECISION
    W = {pre + "qkv.weight": torch.randn(3 * D, D, generator=g, dtype=torch.float64) * D ** -0.5, pre + "q_bias": torch.randn(D, generator=g, dtype=torch.float64),
         pre + "v_bias": torch.randn(D, generator=g, dtype=torch.float64), pre + "proj.weight": torch.randn(D, D, generator=g, dtype=torch.float64) * D ** -0.5,
         pre + "proj.bias": torch.randn(D, generator=g, dtype=torch.float64)}
    x = torch.randn(B, n, D, generator=g, dtype=torch.float64)
    ref = V.attention(x, W, pre, heads)
    bias = torch.cat([W[pre + "q_bias"], torch.zeros(D, dtype=torch.float64), W[pre + "v_bias"]])
    o = R.small(F.linear(x, W[pre + "qkv.weight"], bias), heads)
    assert o.dtype == torch.float64
    assert rel_err(F.linear(o, W[pre + "proj.weight"], W[pre + "proj.bias"]), ref) <= 1e-12


def is_bf16(t):
    return torch.equal(t.to(torch.bfloat16).float(), t)


@pytest.mark.parametrize("hd,M,N", R.SELECTION_SHAPES)
def test_cross_selection_inputs_select_exactly(hd, M, N):
    B, heads = 2, 3
    qk, v, qk_src, v_src, sel_a, sel_b = R.selection_cross(B, N, M, heads, hd)
    for t in (qk, v, qk_src, v_src):
        assert t.dtype == torch.float32 and is_bf16(t)
    assert sel_a.tolist() == [(7 * n + 3) % M for n in range(N)]
    tb = sel_b.tolist()
    assert 0 in tb and N - 1 in tb and (N <= 512 or 512 in tb)  # token 0, the end of the ragged chunk, a second-pass chunk
    assert 4096 * hd ** -0.5 >= 295
    y64, ys64 = R.cross(qk, v, qk_src, v_src, heads, hd ** -0.5)
    assert torch.equal(y64, v_src[:, sel_a].double()) and torch.equal(ys64, v[:, sel_b].double())
    # the same statement in fp32 arithmetic: the losers' weights are exactly 0 there
    D = heads * hd
    t = qk.reshape(B, N, heads, 2, hd).permute(3, 0, 2, 1, 4)
    s = qk_src.reshape(B, M, heads, 2, hd).permute(3, 0, 2, 1, 4)
    scale = torch.tensor(hd ** -0.5, dtype=torch.float32)
    attn = (scale * (t[0] @ s[0].transpose(-2, -1))).softmax(-1)
    attn_s = (scale * (s[1] @ t[1].transpose(-2, -1))).softmax(-1)
    assert attn.dtype == torch.float32 and ((attn == 0) | (attn == 1)).all() and ((attn_s == 0) | (attn_s == 1)).all()
    assert (attn.sum(-1) == 1).all() and (attn_s.sum(-1) == 1).all()
    y32 = (attn @ v_src.reshape(B, M, heads, hd).permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(B, N, D)
    ys32 = (attn_s @ v.reshape(B, N, heads, hd).permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(B, M, D)
    assert torch.equal(y32, v_src[:, sel_a]) and torch.equal(ys32, v[:, sel_b])
    # what a (batch, head) slip would return differs from the right answer
    assert not torch.equal(v_src[0], v_src[1]) and not torch.equal(v_src[:, :, :hd], v_src[:, :, hd:2 * hd])


@pytest.mark.parametrize("hd", [32, 48, 64])
@pytest.mark.parametrize("n", [33, 64])
def test_small_selection_inputs_select_exactly(n, hd):
    B, heads = 2, 3
    qkv, sel = R.selection_small(B, n, heads, hd)
    assert qkv.dtype == torch.float32 and is_bf16(qkv)
    D = heads * hd
    want = qkv[:, :, 2 * D:][:, sel]
    assert torch.equal(R.small(qkv, heads), want.double())
    q, k, v = qkv.reshape(B, n, 3, heads, hd).permute(2, 0, 3, 1, 4)
    attn = ((q * torch.tensor(hd ** -0.5, dtype=torch.float32)) @ k.transpose(-2, -1)).softmax(-1)
    assert attn.dtype == torch.float32 and ((attn == 0) | (attn == 1)).all()
    assert torch.equal((attn @ v).permute(0, 2, 1, 3).reshape(B, n, D), want)
