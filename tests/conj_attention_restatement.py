"""A plain-torch float64 restatement of the two attentions of the IMU-conditioned (conjoined) predictor, on the already projected tensors -- what
csrc/conj_kernels.hip (fp32 VALU forms) and csrc/conj_attention.hip (MFMA forms) compute between the projections:

  cross  `BidirectionalCrossAttention.forward` (cwm/models/transformer.py:314-378, shared_similarity=False) between its qk / v / qk_src / v_src
         projections and its output projections;
  small  `Attention.forward` (cwm/models/VideoMAE/utils.py:87-121) between the qkv projection (bias added) and the output projection.

It is the yardstick of tests/test_conj_kernels_gpu.py; tests/test_conj_kernels_cpu.py pins it to oracle/conj_oracle.py and oracle/vmae_oracle.py, which
tests/test_conj_oracle.py pins to outputs of the reference itself."""
import torch


def cross(qk, v, qk_src, v_src, heads, scale):
    """qk [B, N, 2D], v [B, N, D], qk_src [B, M, 2D], v_src [B, M, D] (D = heads * hd; head h owns columns [2 hd h, 2 hd (h + 1)) of qk / qk_src and
    [hd h, hd (h + 1)) of v / v_src) -> (y [B, N, D], y_src [B, M, D]) in float64:
      the FIRST hd columns of a head's slice:  y     = softmax_M(scale q1 k1^T) v_src
      the SECOND hd columns:                   y_src = softmax_N(scale q2_src k2^T) v"""
    qk, v, qk_src, v_src = (t.double() for t in (qk, v, qk_src, v_src))
    B, N, D = v.shape
    M = v_src.shape[1]
    hd = D // heads
    assert D == heads * hd and qk.shape == (B, N, 2 * D) and qk_src.shape == (B, M, 2 * D) and v_src.shape == (B, M, D)
    t = qk.reshape(B, N, heads, 2, hd).permute(3, 0, 2, 1, 4)      # [2][B, H, N, hd]
    s = qk_src.reshape(B, M, heads, 2, hd).permute(3, 0, 2, 1, 4)  # [2][B, H, M, hd]
    vh = v.reshape(B, N, heads, hd).permute(0, 2, 1, 3)
    vsh = v_src.reshape(B, M, heads, hd).permute(0, 2, 1, 3)
    attn = (scale * (t[0] @ s[0].transpose(-2, -1))).softmax(-1)      # [B, H, N, M]
    attn_src = (scale * (s[1] @ t[1].transpose(-2, -1))).softmax(-1)  # [B, H, M, N]
    y = (attn @ vsh).permute(0, 2, 1, 3).reshape(B, N, D)
    y_src = (attn_src @ vh).permute(0, 2, 1, 3).reshape(B, M, D)
    return y, y_src


def small(qkv, heads):
    """qkv [B, n, 3D] = [q | k | v], head h in columns [hd h, hd (h + 1)) of each third -> o [B, n, D] = softmax(q hd^-0.5 k^T) v in float64"""
    qkv = qkv.double()
    B, n, D3 = qkv.shape
    D = D3 // 3
    hd = D // heads
    assert D3 == 3 * heads * hd
    q, k, v = qkv.reshape(B, n, 3, heads, hd).permute(2, 0, 3, 1, 4)
    attn = ((q * hd ** -0.5) @ k.transpose(-2, -1)).softmax(-1)
    return (attn @ v).permute(0, 2, 1, 3).reshape(B, n, D)


# ---- "selection" inputs: every softmax is exactly one-hot in fp32, so a correct kernel returns the selected V row bit for bit ----------------------
# Queries and keys are 64 (+-e_j): a query and its key score 64 * 64 = 4096, a query and the key of the opposite sign -4096, everything else 0.  After
# the scale (>= 192^-0.5) the winner leads by >= 295, and exp(-295) (2^-426) is below the smallest fp32 denormal: the other weights are exactly 0 in
# fp32 exp / exp2, the winner's exactly 1 (4096 * c is exact, so "score - max" is exactly 0).  The sign lets 32 dimensions tell 64 keys apart.  V is
# drawn from the NON-ZERO integers of [-4, 4]: in float64 the losers' weights (1e-128) are not 0, and a zero of V would come out as 1e-126 instead.
SEL = 64.0
# (head_dim, M, N) of the bitwise cross-attention cases (B = 2, 3 heads): one per MFMA instance (head_dim / 32, M <= 32 or above), and head_dim 192 beyond
# M = 32, which only the VALU form takes
SELECTION_SHAPES = [(32, 64, 545), (96, 50, 33), (192, 32, 1031), (192, 50, 65), (32, 25, 97), (96, 32, 545)]


def sel_dim(j, hd):
    """the dimension key j % 32 lives in: spread over the whole head_dim, so that every 16-wide k-step of a score product carries some key"""
    return (5 * (j % 32) + 1) % hd


def sel_vec(j, hd):
    """key j of up to 64: +64 e_d for j < 32, -64 e_d for j >= 32"""
    assert 0 <= j < 64 and len({sel_dim(i, hd) for i in range(32)}) == 32
    x = torch.zeros(hd)
    x[sel_dim(j, hd)] = SEL if j < 32 else -SEL
    return x


def sel_values(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(1, 5, shape, generator=g).float()
    return x * (2 * torch.randint(0, 2, shape, generator=g).float() - 1)


def cross_targets(N, M):
    """t(m), the main token context row m selects.  Token 0, the last token (of a ragged 32-token chunk when N % 32 != 0; for N = 33 or 545 alone in its
    chunk), token 512 when there is one (the first token of a share's SECOND chunk in the MFMA form, 16 shares of 32-token chunks taken round-robin) and
    the last token below 512 come first; the others are spread over the tokens.  Several rows may select one token."""
    first = [0, N - 1] + ([512, 511] if N > 512 else []) + ([32, 31] if N > 32 else [])
    return [first[m] if m < len(first) else (37 * m + 11) % N for m in range(M)]


def selection_cross(B, N, M, heads, hd, seed=0):
    """-> qk, v, qk_src, v_src (fp32) and the selections: main token n takes context row sel_a[n] = (7 n + 3) % M, context row m takes token sel_b[m]"""
    assert 1 <= M <= 64
    D = heads * hd
    qk, qk_src = torch.zeros(B, N, heads, 2, hd), torch.zeros(B, M, heads, 2, hd)
    sel_a = torch.tensor([(7 * n + 3) % M for n in range(N)])
    sel_b = torch.tensor(cross_targets(N, M))
    for m in range(M):
        qk_src[:, m, :, 0] = sel_vec(m, hd)  # role A: context row m has key m
    for n in range(N):
        qk[:, n, :, 0] = sel_vec(int(sel_a[n]), hd)
    targets = sorted(set(sel_b.tolist()))  # role B: the i-th selected token has key i, every other token key 0
    assert len(targets) <= 64
    for i, t in enumerate(targets):
        qk[:, t, :, 1] = sel_vec(i, hd)
    for m in range(M):
        qk_src[:, m, :, 1] = sel_vec(targets.index(int(sel_b[m])), hd)
    v, v_src = sel_values((B, N, D), seed + 1), sel_values((B, M, D), seed + 2)  # different per batch element and head
    return qk.reshape(B, N, 2 * D), v, qk_src.reshape(B, M, 2 * D), v_src, sel_a, sel_b


def selection_small(B, n, heads, hd, seed=0):
    """-> qkv (fp32) and sel: query i takes key sel[i] = (7 i + 3) % n"""
    assert 1 <= n <= 64
    D = heads * hd
    qkv = torch.zeros(B, n, 3, heads, hd)
    sel = torch.tensor([(7 * i + 3) % n for i in range(n)])
    for i in range(n):
        qkv[:, i, 1] = sel_vec(i, hd)
        qkv[:, i, 0] = sel_vec(int(sel[i]), hd)
    qkv[:, :, 2] = sel_values((B, n, heads, hd), seed + 3)
    return qkv.reshape(B, n, 3 * D), sel
