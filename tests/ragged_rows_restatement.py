"""The launch forms of a ragged batch (rows with different visible-token counts in one batch) restated as plain per-row loops, from what
csrc/kernels.h and include/cwm_hip.h SAY about them (launch_index_gather / launch_mask_to_perm_ragged, launch_fill_mask_tokens_ragged,
AttnParams.key_len, UnembedParams, cwm_model_set_ragged) -- not from the kernels.  tests/test_ragged_kernels_cpu.py pins this file, without a GPU,
to torch's stable argsort, to the rectangular helpers of tests/test_gather_kernels_gpu.py and to tests/golden/ragged_tiny.npz;
tests/test_ragged_kernels_gpu.py holds the kernels to it.

Conventions: mask [B, L], non-zero = masked; n_vis_min <= count <= cap (= the call's n_vis) is a row in range; rows of sample b at and behind its own
count, up to the cap, are PADDING rows."""
import torch


def index_prologue(mask, n_vis_min, cap):
    """-> perm [B, L] int32 = [visible ascending | masked ascending] with the row's OWN count, rank [B, L] int32 (its inverse: the position of
    token tau in perm), counts [B] int32 (visible tokens of the row), flags [B] int32 (the count is outside [n_vis_min, cap])"""
    B, L = mask.shape
    perm = torch.empty(B, L, dtype=torch.int32)
    rank = torch.empty(B, L, dtype=torch.int32)
    counts = torch.empty(B, dtype=torch.int32)
    flags = torch.empty(B, dtype=torch.int32)
    for b in range(B):
        vis = [i for i in range(L) if int(mask[b, i]) == 0]
        hid = [i for i in range(L) if int(mask[b, i]) != 0]
        order = vis + hid
        for pos, tau in enumerate(order):
            perm[b, pos] = tau
            rank[b, tau] = pos
        counts[b] = len(vis)
        flags[b] = 1 if (len(vis) < n_vis_min or len(vis) > cap) else 0
    return perm, rank, counts, flags


def gathered_rows(tok, perm, counts, cap):
    """tok [B, Nt, K] (the tubelets of every token) -> (rows [B, cap, K], padding [B, cap] bool): rows [0, count) of sample b are its tokens
    perm[b, :count]; rows [count, cap) are zeros (the fused form; the unfused one leaves unspecified values there)"""
    B, _, K = tok.shape
    rows = torch.zeros(B, cap, K, dtype=tok.dtype)
    padding = torch.ones(B, cap, dtype=torch.bool)
    for b in range(B):
        for i in range(min(int(counts[b]), cap)):
            rows[b, i] = tok[b, int(perm[b, i])]
            padding[b, i] = False
    return rows, padding


def fill_mask_tokens(x_full, mask_token, pos, perm, counts):
    """x_full [B, Nt, D] fp32 -> a copy with rows [counts[b], Nt) of sample b = mask_token + pos[perm[b, row]] (one fp32 add); every other row as it
    was -- the band [n_vis_min, counts[b]) included"""
    out = x_full.clone()
    B, Nt, _ = x_full.shape
    for b in range(B):
        for j in range(int(counts[b]), Nt):
            out[b, j] = mask_token + pos[int(perm[b, j])]
    return out


def attention_rows(qkv, lens, H):
    """qkv [B, N, 3 * 64 H] -> float64 [B, N, 64 H]: row i < lens[b] of sample b = softmax over keys [0, lens[b]) of q k^T / 8, times v; rows at and past
    lens[b] are NaN here (the kernel does not write them: they keep what the buffer held)"""
    B, N, _ = qkv.shape
    out = torch.full((B, N, 64 * H), float("nan"), dtype=torch.float64)
    x = qkv.double().reshape(B, N, 3, H, 64)
    for b in range(B):
        n = int(lens[b])
        if n < 1 or n > N:
            continue
        for h in range(H):
            q, k, v = x[b, :n, 0, h], x[b, :n, 1, h], x[b, :n, 2, h]
            out[b, :n, 64 * h:64 * h + 64] = torch.softmax((q * 0.125) @ k.T, -1) @ v
    return out


def unembed(y, x, mask, rank, n_vis_min, P):
    """y [B, Nt - n_vis_min, P * P * C] (row j of a sample = decoder row n_vis_min + j; feature order (ph, pw, c)), x [B, T, C, H, W] raw frames, mask
    [B, Nt], rank [B, Nt] -> video [B, T, C, H, W]: a masked patch comes from y row rank - n_vis_min, a visible patch from x.  Pure copies."""
    B, T, C, H, W = x.shape
    gh, gw = H // P, W // P
    out = torch.empty(B, T, C, H, W, dtype=x.dtype)
    for b in range(B):
        for t in range(T):
            for hy in range(gh):
                for wx in range(gw):
                    tau = (t * gh + hy) * gw + wx
                    ys, xs = slice(hy * P, hy * P + P), slice(wx * P, wx * P + P)
                    if int(mask[b, tau]) != 0:
                        patch = y[b, int(rank[b, tau]) - n_vis_min].reshape(P, P, C)  # (ph, pw, c)
                        out[b, t, :, ys, xs] = patch.permute(2, 0, 1)
                    else:
                        out[b, t, :, ys, xs] = x[b, t, :, ys, xs]
    return out
