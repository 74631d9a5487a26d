"""tests/ragged_rows_restatement.py pinned without a GPU: to torch's stable argsort, to the rectangular helpers the gather tests already use
(tests/test_gather_kernels_gpu.py perm_rank_of / gather_rows), to the oracle's patches_to_video and to the reference's own output in
tests/golden/ragged_tiny.npz.  Everything here is an index or a copy: every comparison is exact."""
import os

import numpy as np
import torch

import ragged_rows_restatement as RR
from oracle import vmae_oracle as O
from test_gather_kernels_gpu import gather_rows, mask_with_counts, perm_rank_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_perm_and_rank_are_the_stable_argsort_of_the_mask_and_its_inverse():
    counts = [0, 1, 7, 12, 29, 30]
    mask = mask_with_counts(len(counts), 30, counts, seed=1)
    mask[2][mask[2] != 0] = 200  # any non-zero byte is "masked"
    perm, rank, got_counts, flags = RR.index_prologue(mask, 7, 29)
    want = torch.argsort((mask != 0).to(torch.int8), dim=1, stable=True)
    assert torch.equal(perm.long(), want)
    assert torch.equal(rank.long(), torch.argsort(want, dim=1))
    assert got_counts.tolist() == counts
    assert flags.tolist() == [1, 1, 0, 0, 0, 1]  # 0 and 1 below the minimum, 7 and 29 on the two ends of the range, 30 above the cap


def test_equal_counts_give_the_rectangular_helpers():
    B, Nt, K, n = 3, 30, 48, 10
    mask = mask_with_counts(B, Nt, [n] * B, seed=2)
    tok = torch.randn(B, Nt, K, generator=torch.Generator().manual_seed(3))
    perm, rank, counts, flags = RR.index_prologue(mask, n, n)
    perm_ref, rank_ref = perm_rank_of(mask)
    assert torch.equal(perm, perm_ref) and torch.equal(rank, rank_ref) and counts.tolist() == [n] * B and not flags.any()
    rows, padding = RR.gathered_rows(tok, perm, counts, n)
    rows_ref, pad_ref = gather_rows(tok, perm_ref, n, Nt)
    assert torch.equal(rows.reshape(B * n, K), rows_ref) and not padding.any() and not pad_ref.any()
    # a cap above the count: the same rows, zeros behind them
    rows2, padding2 = RR.gathered_rows(tok, perm, counts, n + 3)
    assert torch.equal(rows2[:, :n], rows) and (rows2[:, n:] == 0).all() and padding2[:, n:].all() and not padding2[:, :n].any()


def test_equal_counts_fill_is_the_rectangular_fill():
    import engine_rows_restatement as R

    B, Nt, D, n = 2, 12, 8, 5
    g = torch.Generator().manual_seed(4)
    x0, tok, pos = torch.randn(B, Nt, D, generator=g), torch.randn(D, generator=g), torch.randn(Nt, D, generator=g)
    perm = torch.stack([torch.randperm(Nt, generator=g) for _ in range(B)]).to(torch.int32)
    assert torch.equal(RR.fill_mask_tokens(x0, tok, pos, perm, [n] * B), R.fill_mask_tokens(x0, tok, pos, perm, n))
    ragged = RR.fill_mask_tokens(x0, tok, pos, perm, [n, Nt])
    assert torch.equal(ragged[1], x0[1]) and torch.equal(ragged[0], R.fill_mask_tokens(x0, tok, pos, perm, n)[0])


def test_equal_counts_unembed_is_the_oracles_composition():
    B, T, C, H, W, P, n = 2, 2, 3, 16, 24, 8, 5
    Nt = T * (H // P) * (W // P)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, T, C, H, W, generator=g)
    y = torch.randn(B, Nt - n, P * P * C, generator=g)
    mask = mask_with_counts(B, Nt, [n] * B, seed=6)
    _, rank, _, _ = RR.index_prologue(mask, n, n)
    assert torch.equal(RR.unembed(y, x, mask, rank, n, P), O.pred_patches_to_video(y, x, mask, P))
    # a patch-sized video of token values comes back as patches_to_video lays it out
    patches = torch.randn(B, Nt, P * P * C, generator=g)
    everything_masked = torch.ones(B, Nt, dtype=torch.uint8)
    ident = torch.arange(Nt, dtype=torch.int32).expand(B, Nt)
    assert torch.equal(RR.unembed(patches, x, everything_masked, ident, 0, P), O.patches_to_video(patches, T, C, H, W, P))


def test_unembed_reproduces_the_reference_video_of_ragged_tiny():
    """make_golden_ragged.py: `video` is the reference's `G.predict(x[r:r+1], mask[r:r+1], frame=None)`, i.e. pred_patches_to_video (prediction.py:245-259)
    on the predictor's output -- y_out[~mask] = patches of the RAW x, y_out[mask] = y, then patches_to_video: a pure copy on both sides, no un-normalisation
    (that branch is for predictors with a main_stream).  `y_tokens` holds the output of a second, identical forward call of the same CPU model on the same
    row; so masked pixels are compared exactly too."""
    g = np.load(os.path.join(GOLDEN, "ragged_tiny.npz"))
    x, mask, y, video = (torch.from_numpy(g[k]) for k in ("x", "mask", "y_tokens", "video"))
    n_vis = g["n_vis"].tolist()
    Nt, P = mask.shape[1], 8
    lo = min(n_vis)
    assert y.shape[1] == Nt - lo and len(set(n_vis)) >= 3
    perm, rank, counts, flags = RR.index_prologue(mask, lo, max(n_vis))
    assert counts.tolist() == n_vis and not flags.any()
    # rows in front of a sample's own predictions must not be read: poison them
    yp = y.clone()
    for b, n in enumerate(n_vis):
        yp[b, :n - lo] = float("nan")
    out = RR.unembed(yp, x, mask, rank, lo, P)
    assert not torch.isnan(out).any()
    vis_pix = O.patches_to_video((~mask)[..., None].expand(-1, -1, 192).float(), 2, 3, 32, 32, P).bool()
    assert torch.equal(out[vis_pix], x[vis_pix]) and vis_pix.any() and (~vis_pix).any()
    assert torch.equal(out[~vis_pix].view(torch.int32), video[~vis_pix].view(torch.int32))
    assert torch.equal(out.view(torch.int32), video.view(torch.int32))


def test_attention_rows_with_full_lengths_is_the_dense_softmax():
    import engine_rows_restatement as R

    qkv = torch.randn(2, 9, 3 * 128, generator=torch.Generator().manual_seed(7))
    full = RR.attention_rows(qkv, [9, 9], 2)
    assert (full - R.attention_window(qkv, 2)).abs().max().item() <= 1e-12
    part = RR.attention_rows(qkv, [4, 10], 2)
    assert torch.isnan(part[0, 4:]).all() and torch.isnan(part[1]).all()  # (10 > N: nothing)
    alone = RR.attention_rows(qkv[:1, :4], [4], 2)
    assert torch.equal(part[0, :4], alone[0])
