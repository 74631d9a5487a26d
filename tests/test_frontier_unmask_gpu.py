"""Frontier unmasking end to end on a real MI355X, with a tiny predictor of random weights (32 x 32, patch 8: a 4 x 4 grid, T = 2):

  * `frontier_unmask` on the fused path (forward to tokens + one `cwm_unmask_step` per step, no read-back in the loop) against the same search composed by
    hand from the public pieces -- `get_error_on_target_region` for the map and for the mean, the restatement's selection (tests/unmask_restatement.py) -- on
    the same device: picks, masks and errors are EQUAL, bit for bit, for 3 steps, k in {1, 3}, top and race mode;
  * against the wrapper's own composed path (a custom error_func sends it through `predict`, `error_func` and `avg_pool3d`): picks and masks equal; the errors
    are then sums of the same fp32 terms in another order, so they agree to (C P^2 + 2) 2^-24 for the patch values plus (T h w + 2) 2^-24 for the mean,
    relative (the bounds of tests/patch_error_restatement.py);
  * `masking.patch_distance_transform` / `patches_adjacent_to_visible` on CUDA tensors against the reference's results (tests/golden/mask_morphology.npz);
  * `greedy_unmask(radius=1)`: every step's candidates are the frontier, and the pick is the brute-force minimum over it."""
import os

import numpy as np
import pytest
import torch

import patch_error_restatement as PR
import unmask_restatement as UR
from counterfactualworldmodels_amd import config as C, masking, prediction, synthetic as S, vmae

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mask_morphology.npz")
TINY = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
B, T, h, w, n = 3, 2, 4, 4, 16


@pytest.fixture(scope="module")
def tiny():
    m = vmae.PretrainVisionTransformer(TINY, mode="parity")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(TINY, 3).items()})
    m = m.to("cuda:0").eval()
    G = prediction.PredictorBasedGenerator(predictor=m, imagenet_normalize_inputs=True, temporal_dim=2)
    x = torch.from_numpy(S.synthetic_frames(B, TINY, 3)).cuda()
    mask = torch.zeros((B, T * n), dtype=torch.bool)
    mask[:, n:] = True
    for b, c in enumerate((0, 15, 6)):  # one visible cell per row: two corners and an inner cell
        mask[b, n + c] = False
    return G, x, mask.cuda()


def no_video(G):
    def refuse(*a, **k):
        raise AssertionError("the composed path ran")
    G.predict = refuse
    return G


def by_hand(G, x, mask, steps, k, radius, gen=None):
    """the search from the public pieces, the selection on the CPU"""
    cur = mask.clone()
    region_mask = torch.ones_like(mask)
    region_mask[:, n:] = False
    thr = UR.threshold(h, w, radius)
    picks, errors = [], []
    for _ in range(steps):
        errors.append(G.get_error_on_target_region(x, cur.clone(), region_mask))
        emap = G.get_error_on_target_region(x, cur.clone(), region_mask, average_error=False)
        e = None if gen is None else torch.empty((B, n), device="cuda").exponential_(generator=gen).cpu()
        st = UR.step(cur.cpu(), emap.cpu(), T, h, w, 1, k, thr, e)
        picks.append(st["picks"].long())
        cur = st["mask_out"].cuda()
    return cur, torch.stack(picks, 1).cuda(), torch.stack(errors, 1)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("sample", [False, True])
def test_fused_equals_the_search_composed_by_hand(tiny, k, sample):
    G, x, mask = tiny
    F = no_video(prediction.PredictorBasedGenerator(predictor=G.predictor, imagenet_normalize_inputs=True, temporal_dim=2))
    gen = (lambda: torch.Generator(device="cuda").manual_seed(17)) if sample else (lambda: None)
    start = mask.clone()
    rng = torch.get_rng_state()
    out, picks, errors, trace = F.frontier_unmask(x, mask, num_steps=3, num_reveal=k, radius=1, sample=sample, generator=gen(), return_trace=True)
    assert torch.equal(mask, start) and torch.equal(rng, torch.get_rng_state())
    assert picks.is_cuda and picks.dtype == torch.int64 and tuple(picks.shape) == (B, 3, k) and tuple(errors.shape) == (B, 3)
    want_out, want_picks, want_errors = by_hand(G, x, mask, 3, k, 1, gen())
    print("picks", picks.tolist(), "errors", errors.tolist())
    assert torch.equal(picks, want_picks) and torch.equal(out, want_out)
    assert torch.equal(errors.view(torch.int32), want_errors.view(torch.int32))
    assert out.sum(1).tolist() == [n - 1 - 3 * k] * B
    # the trace's frontier is the restatement's for the mask of each step
    cur = start.cpu()
    for s, (emap, front) in enumerate(trace):
        assert torch.equal(front.view(B, n).cpu(), UR.frontier(cur[:, n:], h, w, UR.threshold(h, w, 1)))
        cur = cur.clone()
        for b in range(B):
            cur[b, picks[b, s].cpu()] = False


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("sample", [False, True])
def test_fused_equals_the_composed_path(tiny, k, sample):
    G, x, mask = tiny
    F = no_video(prediction.PredictorBasedGenerator(predictor=G.predictor, imagenet_normalize_inputs=True, temporal_dim=2))
    Cp = prediction.PredictorBasedGenerator(predictor=G.predictor, imagenet_normalize_inputs=True, temporal_dim=2,
                                            error_func=lambda a, b: (a - b) ** 2)  # MSE, but not an nn.MSELoss: composed
    gen = (lambda: torch.Generator(device="cuda").manual_seed(29)) if sample else (lambda: None)
    fo, fp, fe = F.frontier_unmask(x, mask, num_steps=3, num_reveal=k, radius=1, sample=sample, generator=gen())
    co, cp, ce = Cp.frontier_unmask(x, mask, num_steps=3, num_reveal=k, radius=1, sample=sample, generator=gen())
    assert torch.equal(fp, cp) and torch.equal(fo, co)
    rel = PR.map_bound(3, 8) + PR.mean_bound(3, 8, T * n)
    err = (fe.double() - ce.double()).abs()
    print("errors: fused against composed, max relative difference %.3e (bound %.3e)" % ((err / ce.double().abs()).max().item(), rel))
    assert bool((err <= rel * ce.double().abs()).all())
    # radius=None and a target of its own take the same two paths
    tgt = x.flip(0).contiguous()
    fo, fp, fe = F.frontier_unmask(x, mask, num_steps=2, num_reveal=k, radius=None, target=tgt)
    co, cp, ce = Cp.frontier_unmask(x, mask, num_steps=2, num_reveal=k, radius=None, target=tgt)
    assert torch.equal(fp, cp) and torch.equal(fo, co)
    assert bool(((fe.double() - ce.double()).abs() <= rel * ce.double().abs()).all())


def test_distance_transform_on_the_device_equals_the_reference():
    g = np.load(GOLDEN)
    for hh, ww in g["grids"].tolist():
        k = "g%dx%d_" % (hh, ww)
        m = torch.from_numpy(np.unpackbits(g[k + "mask"])[: 6 * hh * ww].astype(np.bool_)).view(2, 3, hh, ww).cuda()
        for name, sm in (("dist_self", True), ("dist_noself", False)):
            got = masking.patch_distance_transform(m, self_mask=sm)
            assert got.is_cuda and np.array_equal(got.cpu().numpy().view(np.uint32), g[k + name].view(np.uint32)), (hh, ww, name)
        for r in (1, 2, 3):
            want = np.unpackbits(g[k + "adj_r%d" % r])[: 6 * hh * ww].astype(np.bool_).reshape(2, 3, hh, ww)
            assert np.array_equal(masking.patches_adjacent_to_visible(m, radius=r).cpu().numpy(), want), (hh, ww, r)
        assert np.array_equal(masking.patches_adjacent_to_visible(m, radius=0).cpu().numpy().view(np.uint32), g[k + "adj_r0"].view(np.uint32)), (hh, ww)
    # a non-contiguous view, and a grid over the device limit
    m = torch.rand((2, 2, 6, 10), generator=torch.Generator().manual_seed(1)) < 0.8
    assert torch.equal(masking.patch_distance_transform(m.cuda().transpose(0, 1)).cpu(), masking.patch_distance_transform(m.transpose(0, 1)))
    with pytest.raises(ValueError, match="4096"):
        masking.patch_distance_transform(torch.ones((1, 1, 65, 64), dtype=torch.bool, device="cuda"))


def test_greedy_unmask_with_a_radius_searches_the_frontier(tiny):
    G, x, mask = tiny
    D = no_video(prediction.PredictorBasedGenerator(predictor=G.predictor, imagenet_normalize_inputs=True, temporal_dim=2))
    x1, m1 = x[:1], mask[2:3]  # the row whose visible cell is inside the grid
    out, picks, scores, trace = D.greedy_unmask(x1, m1, num_steps=2, radius=1, return_scores=True)
    region_mask = torch.ones_like(m1)
    region_mask[:, n:] = False
    cur = m1.clone()
    for step, (cand, s) in enumerate(trace):
        front = UR.frontier(cur[:, n:].cpu(), h, w, UR.threshold(h, w, 1))
        assert cand.tolist() == (n + torch.nonzero(front[0]).view(-1)).tolist() and 0 < len(cand) < int(cur[:, n:].sum())
        rows = cur.expand(len(cand), -1).clone()
        rows[torch.arange(len(cand)), torch.from_numpy(cand).cuda()] = False
        direct = G.get_error_on_target_region(x1.expand(len(cand), -1, -1, -1, -1), rows, region_mask.expand(len(cand), -1))
        assert np.array_equal(direct.cpu().numpy(), s)
        assert picks[step] == cand[int(np.flatnonzero(s == s.min())[0])] and scores[step] == s.min()
        cur[0, picks[step]] = False
    assert torch.equal(cur, out)
    # radius=None: the parent's search, over all 15 masked cells
    _, _, _, trace = D.greedy_unmask(x1, m1, num_steps=1, return_scores=True)
    assert trace[0][0].tolist() == [t for t in range(n, 2 * n) if bool(m1[0, t])]
