"""Frontier unmasking without a GPU: the selection rule of `cwm_unmask_step` as restated in tests/unmask_restatement.py and as `frontier_unmask` applies it in
torch (`PredictorBasedGenerator._select_reveal`), the exponential race's distribution, and `frontier_unmask` on CPU tensors with a stub predictor against a
hand-worked example."""
import numpy as np
import pytest
import torch
from torch import nn

import unmask_restatement as UR
from counterfactualworldmodels_amd import prediction

SELECT = prediction.PredictorBasedGenerator._select_reveal
NAN = float("nan")


def both(err, fm, front, k, e=None):
    """the restatement's picks, after checking that the wrapper's torch rule gives the same"""
    want = UR.select(err, fm, front, k, e)
    got = SELECT(err, fm, front, k, e)
    assert torch.equal(got, want), (got, want)
    return want.tolist()


def test_fill_rule_ties_and_nan():
    err = torch.tensor([[5.0, 1.0, 9.0, 1.0, 7.0, 3.0], [2.0, 2.0, 2.0, 2.0, 2.0, 2.0]])
    fm = torch.tensor([[1, 1, 1, 1, 0, 1], [1, 1, 0, 1, 1, 1]], dtype=torch.bool)
    front = torch.tensor([[0, 1, 0, 1, 0, 0], [0, 0, 0, 1, 1, 0]], dtype=torch.bool)
    # row 0: the frontier {1, 3} ties at 1.0 -> index order, then the rest by error: 2 (9), 0 (5), 5 (3); cell 4 is visible and never picked, whatever its error
    # row 1: all equal: frontier 3, 4, then 0, 1, 5
    assert both(err, fm, front, 5) == [[1, 3, 2, 0, 5], [3, 4, 0, 1, 5]]
    assert both(err, fm, front, 1) == [[1], [3]]
    # more picks than masked cells: -1
    assert both(err, fm, front, 6) == [[1, 3, 2, 0, 5, -1], [3, 4, 0, 1, 5, -1]]
    # a NaN ranks above every number, inf included, within its class; -0 and +0 tie
    err = torch.tensor([[1.0, NAN, float("inf"), -0.0, 0.0, NAN]])
    fm = torch.ones((1, 6), dtype=torch.bool)
    front = torch.tensor([[1, 1, 1, 1, 1, 0]], dtype=torch.bool)
    assert both(err, fm, front, 6) == [[1, 2, 0, 3, 4, 5]]
    assert both(err, fm, fm, 6) == [[1, 5, 2, 0, 3, 4]]


def test_race_ordering_with_a_given_e():
    err = torch.tensor([[4.0, 1.0, 2.0, -3.0, 0.5]])
    e = torch.tensor([[8.0, 0.5, 0.25, 1.0, 0.125]])
    fm = torch.ones((1, 5), dtype=torch.bool)
    # keys 0.5, 2, 8, max(-3, 0) / 1 = 0, 4
    assert both(err, fm, fm, 5, e) == [[2, 4, 1, 0, 3]]
    # the frontier still goes first
    front = torch.tensor([[1, 0, 0, 1, 0]], dtype=torch.bool)
    assert both(err, fm, front, 3, e) == [[0, 3, 2]]
    # a NaN error stays NaN through the clamp and wins
    err[0, 1] = NAN
    assert both(err, fm, fm, 2, e) == [[1, 2]]


def test_the_race_draws_in_proportion_to_the_error():
    """First picks of 20 000 races over weights 1:2:3:4 come out at w / sum(w) to within 0.02 (a Bernoulli frequency at N = 20 000 has a standard error of at
    most 0.0035), and the second pick, given the first, in proportion to the remaining weights."""
    N = 20000
    g = torch.Generator().manual_seed(1234)
    w = torch.tensor([1.0, 2.0, 3.0, 4.0])
    err = w[None].expand(N, 4).contiguous()
    e = torch.empty((N, 4)).exponential_(generator=g)
    fm = torch.ones((N, 4), dtype=torch.bool)
    picks = SELECT(err, fm, fm, 2, e)
    first = torch.bincount(picks[:, 0], minlength=4).double() / N
    print("first-pick frequencies", first.tolist())
    assert (first - (w / w.sum()).double()).abs().max() <= 0.02
    assert (picks[:, 0] != picks[:, 1]).all()
    after3 = picks[picks[:, 0] == 3, 1]  # weight 4 went first: the rest race at 1:2:3
    second = torch.bincount(after3, minlength=4).double()[:3] / len(after3)
    assert (second - torch.tensor([1, 2, 3]).double() / 6).abs().max() <= 0.02 * (N / len(after3)) ** 0.5
    # the restatement's rule on a slice of the same draws
    assert torch.equal(UR.select(err[:200], fm[:200], fm[:200], 2, e[:200]), picks[:200])


class ZeroPredictor(nn.Module):
    """predicts black at every masked patch and the input at the visible ones: the error of a patch is its own energy until it is revealed"""
    patch_size = (1, 8, 8)
    image_size = (32, 32)
    num_frames = 2
    t_dim, c_dim = 2, 1

    def __init__(self):
        super().__init__()
        self.calls = 0

    def forward(self, x, mask, *a, **k):  # x [B,C,T,H,W]
        self.calls += 1
        B, C, T, H, W = x.shape
        keep = (~mask.view(B, T, 4, 4)).repeat_interleave(8, 2).repeat_interleave(8, 3)
        return (x.transpose(1, 2) * keep[:, :, None]).contiguous()


def movie(B=2):
    """frame 1, patch c: every pixel (c + 1) / 16 in all three channels -> the error of a masked patch is 3 ((c + 1) / 16)^2, growing with c"""
    x = torch.zeros((B, 2, 3, 32, 32))
    v = ((torch.arange(16) + 1).float() / 16).view(4, 4).repeat_interleave(8, 0).repeat_interleave(8, 1)
    x[:, 1] = v
    return x


def test_frontier_unmask_on_cpu_tensors_follows_the_hand_worked_example():
    """4 x 4 grid, unit (4-1)//2 = 1 patch, radius 1: the frontier is the masked 8-neighbourhood of the visible cells.
    row 0 starts with (0,0) visible:  frontier {1, 4, 5} -> 5, 4;  then {1, 2, 6, 8, 9, 10} -> 10, 9;  then {1, 2, 6, 7, 8, 11, 12, 13, 14, 15} -> 15, 14
    row 1 starts with (3,3) visible:  frontier {10, 11, 14} -> 14, 11;  then the neighbours of {11, 14, 15}: {6, 7, 9, 10, 13} -> 13, 10;  then those of
    {10, 11, 13, 14, 15}: {5, 6, 7, 8, 9, 12} -> 12, 9"""
    G = prediction.PredictorBasedGenerator(predictor=ZeroPredictor(), temporal_dim=2)
    x = movie()
    mask = torch.zeros((2, 32), dtype=torch.bool)
    mask[:, 16:] = True
    mask[0, 16 + 0] = False
    mask[1, 16 + 15] = False
    start = mask.clone()
    out, picks, errors, trace = G.frontier_unmask(x, mask, num_steps=3, num_reveal=2, radius=1, frame=-1, return_trace=True)
    assert torch.equal(mask, start)  # the argument is left alone
    assert picks.dtype == torch.int64 and (picks - 16).tolist() == [[[5, 4], [10, 9], [15, 14]], [[14, 11], [13, 10], [12, 9]]]
    want = start.clone()
    for b in range(2):
        want[b, picks[b].reshape(-1)] = False
    assert torch.equal(out, want) and out.sum(1).tolist() == [9, 9]
    assert G.predictor.calls == 3  # one forward per step for the whole batch
    # errors: the mean over the 16 patches of frame 1 of the energy still masked before each reveal; (64 + 16 + 2) fp32 roundings of non-negative terms
    en = 3 * ((torch.arange(16) + 1).double() / 16) ** 2
    m = start[:, 16:].clone()
    for s in range(3):
        for b in range(2):
            assert abs(errors[b, s].item() - (en * m[b]).sum().item() / 16) <= 82 * 2.0 ** -24 * (en * m[b]).sum().item() / 16, (b, s)
            m[b, picks[b, s] - 16] = False
    assert len(trace) == 3 and tuple(trace[0][0].shape) == (2, 2, 4, 4) and trace[0][1].dtype == torch.bool
    assert torch.nonzero(trace[0][1][0].view(-1)).view(-1).tolist() == [1, 4, 5] and torch.nonzero(trace[1][1][1].view(-1)).view(-1).tolist() == [6, 7, 9, 10, 13]
    # without a radius the largest errors go first, wherever they are
    _, picks, _ = G.frontier_unmask(x, start, num_steps=1, num_reveal=3, radius=None)
    assert (picks - 16).tolist() == [[[15, 14, 13]], [[14, 13, 12]]]
    # a frame with nothing visible: every cell is on the frontier (the reference's distance is 0 there)
    full = torch.zeros((2, 32), dtype=torch.bool)
    full[:, 16:] = True
    _, picks, _ = G.frontier_unmask(x, full, num_reveal=2, radius=1)
    assert (picks - 16).tolist() == [[[15, 14]], [[15, 14]]]
    # a frontier smaller than num_reveal fills up from the other masked cells: {1, 4, 5}, then 15
    _, picks, _ = G.frontier_unmask(x[:1], start[:1], num_reveal=4, radius=1)
    assert (picks - 16).tolist() == [[[5, 4, 1, 15]]]


def test_frontier_unmask_sampling_and_refusals():
    G = prediction.PredictorBasedGenerator(predictor=ZeroPredictor(), temporal_dim=2)
    x = movie()
    mask = torch.zeros((2, 32), dtype=torch.bool)
    mask[:, 16:] = True
    a = G.frontier_unmask(x, mask, num_steps=2, num_reveal=3, radius=None, sample=True, generator=torch.Generator().manual_seed(5))
    b = G.frontier_unmask(x, mask, num_steps=2, num_reveal=3, radius=None, sample=True, generator=torch.Generator().manual_seed(5))
    c = G.frontier_unmask(x, mask, num_steps=2, num_reveal=3, radius=None, sample=True, generator=torch.Generator().manual_seed(6))
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]) and not torch.equal(a[1], c[1])
    assert all(len(set(row.reshape(-1).tolist())) == 6 for row in a[1])  # without replacement
    ragged = mask.clone()
    ragged[0, 20] = False
    with pytest.raises(ValueError, match="same masked count"):
        G.frontier_unmask(x, ragged)
    with pytest.raises(ValueError, match="need 18 masked patches"):
        G.frontier_unmask(x, mask, num_steps=6, num_reveal=3)
    with pytest.raises(ValueError, match="frame must be an index"):
        G.frontier_unmask(x, mask, frame=None)
