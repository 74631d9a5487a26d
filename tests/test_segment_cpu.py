"""Spelke-object segmentation without a GPU: the definition of `cwm_segment_step` as the NumPy restatement states it (tests/segment_restatement.py) on a
hand-worked example, the package's torch composition (`segment_step` on CPU tensors) against the restatement, the selection rule, the direction table, and the
`segment_spelke_object` loop on CPU tensors.  Every input is exact in float32 (see the restatement's docstring), so every comparison is equality."""
import numpy as np
import pytest
import torch

import segment_restatement as SR
from counterfactualworldmodels_amd import config as C, segment_step as SS, segmentation, vmae

NAMES = ("segment", "votes", "cover", "stats", "seed_ref", "active", "passive", "picks")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and np.array_equal(a.view(np.int32), b.astype(np.float32).view(np.int32)) or (
            a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a).view(np.int32), np.nan_to_num(b.astype(np.float32)).view(np.int32)))
    return a.shape == b.shape and np.array_equal(a.astype(np.int64), b.astype(np.int64))


def compare(res, want, selection):
    for k in NAMES:
        got = getattr(res, k)
        if k in ("active", "passive", "picks") and not selection:
            assert got is None
            continue
        assert same(got.cpu().numpy(), want[k]), k


def both(flows, seeds, P, shape=None, **kw):
    """the torch composition on CPU tensors and the restatement, compared; returns the restatement's dict"""
    want = SR.step(flows, seeds, P, shape=shape, **kw)
    tk = dict(kw)
    if tk.get("keys") is not None:
        tk["keys"] = torch.from_numpy(np.asarray(tk["keys"], np.float32))
    tk.setdefault("min_seed_mag", 0.0)
    tk.setdefault("abs_thresh", 0.0)
    res = SS.segment_step(None if flows is None else torch.from_numpy(flows), torch.from_numpy(np.asarray(seeds, np.int32)), P, shape=shape, **tk)
    assert not res.segment.is_cuda
    compare(res, want, kw.get("k_active", 0) > 0)
    return want


def test_hand_worked_example():
    flows, seeds, kw = SR.hand_worked()
    want = both(flows, seeds, 8, **kw)
    assert want["stats"].tolist() == [[4, 192, 232, 1]]  # n_valid, area, n_candidates, seed_hit
    assert want["cover"][0].tolist() == [[.375, .375, 0], [.75, .75, 0], [.375, .375, 0]]
    assert np.isnan(want["seed_ref"][0, 2]) and want["seed_ref"][0, [0, 1, 3, 4]].tolist() == [0.9375, 1.875, 0.9375, 2.8125]
    seg = want["segment"][0].astype(bool)
    assert seg[4:20, 2:14].all() and seg.sum() == 192 and want["votes"][0, 3, 19] == 4 and not seg[2:10, 18:23].any()


def test_serpentine_and_spiral_are_reached_whole():
    m = SR.serpentine(24, 24)
    assert m.sum() == 300
    want = both(SR.flows_of(m, (1, 2)), [[0, 0]], 8, min_seed_mag=0.1, abs_thresh=1.0, vote_frac=1.0)
    assert want["stats"].tolist() == [[2, 300, 300, 1]]
    sp = SR.spiral(24, 24)
    assert SR.components(sp).max() == 1 and sp.sum() > 200
    want = both(SR.flows_of(sp, (4,)), [[0, 3]], 8, min_seed_mag=0.1, abs_thresh=1.0)
    assert want["stats"][0, 1] == sp.sum()


def test_blocks_that_touch_diagonally_are_two_components():
    m = SR.diagonal_pair(24, 24)
    want = both(SR.flows_of(m, (1, 1, 3)), [[3, 3]], 8, min_seed_mag=0.1, abs_thresh=1.0)
    assert want["stats"].tolist() == [[3, 36, 72, 1]] and not want["segment"][0, 8:14, 8:14].any()


def test_nan_inf_clamped_seeds_and_no_valid_sample():
    m = np.zeros((24, 24), bool)
    m[0:12, 0:12] = True
    f = SR.flows_of(m, (1, 2, 1, 4))
    f[0, 0, 2, 3, 1] = np.nan     # a NaN inside the seed cell of sample 1: that sample is not valid
    f[0, 1, 9, 9, 0] = np.nan     # a NaN pixel outside the seed cell: it does not vote in sample 0
    f[0, 0, 10, 10, 2] = np.inf   # an infinite magnitude votes
    want = both(f, [[-5, -7]], 8, min_seed_mag=0.5, abs_thresh=1.0, vote_frac=1.0)  # the seed clamps to (0, 0)
    assert want["stats"][0, 0] == 3 and np.isnan(want["seed_ref"][0, 1]) and want["votes"][0, 9, 9] == 2 and want["votes"][0, 10, 10] == 3
    assert want["segment"][0, 9, 9] == 0 and want["stats"][0, 1] == 143
    want = both(f, [[99, 99]], 8, min_seed_mag=0.5, abs_thresh=1.0)  # clamps to (23, 23): nothing moves there
    assert want["stats"].tolist() == [[0, 0, 0, 0]] and not want["votes"].any()
    f[0, 0, 0, 0, :] = np.inf  # an infinite seed reference is valid; rel_thresh * inf = inf: only infinite pixels vote
    want = both(f, [[0, 0]], 8, min_seed_mag=0.5, abs_thresh=1.0, vote_frac=1.0)
    assert want["stats"][0, 0] == 3 and want["stats"][0, 1] == 1 and want["segment"][0, 0, 0] == 1  # (sample 1 keeps its NaN)


def test_init_step():
    want = both(None, [[10, 5], [40, -1]], 8, shape=(2, 24, 24), k_active=3, k_passive=2)
    assert want["picks"].tolist() == [[9 + 3, -1, -1, -1, -1], [9 + 6, -1, -1, -1, -1]]
    assert want["active"].sum(1).tolist() == [8, 8] and want["passive"][:, 9:].all() and not want["passive"][:, :9].any()
    assert not want["stats"].any() and not want["segment"].any()


def ring_case():
    """32 x 32, P = 4: an 8 x 8 grid; the object fills cells (2..4, 2..4) and half of column 5 of those rows"""
    m = np.zeros((32, 32), bool)
    m[8:20, 8:22] = True
    return SR.flows_of(m, (1, 2, 3)), [[9, 9]]


def test_selection_order_ties_nan_keys_and_short_inside_set():
    f, seeds = ring_case()
    kw = dict(min_seed_mag=0.1, abs_thresh=1.0)
    want = both(f, seeds, 4, k_active=4, k_passive=5, **kw)  # no keys: index order
    inside = [8 * r + c for r in (2, 3, 4) for c in (2, 3, 4)]
    assert want["picks"][0, :4].tolist() == [64 + c for c in [18, 19, 20, 26]] and want["picks"][0, 4:].tolist() == [64 + c for c in (9, 10, 11, 12, 13)]
    want = both(f, seeds, 4, k_active=12, k_passive=0, **kw)  # k_active - 1 = 11 > the 8 other inside cells
    assert want["picks"][0].tolist() == [64 + 18] + [64 + c for c in inside if c != 18] + [-1] * 3
    keys = np.zeros((1, 2, 64), np.float32)
    keys[0, 0, 36], keys[0, 0, 27], keys[0, 0, 20], keys[0, 0, 19], keys[0, 0, 18] = np.nan, 2.0, 2.0, -0.0, 9.0  # (the seed cell's key is not looked at)
    keys[0, 1, 9], keys[0, 1, 14], keys[0, 1, 41] = -1.0, np.nan, 5.0
    want = both(f, seeds, 4, k_active=5, k_passive=3, keys=keys, **kw)
    assert want["picks"][0].tolist() == [64 + c for c in (18, 36, 20, 27, 19, 14, 41, 10)]
    half = both(f, seeds, 4, k_active=20, k_passive=0, inside_frac=0.5, **kw)  # the half-covered column counts at 0.5
    assert sorted(half["picks"][0][half["picks"][0] >= 0].tolist()) == [64 + c for c in sorted(inside + [21, 29, 37])]


@pytest.mark.parametrize("radius,count", [(1, 18), (2, 18 + 26), (9, 64 - 12)])
def test_ring_radius(radius, count):
    f, seeds = ring_case()
    want = both(f, seeds, 4, k_active=1, k_passive=64, ring_radius=radius, min_seed_mag=0.1, abs_thresh=1.0)
    ring = want["picks"][0, 1:]
    assert (ring >= 0).sum() == count and (want["passive"][0, 64:] == 0).sum() == count


def test_directions_and_the_direction_test():
    assert SS.directions(8) == [(0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, -1), (-1, 1)]
    assert SS.directions(11, 2)[8:] == [(0, 2), (2, 0), (0, -2)] and SS.directions(3) == SS.directions(8)[:3]
    m = np.zeros((24, 24), bool)
    m[4:20, 4:20] = True
    f = SR.flows_of(m, (1, 1, 1))              # (0.75, 1.0) k everywhere on the block ...
    f[0, :, 12:20, 4:20, 1] *= -1              # ... sample 1 moves the lower half the other way
    dirs = [(8, 6)] * 3                        # (dy, dx): u dx + v dy = 0.75 * 6 + 1.0 * 8 = 12.5; |d| = 10, m = 1.25: the cosine is exactly 1
    want = both(f, [[5, 5]], 8, dirs=dirs, cos_min=1.0, vote_frac=1.0, min_seed_mag=0.1, abs_thresh=1.0)
    assert want["stats"].tolist() == [[3, 128, 128, 1]] and want["votes"][0, 15, 15] == 2
    want = both(f, [[5, 5]], 8, dirs=dirs, cos_min=-1.0, vote_frac=1.0, min_seed_mag=0.1, abs_thresh=1.0)
    assert want["stats"][0, 1] == 256


# ---- the loop on CPU tensors.  Prompts are built on the GPU only, so here the counterfactual driver itself is the stub: it stands for the predictor and the flow
# model together and returns a fixed table of exact flows in which a known object moves along direction s ----
TINY = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)


def object_table(S, P=8, H=32, W=32):
    """[1,2,H,W,S]: the object (rows 8-23, cols 8-19) moves 8 px along an axis direction, (6, 8) px along a diagonal one: magnitudes 8 and 10, exact"""
    obj = np.zeros((H, W), bool)
    obj[8:24, 8:20] = True
    f = np.zeros((1, 2, H, W, S), np.float32)
    for s, (dy, dx) in enumerate(SS.directions(S)):
        u, v = (6.0 * dx, 8.0 * dy) if dx and dy else (8.0 * dx, 8.0 * dy)
        f[0, 0, :, :, s], f[0, 1, :, :, s] = obj * u, obj * v
    return obj, f


@pytest.mark.parametrize("sample", [False, True])
def test_segment_spelke_object_on_cpu_tensors(sample):
    S = 5
    obj, table = object_table(S)
    G = segmentation.FlowGenerator(predictor=vmae.PretrainVisionTransformer(TINY), imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
    x = torch.zeros((1, 2, 3, 32, 32))
    calls = []

    def driver(xx, active_patches, passive_patches=None, shifts=None, num_samples=8, **kw):
        calls.append((active_patches[..., 0].clone(), passive_patches[..., 0].clone(), list(shifts)))
        assert active_patches.shape == (1, 32, S) and kw["fix_passive"] is True
        G.x = xx
        return None, torch.from_numpy(table).permute(0, 4, 1, 2, 3).reshape(S, 1, 2, 32, 32)

    G.predict_counterfactual_videos_and_flows = driver
    seeds = torch.tensor([[12, 10]])
    state = torch.get_rng_state()
    gen = torch.Generator().manual_seed(3)
    seg, frac, trace = G.segment_spelke_object(x, seeds, num_iters=3, num_samples=S, k_active=3, k_passive=4, sample=sample, generator=gen, return_trace=True,
                                               min_seed_mag=1.0, abs_thresh=1.0)
    assert torch.equal(torch.get_rng_state(), state) and seeds.tolist() == [[12, 10]]
    assert np.array_equal(seg[0].numpy(), obj) and np.array_equal(frac[0].numpy(), obj.astype(np.float32)) and len(calls) == len(trace) == 3
    # by hand: the restatement with the same keys
    gen = torch.Generator().manual_seed(3)
    dirs = [(8 * dy, 8 * dx) for dy, dx in SS.directions(S)]
    want = SR.step(None, seeds.numpy(), 8, shape=(1, 32, 32), k_active=3, k_passive=4)
    for it in range(3):
        act, pas, shifts = calls[it]
        assert shifts == SS.directions(S)
        assert np.array_equal(act.numpy(), want["active"].astype(bool)) and np.array_equal(pas.numpy(), want["passive"].astype(bool)), it
        keys = torch.rand((1, 2, 16), generator=gen).numpy() if sample else None
        want = SR.step(table, seeds.numpy(), 8, min_seed_mag=1.0, abs_thresh=1.0, dirs=dirs, k_active=3, k_passive=4, keys=keys)
        compare(trace[it][0], want, True)
        if it:  # the active picks lie inside the object, the passive ones in its ring
            cells = (trace[it][0].picks[0] - 16).tolist()
            assert cells[0] == 5 and set(cells[:3]) - {-17} <= {5, 9} and all(c not in (5, 6, 9, 10) and c >= 0 for c in cells[3:])
