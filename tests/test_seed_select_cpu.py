"""Seed selection without a GPU: the package's torch composition (`select_seeds` on CPU tensors) against the NumPy restatement of the definition
(tests/seed_select_restatement.py) on every case of its list, its agreement with the orders the package already has (`draw_seed_cells`, `select_reveal`), the
argument refusals, `predict_keypoints` on a stub keypoint module, and the new keywords of `segment_scene` on the stub driver of tests/test_segment_merge_cpu.py."""
import numpy as np
import pytest
import torch

import seed_select_restatement as R
from counterfactualworldmodels_amd import masking, seed_select as SS, segment_merge as SM
from test_segment_merge_cpu import SCENE_KW, stub_generator, two_object_table

CASES = R.cases()


def as_dict(sel):
    return {k: getattr(sel, k).cpu().numpy() for k in SS.SeedSelection.__slots__}


def tensors(kw):
    """the keyword arguments of the restatement as those of select_seeds"""
    kw = dict(kw)
    m, P, K = torch.from_numpy(kw.pop("map")), kw.pop("P"), kw.pop("K")
    for k in ("free", "e", "prior"):
        if kw.get(k) is not None:
            kw[k] = torch.from_numpy(np.asarray(kw[k]))
    return m, K, P, kw


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_torch_composition_equals_the_restatement(name, kw):
    m, K, P, rest = tensors(kw)
    R.assert_equal(as_dict(SS.select_seeds(m, K, P, **rest)), R.want(name, kw), name)


def test_strided_maps_and_a_squeezed_channel():
    name, kw = next(c for c in CASES if c[0] == "grid_5x7_P4")
    m, K, P, rest = tensors(kw)
    B, H, W = m.shape
    chan = torch.rand(B, 3, H, W)
    chan[:, 1] = m
    pad = torch.rand(B, H, W + 8)
    pad[:, :, :W] = m
    for view in (chan[:, 1], pad[:, :, :W], m[:, None]):
        R.assert_equal(as_dict(SS.select_seeds(view, K, P, **rest)), R.want(name, kw), name)
    R.assert_equal(as_dict(SS.select_seeds(m, K, P, shape=(H, W), **rest)), R.want(name, kw), name)


def test_radius_0_is_the_order_the_package_already_has():
    g = torch.Generator().manual_seed(3)
    p = torch.rand(3, 5, 7, generator=g)
    p[0, 1, 2:5] = p[0, 0, 0]  # ties
    free = torch.rand(3, 35, generator=g) < 0.7
    for k in (1, 9, 40):
        top = SS.select_seeds(p, k, 4, radius=0, free=free, cells=True)
        assert torch.equal(top.cells.long(), masking.select_reveal(p.reshape(3, 35), free, torch.zeros_like(free), k))
        assert torch.equal(top.seeds, SM.cell_centres(top.cells.long(), 7, 4))
        e = torch.empty((3, 35)).exponential_(generator=torch.Generator().manual_seed(k))
        race = SS.select_seeds(p, k, 4, radius=0, free=free, e=e, cells=True)
        assert torch.equal(race.cells.long(), SM.draw_seed_cells(p.reshape(3, 35), free, k, torch.Generator().manual_seed(k)))


def test_refusals():
    m = torch.zeros((2, 16, 24))
    for kw, match in ((dict(P=5), "P = 5"), (dict(k=0), "k = 0"), (dict(k=65), "k = 65"), (dict(radius=-1), "radius"), (dict(radius=65), "radius"),
                      (dict(abs_thresh=float("nan")), "abs_thresh"), (dict(rel_thresh=float("inf")), "rel_thresh"), (dict(free=torch.ones(2, 5)), "free"),
                      (dict(e=torch.ones(2, 5)), "e must"), (dict(prior=torch.zeros((2, 65), dtype=torch.int32)), "prior"), (dict(shape=(32, 32)), "map must be"),
                      (dict(shape=(16, 24), cells=True), "map must be")):
        args = dict(k=4, P=4)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            SS.select_seeds(m, args.pop("k"), args.pop("P"), **args)
    with pytest.raises(ValueError, match="do not divide"):
        SS.select_seeds(torch.zeros((1, 6, 6)), 2, 4)  # 6 x 6 cells need cells=True (or shape=)
    with pytest.raises(ValueError, match=r"map must be \[B,H,W\]"):
        SS.select_seeds(torch.zeros((6, 6)), 2, 4)
    with pytest.raises(ValueError, match="4096 patches"):
        SS.select_seeds(torch.zeros((1, 65, 64)), 2, 4, cells=True)
    assert SS.select_seeds(torch.zeros((1, 6, 6)), 2, 4, cells=True).seeds.tolist() == [[[2, 2], [2, 10]]]
    assert SS.select_seeds(torch.zeros((1, 6, 6)), 2, 4, shape=(24, 24), radius=0).cells.tolist() == [[0, 1]]


class Bumps(torch.nn.Module):
    """a keypoint module whose map [B,T-1,1,H,W] has known bumps: logits of -4 with single higher pixels; which set of bumps a movie gets is read off its first
    pixel (the generator asks for the map one movie at a time)"""
    POINTS = [[(21, 9, 3.0), (5, 30, 1.0), (14, 15, 2.0)], [(2, 2, 1.5), (29, 29, 2.5)]]  # (y, x, logit) per row

    def forward(self, x):
        out = torch.full((x.shape[0], x.shape[1] - 1, 1) + tuple(x.shape[-2:]), -4.0)
        for b in range(x.shape[0]):
            for y, xx, v in self.POINTS[int(x[b, 0, 0, 0, 0] > 0.5)]:
                out[b, 0, 0, y, xx] = v
        return out


def test_predict_keypoints_returns_the_bumps_in_order_of_height():
    from test_motion_sampling_cpu import tiny_generator

    G = tiny_generator(keypoint_predictor=Bumps())
    x = torch.rand(2, 2, 3, 32, 32)
    x[0, 0, 0, 0, 0], x[1, 0, 0, 0, 0] = 0.0, 1.0
    points, values = G.predict_keypoints(x, num_points=4, radius=0)
    assert points.dtype == torch.int32 and points.tolist() == [[[21, 9], [14, 15], [5, 30], [-1, -1]], [[29, 29], [2, 2], [-1, -1], [-1, -1]]]
    dist = SM.keypoints_distribution(G, x)
    assert values[0, :3].tolist() == [float(dist[0, 21, 9]), float(dist[0, 14, 15]), float(dist[0, 5, 30])] and values[0, 0] == 1.0 and values[:, 3].tolist() == [0.0, 0.0]
    # row 0 on the 8-pixel grid: the bumps lie in cells (2, 1), (1, 1) and (0, 3); radius 1 drops the middle one, which touches the highest
    assert G.predict_keypoints(x, num_points=4, radius=1)[0].tolist() == [[[21, 9], [5, 30], [-1, -1], [-1, -1]], [[29, 29], [2, 2], [-1, -1], [-1, -1]]]
    with pytest.raises(ValueError, match="keypoint_predictor"):
        tiny_generator().predict_keypoints(x)


def test_segment_scene_seed_keywords():
    a, b, table = two_object_table()
    G = stub_generator(table, [])
    x = torch.zeros((1, 2, 3, 32, 32))
    with pytest.raises(ValueError, match="seed_mode"):
        G.segment_scene(x, num_seeds=2, seed_mode="top", **SCENE_KW)
    with pytest.raises(ValueError, match="keypoint_predictor"):
        G.segment_scene(x, num_seeds=2, seed_distribution="keypoints", **SCENE_KW)
    with pytest.raises(ValueError, match="seed_radius"):
        G.segment_scene(x, num_seeds=2, seed_radius=65, **SCENE_KW)
    with pytest.raises(ValueError, match="seed_distribution"):
        G.segment_scene(x, num_seeds=2, seed_distribution="movability", **SCENE_KW)
    # the defaults are the draw there was before: the same seeds from the same generator state
    old = G.segment_scene(x, num_seeds=3, num_rounds=2, generator=torch.Generator().manual_seed(5), **SCENE_KW)
    new = G.segment_scene(x, num_seeds=3, num_rounds=2, generator=torch.Generator().manual_seed(5), seed_mode="sample", seed_radius=0, seed_rel_thresh=0., **SCENE_KW)
    assert torch.equal(old.seeds, new.seeds) and torch.equal(old.labels, new.labels)
    cells = SM.draw_seed_cells(torch.ones((1, 16)), torch.ones((1, 16), dtype=torch.bool), 3, torch.Generator().manual_seed(5))
    assert torch.equal(old.seeds[:, :3], SM.cell_centres(cells, 4, 8))
    # peaks of a pixel map with one bump on either object and one on the background: the seeds are the bump pixels, highest first, and nothing is drawn
    pix = torch.zeros((1, 32, 32))
    pix[0, 3, 5], pix[0, 22, 30], pix[0, 27, 2] = 3.0, 2.0, 1.0
    state = torch.get_rng_state()
    gen = torch.Generator().manual_seed(9)
    before = gen.get_state()
    out = G.segment_scene(x, num_seeds=3, num_rounds=2, seed_distribution=pix, seed_mode="peaks", seed_radius=1, seed_rel_thresh=0.1, generator=gen, **SCENE_KW)
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(gen.get_state(), before)
    assert out.seeds[0, :3].tolist() == [[3, 5], [22, 30], [27, 2]] and out.num_labels.tolist() == [2]
    assert out.seeds[0, 3:].tolist() == [[-1, -1]] * 3  # round 1: A and B are covered, the third bump is a prior seed, the rest lies below the threshold
    # a callable gives the map; without a threshold round 1 takes plateau cells that are free and more than seed_radius from every earlier seed
    out = G.segment_scene(x, num_seeds=3, num_rounds=2, seed_distribution=lambda movie: pix.expand(movie.shape[0], -1, -1), seed_mode="peaks", seed_radius=1, **SCENE_KW)
    first = SM.seed_cells(out.seeds[:, :3], 4, 8)[0].tolist()
    assert first == [0, 11, 12]
    for y, xx in out.seeds[0, 3:].tolist():
        if y >= 0:
            c = (y // 8, xx // 8)
            assert out.segments[0, :3, y, xx].sum() == 0 and all(max(abs(c[0] - f // 4), abs(c[1] - f % 4)) > 1 for f in first)
    # the race with a spacing: the same draw as the plain race, picks more than seed_radius apart
    gen = torch.Generator().manual_seed(9)
    out = G.segment_scene(x, num_seeds=4, seed_radius=1, generator=gen, **SCENE_KW)
    e = torch.empty((1, 16)).exponential_(generator=torch.Generator().manual_seed(9))
    want = SS.select_seeds(torch.ones((1, 4, 4)), 4, 8, cells=True, radius=1, e=e)
    assert torch.equal(out.seeds, want.seeds)
    got = [(y // 8, xx // 8) for y, xx in out.seeds[0].tolist() if y >= 0]
    assert len(got) >= 2 and all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) > 1 for i, p in enumerate(got) for q in got[:i])
