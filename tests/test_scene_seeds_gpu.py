"""The seeds of `FlowGenerator.segment_scene` on a real MI355X, on the synthetic models of tests/test_scene_segment_gpu.py (the tiny predictor, the stub flow
model with two objects in its table): with the default keywords the loop draws what it drew before there was a choice -- held against the loop composed by
hand there -- and with seed_mode="peaks" on a pixel map of known bumps the seeds of round 0 are those of the NumPy restatement of `cwm_seed_select`, those of
round 1 lie in cells the first merge left uncovered and farther than seed_radius from every seed cell of round 0.  The caller's global CPU RNG state is left
as it was."""
import numpy as np
import pytest
import torch

import seed_select_restatement as R
import segment_merge_restatement as MR
from test_scene_segment_gpu import B, GW, KW, MERGE, P, by_hand, compare, scene  # noqa: F401  (scene: the module's fixture)

pytestmark = pytest.mark.gpu


def test_default_keywords_draw_the_seeds_they_drew_before(scene):
    G, x, a, b = scene
    torch.manual_seed(17)
    state = torch.get_rng_state()
    plain = G.segment_scene(x, num_seeds=5, num_rounds=2, generator=torch.Generator(device="cuda").manual_seed(23), **KW)
    named = G.segment_scene(x, num_seeds=5, num_rounds=2, generator=torch.Generator(device="cuda").manual_seed(23), seed_mode="sample", seed_radius=0,
                            seed_rel_thresh=0., **KW)
    assert torch.equal(torch.get_rng_state(), state)
    for k in ("seeds", "segments", "labels", "scores", "owner", "cover"):
        assert torch.equal(getattr(plain, k), getattr(named, k)), k
    compare(named, by_hand(G, x, None, 5, 2, torch.Generator(device="cuda").manual_seed(23)))
    torch.set_rng_state(state)


def bump_map():
    """[B,32,32]: a low noise floor and single-pixel bumps -- on object A (rows 0-15, columns 0-15), on object B (rows 16-31, columns 24-31), on the
    background next to neither, and lower ones on background cells"""
    m = np.random.RandomState(3).rand(B, 32, 32).astype(np.float32) * 0.01
    for (y, x, h) in ((3, 5, 3.0), (22, 30, 2.0), (27, 2, 1.0), (4, 20, 0.5), (6, 29, 0.4)):
        m[0, y, x] = h
    for (y, x, h) in ((25, 27, 3.0), (12, 9, 2.0), (2, 28, 1.0), (30, 1, 0.5), (20, 12, 0.4)):
        m[1, y, x] = h
    return m


def test_peaks_of_a_pixel_map(scene):
    G, x, a, b = scene
    m, K, radius, rel = bump_map(), 3, 1, 0.1
    torch.manual_seed(19)
    state = torch.get_rng_state()
    gen = torch.Generator(device="cuda").manual_seed(5)
    out = G.segment_scene(x, num_seeds=K, num_rounds=2, seed_distribution=torch.from_numpy(m).cuda(), seed_mode="peaks", seed_radius=radius, seed_rel_thresh=rel,
                          generator=gen, **KW)
    assert torch.equal(torch.get_rng_state(), state)
    seeds = out.seeds.cpu().numpy()
    first = R.select(m, P, K, radius=radius, peaks_only=True, rel_thresh=rel)
    assert np.array_equal(seeds[:, :K], first["seeds"])
    assert first["seeds"][0].tolist() == [[3, 5], [22, 30], [27, 2]] and first["seeds"][1].tolist() == [[25, 27], [12, 9], [2, 28]]  # the bump pixels, highest first
    assert out.num_labels.tolist() == [2, 2]
    cover0 = MR.merge(out.segments[:, :K].cpu().numpy(), out.scores[:, :K].cpu().numpy(), P, **MERGE)["cover"].reshape(B, -1)
    second = R.select(m, P, K, radius=radius, peaks_only=True, rel_thresh=rel, free=cover0 == 0, prior=first["cells"])
    assert np.array_equal(seeds[:, K:], second["seeds"])
    assert (seeds[:, K:, 0] >= 0).any(1).all()  # every row finds a seed in round 1
    for r in range(B):
        for y, xx in seeds[r, K:].tolist():
            if y < 0:
                continue
            assert cover0[r, (y // P) * GW + xx // P] == 0
            assert all(max(abs(y // P - c // GW), abs(xx // P - c % GW)) > radius for c in first["cells"][r].tolist())
    torch.set_rng_state(state)
