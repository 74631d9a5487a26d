"""`FlowGenerator.segment_scene` on a real MI355X against the loop composed by hand from `segment_spelke_object`, the torch score expression and the NumPy
restatement of the merge (tests/segment_merge_restatement.py): the tiny predictor and the stub flow model of tests/test_spelke_segment_gpu.py, with TWO objects
in the stub's table -- a seed on either object gives that object, a seed on the background nothing.  Given seeds, drawn seeds with a seeded generator in one
round and in two; labels, owner, cover and the second round's seeds are equal, and the caller's global CPU RNG state is left as it was."""
import numpy as np
import pytest
import torch

import segment_merge_restatement as MR
from counterfactualworldmodels_amd import masking, segmentation, synthetic as S
from test_segment_cpu import TINY
from test_segment_merge_cpu import S_ as NS, two_object_table
from test_spelke_segment_gpu import TableFlow, predictor

pytestmark = pytest.mark.gpu
KW = dict(num_iters=2, num_samples=NS, k_active=2, k_passive=2, min_seed_mag=1.0, abs_thresh=1.0)
B, P, GW = 2, 8, 4
MERGE = dict(min_area=64, max_area=512, iou_thresh=0.5, contain_thresh=0.6)


@pytest.fixture(scope="module")
def scene():
    a, b, table = two_object_table()
    G = segmentation.FlowGenerator(predictor=predictor(TINY), flow_model=TableFlow(table), imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
    x = torch.from_numpy(S.synthetic_frames(B, TINY, 3)).cuda()
    return G, x, a, b


def by_hand(G, x, seeds, K, rounds, gen):
    """the loop: per round the seeds (given, or the exponential race among the free cells), one segment_spelke_object over the (b, k) rows, the score expression
    in torch, and the restatement's merge over all candidates so far.  Returns (the last merge, seeds [B,rounds K,2], segments, scores) as CPU arrays."""
    segs, scores, all_seeds, want = [], [], [], None
    free = torch.ones((B, GW * GW), dtype=torch.bool, device="cuda")
    for r in range(rounds):
        if r == 0 and seeds is not None:
            rs = seeds.to(torch.int32)
        else:
            e = torch.empty((B, GW * GW), device="cuda", dtype=torch.float32).exponential_(generator=gen)
            cells = masking.select_reveal(torch.ones((B, GW * GW), device="cuda"), free, torch.zeros_like(free), K, e=e)
            rs = torch.stack([cells // GW * P + P // 2, cells % GW * P + P // 2], -1).to(torch.int32)
            rs[cells < 0] = -1
        alive = (rs[..., 0] >= 0).reshape(B * K)
        seg, frac = G.segment_spelke_object(x.repeat_interleave(K, 0), rs.reshape(B * K, 2).clamp(min=0), generator=gen, **KW)
        seg = seg & alive[:, None, None]
        sc = (frac * seg).flatten(1).sum(1) / seg.flatten(1).sum(1).float().clamp(min=1)
        segs.append(seg.reshape(B, K, 32, 32).cpu().numpy())
        scores.append(sc.reshape(B, K).cpu().numpy())
        all_seeds.append(rs.cpu().numpy())
        want = MR.merge(np.concatenate(segs, 1), np.concatenate(scores, 1), P, **MERGE)
        free = torch.from_numpy(want["cover"] == 0).reshape(B, GW * GW).cuda()
    return want, np.concatenate(all_seeds, 1), np.concatenate(segs, 1), np.concatenate(scores, 1)


def compare(out, hand):
    want, seeds, segs, scores = hand
    assert np.array_equal(out.seeds.cpu().numpy(), seeds), "seeds"
    assert np.array_equal(out.segments.cpu().numpy(), segs.astype(bool)) and np.array_equal(out.scores.cpu().numpy(), scores)
    for k in ("labels", "owner", "label_area", "stats"):
        assert np.array_equal(getattr(out, k).cpu().numpy(), want[k]), k
    assert np.array_equal(out.cover.cpu().numpy().view(np.int32), want["cover"].view(np.int32)), "cover"
    assert np.array_equal(out.num_labels.cpu().numpy(), want["stats"][:, 1])
    assert out.labels.is_cuda and out.labels.dtype == torch.uint8 and out.segments.dtype == torch.bool and out.cover.is_cuda


def test_given_seeds(scene):
    G, x, a, b = scene
    seeds = torch.tensor([[[4, 4], [20, 28], [12, 12], [28, 4]], [[28, 28], [28, 4], [4, 12], [4, 8]]], device="cuda")  # row 0: A, B, A, nothing; row 1: B, nothing, A, A
    torch.manual_seed(13)
    state = torch.get_rng_state()
    out = G.segment_scene(x, seeds=seeds, num_seeds=4, seed_batch_size=5, **KW)
    assert torch.equal(torch.get_rng_state(), state)
    compare(out, by_hand(G, x, seeds, 4, 1, None))
    assert out.owner.tolist() == [[1, 2, 1, 0], [1, 0, 2, 2]] and out.num_labels.tolist() == [2, 2]
    lab = out.labels.cpu().numpy()
    assert np.array_equal(lab[0] == 1, a) and np.array_equal(lab[0] == 2, b) and np.array_equal(lab[1] == 1, b) and np.array_equal(lab[1] == 2, a)
    torch.set_rng_state(state)


@pytest.mark.parametrize("rounds", [1, 2])
def test_drawn_seeds(scene, rounds):
    G, x, a, b = scene
    torch.manual_seed(17)
    state = torch.get_rng_state()
    out = G.segment_scene(x, num_seeds=5, num_rounds=rounds, generator=torch.Generator(device="cuda").manual_seed(23), **KW)
    assert torch.equal(torch.get_rng_state(), state)
    hand = by_hand(G, x, None, 5, rounds, torch.Generator(device="cuda").manual_seed(23))
    compare(out, hand)
    if rounds == 2:  # the second round's seeds lie in cells the first left uncovered
        first = MR.merge(hand[2][:, :5], hand[3][:, :5], P, **MERGE)["cover"]
        for r in range(B):
            for y, xx in out.seeds[r, 5:].tolist():
                assert first[r, y // P, xx // P] == 0
    torch.set_rng_state(state)
