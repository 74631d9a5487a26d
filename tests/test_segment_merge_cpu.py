"""Scene segmentation without a GPU: the definition of `cwm_segment_merge` as the NumPy restatement states it (tests/segment_merge_restatement.py) on the
hand-worked case, the package's torch composition (`segment_merge` on CPU tensors) against the restatement, and the `segment_scene` loop on CPU tensors with the
counterfactual driver stubbed.  Every output is an integer or an integer divided by P P: every comparison is equality."""
import numpy as np
import pytest
import torch

import segment_merge_restatement as MR
from counterfactualworldmodels_amd import segment_merge as SM, segment_step as SS, segmentation, vmae
from test_segment_cpu import TINY

NAMES = ("labels", "owner", "area", "label_area", "inter", "cover", "stats")


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind == "f":
        return got.shape == want.shape and np.array_equal(got.view(np.int32), want.astype(np.float32).view(np.int32))
    return got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64))


def compare(res, want):
    for k in NAMES:
        assert same(getattr(res, k).cpu().numpy(), want[k]), k


def both(segs, scores, P, view=None, **kw):
    """the torch composition on CPU tensors and the restatement, compared; `view` maps the tensor of a LARGER buffer to the [B,K,H,W] view that is merged"""
    t = torch.from_numpy(np.ascontiguousarray(segs))
    if view is not None:
        t = view(t)
    want = MR.merge(t.numpy(), scores, P, **kw)
    res = SM.segment_merge(t, None if scores is None else torch.from_numpy(np.asarray(scores, np.float32)), P, want_inter=True, **kw)
    assert not res.labels.is_cuda and res.labels.dtype == torch.uint8 and res.cover.dtype == torch.float32 and res.owner.dtype == torch.int32
    compare(res, want)
    return want


@pytest.mark.parametrize("absorb", [1, 0])
def test_hand_worked_case(absorb):
    segs, scores, P, kw = MR.hand_worked()
    want = both(segs, scores, P, absorb=absorb, **kw)
    for k in ("area", "owner", "inter"):
        assert want[k].tolist() == MR.HAND[k], k
    for k, v in MR.HAND[absorb].items():
        assert want[k].tolist() == v, k
    assert want["labels"][0, 2, 4] == 1 and want["labels"][0, 0, 0] == 2 and want["labels"][0, 0, 6] == (2 if absorb else 0) and want["labels"][0, 0, 11] == 0


def test_score_ties_fall_to_the_index_and_special_scores():
    segs = np.stack([MR.rect(8, 16, 0, 4, 4 * k, 4 * k + 4) for k in range(4)])[None]  # four disjoint squares: labels are the order itself
    assert both(segs, np.array([[1, 2, 2, 1]], np.float32), 4)["owner"].tolist() == [[3, 1, 2, 4]]
    assert both(segs, None, 4)["owner"].tolist() == [[1, 2, 3, 4]]
    assert both(segs, np.array([[-0.0, 0.0, np.nan, np.inf]], np.float32), 4)["owner"].tolist() == [[3, 4, 1, 2]]  # NaN, inf, then -0 = +0 by index
    assert both(segs, np.array([[-np.inf, np.nan, np.nan, -1.0]], np.float32), 4)["owner"].tolist() == [[4, 1, 2, 3]]
    segs, _ = MR.random_rects(5, 2, 10, 16, 24)
    both(segs, MR.special_scores(2, 10), 8, iou_thresh=0.3)


def test_single_candidate_empty_and_identical_sets():
    want = both(MR.rect(8, 8, 1, 5, 2, 7)[None, None], None, 4)
    assert want["stats"].tolist() == [[1, 1, 20, 0]] and want["owner"].tolist() == [[1]]
    want = both(np.zeros((2, 6, 8, 12), np.uint8), MR.special_scores(2, 6), 4)
    assert not want["labels"].any() and want["stats"].tolist() == [[0, 0, 0, 0]] * 2 and not want["owner"].any() and not want["cover"].any()
    want = both(MR.identical(1, 7, 12, 16), MR.special_scores(1, 7), 4)
    assert want["stats"].tolist() == [[7, 1, 10 * 13, 6]] and want["owner"].tolist() == [[1] * 7] and want["label_area"][0].tolist() == [130] + [0] * 6


def test_containment_chain_and_no_chaining_through_a_union():
    segs = MR.chain()  # areas 144, 64, 16: I / min is 1 for every pair, I / U is 4/9, 1/9 and 1/4
    want = both(segs, np.array([[3, 2, 1]], np.float32), 4, iou_thresh=0.9, contain_thresh=0.6)
    assert want["owner"].tolist() == [[1, 1, 1]] and want["stats"].tolist() == [[3, 1, 144, 2]]
    want = both(segs, np.array([[1, 2, 3]], np.float32), 4, iou_thresh=0.9, contain_thresh=0.6)  # the smallest first: it absorbs both larger ones
    assert want["owner"].tolist() == [[1, 1, 1]] and want["label_area"][0].tolist() == [144, 0, 0]
    assert both(segs, np.array([[1, 2, 3]], np.float32), 4, iou_thresh=0.9, contain_thresh=0.6, absorb=0)["label_area"][0].tolist() == [16, 0, 0]
    # a b c in a row, a-b and b-c overlap, a-c do not: with b absorbed by a, c is compared with a and b's OWN segments' keepers only -- a -- and is kept
    row = np.stack([MR.rect(4, 32, 0, 4, 0, 12), MR.rect(4, 32, 0, 4, 4, 16), MR.rect(4, 32, 0, 4, 12, 24)])[None]
    want = both(row, None, 4, iou_thresh=0.3, contain_thresh=2.0)
    assert want["owner"].tolist() == [[1, 1, 2]] and want["label_area"][0].tolist() == [64, 32, 0]


def test_thresholds_are_strict_and_nan_thresholds_absorb_nothing():
    segs = MR.half_overlap()  # I = 16, U = 32, min = 24
    assert both(segs, None, 4, iou_thresh=0.5, contain_thresh=1.0)["owner"].tolist() == [[1, 2]]      # 16 > .5 * 32 is false
    assert both(segs, None, 4, iou_thresh=0.4999, contain_thresh=1.0)["owner"].tolist() == [[1, 1]]
    assert both(MR.chain(), None, 4, iou_thresh=2.0, contain_thresh=1.0)["owner"].tolist() == [[1, 2, 3]]  # I == min: 16 > 1 * 16 is false
    assert both(MR.identical(1, 4, 8, 8), None, 4, iou_thresh=float("nan"), contain_thresh=float("nan"))["owner"].tolist() == [[1, 2, 3, 4]]
    assert both(MR.identical(1, 4, 8, 8), None, 4, iou_thresh=float("nan"))["owner"].tolist() == [[1, 1, 1, 1]]


def test_area_bounds():
    full = np.stack([np.ones((8, 12), np.uint8), MR.rect(8, 12, 0, 4, 0, 4), MR.rect(8, 12, 0, 1, 0, 1)])[None]
    want = both(full, None, 4, max_area=48, contain_thresh=2.0, iou_thresh=2.0)  # the full image is cut, the others stand
    assert want["owner"].tolist() == [[0, 1, 2]] and want["stats"].tolist() == [[2, 2, 16, 0]]
    assert both(full, None, 4, max_area=0, contain_thresh=2.0, iou_thresh=2.0)["owner"].tolist() == [[1, 2, 3]]
    a, b = (both(full, None, 4, min_area=m, contain_thresh=2.0, iou_thresh=2.0) for m in (0, 1))
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)
    assert both(full, None, 4, min_area=2, contain_thresh=2.0, iou_thresh=2.0)["owner"].tolist() == [[1, 2, 0]]


def test_strided_input_is_read_as_a_view():
    segs, scores = MR.random_rects(9, 2, 8, 16, 24)
    segs[:, 5:] = 1  # planes that a [:, :5] slice must not read
    both(segs, scores[:, ::2], 8, view=lambda t: t[:, ::2])
    both(segs, scores[:, :5], 8, view=lambda t: t[:, :5])
    with pytest.raises(ValueError, match="K = 65"):
        SM.segment_merge(torch.zeros((1, 65, 8, 8), dtype=torch.bool), None, 4)
    with pytest.raises(ValueError, match="P = 5"):
        SM.segment_merge(torch.zeros((1, 2, 10, 10), dtype=torch.bool), None, 5)


# ---- the scene loop on CPU tensors: the counterfactual driver is the stub of test_segment_cpu.py, with TWO objects in its table.  A seed on either object gives
# that object (the component that hangs on the seed's patch), a seed on the background gives nothing ----
S_ = 4


def two_object_table(S=S_, H=32, W=32):
    """[1,2,H,W,S]: object A (rows 0-15, cols 0-15) and object B (rows 16-31, cols 24-31) move 8 px along an axis direction; exact magnitudes"""
    a, b = np.zeros((H, W), bool), np.zeros((H, W), bool)
    a[0:16, 0:16] = True
    b[16:32, 24:32] = True
    f = np.zeros((1, 2, H, W, S), np.float32)
    for s, (dy, dx) in enumerate(SS.directions(S)):
        f[0, 0, :, :, s], f[0, 1, :, :, s] = (a | b) * 8.0 * dx, (a | b) * 8.0 * dy
    return a, b, f


def stub_generator(table, calls):
    G = segmentation.FlowGenerator(predictor=vmae.PretrainVisionTransformer(TINY), imagenet_normalize_inputs=True, temporal_dim=2, seed=0)

    def driver(xx, active_patches, passive_patches=None, shifts=None, num_samples=8, **kw):
        R = xx.shape[0]
        calls.append(R)
        G.x = xx
        t = torch.from_numpy(table).permute(0, 4, 1, 2, 3)  # [1,S,2,H,W]
        return None, t.expand(R, -1, -1, -1, -1).reshape(R * t.shape[1], 1, 2, 32, 32)

    G.predict_counterfactual_videos_and_flows = driver
    return G


SCENE_KW = dict(num_iters=1, num_samples=S_, k_active=1, k_passive=0, min_seed_mag=1.0, abs_thresh=1.0)


def test_segment_scene_two_objects_and_the_second_rounds_seeds():
    a, b, table = two_object_table()
    calls = []
    G = stub_generator(table, calls)
    x = torch.zeros((1, 2, 3, 32, 32))
    seeds = torch.tensor([[[4, 4], [20, 28], [12, 12], [28, 4]]])  # A, B, A again, the background
    state = torch.get_rng_state()
    gen = torch.Generator().manual_seed(5)
    out = G.segment_scene(x, seeds=seeds, num_seeds=4, num_rounds=2, generator=gen, seed_batch_size=3, **SCENE_KW)
    assert torch.equal(torch.get_rng_state(), state)
    assert calls == [3, 1, 3, 1]  # chunks of seed_batch_size rows
    assert out.labels.shape == (1, 32, 32) and out.labels.dtype == torch.uint8 and out.segments.shape == (1, 8, 32, 32) and out.segments.dtype == torch.bool
    assert out.num_labels.tolist() == [2] and out.owner[0, :4].tolist() == [1, 2, 1, 0]
    lab = out.labels[0].numpy()
    assert np.array_equal(lab == 1, a) and np.array_equal(lab == 2, b)
    # round 1: drawn among the cells round 0 left uncovered; with the same generator state the draw is the race of the restated rule
    cover0 = MR.merge(out.segments[:, :4].numpy(), out.scores[:, :4].numpy(), 8, min_area=64, max_area=512)["cover"]
    free = torch.from_numpy(cover0 == 0).reshape(1, 16)
    assert int(free.sum()) == 16 - 4 - 2
    gen = torch.Generator().manual_seed(5)
    cells = SM.draw_seed_cells(torch.ones((1, 16)), free, 4, gen)
    assert bool(free[0, cells[0]].all()) and len(set(cells[0].tolist())) == 4
    assert torch.equal(out.seeds[:, 4:], SM.cell_centres(cells, 4, 8)) and torch.equal(out.seeds[:, :4], seeds.to(torch.int32))
    assert out.owner[0, 4:].tolist() == [0, 0, 0, 0] and not out.segments[0, 4:].any()  # the background holds nothing more
    want = MR.merge(out.segments.numpy(), out.scores.numpy(), 8, min_area=64, max_area=512)
    for k in ("labels", "owner", "label_area", "cover", "stats"):
        assert same(getattr(out, k).numpy(), want[k]), k
    assert out.scores[0, :4].tolist() == [1.0, 1.0, 1.0, 0.0]
    area = G.segment_scene(x, seeds=seeds, num_seeds=4, score="area", **SCENE_KW)
    assert area.scores.tolist() == [[256.0, 128.0, 256.0, 0.0]] and area.owner.tolist() == [[1, 2, 1, 0]]


def test_segment_scene_dead_slots_distribution_and_refusals():
    a, b, table = two_object_table()
    G = stub_generator(table, [])
    x = torch.zeros((1, 2, 3, 32, 32))
    dist = torch.zeros((1, 4, 4))
    dist[0, 0, 0], dist[0, 2, 3] = 1.0, 3.0  # only a cell of A and a cell of B carry weight: they are drawn first, in either order
    gen = torch.Generator().manual_seed(1)
    out = G.segment_scene(x, num_seeds=2, num_rounds=2, seed_distribution=dist, generator=gen, free_below=0.5, **SCENE_KW)
    assert sorted(out.seeds[0, :2].tolist()) == [[4, 4], [20, 28]] and out.num_labels.tolist() == [2]
    assert all(out.cover[0, y // 8, x // 8] == 0 for y, x in out.seeds[0, 2:].tolist())
    # 10 free cells are left after the two objects: a round of 12 seeds finds 10 and leaves two dead slots
    out = G.segment_scene(x, seeds=torch.tensor([[[4, 4], [20, 28]] + [[28, 4]] * 10]), num_seeds=12, num_rounds=2, generator=gen, **SCENE_KW)
    assert out.seeds[0, 12:22].min() >= 0 and out.seeds[0, 22:].tolist() == [[-1, -1]] * 2
    assert not out.segments[0, 22:].any() and out.owner[0, 22:].tolist() == [0, 0] and out.scores[0, 22:].tolist() == [0.0, 0.0]
    pix = torch.zeros((1, 32, 32))
    pix[0, 0:8, 8:16] = 1.0  # a pixel distribution is averaged to patches: cell (0, 1) first
    assert G.segment_scene(x, num_seeds=1, seed_distribution=pix, generator=gen, **SCENE_KW).seeds.tolist() == [[[4, 12]]]
    with pytest.raises(ValueError, match="num_rounds \\* num_seeds"):
        G.segment_scene(x, num_seeds=13, num_rounds=5, **SCENE_KW)
    with pytest.raises(ValueError, match="seeds must be"):
        G.segment_scene(x, seeds=torch.zeros((1, 3, 2)), num_seeds=2, **SCENE_KW)
    with pytest.raises(ValueError, match="score"):
        G.segment_scene(x, num_seeds=2, score="iou", **SCENE_KW)
