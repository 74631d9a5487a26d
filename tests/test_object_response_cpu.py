"""`object_response.measure_torch` against the NumPy restatement (tests/object_response_restatement.py) for EQUALITY -- the integer tables by value, the coupling
as int64 bit patterns --, the host decisions `relations` / `groups` / `merge_labels` on the three-object scene with their expected tables pinned, dead rows,
argument errors, and the accepted layouts.  No GPU needed."""
import numpy as np
import pytest
import torch

import object_response_restatement as R
from counterfactualworldmodels_amd import object_response as OR

B, K, H, W, S = 2, 3, 24, 40, 5


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def fields(resp):
    out = {k: getattr(resp, k).reshape((-1,) + tuple(getattr(resp, k).shape[2:])).numpy() for k in R.NAMES}
    out["valid"] = out["valid"].astype(np.uint8)
    return out


def equal(got, want, what=""):
    for k in R.NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, what, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(R.bits(got[k]), R.bits(want[k])), (k, what, int((R.bits(got[k]) != R.bits(want[k])).sum()))


def check(flows, labels, pushed, dirs=None, what="", **kw):
    want = R.response(flows, R.per_row(labels, len(pushed) // len(labels)), pushed, dirs, **kw)
    got = OR.measure(t(flows), t(labels), t(pushed), dirs=t(dirs), **kw)
    assert tuple(got.tab.shape[:2]) == (len(labels), len(pushed) // len(labels)) and got.valid.dtype == torch.bool
    equal(fields(got), want, what)
    return want


def test_random_labels_and_hostile_flows():
    flows, labels, pushed = R.case_random(B, K, H, W, S)
    assert (labels > 64).any() and np.isnan(flows).any() and np.isinf(flows).any() and (flows == 5000).any() and (flows == -4096.5).any()
    assert (flows == 4096).any() and (flows == -4096).any()
    w = check(flows, labels, pushed, R.dirs_of(S), what="random")
    assert w["tab"][..., 7].sum() > 100 and (w["tab"][..., 0] + w["tab"][..., 7]).sum() == B * K * S * H * W
    assert 0 < w["tab"][..., 1].sum() < w["tab"][..., 0].sum()  # the threshold row: some at q2 = min_q2 moved, some one step below did not
    assert w["stats"][1:4, 0].tolist() == [0, 0, 0] and w["valid"].any()
    check(flows, labels, pushed, R.dirs_of(S), min_mag=2.0, min_pixels=6, self_frac=0.2, move_frac=0.9, what="thresholds")
    check(flows, labels, pushed, None, what="no dirs")


def test_threshold_is_an_integer_comparison_at_equality():
    labels = np.ones((1, 4, 4), np.uint8)
    flows = np.zeros((1, 2, 4, 4, 1), np.float32)
    flows[0, 0, 0], flows[0, 1, 0] = 0.6, 0.8           # 154 and 205 in 1/256 px: q2 = 65741 >= 65536
    flows[0, 0, 1] = np.float32(255.4 / 256)            # rounds to 255: below
    flows[0, 0, 2] = np.float32(255.5 / 256)            # half to even: 256, q2 = min_q2 exactly
    w = check(flows, labels, np.array([1], np.int32), what="equality")
    assert w["tab"][0, 0, 1, :2].tolist() == [16, 8]
    w = check(flows, labels, np.array([1], np.int32), min_mag=0.0, what="zero threshold")
    assert w["tab"][0, 0, 1, :2].tolist() == [16, 16]


def test_rows_and_checker_labels():
    for case in (R.case_rows, R.case_checker):
        flows, labels, pushed = case(B, K, H, W, S)
        w = check(flows, labels, pushed, R.dirs_of(S), what=case.__name__)
        assert (w["stats"][:, 1] == pushed).all() and (w["stats"][:, 2] > 0).all()


# the three-object scene, worked out from the restatement and pinned: per pushed slot (1, 2, 3) the vote c0 and the gain c3 of slots 0 .. 3
SCENE_C0 = [[0.0, 1.0, 1.0, 0.0], [0.0, 1.0, 1.0, 0.0], [0.0, 0.0, 1.0, 1.0]]
SCENE_C3 = [[0.0, 1.0, 0.75, 0.0], [0.0, 0.75, 1.0, 0.0], [0.0, 0.0, 0.5, 1.0]]


def scene(Bs=2, Hs=32, Ws=32, Ss=5):
    flows, labels, pushed, dirs = R.case_scene(Bs, Hs, Ws, Ss)
    return flows, labels, pushed, dirs, OR.measure(t(flows), t(labels), t(pushed), dirs=t(dirs))


def test_scene_tables_equal_the_restatement_and_the_pinned_values():
    flows, labels, pushed, dirs, got = scene()
    want = R.response(flows, R.per_row(labels, 3), pushed, dirs)
    equal(fields(got), want, "scene")
    assert want["stats"][:, 0].tolist() == [4] * 6 and want["stats"][:, 1].tolist() == [1, 2, 3] * 2
    assert want["stats"][:, 2].tolist() == [int((labels[0] == s).sum()) for s in (1, 2, 3)] * 2
    assert [want["valid"][r].tolist() for r in range(6)] == [[int(s != r % 5) for s in range(5)] for r in range(6)]
    c = want["coupling"].reshape(2, 3, 65, 4)
    for b in range(2):
        assert c[b, :, :4, 0].tolist() == SCENE_C0 and c[b, :, :4, 3].tolist() == SCENE_C3
        assert not c[b, :, 4:].any() and (c[b, :, :4, 1] == c[b, :, :4, 0]).all()
    # c2 is the mean of (flow . dir) / 256 with dirs in PIXELS of shift (8 px per patch step): row 0 loses sample 0, its valid samples are S, W, N (|d| = 8) and
    # SE (d = (8, 8), flow (2.5, 2.5)): (3 x 2.5 x 8 + 2.5 x 16) / 4 = 25
    assert c[0, 0, 1, 2] == 25.0 and c[0, 0, 2, 2] == 18.75


def test_relations_groups_and_merge_labels_on_the_scene():
    flows, labels, pushed, dirs, got = scene()
    slots = pushed.reshape(2, 3)
    moves, mutual, carries, tested = OR.relations(got, t(slots))
    wm, wmu, wc, wt = R.relations(got.coupling.numpy(), got.stats.numpy(), slots)
    for a, b_ in ((moves, wm), (mutual, wmu), (carries, wc), (tested, wt)):
        assert a.dtype == torch.bool and np.array_equal(a.numpy(), b_)
    for b in range(2):
        assert sorted(map(tuple, np.argwhere(wm[b]).tolist())) == [(1, 2), (2, 1), (3, 2)]  # 3 moves 2 but is not moved by it
        assert sorted(map(tuple, np.argwhere(wmu[b]).tolist())) == [(1, 2), (2, 1)]         # mutual is exactly {1 <-> 2}
        assert np.argwhere(wc[b]).tolist() == [[3, 2]] and np.nonzero(wt[b])[0].tolist() == [1, 2, 3]
    g = OR.groups(mutual)
    assert g.dtype == torch.int32 and np.array_equal(g.numpy(), R.groups(wmu))
    assert g[0].tolist() == [0, 1, 1] + list(range(3, 65))
    merged = OR.merge_labels(t(labels), g)
    want = labels.copy()
    want[want == 2] = 1
    assert merged.dtype == torch.uint8 and np.array_equal(merged.numpy(), want)
    movie = torch.zeros((2, 3, 32, 32), dtype=torch.uint8)
    movie[:, 1:] = t(labels)[:, None]
    movie[0, 1, 0, 0] = 200  # (a byte above 64 reads as 0)
    assert np.array_equal(OR.merge_labels(movie[:, 1:], g)[:, 0].numpy(), want)
    # a stricter gain drops the half-gain link, a chain 1 - 2 - 3 of mutual links is one group, without dirs the gain test is skipped
    assert not OR.relations(got, t(slots), min_gain=0.6)[0][:, 3, 2].any()
    chain = torch.zeros((1, 65, 65), dtype=torch.bool)
    for a, b_ in ((5, 9), (9, 30), (30, 64), (2, 3)):
        chain[0, a, b_] = chain[0, b_, a] = True
    g = OR.groups(chain)[0].tolist()
    assert [g[i] for i in (5, 9, 30, 64, 2, 3, 0, 1, 4)] == [5, 5, 5, 5, 2, 2, 0, 1, 4] and np.array_equal(OR.groups(chain).numpy(), R.groups(chain.numpy()))
    bare = OR.measure(t(flows), t(labels), t(pushed))
    assert not bare.coupling[..., 2:].any() and not bare.agg[..., 2].any()
    assert torch.equal(OR.relations(bare, t(slots))[0], moves)


def test_a_dead_row_has_no_valid_sample_and_zero_coupling():
    flows, labels, pushed, dirs = R.case_scene(1, 32, 32, 4)
    for dead in (0, 65, -1, 7):  # (7: in range, but the map holds no such pixel)
        p = pushed.copy()
        p[1] = dead
        got = OR.measure(t(flows), t(labels), t(p), dirs=t(dirs))
        equal(fields(got), R.response(flows, R.per_row(labels, 3), p, dirs), dead)
        assert got.stats[0, 1].tolist() == [0, dead if dead == 7 else 0, 0, 0] and not got.coupling[0, 1].any() and not got.valid[0, 1].any() and not got.agg[0, 1].any()
        assert got.stats[0, 0, 0] == 3 and got.tab[0, 1].any()  # the tables of the dead row are still summed
        moves, _, _, tested = OR.relations(got, t(p.reshape(1, 3)))
        assert not tested[0, 2] and not moves[0, 2].any() and not moves[0, dead if dead == 7 else 0].any()


def test_layouts_give_equal_results():
    flows, labels, pushed = R.case_random(B, K, H, W, S, seed=8)
    dirs = t(R.dirs_of(S))
    base = fields(OR.measure(t(flows), t(labels), t(pushed), dirs=dirs))
    f = t(flows)
    outer = f.permute(0, 4, 1, 2, 3).contiguous().reshape(B * K * S, 1, 2, H, W)  # the flow model's output, [(r s),1,2,H,W] ...
    view = outer[:, 0].reshape(B * K, S, 2, H, W).movedim(1, -1)                   # ... and its `_batch_to_samples` view
    assert not view.is_contiguous() and view.stride(-1) == 2 * H * W and torch.equal(view.contiguous().view(torch.int32), f.view(torch.int32))
    equal(fields(OR.measure(view, t(labels), t(pushed), dirs=dirs)), base, "sample-outer")
    equal(fields(OR.measure(f.reshape(B, K, 2, H, W, S), t(labels), t(pushed).reshape(B, K), dirs=dirs)), base, "[B,K,..] flows")
    per_push = t(labels)[:, None].expand(B, K, H, W).contiguous()
    equal(fields(OR.measure(f, per_push, t(pushed), dirs=dirs)), base, "[B,K,H,W] labels")
    big = torch.zeros((B, K + 1, H, W), dtype=torch.uint8)
    big[:, 1:] = per_push
    equal(fields(OR.measure(f, big[:, 1:], t(pushed), dirs=dirs)), base, "a slice of a larger map")
    other = per_push.clone()
    other[:, 1] = 0  # a map of its own for push 1: its rows see no slot
    got = fields(OR.measure(f, other, t(pushed), dirs=dirs))
    equal(got, R.response(flows, other.reshape(B * K, H, W).numpy(), pushed, R.dirs_of(S)), "per-push maps")
    assert not np.array_equal(got["tab"], base["tab"])
    equal(fields(OR.measure(f.double(), t(labels), t(pushed).long(), dirs=dirs.float())), base, "other dtypes")


def test_argument_errors():
    flows, labels, pushed = (t(a) for a in R.case_random(1, 2, 8, 12, 2))
    ok = dict(dirs=t(R.dirs_of(2)))
    OR.measure(flows, labels, pushed, **ok)
    bad = [
        lambda: OR.measure(flows[:, :1], labels, pushed),
        lambda: OR.measure(flows[0], labels, pushed),
        lambda: OR.measure(flows, labels[:, :, :8], pushed),
        lambda: OR.measure(flows, labels.float(), pushed),
        lambda: OR.measure(flows, labels, pushed[:1]),
        lambda: OR.measure(flows, labels, pushed.float()),
        lambda: OR.measure(flows, labels, pushed, dirs=t(R.dirs_of(3))),
        lambda: OR.measure(flows, labels, pushed, dirs=torch.full((2, 2), 0.5)),
        lambda: OR.measure(flows[:, :, :6], labels[:, :6], pushed),
        lambda: OR.measure(flows[:, :, :, :10], labels[:, :, :10], pushed),
        lambda: OR.measure(flows.repeat(1, 1, 1, 1, 128), labels, pushed),
        lambda: OR.measure(flows.reshape(3, 2, 8, 8, 2), torch.zeros((2, 8, 8), dtype=torch.uint8), torch.zeros(3, dtype=torch.int32)),
        lambda: OR.measure(flows, labels, pushed, min_mag=-1.0),
        lambda: OR.measure(flows, labels, pushed, min_mag=float("nan")),
        lambda: OR.measure(flows, labels, pushed, min_pixels=0),
        lambda: OR.measure(flows, labels, pushed, self_frac=1.5),
        lambda: OR.measure(flows, labels, pushed, self_frac=float("nan")),
        lambda: OR.measure(flows, labels, pushed, move_frac=-0.1),
        lambda: OR.relations(OR.measure(flows, labels, pushed, **ok), torch.tensor([1, 2, 3])),
        lambda: OR.groups(torch.zeros((1, 64, 64), dtype=torch.bool)),
        lambda: OR.merge_labels(labels.float(), torch.zeros((1, 65), dtype=torch.int32)),
        lambda: OR.merge_labels(labels, torch.zeros((2, 65), dtype=torch.int32)),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d was accepted" % i)


def test_push_masks_move_the_slot_and_never_pin_a_neighbour():
    labels = t(R.scene_labels(1, 32, 32))  # P = 8, a 4 x 4 grid: slot 1 on cells (0..1, 0..1), slot 2 on (0..1, 1..2), slot 3 on (2..3, 1..1)
    slots = torch.tensor([[1, 2, 3, 4, 0, 70]])
    active, passive, pushed = OR.push_masks(labels, slots, 8, k_active=2, k_passive=3)
    assert pushed.tolist() == [[1, 2, 3, 0, 0, 0]] and active.dtype == torch.bool and tuple(active.shape) == (1, 6, 32)
    cells = lambda m: [torch.nonzero(~r[16:])[:, 0].tolist() for r in m[0]]  # noqa: E731
    assert not active[..., :16].any() and not passive[..., :16].any()
    count = lambda s: (labels[0] == s).reshape(4, 8, 4, 8).sum((1, 3)).reshape(-1)  # noqa: E731
    for k, s in enumerate((1, 2, 3)):
        c = count(s)
        order = sorted(range(16), key=lambda i: (-int(c[i]), i))[:2]
        assert sorted(order) == cells(active)[k] and all(c[i] > 0 for i in order)
        occupied = (labels[0] > 0).reshape(4, 8, 4, 8).sum((1, 3)).reshape(-1) > 0
        ring = [i for i in range(16) if not occupied[i] and any(c[j] > 0 and max(abs(i // 4 - j // 4), abs(i % 4 - j % 4)) <= 1 for j in range(16))]
        assert cells(passive)[k] == ring[:3] and len(ring) >= 2
    assert cells(active)[3:] == [[], [], []] and cells(passive)[3:] == [[], [], []]
    g = torch.Generator().manual_seed(5)
    keys = torch.rand((1, 6, 16), generator=g)
    a2, _, _ = OR.push_masks(labels, slots, 8, k_active=2, k_passive=3, keys=keys)
    for k, s in enumerate((1, 2, 3)):
        touched = torch.nonzero(count(s) > 0)[:, 0].tolist()
        assert cells(a2)[k] == sorted(sorted(touched, key=lambda i: (-float(keys[0, k, i]), i))[:2])
