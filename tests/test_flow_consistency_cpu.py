"""`flow_consistency.check_torch` and the occlusion-aware `track_sequence` on CPU tensors against the NumPy restatement (tests/flow_consistency_restatement.py),
for EQUALITY: floats are compared as bit patterns, so NaN and the sign of zero count.  No GPU."""
import numpy as np
import pytest
import torch

import flow_consistency_restatement as R
import segment_track_restatement as TR
from counterfactualworldmodels_amd import flow_consistency as FC
from counterfactualworldmodels_amd import segment_track as ST

FIELD = dict(code="code", res="res", masked="masked", cell="cells", stats="stats")


def equal(got, want, what=""):
    for k in R.NAMES:
        g, w = getattr(got, FIELD[k]), want[k]
        assert (g is None) == (w is None), (k, what)
        if w is not None:
            g = g.numpy()
            assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, g.shape, w.shape, what)
            assert np.array_equal(R.bits(g), R.bits(w)), (k, what)


def check(a, o, alpha, beta, P=0, both=True, what=""):
    want = R.consistency(a, o, alpha, beta, P, both)
    got = FC.check(torch.from_numpy(a), torch.from_numpy(o), alpha=alpha, beta=beta, P=P, both=both, want_res=True, want_masked=True, want_cells=bool(P))
    if not both:
        want = {k: None if v is None else v[0] for k, v in want.items()}
    equal(got, want, what)
    return want


@pytest.mark.parametrize("name", sorted(R.CASES))
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_every_shared_case(H, W, name):
    for B in (1, 3):
        a, o, alpha, beta = R.CASES[name](B, H, W)
        P = 4 if H % 8 or W % 8 else 8
        check(a, o, alpha, beta, P=P, what=(name, B))
        check(a, o, alpha, beta, both=False, what=(name, B))


def test_what_the_cases_are_for():
    B, H, W = 2, 24, 40
    w = check(*R.case_consistent(B, H, W))
    inside = w["code"][0] != 2
    assert inside.sum() == B * (H - 1) * (W - 2) and not w["code"][0][inside].any() and not w["res"][0][inside].any()
    a, o, alpha, beta = R.case_half(B, H, W)
    assert ((a - np.floor(a)) == 0.5).all()
    w = check(a, o, alpha, beta)
    assert all((w["code"][0] == k).any() for k in range(3))
    w = check(*R.case_threshold(B, H, W), both=False)  # res == thr: consistent
    assert not w["code"][:, :, :W - 1].any() and (w["res"][:, :, :W - 1] == 0.25).all() and (w["code"][:, :, W - 1] == 2).all()
    w = check(*R.case_threshold(B, H, W, beta=R.BETA_BELOW), both=False)  # the next smaller beta: inconsistent
    assert (w["code"][:, :, :W - 1] == 1).all() and R.BETA_BELOW < 0.25
    w = check(*R.case_border(B, H, W), both=False)
    assert (w["code"][:, :4] != 2).all(), "targets exactly on the border are inside"
    w = check(*R.case_border(B, H, W, ulp=True), both=False)
    assert (w["code"][:, 0, :4] == 2).all() and (w["code"][:, 0, 4:] != 2).all(), "one ulp outside"
    w = check(*R.case_hostile_a(B, H, W), both=False)
    assert (w["code"] == 2).all() and np.isposinf(w["res"]).all() and (R.bits(w["masked"]) == 0x7fc00000).all() and w["stats"].tolist() == [[0, 0, H * W, 0]] * B
    a, o, alpha, beta = R.case_hostile_o(B, H, W)
    w = check(a, o, alpha, beta, both=False)
    clean = R.one_direction(a, np.nan_to_num(o, nan=0.0, posinf=0.0, neginf=0.0), alpha, beta)
    hit = (w["code"] == 1) & (clean["res"] != w["res"]) & np.isposinf(w["res"])
    assert hit.sum() > 50 and (R.bits(w["masked"][:, 0])[hit] == 0x7fc00000).all()
    a, o, alpha, beta = R.case_random(B, 64, 64)
    fused = R.one_direction(a, o, alpha, beta, contract=True)["res"]
    plain = R.one_direction(a, o, alpha, beta)["res"]
    assert (R.bits(fused) != R.bits(plain)).sum() > 1000, "thousands of pixels whose res bits differ under one fused multiply-add"
    w = check(a, o, alpha, beta, P=8)
    assert all((w["code"] == k).sum() > 100 for k in range(3)) and w["stats"].sum() == 2 * B * 64 * 64 and 0 < w["cell"].min() < w["cell"].max() <= 1


def test_a_movie_is_one_call_over_its_pairs_and_views_are_read_in_place():
    B, T, H, W = 2, 3, 8, 12
    a, o, alpha, beta = R.case_random(B * T, H, W, reach=3.0)
    want = R.consistency(a, o, alpha, beta, 4, True)
    got = FC.check(torch.from_numpy(a).view(B, T, 2, H, W), torch.from_numpy(o).view(B, T, 2, H, W), P=4, both=True, want_res=True, want_masked=True, want_cells=True)
    assert tuple(got.code.shape) == (2, B, T, H, W) and tuple(got.masked.shape) == (2, B, T, 2, H, W) and tuple(got.stats.shape) == (2, B, T, 4)
    for k in R.NAMES:
        assert np.array_equal(R.bits(getattr(got, FIELD[k]).reshape(want[k].shape).numpy()), R.bits(want[k])), k
    wide = torch.full((B * T, 5, H, W), float("nan"))
    wide[:, 1::2] = torch.from_numpy(a)
    got = FC.check(wide[:, 1::2], torch.from_numpy(o).flip(0).flip(0))
    assert got.res is None and got.masked is None and got.cells is None and np.array_equal(got.code.numpy(), want["code"][0])


def test_python_refuses_before_allocating():
    z = torch.zeros((1, 2, 8, 12))
    for a, o, kw in ((torch.zeros((1, 2, 10, 12)), torch.zeros((1, 2, 10, 12)), {}), (torch.zeros((1, 2, 512, 516)), torch.zeros((1, 2, 512, 516)), {}),
                     (z, torch.zeros((1, 2, 8, 8)), {}), (torch.zeros((1, 3, 8, 12)), torch.zeros((1, 3, 8, 12)), {}), (z[0], z[0], {}),
                     (z, z, dict(alpha=-1.0)), (z, z, dict(beta=float("inf"))), (z, z, dict(alpha=float("nan"))), (z, z, dict(want_cells=True)),
                     (z, z, dict(want_cells=True, P=5)), (z, z, dict(want_cells=True, P=8))):
        with pytest.raises(ValueError, match="flow_consistency"):
            FC.check(a, o, **kw)
    with pytest.raises(ValueError, match="fwd_flows"):
        ST.track_sequence(torch.zeros((1, 2, 8, 12), dtype=torch.uint8), None, fwd_flows=torch.zeros((1, 2, 2, 8, 12)))
    with pytest.raises(ValueError, match="fwd_flows"):
        ST.track_sequence(torch.zeros((1, 2, 8, 12), dtype=torch.uint8), torch.zeros((1, 2, 2, 8, 12)), fwd_flows=torch.zeros((1, 3, 2, 8, 12)))


def movie():
    """two overlapping rectangles that move 2 px to the right per frame over a static background.  The strip they uncover has no true backward flow; the flow
    given here answers 0 there, as for the background around it, so the warp finds the object's slot at the same place in the previous frame: the smear.  The
    forward flow of that place is the object's (+2), so the strip fails the round trip.  Frames 0 and 2 are segmented, 1 and 3 are carried"""
    B, T, H, W = 2, 4, 24, 40
    maps, back, fwd = [], np.zeros((B, T, 2, H, W), np.float32), np.zeros((B, T, 2, H, W), np.float32)
    where = []
    for t in range(T):
        m = np.stack([TR.rect(H, W, 4, 14, 5 + 2 * t, 15 + 2 * t, 1), TR.rect(H, W, 8, 20, 3 + 2 * t, 9 + 2 * t, 2)])
        where.append(m > 0)
        maps.append(m if t % 2 == 0 else None)
    for t in range(1, T):
        back[:, t, 0] = np.where(where[t], -2, 0)
        fwd[:, t, 0] = np.where(where[t - 1], 2, 0)
    fwd[:, 0], back[:, 0] = np.nan, np.nan  # entry 0 is not read
    return maps, back, fwd, where


def test_track_sequence_with_forward_flows_against_the_loop_composed_by_hand():
    maps, back, fwd, where = movie()
    B, T, H, W = back.shape[0], back.shape[1], back.shape[3], back.shape[4]
    want, state, prev = [], None, None
    for t, cur in enumerate(maps):
        flow = None if t == 0 else R.one_direction(back[:, t], fwd[:, t], 0.01, 0.5)["masked"]
        want.append(TR.track(prev, cur, flow, state, (B, H, W), max_age=2))
        state, prev = TR.new_state(want[-1]), want[-1]["out"]
    tensors = [None if m is None else torch.from_numpy(m) for m in maps]
    got = ST.track_sequence(tensors, torch.from_numpy(back), fwd_flows=torch.from_numpy(fwd), max_age=2)
    plain = ST.track_sequence(tensors, torch.from_numpy(np.nan_to_num(back)), max_age=2)
    for t in range(T):
        for k, name in (("out", "labels"), ("track_id", "track_id"), ("age", "age"), ("area", "area"), ("bbox", "bbox"), ("moments", "moments"), ("stats", "stats")):
            assert np.array_equal(getattr(got, name)[:, t].numpy(), want[t][k]), (t, k)
    for t in (1, 3):  # a carried frame: the strip the object has just left is 0 with the check and painted without it; the object itself is carried either way
        strip = where[t - 1] & ~where[t]
        assert strip.any() and not got.labels[:, t].numpy()[strip].any() and plain.labels[:, t].numpy()[strip].all()
        assert got.labels[:, t].numpy()[where[t]].all()


def test_track_sequence_without_forward_flows_is_what_it_was():
    maps, back, _, _ = movie()
    back = np.nan_to_num(back)
    B, T, H, W = back.shape[0], back.shape[1], back.shape[3], back.shape[4]
    want = TR.sequence(maps, back, (B, H, W), max_age=2)
    got = ST.track_sequence([None if m is None else torch.from_numpy(m) for m in maps], torch.from_numpy(back), max_age=2)
    same = ST.track_sequence([None if m is None else torch.from_numpy(m) for m in maps], torch.from_numpy(back), fwd_flows=None, occ_alpha=9.0, max_age=2)
    for t in range(T):
        for k, name in (("out", "labels"), ("track_id", "track_id"), ("age", "age"), ("area", "area"), ("bbox", "bbox"), ("moments", "moments"), ("stats", "stats")):
            assert np.array_equal(getattr(got, name)[:, t].numpy(), want[t][k]) and torch.equal(getattr(got, name), getattr(same, name)), (t, k)
