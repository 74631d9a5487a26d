"""`segment_track.track_step_torch` and `track_sequence` on CPU tensors against the NumPy restatement (tests/segment_track_restatement.py), for EQUALITY: every
output is an integer, the warp is one float32 add per coordinate and the link test one float32 multiply and one compare on both sides.  No GPU."""
import numpy as np
import pytest
import torch

import segment_track_restatement as TR
from counterfactualworldmodels_amd import segment_track as ST

NAMES = ("out", "track_id", "age", "next_id", "area", "bbox", "moments", "slot_of_cur", "linked_cur", "table", "warped", "stats")


def to_state(prev, state):
    if prev is None and state is None:
        return None
    st = TR.empty_state(len(prev)) if state is None else state
    return ST.TrackState(None if prev is None else torch.from_numpy(prev), *(torch.from_numpy(st[k]) for k in ("track_id", "age", "next_id")))


def as_dict(r):
    d = {k: getattr(r, k) for k in ("area", "bbox", "moments", "slot_of_cur", "linked_cur", "table", "warped", "stats")}
    d.update(out=r.state.labels, track_id=r.state.track_id, age=r.state.age, next_id=r.state.next_id)
    return {k: v.numpy() for k, v in d.items()}


def equal(got, want, what=""):
    for k in NAMES:
        assert got[k].dtype == want[k].dtype, (k, got[k].dtype, what)
        assert np.array_equal(got[k], want[k]), (k, what)


def check(prev, cur, flow, state, shape=None, **kw):
    shape = shape or next(m for m in (prev, cur) if m is not None).shape
    want = TR.track(prev, cur, flow, state, shape, **kw)
    r = ST.track_step(to_state(prev, state), None if cur is None else torch.from_numpy(cur), None if flow is None else torch.from_numpy(flow), want_table=True,
                      want_warped=True, shape=shape, **kw)
    equal(as_dict(r), want, kw)
    return want


def test_hand_worked_case():
    """8 x 12, two tracks and three labels; iou_thresh 0.3, min_inter 1, min_area 2, max_age 1, carry on.
    prev: slot 1 = rows 0-3 x cols 1-4 (id 7), slot 3 = rows 4-7 x cols 8-11 (id 9), ages 0, next_id 10.  flow u = +1: pixel (y, x) looks at (y, x + 1), so w has slot 1
    at rows 0-3 x cols 0-3 and slot 3 at rows 4-7 x cols 7-10 (column 11 looks outside).  cur: label 1 = rows 0-3 x cols 0-4 (20 px), label 2 = rows 5-7 x cols 0-2
    (9 px), label 3 = the pixel (0, 11).
    Call 1: n[1][1] = 16 > .3 * (20 + 16 - 16): label 1 is LINKED to slot 1.  Slot 3 meets no label, has 16 warped pixels and age 0 + 1 <= 1: it COASTS (age 1).
    Label 2 is BORN into slot 2, the lowest free one, as id 10; label 3 is below min_area and dropped.  45 pixels are painted; track_id (7, 10, 9), next_id 11.
    Call 2 on call 1's output, no flow, the same labels: (1, 1) and (2, 2) link, slot 3 would reach age 2 > 1 and ENDS; track_id (7, 10, 0), 29 pixels."""
    prev, cur, flow, state = TR.hand_worked()
    w1 = check(prev, cur, flow, state, **TR.HAND_KW)
    w2 = check(w1["out"], cur, None, TR.new_state(w1), **TR.HAND_KW)
    for w, hand in ((w1, TR.HAND[0]), (w2, TR.HAND[1])):
        assert w["track_id"][0, :3].tolist() == hand["track_id"] and w["age"][0, :3].tolist() == hand["age"] and w["next_id"].tolist() == hand["next_id"]
        assert w["stats"].tolist() == hand["stats"] and w["area"][0, :3].tolist() == hand["area"] and w["bbox"][0, :3].tolist() == hand["bbox"]
        assert w["moments"][0, :3].tolist() == hand["moments"] and w["slot_of_cur"][0, :3].tolist() == hand["slot_of_cur"]
        assert w["linked_cur"][0, :3].tolist() == hand["linked_cur"] and not w["track_id"][0, 3:].any()
    assert w1["table"][0, 1, 1] == 16 and w1["table"][0, 0, 3] == 16 and w1["table"][0, 0, 0] == 50 and w1["table"][0, 2, 0] == 9
    assert np.count_nonzero(w1["out"] == 3) == 16 and (w1["out"][0, 4:8, 7:11] == 3).all()


@pytest.mark.parametrize("kind", ["int", "half", "frac", "special"])
@pytest.mark.parametrize("H,W", [(8, 12), (20, 12), (24, 40), (64, 64)])
def test_random_rectangles(H, W, kind):
    B = 3
    prev, cur, state = TR.random_maps(H * 7 + W, B, H, W, n_prev=6, n_cur=7)
    flow = TR.flows(kind, H + W, B, H, W)
    want = check(prev, cur, flow, state, iou_thresh=0.25, max_age=2)
    if kind == "int":
        assert want["stats"][:, 0].max() >= 1, "no link in any row"
        assert not np.array_equal(want["out"][0], want["out"][1])
    check(prev, cur, flow, state, iou_thresh=0.25, min_inter=3, min_area=5, max_age=1)


def test_half_integer_flows_round_to_even():
    prev = np.zeros((1, 8, 12), np.uint8)
    prev[0, :, 2], prev[0, :, 3], prev[0, :, 4] = 1, 2, 3
    state = TR.empty_state(1)
    state["track_id"][0, :3] = (5, 6, 7)
    flow = np.zeros((1, 2, 8, 12), np.float32)
    flow[0, 0] = 0.5  # x + 0.5: x = 1 -> 1.5 -> 2, x = 2 -> 2.5 -> 2, x = 3 -> 3.5 -> 4, x = 4 -> 4.5 -> 4, x = 5 -> 5.5 -> 6: slot 2 (column 3) is never seen
    want = check(prev, None, flow, state)
    assert want["warped"][0, 0].tolist() == [0, 1, 1, 3, 3, 0, 0, 0, 0, 0, 0, 0]


def test_bytes_above_64_count_as_zero():
    prev, cur, state = TR.random_maps(5, 2, 24, 40, big_bytes=False)
    prev[:, :3], cur[:, -3:] = 65, 255
    want = check(prev, cur, None, state)
    assert not want["warped"][:, :3].any() and not want["out"][:, -3:][want["warped"][:, -3:] == 0].any()


def test_full_slot_table_drops_births():
    prev, cur, state = TR.full_table(2, 8, 64)
    want = check(prev, cur, None, state, max_age=5)
    assert want["stats"][:, :6].tolist() == [[0, 0, 64, 0, 2, 64]] * 2 and want["next_id"].tolist() == [900, 900] and not want["slot_of_cur"].any()
    want = check(prev, cur, None, state, carry=0)  # every track ends: both labels are born into slots 1 and 2
    assert want["stats"][:, :6].tolist() == [[0, 2, 0, 64, 0, 2]] * 2 and want["slot_of_cur"][0, :2].tolist() == [1, 2] and want["next_id"].tolist() == [902, 902]


def test_thresholds_and_ages():
    prev, cur, state = TR.random_maps(11, 2, 24, 40, n_prev=6, n_cur=6)
    flow = TR.flows("int", 3, 2, 24, 40)
    linked = check(prev, cur, flow, state, iou_thresh=0.0)["stats"][:, 0]
    assert linked.min() >= 1
    assert check(prev, cur, flow, state, iou_thresh=float("nan"))["stats"][:, 0].tolist() == [0, 0]  # a NaN threshold links nothing
    assert check(prev, cur, flow, state, iou_thresh=float("nan"), max_age=0)["stats"][:, 2].tolist() == [0, 0]  # max_age 0: nothing coasts
    assert check(prev, cur, flow, state, iou_thresh=float("nan"), max_age=9)["stats"][:, 2].min() >= 1
    assert check(prev, cur, flow, state, iou_thresh=float("nan"), max_age=9, carry=0)["stats"][:, 2].tolist() == [0, 0]
    check(prev, cur, flow, state, iou_thresh=0.9, min_inter=0, min_area=0)


def test_missing_inputs():
    prev, cur, state = TR.random_maps(12, 2, 20, 12)
    flow = TR.flows("int", 4, 2, 20, 12)
    want = check(prev, None, flow, state)  # no segmentation: pure propagation
    assert want["stats"][:, 0].tolist() == [0, 0] and want["stats"][:, 1].tolist() == [0, 0] and want["stats"][:, 2].min() >= 1
    assert ((want["out"] == want["warped"]) | (want["out"] == 0)).all() and want["out"].any()
    want = check(None, cur, flow, state)  # no previous frame: the live tracks end, every label is born
    assert want["stats"][:, 0].tolist() == [0, 0] and want["stats"][:, 1].min() >= 2 and not want["warped"].any()
    a = check(None, cur, None, None)  # an empty state through NULL pointers ...
    b = check(None, cur, None, TR.empty_state(2))  # ... and through zeros
    equal(a, b)
    assert a["track_id"][0, :int(a["stats"][0, 1])].tolist() == list(range(1, int(a["stats"][0, 1]) + 1))
    check(prev, cur, flow, None)  # a previous map without a state: every slot byte counts as 0
    check(None, None, None, state, shape=(2, 20, 12))


def test_garbage_state():
    prev, cur, _ = TR.random_maps(13, 3, 24, 40)
    check(prev, cur, TR.flows("special", 5, 3, 24, 40), TR.garbage_state(1, 3), max_age=3)


def test_track_sequence_against_the_restatement():
    B, T, H, W = 2, 5, 24, 40
    maps, flows = [], np.zeros((B, T, 2, H, W), np.float32)
    base = np.stack([TR.rect(H, W, 2, 10, 3, 13, 1) + TR.rect(H, W, 12, 20, 20, 30, 2), TR.rect(H, W, 0, 6, 0, 9, 2) + TR.rect(H, W, 8, 19, 11, 31, 1)])
    for t in range(T):  # (no rectangle reaches the border within the movie: np.roll does not wrap one around)
        maps.append(np.roll(base, (t, 2 * t), (1, 2)))
        flows[:, t, 0], flows[:, t, 1] = -2, -1  # the content moves by (+1, +2) per frame
    given = [maps[0], maps[1], None, maps[3], None]
    want = TR.sequence(given, flows, (B, H, W), max_age=2)
    got = ST.track_sequence([None if m is None else torch.from_numpy(m) for m in given], torch.from_numpy(flows), max_age=2)
    for t in range(T):
        for k, name in (("out", "labels"), ("track_id", "track_id"), ("age", "age"), ("area", "area"), ("bbox", "bbox"), ("moments", "moments"), ("stats", "stats")):
            assert np.array_equal(getattr(got, name)[:, t].numpy(), want[t][k]), (t, k)
    assert np.array_equal(got.next_id.numpy(), want[-1]["next_id"])
    # a [B,T,H,W] tensor is the same sequence
    full = ST.track_sequence(torch.from_numpy(np.stack(maps, 1)), torch.from_numpy(flows), max_age=2)
    want_full = TR.sequence(maps, flows, (B, H, W), max_age=2)
    assert all(np.array_equal(full.labels[:, t].numpy(), want_full[t]["out"]) for t in range(T))
    ids = full.track_id.numpy()
    assert all((ids[:, t] == ids[:, 0]).all() for t in range(T)) and ids[:, 0, :2].tolist() == [[1, 2], [1, 2]], "ids persist while the content shifts"
    assert got.track_id[:, 4, :2].tolist() == [[1, 2], [1, 2]] and got.age[:, 4, :2].tolist() == [[1, 1], [1, 1]] and got.age[:, 2, :2].tolist() == [[1, 1], [1, 1]]


def test_python_refuses_before_allocating():
    z = torch.zeros((1, 8, 12), dtype=torch.uint8)
    for bad, kw in ((torch.zeros((1, 10, 12), dtype=torch.uint8), {}), (z, dict(max_age=-1)), (z, dict(min_inter=-1)), (z, dict(min_area=-1)), (z, dict(carry=2)),
                    (torch.zeros((1, 512, 516), dtype=torch.uint8), {})):
        with pytest.raises(ValueError, match="segment_track"):
            ST.track_step(None, bad, None, **kw)
    with pytest.raises(ValueError, match="flow must be"):
        ST.track_step(None, z, torch.zeros((1, 2, 8, 8)))
