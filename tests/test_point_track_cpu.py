"""`point_track.track_torch` against the NumPy restatement (tests/point_track_restatement.py) for EQUALITY -- state, under and owner by value, xy as int32 bit
patterns, NaN included --, the properties of the passing scene, `start`, `grid_points`, the refusals of `_prepare` and the wiring into `track_sequence`.  No GPU.

The passing scene of the definition is 64 px wide and 8 frames long, and its square moves 4 px per frame: a point on the square's rightmost column (x = 19) is at
x = 47 in the last frame and cannot leave the frame, so "a point on the rightmost column leaves the frame and state 2 holds to the end" is asserted on the same
scene run for 14 frames (`case_passing(T=14)`: x = 63 in frame 11, on the last column and inside; 67 in frame 12), and its trajectory through the 8 frames is
asserted as well."""
import numpy as np
import pytest
import torch

import point_track_restatement as R
from counterfactualworldmodels_amd import point_track as PT, segment_track as ST

_CASES = {}


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def passing(T=8):
    if T not in _CASES:
        _CASES[T] = R.case_passing(T=T)
    return _CASES[T]


def run_torch(case, max_coast=8, **kw):
    r = PT.track(t(case["fwd"]), t(case["points"]), max_coast=max_coast, **{k: t(v) for k, v in kw.items()})
    assert isinstance(r, PT.PointTracks)
    return {k: getattr(r, k).numpy() for k in R.NAMES}


def equal(got, want, what=""):
    for k in R.NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, what, got[k].dtype, got[k].shape)
        assert np.array_equal(R.bits(got[k]), R.bits(want[k])), (k, what, np.argwhere(R.bits(got[k]) != R.bits(want[k]))[:4].tolist())


def test_passing_scene_equals_the_restatement():
    c = passing()
    for sub in R.SUBSETS:
        kw = R.pick(c, **sub)
        equal(run_torch(c, **kw), R.track(c["fwd"], c["points"], **kw), sub)


@pytest.mark.parametrize("shape", [(1, 2, 4, 4, 1), (2, 3, 20, 36, 63), (2, 5, 64, 64, 64), (1, 4, 36, 20, 65)])
def test_random_cases_equal_the_restatement_with_each_subset_of_the_inputs(shape):
    c = R.case_random(*shape, seed=sum(shape))
    seen = np.zeros(256, np.int64)
    for i, sub in enumerate(R.SUBSETS):
        kw, mc = R.pick(c, **sub), (8, 1, 0)[i % 3]
        want = R.track(c["fwd"], c["points"], max_coast=mc, **kw)
        equal(run_torch(c, max_coast=mc, **kw), want, (sub, mc))
        seen += np.bincount(want["state"].ravel(), minlength=256)
    if shape[4] > 1:
        assert all(seen[v] > 0 for v in (0, 1, 2, 255)) and (shape[1] < 3 or seen[3] > 0), seen[[0, 1, 2, 3, 255]]
        assert np.isnan(c["fwd"]).any() and (c["labels"] > 64).any() and np.isnan(c["model"]).any() and np.isnan(c["points"]).any()
        assert (c["points"][..., 0] == shape[3] - 1).any() and (c["points"][..., 1] == shape[2] - 1).any() and (np.nan_to_num(c["points"], posinf=0, neginf=0) % 1 == 0.5).any()


def test_the_point_on_the_square_passes_behind_the_pillar():
    c = passing()
    w = run_torch(c, **R.pick(c))
    assert w["state"][0, :, 0].tolist() == [0, 0, 0, 0, 0, 1, 1, 0] and w["owner"][0].tolist() == [1, 1, 0, 2]
    assert np.abs(w["xy"][0, :, 0, 0] - (12 + 4 * np.arange(8))).max() <= 1e-3 and (w["xy"][0, :, 0, 1] == 32).all()
    assert w["under"][0, :, 0].tolist() == [1, 1, 1, 1, 1, 2, 2, 1]
    # the static points stay where they are, visible
    assert not w["state"][0, :, 2:].any() and (w["xy"][0, :, 2] == [50, 8]).all() and (w["xy"][0, :, 3] == [35, 20]).all()
    # without the models the point coasts on its last believed flow vector, which is the same 4 px here
    assert np.array_equal(R.bits(run_torch(c, **R.pick(c, model=False))["xy"]), R.bits(w["xy"]))


def test_with_flows_only_the_point_stops_at_the_pillar():
    """the failure the feature exists to avoid"""
    c = passing()
    w = run_torch(c)
    assert w["xy"][0, 5:, 0, 0].tolist() == [32, 32, 32] and not w["state"][0, :, 0].any() and not w["under"].any() and not w["owner"].any()
    assert w["xy"][0, :5, 0, 0].tolist() == [12, 16, 20, 24, 28]


def test_max_coast_one_loses_the_point():
    c = passing()
    w = run_torch(c, max_coast=1, **R.pick(c))
    assert w["state"][0, :, 0].tolist() == [0, 0, 0, 0, 0, 1, 3, 3]
    assert (R.bits(w["xy"][0, 6:, 0]) == 0x7fc00000).all() and not w["under"][0, 6:, 0].any() and np.isfinite(w["xy"][0, :6, 0]).all()
    w = run_torch(c, max_coast=0, **R.pick(c))
    assert w["state"][0, :, 0].tolist() == [0, 0, 0, 0, 0, 3, 3, 3]


def test_a_point_on_the_rightmost_column_leaves_the_frame():
    c = passing()
    w = run_torch(c, **R.pick(c))
    assert w["xy"][0, :, 1, 0].tolist() == [19, 23, 27, 31, 35, 39, 43, 47] and w["state"][0, :, 1].tolist() == [0, 0, 0, 0, 1, 1, 0, 0]  # (47 < 63: still inside)
    c = passing(14)
    w = run_torch(c, **R.pick(c))
    equal(w, R.track(c["fwd"], c["points"], **R.pick(c)), "14 frames")
    assert w["state"][0, :, 1].tolist() == [0, 0, 0, 0, 1, 1] + [0] * 6 + [2, 2] and w["xy"][0, 11, 1].tolist() == [63, 32]
    assert (R.bits(w["xy"][0, 12:, 1]) == 0x7fc00000).all() and not w["under"][0, 12:, 1].any() and w["owner"][0, 1] == 1


def test_start():
    c = passing()
    start = np.array([[2, 0, 7, 5]], np.int32)
    pts = c["points"].copy()
    pts[0, 0] = [20, 32]  # where the point of the other tests is in frame 2
    w = run_torch(dict(c, points=pts), **dict(R.pick(c), start=start))
    assert w["state"][0, :, 0].tolist() == [255, 255, 0, 0, 0, 1, 1, 0] and w["owner"][0].tolist() == [1, 1, 0, 2]
    assert (R.bits(w["xy"][0, :2, 0]) == 0x7fc00000).all() and not w["under"][0, :2, 0].any() and w["xy"][0, 2:, 0, 0].tolist() == [20, 24, 28, 32, 36, 40]
    assert w["state"][0, :, 2].tolist() == [255] * 7 + [0] and w["state"][0, :, 3].tolist() == [255] * 5 + [0] * 3
    equal(w, R.track(c["fwd"], pts, **dict(R.pick(c), start=start)))
    # the restatement and the torch composition on another device never start a point whose start is outside; on CPU tensors it is refused
    never = R.track(c["fwd"], pts, start=np.array([[8, -1, 0, 0]], np.int32))
    assert (never["state"][0, :, :2] == 255).all() and not never["owner"][0, :2].any()
    for bad in (8, -1):
        with pytest.raises(ValueError, match="start"):
            PT.track(t(c["fwd"]), t(pts), start=torch.tensor([[0, bad, 0, 0]], dtype=torch.int32))


def test_grid_points():
    g = PT.grid_points(6, 10, 4)
    assert tuple(g.shape) == (1, 2, 2) and g.dtype == torch.float32 and g.is_contiguous() and g[0].tolist() == [[2, 2], [6, 2]]
    assert PT.grid_points(8, 8, 4, B=3, offset=0).shape == (3, 4, 2) and PT.grid_points(8, 8, 4, offset=0)[0].tolist() == [[0, 0], [4, 0], [0, 4], [4, 4]]
    every = PT.grid_points(3, 5, 1)
    assert tuple(every.shape) == (1, 15, 2) and every[0, 7].tolist() == [2, 1] and every[0, -1].tolist() == [4, 2]
    assert PT.grid_points(224, 224, 8).shape == (1, 784, 2) and PT.grid_points(224, 224, 1).shape == (1, 50176, 2)
    for bad in (dict(H=0, W=4, stride=1), dict(H=4, W=4, stride=0), dict(H=4, W=4, stride=2, offset=4), dict(H=4, W=4, stride=2, B=0)):
        with pytest.raises(ValueError, match="grid_points"):
            PT.grid_points(**bad)


def test_every_refusal_of_prepare():
    B, T, H, W, K = 2, 3, 6, 10, 5
    fwd, pts = torch.zeros((B, T - 1, 2, H, W)), torch.zeros((B, K, 2))
    lab, mod = torch.zeros((B, T, H, W), dtype=torch.uint8), torch.zeros((B, T, 65, 12), dtype=torch.float64)

    def refused(match, f=fwd, p=pts, **kw):
        for fn in (PT.track, PT.track_torch):
            with pytest.raises(ValueError, match=match):
                fn(f, p, **kw)

    refused("fwd must be", f=torch.zeros((B, 2, H, W)))
    refused("fwd must be", f=torch.zeros((B, T - 1, 3, H, W)))
    refused("fwd must be", f=None)
    refused("2 .. 4096 frames", f=torch.zeros((B, 0, 2, H, W)))
    refused("at most 2\\^18 pixels", f=torch.zeros((1, 1, 2, 512, 513)), p=torch.zeros((1, K, 2)))
    refused("fwd must be a float", f=torch.zeros((B, T - 1, 2, H, W), dtype=torch.int32))
    refused("points must be", p=torch.zeros((B, K, 3)))
    refused("points must be", p=torch.zeros((B + 1, K, 2)))
    refused("points must be", p=torch.zeros((K, 2)))
    refused("K = 0", p=torch.zeros((B, 0, 2)))
    refused("points must be a float", p=torch.zeros((B, K, 2), dtype=torch.int64))
    refused("bwd must be", bwd=torch.zeros((B, T, 2, H, W)))
    refused("bwd must be a float", bwd=torch.zeros((B, T - 1, 2, H, W), dtype=torch.uint8))
    refused("labels must be", labels=torch.zeros((B, T - 1, H, W), dtype=torch.uint8))
    refused("labels must be uint8", labels=torch.zeros((B, T, H, W), dtype=torch.int32))
    refused("model is given without labels", model=mod)
    refused("model must be", labels=lab, model=torch.zeros((B, T - 1, 65, 12), dtype=torch.float64))
    refused("model must be float64", labels=lab, model=mod.float())
    refused("start must be", start=torch.zeros((B, K + 1), dtype=torch.int32))
    refused("start must be int32", start=torch.zeros((B, K)))
    refused("start must lie", start=torch.full((B, K), T, dtype=torch.int32))
    for bad in (-0.1, float("nan"), float("inf")):
        refused("alpha", alpha=bad)
        refused("beta", beta=bad)
    refused("max_coast", max_coast=-1)
    refused("is on", p=torch.zeros((B, K, 2), device="meta"))
    refused("is on", labels=torch.zeros((B, T, H, W), dtype=torch.uint8, device="meta"))
    # negative strides (a flipped view) are read through a copy, not refused and not handed on
    r = PT.track(fwd.flip(1), pts, bwd=fwd.flip(0), labels=lab.flip(1), model=mod.flip(0))
    assert tuple(r.xy.shape) == (B, T, K, 2) and tuple(r.state.shape) == (B, T, K) and tuple(r.under.shape) == (B, T, K) and tuple(r.owner.shape) == (B, K)
    assert r.xy.dtype == torch.float32 and r.state.dtype == r.under.dtype == r.owner.dtype == torch.uint8
    with pytest.raises(RuntimeError):
        PT.track_device(fwd, pts)


def sequence_inputs():
    c = passing()
    fwd, bwd = t(c["fwd"]), t(c["bwd"])
    z = torch.zeros_like(fwd[:, :1])
    return c, t(c["labels"]), torch.cat([z, bwd], 1), torch.cat([z, fwd], 1)


def test_track_sequence_fills_points():
    c, labels, backs, fwds = sequence_inputs()
    pts = t(c["points"])
    ts = ST.track_sequence(labels, backs, fwds, motion=True, points=pts)
    assert isinstance(ts.points, PT.PointTracks) and torch.equal(ts.labels, labels)  # (labels 1 and 2 are born into slots 1 and 2 and linked from then on)
    direct = PT.track(fwds[:, 1:], pts, bwd=backs[:, 1:], labels=ts.labels, model=ts.motion)
    for k in R.NAMES:
        assert np.array_equal(R.bits(getattr(ts.points, k).numpy()), R.bits(getattr(direct, k).numpy())), k
    assert ts.points.state[0, :, 0].tolist() == [0, 0, 0, 0, 0, 1, 1, 0] and ts.points.xy[0, :, 0, 0].tolist() == [12 + 4 * i for i in range(8)]
    # keywords reach the call; without motion the point coasts on its last believed vector
    lost = ST.track_sequence(labels, backs, fwds, motion=True, points=pts, point_kwargs=dict(max_coast=1, start=torch.tensor([[0, 1, 0, 0]], dtype=torch.int32)))
    assert lost.points.state[0, :, 0].tolist() == [0, 0, 0, 0, 0, 1, 3, 3] and int(lost.points.state[0, 0, 1]) == 255
    bare = ST.track_sequence(labels, backs, fwds, points=pts)
    assert bare.motion is None and bare.points.state[0, :, 0].tolist() == [0, 0, 0, 0, 0, 1, 1, 0]


def test_points_off_changes_nothing_and_refusals():
    c, labels, backs, fwds = sequence_inputs()
    pts = t(c["points"])
    for kw in (dict(), dict(fwd_flows=fwds), dict(fwd_flows=fwds, motion=True)):
        plain, off = ST.track_sequence(labels, backs, **kw), ST.track_sequence(labels, backs, points=None, point_kwargs=dict(max_coast=1), **kw)
        assert plain.points is None and off.points is None
        on = ST.track_sequence(labels, backs, points=pts, **kw) if kw else None
        for k in ST.TrackedScene.__slots__:
            if k != "points":
                for other in (off, on):
                    u, v = getattr(plain, k), None if other is None else getattr(other, k)
                    if other is not None:
                        assert (u is None) == (v is None), k
                        if torch.is_tensor(u):
                            assert torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u, v.view(torch.int64) if v.dtype == torch.float64 else v), k
    with pytest.raises(ValueError, match="fwd_flows"):
        ST.track_sequence(labels, backs, points=pts)
    with pytest.raises(ValueError, match="two frames"):
        ST.track_sequence(labels[:, :1], backs[:, :1], backs[:, :1], points=pts)
    with pytest.raises(ValueError, match="occlusion"):
        ST.track_scene(None, torch.zeros((1, 3, 3, 32, 48)), points=pts, occlusion=False)


def test_points_make_no_further_flow_consistency_or_motion_call(monkeypatch):
    from counterfactualworldmodels_amd import flow_consistency as FC, object_motion as OM

    c, labels, backs, fwds = sequence_inputs()
    seen = []
    real_check, real_measure, real_track = FC.check, OM.measure, PT.track
    monkeypatch.setattr(FC, "check", lambda *a, **kw: (seen.append("check"), real_check(*a, **kw))[1])
    monkeypatch.setattr(OM, "measure", lambda *a, **kw: (seen.append("measure"), real_measure(*a, **kw))[1])
    monkeypatch.setattr(PT, "track", lambda *a, **kw: (seen.append("track"), real_track(*a, **kw))[1])
    ST.track_sequence(labels, backs, fwds, motion=True)
    ST.track_sequence(labels, backs, fwds, motion=True, points=t(c["points"]))
    assert seen == ["check", "measure", "check", "measure", "track"]


def test_track_points_of_the_generator_takes_given_flows_and_a_scene():
    from counterfactualworldmodels_amd import segmentation

    c, labels, backs, fwds = sequence_inputs()
    pts = t(c["points"])
    ts = ST.track_sequence(labels, backs, fwds, motion=True)
    calls = []

    class Stub:
        def predict_flow(self, x, backward=False, **kw):
            calls.append((backward, kw))
            return backs[:, 1:].flip(1) if backward else fwds[:, 1:]

    x = torch.zeros((1, 8, 3, 64, 64))
    given = segmentation.FlowGenerator.track_points(Stub(), x, pts, scene=ts, flows=(fwds[:, 1:], backs[:, 1:]))
    made = segmentation.FlowGenerator.track_points(Stub(), x, pts, scene=ts, iters=3)
    assert calls == [(False, dict(iters=3)), (True, dict(iters=3))]
    for r in (given, made):
        assert r.state[0, :, 0].tolist() == [0, 0, 0, 0, 0, 1, 1, 0]
    no_scene = segmentation.FlowGenerator.track_points(Stub(), x, pts, flows=(fwds[:, 1:], backs[:, 1:]), max_coast=2)
    direct = PT.track(fwds[:, 1:], pts, bwd=backs[:, 1:], max_coast=2)
    assert not no_scene.under.any() and torch.equal(no_scene.state, direct.state) and torch.equal(no_scene.xy.view(torch.int32), direct.xy.view(torch.int32))
    assert no_scene.state[0, :, 0].tolist() == [0, 0, 0, 0, 0, 1, 0, 0]  # (no slot maps: the coast is seen, and the pillar's zero flow is then believed)
