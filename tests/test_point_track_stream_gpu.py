"""Stream ordering of `cwm_point_track` (its stream is `base.stream` of the embedded cwm_patch_error_args, so the header gains no stream-taking name): the
protocols of tests/stream_order.py, imported and not edited -- A, late inputs and early consumers on a side stream, and C, two calls back to back behind a
delay without a host synchronisation between them.  The call is documented as asynchronous: it must return while the delay is still running.  B = 2, T = 6,
64 x 64, K = 257, every input and output in use.  The protocols' inputs are the forward flows and the points, and their poison is NaN: a NaN point is outside in
its start frame (state 2 throughout), a NaN flow is never usable, so every point coasts from its first step.  The slot maps, the models, the backward flows and
the starts stay what they are.  xy is returned as its int32 bit patterns."""
import ctypes

import pytest
import torch

import point_track_restatement as R
import stream_order as SO
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
B, T, H, W, K = 2, 6, 64, 64, 257
_FIXED = {}


def fixed():
    if not _FIXED:
        c = R.case_random(B, T, H, W, K, seed=51)
        _FIXED.update({k: torch.from_numpy(c[k]).cuda() for k in ("bwd", "labels", "model", "start")})
    return _FIXED


def inputs(seed):
    """[fwd, points] on the device"""
    c = R.case_random(B, T, H, W, K, seed=seed)
    return [torch.from_numpy(c["fwd"]).cuda(), torch.from_numpy(c["points"]).cuda()]


def call(fwd, points):
    """one call on the current stream, device tensors in and out and no synchronisation"""
    dev, m = fwd.device, fixed()
    xy = torch.full((B, T, K, 2), -7.0, device=dev)
    state, under, owner = (torch.full(s, 77, dtype=torch.uint8, device=dev) for s in ((B, T, K), (B, T, K), (B, K)))
    a = _lib.new_point_track_args()
    _lib.fill_patch_args(a.base, geometry=(B, T, 0, H, W, 0), stream=_lib.current_stream_handle(dev))
    a.fwd_dev, a.bwd_dev, a.labels_dev, a.model_dev = fwd.data_ptr(), m["bwd"].data_ptr(), m["labels"].data_ptr(), m["model"].data_ptr()
    a.points_dev, a.start_dev = points.data_ptr(), m["start"].data_ptr()
    for strides, t, n in ((a.fwd_strides, fwd, 3), (a.bwd_strides, m["bwd"], 3), (a.labels_strides, m["labels"], 2), (a.model_strides, m["model"], 2)):
        for i in range(n):
            strides[i] = t.stride(i)
    a.K, a.max_coast = K, 2
    a.xy_dev, a.state_dev, a.under_dev, a.owner_dev = xy.data_ptr(), state.data_ptr(), under.data_ptr(), owner.data_ptr()
    _lib.check(_lib.get_lib().cwm_point_track(ctypes.byref(a)))
    return [xy.view(torch.int32), state, under, owner]


def plain2(truth):
    first, _ = SO.plain(call, [t.clone() for t in truth])
    want, ms = SO.plain(call, [t.clone() for t in truth])
    assert SO.same(first, want), "the plain run is not bit-stable run to run"
    return want, ms


def poison_of(truth):
    return [SO.poison_like(t) for t in truth]


def test_point_track_late_inputs_and_early_consumers():
    truth = inputs(51)
    poison = poison_of(truth)
    want, ms = plain2(truth)
    state = want[1]
    assert all(int((state == v).sum()) > 0 for v in (0, 1, 2, 3, 255)) and int((want[2] > 0).sum()) > 0 and int((want[3] > 0).sum()) > 0
    SO.check_poison("point_track", truth, poison, want, call)
    SO.protocol_a("point_track", call, truth, poison, want, ms, True)


def test_point_track_back_to_back():
    t1, t2 = inputs(51), inputs(53)
    want1, ms = plain2(t1)
    want2, _ = plain2(t2)
    assert not SO.same(want1, want2)
    SO.protocol_c("point_track", call, t1, t2, poison_of(t1), poison_of(t2), want1, want2, ms, True)
