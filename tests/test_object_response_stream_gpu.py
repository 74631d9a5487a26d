"""Stream ordering of `cwm_object_response` (its stream is `base.stream` of the embedded cwm_patch_error_args, so the header gains no stream-taking name): the
protocols of tests/stream_order.py, imported and not edited -- A, late inputs and early consumers on a side stream, and C, two calls back to back behind a
delay without a host synchronisation between them.  The call is documented as asynchronous: it must return while the delay is still running.  B = 2, K = 3,
S = 5, 64 x 64, the flows as the flow model leaves them ([R,S,2,H,W], read through the sample-outer view).  The protocols' input is the flows, and its poison is
NaN: every pixel becomes unusable, so only entry 7 of the tables counts and no sample is valid.  The slot map, the pushed slots and the shifts are integer
buffers, which the protocols do not poison; they stay what they are.  The table is an accumulation target the call has to zero itself on the stream: every call
takes fresh buffers that start from -9.  The coupling is returned as its int64 bit patterns."""
import ctypes

import pytest
import torch

import object_response_restatement as R
import stream_order as SO
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
B, K, S, H, W = 2, 3, 5, 64, 64
_FIXED = {}


def fixed():
    if not _FIXED:
        _, labels, pushed, dirs = R.case_scene(B, H, W, S)
        _FIXED.update(labels=torch.from_numpy(labels).cuda(), pushed=torch.from_numpy(pushed).cuda(), dirs=torch.from_numpy(dirs).cuda())
    return _FIXED


def inputs(seed):
    """[flows [R,S,2,H,W]] on the device: the scene, with a little noise that differs by seed"""
    flows = torch.from_numpy(R.case_scene(B, H, W, S)[0]).permute(0, 4, 1, 2, 3)
    noise = torch.randint(-64, 65, flows.shape, generator=torch.Generator().manual_seed(seed)).float() / 256
    return [(flows + noise).contiguous().cuda()]


def call(flows):
    """one call on the current stream, device tensors in and out and no synchronisation"""
    dev, m, Rr = flows.device, fixed(), B * K
    full = lambda shape, dtype: torch.full(shape, -9, dtype=dtype, device=dev)  # noqa: E731
    tab, valid, agg = full((Rr, S, 65, 8), torch.int64), full((Rr, S), torch.uint8), full((Rr, 65, 4), torch.int64)
    coupling, stats = full((Rr, 65, 4), torch.float64), full((Rr, 4), torch.int32)
    a = _lib.new_object_response_args()
    _lib.fill_patch_args(a.base, geometry=(B, K, 0, H, W, 0), stream=_lib.current_stream_handle(dev))
    a.flows_dev, a.S = flows.data_ptr(), S
    for i, st in enumerate((S * 2 * H * W, H * W, W, 1, 2 * H * W)):
        a.flow_strides[i] = st
    a.labels_dev, a.labels_strides[0], a.labels_strides[1] = m["labels"].data_ptr(), H * W, 0
    a.pushed_dev, a.dirs_dev = m["pushed"].data_ptr(), m["dirs"].data_ptr()
    a.min_q2, a.min_pixels, a.self_frac, a.move_frac = 256 * 256, 1, 0.5, 0.5
    a.tab_dev, a.valid_dev, a.agg_dev, a.coupling_dev, a.stats_dev = tab.data_ptr(), valid.data_ptr(), agg.data_ptr(), coupling.data_ptr(), stats.data_ptr()
    _lib.check(_lib.get_lib().cwm_object_response(ctypes.byref(a)))
    return [tab, valid, agg, coupling.view(torch.int64), stats]


def plain2(truth):
    first, _ = SO.plain(call, [t.clone() for t in truth])
    want, ms = SO.plain(call, [t.clone() for t in truth])
    assert SO.same(first, want), "the plain run is not bit-stable run to run"
    return want, ms


def poison_of(truth):
    return [SO.poison_like(t) for t in truth]


def test_object_response_late_inputs_and_early_consumers():
    truth = inputs(41)
    poison = poison_of(truth)
    want, ms = plain2(truth)
    tab, valid, stats = want[0], want[1], want[4]
    assert int(stats[:, 0].min()) == S - 1 and int(valid.sum()) == B * K * (S - 1) and int(tab[..., 7].sum()) == 0  # every row has valid samples
    assert int(tab[..., 0].sum()) == B * K * S * H * W
    SO.check_poison("object_response", truth, poison, want, call)
    SO.protocol_a("object_response", call, truth, poison, want, ms, True)


def test_object_response_back_to_back():
    t1, t2 = inputs(41), inputs(43)
    want1, ms = plain2(t1)
    want2, _ = plain2(t2)
    assert not SO.same(want1, want2)
    SO.protocol_c("object_response", call, t1, t2, poison_of(t1), poison_of(t2), want1, want2, ms, True)
