"""Stream ordering of `cwm_object_motion` (its stream is `base.stream` of the embedded cwm_patch_error_args, so the header gains no stream-taking name): the
protocols of tests/stream_order.py, imported and not edited -- A, late inputs and early consumers on a side stream, and C, two calls back to back behind a
delay without a host synchronisation between them.  The call is documented as asynchronous: it must return while the delay is still running.  B = 2, 64 x 64,
every input and output in use.  The protocols' input is the flow, and its poison is NaN: every pixel becomes class 2, so nothing is summed and no occluder is
counted.  The slot maps and the codes are byte maps, which the protocols do not poison; they stay what they are.  The three integer outputs are tables the call
has to zero itself on the stream: the buffers start from -9.  The model is returned as its int64 bit patterns."""
import ctypes

import pytest
import torch

import object_motion_restatement as R
import stream_order as SO
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
B, H, W = 2, 64, 64
_MAPS = {}


def maps():
    if not _MAPS:
        labels, _, code, other = R.case_random(B, H, W, seed=41, top=64)
        _MAPS.update(labels=torch.from_numpy(labels).cuda(), code=torch.from_numpy(code).cuda(), other=torch.from_numpy(other).cuda())
    return _MAPS


def inputs(seed):
    """[flow] on the device"""
    return [torch.from_numpy(R.case_random(B, H, W, seed=seed)[1]).cuda()]


def call(flow):
    """one call on the current stream, device tensors in and out and no synchronisation"""
    dev, m = flow.device, maps()
    full = lambda shape, dtype: torch.full(shape, -9, dtype=dtype, device=dev)  # noqa: E731
    sums, counts, model, occ = full((B, 65, 16), torch.int64), full((B, 65, 4), torch.int32), full((B, 65, 12), torch.float64), full((B, 65, 65), torch.int32)
    a = _lib.new_object_motion_args()
    _lib.fill_patch_args(a.base, geometry=(B, 1, 0, H, W, 0), stream=_lib.current_stream_handle(dev))
    a.labels_dev, a.flow_dev, a.code_dev, a.other_dev = m["labels"].data_ptr(), flow.data_ptr(), m["code"].data_ptr(), m["other"].data_ptr()
    for s in (a.labels_strides, a.code_strides, a.other_strides):
        s[0], s[1] = H * W, 0
    a.flow_strides[0], a.flow_strides[1], a.flow_strides[2] = flow.stride(0), 0, flow.stride(1)
    a.min_pixels, a.min_affine, a.min_det = 1, 16, 1.0
    a.sums_dev, a.counts_dev, a.model_dev, a.occ_dev = sums.data_ptr(), counts.data_ptr(), model.data_ptr(), occ.data_ptr()
    _lib.check(_lib.get_lib().cwm_object_motion(ctypes.byref(a)))
    return [sums, counts, model.view(torch.int64), occ]


def plain2(truth):
    first, _ = SO.plain(call, [t.clone() for t in truth])
    want, ms = SO.plain(call, [t.clone() for t in truth])
    assert SO.same(first, want), "the plain run is not bit-stable run to run"
    return want, ms


def poison_of(truth):
    return [SO.poison_like(t) for t in truth]


def test_object_motion_late_inputs_and_early_consumers():
    truth = inputs(41)
    poison = poison_of(truth)
    want, ms = plain2(truth)
    counts, occ = want[1], want[3]
    assert int(counts[:, :, 0].sum(1).min()) >= 1 and int(counts[:, :, 1].sum(1).min()) >= 1 and int(occ.sum((1, 2)).min()) >= 1  # in every row
    assert int(counts.sum()) == B * H * W
    SO.check_poison("object_motion", truth, poison, want, call)
    SO.protocol_a("object_motion", call, truth, poison, want, ms, True)


def test_object_motion_back_to_back():
    t1, t2 = inputs(41), inputs(43)
    want1, ms = plain2(t1)
    want2, _ = plain2(t2)
    assert not SO.same(want1, want2)
    SO.protocol_c("object_motion", call, t1, t2, poison_of(t1), poison_of(t2), want1, want2, ms, True)
