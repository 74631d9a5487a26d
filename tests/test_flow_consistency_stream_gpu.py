"""Stream ordering of `cwm_flow_consistency` (its stream is `base.stream` of the embedded cwm_patch_error_args, so the header gains no stream-taking name): the
protocols of tests/stream_order.py, imported and not edited -- A, late inputs and early consumers on a side stream, and C, two calls back to back behind a
delay without a host synchronisation between them.  The call is documented as asynchronous: it must return while the delay is still running.  Poison: NaN flows
(every pixel gets code 2).  Both directions and every output; the stats are the one table the call has to zero itself on the stream: in protocol C the second
call's stats buffer is a fresh one, and in the plain runs the buffers start from -9.  Float outputs are returned as their int32 bit patterns, since the masked
flow holds NaN and the protocols compare with torch.equal."""
import ctypes

import pytest
import torch

import flow_consistency_restatement as R
import stream_order as SO
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
B, H, W, P = 2, 64, 64, 8


def inputs(seed):
    """[a, o] on the device"""
    a, o, _, _ = R.case_random(B, H, W, seed=seed)
    return [torch.from_numpy(a).cuda(), torch.from_numpy(o).cuda()]


def call(a, o):
    """one call on the current stream, device tensors in and out and no synchronisation"""
    dev = a.device
    f32 = lambda *s: torch.full(s, -9.0, dtype=torch.float32, device=dev)  # noqa: E731
    code, res, masked, cell = torch.full((2, B, H, W), 99, dtype=torch.uint8, device=dev), f32(2, B, H, W), f32(2, B, 2, H, W), f32(2, B, H // P, W // P)
    stats = torch.full((2, B, 4), -9, dtype=torch.int32, device=dev)
    g = _lib.new_flow_consistency_args()
    _lib.fill_patch_args(g.base, geometry=(B, 1, 0, H, W, P), stream=_lib.current_stream_handle(dev))
    g.a_dev, g.o_dev = a.data_ptr(), o.data_ptr()
    g.a_strides[0], g.a_strides[1], g.o_strides[0], g.o_strides[1] = a.stride(0), a.stride(1), o.stride(0), o.stride(1)
    g.alpha, g.beta, g.both = 0.01, 0.5, 1
    g.code_dev, g.res_dev, g.masked_dev, g.cell_dev, g.stats_dev = (t.data_ptr() for t in (code, res, masked, cell, stats))
    _lib.check(_lib.get_lib().cwm_flow_consistency(ctypes.byref(g)))
    return [code, res.view(torch.int32), masked.view(torch.int32), cell.view(torch.int32), stats]


def plain2(truth):
    first, _ = SO.plain(call, [t.clone() for t in truth])
    want, ms = SO.plain(call, [t.clone() for t in truth])
    assert SO.same(first, want), "the plain run is not bit-stable run to run"
    return want, ms


def poison_of(truth):
    return [SO.poison_like(t) for t in truth]


def test_flow_consistency_late_inputs_and_early_consumers():
    truth = inputs(41)
    poison = poison_of(truth)
    want, ms = plain2(truth)
    assert int(want[4][..., :3].min()) >= 1 and int(want[4].sum()) == 2 * B * H * W  # every code occurs in every row and direction
    SO.check_poison("flow_consistency", truth, poison, want, call)
    SO.protocol_a("flow_consistency", call, truth, poison, want, ms, True)


def test_flow_consistency_back_to_back():
    t1, t2 = inputs(41), inputs(43)
    want1, ms = plain2(t1)
    want2, _ = plain2(t2)
    assert not SO.same(want1, want2)
    SO.protocol_c("flow_consistency", call, t1, t2, poison_of(t1), poison_of(t2), want1, want2, ms, True)
