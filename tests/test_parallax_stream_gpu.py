"""Stream ordering of `cwm_parallax` (its stream is `base.stream` of the embedded cwm_patch_error_args, so the header gains no stream-taking name): the
protocols of tests/stream_order.py, imported and not edited -- A, late inputs and early consumers on a side stream, and C, two calls back to back behind a
delay without a host synchronisation between them.  The call is documented as asynchronous: it must return while the delay is still running.  R = 3, S = 5,
64 x 64, the flows as the flow model leaves them ([R,S,2,H,W], read through the sample-outer view), no dirs: all three kernels run and the reference sums are
gathered in ref_dev.  The protocols' input is the flows, and its poison is NaN: no pixel is usable, no sample live, every pixel lands in n_bad.  The slot map is
an integer buffer, which the protocols do not poison.  The histogram, the slot table and ref are accumulation targets the call has to zero itself on the stream:
every call takes fresh buffers that start from -9.  The float outputs are returned as their integer bit patterns."""
import ctypes

import pytest
import torch

import parallax_restatement as R
import stream_order as SO
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
RR, S, H, W = 3, 5, 64, 64
_FIXED = {}


def fixed():
    if not _FIXED:
        _FIXED.update(labels=torch.from_numpy(R.plane_labels(RR, H, W)).cuda())
    return _FIXED


def inputs(seed):
    """[flows [R,S,2,H,W]] on the device: the three planes, with a little noise that differs by seed"""
    flows = torch.from_numpy(R.case_planes(RR, H, W, S)[0]).permute(0, 4, 1, 2, 3)
    noise = torch.randint(-64, 65, flows.shape, generator=torch.Generator().manual_seed(seed)).float() / 256
    return [(flows + noise).contiguous().cuda()]


def call(flows):
    """one call on the current stream, device tensors in and out and no synchronisation"""
    dev, m = flows.device, fixed()
    full = lambda shape, dtype: torch.full(shape, -9, dtype=dtype, device=dev)  # noqa: E731
    par, spread, off, cnt = full((RR, H, W), torch.float32), full((RR, H, W), torch.float32), full((RR, H, W), torch.float32), full((RR, H, W), torch.uint8)
    ref, hist, tab = full((RR, S, 4), torch.float64), full((RR, 65, 256), torch.int32), full((RR, 65, 8), torch.int32)
    a = _lib.new_parallax_args()
    _lib.fill_patch_args(a.base, geometry=(RR, 1, 0, H, W, 0), stream=_lib.current_stream_handle(dev))
    a.flows_dev, a.S = flows.data_ptr(), S
    for i, st in enumerate((S * 2 * H * W, H * W, W, 1, 2 * H * W)):
        a.flow_strides[i] = st
    a.labels_dev, a.labels_stride, a.ref_slot = m["labels"].data_ptr(), H * W, 0
    a.min_pixels, a.min_ref_q, a.min_samples = 1, 64, 3
    a.par_dev, a.spread_dev, a.off_dev, a.cnt_dev = par.data_ptr(), spread.data_ptr(), off.data_ptr(), cnt.data_ptr()
    a.ref_dev, a.hist_dev, a.slot_tab_dev = ref.data_ptr(), hist.data_ptr(), tab.data_ptr()
    _lib.check(_lib.get_lib().cwm_parallax(ctypes.byref(a)))
    return [par.view(torch.int32), spread.view(torch.int32), off.view(torch.int32), cnt, ref.view(torch.int64), hist, tab]


def plain2(truth):
    first, _ = SO.plain(call, [t.clone() for t in truth])
    want, ms = SO.plain(call, [t.clone() for t in truth])
    assert SO.same(first, want), "the plain run is not bit-stable run to run"
    return want, ms


def poison_of(truth):
    return [SO.poison_like(t) for t in truth]


def test_parallax_late_inputs_and_early_consumers():
    truth = inputs(41)
    poison = poison_of(truth)
    want, ms = plain2(truth)
    cnt, ref, hist, tab = want[3], want[4].view(torch.float64), want[5], want[6]
    assert int(cnt.min()) == S and float(ref[..., 3].min()) == 1.0 and int(hist.sum()) == RR * H * W  # every sample is live, every pixel has a parallax
    assert int(tab[:, :, 1].sum()) == 0 and int(tab[:, :3, 0].sum()) == RR * H * W and int(tab[:, :3, 2].min()) > 128
    SO.check_poison("parallax", truth, poison, want, call)
    SO.protocol_a("parallax", call, truth, poison, want, ms, True)


def test_parallax_back_to_back():
    t1, t2 = inputs(41), inputs(43)
    want1, ms = plain2(t1)
    want2, _ = plain2(t2)
    assert not SO.same(want1, want2)
    SO.protocol_c("parallax", call, t1, t2, poison_of(t1), poison_of(t2), want1, want2, ms, True)
