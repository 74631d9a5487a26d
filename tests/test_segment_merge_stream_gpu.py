"""Stream ordering of `cwm_segment_merge` (its stream is `base.stream` of the embedded cwm_patch_error_args, so the header gains no stream-taking name): the
protocols of tests/stream_order.py, imported and not edited -- A, late inputs and early consumers on a side stream, and C, two calls back to back behind a
delay without a host synchronisation between them.  The call is documented as asynchronous: it must return while the delay is still running.  Poison: ANOTHER
VALID set of segments and NaN scores.  Every call of this file shares ONE workspace, which the call has to initialise itself on the stream: in protocol C the
second call finds what the first one accumulated."""
import ctypes

import pytest
import torch

import segment_merge_restatement as MR
import stream_order as SO
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
B, K, H, W, P = 2, 33, 64, 64, 16
n = (H // P) * (W // P)
_WORK = []


def workspace():
    if not _WORK:
        _WORK.append(torch.full((int(_lib.get_lib().cwm_segment_merge_work_bytes(B, K, H, W)),), 0xA5, dtype=torch.uint8, device="cuda"))
    return _WORK[0]


def inputs(seed):
    segs, scores = MR.random_rects(seed, B, K, H, W)
    return [torch.from_numpy(segs).cuda(), torch.from_numpy(scores).cuda()]


def call(segs, scores):
    """one call on the current stream, device tensors in and out and no synchronisation"""
    dev = segs.device
    i32 = lambda *s: torch.full(s, -9, dtype=torch.int32, device=dev)  # noqa: E731
    out = [torch.full((B, H, W), 99, dtype=torch.uint8, device=dev), i32(B, K), i32(B, K), i32(B, K), i32(B, K, K), torch.full((B, n), -7.0, device=dev), i32(B, 4)]
    work = workspace()
    a = _lib.new_segment_merge_args()
    _lib.fill_patch_args(a.base, geometry=(B, 2, 0, H, W, P), stream=_lib.current_stream_handle(dev))
    a.K, a.segs_dev, a.scores_dev = K, segs.data_ptr(), scores.data_ptr()
    a.seg_strides[0], a.seg_strides[1] = segs.stride(0), segs.stride(1)
    a.min_area, a.max_area, a.iou_thresh, a.contain_thresh, a.absorb = 1, 0, 0.4, 0.6, 1
    a.work_dev, a.work_bytes = work.data_ptr(), work.numel()
    (a.labels_dev, a.owner_dev, a.area_dev, a.label_area_dev, a.inter_dev, a.cover_dev, a.stats_dev) = (t.data_ptr() for t in out)
    _lib.check(_lib.get_lib().cwm_segment_merge(ctypes.byref(a)))
    return out


def plain2(truth):
    first, _ = SO.plain(call, [t.clone() for t in truth])
    want, ms = SO.plain(call, [t.clone() for t in truth])
    assert SO.same(first, want), "the plain run is not bit-stable run to run"
    return want, ms


def poison_of(truth, seed):
    return [inputs(seed)[0], SO.poison_like(truth[1])]


def test_segment_merge_late_inputs_and_early_consumers():
    truth = inputs(41)
    poison = poison_of(truth, 42)
    want, ms = plain2(truth)
    assert int(want[6][:, 1].min()) >= 2  # every row has more than one label
    SO.check_poison("segment_merge", truth, poison, want, call)
    SO.protocol_a("segment_merge", call, truth, poison, want, ms, True)


def test_segment_merge_back_to_back():
    t1, t2 = inputs(41), inputs(43)
    want1, ms = plain2(t1)
    want2, _ = plain2(t2)
    assert not SO.same(want1, want2)
    SO.protocol_c("segment_merge", call, t1, t2, poison_of(t1, 42), poison_of(t2, 44), want1, want2, ms, True)
