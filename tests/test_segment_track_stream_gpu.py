"""Stream ordering of `cwm_segment_track` (its stream is `base.stream` of the embedded cwm_patch_error_args, so the header gains no stream-taking name): the
protocols of tests/stream_order.py, imported and not edited -- A, late inputs and early consumers on a side stream, and C, two calls back to back behind a
delay without a host synchronisation between them.  The call is documented as asynchronous: it must return while the delay is still running.  Poison: ANOTHER
VALID set of maps and state, and NaN flows.  Every call of this file shares ONE workspace, which the call has to initialise itself on the stream: in protocol C
the second call finds what the first one accumulated."""
import ctypes

import pytest
import torch

import segment_track_restatement as TR
import stream_order as SO
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
B, H, W = 2, 64, 64
_WORK = []


def workspace():
    if not _WORK:
        _WORK.append(torch.full((int(_lib.get_lib().cwm_segment_track_work_bytes(B, H, W)),), 0xA5, dtype=torch.uint8, device="cuda"))
    return _WORK[0]


def inputs(seed):
    """[prev, cur, flow, track_id, age, next_id] on the device"""
    prev, cur, state = TR.random_maps(seed, B, H, W, n_prev=12, n_cur=12)
    state["next_id"] += seed  # (so that the next_id of two sets differs)
    flow = TR.flows("frac", seed, B, H, W)
    return [torch.from_numpy(v).cuda() for v in (prev, cur, flow, state["track_id"], state["age"], state["next_id"])]


def call(prev, cur, flow, track_id, age, next_id):
    """one call on the current stream, device tensors in and out and no synchronisation"""
    dev = prev.device
    i32 = lambda *s: torch.full(s, -9, dtype=torch.int32, device=dev)  # noqa: E731
    u8 = lambda: torch.full((B, H, W), 99, dtype=torch.uint8, device=dev)  # noqa: E731
    out = [u8(), i32(B, 64), i32(B, 64), i32(B), i32(B, 64), i32(B, 64, 4), torch.full((B, 64, 2), -9, dtype=torch.int64, device=dev), i32(B, 64), i32(B, 64),
           i32(B, 65, 65), u8(), i32(B, 8)]
    work = workspace()
    a = _lib.new_segment_track_args()
    _lib.fill_patch_args(a.base, geometry=(B, 1, 0, H, W, 0), stream=_lib.current_stream_handle(dev))
    a.prev_dev, a.prev_stride, a.cur_dev, a.cur_stride = prev.data_ptr(), prev.stride(0), cur.data_ptr(), cur.stride(0)
    a.flow_dev = flow.data_ptr()
    a.flow_strides[0], a.flow_strides[1] = flow.stride(0), flow.stride(1)
    a.track_id_in_dev, a.age_in_dev, a.next_id_in_dev = track_id.data_ptr(), age.data_ptr(), next_id.data_ptr()
    a.iou_thresh, a.min_inter, a.min_area, a.max_age, a.carry = 0.2, 1, 1, 3, 1
    a.work_dev, a.work_bytes = work.data_ptr(), work.numel()
    a.out_stride = H * W
    (a.out_dev, a.track_id_out_dev, a.age_out_dev, a.next_id_out_dev, a.area_dev, a.bbox_dev, a.moments_dev, a.slot_of_cur_dev, a.linked_cur_dev, a.table_dev,
     a.warped_dev, a.stats_dev) = (t.data_ptr() for t in out)
    _lib.check(_lib.get_lib().cwm_segment_track(ctypes.byref(a)))
    return out


def plain2(truth):
    first, _ = SO.plain(call, [t.clone() for t in truth])
    want, ms = SO.plain(call, [t.clone() for t in truth])
    assert SO.same(first, want), "the plain run is not bit-stable run to run"
    return want, ms


def poison_of(truth, seed):
    p = inputs(seed)
    p[2] = SO.poison_like(truth[2])
    return p


def test_segment_track_late_inputs_and_early_consumers():
    truth = inputs(41)
    poison = poison_of(truth, 42)
    want, ms = plain2(truth)
    assert int(want[11][:, 0].min()) >= 1 and int(want[11][:, 1].min()) >= 1  # every row links and gives birth
    SO.check_poison("segment_track", truth, poison, want, call)
    SO.protocol_a("segment_track", call, truth, poison, want, ms, True)


def test_segment_track_back_to_back():
    t1, t2 = inputs(41), inputs(43)
    want1, ms = plain2(t1)
    want2, _ = plain2(t2)
    assert not SO.same(want1, want2)
    SO.protocol_c("segment_track", call, t1, t2, poison_of(t1, 42), poison_of(t2, 44), want1, want2, ms, True)
