"""Stream ordering of `cwm_seed_select` (its stream is `base.stream` of the embedded cwm_patch_error_args, so the header gains no stream-taking name): the
protocols of tests/stream_order.py, imported and not edited -- A, late inputs and early consumers on a side stream, and C, two calls back to back behind a
delay without a host synchronisation between them.  The call is documented as asynchronous: it must return while the delay is still running.  Poison: ANOTHER
VALID map and NaN draws `e`.  Every call of this file shares ONE workspace, which the pool pass has to fill itself on the stream: in protocol C the second call
finds what the first one left there."""
import ctypes

import pytest
import torch

import seed_select_restatement as R
import stream_order as SO
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
B, GH, GW, P, K, RADIUS = 2, 12, 10, 8, 7, 1
H, W, n = GH * P, GW * P, GH * GW
_WORK = []


def workspace():
    if not _WORK:
        _WORK.append(torch.full((int(_lib.get_lib().cwm_seed_select_work_bytes(B, H, W, P)),), 0xA5, dtype=torch.uint8, device="cuda"))
    return _WORK[0]


def inputs(seed):
    return [torch.from_numpy(R.bumps(seed, B, GH, GW, P)).cuda(), torch.from_numpy(R.draws(seed + 100, B, n)).cuda()]


def call(m, e):
    """one call on the current stream (pixels form, race mode, peaks asked for), device tensors in and out and no synchronisation"""
    dev = m.device
    i32 = lambda *s: torch.full(s, -9, dtype=torch.int32, device=dev)  # noqa: E731
    out = [i32(B, K, 2), i32(B, K), torch.full((B, K), -7.0, device=dev), torch.full((B, n), -7.0, device=dev), torch.full((B, n), 99, dtype=torch.uint8, device=dev), i32(B, 4)]
    work = workspace()
    a = _lib.new_seed_select_args()
    _lib.fill_patch_args(a.base, geometry=(B, 1, 0, H, W, P), stream=_lib.current_stream_handle(dev))
    a.map_dev, a.cells, a.e_dev = m.data_ptr(), 0, e.data_ptr()
    a.map_strides[0], a.map_strides[1] = m.stride(0), m.stride(1)
    a.K, a.radius, a.peaks_only, a.abs_thresh, a.rel_thresh = K, RADIUS, 0, float("-inf"), 0.05
    a.work_dev, a.work_bytes = work.data_ptr(), work.numel()
    (a.seeds_dev, a.cells_dev, a.values_dev, a.pooled_dev, a.peaks_dev, a.stats_dev) = (t.data_ptr() for t in out)
    _lib.check(_lib.get_lib().cwm_seed_select(ctypes.byref(a)))
    return out


def plain2(truth):
    first, _ = SO.plain(call, [t.clone() for t in truth])
    want, ms = SO.plain(call, [t.clone() for t in truth])
    assert SO.same(first, want), "the plain run is not bit-stable run to run"
    return want, ms


def poison_of(truth, seed):
    return [inputs(seed)[0], SO.poison_like(truth[1])]


def test_seed_select_late_inputs_and_early_consumers():
    truth = inputs(41)
    poison = poison_of(truth, 42)
    want, ms = plain2(truth)
    ref = R.select(truth[0].cpu().numpy(), P, K, radius=RADIUS, rel_thresh=0.05, e=truth[1].cpu().numpy())
    R.assert_equal(dict(zip(("seeds", "cells", "values", "pooled", "peaks", "stats"), (t.cpu().numpy() for t in want))), ref, "plain")
    assert int(want[5][:, 2].min()) == K  # every row finds all its seeds
    SO.check_poison("seed_select", truth, poison, want, call)
    SO.protocol_a("seed_select", call, truth, poison, want, ms, True)


def test_seed_select_back_to_back():
    t1, t2 = inputs(41), inputs(43)
    want1, ms = plain2(t1)
    want2, _ = plain2(t2)
    assert not SO.same(want1, want2)
    SO.protocol_c("seed_select", call, t1, t2, poison_of(t1, 42), poison_of(t2, 44), want1, want2, ms, True)
