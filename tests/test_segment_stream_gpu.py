"""Stream ordering of `cwm_segment_step` (its stream is `base.stream` of the embedded cwm_patch_error_args, so the header gains no stream-taking name): the
protocols of tests/stream_order.py, imported and not edited -- A, late inputs and early consumers on a side stream, and C, two calls back to back behind a
delay without a host synchronisation between them.  The call is documented as asynchronous: it must return while the delay is still running.  Poison: NaN
flows, directions and keys, and ANOTHER VALID seed per row."""
import ctypes

import numpy as np
import pytest
import torch

import segment_restatement as SR
import stream_order as SO
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
B, H, W, P, S, KA, KP = 2, 32, 32, 4, 6, 4, 5
n = (H // P) * (W // P)


def inputs(seed):
    g = np.random.default_rng(seed)
    masks = np.zeros((B, H, W), bool)
    seeds = np.zeros((B, 2), np.int32)
    for b in range(B):
        y0, x0 = g.integers(2, 10, 2)
        masks[b, y0:y0 + g.integers(10, 18), x0:x0 + g.integers(10, 18)] = True
        seeds[b] = (y0 + 3, x0 + 3)
    flows = np.concatenate([SR.flows_of(masks[b], g.integers(0, 4, S)) for b in range(B)], 0)
    dirs = np.tile(np.array([[8.0, 6.0]], np.float32), (S, 1))
    keys = g.random((B, 2, n), dtype=np.float32)
    view = torch.from_numpy(flows).permute(0, 4, 1, 2, 3).contiguous().cuda()  # [B,S,2,H,W]: the flow model's batch
    return [view, torch.from_numpy(seeds).cuda(), torch.from_numpy(dirs).cuda(), torch.from_numpy(keys).cuda()]


def call(view, seeds, dirs, keys):
    """one call on the current stream, device tensors in and out and no synchronisation"""
    f = view.permute(0, 2, 3, 4, 1)
    dev = f.device
    out = [torch.full((B, S), -7.0, device=dev), torch.full((B, H, W), 9, dtype=torch.uint8, device=dev), torch.full((B, H, W), 9, dtype=torch.uint8, device=dev),
           torch.full((B, n), -7.0, device=dev), torch.full((B, 4), -9, dtype=torch.int32, device=dev), torch.full((B, KA + KP), -9, dtype=torch.int32, device=dev),
           torch.full((B, 2 * n), 9, dtype=torch.uint8, device=dev), torch.full((B, 2 * n), 9, dtype=torch.uint8, device=dev)]
    a = _lib.new_segment_step_args()
    _lib.fill_patch_args(a.base, geometry=(B, 2, 0, H, W, P), stream=_lib.current_stream_handle(dev))
    a.flows_dev, a.C, a.S = f.data_ptr(), 2, S
    for i, st in enumerate(f.stride()):
        a.flow_strides[i] = st
    a.seeds_dev, a.dirs_dev, a.keys_dev = seeds.data_ptr(), dirs.data_ptr(), keys.data_ptr()
    a.min_seed_mag, a.abs_thresh, a.rel_thresh, a.vote_frac, a.cos_min, a.inside_frac = 0.5, 1.0, 0.5, 0.5, 0.5, 0.5
    a.k_active, a.k_passive, a.ring_radius = KA, KP, 1
    (a.seed_ref_dev, a.votes_dev, a.segment_dev, a.cover_dev, a.stats_dev, a.picks_dev, a.active_out_dev, a.passive_out_dev) = (t.data_ptr() for t in out)
    _lib.check(_lib.get_lib().cwm_segment_step(ctypes.byref(a)))
    out[0] = torch.nan_to_num(out[0], nan=-1.0)  # (seed_ref marks a sample that is not valid with a NaN; SO.same compares with torch.equal)
    return out


def plain2(truth):
    first, _ = SO.plain(call, [t.clone() for t in truth])
    want, ms = SO.plain(call, [t.clone() for t in truth])
    assert SO.same(first, want), "the plain run is not bit-stable run to run"
    return want, ms


def poison_of(truth, seed):
    view, seeds, dirs, keys = truth
    return [SO.poison_like(view), inputs(seed)[1], SO.poison_like(dirs), SO.poison_like(keys)]


def test_segment_step_late_inputs_and_early_consumers():
    truth = inputs(31)
    poison = poison_of(truth, 32)
    want, ms = plain2(truth)
    assert int(want[4][:, 1].min()) > 0  # every row has a segment
    SO.check_poison("segment_step", truth, poison, want, call)
    SO.protocol_a("segment_step", call, truth, poison, want, ms, True)


def test_segment_step_back_to_back():
    t1, t2 = inputs(31), inputs(33)
    want1, ms = plain2(t1)
    want2, _ = plain2(t2)
    assert not SO.same(want1, want2)
    SO.protocol_c("segment_step", call, t1, t2, poison_of(t1, 32), poison_of(t2, 34), want1, want2, ms, True)
