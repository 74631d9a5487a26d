"""Stream ordering of `cwm_unmask_step` (its stream is `base.stream` of the embedded cwm_patch_error_args, so the header gains no stream-taking name): the
protocols of tests/stream_order.py, imported and not edited -- A, late inputs and early consumers on a side stream, and C, two calls back to back behind a
delay without a host synchronisation between them.  The call is documented as asynchronous: it must return while the delay is still running.  Poison: NaN
tokens, frames and race draws, and ANOTHER VALID mask of the same count per row."""
import pytest
import torch

import stream_order as SO
from test_unmask_step_gpu import Cc, F, P, T, frame_mask, run_on_device

pytestmark = pytest.mark.gpu
B, H, W = 3, 12, 20
h, w, n = H // P, W // P, (H // P) * (W // P)


def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, T, Cc, H, W), generator=g)
    mask = frame_mask(B, h, w, [torch.randperm(n, generator=g)[:9].tolist() for _ in range(B)])
    y = torch.randn((B, 9, P * P * Cc), generator=g)
    e = torch.empty((B, n)).exponential_(generator=g)
    return [t.cuda() for t in (y, x, mask, e)]


def call(y, x, mask, e):
    return run_on_device(x, mask, y, 4, 1.0, e)


def plain2(truth):
    first, _ = SO.plain(call, [t.clone() for t in truth])
    want, ms = SO.plain(call, [t.clone() for t in truth])
    assert SO.same(first, want), "the plain run is not bit-stable run to run"
    return want, ms


def poison_of(truth, seed):
    y, x, mask, e = truth
    return [SO.poison_like(y), SO.poison_like(x), inputs(seed)[2], SO.poison_like(e)]


def test_unmask_step_late_inputs_and_early_consumers():
    truth = inputs(21)
    poison = poison_of(truth, 22)
    want, ms = plain2(truth)
    SO.check_poison("unmask_step", truth, poison, want, call)
    SO.protocol_a("unmask_step", call, truth, poison, want, ms, True)


def test_unmask_step_back_to_back():
    t1, t2 = inputs(21), inputs(23)
    want1, ms = plain2(t1)
    want2, _ = plain2(t2)
    assert not SO.same(want1, want2)
    SO.protocol_c("unmask_step", call, t1, t2, poison_of(t1, 22), poison_of(t2, 24), want1, want2, ms, True)
