"""`MovabilityPredictor` without a GPU: the constructor's defaults against the reference's recorded ones, the result lists, the keypoint
distribution without a keypoint predictor, and the calls that raise."""
import inspect
import json
import os

import pytest
import torch

from counterfactualworldmodels_amd import config as C, movability, segmentation, vmae

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)


def build(**kw):
    return movability.MovabilityPredictor(predictor=vmae.PretrainVisionTransformer(TINY, mode="parity"), temporal_dim=2, **kw)


def test_constructor_defaults_equal_the_reference():
    with open(os.path.join(GOLDEN, "movability_defaults.json")) as fh:
        want = json.load(fh)
    sig = inspect.signature(movability.MovabilityPredictor.__init__)
    got = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert got == want and len(want) == 14
    M = build()
    assert issubclass(movability.MovabilityPredictor, segmentation.ImuConditionedFlowGenerator)
    for k, v in want.items():
        assert getattr(M, k) == v, k
    assert M.keypoints_distribution is None and M.VERBOSE is False
    M.set_verbosity()
    assert M.VERBOSE is True and movability.MovabilityPredictor.VERBOSE is False
    M2 = build(num_iters=5, sample_passives_from_movable=True, keypoints_power=2)
    assert (M2.num_iters, M2.sample_passives_from_movable, M2.keypoints_power) == (5, True, 2)
    assert not hasattr(M, "visualize_iterations")


def test_result_lists():
    M = build()
    M.reset_samples()
    assert M.movability_maps == M.flow_samples_per_iter == M.active_patches_per_iter == M.passive_patches_per_iter == []
    assert M.get_total_movability() is None and M.get_minimum_movability() is None
    r0 = tuple(torch.full((1,), float(i)) for i in range(4))
    r1 = tuple(torch.full((1,), float(10 + i)) for i in range(4))
    M._update_results(r0)
    M._update_results(r1)
    for i, lst in enumerate((M.movability_maps, M.flow_samples_per_iter, M.active_patches_per_iter, M.passive_patches_per_iter)):
        assert len(lst) == 2 and lst[0] is r0[i] and lst[1] is r1[i]
    M.reset_samples()
    assert M.movability_maps == [] and M.flow_samples_per_iter == []


def test_keypoints_distribution_without_a_keypoint_predictor():
    M = build()
    x = torch.rand(1, 2, 3, 32, 32)
    M.keypoints_distribution = "stale"
    M.set_keypoints_distribution(x)
    assert M.keypoints_distribution is None
    M.set_input(x)
    M.keypoints_distribution = "stale"
    M.set_keypoints_distribution()
    assert M.keypoints_distribution is None
    M.x = None
    with pytest.raises(AssertionError):
        M.set_keypoints_distribution()


def test_forward_with_initial_patches_raises():
    M = build()
    x = torch.rand(1, 2, 3, 32, 32)
    M.reset_samples()
    M._update_results(tuple(torch.zeros(1) for _ in range(4)))
    with pytest.raises(NotImplementedError, match="pass initial patches"):
        M(x, initial_active_patches=torch.zeros(1, 32, 4, dtype=torch.bool))
    assert M.x is x and M.movability_maps == [] and M.it == 0  # the input is set and the lists reset before the refusal, as in the reference
    with pytest.raises(AssertionError):
        build()._iterate_motion_map(None)  # no input set
