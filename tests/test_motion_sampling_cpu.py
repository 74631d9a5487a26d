"""Counterfactual motion-map sampling, the host side: the energy samplers and `FlowGenerator`'s sampling surface against goldens recorded from
the reference (tests/golden/make_golden_motion_sampling.py), and the torch restatement of the flow-sample filter that the GPU tests and
`tools/flow_filter_step.py` use, pinned to the reference's own statistics and decisions."""
import json
import os

import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import config as C, sampling, segmentation, synthetic as S, vmae

import flow_filter_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
FILTER_CASES = ["f224_g28", "f224_g56", "f96_g10"]


def load_filter_case(g, tag):
    """(flows [B,2,H,W,S] float32 regenerated from the seed, active [B,Np,S] bool); asserts the fixture's checksum first."""
    active = np.unpackbits(g[tag + "_active"])[: int(np.prod(g[tag + "_active_shape"]))].reshape(g[tag + "_active_shape"]).astype(bool)
    flows = S.blob_flow_samples(int(g[tag + "_size"]), int(g[tag + "_seed"]), g[tag + "_blobs"], scaled_pixels=g[tag + "_scaled_pixels"],
                                nan_pixels=g[tag + "_nan_pixels"])
    assert S.flow_checksum(flows) == str(g[tag + "_checksum"]), "the regenerated flows are not the ones the golden was computed from"
    return flows, active


def patch_mag_bound(g, tag, active):
    """The larger of 8 x the reference's recorded fp32-vs-float64 difference and (4 n_active + 4) 2^-23 (2 ulp per magnitude, one rounding per
    weighted term and per addition of at most 4 n_active non-negative terms); relative."""
    grid = int(g[tag + "_grid"])
    n_active = (~active[:, grid * grid:]).sum(1).max()
    return max(8.0 * float(g[tag + "_patch_mag_rounding"]), (4 * n_active + 4) * 2.0 ** -23)


def tiny_generator(**kw):
    m = vmae.PretrainVisionTransformer(TINY)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(TINY, 3).items()})
    return segmentation.FlowGenerator(predictor=m.eval(), imagenet_normalize_inputs=True, temporal_dim=2, seed=0, **kw)


def test_sampler_masks_bit_equal_to_reference():
    g = np.load(os.path.join(GOLDEN, "motion_sampler.npz"))
    for n, (tag, input_size, side, kw, num_visible, one_hot) in enumerate(json.loads(str(g["cases"]))):
        gen = sampling.RotatedTableEnergyMaskingGenerator(input_size=tuple(input_size), mask_ratio=0, seed=11 + n, always_batch=True, eps=1e-16, resize=False, **kw)
        gen.num_visible = num_visible * gen.clumping_factor ** 2
        assert [gen.num_visible, gen.mask_ratio, gen.clumping_factor, gen.visible_frames] == g[tag + "_attrs"].tolist(), tag
        energy = torch.from_numpy(S.sampler_energy(2, side, 50 + n, one_hot))
        torch.manual_seed(1000 + n)
        masks = torch.stack([gen(energy) for _ in range(3)], -1)
        want = np.unpackbits(g[tag])[: int(np.prod(g[tag + "_shape"]))].reshape(g[tag + "_shape"]).astype(bool)
        assert masks.dtype == torch.bool and np.array_equal(masks.numpy(), want), tag
        if num_visible and not kw.get("randomize_num_visible"):
            cells = num_visible * gen.clumping_factor ** 2
            assert ((~masks[:, input_size[1] * input_size[2]:]).sum(1) <= cells).all() and (~masks).any(), tag


def test_sampler_resize_needs_torchvision_and_bad_pool_mode():
    with pytest.raises(NotImplementedError, match="torchvision"):
        sampling.RotatedTableEnergyMaskingGenerator(input_size=(2, 4, 4), mask_ratio=0)  # the reference's default is resize=True
    gen = sampling.EnergySamplingMaskingGenerator(input_size=(1, 4, 4), mask_ratio=0, resize=False, pool_mode="median")
    with pytest.raises(ValueError, match="pool_mode"):
        gen(torch.rand(1, 1, 8, 8))


def test_flow_generator_accepts_the_demo_constructor_line_and_sampler_surface():
    G = tiny_generator(patch_sampling_kwargs={"clumping_factor": 2})
    assert isinstance(G.patch_sampler, sampling.RotatedTableEnergyMaskingGenerator) and G.patch_sampler.clumping_factor == 2
    assert G.patch_sampler.num_visible == 4 and G.patch_sampler.visible_frames == 1 and G.patch_sampler.eps == 1e-16
    assert isinstance(G.flow_sample_filter, sampling.FlowSampleFilter)
    assert G.flow_sample_filter.flow_magnitude_threshold == 5.0 and G.flow_sample_filter.filter_methods == sampling.FlowSampleFilter.ALL_FILTERS
    assert repr(G.flow_sample_filter) == ("filtering by ['patch_magnitude', 'flow_area', 'num_corners']\nusing flow_magnitude_threshold 5.0\n"
                                          "using flow_area_threshold 0.75\nusing num_corners_threshold 2")
    G.set_flow_sample_filter(None)
    assert G.flow_sample_filter is None
    G.set_flow_sample_filter({"filter_methods": ["flow_area"], "flow_area_threshold": 0.5})
    assert G.flow_sample_filter.filter_methods == ["flow_area"] and G.flow_sample_filter.flow_area_threshold == 0.5
    assert tiny_generator(flow_sample_filter=None).flow_sample_filter is None
    assert tiny_generator(flow_sample_filter_params={"flow_magnitude_threshold": 2.0}).flow_sample_filter.flow_magnitude_threshold == 2.0
    # re-creation only when keyword arguments are given; every creation draws one rng.randint(9999)
    ref = np.random.RandomState(seed=0)
    G = tiny_generator()
    assert G.patch_sampler.seed == ref.randint(9999)
    first = G.patch_sampler
    G.set_patch_sampler(num_visible=3)
    assert G.patch_sampler is first and first.num_visible == 3
    G.set_patch_sampler(mask_ratio=0.5)
    assert G.patch_sampler is first and first.mask_ratio == 0.5
    G.set_patch_sampler(num_visible=2, clumping_factor=2)
    assert G.patch_sampler is not first and G.patch_sampler.seed == ref.randint(9999) and G.patch_sampler.num_visible == 8
    with pytest.raises(NotImplementedError):
        G.set_patch_sampler(resize=True)


def test_sample_patches_from_energy_matches_reference():
    g = np.load(os.path.join(GOLDEN, "motion_sampler.npz"))
    G = tiny_generator()
    G.set_input(torch.from_numpy(S.synthetic_frames(2, TINY, 41)))
    energy = torch.from_numpy(g["spe_energy"])
    got = {"spe_v1": G.sample_patches_from_energy(energy, num_samples=8, num_visible=1),
           "spe_v2_beta": G.sample_patches_from_energy(energy, num_samples=8, num_visible=2, beta=3.0),
           "spe_v0": G.sample_patches_from_energy(energy, num_samples=8, num_visible=0),
           "spe_uniform": G.sample_patches_from_energy(None, num_samples=8, num_visible=1),
           "spe_cf2": G.sample_patches_from_energy(energy, num_samples=8, num_visible=1, clumping_factor=2),
           "spe_after_recreate": G.sample_patches_from_energy(energy, num_samples=8, num_visible=1)}
    for k, v in got.items():
        assert v.shape == (2, 32, 8) and v.dtype == torch.bool and np.array_equal(v.numpy(), g[k]), k
    assert G.rng.randint(99999) == int(g["spe_rng_next"])
    assert not got["spe_v0"][:, :16].any() and got["spe_v0"][:, 16:].all()


def test_keypoint_hooks():
    G = tiny_generator()
    x = torch.rand(2, 2, 3, 32, 32)
    assert torch.equal(G.predict_keypoints_map(x), torch.ones(2, 1, 1, 32, 32))
    assert G.predict_keypoints_distribution(x[:1]).shape == (1, 1, 32, 32)  # (the reference's amin without keepdim broadcasts at B = 1 only)
    K = tiny_generator(keypoint_predictor=torch.nn.Conv3d(2, 1, 1))
    assert K.predict_keypoints_map(x).shape == (2, 1, 3, 32, 32)


@pytest.mark.parametrize("tag", FILTER_CASES)
def test_torch_restatement_matches_reference_filter(tag):
    g = np.load(os.path.join(GOLDEN, "motion_filter.npz"))
    flows, active = load_filter_case(g, tag)
    thr, area_thr, corner_thr = g["thresholds"]
    f, act = torch.from_numpy(flows), torch.from_numpy(active)
    pm, area, corners, _ = R.flow_filter_stats(f, act, thr)
    assert np.array_equal(pm.numpy(), g[tag + "_patch_mag"], equal_nan=True)  # the same ops in the same order on the same host arithmetic
    assert np.array_equal(area.numpy(), g[tag + "_area_count"]) and np.array_equal(corners.numpy(), g[tag + "_corner_count"])
    assert np.isnan(g[tag + "_patch_mag"]).sum() == 2 and patch_mag_bound(g, tag, active) < 1e-3 / 30
    for sub, want in zip(json.loads(str(g["subsets"])), g[tag + "_reject"]):
        x = f.clone()
        out, mask, dec = R.flow_filter_forward(x, act, sub, thr, area_thr, int(corner_thr))
        assert np.array_equal(dec.numpy(), want), sub
        assert mask.shape == f.shape and torch.equal(mask.amax((1, 2, 3)), dec) and out.is_contiguous()
        keep = ~dec
        assert (out[0, ..., dec[0]] == 0).all() and torch.equal(out[0, ..., keep[0]].nan_to_num(7.0), f[0, ..., keep[0]].nan_to_num(7.0))


def test_filter_on_cpu_tensor_raises_and_unknown_method():
    filt = sampling.FlowSampleFilter()
    with pytest.raises(RuntimeError):
        filt(torch.zeros(1, 2, 8, 8, 2), torch.ones(1, 8, 2, dtype=torch.bool))
    with pytest.raises(ValueError, match="Filter method"):
        sampling.FlowSampleFilter(filter_methods=["patch_magnitude", "speed"])(torch.zeros(1, 2, 8, 8, 2), torch.ones(1, 8, 2, dtype=torch.bool))
    assert sampling.FlowSampleFilter.ALL_FILTERS == ["patch_magnitude", "flow_area", "num_corners"]
    fm = torch.rand(1, 8, 8, 3) * 10
    assert filt.filter_by_flow_area(fm).shape == (1, 3) and filt.filter_by_num_corners(fm).shape == (1, 3)
    assert torch.equal(filt.filter_by_patch_magnitude(torch.tensor([[4.0, 5.0, float("nan")]])), torch.tensor([[True, False, False]]))
    mag, down, pm, act2 = filt.compute_flow_magnitude(torch.rand(1, 2, 8, 8, 3), torch.zeros(1, 8, 3, dtype=torch.bool))
    assert mag.shape == (1, 8, 8, 3) and down.shape == (1, 3, 4) and pm.shape == (1, 3) and act2.shape == (1, 3, 4)
