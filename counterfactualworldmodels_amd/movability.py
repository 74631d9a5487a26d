"""`MovabilityPredictor`: which parts of a scene are movable, estimated by trying to move patches and looking at the counterfactual flow
(reference: cwm/models/movability.py:13-360, the class the demo notebook `MovabilityAndMotionCovariance.ipynb` builds around a keypoint RAFT).

A host-side loop over calls that already run on the device: `ImuConditionedFlowGenerator.sample_counterfactual_motion_map` (prompt kernels,
predictor, flow model, flow-sample filter) and the motion-map kernels of `flowstats`.  It draws from the wrapper's numpy stream, the global torch
generator and the mask rectangulariser in the reference's order, so the same seeds give the same patches and shifts.  `visualize_iterations`
(matplotlib) is not provided; `sample_and_visualize_keypoints` returns its tensors and plots nothing, as in the reference.

    keypoints = load_raft_model(None, output_dim=1); keypoints.load_state_dict(torch.load(path)["model"])
    M = MovabilityPredictor(predictor=imu_predictor, head_motion_predictor=flow2imu, flow_model=raft, keypoint_predictor=keypoints,
                            imagenet_normalize_inputs=True, mask_generator=generator).cuda()
    movability = M(x)                      # x [1,T,3,H,W] in [0,1] -> [1,1,H,W] in [0,1]; the loop runs at B = 1, like the reference's
    total = M.get_total_movability()

`get_total_movability` (movability.py:283-290) concatenates every iteration's flows and reduces them again each iteration; here each iteration's
magnitude sum is computed once (`cwm_flow_motion_sum`) and the sums are combined and finished with 1 / S_total (`cwm_flow_map_finish`).
"""
from __future__ import annotations

from time import time

import torch

from . import flowstats
from .segmentation import ImuConditionedFlowGenerator


class MovabilityPredictor(ImuConditionedFlowGenerator):
    """Movability by iterated counterfactual motion (movability.py:13-47): sample patches, try to move them, see where the counterfactual flow is
    high; then resample `num_iters` times from the places of high movability, optionally with static "passive" patches that isolate independent
    object motion.  A predictor without head-motion conditioning works too, with flows biased toward camera motion."""

    VERBOSE = False

    def __init__(self, *args, initialize_from_keypoints=True, iterate_from_keypoints=False, keypoints_power=8, movability_power=1,
                 num_initial_samples=16, num_initial_active_patches=1, num_initial_passive_patches=0, num_samples_per_iteration=16,
                 num_active_patches_per_sample=1, num_passive_patches_per_sample=1, sample_passives_from_movable=False,
                 update_distribution_per_iteration=True, num_iters=2, sample_batch_size=4, **kwargs):
        super().__init__(*args, **kwargs)
        # using keypoints to sample
        self.initialize_from_keypoints = initialize_from_keypoints
        self.keypoints_power = keypoints_power
        self.keypoints_distribution = None
        # sampling parameters
        self.sample_batch_size = sample_batch_size
        self.movability_power = movability_power
        self.sample_passives_from_movable = sample_passives_from_movable
        # iteration parameters
        self.iterate_from_keypoints = iterate_from_keypoints
        self.num_initial_samples = num_initial_samples
        self.num_initial_active_patches = num_initial_active_patches
        self.num_initial_passive_patches = num_initial_passive_patches
        self.num_samples_per_iteration = num_samples_per_iteration
        self.num_active_patches_per_sample = num_active_patches_per_sample
        self.num_passive_patches_per_sample = num_passive_patches_per_sample
        self.num_iters = num_iters
        self.update_distribution_per_iteration = update_distribution_per_iteration
        self._map_sums = []

    def set_verbosity(self, is_verbose=True):
        self.VERBOSE = is_verbose

    def set_keypoints_distribution(self, x=None):
        """movability.py:75-87: the keypoint predictor's distribution of x (default: the current input), None without a keypoint predictor."""
        if x is None:
            x = self.x
        assert x is not None
        if self.keypoint_predictor is not None:
            self.keypoints_distribution = self.predict_keypoints_distribution(x, power=self.keypoints_power)
        else:
            self.keypoints_distribution = None

    def sample_and_visualize_keypoints(self, x=None, sampled_keypoints=None, sampled_passive_patches=None, num_samples=32):
        """(sampled_keypoints [B,Nt,S], img): x with the patches any sample chose tinted red, the passive ones blue (movability.py:89-125)."""
        if x is None:
            assert self.x is not None
            x = self.x
        if sampled_keypoints is None:
            self.set_keypoints_distribution(x)
            sampled_keypoints = self.sample_patches_from_energy(self.keypoints_distribution, num_visible=1, num_samples=num_samples)
        kps = sampled_keypoints.amin(-1)
        img = x.clone()
        alpha = self.get_masked_pred_patches(torch.zeros_like(x), kps, fill_value=[1, 0, 0])[:, :, 0:1]
        red = torch.cat([alpha, torch.zeros_like(alpha), torch.zeros_like(alpha)], -3)
        img = img * (1 - alpha) + 0.5 * alpha * (red + img)
        if sampled_passive_patches is not None:
            passives = sampled_passive_patches.amin(-1)
            alpha = self.get_masked_pred_patches(torch.zeros_like(x), passives, fill_value=[0, 0, 1])[:, :, 2:3]
            blue = torch.cat(2 * [torch.zeros_like(alpha)] + [alpha], -3)
            img = img * (1 - alpha) + 0.5 * alpha * (blue + img)
        return (sampled_keypoints, img)

    def _sample_initial_motion_map(self, x, num_samples=None, sample_batch_size=None, do_filter=True, mask_head_motion=False,
                                   static_head_motion=True, normalize=True, patch_sampling_kwargs={}, **kwargs):
        """movability.py:127-166: iteration 0, active patches drawn from the keypoint distribution (or uniformly)."""
        self.set_input(x)
        if self.initialize_from_keypoints:
            self.set_keypoints_distribution()
            sampling_dist = self.keypoints_distribution
            passive_dist = 1 - self.keypoints_distribution
        else:
            sampling_dist = None
            passive_dist = None
        flows, motion_patches, static_patches = self.sample_counterfactual_motion_map(
            x=self.x, active_sampling_distribution=sampling_dist, passive_sampling_distribution=passive_dist,
            num_active_patches=self.num_initial_active_patches, num_passive_patches=self.num_initial_passive_patches,
            num_samples=(num_samples or self.num_initial_samples), sample_batch_size=(sample_batch_size or self.sample_batch_size),
            do_filter=do_filter, mask_head_motion=mask_head_motion, static_head_motion=static_head_motion,
            patch_sampling_kwargs=patch_sampling_kwargs, **kwargs)
        motion_map = self.compute_mean_motion_map(flows, normalize_per_sample=False, normalize=normalize)
        return (motion_map, flows, motion_patches, static_patches)

    def _iterate_motion_map(self, movability_distribution, sample_passives_from_movable=True, num_active_patches=None, num_passive_patches=None,
                            num_samples=None, sample_batch_size=None, do_filter=True, mask_head_motion=False, static_head_motion=True,
                            patch_sampling_kwargs={}, normalize=True, **kwargs):
        """movability.py:168-217: one more round, active patches drawn from `movability_distribution` [B,1,H,W] (None: uniform), passive ones from
        it or from its complement."""
        assert self.x is not None
        if movability_distribution is None:
            movability_distribution = torch.ones_like(self.x[:, 0:1, 0])
        movability_distribution = self.compute_mean_motion_map(movability_distribution)
        movability_distribution = movability_distribution ** self.movability_power
        if sample_passives_from_movable:
            passive_distribution = movability_distribution
        else:
            passive_distribution = (1 - movability_distribution).relu()
        if self.iterate_from_keypoints:
            self.set_keypoints_distribution(self.x)
            # in place, as in the reference: with sample_passives_from_movable the two names are one tensor and it is multiplied twice
            movability_distribution *= self.keypoints_distribution
            passive_distribution *= self.keypoints_distribution
        flows, motion_patches, static_patches = self.sample_counterfactual_motion_map(
            x=self.x, active_sampling_distribution=movability_distribution, passive_sampling_distribution=passive_distribution,
            num_active_patches=(num_active_patches or self.num_active_patches_per_sample),
            num_passive_patches=(num_passive_patches or self.num_passive_patches_per_sample),
            num_samples=(num_samples or self.num_samples_per_iteration), sample_batch_size=(sample_batch_size or self.sample_batch_size),
            do_filter=do_filter, mask_head_motion=mask_head_motion, static_head_motion=static_head_motion,
            patch_sampling_kwargs=patch_sampling_kwargs, **kwargs)
        motion_map = self.compute_mean_motion_map(flows, normalize_per_sample=False, normalize=normalize)
        return (motion_map, flows, motion_patches, static_patches)

    def reset_samples(self):
        self.movability_maps = []
        self.flow_samples_per_iter = []
        self.active_patches_per_iter = []
        self.passive_patches_per_iter = []
        self._map_sums = []

    def _update_results(self, results):
        movability, flows, active_patches, passive_patches = results
        self.movability_maps.append(movability)
        self.flow_samples_per_iter.append(flows)
        self.active_patches_per_iter.append(active_patches)
        self.passive_patches_per_iter.append(passive_patches)

    def _magnitude_sums(self):
        """[(flows, sum over its samples of |flow| [B,1,H,W])] for every stored iteration; a sum is computed once, when first asked for, and kept
        for as long as the entry of `flow_samples_per_iter` it belongs to is the same tensor."""
        kept = self._map_sums[:len(self.flow_samples_per_iter)]
        sums = []
        for i, flows in enumerate(self.flow_samples_per_iter):
            if i < len(kept) and kept[i][0] is flows:
                sums.append(kept[i])
            else:
                sums.append((flows, flowstats.motion_map_sum(flows)))
        self._map_sums = sums
        return sums

    def get_total_movability(self):
        """The normalised mean flow magnitude over the samples of all iterations (movability.py:283-290), from the per-iteration sums."""
        if len(self.flow_samples_per_iter) == 0:
            return None
        sums = self._magnitude_sums()
        total = sums[0][1]
        for _, s in sums[1:]:
            total = total + s
        return flowstats.finish_motion_map(total, sum(f.shape[-1] for f, _ in sums), normalize=True)

    def get_minimum_movability(self):
        if len(self.flow_samples_per_iter) == 0:
            return None
        mags = torch.stack([self.compute_mean_motion_map(fs) for fs in self.flow_samples_per_iter], -1)
        return mags.amin(-1)

    def forward(self, x, initial_active_patches=None, initial_passive_patches=None, initial_sampling_distribution=None, num_initial_samples=None,
                num_samples_per_iteration=None, sample_batch_size=None, num_iters=None, **kwargs):
        """The final movability map [B,1,H,W] after iteration 0 and `num_iters` more (movability.py:299-360); every iteration's map, flows and
        patches are kept in `movability_maps / flow_samples_per_iter / active_patches_per_iter / passive_patches_per_iter`."""
        self.set_input(x)
        self.reset_samples()
        self.it = 0
        t0 = time()
        if initial_active_patches is not None:
            raise NotImplementedError("pass initial patches")
        results = self._sample_initial_motion_map(x=self.x, num_samples=num_initial_samples, sample_batch_size=sample_batch_size, **kwargs)
        self._update_results(results)
        if self.VERBOSE:
            t1 = time()
            print("Completed iter %d with %d samples in %0.3f s" % (self.it, results[1].size(-1), (t1 - t0)))
            t0 = time()
        for self.it in range(1, (num_iters or self.num_iters) + 1):
            if self.update_distribution_per_iteration:
                dist = self.get_total_movability()
            else:
                dist = self.movability_maps[-1]
            results = self._iterate_motion_map(dist, sample_passives_from_movable=self.sample_passives_from_movable,
                                               num_samples=num_samples_per_iteration, sample_batch_size=sample_batch_size, **kwargs)
            self._update_results(results)
            if self.VERBOSE:
                t1 = time()
                print("Completed iter %d with %d samples in %0.3f s" % (self.it, results[1].size(-1), (t1 - t0)))
                t0 = time()
        return self.movability_maps[-1]
