"""`MovabilityPredictor` on the GPU against the reference's recorded loop (tests/golden/make_golden_movability.py: tiny IMU-conditioned
predictor and flow -> IMU model, the `SyntheticFlow` / `SyntheticKeypoints` stand-ins, a [1,2,3,32,32] movie, 8 + 2 x 8 samples).

What is exact and what is bounded.  Patches, shifts and filter decisions are discrete and must equal the reference's.  The flows are held to the
bound the merged driver test gives this stack, EPS_FLOW = 4e-3 px per component (tests/test_head_motion_gpu.py::test_driver_vs_reference).  A map is
n = (m - min m) / max(range m, eps) with m the mean over the samples of |flow|: | |a| - |b| | <= |a - b| <= sqrt(2) EPS_FLOW =: d per sample, hence
for the mean; the minimum and the maximum move by at most d each, so the numerator by 2 d and the range by 2 d, and with n <= 1
|dn| <= (2 d + n 2 d) / range <= 4 sqrt(2) EPS_FLOW / range, range = the range of the reference's un-normalised map, computed from the recorded
flows.  The minimum over the iterations' maps moves by at most the largest of their bounds.

Open and closed loop.  From iteration 1 on the sampler's energies come from flows.  In the open-loop test every energy handed to
`sample_patches_from_energy` is replaced by the recorded one, so a flipped draw could only come from the sampler or the RNG order itself; in the
closed-loop test nothing is replaced: the fixture's maker has shown that the reference's own draws and decisions survive a perturbation of the
energies five times larger than the flow bound allows, and that no patch magnitude is within 1e-2 (relative) of the threshold.  Every iteration
is compared in both."""
import json
import os

import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import config as C, conjoined_vmae as CV, flowstats, masking, movability, sampling, synthetic as S
from counterfactualworldmodels_amd.raft import RAFT, _args

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS_FLOW = 4e-3  # px, tests/test_head_motion_gpu.py::test_driver_vs_reference
CASES = ["default", "keypoints"]


def weights(cfg, seed):
    return {k: torch.from_numpy(S.synthetic_tensor(k, shp, seed)) for k, shp in C.conj_state_dict_schema(cfg).items()}


def build(g, energies=None):
    """The generator of the fixture, with the recording hooks of its maker; `energies`: the recorded energies to hand to the sampler (open loop)."""
    from test_conj_oracle import TINY_CONJ
    from test_head_motion_cpu import TINY_FLOW2IMU

    pred = CV.ConjoinedPaddedVisionTransformer(TINY_CONJ)
    pred.load_state_dict(weights(TINY_CONJ, int(g["seed_pred"])))
    f2i = CV.ConjoinedPretrainVisionTransformer(TINY_FLOW2IMU)
    f2i.load_state_dict(weights(TINY_FLOW2IMU, int(g["seed_f2i"])))
    gen = masking.RotatedTableUniformMaskingGenerator(input_size=pred.mask_size, mask_ratio=0.9, clumping_factor=2)
    n_init, n_iter, iters, sbs = (int(v) for v in g["settings"])
    M = movability.MovabilityPredictor(
        predictor=pred, head_motion_predictor=f2i, flow_model=S.SyntheticFlow(), keypoint_predictor=S.SyntheticKeypoints(), temporal_dim=2,
        imagenet_normalize_inputs=True, mask_generator=gen, seed=int(g["seed"]), flow_sample_filter=sampling.FlowSampleFilter(**json.loads(str(g["filter_params"]))),
        num_initial_samples=n_init, num_samples_per_iteration=n_iter, num_iters=iters, sample_batch_size=sbs, **json.loads(str(g["kwargs"]))).to("cuda")
    rec = {"energies": [], "shifts": [], "reject": [], "patch_mag": []}
    spe, scmm = M.sample_patches_from_energy, M.sample_counterfactual_motion_map

    def sample_patches_from_energy(energy=None, **kw):
        rec["energies"].append(None if energy is None else energy.detach().cpu().numpy())
        if energies is not None:
            e = energies[len(rec["energies"]) - 1]
            energy = None if e.size == 0 else torch.from_numpy(e).cuda()
        return spe(energy=energy, **kw)

    def sample_counterfactual_motion_map(*a, **kw):
        r = scmm(*a, **kw)
        rec["shifts"].append(np.array(M.shifts, dtype=np.int32))
        rec["reject"].append(M.flow_sample_filter.last_stats["reject"].cpu().numpy())
        rec["patch_mag"].append(M.flow_sample_filter.last_stats["patch_mag"].cpu().numpy())
        return r

    M.sample_patches_from_energy = sample_patches_from_energy
    M.sample_counterfactual_motion_map = sample_counterfactual_motion_map
    return M, rec


def map_range(flows):
    """range over (H, W) of the un-normalised mean |flow| of recorded samples [1,2,H,W,S] (float64)."""
    m = np.sqrt((flows.astype(np.float64) ** 2).sum(1)).mean(-1)
    return float(m.max() - m.min())


def map_bound(flows):
    return 4 * np.sqrt(2.0) * EPS_FLOW / map_range(flows)


def compare_iterations(tag, g, M, rec):
    n_it = int(g["settings"][2]) + 1
    assert len(M.movability_maps) == len(M.flow_samples_per_iter) == len(M.active_patches_per_iter) == len(M.passive_patches_per_iter) == n_it
    assert len(rec["shifts"]) == len(rec["reject"]) == n_it and len(rec["energies"]) == 2 * n_it
    thr = json.loads(str(g["filter_params"]))["flow_magnitude_threshold"]
    for it in range(n_it):
        assert np.array_equal(M.active_patches_per_iter[it].cpu().numpy(), g["active_it%d" % it]), (tag, it, "active patches")
        assert np.array_equal(M.passive_patches_per_iter[it].cpu().numpy(), g["passive_it%d" % it]), (tag, it, "passive patches")
        assert np.array_equal(rec["shifts"][it], g["shifts_it%d" % it]), (tag, it, "shifts")
        assert np.array_equal(rec["reject"][it], g["reject_it%d" % it]), (tag, it, "filter decisions", rec["patch_mag"][it], g["patch_mag_it%d" % it])
        assert rec["reject"][it].any() and not rec["reject"][it].all()
        flows = M.flow_samples_per_iter[it].cpu().numpy()
        e_f = float(np.abs(flows - g["flows_it%d" % it]).max())
        e_pm = float(np.abs(rec["patch_mag"][it] - g["patch_mag_it%d" % it]).max())
        bound = map_bound(g["flows_it%d" % it])
        e_m = float(np.abs(M.movability_maps[it].cpu().numpy() - g["map_it%d" % it]).max())
        print(f"[{tag} it{it}] rejected {int(rec['reject'][it].sum())}/{rec['reject'][it].size}, flows {e_f:.3e} px (bound {EPS_FLOW:g}), patch magnitudes "
              f"{e_pm:.3e} (nearest to the threshold {float(np.abs(g['patch_mag_it%d' % it] / thr - 1).min()):.2e} relative), map {e_m:.3e} (bound {bound:.3e})")
        assert flows.shape == g["flows_it%d" % it].shape and e_f <= EPS_FLOW, (tag, it, e_f)
        assert e_pm <= np.sqrt(2.0) * EPS_FLOW  # a mean of bilinear samples of |flow|
        assert e_m <= bound, (tag, it, e_m, bound)


@pytest.mark.parametrize("case", CASES)
def test_open_loop_recorded_distributions(case):
    """(a) every iteration's sampling calls are fed the recorded distributions: patches, shifts and filter decisions equal the reference's, flows
    and maps within their bounds; the energies this stack would have handed over are compared with the recorded ones on the way."""
    g = np.load(os.path.join(GOLDEN, "movability_%s.npz" % case))
    n_it = int(g["settings"][2]) + 1
    energies = [g["energy_%s_it%d" % (role, it)] for it in range(n_it) for role in ("active", "passive")]
    M, rec = build(g, energies)
    torch.manual_seed(int(g["torch_seed"]))
    M(torch.from_numpy(g["x"]).cuda())
    compare_iterations(case + " open", g, M, rec)
    for i, (mine, want) in enumerate(zip(rec["energies"], energies)):
        assert (mine is None) == (want.size == 0)
        if mine is not None:
            print(f"[{case} open] energy {i}: max-abs vs recorded {float(np.abs(mine - want).max()):.3e}")


@pytest.mark.parametrize("case", CASES)
def test_closed_loop_forward(case):
    """(b) `forward` under the recorded seeds, nothing replaced: the same exact / bounded split for every iteration, then the final map, the total and
    the minimum movability."""
    g = np.load(os.path.join(GOLDEN, "movability_%s.npz" % case))
    M, rec = build(g)
    torch.manual_seed(int(g["torch_seed"]))
    final = M(torch.from_numpy(g["x"]).cuda())
    compare_iterations(case + " closed", g, M, rec)
    n_it = int(g["settings"][2]) + 1
    assert final is M.movability_maps[-1] and M.it == n_it - 1
    e_final = float(np.abs(final.cpu().numpy() - g["final_map"]).max())
    b_final = map_bound(g["flows_it%d" % (n_it - 1)])
    all_flows = np.concatenate([g["flows_it%d" % it] for it in range(n_it)], -1)
    e_total = float(np.abs(M.get_total_movability().cpu().numpy() - g["total_movability"]).max())
    b_total = map_bound(all_flows)
    e_min = float(np.abs(M.get_minimum_movability().cpu().numpy() - g["minimum_movability"]).max())
    b_min = max(map_bound(g["flows_it%d" % it]) for it in range(n_it))
    print(f"[{case} closed] final map {e_final:.3e} (bound {b_final:.3e}), total movability {e_total:.3e} (bound {b_total:.3e}), "
          f"minimum movability {e_min:.3e} (bound {b_min:.3e})")
    assert float(g["final_map"].max() - g["final_map"].min()) > 0.5  # the loop did not degenerate
    assert e_final <= b_final and e_total <= b_total and e_min <= b_min
    assert final.shape == (1, 1, 32, 32) and float(final.min()) >= 0 and float(final.max()) <= 1


def test_running_sum_total_equals_concatenation():
    """(c) `get_total_movability` from one magnitude sum per iteration equals the reference's way, `compute_mean_motion_map(cat(flows))`, to 1e-5: two
    fp32 sums of 24 positive terms in different order differ by at most 2 x 23 x 6e-8 relative (2.8e-6), and the minimum, the range and the value
    each carry that through the normalisation."""
    g = np.load(os.path.join(GOLDEN, "movability_default.npz"))
    M, _ = build(g)
    torch.manual_seed(int(g["torch_seed"]))
    x = torch.from_numpy(g["x"]).cuda()
    M(x)
    flows = M.flow_samples_per_iter
    assert len(flows) == 3 and sum(f.shape[-1] for f in flows) == 24
    want = flowstats.compute_mean_motion_map(torch.cat(flows, -1), normalize_per_sample=False, normalize=True)
    got = M.get_total_movability()
    err = (got - want).abs().max().item()
    print(f"[running sum] total movability vs concatenation {err:.3e}")
    assert got.shape == want.shape == (1, 1, 32, 32) and err <= 1e-5
    # the sums are kept: a second call computes none, and a replaced entry is recomputed
    kept = [s for _, s in M._map_sums]
    assert torch.equal(M.get_total_movability(), got) and all(a is b for a, b in zip(kept, (s for _, s in M._map_sums)))
    M.flow_samples_per_iter[1] = flows[1] * 2.0
    want2 = flowstats.compute_mean_motion_map(torch.cat(M.flow_samples_per_iter, -1))
    assert (M.get_total_movability() - want2).abs().max().item() <= 1e-5
    # sample_and_visualize_keypoints: the sampled masks and the tinted movie, nothing plotted
    kps, img = M.sample_and_visualize_keypoints(x, num_samples=5)
    assert kps.shape == (1, 128, 5) and img.shape == x.shape and torch.isfinite(img).all()
    _, img2 = M.sample_and_visualize_keypoints(x, sampled_keypoints=M.active_patches_per_iter[0], sampled_passive_patches=M.passive_patches_per_iter[1])
    assert img2.shape == x.shape and not torch.equal(img2, x)


def test_full_size_run_with_raft_and_keypoint_raft():
    """(d) shapes and invariants at full size: the IMU-conditioned base-4x4 predictor and the flow -> IMU model with synthetic weights, RAFT-large as
    the flow model and the keypoint RAFT (output_dim = 1) as keypoint predictor, 224^2."""
    def conj(m, seed):
        m.load_state_dict(weights(m.cfg, seed), strict=False)
        return m

    def raft(seed, output_dim=None):
        m = RAFT(_args(output_dim=output_dim))
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(seed, output_dim=output_dim).items()})
        return m

    pred = conj(CV.imu400_base_4x4patch_2frames_1tube(), 1)
    gen = masking.RotatedTableUniformMaskingGenerator(input_size=pred.mask_size, mask_ratio=0.99, clumping_factor=2)
    M = movability.MovabilityPredictor(
        predictor=pred, head_motion_predictor=conj(CV.imu400_8x8patch_2frames_1tube_flowbackrgb01(), 0), flow_model=raft(0), keypoint_predictor=raft(10, 1),
        temporal_dim=2, imagenet_normalize_inputs=True, mask_generator=gen, seed=0, raft_iters=12, num_initial_samples=4, num_samples_per_iteration=4,
        num_iters=2, sample_batch_size=4).requires_grad_(False).to("cuda")
    x = torch.from_numpy(S.raft_frames(1, 224, 224, 11)).cuda()
    final = M(x)
    assert final.shape == (1, 1, 224, 224)
    assert M.keypoints_distribution.shape == (1, 1, 224, 224) and float(M.keypoints_distribution.max()) == 1.0 and float(M.keypoints_distribution.min()) == 0.0
    lists = (M.movability_maps, M.flow_samples_per_iter, M.active_patches_per_iter, M.passive_patches_per_iter)
    assert all(len(v) == 3 for v in lists)
    for it in range(3):
        assert M.flow_samples_per_iter[it].shape == (1, 2, 224, 224, 4) and torch.isfinite(M.flow_samples_per_iter[it]).all()
        assert M.active_patches_per_iter[it].shape == M.passive_patches_per_iter[it].shape == (1, 2 * 56 * 56, 4)
        n_active = (~M.active_patches_per_iter[it][:, 56 * 56:]).sum(1)
        assert torch.all(n_active == n_active[0, 0]) and int(n_active[0, 0]) >= 1  # every sample moves the same number of patches
        assert not M.active_patches_per_iter[it][:, :56 * 56].any()
    for m in lists[0] + [M.get_total_movability(), M.get_minimum_movability()]:
        assert m.shape == (1, 1, 224, 224) and torch.isfinite(m).all() and float(m.min()) >= 0 and float(m.max()) <= 1
