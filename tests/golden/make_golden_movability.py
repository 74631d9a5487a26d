"""Goldens of the keypoint RAFT (`load_raft_model(None, output_dim=1)`, cwm/models/raft/raft_model.py:152-161, 257-272) and of the reference's
`MovabilityPredictor` (cwm/models/movability.py:13-360), recorded by RUNNING THE REFERENCE on the CPU (through ref_import.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_movability.py [raft] [movability]

  raft_keypoint_224_b1.npz      224^2, B = 1: the multi-frame call at 24 iterations and at 1, the two-image call at both (its low-resolution flow;
                                its second output equals the multi-frame map bit for bit, asserted here), T = 1 (the frame repeated), the reference's `predict_keypoints_distribution` of the 24-iteration map and R = max - min of sigmoid(map)^8
  raft_keypoint_128x160_t3.npz  128 x 160, T = 3, forward and backward
  raft_keypoint_224_b2.npz      224^2, B = 2
                                (weights `synthetic.raft_state_dict(seed, output_dim=1)`, frames `synthetic.raft_frames`; every output with `drift_*`,
                                the reference's own fp32-vs-float64 difference; the 183 keys / shapes and the parameter count)
  movability_default.npz        the reference `MovabilityPredictor` on the tiny models of head_motion_driver.npz, the `synthetic.SyntheticFlow` /
  movability_keypoints.npz      `synthetic.SyntheticKeypoints` stand-ins, a [1,2,3,32,32] movie, 8 + 2 x 8 samples, sample_batch_size 4: per iteration
                                the energies handed to the sampler, patches, shifts, filter decisions, patch magnitudes, flows, movability map; total
                                and minimum movability and the final map.  `default`: the constructor's defaults; `keypoints`:
                                initialize_from_keypoints, iterate_from_keypoints, sample_passives_from_movable, no per-iteration update.
  movability_defaults.json      the defaults of the reference constructor's own keyword arguments

Guard condition of the closed loop (asserted here, relied on by tests/test_movability_gpu.py): from iteration 1 on the sampler's energy comes from
flows, which differ from the reference's in the last digits on another stack.  Every fixture's seed is one under which the reference ALONE is stable:
the loop is re-run three times with every energy e handed to `sample_patches_from_energy` replaced by e (1 + 1e-3 u) + 1e-3 max(e) u' (u, u' uniform
in [-1, 1]) and must draw the same patches and shifts and take the same filter decisions; every patch magnitude is at least 1e-2 (relative) from
the threshold; every iteration keeps at least one sample and rejects at least one; the final map is not constant.  A seed that fails is skipped (at most
20 are tried) and the one used is recorded.
"""
from __future__ import annotations

import importlib
import inspect
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/: the tiny configs
sys.path.insert(0, ROOT)

import ref_import  # noqa: E402
from make_golden_raft import raft_module, run_both  # noqa: E402
from counterfactualworldmodels_amd import synthetic as S  # noqa: E402

POWER = 8


# ---- the keypoint RAFT ---------------------------------------------------------------------------------------------------------------------
def build_keypoint_raft(rm, seed: int, multiframe: bool = True):
    args = rm.get_args("")
    args.multiframe, args.scale_inputs, args.output_dim = multiframe, True, 1
    m = rm.RAFT(args)
    sd = m.state_dict()
    n_params = sum(v.numel() for v in m.parameters())
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(seed, output_dim=1).items()})
    return m.eval().requires_grad_(False), [(k, list(v.shape)) for k, v in sd.items()], n_params


def run_raft_cases(ns):
    rm = raft_module()
    t0 = time.time()
    # ---- 224^2, B = 1
    m, keys, n_params = build_keypoint_raft(rm, 10)
    assert len(keys) == 183 and [k for k, _ in keys[-4:]] == ["output_block.0.weight", "output_block.0.bias", "output_block.2.weight", "output_block.2.bias"]
    x = torch.from_numpy(S.raft_frames(1, 224, 224, 11))
    out = {"seed": np.array(10), "frames_seed": np.array(11), "keys": np.array(json.dumps(keys)), "num_parameters": np.array(n_params), "power": np.array(POWER)}

    def two_image(mm, dt, iters):
        xx = x.to(dt) * 255.0
        return mm._forward_two_images(xx[:, 0], xx[:, 1], iters=iters, test_mode=True)

    for iters in (24, 1):
        (y,), d = run_both(m, lambda mm, dt: mm(x.to(dt), iters=iters))
        (lo, up), d2 = run_both(m, lambda mm, dt: two_image(mm, dt, iters))
        assert y.shape == (1, 1, 1, 224, 224) and up.shape == (1, 1, 224, 224) and lo.shape == (1, 2, 28, 28)
        assert np.array_equal(y[:, 0], up)
        out["map_it%d" % iters], out["drift_it%d" % iters] = y, np.array(d)
        out["two_low_it%d" % iters], out["drift_two_it%d" % iters] = lo, np.array(d2)  # (the second output is map_it*[:, 0], bit for bit: asserted above)
    (y1,), d1 = run_both(m, lambda mm, dt: mm(x[:, :1].to(dt), iters=24))
    out["map_t1"], out["drift_t1"] = y1, np.array(d1)

    class _Keypoints:  # the reference's two methods (prediction.py:816-828) around the model
        keypoint_predictor = m
        predict_keypoints_map = ns.prediction.PredictorBasedGenerator.predict_keypoints_map
        predict_keypoints_distribution = ns.prediction.PredictorBasedGenerator.predict_keypoints_distribution

    with torch.no_grad():
        dist = _Keypoints().predict_keypoints_distribution(x, power=POWER)
    p = torch.from_numpy(out["map_it24"]).sigmoid() ** POWER
    R = float(p.max() - p.min())
    assert R >= 0.2, R
    out["distribution"], out["R"] = dist.numpy(), np.array(R)
    np.savez_compressed(os.path.join(HERE, "raft_keypoint_224_b1.npz"), **out)
    print("[golden] raft_keypoint_224_b1: map [%.2f, %.2f] std %.2f, R %.3f, drift it24 %.2e it1 %.2e t1 %.2e, %d parameters (%.0fs)"
          % (out["map_it24"].min(), out["map_it24"].max(), out["map_it24"].std(), R, out["drift_it24"], out["drift_it1"], d1, n_params, time.time() - t0))
    # ---- 128 x 160, T = 3, forward and backward
    m, _, _ = build_keypoint_raft(rm, 12)
    x3 = torch.from_numpy(S.raft_frames(1, 128, 160, 13, shift=(2, -3), frames=3))
    (yf,), df = run_both(m, lambda mm, dt: mm(x3.to(dt), iters=24))
    (yb,), db = run_both(m, lambda mm, dt: mm(x3.to(dt), iters=24, backward=True))
    assert yf.shape == (1, 2, 1, 128, 160)
    np.savez_compressed(os.path.join(HERE, "raft_keypoint_128x160_t3.npz"), map_fwd=yf, map_bwd=yb, seed=np.array(12), frames_seed=np.array(13),
                        shift=np.array([2, -3]), drift_fwd=np.array(df), drift_bwd=np.array(db))
    print("[golden] raft_keypoint_128x160_t3 drift %.2e / %.2e (%.0fs)" % (df, db, time.time() - t0))
    # ---- 224^2, B = 2
    m, _, _ = build_keypoint_raft(rm, 14)
    x2 = torch.from_numpy(S.raft_frames(2, 224, 224, 15))
    (y2,), d2 = run_both(m, lambda mm, dt: mm(x2.to(dt), iters=24))
    np.savez_compressed(os.path.join(HERE, "raft_keypoint_224_b2.npz"), map=y2, seed=np.array(14), frames_seed=np.array(15), drift=np.array(d2))
    print("[golden] raft_keypoint_224_b2 %s drift %.2e (%.0fs)" % (y2.shape, d2, time.time() - t0))


# ---- MovabilityPredictor -------------------------------------------------------------------------------------------------------------------
NUM_INITIAL, NUM_PER_ITER, NUM_ITERS, SBS = 8, 8, 2, 4
MOVIE_SEED = 31
# All three methods run, but only patch_magnitude can reject: the stand-in flow moves the whole image, so a live area or corner test would reject every
# sample (both are covered by motion_filter.npz); an area fraction cannot exceed 2 and there are four corners.  The magnitude threshold sits near
# the median patch magnitude of this stack so that every iteration keeps some samples and rejects some.
FILTER = {"filter_methods": ["patch_magnitude", "flow_area", "num_corners"], "flow_magnitude_threshold": 12.6, "flow_area_threshold": 2.0,
          "num_corners_threshold": 5}
CONFIGS = {
    "default": {},
    "keypoints": {"initialize_from_keypoints": True, "iterate_from_keypoints": True, "sample_passives_from_movable": True,
                  "update_distribution_per_iteration": False},
}


def movability_module():
    return importlib.import_module("cwm.models.movability")


def build_ref_predictor(ns, seed, kwargs, noise_seed=None):
    """The reference MovabilityPredictor with recording hooks; `noise_seed`: perturb every energy handed to the sampler (the guard runs)."""
    from make_golden import build_ref_conj
    from make_golden_head_motion import build_ref_tiny_flow2imu
    from test_conj_oracle import TINY_CONJ
    from test_head_motion_cpu import TINY_FLOW2IMU

    pred = build_ref_conj(ns, TINY_CONJ, 5)
    f2i, _ = build_ref_tiny_flow2imu(ns, TINY_FLOW2IMU, 6)
    gen = ns.masking.RotatedTableUniformMaskingGenerator(input_size=pred.mask_size, mask_ratio=0.9, clumping_factor=2)
    Filter = importlib.import_module("cwm.models.sampling").FlowSampleFilter
    G = movability_module().MovabilityPredictor(
        predictor=pred, head_motion_predictor=f2i, flow_model=S.SyntheticFlow(), keypoint_predictor=S.SyntheticKeypoints(), temporal_dim=2,
        imagenet_normalize_inputs=True, mask_generator=gen, seed=seed, flow_sample_filter=Filter(**FILTER),
        num_initial_samples=NUM_INITIAL, num_samples_per_iteration=NUM_PER_ITER, num_iters=NUM_ITERS, sample_batch_size=SBS, **kwargs)
    rec = {"energies": [], "shifts": [], "reject": [], "patch_mag": [], "raw_flows": []}
    noise = np.random.Generator(np.random.PCG64(noise_seed)) if noise_seed is not None else None

    spe = G.sample_patches_from_energy

    def sample_patches_from_energy(energy=None, **kw):
        rec["energies"].append(None if energy is None else energy.detach().clone().numpy())
        if noise is not None and energy is not None:
            u = torch.from_numpy(noise.uniform(-1, 1, size=tuple(energy.shape)).astype(np.float32))
            u2 = torch.from_numpy(noise.uniform(-1, 1, size=tuple(energy.shape)).astype(np.float32))
            energy = energy * (1 + 1e-3 * u) + 1e-3 * energy.max() * u2
        return spe(energy=energy, **kw)

    G.sample_patches_from_energy = sample_patches_from_energy
    filt = G.flow_sample_filter
    filt_forward = filt.forward

    def forward(flow_samples, active_patches):
        rec["raw_flows"].append(flow_samples.detach().clone().numpy())
        rec["patch_mag"].append(filt.compute_flow_magnitude(flow_samples.clone(), active_patches)[2].numpy())
        flows, mask = filt_forward(flow_samples, active_patches)
        rec["reject"].append(mask.amax((1, 2, 3)).numpy().astype(bool))
        return flows, mask

    filt.forward = forward
    scmm = G.sample_counterfactual_motion_map

    def sample_counterfactual_motion_map(*a, **kw):
        r = scmm(*a, **kw)
        rec["shifts"].append(np.array(G.shifts, dtype=np.int32))
        return r

    G.sample_counterfactual_motion_map = sample_counterfactual_motion_map
    return G, rec


def run_loop(ns, seed, kwargs, x, noise_seed=None):
    G, rec = build_ref_predictor(ns, seed, kwargs, noise_seed)
    with torch.no_grad():
        torch.manual_seed(1000 + seed)
        final = G(x)
    return G, rec, final


def discrete_trace(G, rec):
    return ([p.numpy() for p in G.active_patches_per_iter], [p.numpy() for p in G.passive_patches_per_iter], rec["shifts"], rec["reject"])


def same_trace(a, b):
    return all(len(u) == len(v) and all(np.array_equal(p, q) for p, q in zip(u, v)) for u, v in zip(a, b))


def run_movability_case(ns, tag, kwargs):
    g = np.random.Generator(np.random.PCG64(MOVIE_SEED))
    x = torch.from_numpy(g.random((1, 2, 3, 32, 32), dtype=np.float32))
    thr = FILTER["flow_magnitude_threshold"]
    for seed in range(20):
        G, rec, final = run_loop(ns, seed, kwargs, x)
        trace = discrete_trace(G, rec)
        n_it = NUM_ITERS + 1
        assert len(G.movability_maps) == len(rec["reject"]) == len(rec["shifts"]) == n_it and len(rec["energies"]) == 2 * n_it
        pm = np.concatenate([p.reshape(-1) for p in rec["patch_mag"]])
        band = float(np.abs(pm / thr - 1).min())
        both = all(r.any() and (~r).any() for r in rec["reject"])
        varied = float(final.max() - final.min()) > 0.5
        stable = all(same_trace(trace, discrete_trace(*run_loop(ns, seed, kwargs, x, noise_seed=100 * seed + n)[:2])) for n in range(3))
        print("[golden] movability %s seed %d: rejected %s, patch_mag [%.2f, %.2f] band %.2e, stable under perturbation %s"
              % (tag, seed, [int(r.sum()) for r in rec["reject"]], pm.min(), pm.max(), band, stable))
        if both and varied and stable and band >= 1e-2:
            break
    else:
        raise AssertionError("no seed in 0..19 meets the guard condition for " + tag)
    with torch.no_grad():
        total, minimum = G.get_total_movability(), G.get_minimum_movability()
    out = {"x": x.numpy(), "seed": np.array(seed), "torch_seed": np.array(1000 + seed), "kwargs": np.array(json.dumps(kwargs)),
           "filter_params": np.array(json.dumps(FILTER)), "settings": np.array([NUM_INITIAL, NUM_PER_ITER, NUM_ITERS, SBS]), "band": np.array(band),
           "total_movability": total.numpy(), "minimum_movability": minimum.numpy(), "final_map": final.numpy(),
           "seed_pred": np.array(5), "seed_f2i": np.array(6)}
    for it in range(n_it):
        for j, role in enumerate(("active", "passive")):
            e = rec["energies"][2 * it + j]
            out["energy_%s_it%d" % (role, it)] = np.zeros((0,), dtype=np.float32) if e is None else e
        out["active_it%d" % it], out["passive_it%d" % it] = trace[0][it], trace[1][it]
        out["shifts_it%d" % it], out["reject_it%d" % it], out["patch_mag_it%d" % it] = rec["shifts"][it], rec["reject"][it], rec["patch_mag"][it]
        out["flows_it%d" % it], out["map_it%d" % it] = G.flow_samples_per_iter[it].numpy(), G.movability_maps[it].numpy()
        out["raw_flows_it%d" % it] = rec["raw_flows"][it]
    np.savez_compressed(os.path.join(HERE, "movability_%s.npz" % tag), **out)
    print("[golden] movability_%s.npz seed %d, final map range %.3f" % (tag, seed, float(final.max() - final.min())))


def write_defaults():
    sig = inspect.signature(movability_module().MovabilityPredictor.__init__)
    d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    with open(os.path.join(HERE, "movability_defaults.json"), "w") as fh:
        json.dump(d, fh, indent=1, sort_keys=True)
        fh.write("\n")


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ns = ref_import.import_reference()
    assert ns.segmentation is not None, getattr(ns, "segmentation_error", None)
    only = sys.argv[1:]
    if not only or "raft" in only:
        run_raft_cases(ns)
    if not only or "movability" in only:
        write_defaults()
        for tag, kwargs in CONFIGS.items():
            run_movability_case(ns, tag, kwargs)


if __name__ == "__main__":
    main()
