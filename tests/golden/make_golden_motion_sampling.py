"""Goldens of the counterfactual motion-map sampling layer, recorded from the REFERENCE on the CPU (through ref_import.py):

  motion_filter.npz        `FlowSampleFilter` (cwm/models/sampling.py:128-286) on seeded blob flows (`synthetic.blob_flow_samples`): per case
                           the blob table, active patches, the reference's statistics / decisions for every subset of methods, its float64
                           evaluation and its own fp32 rounding of patch_mag (max relative difference from float64), a checksum of the flows.
  motion_sampler.npz       masks of `RotatedTableEnergyMaskingGenerator` (:11-126) and of `FlowGenerator.sample_patches_from_energy` under recorded seeds.
  motion_sampling_e2e.npz  the reference's own `FlowGenerator.sample_counterfactual_motion_map` (segmentation.py:434-477) on the tiny predictor and the
                           `synthetic.SyntheticFlow` stand-in: two movies (B=1 each: the reference's loop runs at B=1 only), S=8, two sample_batch_sizes, filter on and off.

The maker asserts the guard bands the GPU tests rely on: no per-sample statistic within 1e-3 (relative) of its threshold, no pixel magnitude within
1e-6 (relative) of the magnitude threshold (sqrt(u u + v v) in fp32, fused or not, is within 2 ulp = 2.4e-7 of exact: 1e-6 is four times that); an
offending pixel is scaled by 1 + 1e-5 and listed in the fixture.  Run: python tests/golden/make_golden_motion_sampling.py
"""
from __future__ import annotations

import itertools
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import ref_import  # noqa: E402
from counterfactualworldmodels_amd import config as C  # noqa: E402
from counterfactualworldmodels_amd import synthetic as S  # noqa: E402

METHODS = ["patch_magnitude", "flow_area", "num_corners"]
SUBSETS = [list(c) for n in (1, 2, 3) for c in itertools.combinations(METHODS, n)]
THR, AREA_THR, CORNER_THR = 5.0, 0.75, 2
TINY = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)


def tap_axis(size, grid):
    """(i0, i1) of F.interpolate(bilinear, align_corners=False) per destination index, float32 arithmetic as torch does it."""
    scale = np.float32(size) / np.float32(grid)
    src = np.maximum((np.arange(grid, dtype=np.float32) + np.float32(0.5)) * scale - np.float32(0.5), np.float32(0))
    i0 = np.minimum(src.astype(np.int64), size - 1)
    return i0, i0 + (i0 < size - 1)


def filter_plan(size, grid, num_b=2, num_s=12):
    """blobs [B,S,3,5], active [B,2 grid^2,S] (0 = active), nan_pixels [n,4] for one case (see the module docstring of the tests for the roles)."""
    ratio = size / grid
    blobs = np.zeros((num_b, num_s, 3, 5), dtype=np.float32)
    active = np.ones((num_b, 2 * grid * grid, num_s), dtype=bool)
    active[:, : grid * grid] = False  # frame 1 is all visible; the filter must not read it
    nan_pixels = []
    i0, i1 = tap_axis(size, grid)
    taps = set(i0.tolist()) | set(i1.tolist())
    free = [v for v in range(size) if v not in taps]  # rows / columns no bilinear tap reads

    def centre(p):
        return (p + 0.5) * ratio - 0.5

    def on(b, s, py, px):
        active[b, grid * grid + py * grid + px, s] = False

    for b in range(num_b):
        o = 2 * b  # the second movie is the first moved by two patches
        big, small = 1.2 * ratio + 6, 0.8 * ratio
        # 0: kept, one active patch under a blob
        on(b, 0, 6 + o, 5); blobs[b, 0, 0] = (centre(6 + o), centre(5), big, 14, -12)
        # 1: kept, a clumped 2 x 2 active set under a blob
        for dy in (0, 1):
            for dx in (0, 1):
                on(b, 1, 2 + o + dy, 6 + dx)
        blobs[b, 1, 0] = (centre(2.5 + o), centre(6.5), 1.5 * big, -16, 10)
        # 2: rejected by patch_magnitude alone: the blob is far from the active patch
        on(b, 2, grid - 3, grid - 3 - o); blobs[b, 2, 0] = (centre(2), centre(2 + o), big, 15, 15)
        # 3: rejected by flow_area alone: |flow| > 5 inside a disc that covers ~0.79 of the image but none of the corners
        on(b, 3, grid // 2, grid // 2); blobs[b, 3, 0] = ((size - 1) / 2, (size - 1) / 2, size * 60 / 224, 16.05 + b, 16.05)
        # 4: rejected by num_corners alone: two small blobs on two corners, the active patch under one of them
        on(b, 4, 0, 0); blobs[b, 4, 0] = (0, 0, small + 2, 14, 14 + b); blobs[b, 4, 1] = (0, size - 1, small + 2, -14, 14)
        # 5: an empty active set (patch_mag = 0 / 1e-12 = 0: rejected by patch_magnitude), a blob anyway
        blobs[b, 5, 0] = (centre(4), centre(4 + o), big, 12, 9)
        # 6: kept, active patches on the last grid row and column (the clamped bilinear neighbours), a blob on each
        for k, (py, px) in enumerate([(grid - 1, grid - 1), (grid - 1, 3 + o), (3 + o, grid - 1)]):
            on(b, 6, py, px); blobs[b, 6, k] = (centre(py), centre(px), small, 20, -21)
        # 7: NaN pixels: one under a tap of the active patch (patch_mag is NaN on both sides: never rejects by itself), three where no tap reads
        on(b, 7, 5, 6 + o); blobs[b, 7, 0] = (centre(5), centre(6 + o), big, 13, 13)
        nan_pixels += [(b, 7, int(i0[5]), int(i1[6 + o])), (b, 7, free[0], free[1]), (b, 7, free[2], int(i0[3])), (b, 7, int(i0[2]), free[-1])]
        # 8: rejected by flow_area and num_corners: everything moves
        on(b, 8, 3, 3); blobs[b, 8, 0] = ((size - 1) / 2, (size - 1) / 2, float(size), 40, -45)
        # 9: kept, two active patches, two blobs
        on(b, 9, 2, 2 + o); on(b, 9, grid - 4, 4); blobs[b, 9, 0] = (centre(2), centre(2 + o), big, 18, 5); blobs[b, 9, 1] = (centre(grid - 4), centre(4), big, 5, -18)
        # 10: rejected by patch_magnitude alone: background noise only
        on(b, 10, 4, grid - 5 - o)
        # 11: kept, a strong narrow blob
        on(b, 11, grid // 2 + 1, 2 + o); blobs[b, 11, 0] = (centre(grid // 2 + 1), centre(2 + o), small + 3, -30, 2)
    return blobs, active, np.array(nan_pixels, dtype=np.int64)


def run_filter_case(ns, tag, size, grid, seed):
    Ref = ns_sampling(ns).FlowSampleFilter
    blobs, active, nan_pixels = filter_plan(size, grid)
    act = torch.from_numpy(active)
    scaled = np.zeros((0, 4), dtype=np.int64)
    for _ in range(20):  # move every pixel magnitude out of the 1e-6 band around the threshold
        flows = S.blob_flow_samples(size, seed, blobs, scaled_pixels=scaled, nan_pixels=nan_pixels)
        mag64 = np.sqrt((flows.astype(np.float64) ** 2).sum(1))  # [B,H,W,S]
        with np.errstate(invalid="ignore"):
            close = np.argwhere(np.abs(mag64 / THR - 1.0) < 1e-6)
        if len(close) == 0:
            break
        scaled = np.concatenate([scaled, close[:, [0, 3, 1, 2]]], 0)
    else:
        raise AssertionError("pixel guard band not cleared")
    f32 = torch.from_numpy(flows)
    filt = Ref()
    with torch.no_grad():
        mag, _, pm32, _ = filt.compute_flow_magnitude(f32, act)
        _, _, pm64, _ = filt.compute_flow_magnitude(f32.double(), act)
        area = (mag > THR).flatten(1, 2).sum(1)
        corners = (mag > THR)[:, [0, 0, -1, -1], [0, -1, 0, -1]].sum(1)
        area64 = (torch.from_numpy(mag64) > THR).flatten(1, 2).sum(1)
        assert torch.equal(area, area64), "the fp32 and float64 counts differ: the pixel guard band is not doing its job"
        reject = np.zeros((len(SUBSETS),) + tuple(pm32.shape), dtype=bool)
        for i, sub in enumerate(SUBSETS):
            out, mask = Ref(filter_methods=sub)(f32.clone(), act)
            reject[i] = mask.amax((1, 2, 3)).numpy()
    ok = ~torch.isnan(pm64)
    assert torch.equal(torch.isnan(pm32), torch.isnan(pm64)) and int((~ok).sum()) >= 1
    rounding = float(((pm32.double() - pm64).abs() / pm64.abs().clamp(min=1e-30))[ok & (pm64 > 0)].max())
    frac = area.double() / (size * size)
    band_pm = float((pm64[ok] / THR - 1).abs().min())
    band_area = float((frac / AREA_THR - 1).abs().min())
    assert band_pm >= 1e-3 and band_area >= 1e-3, (band_pm, band_area)
    for i, sub in enumerate(SUBSETS[:3]):  # each method alone: both outcomes, and a sample only this method rejects
        others = np.zeros_like(reject[0])
        for j in range(3):
            if j != i:
                others |= reject[j]
        assert reject[i].any() and (~reject[i]).any() and (reject[i] & ~others).any(), sub
    assert (~reject[-1]).any()
    n_active = (~active[:, grid * grid:]).sum(1)
    print("[golden] filter %s: %d px scaled, patch_mag fp32 rounding %.2e, bands pm %.2e area %.2e, rejected %s, n_active max %d"
          % (tag, len(scaled), rounding, band_pm, band_area, reject[-1].astype(int).tolist(), n_active.max()))
    return {tag + "_size": np.array(size), tag + "_grid": np.array(grid), tag + "_seed": np.array(seed), tag + "_blobs": blobs,
            tag + "_active": np.packbits(active), tag + "_active_shape": np.array(active.shape), tag + "_nan_pixels": nan_pixels, tag + "_scaled_pixels": scaled,
            tag + "_checksum": np.array(S.flow_checksum(flows)), tag + "_patch_mag": pm32.numpy(), tag + "_patch_mag64": pm64.numpy(),
            tag + "_area_count": area.numpy().astype(np.int32), tag + "_corner_count": corners.numpy().astype(np.int32), tag + "_reject": reject,
            tag + "_patch_mag_rounding": np.array(rounding)}


def ns_sampling(ns):
    import importlib

    return importlib.import_module("cwm.models.sampling")


def run_filter_cases(ns):
    out = {"subsets": np.array(json.dumps(SUBSETS)), "thresholds": np.array([THR, AREA_THR, CORNER_THR])}
    out.update(run_filter_case(ns, "f224_g28", 224, 28, 101))
    out.update(run_filter_case(ns, "f224_g56", 224, 56, 102))
    out.update(run_filter_case(ns, "f96_g10", 96, 10, 103))
    np.savez_compressed(os.path.join(HERE, "motion_filter.npz"), **out)


sampler_energy = S.sampler_energy


SAMPLER_CASES = [  # (tag, input_size, energy side, kwargs, num_visible, one_hot)
    ("g28_v1", (2, 28, 28), 224, {}, 1, False),
    ("g28_v4", (2, 28, 28), 224, {}, 4, False),
    ("g28_v0", (2, 28, 28), 224, {}, 0, False),
    ("g56_v1", (2, 56, 56), 224, {}, 1, False),
    ("g28_cf2_v1", (2, 28, 28), 224, {"clumping_factor": 2}, 1, False),
    ("g56_cf2_v4", (2, 56, 56), 224, {"clumping_factor": 2}, 4, False),
    ("g28_max", (2, 28, 28), 224, {"pool_mode": "max"}, 4, False),
    ("g28_min", (2, 28, 28), 224, {"pool_mode": "min"}, 4, False),
    ("g28_temp2", (2, 28, 28), 224, {"temperature": 2.0}, 4, False),
    ("g28_pow4", (2, 28, 28), 224, {"energy_power": 4}, 4, False),
    ("g28_patchres", (2, 28, 28), 28, {}, 4, False),
    ("g28_onehot", (2, 28, 28), 28, {}, 1, True),
    ("g28_randvis", (2, 28, 28), 224, {"randomize_num_visible": True}, 4, False),
]


def run_sampler_cases(ns):
    Ref = ns_sampling(ns).RotatedTableEnergyMaskingGenerator
    out = {"cases": np.array(json.dumps([[t, list(i), e, k, v, o] for t, i, e, k, v, o in SAMPLER_CASES]))}
    for n, (tag, input_size, side, kw, num_visible, one_hot) in enumerate(SAMPLER_CASES):
        gen = Ref(input_size=input_size, mask_ratio=0, seed=11 + n, always_batch=True, eps=1e-16, resize=False, **kw)
        gen.num_visible = num_visible * gen.clumping_factor ** 2
        energy = torch.from_numpy(sampler_energy(2, side, 50 + n, one_hot))
        torch.manual_seed(1000 + n)
        masks = torch.stack([gen(energy) for _ in range(3)], -1)
        assert masks.shape == (2, 2 * input_size[1] * input_size[2], 3) and not masks[:, : input_size[1] * input_size[2]].any()
        out[tag] = np.packbits(masks.numpy())
        out[tag + "_shape"] = np.array(masks.shape)
        out[tag + "_attrs"] = np.array([gen.num_visible, gen.mask_ratio, gen.clumping_factor, gen.visible_frames], dtype=np.float64)
        if one_hot:
            e = energy.flatten(1)
            assert all((~masks[b, 28 * 28:, s]).nonzero().flatten().tolist() == [int(e[b].argmax())] for b in range(2) for s in range(3))
    # sample_patches_from_energy through a reference FlowGenerator (tiny predictor: mask_size (2, 4, 4)); S = 8
    G = ref_generator(ns, seed=0)
    x = torch.from_numpy(S.synthetic_frames(2, TINY, 41))
    G.set_input(x)
    energy = torch.from_numpy(sampler_energy(2, 32, 77))
    out["spe_energy"] = energy.numpy()
    out["spe_v1"] = G.sample_patches_from_energy(energy, num_samples=8, num_visible=1).numpy()
    out["spe_v2_beta"] = G.sample_patches_from_energy(energy, num_samples=8, num_visible=2, beta=3.0).numpy()
    out["spe_v0"] = G.sample_patches_from_energy(energy, num_samples=8, num_visible=0).numpy()
    out["spe_uniform"] = G.sample_patches_from_energy(None, num_samples=8, num_visible=1).numpy()
    out["spe_cf2"] = G.sample_patches_from_energy(energy, num_samples=8, num_visible=1, clumping_factor=2).numpy()
    out["spe_after_recreate"] = G.sample_patches_from_energy(energy, num_samples=8, num_visible=1).numpy()
    out["spe_rng_next"] = np.array(G.rng.randint(99999))  # where the wrapper's numpy stream stands after these calls
    np.savez_compressed(os.path.join(HERE, "motion_sampler.npz"), **out)
    print("[golden] motion_sampler.npz", len(SAMPLER_CASES), "sampler cases;", {k: v.shape for k, v in out.items() if k.startswith("spe_")})


def ref_generator(ns, seed=0, **kw):
    from make_golden import build_ref_model

    m = build_ref_model(ns, TINY, 3)
    m = m[0] if isinstance(m, tuple) else m
    return ns.segmentation.FlowGenerator(predictor=m, flow_model=S.SyntheticFlow(), imagenet_normalize_inputs=True, temporal_dim=2, seed=seed, **kw)


# The stand-in flow has |flow| of 9.5 - 15.3 px at the active patches and ~0.5 of the image above 11.9 px: patch_magnitude then rejects about half of the
# samples, every patch_mag is >= 1.5e-2 (relative) from 11.9 and every area fraction >= 0.15 from 0.6; no corner count can reach 5.
E2E_FILTER = {"filter_methods": METHODS, "flow_magnitude_threshold": 11.9, "flow_area_threshold": 0.6, "num_corners_threshold": 5}


def run_e2e_case(ns, params):
    """The reference's batch loop indexes `shifts[i]` for i < B S with S shifts (segmentation.py:323-331): it runs at B = 1 only, so the two movies
    are two calls, each on a fresh generator."""
    out = {"filter_params": np.array(json.dumps(params))}
    x = torch.from_numpy(S.synthetic_frames(2, TINY, 43))
    out["x"] = x.numpy()
    Filter = ns_sampling(ns).FlowSampleFilter
    all_rej, band = [], 1.0
    for movie in (0, 1):
        for sbs in (8, 3):
            for do_filter in (True, False):
                G = ref_generator(ns, seed=movie, flow_sample_filter=Filter(**params))
                with torch.no_grad():
                    flows, active, passive = G.sample_counterfactual_motion_map(x[movie:movie + 1], num_samples=8, sample_batch_size=sbs, do_filter=do_filter)
                tag = "m%d_sbs%d_%s" % (movie, sbs, "filter" if do_filter else "raw")
                out["flows_" + tag], out["active_" + tag], out["passive_" + tag] = flows.numpy(), active.numpy(), passive.numpy()
                out["shifts_" + tag] = np.array(G.shifts)
                if not do_filter:
                    f = Filter(**params)
                    mag, _, pm, _ = f.compute_flow_magnitude(flows.clone(), active)
                    frac = (mag > params["flow_magnitude_threshold"]).flatten(1, 2).sum(1) / (32 * 32)
                    _, mask = f(flows.clone(), active)
                    rej = mask.amax((1, 2, 3))
                    out["patch_mag_" + tag], out["area_frac_" + tag], out["reject_" + tag] = pm.numpy(), frac.numpy(), rej.numpy()
                    band = min(band, float((pm / params["flow_magnitude_threshold"] - 1).abs().min()), float((frac / params["flow_area_threshold"] - 1).abs().min()))
                    if sbs == 8:
                        all_rej.append(rej)
                        print("[golden] e2e movie", movie, "patch_mag", pm.numpy().round(3).tolist(), "area", frac.numpy().round(3).tolist(), "reject", rej.int().tolist())
        assert np.array_equal(out["reject_m%d_sbs8_raw" % movie], out["reject_m%d_sbs3_raw" % movie])
        assert np.array_equal(out["flows_m%d_sbs8_filter" % movie] == 0, np.broadcast_to(out["reject_m%d_sbs8_raw" % movie][:, None, None, None], out["flows_m%d_sbs8_filter" % movie].shape) | (out["flows_m%d_sbs8_raw" % movie] == 0))
    rej = torch.cat(all_rej)
    print("[golden] e2e band %.3e" % band)
    assert rej.any() and (~rej).any() and band >= 1e-2, band
    np.savez_compressed(os.path.join(HERE, "motion_sampling_e2e.npz"), **out)


def main():
    ns = ref_import.import_reference()
    assert ns.segmentation is not None, getattr(ns, "segmentation_error", None)
    torch.set_num_threads(8)
    if "--only-e2e" not in sys.argv:
        run_filter_cases(ns)
        run_sampler_cases(ns)
    run_e2e_case(ns, dict(E2E_FILTER))


if __name__ == "__main__":
    main()
