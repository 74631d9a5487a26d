"""Golden vectors for the mask morphology (`masking.patch_distance_transform`, `masking.patches_adjacent_to_visible`; masking.py:32-71) and for the two
generator methods built on it (`get_nearby_patches` prediction.py:345-351, `generate_cutout_mask` prediction.py:650-659), by RUNNING THE REFERENCE (this
container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mask_morphology.py

  mask_morphology.npz   grids 3x3, 3x7, 4x5, 5x4, 7x7, 8x6, 14x14, 17x29 and 28x28, each as one [2,3,h,w] batch of six masks: 2 %, 50 % and 97 % masked
                        (torch.rand(generator seed) < density), all masked, all visible, and one visible corner cell.  Per grid `g<h>x<w>_`:
                          mask (packed bits), dist_self / dist_noself (float32), adj_r1 .. adj_r3 (bool, packed), adj_r0 (float32: the soft branch) and
                          adj_sized_r1: the same masks flat, through size=(h, w).
                        TINY generator (32 x 32, patch 8: a 4 x 4 grid, T = 2), `near_*`: get_nearby_patches of a [3,32] mask for radius 1, 2, 0, None and
                        upsample=True; `cutout_*`: generate_cutout_mask(frame 0 and 1, radius 1 and 0, (h, w) patch lists with the default stride and
                        stride=1, one movie: with B > 1 the reference writes into a stride-0 expand and raises); `cutout_default_frame_error`: the text of the exception the reference raises for its own default frame=-1.

`EnergySampleUnmask` (perturbation.py:589-640) is not recorded, because it does not run: with num_visible set, `perturb` calls
`masking.EnergyMaskingGenerator`, which does not exist (AttributeError); with radius set and num_visible None, `energy[:, frame:frame+1] * nearby_mask`
multiplies [B,1,H,W] by [B*T,1,H,W] and raises for B > 1 and T > 1.  Both calls are made below and their exception types stored
(`energy_sample_unmask_errors`), so that a reference in which they start to work is noticed.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_import  # noqa: E402
import make_golden as MG  # noqa: E402
from counterfactualworldmodels_amd import synthetic as S  # noqa: E402

GRIDS = [(3, 3), (3, 7), (4, 5), (5, 4), (7, 7), (8, 6), (14, 14), (17, 29), (28, 28)]
DENSITIES = (0.02, 0.5, 0.97)


def grid_masks(h, w, seed):
    """[2,3,h,w] bool: three densities, all masked, all visible, one visible corner"""
    g = torch.Generator().manual_seed(seed)
    ms = [torch.rand((h, w), generator=g) < d for d in DENSITIES]
    ms += [torch.ones((h, w), dtype=torch.bool), torch.zeros((h, w), dtype=torch.bool)]
    corner = torch.ones((h, w), dtype=torch.bool)
    corner[h - 1, 0] = False
    ms.append(corner)
    return torch.stack(ms, 0).view(2, 3, h, w)


def main():
    ns = ref_import.import_reference()
    M = ns.masking
    out = {"grids": np.asarray(GRIDS), "densities": np.asarray(DENSITIES)}
    for i, (h, w) in enumerate(GRIDS):
        m = grid_masks(h, w, 100 + i)
        k = "g%dx%d_" % (h, w)
        out[k + "mask"] = np.packbits(m.numpy())
        out[k + "dist_self"] = M.patch_distance_transform(m.clone(), self_mask=True).numpy()
        out[k + "dist_noself"] = M.patch_distance_transform(m.clone(), self_mask=False).numpy()
        for r in (1, 2, 3):
            a = M.patches_adjacent_to_visible(m.clone(), radius=r)
            assert a.dtype == torch.bool
            out[k + "adj_r%d" % r] = np.packbits(a.numpy())
        out[k + "adj_r0"] = M.patches_adjacent_to_visible(m.clone(), radius=0).numpy()
        a = M.patches_adjacent_to_visible(m.clone().view(6, -1), radius=1, size=(h, w))
        assert tuple(a.shape) == (6, 1, h, w)
        out[k + "adj_sized_r1"] = np.packbits(a.numpy())
        assert M.patches_adjacent_to_visible(m, radius=None) is m

    cfg = MG.TINY
    model = MG.build_ref_model(ns, cfg, 3)
    G = ns.prediction.PredictorBasedGenerator(predictor=model, imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
    x = torch.from_numpy(S.synthetic_frames(3, cfg, 3))
    G.set_input(x)
    g = torch.Generator().manual_seed(9)
    mask = torch.rand((3, 32), generator=g) < 0.7
    out["near_mask"] = mask.numpy()
    for r in (1, 2):
        out["near_r%d" % r] = G.get_nearby_patches(mask.clone(), radius=r).numpy()
    out["near_r0"] = G.get_nearby_patches(mask.clone(), radius=0).numpy()
    out["near_none"] = G.get_nearby_patches(mask.clone(), radius=None).numpy()
    out["near_r1_up"] = G.get_nearby_patches(mask.clone(), radius=1, upsample=True).numpy()
    out["near_r1_shape"] = G.get_nearby_patches(mask.clone(), radius=1, shape=(1, 4, 8)).numpy()
    G.set_input(x[:1])  # (with B > 1 the reference's all-visible mask is a stride-0 expand and the cutout's row assignment raises: one movie)
    pix = [[9, 17], [30, 2]]   # image coordinates: default stride 32 // 4 = 8 -> patches (1, 2), (3, 0)
    cells = [[0, 3], [2, 2], [3, 1]]
    out["cutout_pix"], out["cutout_cells"] = np.asarray(pix), np.asarray(cells)
    for f in (0, 1):
        for r in (1, 0):
            out["cutout_f%d_r%d_pix" % (f, r)] = G.generate_cutout_mask(pix, radius=r, frame=f).numpy()
            out["cutout_f%d_r%d_cells" % (f, r)] = G.generate_cutout_mask(cells, radius=r, stride=1, frame=f).numpy()
    try:
        G.generate_cutout_mask(pix)
        raise SystemExit("the reference's generate_cutout_mask(frame=-1) now runs: record it")
    except (RuntimeError, IndexError, ValueError) as e:
        out["cutout_default_frame_error"] = np.asarray(type(e).__name__ + ": " + str(e).splitlines()[0][:120])

    errs = []
    P = ns.perturbation
    for kw in (dict(num_visible=4), dict(radius=1)):
        try:
            pert = P.EnergySampleUnmask(patch_size=(1, 8, 8), **kw)
            m2 = torch.rand((3, 32), generator=g) < 0.7
            pert(x, m2, energy=torch.rand((3, 2, 32, 32), generator=g))
            raise SystemExit("the reference's EnergySampleUnmask(%s) now runs: port it" % kw)
        except SystemExit:
            raise
        except Exception as e:  # noqa: BLE001 (whatever it raises is the record)
            errs.append("%s -> %s" % (sorted(kw), type(e).__name__))
    out["energy_sample_unmask_errors"] = np.asarray(errs)
    path = os.path.join(HERE, "mask_morphology.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", errs, str(out["cutout_default_frame_error"]))


if __name__ == "__main__":
    main()
