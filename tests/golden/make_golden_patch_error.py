"""Golden vectors for the patch-error methods of `PredictorBasedGenerator` (`get_error_on_target_region`, `error_with_mask`, `unmask_one_patch`,
`patch_idx_list_from_mask`; prediction.py:542-615) and for `greedy_unmask`, by RUNNING THE REFERENCE (this container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_patch_error.py

  patch_error.npz   TINY model (32 x 32, patch 8), seed 3, B = 3, 4 visible frame-2 patches per row: the masks after the reference's rectangularisation,
                    the reference's predicted tokens, a target mask different from the mask, a target different from x, and the reference's results
                    for the default call, average_error=False, frame=0, frame=None, target=, aggregate_over_patches=False, `error_with_mask` and the
                    two static methods; `dmax_*`: the largest |prediction - target| of each case (what the comparison's bound is made of).
                    greedy_*: one movie whose frame-1 patches 5, 10, 3 and 12 are raised by 8, 6, 4 and 2; the start mask has frame 0 visible and frame 1
                    masked except its patch 0; four steps of the search over ALL candidates, each candidate scored by the reference alone at batch 1
                    (`unmask_one_patch` + `get_error_on_target_region`).  Stored: the picks (token indices), the final mask, every step's best score and
                    its gap to the second best, and the bound C (2 dmax tau + tau^2), tau = 1e-3, that a parity-mode score may be off by.  The maker
                    FAILS unless every gap is at least 10 x that bound: the picks are then decided by the frames, not by rounding.
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

TAU = 1e-3  # the project's parity bound on predicted tokens (tests/test_model_gpu.py)
RAISED = {5: 8.0, 10: 6.0, 3: 4.0, 12: 2.0}  # frame-1 patch -> offset


def score_bound(C, dmax):
    return C * (2 * dmax * TAU + TAU * TAU)


def dmax_of(G, x, mask, target, frame):
    pred = G.predict(x, mask.clone(), frame=frame)
    return float((pred - target).abs().max())


def main():
    torch.set_num_threads(os.cpu_count() or 1)
    ns = ref_import.import_reference()
    cfg = MG.TINY
    seed, B = 3, 3
    m = MG.build_ref_model(ns, cfg, seed)
    G = ns.prediction.PredictorBasedGenerator(predictor=m, imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
    x = torch.from_numpy(S.synthetic_frames(B, cfg, seed))
    mask = torch.from_numpy(S.synthetic_masks(B, cfg, 4, seed))
    target_mask = torch.from_numpy(S.synthetic_masks(B, cfg, 6, seed + 10))
    target = torch.from_numpy(S.synthetic_frames(B, cfg, seed + 4))
    assert not torch.equal(mask, target_mask) and not torch.equal(x, target)
    out = {"seed": np.array(seed), "target_mask_seed": np.array(seed + 10), "target_seed": np.array(seed + 4)}
    with torch.no_grad():
        G.set_input(x)  # (the reference's mask_shape needs inp_shape)
        mask = G.mask_rectangularizer(mask.clone())
        out["mask"], out["target_mask"], out["target_x"] = mask.numpy(), target_mask.numpy(), target.numpy()
        out["y_tokens"] = m(G._preprocess(x), mask.clone()).numpy()
        calls = {
            "default": dict(),
            "map": dict(average_error=False),
            "frame0": dict(frame=0),
            "frame0_map": dict(frame=0, average_error=False),
            "each": dict(frame=None),
            "each_map": dict(frame=None, average_error=False),
            "target": dict(target=target),
            "target_map": dict(target=target, average_error=False),
            "pixels": dict(aggregate_over_patches=False),
        }
        for name, kw in calls.items():
            out[name] = G.get_error_on_target_region(x, mask.clone(), target_mask, **kw).numpy()
            out["dmax_" + name] = np.array(dmax_of(G, x, mask, kw.get("target", x), kw.get("frame", -1)))
            print("[golden] %-11s %s dmax %.3f" % (name, out[name].shape, out["dmax_" + name]))
        G.set_input(x)
        out["error_with_mask"] = G.error_with_mask(mask.clone()).numpy()

        # the two static methods
        U = ns.prediction.PredictorBasedGenerator.unmask_one_patch
        shape = (2, 4, 4)
        full = torch.ones(B, cfg.num_tokens, dtype=torch.bool)
        out["unmask_token"] = U(full, idx=21).numpy()
        out["unmask_hw"] = U(full, idx=(1, 2), mask_shape=shape, frame=1).numpy()
        out["unmask_thw"] = U(full, idx=[1, 2, 3], mask_shape=shape).numpy()
        out["unmask_bthw"] = U(full, idx=[2, 1, 0, 3], mask_shape=shape).numpy()
        assert full.all()  # inplace=False
        lst = ns.prediction.PredictorBasedGenerator.patch_idx_list_from_mask(mask.view(B, *shape))
        out["patch_idx_list"] = np.array([[int(v) for v in p] for p in lst], dtype=np.int64)

        # the greedy search, by the reference's own methods at batch 1
        n = cfg.tokens_per_frame
        gw = cfg.img_size[1] // cfg.patch
        xg = torch.from_numpy(S.synthetic_frames(1, cfg, seed)).clone()
        for patch, up in RAISED.items():
            i, j = divmod(patch, gw)
            xg[0, 1, :, i * cfg.patch:(i + 1) * cfg.patch, j * cfg.patch:(j + 1) * cfg.patch] += up
        cur = torch.zeros(1, 2 * n, dtype=torch.bool)
        cur[0, n + 1:] = True
        region_mask = torch.ones(1, 2 * n, dtype=torch.bool)
        region_mask[0, n:] = False  # the region is what the target mask leaves visible: every patch of frame 1
        out["greedy_x"], out["greedy_mask"] = xg.numpy(), cur.numpy().copy()
        G.set_input(xg)
        rng = torch.get_rng_state()
        picks, best, gaps, bounds = [], [], [], []
        for step in range(4):
            cand = [t for t in range(n, 2 * n) if bool(cur[0, t])]
            scores, dmax = [], 0.0
            for t in cand:
                row = U(cur, idx=t)
                scores.append(float(G.get_error_on_target_region(xg, row, region_mask)))
                dmax = max(dmax, dmax_of(G, xg, row, xg, -1))
            order = np.lexsort((np.array(cand), np.array(scores)))
            pick, gap, bound = cand[order[0]], scores[order[1]] - scores[order[0]], score_bound(cfg.in_chans, dmax)
            print("[golden] greedy step %d: pick token %d (frame-1 patch %d) score %.4f gap %.4f = %.1f x bound %.4f" % (step, pick, pick - n, scores[order[0]], gap, gap / bound, bound))
            assert gap >= 10 * bound, (step, gap, bound)
            picks.append(pick), best.append(scores[order[0]]), gaps.append(gap), bounds.append(bound)
            cur = U(cur, idx=pick)
        assert torch.equal(rng, torch.get_rng_state())  # single rows: nothing was rectangularised
        assert [p - n for p in picks] == list(RAISED), picks
        out.update(greedy_picks=np.array(picks, dtype=np.int64), greedy_scores=np.array(best, dtype=np.float32), greedy_gaps=np.array(gaps, dtype=np.float32),
                   greedy_bounds=np.array(bounds, dtype=np.float32), greedy_final_mask=cur.numpy())
    path = os.path.join(HERE, "patch_error.npz")
    np.savez_compressed(path, **out)
    print("[golden] patch_error.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
