"""Timings of seed selection on the GPU, in one session, at 224 x 224, P = 8, batch 1 and 8:

  * `cwm_seed_select` alone through `select_seeds_device` (the allocation of its outputs and workspace is inside) for K = 8 and K = 64, as pixels and as cells
  * the same inputs through the package's torch composition (`seed_select.select_seeds_torch`) on the same GPU
  * one `segment_scene` round of 8 seeds (ViT-B/8 at synthetic weights, RAFT at random weights, S = 8) with seed_mode="peaks" against seed_mode="sample",
    alternated call by call

    python tools/seed_step.py [--reps 20] [--raft-iters 12] [--mode fast|parity] [--json PATH]
    python tools/seed_step.py --trace     # under `rocprofv3 --kernel-trace --stats`: only library calls, over many distinct maps (see trace())

Device events around work that is synchronised before it is read; every shape is warmed up first; calls alternate and medians are reported.  Prints one JSON
line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from counterfactualworldmodels_amd import _lib, config as C, seed_select as SS, segmentation, synthetic as S, vmae  # noqa: E402
from counterfactualworldmodels_amd.raft import RAFT, _args  # noqa: E402
from tools.segment_step import alternate  # noqa: E402

H = W = 224
P = 8


def score_map(B, seed):
    """[B,H,W] on the device: smooth bumps on a noise floor, as a keypoint distribution looks"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    m = 0.02 * g.random((B, H, W), dtype=np.float32)
    for b in range(B):
        for _ in range(24):
            cy, cx, s, h = g.uniform(0, H), g.uniform(0, W), g.uniform(3, 12), g.uniform(0.2, 1.0)
            m[b] += (h * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))).astype(np.float32)
    return torch.from_numpy(m).cuda()


def select_alone(B, K, reps):
    """us per call of the library call (20 calls per timing) and of the torch composition, pixels and cells form"""
    m = score_map(B, K + B)
    cells = SS.select_seeds_device(m, K, P, radius=2).pooled.clone()
    kw = dict(radius=2, peaks_only=True, rel_thresh=0.1)
    out = {"input_bytes": m.numel() * 4}
    for form, src, extra in (("pixels", m, {}), ("cells", cells, {"cells": True})):
        calls = {"select": lambda: [SS.select_seeds_device(src, K, P, **kw, **extra) for _ in range(20)],
                 "torch_composition": lambda: SS.select_seeds_torch(src, K, P, **kw, **extra)}
        res, ref = SS.select_seeds_device(src, K, P, **kw, **extra), SS.select_seeds_torch(src, K, P, **kw, **extra)
        torch.cuda.synchronize()
        o = {"stats": res.stats.tolist(), "equals_torch": all(torch.equal(getattr(res, k), getattr(ref, k)) for k in SS.SeedSelection.__slots__)}
        for name, t in alternate(calls, reps).items():
            per = 1 if name == "torch_composition" else 20
            o[name + "_us"] = {"median": round(t["median_ms"] * 1e3 / per, 2), "min": round(t["min_ms"] * 1e3 / per, 2)}
        out[form] = o
    return out


def trace():
    """For a kernel trace: 200 library calls per batch size, each on a map of its own.  At batch 8 the 200 maps are 321 MB, more than the 256 MB last-level
    cache, so a map's earlier visit cannot serve its pool pass; at batch 1 they are 40 MB and may all be cache-resident."""
    for B in (1, 8):
        maps = [score_map(B, 0)]
        maps += [maps[0] + 1e-3 * i for i in range(1, 200)]
        torch.cuda.synchronize()
        for _ in range(2):
            for m in maps:
                SS.select_seeds_device(m, 8, P, radius=2, peaks_only=True, rel_thresh=0.1)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="fast", choices=("fast", "parity"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--raft-iters", type=int, default=12)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    if args.trace:
        return trace()
    out = {"device": torch.cuda.get_device_name(0), "mode": args.mode, "raft_iters": args.raft_iters}
    for B in (1, 8):
        for K in (8, 64):
            out["B%d_K%d" % (B, K)] = select_alone(B, K, args.reps)

    cfg = C.CONFIGS["base_8x8patch_2frames_1tube"]
    m = vmae.PretrainVisionTransformer(cfg, mode=args.mode)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 0).items()})
    raft = RAFT(_args(mixed_precision=(args.mode == "fast")))
    raft.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(0).items()})
    G = segmentation.FlowGenerator(predictor=m.cuda().eval(), flow_model=raft.cuda().eval(), imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
    kw = dict(num_seeds=8, num_iters=1, num_samples=8, raft_iters=args.raft_iters)
    for B in (1, 8):
        x = torch.from_numpy(S.synthetic_frames(B, cfg, 0)).cuda()
        dist = score_map(B, 99)
        gen = torch.Generator(device="cuda").manual_seed(0)
        calls = {"scene_round_sample": lambda: G.segment_scene(x, seed_distribution=dist, generator=gen, **kw),
                 "scene_round_peaks": lambda: G.segment_scene(x, seed_distribution=dist, seed_mode="peaks", seed_radius=2, seed_rel_thresh=0.1, **kw)}
        for fn in calls.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        out["B%d_round" % B] = alternate(calls, max(3, args.reps // 2))
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
