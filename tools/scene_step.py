"""Timings of the scene-segmentation merge on the GPU, in one session:

  * `cwm_segment_merge` alone (pack, intersections, suppression, paint) at 224 x 224, P = 8, for K = 8 and K = 64 candidates
  * the same inputs through the package's torch composition (`segment_merge.segment_merge_torch`) on the same GPU
  * one `segment_scene` round (ViT-B/8 at synthetic weights, RAFT at random weights, S = 8, 8 seeds) against the `segment_spelke_object` call on the same 8 rows
    that it is built on, alternated call by call

    python tools/scene_step.py [--batch 1] [--reps 20] [--raft-iters 12] [--mode fast|parity] [--json PATH]

Device events around work that is synchronised before it is read; every shape is warmed up first; calls alternate and medians are reported.  Prints one JSON
line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from counterfactualworldmodels_amd import _lib, config as C, segment_merge as SM, segmentation, synthetic as S, vmae  # noqa: E402
from counterfactualworldmodels_amd.raft import RAFT, _args  # noqa: E402
from tools.segment_step import alternate  # noqa: E402


def candidates(B, K, H, W, seed):
    """[B,K,H,W] bool on the CPU: ellipses around K // 2 centres, each centre twice with a slightly different size (a duplicate to absorb), and their scores"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    segs = np.zeros((B, K, H, W), bool)
    for b in range(B):
        for k in range(K):
            if k % 2 == 0:
                cy, cx, ry, rx = g.uniform(0.1, 0.9) * H, g.uniform(0.1, 0.9) * W, g.uniform(0.05, 0.2) * H, g.uniform(0.05, 0.2) * W
            segs[b, k] = ((yy - cy) / (ry + k % 2)) ** 2 + ((xx - cx) / (rx + k % 2)) ** 2 < 1
    return torch.from_numpy(segs), torch.from_numpy(g.random((B, K), dtype=np.float32))


def merge_alone(B, K, reps):
    """us per call of the library merge (20 calls per timing) and of the torch composition"""
    H = W = 224
    segs, scores = candidates(B, K, H, W, K)
    segs, scores = segs.cuda(), scores.cuda()
    kw = dict(min_area=64, max_area=H * W // 2, want_inter=True)
    calls = {"merge": lambda: [SM.segment_merge_device(segs, scores, 8, **kw) for _ in range(20)], "torch_composition": lambda: SM.segment_merge_torch(segs, scores, 8, **kw)}
    res, ref = SM.segment_merge_device(segs, scores, 8, **kw), SM.segment_merge_torch(segs, scores, 8, **kw)
    torch.cuda.synchronize()
    out = {"stats": res.stats.tolist(), "input_bytes": segs.numel(),
           "equals_torch": all(torch.equal(getattr(res, k), getattr(ref, k)) for k in ("labels", "owner", "area", "label_area", "inter", "cover", "stats"))}
    for name, t in alternate(calls, reps).items():
        per = 1 if name == "torch_composition" else 20
        out[name + "_us"] = {"median": round(t["median_ms"] * 1e3 / per, 2), "min": round(t["min_ms"] * 1e3 / per, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--mode", default="fast", choices=("fast", "parity"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--raft-iters", type=int, default=12)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    B = args.batch
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "mode": args.mode, "raft_iters": args.raft_iters}
    out["K8"] = merge_alone(B, 8, args.reps)
    out["K64"] = merge_alone(B, 64, args.reps)

    cfg = C.CONFIGS["base_8x8patch_2frames_1tube"]
    m = vmae.PretrainVisionTransformer(cfg, mode=args.mode)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 0).items()})
    raft = RAFT(_args(mixed_precision=(args.mode == "fast")))
    raft.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(0).items()})
    G = segmentation.FlowGenerator(predictor=m.cuda().eval(), flow_model=raft.cuda().eval(), imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
    x = torch.from_numpy(S.synthetic_frames(B, cfg, 0)).cuda()
    Sn, K = 8, 8
    gen = torch.Generator(device="cuda").manual_seed(0)
    seeds = SM.cell_centres(SM.draw_seed_cells(torch.ones((B, 28 * 28), device="cuda"), torch.ones((B, 28 * 28), dtype=torch.bool, device="cuda"), K, gen), 28, 8)
    rows, flat = x.repeat_interleave(K, 0), seeds.reshape(B * K, 2)
    kw = dict(num_iters=1, num_samples=Sn, raft_iters=args.raft_iters)
    calls = {"spelke_object_rows": lambda: G.segment_spelke_object(rows, flat, **kw), "scene_round": lambda: G.segment_scene(x, seeds=seeds, num_seeds=K, **kw)}
    for fn in calls.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out.update(alternate(calls, max(3, args.reps // 2)))
    out["merge_share_of_round"] = round(1 - out["spelke_object_rows"]["median_ms"] / out["scene_round"]["median_ms"], 4)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
