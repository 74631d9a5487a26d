"""Timings of the forward-backward consistency check on the GPU, in one session:

  * `cwm_flow_consistency` alone (one kernel behind a memset of the stats, and the allocation of its outputs) at 224 x 224, batch 1 and 8, one direction and
    both, codes only and all outputs (res, masked, cells at P = 8)
  * a torch composition of the same check on the same GPU in the same cases: `grid_sample` (bilinear, align_corners, border padding) of the other flow at the
    targets plus the elementwise threshold test, as a user would write it today -- not bit-equal to the call, so only the codes' agreement is reported
  * `track_scene` on a three-frame movie (two segmented frames, one carried; ViT-B/8 at synthetic weights, RAFT at random weights, S = 8, 8 seeds) with and
    without `occlusion`, against the `predict_flow` call the option adds, alternated call by call

    python tools/consistency_step.py [--reps 20] [--raft-iters 12] [--mode fast|parity] [--call-only] [--batches 1,8] [--directions one,both]
                                     [--outputs codes,all] [--json PATH]

Device events around work that is synchronised before it is read; every shape is warmed up first; calls alternate and medians are reported.  Prints one JSON
line.  `--call-only` stops after the call alone (the form to run under a kernel trace)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from counterfactualworldmodels_amd import _lib, config as C, flow_consistency as FC, segment_merge as SM, segmentation, synthetic as S, vmae  # noqa: E402
from counterfactualworldmodels_amd.raft import RAFT, _args  # noqa: E402
from tools.segment_step import alternate  # noqa: E402


def flows(B, H, W, seed):
    """(a, o) [B,2,H,W] on the CPU: an ellipse moves by (4, 2.5) px over a background of small noise; o is the negative of a moved along, and the strip the ellipse
    uncovers keeps the background's flow: consistent nearly everywhere, occluded along one edge"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    obj = lambda dy, dx: ((yy - dy - H * 0.45) / (H * 0.3)) ** 2 + ((xx - dx - W * 0.55) / (W * 0.22)) ** 2 < 1  # noqa: E731
    a = 0.05 * g.standard_normal((B, 2, H, W)).astype(np.float32)
    o = 0.05 * g.standard_normal((B, 2, H, W)).astype(np.float32)
    a[:, 0] += obj(0, 0) * 4.0
    a[:, 1] += obj(0, 0) * 2.5
    o[:, 0] -= obj(2.5, 4.0) * 4.0
    o[:, 1] -= obj(2.5, 4.0) * 2.5
    return torch.from_numpy(a), torch.from_numpy(o)


def torch_check(a, o, alpha, beta, both, full, P):
    """the composition a user writes today: grid_sample and elementwise launches; code uint8 [D,B,H,W] and, with full, res, masked and cells"""
    outs = []
    for x, y in ((a, o), (o, a))[:2 if both else 1]:
        B, _, H, W = x.shape
        ys, xs = torch.meshgrid(torch.arange(H, device=x.device, dtype=x.dtype), torch.arange(W, device=x.device, dtype=x.dtype), indexing="ij")
        fx, fy = xs + x[:, 0], ys + x[:, 1]
        inside = (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
        grid = torch.stack([fx * (2.0 / (W - 1)) - 1, fy * (2.0 / (H - 1)) - 1], -1)
        s = F.grid_sample(y, grid.nan_to_num(0.0), mode="bilinear", padding_mode="border", align_corners=True)
        res = ((x + s) ** 2).sum(1)
        thr = alpha * ((x ** 2).sum(1) + (s ** 2).sum(1)) + beta
        code = torch.where(inside, (~(res <= thr)).to(torch.uint8), torch.full_like(res, 2, dtype=torch.uint8))
        if full:
            masked = torch.where((code == 0)[:, None], x, torch.full_like(x, float("nan")))
            cells = F.avg_pool2d((code != 0).float()[:, None], P)[:, 0]
            outs.append((code, torch.where(inside & (res == res), res, torch.full_like(res, float("inf"))), masked, cells))
        else:
            outs.append((code,))
    return [torch.stack(t) for t in zip(*outs)]


def call_alone(B, both, full, reps):
    """us per call of the library call (20 calls per timing, outputs allocated by every call) and of the torch composition"""
    H = W = 224
    P = 8
    a, o = (t.cuda() for t in flows(B, H, W, B))
    kw = dict(both=both, P=P, want_res=full, want_masked=full, want_cells=full)
    calls = {"consistency": lambda: [FC.check_device(a, o, **kw) for _ in range(20)], "torch_composition": lambda: torch_check(a, o, 0.01, 0.5, both, full, P)}
    res, ref = FC.check_device(a, o, **kw), torch_check(a, o, 0.01, 0.5, both, full, P)
    torch.cuda.synchronize()
    code = res.code if both else res.code[None]
    D = 2 if both else 1
    # what the call moves: u and v of the checked flow (8 bytes per pixel), the taps of the other flow (its two planes, 8 bytes per pixel when every line is
    # fetched once), a code byte; with all outputs res (4), the two masked planes (8) and the cells
    moved = D * B * H * W * (8 + 8 + 1 + (12 if full else 0)) + (D * B * (H // P) * (W // P) * 4 if full else 0) + D * B * 16
    out = {"stats": res.stats.tolist(), "codes_differing_from_torch": int((code != ref[0]).sum()), "bytes_moved": moved}
    for name, t in alternate(calls, reps).items():
        per = 1 if name == "torch_composition" else 20
        out[name + "_us"] = {"median": round(t["median_ms"] * 1e3 / per, 2), "min": round(t["min_ms"] * 1e3 / per, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="fast", choices=("fast", "parity"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--raft-iters", type=int, default=12)
    ap.add_argument("--call-only", action="store_true")
    ap.add_argument("--batches", default="1,8", help="batch sizes of the call alone")
    ap.add_argument("--directions", default="one,both", help="of the call alone: one, both")
    ap.add_argument("--outputs", default="codes,all", help="of the call alone: codes, all")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "mode": args.mode, "raft_iters": args.raft_iters}
    for B in (int(v) for v in args.batches.split(",")):
        for both in (v == "both" for v in args.directions.split(",")):
            for full in (v == "all" for v in args.outputs.split(",")):
                out["B%d_%s_%s" % (B, "both" if both else "one", "all" if full else "codes")] = call_alone(B, both, full, args.reps)

    if not args.call_only:
        cfg = C.CONFIGS["base_8x8patch_2frames_1tube"]
        m = vmae.PretrainVisionTransformer(cfg, mode=args.mode)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 0).items()})
        raft = RAFT(_args(mixed_precision=(args.mode == "fast")))
        raft.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(0).items()})
        G = segmentation.FlowGenerator(predictor=m.cuda().eval(), flow_model=raft.cuda().eval(), imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
        pair = torch.from_numpy(S.synthetic_frames(1, cfg, 0)).cuda()
        x = torch.cat([pair, pair[:, :1]], 1)  # three frames: frames 0 and 1 are segmented, frame 2 is carried
        Sn, K = 8, 8
        gen = torch.Generator(device="cuda").manual_seed(0)
        seeds = SM.cell_centres(SM.draw_seed_cells(torch.ones((1, 28 * 28), device="cuda"), torch.ones((1, 28 * 28), dtype=torch.bool, device="cuda"), K, gen), 28, 8)
        kw = dict(num_iters=1, num_samples=Sn, raft_iters=args.raft_iters, seeds=seeds, num_seeds=K, flow_kwargs=dict(iters=args.raft_iters))
        calls = {"scene_round": lambda: G.segment_scene(x[:, :2], seeds=seeds, num_seeds=K, num_iters=1, num_samples=Sn, raft_iters=args.raft_iters),
                 "predict_flow_forward_3_frames": lambda: G.predict_flow(x, iters=args.raft_iters),
                 "track_scene_3_frames": lambda: G.track_scene(x, **kw),
                 "track_scene_3_frames_occlusion": lambda: G.track_scene(x, occlusion=True, **kw),
                 "predict_flow_and_occlusion_3_frames": lambda: G.predict_flow_and_occlusion(x, iters=args.raft_iters)}
        for fn in calls.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        out.update(alternate(calls, max(3, args.reps // 2)))
        # the option adds one forward flow call; what is left is the consistency call, the concatenations around it and the loop's changes
        out["occlusion_less_its_flow_call_ms"] = round(out["track_scene_3_frames_occlusion"]["median_ms"] - out["track_scene_3_frames"]["median_ms"]
                                                       - out["predict_flow_forward_3_frames"]["median_ms"], 4)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
