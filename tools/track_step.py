"""Timings of the track link step on the GPU, in one session:

  * `cwm_segment_track` alone (count, link, paint, finish, and the allocation of its outputs) at 224 x 224, batch 1 and 8, with few (4) and many (64) live
    tracks and as many labels
  * the same inputs through the package's torch composition (`segment_track.track_step_torch` on device tensors) on the same GPU
  * `track_scene` on a three-frame movie (two segmented frames, one carried; ViT-B/8 at synthetic weights, RAFT at random weights, S = 8, 8 seeds) against the
    `segment_scene` round and the `predict_flow(backward=True)` call it is built on, alternated call by call

    python tools/track_step.py [--reps 20] [--raft-iters 12] [--mode fast|parity] [--link-only] [--batches 1,8] [--tracks 4,64] [--json PATH]

Device events around work that is synchronised before it is read; every shape is warmed up first; calls alternate and medians are reported.  Prints one JSON
line.  `--link-only` stops after the link step (the form to run under a kernel trace)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from counterfactualworldmodels_amd import _lib, config as C, segment_merge as SM, segment_track as ST, segmentation, synthetic as S, vmae  # noqa: E402
from counterfactualworldmodels_amd.raft import RAFT, _args  # noqa: E402
from tools.segment_step import alternate  # noqa: E402

OUTPUTS = ("area", "bbox", "moments", "slot_of_cur", "linked_cur", "stats")


def scene(B, n, H, W, seed):
    """(state, cur [B,H,W], flow [B,2,H,W]) on the CPU: n ellipses as live tracks, the labels are the same ellipses moved by about a pixel and renumbered, the flow
    is a smooth field of up to two pixels"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    prev, cur = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.uint8)
    side = int(np.ceil(np.sqrt(n)))
    for b in range(B):
        for k in range(n):
            cy, cx = (k // side + 0.5) * H / side, (k % side + 0.5) * W / side
            ry, rx = g.uniform(0.25, 0.45) * H / side, g.uniform(0.25, 0.45) * W / side
            prev[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1] = k + 1
            cur[b][((yy - cy - 1) / ry) ** 2 + ((xx - cx - 1) / rx) ** 2 < 1] = n - k
    flow = np.stack([1.0 + np.sin(yy / 17.0) * np.ones((B, 1, 1)), 1.0 + np.cos(xx / 23.0) * np.ones((B, 1, 1))], 1).astype(np.float32)
    state = ST.TrackState.empty(B, H, W)
    state.labels = torch.from_numpy(prev)
    state.track_id[:, :n] = torch.arange(1, n + 1, dtype=torch.int32)
    state.next_id[:] = n + 1
    return state, torch.from_numpy(cur), torch.from_numpy(flow)


def link_alone(B, n, reps):
    """us per call of the library step (20 calls per timing, outputs allocated by every call) and of the torch composition"""
    H = W = 224
    state, cur, flow = scene(B, n, H, W, n)
    state = ST.TrackState(*(t.cuda() for t in (state.labels, state.track_id, state.age, state.next_id)))
    cur, flow = cur.cuda(), flow.cuda()
    kw = dict(want_table=True, want_warped=True)
    calls = {"track": lambda: [ST.track_step_device(state, cur, flow, **kw) for _ in range(20)], "torch_composition": lambda: ST.track_step_torch(state, cur, flow, **kw)}
    res, ref = ST.track_step_device(state, cur, flow, **kw), ST.track_step_torch(state, cur, flow, **kw)
    torch.cuda.synchronize()
    same = all(torch.equal(getattr(res, k), getattr(ref, k)) for k in OUTPUTS + ("table", "warped"))
    same = same and all(torch.equal(getattr(res.state, k), getattr(ref.state, k)) for k in ("labels", "track_id", "age", "next_id"))
    # what the count pass reads and writes: cur, u, v, one gathered byte and the warped byte per pixel; the paint pass: cur, warped, out and the warped output
    out = {"stats": res.stats.tolist(), "equals_torch": same, "count_bytes": B * H * W * (1 + 8 + 1 + 1), "paint_bytes": B * H * W * 4}
    for name, t in alternate(calls, reps).items():
        per = 1 if name == "torch_composition" else 20
        out[name + "_us"] = {"median": round(t["median_ms"] * 1e3 / per, 2), "min": round(t["min_ms"] * 1e3 / per, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="fast", choices=("fast", "parity"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--raft-iters", type=int, default=12)
    ap.add_argument("--link-only", action="store_true")
    ap.add_argument("--batches", default="1,8", help="batch sizes of the link step alone")
    ap.add_argument("--tracks", default="4,64", help="live tracks (and labels) of the link step alone")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "mode": args.mode, "raft_iters": args.raft_iters}
    for B in (int(v) for v in args.batches.split(",")):
        for n in (int(v) for v in args.tracks.split(",")):
            out["B%d_tracks%d" % (B, n)] = link_alone(B, n, args.reps)

    if not args.link_only:
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
        kw = dict(num_iters=1, num_samples=Sn, raft_iters=args.raft_iters)
        calls = {"scene_round": lambda: G.segment_scene(x[:, :2], seeds=seeds, num_seeds=K, **kw),
                 "predict_flow_backward_3_frames": lambda: G.predict_flow(x, backward=True, iters=args.raft_iters),
                 "track_scene_3_frames": lambda: G.track_scene(x, seeds=seeds, num_seeds=K, flow_kwargs=dict(iters=args.raft_iters), **kw)}
        for fn in calls.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        out.update(alternate(calls, max(3, args.reps // 2)))
        # two segmented frames and one backward flow call: what is left is the three link steps and the loop around them
        out["track_scene_less_its_parts_ms"] = round(out["track_scene_3_frames"]["median_ms"] - 2 * out["scene_round"]["median_ms"]
                                                     - out["predict_flow_backward_3_frames"]["median_ms"], 4)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
