"""Timings of the Spelke-object segment step on the GPU, in one session:

  * `cwm_segment_step` alone (seed references, votes, component, coverage, selection of 4 + 4 patches) at 224 x 224, P = 8, for S = 8 and S = 64 flow samples,
    in the sample-outermost view of the flow model's output and in the packed [B,2,H,W,S] layout
  * the same inputs through the package's torch composition (`segment_step.segment_step_torch`) on the same GPU
  * one `segment_spelke_object` iteration (ViT-B/8 at synthetic weights, RAFT at random weights, S = 8) against the `predict_counterfactual_videos_and_flows`
    call it is built on, alternated call by call

    python tools/segment_step.py [--batch 1] [--reps 20] [--raft-iters 12] [--mode fast|parity] [--json PATH]

Device events around work that is synchronised before it is read; every shape is warmed up first.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from counterfactualworldmodels_amd import _lib, config as C, segment_step as SS, segmentation, synthetic as S, vmae  # noqa: E402
from counterfactualworldmodels_amd.raft import RAFT, _args  # noqa: E402


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(calls, reps):
    """{name: median / min ms}: the calls take turns, so that all of them see the same clocks and the same neighbours"""
    rounds = {k: [] for k in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            rounds[name].append(once(fn))
    out = {}
    for name, ts in rounds.items():
        ts.sort()
        out[name] = {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "reps": len(ts)}
    return out


def object_flows(B, H, W, Sn, seed):
    """[B,2,H,W,S] on the CPU: an ellipse with a ragged edge moves by (0.75, 1.0) k_s pixels over a background of small noise"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    obj = ((yy - H * 0.45) / (H * 0.3)) ** 2 + ((xx - W * 0.55) / (W * 0.22)) ** 2 < 1 + 0.15 * g.standard_normal((H, W))
    f = 0.05 * g.standard_normal((B, 2, H, W, Sn)).astype(np.float32)
    k = g.integers(0, 5, (B, Sn)).astype(np.float32)
    f[:, 0] += obj[None, :, :, None] * 0.75 * k[:, None, None, :]
    f[:, 1] += obj[None, :, :, None] * 1.0 * k[:, None, None, :]
    return torch.from_numpy(f), obj


def step_alone(B, Sn, reps):
    """us per call of the library step in both layouts and of the torch composition, 20 calls per timing"""
    H = W = 224
    f, obj = object_flows(B, H, W, Sn, Sn)
    seeds = torch.tensor([[int(H * 0.45), int(W * 0.55)]] * B, dtype=torch.int32).cuda()
    layouts = {"view": f.permute(0, 4, 1, 2, 3).contiguous().cuda().permute(0, 2, 3, 4, 1), "packed": f.cuda()}
    kw = dict(min_seed_mag=0.5, abs_thresh=0.5, rel_thresh=0.5, vote_frac=0.5, k_active=4, k_passive=4)
    calls = {"step_" + name: (lambda t=t: [SS.segment_step_device(t, seeds, 8, **kw) for _ in range(20)]) for name, t in layouts.items()}
    calls["torch_composition"] = lambda: SS.segment_step_torch(layouts["view"], seeds, 8, **kw)
    res = {k: SS.segment_step_device(t, seeds, 8, **kw) for k, t in layouts.items()}
    ref = SS.segment_step_torch(layouts["view"], seeds, 8, **kw)
    torch.cuda.synchronize()
    out = {"area": res["view"].stats[:, 1].tolist(), "object_pixels": int(obj.sum()),
           "layouts_equal": all(torch.equal(getattr(res["view"], k), getattr(res["packed"], k)) for k in ("segment", "votes", "picks", "stats")),
           "segment_equals_torch": bool(torch.equal(res["view"].segment, ref.segment))}
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
    out["S8"] = step_alone(B, 8, args.reps)
    out["S64"] = step_alone(B, 64, args.reps)

    cfg = C.CONFIGS["base_8x8patch_2frames_1tube"]
    m = vmae.PretrainVisionTransformer(cfg, mode=args.mode)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 0).items()})
    raft = RAFT(_args(mixed_precision=(args.mode == "fast")))
    raft.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(0).items()})
    G = segmentation.FlowGenerator(predictor=m.cuda().eval(), flow_model=raft.cuda().eval(), imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
    x = torch.from_numpy(S.synthetic_frames(B, cfg, 0)).cuda()
    seeds = torch.tensor([[100, 120]] * B, dtype=torch.int32).cuda()
    Sn = 8
    init = G.segment_step(None, seeds, min_seed_mag=1.0, abs_thresh=1.0, k_active=4, k_passive=4, shape=(B, 224, 224))
    act, pas = init.active.unsqueeze(-1).expand(-1, -1, Sn), init.passive.unsqueeze(-1).expand(-1, -1, Sn)
    calls = {"counterfactuals_and_flows": lambda: G.predict_counterfactual_videos_and_flows(x, act, pas, shifts=SS.directions(Sn), num_samples=Sn, sample_batch_size=None,
                                                                                             fix_passive=True, raft_iters=args.raft_iters),
             "segment_iteration": lambda: G.segment_spelke_object(x, seeds, num_iters=1, num_samples=Sn, raft_iters=args.raft_iters)}
    for fn in calls.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out.update(alternate(calls, max(3, args.reps // 2)))
    out["step_share_of_iteration"] = round(1 - out["counterfactuals_and_flows"]["median_ms"] / out["segment_iteration"]["median_ms"], 4)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
