"""Timings of the point tracker on the GPU, in one session:

  * `cwm_point_track` alone (one kernel launch, and the allocation of its four outputs) at 224 x 224, T = 8, for K = 64, 784 (every 8th pixel) and 50176 (every
    pixel) points at batch 1 and 8, with the forward flows only, with the backward flows as well, and with all inputs (slot maps and models)
  * a torch composition of the flows-only variant on the same GPU in the same cases, as a user would write it today: a Python loop over the pairs with one
    `grid_sample` (bilinear, align_corners=True) of the forward flow per step -- its positions are compared with the call's
  * `track_scene` on a three-frame movie (two segmented frames, one carried; ViT-B/8 at synthetic weights, RAFT at random weights, S = 8, 8 seeds) with
    `occlusion=True, motion=True`, with and without `points` (784 of them), alternated call by call
  * with `--parent-root PATH` (a tree of the parent commit with its built library): the default `track_scene` from that tree and from this one, each in
    processes of its own, alternated, two runs each (the child is `tools/motion_step.py --default-only`, which both trees can run)

    python tools/point_step.py [--reps 20] [--raft-iters 12] [--mode fast|parity] [--call-only] [--batches 1,8] [--points 64,784,50176]
                               [--inputs flows,bwd,all] [--parent-root PATH] [--json PATH]

Device events around work that is synchronised before it is read; every shape is warmed up first; calls alternate and medians are reported.  The inputs are
warm: a 224 x 224 plane is 200 KB and the calls repeat on the same buffers.  Prints one JSON line.  `--call-only` stops after the call alone (the form to run
under a kernel trace)."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from counterfactualworldmodels_amd import _lib, point_track as PT  # noqa: E402
from tools.motion_step import generator, movie  # noqa: E402
from tools.segment_step import alternate  # noqa: E402

H = W = 224
T = 8


def scene(B, seed):
    """fwd, bwd, labels, model on the CPU: 16 rectangles on a grid over a background, each moving by its own (dx, dy) of up to 3 px per frame plus small noise
    in the flows; a static bar across the middle is painted over them, so that points pass behind it; the models are the rectangles' translations"""
    g = np.random.default_rng(seed)
    n, ch, cw = 4, H // 4, W // 4
    labels = np.zeros((B, T, H, W), np.uint8)
    fwd = 0.05 * g.standard_normal((B, T - 1, 2, H, W)).astype(np.float32)
    bwd = 0.05 * g.standard_normal((B, T - 1, 2, H, W)).astype(np.float32)
    model = np.zeros((B, T, 65, 12))
    model[:, :, 0, 0] = 1
    for s in range(n * n):
        y0, x0 = (s // n) * ch + ch // 6, (s % n) * cw + cw // 6
        dx, dy = int(g.integers(-3, 4)), int(g.integers(-3, 4))
        for t in range(T):
            ya, xa = np.clip([y0 + dy * t, y0 + dy * t + 2 * ch // 3], 0, H), np.clip([x0 + dx * t, x0 + dx * t + 2 * cw // 3], 0, W)
            labels[:, t, ya[0]:ya[1], xa[0]:xa[1]] = s + 1
        model[:, :, s + 1, :3] = (1, dx, dy)
    labels[:, :, :, W // 2 - 6:W // 2 + 6] = 17  # the bar
    for s in range(n * n):
        dx, dy = model[0, 0, s + 1, 1:3]
        for t in range(T - 1):
            on, on_next = labels[:, t] == s + 1, labels[:, t + 1] == s + 1
            fwd[:, t, 0][on] += dx
            fwd[:, t, 1][on] += dy
            bwd[:, t, 0][on_next] -= dx
            bwd[:, t, 1][on_next] -= dy
    return tuple(torch.from_numpy(a) for a in (fwd, bwd, labels, model))


def torch_track(fwd, points):
    """the loop a user writes today for the flows-only variant: one grid_sample per pair, no occlusion reasoning; returns xy [B,T,K,2]"""
    B = fwd.shape[0]
    p = points.clone()
    scale = torch.tensor([2.0 / (W - 1), 2.0 / (H - 1)], device=fwd.device)
    out = [p]
    for t in range(fwd.shape[1]):
        grid = (p * scale - 1.0).view(B, 1, -1, 2)
        a = torch.nn.functional.grid_sample(fwd[:, t], grid, mode="bilinear", padding_mode="border", align_corners=True)  # [B,2,1,K]
        p = p + a[:, :, 0].permute(0, 2, 1)
        out.append(p)
    return torch.stack(out, 1)


def call_alone(B, K, inputs, reps):
    """us per call of the library call (20 calls per timing, outputs allocated by every call) and, for the flows-only variant, of the torch composition"""
    fwd, bwd, labels, model = (t.cuda() for t in scene(B, K + B))
    stride = {64: 28, 784: 8, 50176: 1}.get(K)
    points = PT.grid_points(H, W, stride, B=B, device="cuda") if stride else torch.rand((B, K, 2), device="cuda") * (W - 1)
    assert points.shape[1] == K
    kw = {"flows": {}, "bwd": dict(bwd=bwd), "all": dict(bwd=bwd, labels=labels, model=model)}[inputs]
    calls = {"point_track": lambda: [PT.track_device(fwd, points, **kw) for _ in range(20)]}
    res = PT.track_device(fwd, points, **kw)
    torch.cuda.synchronize()
    out = {"states": torch.bincount(res.state.reshape(-1).long(), minlength=4)[:4].tolist(),
           # what a point moves per frame: 8 or 16 taps of 4 bytes, a label byte, 10 bytes written; the model rows only when it coasts
           "bytes_moved": B * K * (T * 10 + (T - 1) * (32 * (2 if "bwd" in kw else 1) + (1 if "labels" in kw else 0)))}
    if inputs == "flows":
        calls["torch_composition"] = lambda: torch_track(fwd, points)
        ref = torch_track(fwd, points)
        both = (res.state == 0) & torch.isfinite(ref).all(-1)
        out["max_abs_difference_to_torch_px"] = float((res.xy - ref)[both].abs().max())
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
    ap.add_argument("--parent-root", default=None, help="a tree of the parent commit with its built library: the default track_scene of both, alternated")
    ap.add_argument("--batches", default="1,8", help="batch sizes of the call alone")
    ap.add_argument("--points", default="64,784,50176", help="points per row of the call alone")
    ap.add_argument("--inputs", default="flows,bwd,all", help="of the call alone: flows (forward flows only), bwd (both flows), all (with slot maps and models)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "mode": args.mode, "raft_iters": args.raft_iters, "frames": T, "plane": [H, W]}
    for B in (int(v) for v in args.batches.split(",")):
        for K in (int(v) for v in args.points.split(",")):
            for inputs in args.inputs.split(","):
                out["B%d_K%d_%s" % (B, K, inputs)] = call_alone(B, K, inputs, args.reps)
                print("B%d_K%d_%s" % (B, K, inputs), out["B%d_K%d_%s" % (B, K, inputs)], file=sys.stderr, flush=True)
    if not args.call_only:
        G, x, kw = generator(args.mode, args.raft_iters)
        pts = PT.grid_points(H, W, 8, device="cuda")
        out.update(movie({"track_scene_3_frames_occlusion_motion": lambda: G.track_scene(x, occlusion=True, motion=True, **kw),
                          "track_scene_3_frames_occlusion_motion_points": lambda: G.track_scene(x, occlusion=True, motion=True, points=pts, **kw)}, args.reps))
        out["points_ms"] = round(out["track_scene_3_frames_occlusion_motion_points"]["median_ms"] - out["track_scene_3_frames_occlusion_motion"]["median_ms"], 4)
    if args.parent_root:
        runs = []
        child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "motion_step.py")
        for name, root in (("parent", args.parent_root), ("this", os.getcwd())) * 2:  # (processes of their own, one at a time, taking turns)
            cmd = [sys.executable, child, "--default-only", "--root", root, "--mode", args.mode, "--reps", str(args.reps), "--raft-iters", str(args.raft_iters)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError("the %s tree failed:\n%s" % (name, r.stderr[-2000:]))
            got = json.loads(r.stdout.strip().splitlines()[-1])
            print(name, got["track_scene_3_frames"], file=sys.stderr, flush=True)
            runs.append({"tree": name, "package": got["package"], "library_source_hash": got["library_source_hash"], **got["track_scene_3_frames"]})
        out["default_track_scene_parent_and_this"] = runs
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
