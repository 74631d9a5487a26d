"""Timings of the object-motion read-out on the GPU, in one session:

  * `cwm_object_motion` alone (two memsets or three, the accumulate and the finalise kernel, and the allocation of its outputs) at 224 x 224 with 4 and 64 live
    slots, batch 1 and 8, bare (labels and flow) and full (with `code` and `other`)
  * a torch composition of the same tables on the same GPU in the same cases, as a user would write it today: `bincount` for the counts and the occluder table,
    one int64 `scatter_add_` per sum, and the fit as batched float64 tensor operations -- its integer tables are compared with the call's
  * `track_scene` on a three-frame movie (two segmented frames, one carried; ViT-B/8 at synthetic weights, RAFT at random weights, S = 8, 8 seeds) with
    `occlusion=True`, with and without `motion=True`, alternated call by call
  * with `--parent-root PATH` (a tree of the parent commit with its built library): the default `track_scene` from that tree and from this one, each in
    processes of its own, alternated, two runs each

    python tools/motion_step.py [--reps 20] [--raft-iters 12] [--mode fast|parity] [--call-only] [--batches 1,8] [--slots 4,64] [--inputs bare,full]
                                [--parent-root PATH] [--json PATH]

Device events around work that is synchronised before it is read; every shape is warmed up first; calls alternate and medians are reported.  Prints one JSON
line.  `--call-only` stops after the call alone (the form to run under a kernel trace); `--default-only --root PATH` is the child of `--parent-root`."""
import argparse
import json
import os
import subprocess
import sys

if "--root" in sys.argv:  # (the child of --parent-root: the package of another tree, the tools of this one)
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--root") + 1]))
    sys.path.append(os.getcwd())
else:
    sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from counterfactualworldmodels_amd import _lib, config as C, segment_merge as SM, segmentation, synthetic as S, vmae  # noqa: E402
from counterfactualworldmodels_amd.raft import RAFT, _args  # noqa: E402
from tools.segment_step import alternate  # noqa: E402


def scene(B, H, W, slots, seed):
    """labels, flow, code, other on the CPU: `slots` rectangles on a grid over a background, each moving by its own (dx, dy) of a few pixels plus small noise,
    the other frame's map the rectangles moved along, the codes 1 on the strip each rectangle runs into"""
    g = np.random.default_rng(seed)
    n = int(np.ceil(np.sqrt(slots)))
    ch, cw = H // n, W // n
    labels, other = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.uint8)
    flow = 0.05 * g.standard_normal((B, 2, H, W)).astype(np.float32)
    code = np.zeros((B, H, W), np.uint8)
    for s in range(slots):
        y0, x0 = (s // n) * ch + ch // 6, (s % n) * cw + cw // 6
        y1, x1 = y0 + 2 * ch // 3, x0 + 2 * cw // 3
        dx, dy = int(g.integers(-3, 4)), int(g.integers(-3, 4))
        labels[:, y0:y1, x0:x1] = s + 1
        other[:, max(y0 + dy, 0):min(y1 + dy, H), max(x0 + dx, 0):min(x1 + dx, W)] = s + 1
        flow[:, 0, y0:y1, x0:x1] += dx
        flow[:, 1, y0:y1, x0:x1] += dy
        code[:, y0:y1, x1 - 2:x1] = 1
    return tuple(torch.from_numpy(a) for a in (labels, flow, code, other))


def torch_motion(labels, flow, code, other, min_affine=16, min_det=1.0):
    """the composition a user writes today, [B,H,W] maps; returns sums [B,65,14] int64, counts [B,65,3], model [B,65,11] float64, occ [B,65,65] or None"""
    B, H, W = labels.shape
    dev = labels.device
    l = labels.long()
    l = torch.where(l > 64, 0, l)
    u, v = flow[:, 0], flow[:, 1]
    xs = torch.arange(W, device=dev).expand(B, H, W)
    ys = torch.arange(H, device=dev)[:, None].expand(B, H, W)
    fx, fy = xs + u, ys + v
    ok = (u.abs() <= 4096) & (v.abs() <= 4096) & (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
    k = torch.where(ok, (code != 0).long() if code is not None else torch.zeros_like(l), 2)
    row = torch.arange(B, device=dev)[:, None, None] * 65
    counts = torch.bincount(((row + l) * 3 + k).reshape(-1), minlength=B * 65 * 3).reshape(B, 65, 3)
    k0 = k == 0
    qu, qv = torch.round(torch.where(k0, u, 0.0) * 256).long(), torch.round(torch.where(k0, v, 0.0) * 256).long()
    terms = [k0.long(), xs, ys, xs * xs, xs * ys, ys * ys, qu, qv, xs * qu, ys * qu, xs * qv, ys * qv, qu * qu, qv * qv]
    index = (row + l).reshape(-1)
    sums = torch.stack([torch.zeros(B * 65, dtype=torch.long, device=dev).scatter_add_(0, index, torch.where(k0, t, 0).reshape(-1)) for t in terms], -1)
    occ = None
    if other is not None:
        k1 = k == 1
        src = torch.where(k1, torch.round(fy).long() * W + torch.round(fx).long(), 0)
        m = other.reshape(B, -1).long().gather(1, src.reshape(B, -1)).reshape(B, H, W)
        m = torch.where(m > 64, 0, m)
        occ = torch.bincount(((row + l) * 65 + m)[k1], minlength=B * 65 * 65).reshape(B, 65, 65)
    S_ = sums.double()
    n = S_[:, 0].clamp(min=1)
    mean = S_[:, [1, 2, 6, 7]] / n[:, None]
    mx, my, mu, mv = mean.unbind(1)
    cxx, cxy, cyy = S_[:, 3] / n - mx * mx, S_[:, 4] / n - mx * my, S_[:, 5] / n - my * my
    cxu, cyu, cxv, cyv = S_[:, 8] / n - mx * mu, S_[:, 9] / n - my * mu, S_[:, 10] / n - mx * mv, S_[:, 11] / n - my * mv
    det = cxx * cyy - cxy * cxy
    affine = (sums[:, 0] >= min_affine) & (det >= min_det)
    A = [torch.where(affine, a / det / 256, 0.0) for a in (cxu * cyy - cyu * cxy, cyu * cxx - cxu * cxy, cxv * cyy - cyv * cxy, cyv * cxx - cxv * cxy)]
    model = torch.stack([affine.double() + 1, mu / 256, mv / 256] + A + [mx, my, (S_[:, 12] / n - mu * mu) / 65536, (S_[:, 13] / n - mv * mv) / 65536], -1)
    return sums.reshape(B, 65, 14), counts, torch.where((sums[:, 0] >= 1)[:, None], model, 0.0).reshape(B, 65, 11), occ


def call_alone(B, slots, full, reps):
    """us per call of the library call (20 calls per timing, outputs allocated by every call) and of the torch composition"""
    from counterfactualworldmodels_amd import object_motion as OM

    H = W = 224
    labels, flow, code, other = (t.cuda() for t in scene(B, H, W, slots, slots + B))
    kw = dict(code=code, other=other) if full else {}
    calls = {"object_motion": lambda: [OM.measure_device(labels, flow, **kw) for _ in range(20)],
             "torch_composition": lambda: torch_motion(labels, flow, kw.get("code"), kw.get("other"))}
    res, ref = OM.measure_device(labels, flow, **kw), torch_motion(labels, flow, kw.get("code"), kw.get("other"))
    torch.cuda.synchronize()
    agree = torch.equal(res.sums[..., :14], ref[0]) and torch.equal(res.counts[..., :3].long(), ref[1]) and (not full or torch.equal(res.occluders.long(), ref[3]))
    # what the call moves: a label byte, u and v (8 bytes per pixel), with `full` a code byte (the occluder gathers are a few per cent of the pixels), and the
    # tables it zeroes, adds into and writes
    tables = B * 65 * (16 * 8 + 4 * 4 + 12 * 8 + (65 * 4 if full else 0))
    out = {"live_slots": int((res.counts.sum(-1) > 0).sum(-1).max()) - 1, "class_counts": res.counts.sum(1)[0, :3].tolist(), "tables_equal_torch": bool(agree),
           "occluder_pixels": int(res.occluders.sum()) // B if full else 0, "bytes_moved": B * H * W * (10 if full else 9) + 2 * tables}
    for name, t in alternate(calls, reps).items():
        per = 1 if name == "torch_composition" else 20
        out[name + "_us"] = {"median": round(t["median_ms"] * 1e3 / per, 2), "min": round(t["min_ms"] * 1e3 / per, 2)}
    return out


def generator(mode, raft_iters):
    cfg = C.CONFIGS["base_8x8patch_2frames_1tube"]
    m = vmae.PretrainVisionTransformer(cfg, mode=mode)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 0).items()})
    raft = RAFT(_args(mixed_precision=(mode == "fast")))
    raft.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(0).items()})
    G = segmentation.FlowGenerator(predictor=m.cuda().eval(), flow_model=raft.cuda().eval(), imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
    pair = torch.from_numpy(S.synthetic_frames(1, cfg, 0)).cuda()
    x = torch.cat([pair, pair[:, :1]], 1)  # three frames: frames 0 and 1 are segmented, frame 2 is carried
    Sn, K = 8, 8
    gen = torch.Generator(device="cuda").manual_seed(0)
    seeds = SM.cell_centres(SM.draw_seed_cells(torch.ones((1, 28 * 28), device="cuda"), torch.ones((1, 28 * 28), dtype=torch.bool, device="cuda"), K, gen), 28, 8)
    kw = dict(num_iters=1, num_samples=Sn, raft_iters=raft_iters, seeds=seeds, num_seeds=K, flow_kwargs=dict(iters=raft_iters))
    return G, x, kw


def movie(calls, reps):
    for fn in calls.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    return alternate(calls, max(3, reps // 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="fast", choices=("fast", "parity"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--raft-iters", type=int, default=12)
    ap.add_argument("--call-only", action="store_true")
    ap.add_argument("--default-only", action="store_true", help="only the default track_scene (the child of --parent-root)")
    ap.add_argument("--root", default=None, help="with --default-only: the tree whose package is measured")
    ap.add_argument("--parent-root", default=None, help="a tree of the parent commit with its built library: the default track_scene of both, alternated")
    ap.add_argument("--batches", default="1,8", help="batch sizes of the call alone")
    ap.add_argument("--slots", default="4,64", help="live slots of the call alone")
    ap.add_argument("--inputs", default="bare,full", help="of the call alone: bare (labels and flow), full (with code and other)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "mode": args.mode, "raft_iters": args.raft_iters}
    if args.default_only:
        G, x, kw = generator(args.mode, args.raft_iters)
        out["package"] = os.path.dirname(os.path.abspath(segmentation.__file__))
        out["library_source_hash"] = _lib.get_lib().cwm_source_hash().decode()
        out.update(movie({"track_scene_3_frames": lambda: G.track_scene(x, **kw)}, args.reps))
    else:
        for B in (int(v) for v in args.batches.split(",")):
            for slots in (int(v) for v in args.slots.split(",")):
                for full in (v == "full" for v in args.inputs.split(",")):
                    out["B%d_slots%d_%s" % (B, slots, "full" if full else "bare")] = call_alone(B, slots, full, args.reps)
        if not args.call_only:
            G, x, kw = generator(args.mode, args.raft_iters)
            out.update(movie({"track_scene_3_frames": lambda: G.track_scene(x, **kw),
                              "track_scene_3_frames_occlusion": lambda: G.track_scene(x, occlusion=True, **kw),
                              "track_scene_3_frames_occlusion_motion": lambda: G.track_scene(x, occlusion=True, motion=True, **kw)}, args.reps))
            out["motion_ms"] = round(out["track_scene_3_frames_occlusion_motion"]["median_ms"] - out["track_scene_3_frames_occlusion"]["median_ms"], 4)
        if args.parent_root:
            runs = []
            for name, root in (("parent", args.parent_root), ("this", os.getcwd())) * 2:  # (processes of their own, one at a time, taking turns)
                cmd = [sys.executable, os.path.abspath(__file__), "--default-only", "--root", root, "--mode", args.mode, "--reps", str(args.reps),
                       "--raft-iters", str(args.raft_iters)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError("the %s tree failed:\n%s" % (name, r.stderr[-2000:]))
                got = json.loads(r.stdout.strip().splitlines()[-1])
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
