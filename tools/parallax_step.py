"""Timings of the parallax read-out on the GPU, in one session, at 224 x 224 with patches of 8:

  * `cwm_parallax` alone (its memsets, the reference, pixel and finalise kernels, and the allocation of its outputs) at S = 8 and 64 samples, batch 1 and 8,
    in the variants `full` (labels, no dirs: all three kernels, every output), `dirs` (labels and dirs: no reference kernel), `bare` (no labels, no dirs, par
    and cnt only), on the sample-outer view of the flow model's output and on a packed [R,2,H,W,S] tensor
  * a torch composition of the same outputs on the same GPU, as a user would write it today -- `sort` along S, `gather` at the order statistics, `scatter_add_`
    for the histogram --, whose parallax map and histogram are compared with the call's
  * one `FlowGenerator.parallax` call (ViT-B/8 at synthetic weights, RAFT at random weights, S = 8, nine anchors) against the
    `predict_counterfactual_videos_and_flows` call it is built on, alternated: what the anchors, the read-out and the depth order add to the call they follow
  * with `--parent-root PATH` (a tree of the parent commit with its built library): the default `track_scene` from that tree and from this one, each in
    processes of its own, alternated, two runs each (the child is `tools/motion_step.py --default-only`, which both trees can run)

    python tools/parallax_step.py [--reps 20] [--raft-iters 12] [--mode fast|parity] [--call-only] [--batches 1,8] [--samples 8,64]
                                  [--variants full,dirs,bare] [--parent-root PATH] [--json PATH]

Device events around work that is synchronised before it is read; every shape is warmed up first; calls alternate and medians are reported.  The inputs are
warm: the calls repeat on the same buffers.  Prints one JSON line.  `--call-only` stops after the call alone (the form to run under a kernel trace)."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from counterfactualworldmodels_amd import _lib, parallax as PX, segment_step as SS, segmentation  # noqa: E402
from tools.segment_step import alternate  # noqa: E402

H = W = 224
P = 8


def grid_labels(B, slots=8):
    """[B,H,W] uint8 on the device: `slots` rectangles on a grid over a background"""
    n = int(np.ceil(np.sqrt(slots)))
    ch, cw = H // n, W // n
    labels = np.zeros((B, H, W), np.uint8)
    for s in range(slots):
        y0, x0 = (s // n) * ch + ch // 6, (s % n) * cw + cw // 6
        labels[:, y0:y0 + 2 * ch // 3, x0:x0 + 2 * cw // 3] = s + 1
    return torch.from_numpy(labels).cuda()


def pans(labels, Sn, seed):
    """the flow model's output [(b s),1,2,H,W] for Sn pans: the background moves by the sample's shift, slot l by (1 + l / 4) times it, plus small noise"""
    B = labels.shape[0]
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = 0.05 * torch.randn((B, Sn, 2, H, W), generator=g, device="cuda")
    d = torch.tensor(SS.directions(Sn), dtype=torch.float32, device="cuda") * P  # (dy, dx) in pixels
    gain = 1.0 + labels.float() / 4.0  # [B,H,W]
    out[:, :, 0] += d[None, :, 1, None, None] * gain[:, None]
    out[:, :, 1] += d[None, :, 0, None, None] * gain[:, None]
    return out.reshape(B * Sn, 1, 2, H, W)


def torch_parallax(flows, labels, dirs, min_samples):
    """the composition a user writes today: flows [B,2,H,W,S] view, labels [B,H,W] or None, dirs [S,2] or None; returns (par [B,H,W] float32, hist or None)"""
    B, _, _, _, Sn = flows.shape
    dev = flows.device
    u, v = flows[:, 0], flows[:, 1]
    ok = (u.abs() <= 4096) & (v.abs() <= 4096)
    qu, qv = torch.round(torch.where(ok, u, 0.0) * 256).long(), torch.round(torch.where(ok, v, 0.0) * 256).long()
    if dirs is not None:
        mu, mv = (256 * dirs[:, 1].long()).double()[None].expand(B, Sn), (256 * dirs[:, 0].long()).double()[None].expand(B, Sn)
        N = torch.full((B, Sn), H * W, device=dev)
    else:
        member = ok & (labels == 0)[..., None] if labels is not None else ok
        N = member.sum((1, 2))
        mu = torch.where(member, qu, 0).sum((1, 2)).double() / N.clamp(min=1).double()
        mv = torch.where(member, qv, 0).sum((1, 2)).double() / N.clamp(min=1).double()
    den = mu * mu + mv * mv
    live = (N >= 1) & (den >= 64.0 * 64.0)
    ok = ok & live[:, None, None]
    p = (qu.double() * mu[:, None, None] + qv.double() * mv[:, None, None]) / torch.where(live, den, 1.0)[:, None, None]
    n = ok.sum(-1)
    good = n >= min_samples
    ordered = torch.sort(torch.where(ok, p, float("inf")), dim=-1, stable=True).values
    med = torch.where(good, ordered.gather(-1, ((n - 1).clamp(min=0) // 2)[..., None])[..., 0], 0.0)
    par = torch.where(good, med.float(), float("nan"))
    if labels is None:
        return par, None
    l = labels.long()
    bins = (torch.floor(med * 32.0) + 128.0).clamp(0.0, 255.0).long()
    index = ((torch.arange(B, device=dev)[:, None, None] * 65 + l) * 256 + bins).reshape(-1)
    return par, torch.zeros(B * 65 * 256, dtype=torch.long, device=dev).scatter_add_(0, index, good.long().reshape(-1)).reshape(B, 65, 256)


def call_alone(B, Sn, variant, reps):
    """us per call of the library call on both layouts (10 calls per timing, outputs allocated by every call) and of the torch composition"""
    labels = grid_labels(B)
    outer = pans(labels, Sn, B + Sn)
    view = segmentation.FlowGenerator.batch_to_samples(outer, B=B)  # [B,2,H,W,S], sample-outer
    packed = view.contiguous()
    dirs = torch.tensor([(dy * P, dx * P) for dy, dx in SS.directions(Sn)], dtype=torch.int32, device="cuda")
    kw = {"full": dict(labels=labels, ref_slot=0), "dirs": dict(labels=labels, dirs=dirs), "bare": dict(want_spread=False, want_off=False)}[variant]
    per = 10
    calls = {"sample_outer": lambda: [PX.measure_device(view, **kw) for _ in range(per)],
             "packed": lambda: [PX.measure_device(packed, **kw) for _ in range(per)],
             "torch_composition": lambda: torch_parallax(view, kw.get("labels"), kw.get("dirs"), (Sn + 1) // 2)}
    a, b = PX.measure_device(view, **kw), PX.measure_device(packed, **kw)
    ref_par, ref_hist = torch_parallax(view, kw.get("labels"), kw.get("dirs"), (Sn + 1) // 2)
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    # what the call moves: u and v of every (row, sample, pixel) -- twice where the reference kernel runs, and once more for `off` --, the maps it writes and
    # the tables it zeroes, adds into and reads
    reads = 1 + (0 if "dirs" in kw else 1) + (0 if variant == "bare" else 1)
    tables = B * (65 * 256 * 4 + 65 * 8 * 4 + Sn * 32) if variant != "bare" else B * Sn * 32
    out = {"rows": B, "samples": Sn, "variant": variant, "layouts_equal": bool(torch.equal(bits(a.par), bits(b.par))),
           "par_equal_torch": bool(torch.equal(bits(a.par), bits(ref_par))), "flow_bytes": B * Sn * H * W * 8,
           "bytes_moved": reads * B * Sn * H * W * 8 + B * H * W * (5 if variant == "bare" else 14) + 2 * tables}
    if ref_hist is not None:
        out["hist_equal_torch"] = bool(torch.equal(a.hist.long(), ref_hist))
        out["median_bins"] = a.slot_tab[0, :3, 2].tolist()
    for name, t in alternate(calls, reps).items():
        n = 1 if name == "torch_composition" else per
        out[name + "_us"] = {"median": round(t["median_ms"] * 1e3 / n, 2), "min": round(t["min_ms"] * 1e3 / n, 2)}
    return out


def driver(mode, raft_iters, reps):
    from tools.motion_step import generator, movie

    G, x3, _ = generator(mode, raft_iters)
    x = x3[:, :2]
    Sn = 8
    labels = grid_labels(1)
    anchors = torch.tensor(PX.lattice_anchors(H // P, W // P, 9), device="cuda")
    n = (H // P) * (W // P)
    active = torch.ones((1, 2 * n), dtype=torch.bool, device="cuda")
    active[:, :n] = False
    active[:, n + anchors] = False
    a, shifts = active.unsqueeze(-1).expand(-1, -1, Sn), SS.directions(Sn, 2)

    def counterfactuals():
        with torch.random.fork_rng(devices=[]):
            return G.predict_counterfactual_videos_and_flows(x, a, None, shifts=shifts, num_samples=Sn, sample_batch_size=None, fix_passive=True, raft_iters=raft_iters)

    out = movie({"counterfactual_call": counterfactuals, "parallax": lambda: G.parallax(x, labels, num_samples=Sn, raft_iters=raft_iters)}, reps)
    res = G.parallax(x, labels, num_samples=Sn, raft_iters=raft_iters)
    out["pixels_with_parallax"], out["nearer_pairs"] = int(res.hist.sum()), int(res.nearer.sum())
    out["added_ms"] = round(out["parallax"]["median_ms"] - out["counterfactual_call"]["median_ms"], 4)
    out["added_share"] = round(out["added_ms"] / out["counterfactual_call"]["median_ms"], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="fast", choices=("fast", "parity"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--raft-iters", type=int, default=12)
    ap.add_argument("--call-only", action="store_true")
    ap.add_argument("--parent-root", default=None, help="a tree of the parent commit with its built library: the default track_scene of both, alternated")
    ap.add_argument("--batches", default="1,8", help="rows of the call alone")
    ap.add_argument("--samples", default="8,64", help="samples S of the call alone")
    ap.add_argument("--variants", default="full,dirs,bare", help="of the call alone: full (labels, no dirs), dirs (labels and dirs), bare (neither; par and cnt only)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "mode": args.mode, "raft_iters": args.raft_iters, "plane": [H, W]}
    for B in (int(v) for v in args.batches.split(",")):
        for Sn in (int(v) for v in args.samples.split(",")):
            for variant in args.variants.split(","):
                key = "B%d_S%d_%s" % (B, Sn, variant)
                out[key] = call_alone(B, Sn, variant, args.reps)
                print(key, out[key], file=sys.stderr, flush=True)
    if not args.call_only:
        out["driver"] = driver(args.mode, args.raft_iters, args.reps)
        print("driver", out["driver"], file=sys.stderr, flush=True)
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
