"""Timings of the object-interaction read-out on the GPU, in one session, at 224 x 224 with patches of 8:

  * `cwm_object_response` alone (one memset, the accumulate and the finalise kernel, and the allocation of its five outputs) at S = 8 and 64 samples for
    K = 8 and 64 pushes, on the sample-outer view of the flow model's output and on a packed [R,2,H,W,S] tensor
  * a torch composition of the same tables on the same GPU, as a user would write it today -- one int64 `scatter_add_` per table entry over widened
    temporaries --, whose integer tables are compared with the call's (cases of at most --compose-max rows x samples)
  * one `object_interactions` call of 8 slots (ViT-B/8 at synthetic weights, RAFT at random weights, S = 8) against the
    `predict_counterfactual_videos_and_flows` call on the same rows, alternated: what the masks, the read-out and the relations add to the call they follow

    python tools/interaction_step.py [--reps 20] [--raft-iters 12] [--mode fast|parity] [--call-only] [--rows 8,64] [--samples 8,64] [--json PATH]

Device events around work that is synchronised before it is read; every shape is warmed up first; calls alternate and medians are reported.  Prints one JSON
line.  `--call-only` stops after the call alone (the form to run under a kernel trace)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from counterfactualworldmodels_amd import _lib, config as C, object_response as OR, segment_step as SS, segmentation, synthetic as S, vmae  # noqa: E402
from counterfactualworldmodels_amd.raft import RAFT, _args  # noqa: E402
from tools.segment_step import alternate  # noqa: E402

H = W = 224
P = 8


def grid_labels(slots):
    """[1,H,W] uint8 on the device: `slots` rectangles on a grid over a background"""
    n = int(np.ceil(np.sqrt(slots)))
    ch, cw = H // n, W // n
    labels = np.zeros((1, H, W), np.uint8)
    for s in range(slots):
        y0, x0 = (s // n) * ch + ch // 6, (s % n) * cw + cw // 6
        labels[:, y0:y0 + 2 * ch // 3, x0:x0 + 2 * cw // 3] = s + 1
    return torch.from_numpy(labels).cuda()


def pushes(labels, K, Sn, seed):
    """the flow model's output [(k s),1,2,H,W] for K pushes of Sn samples: small noise, the pushed slot k + 1 moving 2 px along sample s's shift"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = 0.05 * torch.randn((K, Sn, 2, H, W), generator=g, device="cuda")
    d = torch.tensor(SS.directions(Sn), dtype=torch.float32, device="cuda")  # (dy, dx)
    on = (labels[0][None] == torch.arange(1, K + 1, device="cuda")[:, None, None]).float()  # [K,H,W]
    out[:, :, 0] += 2.0 * d[None, :, 1, None, None] * on[:, None]
    out[:, :, 1] += 2.0 * d[None, :, 0, None, None] * on[:, None]
    return out.reshape(K * Sn, 1, 2, H, W)


def torch_tables(flows, labels, min_q2):
    """the composition a user writes today: flows [R,2,H,W,S] view, labels [1,H,W]; returns tab [R,S,65,8] int64"""
    R, _, _, _, Sn = flows.shape
    dev = flows.device
    l = labels.long()
    l = torch.where(l > 64, 0, l)[:, :, :, None].expand(R, H, W, Sn)
    u, v = flows[:, 0], flows[:, 1]
    ok = (u.abs() <= 4096) & (v.abs() <= 4096)
    qu, qv = torch.round(torch.where(ok, u, 0.0) * 256).long(), torch.round(torch.where(ok, v, 0.0) * 256).long()
    q2 = qu * qu + qv * qv
    moved = ok & (q2 >= min_q2)
    index = (((torch.arange(R, device=dev)[:, None, None, None] * Sn + torch.arange(Sn, device=dev)) * 65) + l).reshape(-1)
    terms = [ok.long(), moved.long(), qu, qv, torch.where(moved, qu, 0), torch.where(moved, qv, 0), q2, (~ok).long()]
    return torch.stack([torch.zeros(R * Sn * 65, dtype=torch.long, device=dev).scatter_add_(0, index, t.reshape(-1)) for t in terms], -1).reshape(R, Sn, 65, 8)


def call_alone(K, Sn, reps, compose):
    """us per call of the library call on both layouts (10 calls per timing, outputs allocated by every call) and of the torch composition"""
    labels = grid_labels(max(K, 8))
    outer = pushes(labels, K, Sn, K + Sn)
    view = segmentation.FlowGenerator.batch_to_samples(outer, B=K)  # [K,2,H,W,S], sample-outer
    packed = view.contiguous()
    pushed = torch.arange(1, K + 1, dtype=torch.int32, device="cuda")
    dirs = torch.tensor([(dy * P, dx * P) for dy, dx in SS.directions(Sn)], dtype=torch.int32, device="cuda")
    kw = dict(dirs=dirs, min_mag=1.0)
    per = 10
    calls = {"sample_outer": lambda: [OR.measure_device(view, labels, pushed, **kw) for _ in range(per)],
             "packed": lambda: [OR.measure_device(packed, labels, pushed, **kw) for _ in range(per)]}
    a, b = OR.measure_device(view, labels, pushed, **kw), OR.measure_device(packed, labels, pushed, **kw)
    torch.cuda.synchronize()
    same = all(torch.equal(getattr(a, k).view(torch.int64) if k == "coupling" else getattr(a, k), getattr(b, k).view(torch.int64) if k == "coupling" else getattr(b, k))
               for k in OR.ObjectResponse.__slots__[:5])
    # what the accumulate pass moves: u and v of every (row, sample, pixel), the label byte per (row, sample) -- the map itself is 50 KB and stays in cache --,
    # and the table it zeroes and adds into
    table = K * Sn * 65 * 8 * 8
    out = {"rows": K, "samples": Sn, "n_valid": a.stats[0, :, 0].tolist()[:4], "layouts_equal": bool(same), "flow_bytes": K * Sn * H * W * 8,
           "bytes_moved": K * Sn * H * W * 9 + 2 * table, "table_bytes": table}
    if compose:
        calls["torch_composition"] = lambda: torch_tables(view, labels, 65536)
        out["tables_equal_torch"] = bool(torch.equal(a.tab[0], torch_tables(view, labels, 65536)))
    for name, t in alternate(calls, reps).items():
        n = 1 if name == "torch_composition" else per
        out[name + "_us"] = {"median": round(t["median_ms"] * 1e3 / n, 2), "min": round(t["min_ms"] * 1e3 / n, 2)}
        if name != "torch_composition":
            out[name + "_call_TBps"] = round(out["bytes_moved"] / (t["median_ms"] * 1e-3 / n) / 1e12, 3)
    return out


def driver(mode, raft_iters, reps):
    cfg = C.CONFIGS["base_8x8patch_2frames_1tube"]
    m = vmae.PretrainVisionTransformer(cfg, mode=mode)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 0).items()})
    raft = RAFT(_args(mixed_precision=(mode == "fast")))
    raft.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(0).items()})
    G = segmentation.FlowGenerator(predictor=m.cuda().eval(), flow_model=raft.cuda().eval(), imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
    x = torch.from_numpy(S.synthetic_frames(1, cfg, 0)).cuda()
    Sn, K = 8, 8
    labels = grid_labels(K)
    slots = torch.arange(1, K + 1, device="cuda")[None]
    active, passive, _ = OR.push_masks(labels, slots, P)
    a, p = (t.reshape(K, -1).unsqueeze(-1).expand(-1, -1, Sn) for t in (active, passive))
    rows_x, shifts = x.repeat_interleave(K, 0), SS.directions(Sn)

    def counterfactuals():
        with torch.random.fork_rng(devices=[]):
            return G.predict_counterfactual_videos_and_flows(rows_x, a, p, shifts=shifts, num_samples=Sn, sample_batch_size=None, fix_passive=True, raft_iters=raft_iters)

    calls = {"counterfactual_call": counterfactuals,
             "object_interactions": lambda: G.object_interactions(x, labels, num_slots=K, num_samples=Sn, raft_iters=raft_iters)}
    for fn in calls.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out = alternate(calls, max(3, reps // 2))
    res = G.object_interactions(x, labels, num_slots=K, num_samples=Sn, raft_iters=raft_iters)
    out["n_valid"], out["links"] = res.stats[0, :, 0].tolist(), int(res.moves.sum())
    out["added_ms"] = round(out["object_interactions"]["median_ms"] - out["counterfactual_call"]["median_ms"], 4)
    out["added_share"] = round(out["added_ms"] / out["counterfactual_call"]["median_ms"], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="fast", choices=("fast", "parity"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--raft-iters", type=int, default=12)
    ap.add_argument("--call-only", action="store_true")
    ap.add_argument("--rows", default="8,64", help="pushes K of the call alone")
    ap.add_argument("--samples", default="8,64", help="samples S of the call alone")
    ap.add_argument("--compose-max", type=int, default=512, help="the torch composition runs where rows x samples is at most this")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "mode": args.mode, "raft_iters": args.raft_iters}
    for K in (int(v) for v in args.rows.split(",")):
        for Sn in (int(v) for v in args.samples.split(",")):
            out["K%d_S%d" % (K, Sn)] = call_alone(K, Sn, args.reps, K * Sn <= args.compose_max)
    if not args.call_only:
        out["driver_8_slots"] = driver(args.mode, args.raft_iters, args.reps)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
