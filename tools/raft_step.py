"""Time RAFT-large (counterfactualworldmodels_amd.raft) at 224^2, 24 iterations:  python tools/raft_step.py [--batch 1 8 32] [--steps 10] [--warmup 3] [--mode fast]

Reports ms per call, frame pairs/s and algorithmic TFLOP/s on the FLOPs this path computes (config.raft_algorithmic_flops: the mask head
once, ~122 GFLOP per pair), one JSON line per batch size.  For the kernel split run it once under
`rocprofv3 --kernel-trace --stats -- python tools/raft_step.py --batch 32 --steps 3`.

`--output-dim 1` times the keypoint predictor instead (the model with the output head: one more 3x3 convolution, the 256 -> 1 projection and a
one-channel convex upsampling in place of the flow's two-channel one); its FLOPs add the head's convolution and projection.
`--mode fast` times the bf16-operand mode instead of parity; every line names its mode.
`--corr on_the_fly` times the forward that computes its correlations at lookup time (RAFT.set_corr) and books its FLOPs; every line names
the form and the bytes of workspace the handle holds after the timed forwards (`workspace_bytes`).
`--flow-init` times a warm-started forward (`flow_init`: one seeded [1,2,H/8,W/8] field for every pair; one more small launch).
`--per-iteration` times the list form (the two-image call with `test_mode=False`: the mask head and the upsampling in every iteration, +0.69 GFLOP
and one full-resolution write each) and prints, per iteration, max-abs and mean-abs of (prediction i - prediction i-1) in pixels: how fast the
flow settles, which is what `set_raft_iters` is chosen from.
`--warm-start --frames T` times a movie of T frames three ways in one process and prints one line with all three: the warm chain on the device
(`warm_start=True`: T-1 forwards one after another with `forward_interpolate` between them), the cold multi-frame call on the same
movie (all pairs in one launch set), and the same chain with the interpolation done on the host between two-image calls, by the numpy restatement
of tests/raft_video_restatement.py: the synchronisation, the copy down, the search and the copy back a user of the reference's protocol pays; and the
interpolation kernel alone.
`--share` turns `share_frames` on (the encoders once per distinct frame of a call) for whatever else is timed; `--frames T` without
`--warm-start` times the cold multi-frame call on a movie of T frames.  `--shared-first S` times B rows x S pairs on one first frame per row through
`RAFT.flow_pairs`, with the flag off and then on in one session, and prints both with `last_encoder_images` (fnet, cnet) and their ratio."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from counterfactualworldmodels_amd import config as C, synthetic as S  # noqa: E402
from counterfactualworldmodels_amd.raft import RAFT, _args, forward_interpolate  # noqa: E402


def timed(run, warmup, steps):
    """median and min ms of run() followed by a device synchronise"""
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(times)), 1e3 * min(times)


def warm_start_lines(m, args):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import raft_video_restatement as R

    H, W = args.size
    T = args.frames
    for B in args.batch:
        x = torch.from_numpy(S.raft_frames(B, H, W, 1, frames=T)).cuda()
        x255 = x * 255.0

        def host_chain():
            init, ups = None, []
            for t in range(T - 1):
                low, up = m._forward_two_images(x255[:, t], x255[:, t + 1], iters=args.iters, flow_init=init)
                ups.append(up)
                if t + 1 < T - 1:  # .cpu() synchronises; the search runs on the host; the result goes back up
                    init = torch.from_numpy(R.forward_interpolate(low.cpu().numpy())).cuda()
            return ups

        low = m._forward_two_images(x255[:, 0], x255[:, 1], iters=args.iters)[0]
        chain = timed(lambda: m(x, iters=args.iters, warm_start=True), args.warmup, args.steps)
        cold = timed(lambda: m(x, iters=args.iters), args.warmup, args.steps)
        host = timed(host_chain, args.warmup, args.steps)
        kern = timed(lambda: forward_interpolate(low), args.warmup, max(args.steps, 20))
        same = all(torch.equal(a, b) for a, b in zip(host_chain(), m(x, iters=args.iters, warm_start=True).unbind(1)))
        print(json.dumps({"warm_start": True, "mode": m.mode, "batch": B, "frames": T, "size": [H, W], "iters": args.iters,
                          "corr": m.corr, "workspace_bytes": m.workspace_bytes(),
                          "chain_device_ms": round(chain[0], 3), "chain_device_ms_min": round(chain[1], 3),
                          "cold_multiframe_ms": round(cold[0], 3), "cold_multiframe_ms_min": round(cold[1], 3),
                          "chain_through_host_ms": round(host[0], 3), "chain_through_host_ms_min": round(host[1], 3),
                          "forward_interpolate_ms": round(kern[0], 4), "device_chain_equals_host_chain": bool(same),
                          "chain_device_ms_per_pair": round(chain[0] / (B * (T - 1)), 3), "cold_ms_per_pair": round(cold[0] / (B * (T - 1)), 3),
                          "chain_through_host_ms_per_pair": round(host[0] / (B * (T - 1)), 3)}), flush=True)


def shared_first_lines(m, args):
    """B rows x S pairs on one first frame per row (`flow_pairs` on an expanded view): unshared, then shared, in one session"""
    H, W = args.size
    S_ = args.shared_first
    for B in args.batch:
        x = torch.from_numpy(S.raft_frames(B, H, W, 1, frames=S_ + 1)).cuda()
        first, second = x[:, :1].expand(-1, S_, -1, -1, -1), x[:, 1:]
        res = {}
        for share in (False, True, False, True):  # (each setting twice, alternating: a drift of the clock would show)
            ms = timed(lambda: m.flow_pairs(first, second, iters=args.iters, share=share), args.warmup, args.steps)
            res.setdefault(share, []).append((ms, m.last_encoder_images, m.workspace_bytes()))
        off, on = (min(res[k], key=lambda r: r[0][0]) for k in (False, True))
        err = (m.flow_pairs(first, second, iters=args.iters, share=True) - m.flow_pairs(first, second, iters=args.iters, share=False)).abs().max().item()
        print(json.dumps({"shared_first": S_, "mode": m.mode, "corr": m.corr, "batch": B, "size": [H, W], "iters": args.iters,
                          "off_ms_median": round(off[0][0], 3), "off_ms_min": round(off[0][1], 3), "off_encoder_images": list(off[1]), "off_workspace_bytes": off[2],
                          "on_ms_median": round(on[0][0], 3), "on_ms_min": round(on[0][1], 3), "on_encoder_images": list(on[1]), "on_workspace_bytes": on[2],
                          "all_ms_median": {str(k): [round(r[0][0], 3) for r in v] for k, v in res.items()},
                          "on_over_off": round(on[0][0] / off[0][0], 4), "max_abs_on_minus_off_px": err}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--size", type=int, nargs=2, default=[224, 224])
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--output-dim", type=int, default=None, choices=[1], help="time the keypoint forward (the output head) instead of the flow forward")
    ap.add_argument("--mode", default="parity", choices=["parity", "fast"], help="arithmetic of the convolutions (RAFT.set_mode)")
    ap.add_argument("--corr", default="all_pairs", choices=["all_pairs", "on_the_fly"], help="the correlation: the all-pairs volume, or computed at lookup time (RAFT.set_corr)")
    ap.add_argument("--flow-init", action="store_true", help="time a warm-started forward (flow_init)")
    ap.add_argument("--per-iteration", action="store_true", help="time the list form (test_mode=False) and print how much each iteration moves the prediction")
    ap.add_argument("--warm-start", action="store_true", help="time a warm-started movie: the device chain, the cold call and the chain through the host")
    ap.add_argument("--frames", type=int, default=None, help="frames of the movie (default 2; 4 with --warm-start)")
    ap.add_argument("--share", action="store_true", help="share_frames: the encoders once per distinct frame of a call (RAFT.set_share_frames)")
    ap.add_argument("--shared-first", type=int, default=None, metavar="S", help="time B rows x S pairs on one first frame per row (flow_pairs), flag off and on")
    args = ap.parse_args()
    if args.frames is None:
        args.frames = 4 if args.warm_start else 2
    if args.shared_first is not None and (args.shared_first < 1 or args.warm_start or args.per_iteration or args.flow_init or args.output_dim):
        ap.error("--shared-first S >= 1 times the flow forward only: it excludes --warm-start, --per-iteration, --flow-init and --output-dim")
    if args.warm_start and (args.frames < 3 or args.flow_init or args.per_iteration):
        ap.error("--warm-start needs --frames >= 3 and excludes --flow-init and --per-iteration")
    H, W = args.size
    m = RAFT(_args(output_dim=args.output_dim)) if args.output_dim else RAFT()
    m.set_mode(args.mode)
    m.set_corr(args.corr)
    m.set_share_frames(args.share)
    sd = S.raft_state_dict(0, output_dim=args.output_dim) if args.output_dim else S.raft_state_dict(0)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.cuda().eval()
    flops = C.raft_algorithmic_flops(H, W, args.iters, corr=args.corr)
    if args.output_dim:  # output_block.0 (3x3, 128 -> 256) and output_block.2 (256 -> output_dim) at 1/8 resolution
        flops += 2.0 * (H // 8) * (W // 8) * 256 * (128 * 9 + args.output_dim)
    if args.per_iteration:  # the mask head (3x3, 128 -> 256, and 1x1, 256 -> 576) in every iteration instead of once; with the head, output_block too
        per_it = 2.0 * (H // 8) * (W // 8) * 256 * (128 * 9 + 576)
        if args.output_dim:
            per_it += 2.0 * (H // 8) * (W // 8) * 256 * (128 * 9 + args.output_dim)
        flops += (args.iters - 1) * per_it
    if args.warm_start:
        return warm_start_lines(m, args)
    if args.shared_first is not None:
        return shared_first_lines(m, args)
    init = None
    if args.flow_init:
        g = torch.Generator().manual_seed(2)
        init = (4.0 * torch.rand(1, 2, H // 8, W // 8, generator=g) - 2.0).cuda()
    for B in args.batch:
        x = torch.from_numpy(S.raft_frames(B, H, W, 1, frames=args.frames)).cuda()
        pairs = B * max(args.frames - 1, 1)
        if args.per_iteration:
            x1, x2 = (x[:, 0] * 255.0).contiguous(), (x[:, 1] * 255.0).contiguous()

            def run():
                return m._forward_two_images(x1, x2, iters=args.iters, flow_init=init, test_mode=False)
        else:
            def run():
                return m(x, iters=args.iters, flow_init=init)
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            out = run()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        ms = 1e3 * float(np.median(times))
        if args.per_iteration:
            for i in range(1, len(out)):
                d = (out[i] - out[i - 1]).abs()
                print(json.dumps({"batch": B, "iteration": i + 1, "step_max_abs_px": round(d.max().item(), 4), "step_mean_abs_px": round(d.mean().item(), 5)}), flush=True)
        print(json.dumps({"output": "keypoints" if args.output_dim else "flow", "mode": m.mode, "corr": m.corr, "flow_init": bool(args.flow_init), "per_iteration": bool(args.per_iteration), "batch": B, "frames": args.frames, "share_frames": m.share_frames,
                          "encoder_images": list(m.last_encoder_images), "size": [H, W], "iters": args.iters, "workspace_bytes": m.workspace_bytes(), "ms_median": round(ms, 3), "ms_min": round(1e3 * min(times), 3),
                          "pairs_per_s": round(pairs / (ms / 1e3), 2), "gflop_per_pair": round(flops / 1e9, 2),
                          "tflops": round(pairs * flops / (ms / 1e3) / 1e12, 2)}), flush=True)


if __name__ == "__main__":
    main()
