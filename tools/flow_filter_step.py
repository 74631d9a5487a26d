"""Time `FlowSampleFilter.forward` at B=1, 224^2, 28^2 patches:  python tools/flow_filter_step.py [--samples 24 256] [--steps 50] [--warmup 5]

For each S and each layout -- `view`: the sample-outermost view `_batch_to_samples` hands over; `packed`: the contiguous sample-innermost tensor --
device-event times (medians over --steps calls after --warmup, every call on a fresh copy of the same flows so that each one zeroes the same samples) of

  * `forward` (statistics + zeroing + the contiguous result),
  * its parts: the statistics pass alone, and for `view` the transposing pack kernel against `apply + .contiguous()`,
  * a torch restatement of the reference's forward (tests/flow_filter_restatement.py) on the same device: the yardstick,

and the statistics pass's achieved bytes/s on the bytes it must read (the flows once + the mask of frame 2).  One JSON line per (S, layout).
About half of the samples are rejected (blobs placed off their active patch); decisions are checked against the restatement before timing."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import flow_filter_restatement as R  # noqa: E402
from counterfactualworldmodels_amd import _lib, sampling, segmentation, synthetic as S  # noqa: E402


def make_case(Sn, size=224, grid=28, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed + Sn))
    blobs = np.zeros((1, Sn, 1, 5), dtype=np.float32)
    active = np.ones((1, 2 * grid * grid, Sn), dtype=bool)
    active[:, : grid * grid] = False
    ratio = size // grid
    for s in range(Sn):
        py, px = rng.integers(2, grid - 2, size=2)
        active[0, grid * grid + py * grid + px, s] = False
        off = 0 if s % 2 else 80  # every other blob misses its active patch: rejected by patch_magnitude
        blobs[0, s, 0] = (((py + 0.5) * ratio + off) % size, (px + 0.5) * ratio, 20.0, 15.0, -12.0)
    return S.blob_flow_samples(size, seed, blobs), active


def timed(fn, fresh, steps, warmup):
    """Median device time (ms) of fn(x) over fresh inputs x = fresh(); the copies are outside the timed window."""
    times = []
    for i in range(warmup + steps):
        x = fresh()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn(x)
        end.record()
        end.synchronize()
        if i >= warmup:
            times.append(start.elapsed_time(end))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, nargs="+", default=[24, 256])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    _lib.require_gpu()
    for Sn in args.samples:
        flows_np, active = make_case(Sn)
        act = torch.from_numpy(active).cuda()
        packed = torch.from_numpy(flows_np).cuda()
        B, Cc, H, W, _ = packed.shape
        batch = packed.permute(0, 4, 1, 2, 3).reshape(B * Sn, 1, Cc, H, W).contiguous()
        filt = sampling.FlowSampleFilter()
        for layout in ("view", "packed"):
            def fresh():
                return segmentation.FlowGenerator.batch_to_samples(batch.clone(), t=0, B=B) if layout == "view" else packed.clone()

            out, _ = filt(fresh(), act)
            want, _, dec = R.flow_filter_forward(fresh(), act)
            assert torch.equal(filt.last_stats["reject"], dec) and torch.equal(out, want), "decisions differ from the restatement"
            rej = filt.last_stats["reject"]

            def apply_then_contiguous(x):
                f, st = sampling._strides5(x)
                _lib.check(_lib.get_lib().cwm_flow_filter_apply(f.data_ptr(), st, B, Cc, H, W, Sn, rej.data_ptr(), _lib.current_stream_handle(f.device)))
                return f.contiguous()

            def apply_then_pack(x):
                f, st = sampling._strides5(x)
                lib, stream = _lib.get_lib(), _lib.current_stream_handle(f.device)
                _lib.check(lib.cwm_flow_filter_apply(f.data_ptr(), st, B, Cc, H, W, Sn, rej.data_ptr(), stream))
                o = torch.empty((B, Cc, H, W, Sn), device=f.device, dtype=torch.float32)
                _lib.check(lib.cwm_flow_filter_pack(f.data_ptr(), st, B, Cc, H, W, Sn, rej.data_ptr(), o.data_ptr(), stream))
                return o

            t = {"forward_ms": timed(lambda x: filt(x, act), fresh, args.steps, args.warmup),
                 "stats_ms": timed(lambda x: filt.compute_stats(x, act), fresh, args.steps, args.warmup),
                 "torch_restatement_ms": timed(lambda x: R.flow_filter_forward(x, act), fresh, args.steps, args.warmup)}
            if layout == "view":
                t["apply_pack_ms"] = timed(apply_then_pack, fresh, args.steps, args.warmup)
                t["apply_contiguous_ms"] = timed(apply_then_contiguous, fresh, args.steps, args.warmup)
            else:
                t["apply_ms"] = timed(apply_then_contiguous, fresh, args.steps, args.warmup)
            stats_bytes = packed.numel() * 4 + active.shape[1] // 2 * Sn
            line = {"tool": "flow_filter_step", "B": B, "S": Sn, "size": [H, W], "patches": active.shape[1] // 2, "layout": layout, "rejected": int(rej.sum()),
                    "steps": args.steps, "device": torch.cuda.get_device_name(0)}
            line.update({k: round(v, 4) for k, v in t.items()})
            line["torch_over_forward"] = round(t["torch_restatement_ms"] / t["forward_ms"], 2)
            line["stats_bytes"] = stats_bytes
            line["stats_gbytes_per_s"] = round(stats_bytes / (t["stats_ms"] * 1e-3) / 1e9, 1)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
