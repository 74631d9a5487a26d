"""Time one `MovabilityPredictor.forward` at the demo notebook's settings (16 + 2 x 16 samples, sample_batch_size 4, 224^2, 24 RAFT iterations):

    python tools/movability_step.py [--steps 3] [--warmup 1] [--samples 16] [--iters 2] [--raft-mode fast]

The IMU-conditioned base-4x4 predictor and the flow -> IMU model carry synthetic weights, RAFT-large is the flow model and the keypoint RAFT
(output_dim = 1) the keypoint predictor; `--raft-mode fast` runs both RAFT models with bf16-operand convolutions.  Prints one JSON line: ms per forward and its split into the predictors (the conditioned predictor and the
flow -> IMU model, without the RAFT calls inside it), RAFT (flow and keypoint forwards) and the rest (sampling, prompts, filter, motion maps, host).
The split synchronises around every model call, so `ms_split_total` is a little above the unsplit `ms_median`, which is timed in a pass of its own.
`--share-static-frame` builds the predictor with `share_static_frame=True`: the samples of a movie go to RAFT as pairs on one first frame, encoded once
(DESIGN.md §8.18); the line then carries the flow model's `last_encoder_images`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from counterfactualworldmodels_amd import config as C, conjoined_vmae as CV, masking, movability, synthetic as S  # noqa: E402
from counterfactualworldmodels_amd.raft import RAFT, _args  # noqa: E402


def conj(m, seed):
    m.load_state_dict({k: torch.from_numpy(S.synthetic_tensor(k, shp, seed)) for k, shp in C.conj_state_dict_schema(m.cfg).items()}, strict=False)
    return m


def raft(seed, output_dim=None):
    m = RAFT(_args(output_dim=output_dim))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(seed, output_dim=output_dim).items()})
    return m


class Clock:
    """Wall time spent inside the forward of the hooked modules, nested calls charged to the innermost bucket."""

    def __init__(self):
        self.total = {}
        self.stack = []
        self.on = False

    def hook(self, module, bucket):
        def pre(_m, _a):
            if self.on:
                torch.cuda.synchronize()
                self.stack.append([bucket, time.perf_counter(), 0.0])

        def post(_m, _a, _o):
            if self.on:
                torch.cuda.synchronize()
                b, t0, inner = self.stack.pop()
                dt = time.perf_counter() - t0
                self.total[b] = self.total.get(b, 0.0) + dt - inner
                if self.stack:
                    self.stack[-1][2] += dt

        module.register_forward_pre_hook(pre)
        module.register_forward_hook(post)
        if hasattr(module, "flow_pairs"):  # the shared-frame route does not go through forward: the same bucket
            inner = module.flow_pairs

            def flow_pairs(*a, **k):
                pre(module, a)
                out = inner(*a, **k)
                post(module, a, out)
                return out

            object.__setattr__(module, "flow_pairs", flow_pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--sample-batch-size", type=int, default=4)
    ap.add_argument("--raft-mode", default="parity", choices=["parity", "fast"], help="arithmetic of the flow model and the keypoint predictor")
    ap.add_argument("--share-static-frame", action="store_true", help="the samples of a movie share their first frame's RAFT features")
    args = ap.parse_args()
    pred = conj(CV.imu400_base_4x4patch_2frames_1tube(), 1)
    f2i = conj(CV.imu400_8x8patch_2frames_1tube_flowbackrgb01(), 0)
    flow_model, keypoints = raft(0).set_mode(args.raft_mode), raft(10, 1).set_mode(args.raft_mode)
    gen = masking.RotatedTableUniformMaskingGenerator(input_size=pred.mask_size, mask_ratio=0.99, clumping_factor=2)
    M = movability.MovabilityPredictor(
        predictor=pred, head_motion_predictor=f2i, flow_model=flow_model, keypoint_predictor=keypoints, temporal_dim=2, imagenet_normalize_inputs=True,
        mask_generator=gen, seed=0, num_initial_samples=args.samples, num_samples_per_iteration=args.samples, num_iters=args.iters,
        sample_batch_size=args.sample_batch_size, share_static_frame=args.share_static_frame).requires_grad_(False).to("cuda")
    clock = Clock()
    for mod, bucket in ((pred, "predictor"), (f2i, "predictor"), (flow_model, "raft"), (keypoints, "raft")):
        clock.hook(mod, bucket)
    x = torch.from_numpy(S.raft_frames(1, 224, 224, 11)).cuda()
    for _ in range(args.warmup):
        M(x)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        M(x)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    clock.on = True
    split = []
    for _ in range(args.steps):
        clock.total = {}
        t0 = time.perf_counter()
        M(x)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        split.append((dt, clock.total.get("predictor", 0.0), clock.total.get("raft", 0.0)))
    dt, p, r = (1e3 * float(np.median([s[i] for s in split])) for i in range(3))
    n = args.samples * (1 + args.iters)
    print(json.dumps({"raft_mode": args.raft_mode, "share_static_frame": bool(M.share_static_frame), "flow_encoder_images": list(flow_model.last_encoder_images), "samples": n, "iterations": args.iters, "sample_batch_size": args.sample_batch_size, "ms_median": round(1e3 * float(np.median(times)), 2),
                      "ms_min": round(1e3 * min(times), 2), "ms_split_total": round(dt, 2), "ms_predictor": round(p, 2), "ms_raft": round(r, 2),
                      "ms_rest": round(dt - p - r, 2), "kept_samples": [int((f.abs().amax((1, 2, 3)) > 0).sum()) for f in M.flow_samples_per_iter]}), flush=True)


if __name__ == "__main__":
    main()
