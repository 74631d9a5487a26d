"""Time ragged batches against rectangular ones:  python tools/ragged_step.py [--batch 32] [--reps 7] [--calls 10] [--warmup 3]

ViT-B/8 (synthetic weights, parity mode), one MI355X, one process:
  model level    `predict_video` of `--batch` rows: rectangular at n_vis = 792 (every row has 8 visible frame-2 patches) against ragged with the rows'
                 counts spread over 785 ... 792 (cap 792, `n_vis_range` given: no read-back).  ms per forward.
  wrapper level  `G.predict` on the unequal rows with the rectangulariser (the default: one read-back, host `randperm` draws, `cwm_mask_flip_picks`)
                 and with `ragged_batches=True` (one read-back of the counts' range).  ms per call, host clock around a call that ends in a
                 device synchronise.
A measurement is `--calls` back-to-back calls between two device events (model level) or synchronised host clocks (wrapper level) divided by their
number; `--reps` measurements per configuration, taken in alternation, reported as median, minimum and maximum.  One JSON line per configuration."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from counterfactualworldmodels_amd import _lib, config as C, prediction, synthetic as S, vmae  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    _lib.require_gpu()
    cfg = C.CONFIGS["base_8x8patch_2frames_1tube"]
    B = args.batch
    m = vmae.PretrainVisionTransformer(cfg, mode="parity")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 0).items()})
    m = m.to("cuda:0").eval()
    x = torch.from_numpy(S.synthetic_frames(B, cfg, 0)).cuda()
    rect_mask = torch.from_numpy(S.synthetic_masks(B, cfg, 8, 0)).cuda()
    ks = [1 + (r % 8) for r in range(B)]  # 785 ... 792 visible tokens
    ragged_mask = torch.from_numpy(np.stack([S.synthetic_masks(1, cfg, k, r)[0] for r, k in enumerate(ks)])).cuda()
    tokens_rect = torch.empty(B, cfg.num_tokens - 792, cfg.out_dim, device="cuda")
    tokens_ragged = torch.empty(B, cfg.num_tokens - 785, cfg.out_dim, device="cuda")
    video = torch.empty_like(x)
    G_rect = prediction.PredictorBasedGenerator(predictor=m, imagenet_normalize_inputs=True, temporal_dim=2)
    G_ragged = prediction.PredictorBasedGenerator(predictor=m, imagenet_normalize_inputs=True, temporal_dim=2, ragged_batches=True)

    configs = {
        "model_rectangular_792": lambda: m.predict_video(x, rect_mask, n_vis=792, check=False, out_tokens=tokens_rect, out_video=video),
        "model_ragged_785_792": lambda: m.predict_video(x, ragged_mask, check=False, out_tokens=tokens_ragged, out_video=video, ragged=True, n_vis_range=(785, 792)),
        "wrapper_rectangulariser": lambda: G_rect.predict(x, ragged_mask.clone(), frame=None),
        "wrapper_ragged_batches": lambda: G_ragged.predict(x, ragged_mask.clone(), frame=None),
    }

    def measure(name, call):
        if name.startswith("model_"):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.calls):
                call()
            end.record()
            end.synchronize()
            return start.elapsed_time(end) / args.calls
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    torch.manual_seed(0)
    for call in configs.values():
        for _ in range(args.warmup):
            call()
    torch.cuda.synchronize()
    times = {name: [] for name in configs}
    for _ in range(args.reps):
        for name, call in configs.items():
            times[name].append(measure(name, call))
    for name, t in times.items():
        t = np.array(t)
        print(json.dumps({"tool": "ragged_step", "config": name, "model": cfg.name, "mode": "parity", "batch": B, "calls_per_measurement": args.calls, "reps": args.reps,
                          "ms_per_call": [round(float(np.median(t)), 4), round(float(t.min()), 4), round(float(t.max()), 4)],
                          "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
