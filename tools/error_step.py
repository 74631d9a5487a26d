"""Timings of the patch-error path on the GPU, in one session (ViT-B/8, 224 x 224, synthetic weights):

  * `get_error_on_target_region` at batch B (default 32): the fused path (tokens -> cwm_patch_error) against the composed path (predicted video -> MSELoss ->
    avg_pool3d), alternated call by call, with the peak allocated memory of each
  * one `greedy_unmask` step over all 784 candidates of frame 1 at sample_batch_size 32 and 64
  * the kernel alone (cwm_patch_error on the tokens of one batch): time, and the bytes it has to move over that time

    python tools/error_step.py [--batch 32] [--mode fast|parity] [--reps 20] [--json PATH]

Device events around work that is synchronised before it is read; every shape is warmed up first.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from counterfactualworldmodels_amd import _lib, config as C, prediction, synthetic as S, vmae  # noqa: E402


def timed(fn, reps):
    """median and minimum milliseconds of `fn` over `reps` calls, each between two device events"""
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"median_ms": round(times[len(times) // 2], 4), "min_ms": round(times[0], 4), "reps": reps}


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def kernel_bytes(mask, T, Cc, P, n, frame):
    """What the kernel has to move for target = x: per (b, t) the tokens and the target pixels of the masked patches of the predicted frame f, both frames'
    pixels at its visible patches unless f = t (a patch against itself is 0 and is not read), and the map."""
    B = mask.shape[0]
    patch = P * P * Cc * 4
    per_frame = mask.view(B, T, n).sum(2)  # masked patches of frame f, per row
    total = 0
    for t in range(T):
        f = t if frame is None else frame % T
        nm = int(per_frame[:, f].sum())
        total += 2 * nm * patch + (0 if f == t else 2 * (B * n - nm) * patch) + B * n * 4
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--mode", default="fast", choices=("fast", "parity"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    cfg = C.CONFIGS["base_8x8patch_2frames_1tube"]
    m = vmae.PretrainVisionTransformer(cfg, mode=args.mode)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 0).items()})
    m = m.cuda().eval()
    fused = prediction.PredictorBasedGenerator(predictor=m, imagenet_normalize_inputs=True, temporal_dim=2)
    composed = prediction.PredictorBasedGenerator(predictor=m, imagenet_normalize_inputs=True, temporal_dim=2)
    composed._error_takes_fused_path = lambda *a, **k: False
    B, n, Nt, P = args.batch, cfg.tokens_per_frame, cfg.num_tokens, cfg.patch
    x = torch.from_numpy(S.synthetic_frames(B, cfg, 0)).cuda()
    mask = torch.from_numpy(S.synthetic_masks(B, cfg, 8, 0, 1)).cuda()
    target_mask = torch.ones_like(mask)
    target_mask[:, n:] = False  # the region: every patch of frame 1
    out = {"config": cfg.name, "mode": args.mode, "batch": B, "device": torch.cuda.get_device_name(0)}

    calls = {"fused": lambda: fused.get_error_on_target_region(x, mask, target_mask), "composed": lambda: composed.get_error_on_target_region(x, mask, target_mask)}
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    a, b = calls["fused"](), calls["composed"]()
    out["fused_vs_composed_max_abs"] = float((a - b).abs().max())
    rounds = {"fused": [], "composed": []}
    for _ in range(args.reps):  # alternated: both see the same clocks and the same neighbours
        for name, fn in calls.items():
            rounds[name].append(timed(fn, 1)["median_ms"])
    for name, ts in rounds.items():
        ts.sort()
        out["error_" + name] = {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "reps": len(ts), "peak_mib": peak_mib(calls[name])}

    # the kernel alone, on the tokens of this batch
    y, _ = m.predict_video(x, mask, normalize=True)
    emap = torch.empty((B, 2, cfg.img_size[0] // P, cfg.img_size[1] // P), device="cuda")
    mean = torch.empty((B,), device="cuda")
    region = (1 - target_mask.view(B, 2, *emap.shape[2:]).float()).contiguous()
    pa = _lib.fill_patch_args(_lib.new_patch_error_args(), x=x, mask=mask, region=region, y=y, geometry=(B, 2, cfg.in_chans, cfg.img_size[0], cfg.img_size[1], P),
                              n_vis=Nt - y.shape[1], map=emap, mean=mean, stream=_lib.current_stream_handle(torch.device("cuda:0")))
    lib = _lib.get_lib()
    import ctypes

    for frame, label in ((1, "frame1"), (-1, "each")):
        pa.frame = frame

        def launch(k=50):
            for _ in range(k):
                _lib.check(lib.cwm_patch_error(ctypes.byref(pa)))

        launch(5)
        t = timed(launch, max(3, args.reps // 4))
        nbytes = kernel_bytes(mask, 2, cfg.in_chans, P, n, None if frame < 0 else frame)
        out["kernel_" + label] = {"us_per_call": round(t["median_ms"] * 1e3 / 50, 2), "bytes": nbytes, "gb_per_s": round(nbytes / (t["median_ms"] * 1e-3 / 50) / 1e9, 1),
                                  "note": "map + mean launches, 50 calls back to back per timing"}

    # one greedy step over all candidates of frame 1
    x1 = x[:1]
    start = torch.zeros((1, Nt), dtype=torch.bool, device="cuda")
    start[:, n:] = True
    for sbs in (32, 64):
        step = lambda: fused.greedy_unmask(x1, start, num_steps=1, sample_batch_size=sbs)  # noqa: E731
        step()
        torch.cuda.synchronize()
        t = timed(step, max(3, args.reps // 6))
        out["greedy_step_sbs%d" % sbs] = dict(t, candidates=n, peak_mib=peak_mib(step), videos_not_written_gb=round(n * x1[0].numel() * 4 / 1e9, 3))
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
