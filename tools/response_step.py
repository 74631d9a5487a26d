"""Timings of the marker-response path on the GPU, in one session (ViT-B/8, 224 x 224, synthetic weights):

  * `predict_marker_responses` for K = 32 and K = 784 markers (every patch of frame 0) in chunks of `--chunk` rows: the fused path (tokens ->
    cwm_token_response) against the composed path (predicted videos -> squared difference -> statistics in torch), alternated call by call, with the peak
    allocated memory of each
  * the kernel alone (cwm_token_response on the tokens of one chunk, one shared reference): time, and the bytes it has to move over that time

    python tools/response_step.py [--chunk 32] [--mode fast|parity] [--reps 10] [--json PATH]

Device events around work that is synchronised before it is read; every shape is warmed up first.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from counterfactualworldmodels_amd import _lib, config as C, prediction, synthetic as S, vmae  # noqa: E402


def timed(fn, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--mode", default="fast", choices=("fast", "parity"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    cfg = C.CONFIGS["base_8x8patch_2frames_1tube"]
    m = vmae.PretrainVisionTransformer(cfg, mode=args.mode)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 0).items()})
    m = m.cuda().eval()
    fused = prediction.PredictorBasedGenerator(predictor=m, imagenet_normalize_inputs=True, temporal_dim=2)
    composed = prediction.PredictorBasedGenerator(predictor=m, imagenet_normalize_inputs=True, temporal_dim=2)
    composed._responses_take_fused_path = lambda *a, **k: False
    n, Nt, P = cfg.tokens_per_frame, cfg.num_tokens, cfg.patch
    H, W = cfg.img_size
    g = W // P
    x = torch.from_numpy(S.synthetic_frames(1, cfg, 0)).cuda()
    every = [[i, j] for i in range(H // P) for j in range(g)]
    out = {"config": cfg.name, "mode": args.mode, "chunk": args.chunk, "device": torch.cuda.get_device_name(0)}
    for K in (32, len(every)):
        patches = every[:: len(every) // K][:K]
        calls = {"fused": lambda: fused.predict_marker_responses(x, patches, sample_batch_size=args.chunk),
                 "composed": lambda: composed.predict_marker_responses(x, patches, sample_batch_size=args.chunk)}
        for fn in calls.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        a, b = calls["fused"](), calls["composed"]()
        rec = {"peaks_equal": bool(np.array_equal(a.peak_yx, b.peak_yx)), "mass_max_rel": float(np.abs(a.mass - b.mass).max() / np.abs(b.mass).max()),
               "videos_and_maps_not_written_gb": round(K * (x[0].numel() + H * W) * 4 / 1e9, 3)}
        reps = args.reps if K <= 64 else max(2, args.reps // 4)
        rounds = {"fused": [], "composed": []}
        for _ in range(reps):  # alternated: both see the same clocks and the same neighbours
            for name, fn in calls.items():
                rounds[name].append(timed(fn, 1)["median_ms"])
        for name, ts in rounds.items():
            ts.sort()
            rec[name] = {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "reps": len(ts), "peak_mib": peak_mib(calls[name])}
        out["K%d" % K] = rec

    # the kernel alone, on the tokens of one chunk against one shared reference
    B = args.chunk
    mask = fused.get_zeros_mask(x, frame=-1).expand(B, -1).contiguous()
    y = m.predict_video(torch.from_numpy(S.synthetic_frames(B, cfg, 1)).cuda(), mask, normalize=True)[0]
    y_ref = m.predict_video(x, mask[:1], normalize=True)[0]
    index = torch.empty((B,), device="cuda", dtype=torch.int32)
    stats = torch.empty((B, 4), device="cuda")
    scratch = torch.empty((B, H // P, 8), device="cuda")
    pixels = torch.empty((B, H, W), device="cuda")
    a = _lib.new_token_response_args()
    _lib.fill_patch_args(a.base, mask=mask, y=y, geometry=(B, 2, cfg.in_chans, H, W, P), n_vis=Nt - y.shape[1], frame=1, scratch=scratch,
                         stream=_lib.current_stream_handle(torch.device("cuda:0")))
    a.y_ref_dev, a.y_ref_stride_b, a.peak_index_dev, a.stats_dev = y_ref.data_ptr(), 0, index.data_ptr(), stats.data_ptr()
    lib = _lib.get_lib()
    for label, pix in (("statistics", None), ("statistics_and_pixel_map", pixels)):
        a.pixel_map_dev = _lib.ptr(pix)

        def launch(k=50):
            for _ in range(k):
                _lib.check(lib.cwm_token_response(ctypes.byref(a)))

        launch(5)
        t = timed(launch, max(3, args.reps // 2))
        nbytes = y.numel() * 4 + y_ref.numel() * 4 + (0 if pix is None else pix.numel() * 4)  # (the shared reference is read once from memory, then from cache)
        out["kernel_" + label] = {"us_per_call": round(t["median_ms"] * 1e3 / 50, 2), "bytes": nbytes, "gb_per_s": round(nbytes / (t["median_ms"] * 1e-3 / 50) / 1e9, 1),
                                  "note": "both launches, 50 calls back to back per timing"}
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
