"""Timings of frontier unmasking on the GPU, in one session (ViT-B/8, 224 x 224, synthetic weights):

  * one `frontier_unmask` step at batch B (default 32; top and race mode) against the fused `get_error_on_target_region` at the same batch -- the forward and
    the error map without the selection, i.e. what a caller paid before -- alternated call by call
  * the selection alone (`cwm_unmask_step` with nothing to reveal is the distance transform; with k = 8 the whole call minus `cwm_patch_error`, timed beside it)
    at 28 x 28 and 56 x 56 patches per frame
  * one `greedy_unmask` step with radius=1 against radius=None, from a mask with 8 visible patches in the frame, alternated

    python tools/unmask_step.py [--batch 32] [--mode fast|parity] [--reps 20] [--json PATH]

Device events around work that is synchronised before it is read; every shape is warmed up first.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from counterfactualworldmodels_amd import _lib, config as C, masking, prediction, synthetic as S, vmae  # noqa: E402


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(calls, reps):
    """{name: median / min ms}: the calls take turns, so that all of them see the same clocks and the same neighbours"""
    rounds = {k: [] for k in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            rounds[name].append(once(fn))
    out = {}
    for name, ts in rounds.items():
        ts.sort()
        out[name] = {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "reps": len(ts)}
    return out


def selection_alone(P, side, B, reps):
    """us per call of cwm_patch_error, of cwm_unmask_step (k = 8, radius 1) on the same arguments and of the distance transform alone, 50 calls per timing"""
    H = W = side * P
    n = side * side
    g = torch.Generator().manual_seed(0)
    x = torch.rand((B, 2, 3, H, W), generator=g).cuda()
    mask = torch.zeros((B, 2 * n), dtype=torch.bool)
    for b in range(B):
        mask[b, n + torch.randperm(n, generator=g)[: n - 8]] = True
    mask = mask.cuda()
    y = torch.randn((B, n - 8, P * P * 3), generator=g).cuda()
    emap, mean = torch.empty((B, 2, side, side), device="cuda"), torch.empty((B,), device="cuda")
    thr = torch.tensor([masking.frontier_threshold(side, side, 1)]).cuda()
    out_mask, picks = torch.empty_like(mask), torch.empty((B, 8), dtype=torch.int32, device="cuda")
    dist = torch.empty((B, n), device="cuda")
    a = _lib.new_unmask_step_args()
    _lib.fill_patch_args(a.base, x=x, mask=mask, y=y, geometry=(B, 2, 3, H, W, P), n_vis=n + 8, frame=1, map=emap, mean=mean,
                         stream=_lib.current_stream_handle(torch.device("cuda:0")))
    a.frame, a.threshold_dev, a.mask_out_dev, a.picks_dev = 1, thr.data_ptr(), out_mask.data_ptr(), picks.data_ptr()
    lib = _lib.get_lib()

    def error_only(k=50):
        for _ in range(k):
            _lib.check(lib.cwm_patch_error(ctypes.byref(a.base)))

    def step(k=50):
        a.num_reveal, a.dist_dev = 8, None
        for _ in range(k):
            _lib.check(lib.cwm_unmask_step(ctypes.byref(a)))

    def distance(k=50):
        a.num_reveal, a.dist_dev = 0, dist.data_ptr()
        for _ in range(k):
            _lib.check(lib.cwm_unmask_step(ctypes.byref(a)))

    calls = {"patch_error": error_only, "unmask_step_k8": step, "distance_only": distance}
    for fn in calls.values():
        fn(5)
    torch.cuda.synchronize()
    t = alternate(calls, reps)
    res = {name: round(v["median_ms"] * 1e3 / 50, 2) for name, v in t.items()}
    res["selection_us"] = round(res["unmask_step_k8"] - res["patch_error"], 2)
    return dict(res, batch=B, patches=n, note="us per call, 50 calls back to back per timing, alternated")


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
    G = prediction.PredictorBasedGenerator(predictor=m, imagenet_normalize_inputs=True, temporal_dim=2)
    B, n, Nt = args.batch, cfg.tokens_per_frame, cfg.num_tokens
    x = torch.from_numpy(S.synthetic_frames(B, cfg, 0)).cuda()
    mask = torch.from_numpy(S.synthetic_masks(B, cfg, 8, 0, 1)).cuda()
    target_mask = torch.ones_like(mask)
    target_mask[:, n:] = False  # the region: every patch of frame 1
    out = {"config": cfg.name, "mode": args.mode, "batch": B, "device": torch.cuda.get_device_name(0)}
    gen = torch.Generator(device="cuda").manual_seed(0)
    calls = {"error_fused": lambda: G.get_error_on_target_region(x, mask, target_mask),
             "frontier_step_top": lambda: G.frontier_unmask(x, mask, num_reveal=8, radius=1),
             "frontier_step_race": lambda: G.frontier_unmask(x, mask, num_reveal=8, radius=1, sample=True, generator=gen)}
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out.update(alternate(calls, args.reps))
    out["selection_28x28"] = selection_alone(8, 28, B, max(3, args.reps // 4))
    out["selection_56x56"] = selection_alone(4, 56, B, max(3, args.reps // 4))

    x1 = x[:1]
    start = torch.from_numpy(S.synthetic_masks(1, cfg, 8, 0, 1)).cuda()
    greedy = {"greedy_step_all": lambda: G.greedy_unmask(x1, start, num_steps=1, sample_batch_size=32),
              "greedy_step_radius1": lambda: G.greedy_unmask(x1, start, num_steps=1, sample_batch_size=32, radius=1)}
    for fn in greedy.values():  # (warm-up)
        fn()
    torch.cuda.synchronize()
    out.update(alternate(greedy, max(3, args.reps // 4)))
    out["greedy_step_all"]["candidates"] = len(G.greedy_unmask(x1, start, num_steps=1, sample_batch_size=32, return_scores=True)[3][0][0])
    out["greedy_step_radius1"]["candidates"] = len(G.greedy_unmask(x1, start, num_steps=1, sample_batch_size=32, radius=1, return_scores=True)[3][0][0])
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
