"""Time multi-shift prompt construction alone:  python tools/multi_shift_step.py [--samples 256] [--reps 7] [--launches 50] [--warmup 10]

The 256-prompt workload (B = 1, S = 256, 224^2, P = 8, T = 2, static movie) through `cwm_multi_shift_prompts` for K = 1 whole-patch shifts,
K = 4 whole-patch shifts and K = 4 fractional shifts (odd sx among them), and through `cwm_shift_prompts` (the single-shift kernel pair) on the
K = 1 tables, in the same process.  Per configuration: frames + masks in one call, and the frames kernel alone (mask output NULL).  A
measurement is the device-event time of `--launches` back-to-back calls divided by their number; `--reps` measurements per configuration are
taken in alternation (one round over all configurations after the other) and reported as median, minimum and maximum.  The K = 1 outputs of the
two entry points are compared bitwise before anything is timed.  One JSON line per configuration; bytes/s is on the bytes the frames kernel writes
(every prompt's frames once; what it reads is one movie, which stays in cache)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from counterfactualworldmodels_amd import _lib  # noqa: E402


def tables(Sn, K, fractional, H=224, W=224, P=8, seed=0):
    """One moved patch of frame 1 per step and prompt, nothing passive but frame 0; shifts of up to 3 patches (+ a sub-patch part)."""
    rng = np.random.Generator(np.random.PCG64(seed + 10 * K + fractional))
    gh, gw = H // P, W // P
    n = gh * gw
    points = np.zeros((Sn, K, 2 * n), dtype=bool)
    shifts = np.zeros((Sn, K, 2), dtype=np.int32)
    for s in range(Sn):
        for k in range(K):
            points[s, k, n + rng.integers(3, gh - 3) * gw + rng.integers(3, gw - 3)] = True
            shifts[s, k] = rng.integers(-3, 4, size=2) * P + (rng.integers(-(P - 1), P, size=2) if fractional else 0)
    base = np.ones((Sn, 1, 2 * n), dtype=bool)
    base[:, :, :n] = False
    return points, base, shifts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    _lib.require_gpu()
    lib, dev = _lib.get_lib(), torch.device("cuda:0")
    stream = _lib.current_stream_handle(dev)
    Sn, T, Cc, H, W, P = args.samples, 2, 3, 224, 224, 8
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(1, T, Cc, H, W, generator=gen).to(dev)
    x_out = torch.empty(Sn, T, Cc, H, W, device=dev)
    m_out = torch.empty(Sn, T * (H // P) * (W // P), dtype=torch.bool, device=dev)
    configs = {}
    for name, K, fractional in (("k1_whole", 1, False), ("k4_whole", 4, False), ("k4_fractional", 4, True)):
        pts, base, sh = tables(Sn, K, fractional)
        dev_t = (torch.from_numpy(pts).to(dev), torch.from_numpy(base).to(dev), torch.from_numpy(sh).to(dev))
        max_abs = int(np.abs(sh).max())

        def call(frames_only, dev_t=dev_t, K=K, max_abs=max_abs):
            _lib.check(lib.cwm_multi_shift_prompts(x.data_ptr(), 1, T, Cc, H, W, P, 1, Sn, K, 1, dev_t[0].data_ptr(), dev_t[1].data_ptr(), 1, dev_t[2].data_ptr(),
                                                   max_abs, x_out.data_ptr(), None if frames_only else m_out.data_ptr(), stream))

        configs[name] = dict(call=call, K=K, fractional=fractional, odd_sx=bool((sh[..., 1] % 2 != 0).any()))
    # the single-shift kernels on the K = 1 tables (active: 0 = moved; shifts in patches), and the bitwise comparison of the two entry points
    pts, base, sh = tables(Sn, 1, False)
    active = torch.from_numpy(~pts[:, 0]).to(dev)
    passive = torch.from_numpy(base[:, 0]).to(dev)
    patch_shifts = torch.from_numpy(sh[:, 0] // P).to(dev)

    def single(frames_only):
        _lib.check(lib.cwm_shift_prompts(x.data_ptr(), 1, T, Cc, H, W, P, 1, Sn, 1, active.data_ptr(), passive.data_ptr(), patch_shifts.data_ptr(), x_out.data_ptr(),
                                         None if frames_only else m_out.data_ptr(), stream))

    single(False)
    want_x, want_m = x_out.clone(), m_out.clone()
    x_out.zero_(), m_out.zero_()
    configs["k1_whole"]["call"](False)
    assert torch.equal(x_out, want_x) and torch.equal(m_out, want_m), "K = 1 differs from cwm_shift_prompts"
    del want_x
    configs["single_shift_k1"] = dict(call=single, K=1, fractional=False, odd_sx=False)

    def measure(call, frames_only):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.launches):
            call(frames_only)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3 / args.launches  # us per call

    for c in configs.values():
        for frames_only in (False, True):
            for _ in range(args.warmup):
                c["call"](frames_only)
    torch.cuda.synchronize()
    times = {(name, fo): [] for name in configs for fo in (False, True)}
    for _ in range(args.reps):
        for name, c in configs.items():
            for fo in (False, True):
                times[(name, fo)].append(measure(c["call"], fo))
    written = x_out.numel() * 4
    ref = float(np.median(times[("single_shift_k1", True)]))
    for name, c in configs.items():
        both, frames = np.array(times[(name, False)]), np.array(times[(name, True)])
        print(json.dumps({"tool": "multi_shift_step", "config": name, "K": c["K"], "fractional": c["fractional"], "odd_sx": c["odd_sx"], "prompts": Sn, "size": [H, W], "patch": P,
                          "launches_per_measurement": args.launches, "reps": args.reps,
                          "both_us": [round(float(np.median(both)), 2), round(float(both.min()), 2), round(float(both.max()), 2)],
                          "frames_us": [round(float(np.median(frames)), 2), round(float(frames.min()), 2), round(float(frames.max()), 2)],
                          "frames_bytes_written": written, "frames_tbytes_per_s": round(written / (float(np.median(frames)) * 1e-6) / 1e12, 3),
                          "frames_over_single_shift": round(float(np.median(frames)) / ref, 3), "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
