"""Golden vectors of RAFT's warm start (`flow_init`) and per-iteration outputs (`test_mode=False`), raft_model.py:199-300, captured by RUNNING
THE REFERENCE on the CPU (this container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_raft_warm.py

Weights and frames come from `synthetic.raft_state_dict` / `synthetic.raft_frames` (seeds stored); the init fields are seeded products of sines
and are stored, being small.  Every case records the reference's own fp32 rounding (`run_both` of make_golden_raft.py: the same network in
float64).  The maker asserts, on the reference alone, what makes the fixtures discriminate: a warm start moves the output by >= 0.5 px,
successive list elements differ by >= 0.1 px, a zeros init equals no init bit for bit, and list element k equals the `iters=k+1` call bit for bit.
The seeds of the weights, frames and init fields are this maker's own choice (10-16, chosen not to repeat those of make_golden_raft.py), so the
guard values it prints -- 22.99 and 21.80 px warm vs cold, 0.55 / 0.43 px between list elements -- are those of these inputs.  The request for these
fixtures quoted 22.9 / 19.2 px and 0.41 / 0.38 px without naming its seeds or the sines' frequencies: other inputs of the same recipe, values of the
same size, all far above the 0.5 / 0.1 px guards.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_raft import S, raft_module, run_both  # noqa: E402

WARM_MIN_PX = 0.5   # warm vs cold output, max-abs
STEP_MIN_PX = 0.1   # successive list elements, max-abs


def build(rm, seed: int, multiframe: bool, output_dim=None):
    args = rm.get_args("")
    args.multiframe, args.scale_inputs, args.output_dim = multiframe, True, output_dim
    m = rm.RAFT(args)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(seed, output_dim=output_dim).items()})
    return m.eval().requires_grad_(False)


def sine_field(B: int, h: int, w: int, seed: int, amp: float = 3.0) -> np.ndarray:
    """float32 [B,2,h,w], |v| <= amp: amp * sin(2 pi (fy y / h + py)) * sin(2 pi (fx x / w + px)) with seeded frequencies in [0.5, 2) and
    phases per batch row and channel: a smooth flow of a few 1/8-resolution pixels."""
    g = np.random.Generator(np.random.PCG64(seed))
    fy, fx = g.uniform(0.5, 2.0, (2, B, 2, 1, 1))
    py, px = g.uniform(0.0, 1.0, (2, B, 2, 1, 1))
    y = np.arange(h, dtype=np.float64).reshape(1, 1, h, 1) / h
    x = np.arange(w, dtype=np.float64).reshape(1, 1, 1, w) / w
    return (amp * np.sin(2 * np.pi * (fy * y + py)) * np.sin(2 * np.pi * (fx * x + px))).astype(np.float32)


def maxabs(a, b) -> float:
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def main():
    torch.set_num_threads(os.cpu_count() or 1)
    rm = raft_module()
    only = sys.argv[1:]
    t0 = time.time()

    def want(name):
        return not only or name in only

    # ---- 1: the two-image call with an init, 136 x 152 (odd 17 x 19 grid), B = 2, 4 iterations
    if want("raft_warm_136x152_b2"):
        seed, fseed, iseed, iters = 10, 11, 12, 4
        m = build(rm, seed, multiframe=False)
        x = torch.from_numpy(S.raft_frames(2, 136, 152, fseed, shift=(-3, 2)))
        init = sine_field(2, 17, 19, iseed)
        assert np.abs(init).max() <= 3.0

        def call(mm, dt, f):
            xx = x.to(dt) * 255.0
            return mm._forward_two_images(xx[:, 0], xx[:, 1], iters=iters, flow_init=None if f is None else torch.from_numpy(f).to(dt), test_mode=True)

        (low, up), drift = run_both(m, lambda mm, dt: call(mm, dt, init))
        with torch.no_grad():
            low_c, up_c = (t.numpy() for t in call(m, torch.float32, None))
            low_z, up_z = (t.numpy() for t in call(m, torch.float32, np.zeros_like(init)))
        warm = maxabs(up, up_c)
        assert warm >= WARM_MIN_PX, warm
        assert np.array_equal(low_z, low_c) and np.array_equal(up_z, up_c)  # a zeros init is no init, bit for bit
        np.savez_compressed(os.path.join(HERE, "raft_warm_136x152_b2.npz"), low=low, up=up, init=init, seed=np.array(seed), frames_seed=np.array(fseed),
                            shift=np.array([-3, 2]), iters=np.array(iters), drift=np.array(drift), warm_vs_cold=np.array(warm))
        print(f"[golden] raft_warm_136x152_b2 up {up.shape} max |up| {np.abs(up).max():.2f} warm vs cold {warm:.2f} px drift {drift:.3e} ({time.time() - t0:.0f}s)")

    # ---- 2: test_mode=False with an init, 128 x 128 (the smallest legal grid), B = 1, 3 iterations: the flow model and the output_dim = 1 model
    if want("raft_warm_list_128"):
        seed, fseed, iseed, iters = 12, 13, 14, 3
        x = torch.from_numpy(S.raft_frames(1, 128, 128, fseed))
        init = sine_field(1, 16, 16, iseed)
        out = {}
        for pre, output_dim in (("", None), ("kp_", 1)):
            m = build(rm, seed, multiframe=False, output_dim=output_dim)

            def call(mm, dt, n, test_mode):
                xx = x.to(dt) * 255.0
                y = mm._forward_two_images(xx[:, 0], xx[:, 1], iters=n, flow_init=torch.from_numpy(init).to(dt), test_mode=test_mode)
                return tuple(y)

            preds, drift = run_both(m, lambda mm, dt: call(mm, dt, iters, False))
            assert len(preds) == iters and all(p.shape == (1, output_dim or 2, 128, 128) for p in preds)
            steps = [maxabs(preds[k], preds[k - 1]) for k in range(1, iters)]
            if output_dim is None:  # (the keypoint map is no flow: its steps are recorded, not bounded in pixels)
                assert min(steps) >= STEP_MIN_PX, steps
            with torch.no_grad():
                for k in range(iters):  # list element k is the iters = k + 1 call, bit for bit
                    _, up_k = call(m, torch.float32, k + 1, True)
                    assert np.array_equal(up_k.numpy(), preds[k]), k
            out[pre + "preds"] = np.stack(preds)
            out[pre + "drift"] = np.array(drift)
            out[pre + "steps"] = np.array(steps)
            print(f"[golden] raft_warm_list_128 {pre or 'flow'} {out[pre + 'preds'].shape} steps {steps} drift {drift:.3e} ({time.time() - t0:.0f}s)")
        np.savez_compressed(os.path.join(HERE, "raft_warm_list_128.npz"), init=init, seed=np.array(seed), frames_seed=np.array(fseed), iters=np.array(iters),
                            **out)

    # ---- 3: the multi-frame call with one [1,2,16,20] init for every pair, 128 x 160, T = 3, 3 iterations, forward and backward
    if want("raft_warm_128x160_t3"):
        seed, fseed, iseed, iters = 14, 15, 16, 3
        m = build(rm, seed, multiframe=True)
        x = torch.from_numpy(S.raft_frames(1, 128, 160, fseed, shift=(2, -3), frames=3))
        init = sine_field(1, 16, 20, iseed)

        def call(mm, dt, f, backward):
            return mm(x.to(dt), iters=iters, backward=backward, flow_init=None if f is None else torch.from_numpy(f).to(dt))

        (yf,), df = run_both(m, lambda mm, dt: call(mm, dt, init, False))
        (yb,), db = run_both(m, lambda mm, dt: call(mm, dt, init, True))
        with torch.no_grad():
            cold = call(m, torch.float32, None, False).numpy()
            zero = call(m, torch.float32, np.zeros_like(init), False).numpy()
        warm = maxabs(yf, cold)
        assert warm >= WARM_MIN_PX, warm
        assert np.array_equal(zero, cold)
        np.savez_compressed(os.path.join(HERE, "raft_warm_128x160_t3.npz"), flow_fwd=yf, flow_bwd=yb, init=init, seed=np.array(seed),
                            frames_seed=np.array(fseed), shift=np.array([2, -3]), iters=np.array(iters), drift_fwd=np.array(df), drift_bwd=np.array(db),
                            warm_vs_cold=np.array(warm))
        print(f"[golden] raft_warm_128x160_t3 {yf.shape} warm vs cold {warm:.2f} px drift {df:.3e} / {db:.3e} ({time.time() - t0:.0f}s)")

    limit = os.path.getsize(os.path.join(HERE, "base8_k8_b2.npz"))  # the largest fixture committed before these
    for name in ("raft_warm_136x152_b2", "raft_warm_list_128", "raft_warm_128x160_t3"):
        p = os.path.join(HERE, name + ".npz")
        if os.path.exists(p):
            assert os.path.getsize(p) <= limit, (name, os.path.getsize(p), limit)
            print(f"[golden] {name}.npz {os.path.getsize(p)} bytes (limit {limit})")


if __name__ == "__main__":
    main()
