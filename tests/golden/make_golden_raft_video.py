"""Golden vectors of RAFT's video warm start: `forward_interpolate` (cwm/models/raft/utils.py:28-56, scipy's `griddata(..., method='nearest')`) on seeded
fields, and a warm-started chain over a 4-frame movie built from the reference's `_forward_two_images` and `forward_interpolate`, captured by RUNNING
THE REFERENCE on the CPU (this container only; scipy 1.15.3):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_raft_video.py

`raft_finterp_fields.npz`: per field `<name>_in` and `<name>_out` [2,h,w] float32 and `<name>_gap`.  A field is `sine_field` of make_golden_raft_warm.py
(a product of sines per channel) plus 0.05 * standard normal noise, which separates the landing points of a smooth field: without it neighbouring
sources land at near-equal distances from a target.  On the reference alone the maker asserts for every field that the float64 brute-force restatement
(tests/raft_video_restatement.py) equals scipy's result bit for bit on every element, that the smallest gap between the best and the second-best
squared distance over all targets is >= 1e-9 (no ties: scipy's tie order is its KD-tree's own), that >= 3 % of the sources are invalid and that
>= half of the targets change value.

`raft_video_128x160_t4.npz`: weights `raft_state_dict(seed)`, frames `raft_frames(1, 128, 160, frames_seed, shift=(2,-3), frames=4)`, 3 iterations.
Forward chain: pair t = (x[t], x[t+1]), t = 0, 1, 2; backward chain: pair t = (x[t+1], x[t]), t = 2, 1, 0; the first pair of a chain is cold, every
later one starts from the reference's `forward_interpolate(low of the pair before it)`.  Stored per chain step k: `<dir>_init_k` (k >= 1), `<dir>_low_k`,
and `fwd_up_k`; the cold multi-frame call's `cold_fwd` / `cold_bwd` low-resolution flows; `warm_vs_cold_<dir>` [3] (max-abs of the full-resolution flow
against the cold call's, pixels, per chain step) and `drift_<dir>` [3]: each pair's fp32 result against the same network in float64 fed the same init
(`run_both`: teacher-forced, because a nearest-neighbour choice is discontinuous and a free-running float64 chain may pick other sources).
The maker asserts warm_vs_cold >= 0.5 px on every step after the first, the >= 1e-9 gap on every low it interpolates, and the restatement bit-equal to
scipy on those too."""
from __future__ import annotations

import importlib
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden_raft import S, raft_module, run_both  # noqa: E402
from make_golden_raft_warm import WARM_MIN_PX, build, maxabs, sine_field  # noqa: E402
import raft_video_restatement as R  # noqa: E402

GAP_MIN = 1e-9
NOISE = 0.05
# name: (h, w, amplitude, seed); "16x16_t" is the transposed content of "16x16_a6" (channels swapped, planes transposed)
FIELDS = {"16x16_a1": (16, 16, 1.0, 21), "16x16_a6": (16, 16, 6.0, 22), "17x19_a3": (17, 19, 3.0, 23), "28x28_a3": (28, 28, 3.0, 24),
          "40x56_a8": (40, 56, 8.0, 25)}


def noisy_field(h: int, w: int, amp: float, seed: int) -> np.ndarray:
    g = np.random.Generator(np.random.PCG64(seed + 1000))
    return (sine_field(1, h, w, seed, amp)[0] + NOISE * g.standard_normal((2, h, w))).astype(np.float32)


def checked_interpolate(ref_fi, flow: np.ndarray, name: str):
    """the reference's forward_interpolate of flow [2,h,w] float32, asserted equal to the restatement and free of ties -> (result float32, min gap)"""
    out = ref_fi(torch.from_numpy(flow)).numpy()
    assert out.dtype == np.float32 and out.shape == flow.shape
    assert np.array_equal(out, R.forward_interpolate(flow)), name  # every element, bit for bit
    gap = R.min_gap(flow)
    assert gap >= GAP_MIN, (name, gap)
    return out, gap


def main():
    torch.set_num_threads(os.cpu_count() or 1)
    rm = raft_module()
    ref_fi = importlib.import_module("cwm.models.raft.utils").forward_interpolate
    only = sys.argv[1:]
    t0 = time.time()

    def want(name):
        return not only or name in only

    if want("raft_finterp_fields"):
        fields = {k: noisy_field(*v) for k, v in FIELDS.items()}
        a = fields["16x16_a6"]
        fields["16x16_t"] = np.ascontiguousarray(np.stack([a[1].T, a[0].T]))
        out = {}
        for name, f in fields.items():
            y, gap = checked_interpolate(ref_fi, f, name)
            valid = R.landing_points(f)[2]
            changed = float((np.abs(y - f).max(axis=0) > 0).mean())
            assert 1.0 - valid.mean() >= 0.03, (name, valid.mean())
            assert changed >= 0.5, (name, changed)
            out[name + "_in"], out[name + "_out"], out[name + "_gap"] = f, y, np.array(gap)
            print(f"[golden] field {name} {f.shape} valid {100 * valid.mean():.1f} % min gap {gap:.2e} targets changed {100 * changed:.0f} %")
        np.savez_compressed(os.path.join(HERE, "raft_finterp_fields.npz"), names=np.array(sorted(fields)), **out)

    if want("raft_video_128x160_t4"):
        seed, fseed, iters, T = 18, 19, 3, 4
        m = build(rm, seed, multiframe=False)
        mf = build(rm, seed, multiframe=True)
        x = torch.from_numpy(S.raft_frames(1, 128, 160, fseed, shift=(2, -3), frames=T))
        out = {}
        for d, backward in (("fwd", False), ("bwd", True)):
            with torch.no_grad():
                cold_up = mf(x, iters=iters, backward=backward).numpy()  # [1,3,2,H,W], present order
            init, warm, drift, cold_low = None, [], [], []
            for k in range(T - 1):
                t = T - 2 - k if backward else k
                i1, i2 = (t + 1, t) if backward else (t, t + 1)

                def call(mm, dt, f):
                    xx = x.to(dt) * 255.0
                    return mm._forward_two_images(xx[:, i1], xx[:, i2], iters=iters, flow_init=None if f is None else torch.from_numpy(f).to(dt), test_mode=True)

                (low, up), dr = run_both(m, lambda mm, dt: call(mm, dt, init))
                with torch.no_grad():
                    cl, cu = (v.numpy() for v in call(m, torch.float32, None))
                at = T - 2 - t if backward else t
                assert np.array_equal(cu, cold_up[:, at])  # the cold multi-frame call is the per-pair cold calls
                cold_low.append(cl)
                warm.append(maxabs(up, cold_up[:, at]))
                drift.append(dr)
                out["%s_low_%d" % (d, k)] = low
                if init is not None:
                    out["%s_init_%d" % (d, k)] = init
                    assert warm[-1] >= WARM_MIN_PX, (d, k, warm[-1])
                if not backward:
                    out["fwd_up_%d" % k] = up
                if k + 1 < T - 1:
                    nxt, gap = checked_interpolate(ref_fi, low[0], "%s low %d" % (d, k))
                    out["%s_gap_%d" % (d, k)] = np.array(gap)
                    init = nxt[None]
            out["cold_" + d] = np.stack(cold_low, axis=1)  # [1,3,2,16,20] in chain order
            out["warm_vs_cold_" + d], out["drift_" + d] = np.array(warm), np.array(drift)
            print(f"[golden] raft_video_128x160_t4 {d} warm vs cold {warm} px drift {drift} ({time.time() - t0:.0f}s)")
        np.savez_compressed(os.path.join(HERE, "raft_video_128x160_t4.npz"), seed=np.array(seed), frames_seed=np.array(fseed), shift=np.array([2, -3]),
                            iters=np.array(iters), **out)

    limit = os.path.getsize(os.path.join(HERE, "base8_k8_b2.npz"))
    for name in ("raft_finterp_fields", "raft_video_128x160_t4"):
        p = os.path.join(HERE, name + ".npz")
        if os.path.exists(p):
            assert os.path.getsize(p) <= limit, (name, os.path.getsize(p), limit)
            print(f"[golden] {name}.npz {os.path.getsize(p)} bytes (limit {limit})")


if __name__ == "__main__":
    main()
