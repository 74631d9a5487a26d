"""A numpy-only restatement of the reference's `forward_interpolate` (cwm/models/raft/utils.py:28-56) without scipy: the nearest valid landing
point by brute force in float64, statement for statement up to the `griddata(..., method='nearest')` query, which is replaced by the definition of
what it returns.  Two things the reference leaves open are fixed here, as in csrc/raft_kernels.hip `forward_interpolate_kernel`: among equal
distances the lowest source index wins (`argmin` returns the first), and a field with no valid source gives zeros.  It is the yardstick of
`tests/test_raft_video_gpu.py` for what scipy does not define, the host step of `tools/raft_step.py --warm-start`, and
`tests/golden/make_golden_raft_video.py` asserts it equal to scipy bit for bit on every field it stores."""
import numpy as np


def landing_points(flow):
    """flow [2,h,w] -> (x1 [N], y1 [N] float64, valid [N] bool), N = h * w: raft/utils.py:30-43."""
    flow = np.asarray(flow)
    dx, dy = flow[0], flow[1]
    ht, wd = dx.shape
    x0, y0 = np.meshgrid(np.arange(wd), np.arange(ht))
    with np.errstate(invalid="ignore"):
        x1 = (x0 + dx).astype(np.float64).reshape(-1)  # int64 + float32 is float64 in numpy: the sums are exact
        y1 = (y0 + dy).astype(np.float64).reshape(-1)
        valid = (x1 > 0) & (x1 < wd) & (y1 > 0) & (y1 < ht)
    return x1, y1, valid


def nearest_sources(flow, rows_per_block=512):
    """flow [2,h,w] -> (index [N] int64 of the nearest valid source of every target, -1 when there is none; gap [N] float64: the second-smallest minus
    the smallest squared distance, inf with fewer than two valid sources)."""
    x1, y1, valid = landing_points(flow)
    ht, wd = np.asarray(flow).shape[-2:]
    n = ht * wd
    gx = (np.arange(n) % wd).astype(np.float64)
    gy = (np.arange(n) // wd).astype(np.float64)
    index = np.full(n, -1, dtype=np.int64)
    gap = np.full(n, np.inf)
    if not valid.any():
        return index, gap
    sx, sy = np.where(valid, x1, 0.0), np.where(valid, y1, 0.0)
    for r0 in range(0, n, rows_per_block):
        r1 = min(n, r0 + rows_per_block)
        d2 = (gx[r0:r1, None] - sx[None, :]) ** 2 + (gy[r0:r1, None] - sy[None, :]) ** 2
        d2[:, ~valid] = np.inf
        index[r0:r1] = np.argmin(d2, axis=1)  # the first of equal minima: the lowest source index
        if n > 1:
            two = np.partition(d2, 1, axis=1)[:, :2]
            with np.errstate(invalid="ignore"):
                gap[r0:r1] = np.where(np.isinf(two[:, 1]), np.inf, two[:, 1] - two[:, 0])
    return index, gap


def forward_interpolate(flow):
    """flow [2,h,w] or [P,2,h,w] (any float dtype) -> float32 of the same shape."""
    flow = np.asarray(flow)
    if flow.ndim == 4:
        return np.stack([forward_interpolate(f) for f in flow])
    index, _ = nearest_sources(flow)
    src = flow.reshape(2, -1).astype(np.float32)
    out = np.where(index[None, :] >= 0, src[:, np.maximum(index, 0)], np.float32(0)).astype(np.float32)
    return out.reshape(flow.shape)


def min_gap(flow) -> float:
    """the smallest gap between the best and the second-best squared distance over all targets: how far the field is from a tie"""
    return float(nearest_sources(flow)[1].min())
