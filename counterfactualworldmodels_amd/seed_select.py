"""Seed selection: a score map -- `predict_keypoints_distribution`, a movability map, the patch distribution of `segment_scene` -- becomes at most k well-spaced
seed pixels per row (no counterpart in the reference, whose `sample_patches_from_energy` and `sample_and_visualize_keypoints` only ever sample and never space).
The strongest peaks first, or an exponential race in proportion to the map; both under non-maximum suppression and both excluding the neighbourhood of earlier
seeds.

The definition is the header comment of csrc/seed_select.hip (include/cwm_hip.h `cwm_seed_select`).  Device tensors take the library call
(`select_seeds_device`: one call, the map read in place where its strides allow it, nothing read back); CPU tensors take the same definition composed in plain
torch (`select_seeds_torch`).  Every output is an integer, a value of the map itself or a comparison of such values, and the two float operations (the relative
threshold's multiply, the race's division) are single correctly rounded float32 operations, so both give equal results."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib

MAX_K, MAX_CELLS, MAX_PIXELS, MAX_RADIUS, MAX_PRIOR = 64, 4096, 1 << 18, 64, 64


class SeedSelection:
    """seeds [B,k,2] int32 (y, x), (-1, -1) for a dead slot; cells [B,k] int32, -1 for a dead slot; values [B,k] float32 (v of the picked cell, 0 for a dead
    slot); pooled [B,gh,gw] float32 (v); peaks [B,gh,gw] bool (step 4 of the definition, whether peaks_only was set or not); stats [B,4] int32 (free non-NaN
    cells, candidates, picks made, 0)"""
    __slots__ = ("seeds", "cells", "values", "pooled", "peaks", "stats")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _prepare(map, k, P, radius, peaks_only, abs_thresh, rel_thresh, free, e, prior, shape, cells):
    """The checks both paths share (the library, csrc/seed_select.hip, is the statement of the limits and refuses everything else) and the inputs in their
    canonical shapes: (map [B,H,W] or [B,gh,gw] float32, cells flag, B, H, W, free [B,n] bool or None, e [B,n] float32 or None, prior [B,q] int32 or None)"""
    if P not in (4, 8, 16):
        raise ValueError("select_seeds: patches of 4, 8 or 16 pixels, got P = %r" % (P,))
    m = torch.as_tensor(map)
    if m.dim() == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.dim() != 3:
        raise ValueError("select_seeds: map must be [B,H,W] pixels or [B,gh,gw] cells ([B,1,.,.] is squeezed), got %s" % (tuple(m.shape),))
    if m.dtype != torch.float32:
        m = m.to(torch.float32)
    B, a, b = m.shape
    if shape is not None:
        H, W = int(shape[0]), int(shape[1])
        if H <= 0 or W <= 0 or H % P or W % P:
            raise ValueError("select_seeds: patches of %d pixels do not divide shape = %d x %d" % (P, H, W))
        as_pixels, as_cells = (a, b) == (H, W), (a, b) == (H // P, W // P)
        if as_pixels and as_cells:
            raise ValueError("select_seeds: a %d x %d map is both the pixels and the cells of shape = %d x %d" % (a, b, H, W))
        if not (as_pixels or as_cells) or (cells is not None and bool(cells) != as_cells):
            raise ValueError("select_seeds: map must be [B,H,W] = (%d, %d, %d) pixels or [B,gh,gw] = (%d, %d, %d) cells, got %s%s" % (
                B, H, W, B, H // P, W // P, tuple(m.shape), "" if cells is None else " with cells = %r" % (cells,)))
        cells = as_cells
    else:
        cells = bool(cells)
        H, W = (a * P, b * P) if cells else (a, b)
        if H % P or W % P:
            raise ValueError("select_seeds: patches of %d pixels do not divide the %d x %d map (a map of cells: pass cells=True or shape=(H, W))" % (P, H, W))
    n = (H // P) * (W // P)
    if B < 1 or H * W > MAX_PIXELS or n > MAX_CELLS:
        raise ValueError("select_seeds: %d rows of %d x %d pixels, %d patches: at least one row, at most 2^18 pixels and 4096 patches" % (B, H, W, n))
    if not 1 <= int(k) <= MAX_K:
        raise ValueError("select_seeds: k = %r seeds, 1 .. %d" % (k, MAX_K))
    if not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError("select_seeds: radius = %r cells, 0 .. %d" % (radius, MAX_RADIUS))
    if abs_thresh != abs_thresh:
        raise ValueError("select_seeds: abs_thresh must not be a NaN (-inf disables it)")
    if rel_thresh != rel_thresh or rel_thresh in (float("inf"), float("-inf")):
        raise ValueError("select_seeds: rel_thresh = %r must be finite (<= 0 disables it)" % (rel_thresh,))
    dev = m.device
    if free is not None:
        free = torch.as_tensor(free).to(device=dev)
        if free.numel() != B * n:
            raise ValueError("select_seeds: free must hold [B,n] = (%d, %d) cells, got %s" % (B, n, tuple(free.shape)))
        free = (free != 0).reshape(B, n).contiguous()
    if e is not None:
        e = torch.as_tensor(e).to(device=dev, dtype=torch.float32)
        if e.numel() != B * n:
            raise ValueError("select_seeds: e must hold [B,n] = (%d, %d) draws, got %s" % (B, n, tuple(e.shape)))
        e = e.reshape(B, n).contiguous()
    if prior is not None:
        prior = torch.as_tensor(prior).to(device=dev, dtype=torch.int32)
        if prior.dim() != 2 or prior.shape[0] != B or prior.shape[1] > MAX_PRIOR:
            raise ValueError("select_seeds: prior must be [B,q] cells of earlier seeds with q <= %d, got %s" % (MAX_PRIOR, tuple(prior.shape)))
        prior = prior.contiguous() if prior.shape[1] else None
    return m, cells, B, H, W, free, e, prior


def select_seeds_device(map, k, P, *, radius=1, peaks_only=False, abs_thresh=float("-inf"), rel_thresh=0., free=None, e=None, prior=None, shape=None,
                        cells=None) -> SeedSelection:
    """the library call on device tensors; asynchronous on the current stream"""
    _lib.require_gpu()
    m, cells, B, H, W, free, e, prior = _prepare(map, k, P, radius, peaks_only, abs_thresh, rel_thresh, free, e, prior, shape, cells)
    dev = m.device
    if dev.type != "cuda":
        raise RuntimeError("select_seeds_device needs device tensors, got %s" % dev)
    k = int(k)
    gh, gw = H // P, W // P
    if cells:
        m = m.contiguous()
    elif m.stride(2) != 1 or m.stride(1) < W or m.stride(0) < 0:  # (a channel of [B,C,H,W] or a padded buffer is read in place)
        m = m.contiguous()
    lib = _lib.get_lib()
    i32 = lambda *s: torch.empty(s, device=dev, dtype=torch.int32)  # noqa: E731
    r = SeedSelection(seeds=i32(B, k, 2), cells=i32(B, k), values=torch.empty((B, k), device=dev, dtype=torch.float32),
                      pooled=torch.empty((B, gh, gw), device=dev, dtype=torch.float32), peaks=torch.empty((B, gh, gw), device=dev, dtype=torch.bool), stats=i32(B, 4))
    a = _lib.new_seed_select_args()
    _lib.fill_patch_args(a.base, geometry=(B, 1, 0, H, W, P), stream=_lib.current_stream_handle(dev))
    a.map_dev, a.cells = m.data_ptr(), int(cells)
    work = None
    if not cells:
        a.map_strides[0], a.map_strides[1] = m.stride(0), m.stride(1)
        nbytes = int(lib.cwm_seed_select_work_bytes(B, H, W, P))
        work = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
        a.work_dev, a.work_bytes = work.data_ptr(), nbytes
    a.free_dev, a.e_dev, a.prior_dev, a.n_prior = _lib.ptr(free), _lib.ptr(e), _lib.ptr(prior), 0 if prior is None else prior.shape[1]
    a.K, a.radius, a.peaks_only, a.abs_thresh, a.rel_thresh = k, int(radius), int(bool(peaks_only)), abs_thresh, rel_thresh
    a.seeds_dev, a.cells_dev, a.values_dev = r.seeds.data_ptr(), r.cells.data_ptr(), r.values.data_ptr()
    a.pooled_dev, a.peaks_dev, a.stats_dev = r.pooled.data_ptr(), r.peaks.data_ptr(), r.stats.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(lib.cwm_seed_select(C.byref(a)))
    return r


def key_order(v):
    """csrc/select_order.h um_order as int64 [..]: orders float32 keys as torch.sort(descending=True) does -- a NaN above every number, -0 equal to +0"""
    v = torch.where(v == 0, torch.zeros_like(v), v)
    u = v.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = torch.where(u >= 0x80000000, u ^ 0xFFFFFFFF, u | 0x80000000)
    return torch.where(torch.isnan(v), torch.full_like(u, 0xFFFFFFFF), u)


def select_seeds_torch(map, k, P, *, radius=1, peaks_only=False, abs_thresh=float("-inf"), rel_thresh=0., free=None, e=None, prior=None, shape=None,
                       cells=None) -> SeedSelection:
    """the same definition in plain torch, on the tensors' own device: rank words as exact integers (below 2^45, so also exact in the float64 the windowed
    maximum runs in), K vectorised rounds"""
    m, cells, B, H, W, free, e, prior = _prepare(map, k, P, radius, peaks_only, abs_thresh, rel_thresh, free, e, prior, shape, cells)
    dev, k, r = m.device, int(k), int(radius)
    gh, gw = H // P, W // P
    n = gh * gw
    idx = torch.arange(n, device=dev)
    cy, cx = torch.div(idx, gw, rounding_mode="floor"), idx % gw
    # 1 pool
    if cells:
        v = m.reshape(B, n)
        sy, sx = (cy * P + P // 2).expand(B, n), (cx * P + P // 2).expand(B, n)
    else:
        px = m.reshape(B, gh, P, gw, P).permute(0, 1, 3, 2, 4).reshape(B, n, P * P)
        word = torch.where(torch.isnan(px), torch.zeros((), dtype=torch.int64, device=dev), key_order(px) * 256 + (255 - torch.arange(P * P, device=dev)))
        best = word.max(2).values
        o = torch.where(best > 0, 255 - (best & 255), torch.zeros_like(best))
        v = torch.where(best > 0, px.gather(2, o[..., None])[..., 0], torch.full((), float("nan"), device=dev))
        sy, sx = cy * P + torch.div(o, P, rounding_mode="floor"), cx * P + o % P
    number = ~torch.isnan(v)
    # 2, 3 the row maximum and the threshold
    has = number.any(1)
    top = torch.where(number, v, torch.full((), float("-inf"), device=dev)).amax(1)
    t = torch.full((B,), abs_thresh, dtype=torch.float32, device=dev)
    if rel_thresh > 0:
        t = torch.maximum(t, torch.tensor(rel_thresh, dtype=torch.float32, device=dev) * top)
    # 4 peaks: the separable windowed maximum of (um_order(v), the lower index higher)
    word = torch.where(number, key_order(v) * MAX_CELLS + (MAX_CELLS - 1 - idx), torch.zeros((), dtype=torch.int64, device=dev))
    wmax = word.to(torch.float64).reshape(B, 1, gh, gw)
    for lo in range(0, r, 32):  # (max_pool2d pads by at most half its window: windows of up to 65 cells, composed)
        s = min(32, r - lo)
        wmax = F.max_pool2d(F.max_pool2d(wmax, (1, 2 * s + 1), 1, (0, s)), (2 * s + 1, 1), 1, (s, 0))
    peaks = number & (wmax.reshape(B, n) == word.to(torch.float64))
    # 5 candidates
    cand = has[:, None] & number & (v >= t[:, None])
    if free is not None:
        cand &= free
    n_free = (number & free).sum(1) if free is not None else number.sum(1)
    if peaks_only:
        cand &= peaks
    if prior is not None:
        q = prior.to(torch.int64)
        ok = (q >= 0) & (q < n)
        q = q.clamp(0, n - 1)
        near = ((cy[None, None] - cy[q][..., None]).abs() <= r) & ((cx[None, None] - cx[q][..., None]).abs() <= r) & ok[..., None]
        cand &= ~near.any(1)
    # 6 key, 7 selection
    key = v if e is None else v.clamp(min=0) / e
    comp = torch.where(cand, (1 << 44) + key_order(key) * MAX_CELLS + (MAX_CELLS - 1 - idx), torch.zeros((), dtype=torch.int64, device=dev))
    n_cand = cand.sum(1)
    out_cells = torch.full((B, k), -1, dtype=torch.int64, device=dev)
    for rd in range(k):
        best, c = comp.max(1)
        live = best > 0
        out_cells[:, rd] = torch.where(live, c, torch.full_like(c, -1))
        window = ((cy[None] - cy[c][:, None]).abs() <= r) & ((cx[None] - cx[c][:, None]).abs() <= r) & live[:, None]
        comp = torch.where(window, torch.zeros_like(comp), comp)
    live = out_cells >= 0
    c = out_cells.clamp(min=0)
    seeds = torch.where(live[..., None], torch.stack([sy.expand(B, n).gather(1, c), sx.expand(B, n).gather(1, c)], -1), torch.full((), -1, dtype=torch.int64, device=dev))
    values = torch.where(live, v.gather(1, c), torch.zeros((), device=dev))
    stats = torch.stack([n_free, n_cand, live.sum(1), torch.zeros_like(n_cand)], 1)
    return SeedSelection(seeds=seeds.to(torch.int32), cells=out_cells.to(torch.int32), values=values, pooled=v.reshape(B, gh, gw).clone(), peaks=peaks.reshape(B, gh, gw),
                         stats=stats.to(torch.int32))


def select_seeds(map, k, P, **kw) -> SeedSelection:
    """At most k well-spaced seeds per row of a score map: [B,H,W] is a map of pixels (a seed is the pixel where its cell peaks), [B,gh,gw] one of cells (a seed
    is its cell's centre); [B,1,.,.] is squeezed.  Which of the two a map is follows from shape=(H, W) when given, else from cells=True / False (default: pixels).
    radius (Chebyshev, in cells) spaces the picks, is the window of the peak test and the reach of the `prior` cells [B,q] of earlier seeds (-1: none);
    peaks_only keeps the local maxima alone; abs_thresh / rel_thresh (a fraction of the row's maximum) drop weak cells; `free` [B,n] keeps candidates to its
    nonzero cells; `e` [B,n] (positive draws, torch.empty(..).exponential_()) makes it the exponential race key = max(v, 0) / e of `frontier_unmask(sample=True)`
    in place of the strongest first.  Device tensors: the library call; CPU tensors: the torch composition.  Returns a `SeedSelection`."""
    return (select_seeds_device if torch.as_tensor(map).is_cuda else select_seeds_torch)(map, k, P, **kw)
