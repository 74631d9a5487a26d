"""The contract of `cwm_unmask_step` (include/cwm_hip.h) restated in plain torch on the CPU, written from the header's text and not from the kernel: the
distance by brute force over every (cell, visible cell) pair in fp32 as the reference divides, the selection by an explicit sort of (class, key, index)
tuples.  Shared by the CPU and GPU tests; nothing here loads the native library."""
from __future__ import annotations

import functools
import math

import torch


def threshold(h, w, radius):
    """the reference's `r * radius` (masking.py:66-67) as the float32 comparison sees it; -1: no restriction"""
    if radius is None:
        return -1.0
    return float(torch.tensor((1 / ((min(h, w) - 1) // 2)) * radius, dtype=torch.float32))


@functools.lru_cache(maxsize=4)
def _pairs(h, w):
    """max(|dy| / sy, |dx| / sx) of every (cell, cell) pair, fp32 divisions"""
    n = h * w
    sy, sx = float((h - 1) // 2), float((w - 1) // 2)
    ys = (torch.arange(n) // w).float()
    xs = (torch.arange(n) % w).float()
    return torch.maximum((ys[:, None] - ys[None, :]).abs() / sy, (xs[:, None] - xs[None, :]).abs() / sx)


def distance(frame_mask, h, w, self_mask=False):
    """frame_mask [B, h*w] bool -> d [B, h*w] float32: min over the visible cells of max(|dy| / sy, |dx| / sx), every quotient an fp32 division; zeros for a
    row without a visible cell; self_mask: the visible cells get the row's maximum"""
    B, n = frame_mask.shape
    pair = _pairs(h, w)  # [cell, visible cell]
    out = torch.zeros((B, n), dtype=torch.float32)
    for b in range(B):
        vis = ~frame_mask[b]
        if vis.any():
            d = pair[:, vis].amin(1)
            if self_mask:
                d = torch.where(vis, d.amax(), d)
            out[b] = d
    return out


def frontier(frame_mask, h, w, thr):
    """masked cells with d <= thr (thr < 0: every masked cell)"""
    if thr < 0:
        return frame_mask.clone()
    return frame_mask & (distance(frame_mask, h, w) <= thr)


def _rank(v):
    """sort key of an fp32 value, descending with NaN first and -0 == +0"""
    if math.isnan(v):
        return (0, 0.0)
    return (1, -(v + 0.0))


def select(err, frame_mask, front, k, e=None):
    """err [B,n] float32 (the cell's error, region weight applied), frame_mask / front [B,n] bool, e [B,n] or None -> cells [B,k] int64, -1 where the row has
    run out of masked cells: frontier cells before the other masked cells, the higher key first (NaN above every number), the lower index first"""
    B, n = err.shape
    key = err if e is None else torch.where(torch.isnan(err), err, err.clamp(min=0) / e)
    out = torch.full((B, k), -1, dtype=torch.int64)
    for b in range(B):
        cells = [c for c in range(n) if bool(frame_mask[b, c])]
        cells.sort(key=lambda c: (0 if bool(front[b, c]) else 1,) + _rank(float(key[b, c])) + (c,))
        for r, c in enumerate(cells[:k]):
            out[b, r] = c
    return out


def step(mask, err_map, T, h, w, frame, k, thr, e=None, region=None):
    """one whole call on CPU tensors: mask [B,Nt] bool, err_map [B,T,h,w] -> dict(dist, frontier, picks, mask_out); picks are token indices"""
    B = mask.shape[0]
    n = h * w
    fm = mask[:, frame * n:(frame + 1) * n]
    front = frontier(fm, h, w, thr)
    out = {"dist": distance(fm, h, w), "frontier": front.to(torch.uint8)}
    if k > 0:
        err = err_map[:, frame].reshape(B, n)
        if region is not None:
            err = err * region[:, frame].reshape(B, n)
        cells = select(err, fm, front, k, e)
        picks = torch.where(cells >= 0, cells + frame * n, cells)
        mask_out = mask.clone()
        for b in range(B):
            for c in picks[b].tolist():
                if c >= 0:
                    mask_out[b, c] = False
        out.update(picks=picks.to(torch.int32), mask_out=mask_out)
    return out
