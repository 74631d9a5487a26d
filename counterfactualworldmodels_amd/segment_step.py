"""One step of Spelke-object segmentation (no counterpart in the reference, whose README names the use -- "asking which points would also move along with a
selected point is a way of segmenting a scene into independently movable Spelke objects" -- and lists the algorithm as coming): from the S counterfactual flows
of a seed point to the connected region that moves with it, the per-patch coverage and the active / passive patches of the next round of counterfactuals.

The definition is the header comment of csrc/segment.hip (include/cwm_hip.h `cwm_segment_step`).  Device tensors take the library call
(`segment_step_device`: three launches, nothing read back); CPU tensors take the same definition composed in plain torch (`segment_step_torch`), the component
found by bounded iterative dilation.  Both give equal results wherever the arithmetic is exact; elsewhere a compiler's contraction of u u + v v may move a
magnitude by an ulp."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib
from .flowstats import _strides5
from .masking import select_reveal

# the 8 compass shifts (dy, dx) in their fixed order: E, S, W, N, then SE, SW, NW, NE
COMPASS = ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, -1), (-1, 1))
MAX_SAMPLES, MAX_PICKS, MAX_CELLS, MAX_PIXELS = 255, 64, 4096, 1 << 18


def directions(num_samples: int, shift: int = 1):
    """`num_samples` shifts (dy, dx) of `shift` patches: COMPASS, cycled"""
    return [(COMPASS[s % 8][0] * int(shift), COMPASS[s % 8][1] * int(shift)) for s in range(int(num_samples))]


class SegmentStepResult:
    """segment [B,H,W] bool; votes [B,H,W] uint8; cover [B,gh,gw] float32; stats [B,4] int32 (n_valid, area, n_candidates, seed_hit); seed_ref [B,S] float32 (NaN: the
    sample is not valid); with k_active > 0 also active / passive [B,2n] bool (0 = active, resp. 0 = passive and visible) and picks [B,k_active+k_passive] int32
    (token n + cell, -1: the slot found no cell), else None"""
    __slots__ = ("segment", "votes", "cover", "stats", "seed_ref", "active", "passive", "picks")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _check(B, H, W, S, P, k_active, k_passive, ring_radius, init):
    """What Python must refuse before it allocates the outputs or divides by P; the library's check_patch_grid and check_segment_step (csrc/readout.hip,
    csrc/segment.hip) are the statement of the limits and refuse everything else"""
    if P not in (4, 8, 16) or H % P or W % P:
        raise ValueError("segment_step: patches of 4, 8 or 16 pixels that divide the image, got P = %d for %d x %d" % (P, H, W))
    if H * W > MAX_PIXELS or (H // P) * (W // P) > MAX_CELLS or H * ((W + 31) // 32) > 8192:
        raise ValueError("segment_step: %d x %d pixels, %d patches: at most 2^18 pixels, 8192 words of bit rows and 4096 patches" % (H, W, (H // P) * (W // P)))
    if not init and not 1 <= S <= MAX_SAMPLES:
        raise ValueError("segment_step: S = %d samples, 1 .. %d" % (S, MAX_SAMPLES))
    if not (0 <= k_active <= MAX_PICKS and 0 <= k_passive <= MAX_PICKS):
        raise ValueError("segment_step: k_active = %d, k_passive = %d, 0 .. %d each" % (k_active, k_passive, MAX_PICKS))
    if ring_radius < 1:
        raise ValueError("segment_step: ring_radius = %d, at least 1" % ring_radius)


def _dirs_tensor(dirs, S, device):
    if dirs is None:
        return None
    d = torch.as_tensor(dirs, dtype=torch.float32).to(device).reshape(-1, 2).contiguous()
    if d.shape[0] != S:
        raise ValueError("segment_step: %d directions for %d samples" % (d.shape[0], S))
    return d


def segment_step_device(flows, seeds, P, *, min_seed_mag, abs_thresh, rel_thresh=0.5, vote_frac=0.5, dirs=None, cos_min=0.0, k_active=0, k_passive=0,
                        inside_frac=1.0, ring_radius=1, keys=None, shape=None) -> SegmentStepResult:
    """the library call on device tensors; flows [B,2,H,W,S] in any strides (the `_batch_to_samples` view without a copy), or None with shape = (B, H, W): the
    init step.  Asynchronous on the current stream."""
    _lib.require_gpu()
    init = flows is None
    if init:
        B, H, W = shape
        S, dev = 0, seeds.device
    else:
        flows, strides = _strides5(flows)
        B, Cc, H, W, S = flows.shape
        dev = flows.device
        if Cc != 2:
            raise ValueError("segment_step: flow samples have 2 channels, got %d" % Cc)
    if dev.type != "cuda":
        raise RuntimeError("segment_step_device needs device tensors, got %s" % dev)
    _check(B, H, W, S, P, k_active, k_passive, ring_radius, init)
    if vote_frac != vote_frac:
        raise ValueError("segment_step: vote_frac is a NaN")
    gh, gw = H // P, W // P
    n, K = gh * gw, k_active + k_passive
    seeds = seeds.to(device=dev, dtype=torch.int32).reshape(B, 2).contiguous()
    dirs = _dirs_tensor(dirs, S, dev)
    if keys is not None:
        keys = keys.to(device=dev, dtype=torch.float32).reshape(B, 2, n).contiguous()
    sel = k_active > 0
    r = SegmentStepResult(
        segment=torch.empty((B, H, W), device=dev, dtype=torch.bool), votes=torch.empty((B, H, W), device=dev, dtype=torch.uint8),
        cover=torch.empty((B, gh, gw), device=dev, dtype=torch.float32), stats=torch.empty((B, 4), device=dev, dtype=torch.int32),
        seed_ref=torch.empty((B, S), device=dev, dtype=torch.float32),
        active=torch.empty((B, 2 * n), device=dev, dtype=torch.bool) if sel else None, passive=torch.empty((B, 2 * n), device=dev, dtype=torch.bool) if sel else None,
        picks=torch.empty((B, K), device=dev, dtype=torch.int32) if sel else None)
    a = _lib.new_segment_step_args()
    _lib.fill_patch_args(a.base, geometry=(B, 2, 0, H, W, P), stream=_lib.current_stream_handle(dev))
    if not init:
        a.flows_dev, a.C, a.S = flows.data_ptr(), 2, S
        for i in range(5):
            a.flow_strides[i] = strides[i]
    a.seeds_dev, a.dirs_dev, a.keys_dev = seeds.data_ptr(), _lib.ptr(dirs), _lib.ptr(keys)
    a.min_seed_mag, a.abs_thresh, a.rel_thresh, a.vote_frac, a.cos_min, a.inside_frac = min_seed_mag, abs_thresh, rel_thresh, vote_frac, cos_min, inside_frac
    a.k_active, a.k_passive, a.ring_radius = k_active, k_passive, ring_radius
    a.seed_ref_dev, a.votes_dev, a.segment_dev, a.cover_dev, a.stats_dev = _lib.ptr(r.seed_ref), r.votes.data_ptr(), r.segment.data_ptr(), r.cover.data_ptr(), r.stats.data_ptr()
    a.picks_dev, a.active_out_dev, a.passive_out_dev = _lib.ptr(r.picks), _lib.ptr(r.active), _lib.ptr(r.passive)
    with torch.cuda.device(dev):
        _lib.check(_lib.get_lib().cwm_segment_step(C.byref(a)))
    return r


def _select(key, eligible, k):
    """cells [B,k] int64 (-1: none left) of the eligible cells in the order of cwm_unmask_step: the higher key first, a NaN above every number, the lower index first"""
    return select_reveal(key, eligible, torch.zeros_like(eligible), k)


def segment_step_torch(flows, seeds, P, *, min_seed_mag, abs_thresh, rel_thresh=0.5, vote_frac=0.5, dirs=None, cos_min=0.0, k_active=0, k_passive=0,
                       inside_frac=1.0, ring_radius=1, keys=None, shape=None) -> SegmentStepResult:
    """the same definition in plain torch, on the tensors' own device"""
    init = flows is None
    if init:
        B, H, W = shape
        dev = seeds.device
        flows = torch.zeros((B, 2, H, W, 0), device=dev)
    flows = flows.float()
    dev = flows.device
    B, Cc, H, W, S = flows.shape
    if Cc != 2:
        raise ValueError("segment_step: flow samples have 2 channels, got %d" % Cc)
    _check(B, H, W, S, P, k_active, k_passive, ring_radius, init)
    gh, gw = H // P, W // P
    n, K = gh * gw, k_active + k_passive
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)  # noqa: E731
    seeds = seeds.to(device=dev, dtype=torch.int64).reshape(B, 2)
    sy, sx = seeds[:, 0].clamp(0, H - 1), seeds[:, 1].clamp(0, W - 1)
    cy0, cx0 = sy // P, sx // P
    c0 = cy0 * gw + cx0
    rows = torch.arange(B, device=dev)
    u, v = flows[:, 0], flows[:, 1]  # [B,H,W,S]
    m = torch.sqrt(u * u + v * v)
    acc = torch.zeros((B, S), device=dev)
    for r in range(P):  # the fixed order of the definition: row-major, one add at a time
        for c in range(P):
            acc = acc + m[rows, cy0 * P + r, cx0 * P + c]
    ref = acc / float(P * P)
    valid = ref >= f32(min_seed_mag)
    thr = torch.fmax(f32(abs_thresh), f32(rel_thresh) * ref)
    ok = (m >= thr[:, None, None]) & valid[:, None, None]
    if dirs is not None:
        d = _dirs_tensor(dirs, S, dev)
        dy, dx = d[:, 0], d[:, 1]
        ok = ok & (u * dx + v * dy >= (f32(cos_min) * m) * torch.sqrt(dx * dx + dy * dy))
    votes = ok.sum(-1).to(torch.uint8)
    n_valid = valid.sum(1)
    nf = torch.ceil(f32(vote_frac) * n_valid.float())
    need = torch.where(nf >= 256, torch.full_like(nf, 256), torch.where(nf >= 1, nf, torch.ones_like(nf))).to(torch.int64)
    cand = (votes.to(torch.int64) >= need[:, None, None]) & (n_valid > 0)[:, None, None]
    yy, xx = torch.arange(H, device=dev)[None, :, None], torch.arange(W, device=dev)[None, None, :]
    cell = (yy // P == cy0[:, None, None]) & (xx // P == cx0[:, None, None])
    reach = cand & cell
    seed_hit = reach.flatten(1).any(1)
    for _ in range(H * W + 1):  # bounded as the kernel's sweeps are: a changing pass sets at least one pixel
        grow = reach.clone()
        grow[:, 1:] |= reach[:, :-1]
        grow[:, :-1] |= reach[:, 1:]
        grow[:, :, 1:] |= reach[:, :, :-1]
        grow[:, :, :-1] |= reach[:, :, 1:]
        grow &= cand
        if torch.equal(grow, reach):
            break
        reach = grow
    count = reach.reshape(B, gh, P, gw, P).sum((2, 4))
    cover = count.float() / float(P * P)
    stats = torch.stack([n_valid, reach.flatten(1).sum(1), cand.flatten(1).sum(1), seed_hit.to(torch.int64)], 1).to(torch.int32)
    res = SegmentStepResult(segment=reach, votes=votes, cover=cover, stats=stats, seed_ref=torch.where(valid, ref, torch.full_like(ref, float("nan"))))
    if k_active <= 0:
        return res
    inside = (cover >= f32(inside_frac)).reshape(B, n)
    touched = count > 0
    R = min(int(ring_radius), max(gh, gw))
    near = F.max_pool2d(touched[:, None].float(), 2 * R + 1, stride=1, padding=R)[:, 0] > 0
    ring = (near & ~touched).reshape(B, n)
    if keys is None:
        keys = torch.zeros((B, 2, n), device=dev)
    keys = keys.to(device=dev, dtype=torch.float32).reshape(B, 2, n)
    not_seed = torch.arange(n, device=dev)[None] != c0[:, None]
    act = torch.cat([c0[:, None], _select(keys[:, 0], inside & not_seed, k_active - 1)], 1)
    pas = _select(keys[:, 1], ring, k_passive)
    masks = []
    for cells in (act, pas):
        mk = torch.ones((B, 2 * n + 1), dtype=torch.bool, device=dev)  # (one spare column takes the -1 slots)
        mk[:, :n] = False
        mk[rows[:, None], torch.where(cells >= 0, n + cells, torch.full_like(cells, 2 * n))] = False
        masks.append(mk[:, :2 * n].contiguous())
    picks = torch.cat([act, pas], 1)
    res.active, res.passive = masks
    res.picks = torch.where(picks >= 0, n + picks, picks).to(torch.int32)
    return res


def segment_step(flows, seeds, P, **kw) -> SegmentStepResult:
    """device tensors: the library call; CPU tensors: the torch composition"""
    t = seeds if flows is None else flows
    return (segment_step_device if t.is_cuda else segment_step_torch)(flows, seeds, P, **kw)
