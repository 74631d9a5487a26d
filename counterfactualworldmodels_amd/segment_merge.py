"""Scene segmentation: many seeded Spelke segments merged into one label map (no counterpart in the reference, whose README leads with "segmenting a scene into
independently movable Spelke objects" and lists the algorithm as coming).  `segment_step.py` is the seeded half -- one seed, one object; this module makes
"objects" plural: K candidate segments per row are ranked, duplicates and parts are absorbed, empty and oversized ones dropped, overlaps resolved, and the
per-patch coverage of the result says where the next seeds belong.

The definition is the header comment of csrc/segment_merge.hip (include/cwm_hip.h `cwm_segment_merge`).  Device tensors take the library call
(`segment_merge_device`: one call, nothing read back); CPU tensors take the same definition composed in plain torch (`segment_merge_torch`).  Every output is an
integer or an integer divided by P P and each threshold test is one float32 multiply and one compare, so both give equal results.

`segment_scene` is the loop on top: rounds of seeds, each run through `FlowGenerator.segment_spelke_object`, merged after every round, the next round's seeds
drawn among the patches the merge leaves uncovered -- by the exponential race, or through `seed_select.select_seeds` spaced and on the peaks of a keypoint or
movability map."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib
from .masking import select_reveal

MAX_K, MAX_CELLS, MAX_PIXELS = 64, 4096, 1 << 18


class SegmentMergeResult:
    """labels [B,H,W] uint8 (0: no object, m = 1 .. num_labels); owner [B,K] int32 (the label of candidate k: its own if kept, its absorber's if absorbed, 0 if not
    valid); area [B,K] int32; label_area [B,K] int32 (pixels with label m at [m-1]); inter [B,K,K] int32 or None; cover [B,gh,gw] float32 (the labelled fraction of
    every patch); stats [B,4] int32 (n_valid, num_labels, labelled pixels, n_absorbed)"""
    __slots__ = ("labels", "owner", "area", "label_area", "inter", "cover", "stats")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class SceneSegmentation:
    """labels [B,H,W] uint8; num_labels [B] int32; seeds [B,K,2] int32 (y, x), (-1, -1) for a dead slot; segments [B,K,H,W] bool, the candidates in seed order;
    scores [B,K] float32; owner [B,K] int32; label_area [B,K] int32; cover [B,gh,gw] float32; stats [B,4] int32 -- K = num_rounds * num_seeds, round r in
    columns r * num_seeds .. (r + 1) * num_seeds - 1; owner, label_area, cover and stats are those of the last merge"""
    __slots__ = ("labels", "num_labels", "seeds", "segments", "scores", "owner", "label_area", "cover", "stats")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _check(B, K, H, W, P, min_area, max_area, absorb):
    """What Python must refuse before it allocates the outputs or divides by P; the library (csrc/segment_merge.hip, check_patch_grid of csrc/readout.hip) is the
    statement of the limits and refuses everything else"""
    if P not in (4, 8, 16) or H % P or W % P:
        raise ValueError("segment_merge: patches of 4, 8 or 16 pixels that divide the image, got P = %d for %d x %d" % (P, H, W))
    if not 1 <= K <= MAX_K:
        raise ValueError("segment_merge: K = %d candidates, 1 .. %d" % (K, MAX_K))
    if B < 1 or H * W > MAX_PIXELS or (H // P) * (W // P) > MAX_CELLS:
        raise ValueError("segment_merge: %d rows of %d x %d pixels, %d patches: at least one row, at most 2^18 pixels and 4096 patches" % (B, H, W, (H // P) * (W // P)))
    if min_area < 0 or max_area < 0:
        raise ValueError("segment_merge: min_area = %d, max_area = %d must not be negative" % (min_area, max_area))
    if absorb not in (0, 1):
        raise ValueError("segment_merge: absorb = %r, 0 or 1" % (absorb,))


def _planes(segments):
    """[B,K,H,W] bytes whose H x W planes are contiguous, without a copy where the tensor already is (a slice [:, :k] or [:, ::2] of a larger buffer stays a view)"""
    if segments.dim() != 4:
        raise ValueError("segment_merge: segments must be [B,K,H,W], got %s" % (tuple(segments.shape),))
    if segments.dtype not in (torch.bool, torch.uint8):
        segments = segments != 0
    W = segments.shape[-1]
    if segments.stride(-1) != 1 or segments.stride(-2) != W or segments.stride(0) < 0 or segments.stride(1) < 0:
        segments = segments.contiguous()
    return segments


def segment_merge_device(segments, scores=None, P=8, *, min_area=1, max_area=0, iou_thresh=0.5, contain_thresh=0.6, absorb=True, want_inter=False) -> SegmentMergeResult:
    """the library call on device tensors; asynchronous on the current stream"""
    _lib.require_gpu()
    segments = _planes(segments)
    B, K, H, W = segments.shape
    dev = segments.device
    if dev.type != "cuda":
        raise RuntimeError("segment_merge_device needs device tensors, got %s" % dev)
    min_area, max_area, absorb = int(min_area), int(max_area), int(absorb)
    _check(B, K, H, W, P, min_area, max_area, absorb)
    if scores is not None:
        scores = scores.to(device=dev, dtype=torch.float32).reshape(B, K).contiguous()
    gh, gw = H // P, W // P
    lib = _lib.get_lib()
    i32 = lambda *s: torch.empty(s, device=dev, dtype=torch.int32)  # noqa: E731
    r = SegmentMergeResult(labels=torch.empty((B, H, W), device=dev, dtype=torch.uint8), owner=i32(B, K), area=i32(B, K), label_area=i32(B, K),
                           inter=i32(B, K, K) if want_inter else None, cover=torch.empty((B, gh, gw), device=dev, dtype=torch.float32), stats=i32(B, 4))
    nbytes = int(lib.cwm_segment_merge_work_bytes(B, K, H, W))
    work = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    a = _lib.new_segment_merge_args()
    _lib.fill_patch_args(a.base, geometry=(B, 2, 0, H, W, P), stream=_lib.current_stream_handle(dev))
    a.K, a.segs_dev, a.scores_dev = K, segments.data_ptr(), _lib.ptr(scores)
    a.seg_strides[0], a.seg_strides[1] = segments.stride(0), segments.stride(1)
    a.min_area, a.max_area, a.iou_thresh, a.contain_thresh, a.absorb = min_area, max_area, iou_thresh, contain_thresh, absorb
    a.work_dev, a.work_bytes = work.data_ptr(), nbytes
    a.labels_dev, a.owner_dev, a.area_dev, a.label_area_dev = r.labels.data_ptr(), r.owner.data_ptr(), r.area.data_ptr(), r.label_area.data_ptr()
    a.inter_dev, a.cover_dev, a.stats_dev = _lib.ptr(r.inter), r.cover.data_ptr(), r.stats.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(lib.cwm_segment_merge(C.byref(a)))
    return r


def segment_merge_torch(segments, scores=None, P=8, *, min_area=1, max_area=0, iou_thresh=0.5, contain_thresh=0.6, absorb=True, want_inter=False) -> SegmentMergeResult:
    """the same definition in plain torch, on the tensors' own device"""
    if segments.dim() != 4:
        raise ValueError("segment_merge: segments must be [B,K,H,W], got %s" % (tuple(segments.shape),))
    seg = segments != 0
    B, K, H, W = seg.shape
    dev = seg.device
    min_area, max_area, absorb = int(min_area), int(max_area), int(absorb)
    _check(B, K, H, W, P, min_area, max_area, absorb)
    gh, gw = H // P, W // P
    flat = seg.flatten(2).to(torch.float32)
    inter = torch.bmm(flat, flat.transpose(1, 2)).to(torch.int64)  # counts of at most 2^18 ones: every partial sum is an integer below 2^24, exact in float32
    area = torch.diagonal(inter, dim1=1, dim2=2)
    valid = (area >= max(1, min_area)) & (area <= (max_area if max_area > 0 else H * W))
    score = torch.zeros((B, K), device=dev) if scores is None else scores.to(device=dev, dtype=torch.float32).reshape(B, K)
    order = select_reveal(score, valid, torch.zeros_like(valid), K)  # [B,K], -1 behind the valid candidates
    rows, slots = torch.arange(B, device=dev), torch.arange(K, device=dev)[None]
    iou_t, con_t = torch.tensor(iou_thresh, dtype=torch.float32, device=dev), torch.tensor(contain_thresh, dtype=torch.float32, device=dev)
    kept = torch.zeros((B, K), dtype=torch.int64, device=dev)  # kept[b, m - 1]: the candidate with label m
    nkept = torch.zeros((B,), dtype=torch.int64, device=dev)
    owner = torch.zeros((B, K), dtype=torch.int64, device=dev)
    keeper = torch.zeros((B, K), dtype=torch.bool, device=dev)
    for r in range(K):
        k = order[:, r]
        live, kk = k >= 0, k.clamp(min=0)
        I = inter[rows[:, None], kept, kk[:, None]]
        aj, ak = area.gather(1, kept), area.gather(1, kk[:, None]).expand(B, K)
        hit = (I.float() > iou_t * (aj + ak - I).float()) | (I.float() > con_t * torch.minimum(aj, ak).float())
        hit &= slots < nkept[:, None]
        absorbed = hit.any(1)
        first = hit.float().argmax(1)  # the first of several maxima: the first kept candidate that absorbs
        keep = live & ~absorbed
        owner[rows, kk] = torch.where(live, torch.where(absorbed, first + 1, nkept + 1), owner[rows, kk])
        keeper[rows, kk] |= keep
        at = nkept.clamp(max=K - 1)
        kept[rows, at] = torch.where(keep, kk, kept[rows, at])
        nkept = nkept + keep.to(torch.int64)
    paints = (owner > 0) & (keeper if not absorb else torch.ones_like(keeper))
    none = K + 1
    lab = torch.where(seg & paints[:, :, None, None], owner.to(torch.int16)[:, :, None, None], torch.tensor(none, dtype=torch.int16, device=dev)).amin(1)
    labels = torch.where(lab == none, torch.zeros_like(lab), lab).to(torch.uint8)
    label_area = torch.zeros((B, K + 1), dtype=torch.int64, device=dev).scatter_add_(1, labels.flatten(1).to(torch.int64), torch.ones((B, H * W), dtype=torch.int64, device=dev))[:, 1:]
    count = (labels > 0).reshape(B, gh, P, gw, P).sum((2, 4))
    n_valid = valid.sum(1)
    stats = torch.stack([n_valid, nkept, label_area.sum(1), n_valid - nkept], 1)
    return SegmentMergeResult(labels=labels, owner=owner.to(torch.int32), area=area.to(torch.int32), label_area=label_area.to(torch.int32),
                              inter=inter.to(torch.int32) if want_inter else None, cover=count.float() / float(P * P), stats=stats.to(torch.int32))


def segment_merge(segments, scores=None, P=8, **kw) -> SegmentMergeResult:
    """device tensors: the library call; CPU tensors: the torch composition"""
    return (segment_merge_device if segments.is_cuda else segment_merge_torch)(segments, scores, P, **kw)


# ---- the scene loop ---------------------------------------------------------------------------------------------------------------------------------------------
def patch_distribution(dist, B, H, W, P, device):
    """[B,n] float32 weights of the patches: None = uniform; [B,H,W] pixels are averaged to patches; [B,gh,gw] is taken as it is"""
    gh, gw = H // P, W // P
    if dist is None:
        return torch.ones((B, gh * gw), device=device, dtype=torch.float32)
    dist = torch.as_tensor(dist).to(device=device, dtype=torch.float32)
    if tuple(dist.shape) == (B, H, W):
        dist = F.avg_pool2d(dist[:, None], P)[:, 0]
    if tuple(dist.shape) != (B, gh, gw):
        raise ValueError("segment_scene: seed_distribution must be [B,H,W] or [B,gh,gw] = (%d, %d, %d) / (%d, %d, %d), got %s" % (B, H, W, B, gh, gw, tuple(dist.shape)))
    return dist.reshape(B, gh * gw)


def draw_seed_cells(p, free, k, generator=None):
    """k cells per row [B,k] int64 among the `free` ones, without replacement and in proportion to p [B,n]: the exponential race of frontier_unmask(sample=True) --
    key = p / e with e drawn from `generator`, in the order of `masking.select_reveal`; -1 where a row has fewer than k free cells"""
    e = torch.empty(p.shape, device=p.device, dtype=torch.float32).exponential_(generator=generator)
    return select_reveal(p, free, torch.zeros_like(free), k, e=e)


def cell_centres(cells, gw, P):
    """seeds [B,k,2] int32 (y, x): the centre pixel of every cell, (-1, -1) for a slot that found none"""
    c = cells.clamp(min=0)
    yx = torch.stack([torch.div(c, gw, rounding_mode="floor") * P + P // 2, (c % gw) * P + P // 2], -1)
    return torch.where((cells >= 0)[..., None], yx, torch.full_like(yx, -1)).to(torch.int32)


def seed_cells(seeds, gw, P):
    """[B,k] int32 cells of the seeds [B,k,2] (y, x), -1 for a dead slot (-1, -1); x is clamped into the image as `segment_step` clamps a seed (a y below the
    image gives a cell past the grid, which `select_seeds` ignores)"""
    cells = torch.div(seeds[..., 0], P, rounding_mode="floor") * gw + torch.div(seeds[..., 1].clamp(0, gw * P - 1), P, rounding_mode="floor")
    return torch.where(seeds[..., 0] >= 0, cells, torch.full_like(cells, -1)).to(torch.int32)


def keypoints_distribution(G, movie, power=8):
    """[B,H,W]: `G.predict_keypoints_distribution` of the first frame pair of every movie, one row at a time (as in the reference, its normalisation broadcasts
    for a single row only)"""
    return torch.cat([G.predict_keypoints_distribution(movie[b:b + 1], power=power)[:, 0] for b in range(movie.shape[0])])


def segment_scores(segment, frac, score):
    """[R] float32 scores of R segments [R,H,W] bool with their vote fractions: "votes" the mean vote fraction inside the segment, "area" the area"""
    area = segment.flatten(1).sum(1).to(torch.float32)
    if score == "area":
        return area
    if score != "votes":
        raise ValueError("segment_scene: score = %r, 'votes' or 'area'" % (score,))
    return (frac * segment).flatten(1).sum(1) / area.clamp(min=1)


def segment_scene(G, x, seeds=None, num_seeds=8, num_rounds=1, seed_distribution=None, generator=None, score="votes", seed_batch_size=None, free_below=None,
                  min_area=None, max_area_frac=0.5, iou_thresh=0.5, contain_thresh=0.6, absorb=True, seed_mode="sample", seed_radius=0, seed_rel_thresh=0.,
                  **kwargs) -> SceneSegmentation:
    """`FlowGenerator.segment_scene` (its docstring says what this does); G is the generator"""
    from .seed_select import MAX_RADIUS, select_seeds

    K, R = int(num_seeds), int(num_rounds)
    if seed_mode not in ("sample", "peaks"):
        raise ValueError("segment_scene: seed_mode = %r, 'sample' or 'peaks'" % (seed_mode,))
    seed_radius = int(seed_radius)
    if not 0 <= seed_radius <= MAX_RADIUS:
        raise ValueError("segment_scene: seed_radius = %d cells, 0 .. %d" % (seed_radius, MAX_RADIUS))
    if isinstance(seed_distribution, str):
        if seed_distribution != "keypoints":
            raise ValueError("segment_scene: seed_distribution = %r: a tensor, a callable, None or 'keypoints'" % (seed_distribution,))
        if getattr(G, "keypoint_predictor", None) is None:
            raise ValueError("segment_scene: seed_distribution = 'keypoints' needs a generator built with a keypoint_predictor")
    if K < 1 or R < 1 or K * R > MAX_K:
        raise ValueError("segment_scene: num_rounds * num_seeds = %d x %d candidates, 1 .. %d" % (R, K, MAX_K))
    if score not in ("votes", "area"):
        raise ValueError("segment_scene: score = %r, 'votes' or 'area'" % (score,))
    movie, _ = G._two_frame_movie(x, True)
    B, (H, W) = movie.shape[0], movie.shape[-2:]
    P, dev = G.patch_size[-1], movie.device
    gw = W // P
    if isinstance(seed_distribution, str):
        seed_distribution = keypoints_distribution(G, movie)
    elif callable(seed_distribution) and not torch.is_tensor(seed_distribution):
        seed_distribution = seed_distribution(movie)
    if torch.is_tensor(seed_distribution) and seed_distribution.dim() == 4 and seed_distribution.shape[1] == 1:
        seed_distribution = seed_distribution[:, 0]
    p = patch_distribution(seed_distribution, B, H, W, P, dev)
    # seed_mode="peaks" on a map of pixels: the seeds are the pixels where the cells peak, not the cells' centres
    pixels = seed_distribution.to(device=dev, dtype=torch.float32) if torch.is_tensor(seed_distribution) and tuple(seed_distribution.shape) == (B, H, W) else None
    select = seed_mode == "peaks" or seed_radius > 0  # (otherwise: the draw of draw_seed_cells, as before there was a choice)
    if seeds is not None:
        seeds = torch.as_tensor(seeds).to(device=dev, dtype=torch.int32)
        if tuple(seeds.shape) != (B, K, 2):
            raise ValueError("segment_scene: seeds must be [B,num_seeds,2] = (%d, %d, 2), got %s" % (B, K, tuple(seeds.shape)))
    merge_kw = dict(min_area=P * P if min_area is None else int(min_area), max_area=max(1, int(max_area_frac * H * W)), iou_thresh=iou_thresh,
                    contain_thresh=contain_thresh, absorb=absorb)
    segments = torch.zeros((B, R * K, H, W), device=dev, dtype=torch.bool)
    scores = torch.zeros((B, R * K), device=dev, dtype=torch.float32)
    all_seeds = torch.full((B, R * K, 2), -1, device=dev, dtype=torch.int32)
    step = int(seed_batch_size) if seed_batch_size else B * K
    rows_x = x.repeat_interleave(K, 0)  # row b K + k: movie b under seed k
    free = torch.ones_like(p, dtype=torch.bool)
    merged = None
    with torch.random.fork_rng(devices=[]):  # (the counterfactual driver draws on torch's global CPU generator; the caller's stream of draws is put back)
        for r in range(R):
            prior = seed_cells(all_seeds[:, :r * K], gw, P) if select and r > 0 else None
            if r == 0 and seeds is not None:
                rs = seeds
            elif not select:
                rs = cell_centres(draw_seed_cells(p, free, K, generator), gw, P)
            elif seed_mode == "peaks":
                rs = select_seeds(pixels if pixels is not None else p.reshape(B, H // P, gw), K, P, shape=(H, W), radius=seed_radius, peaks_only=True,
                                  rel_thresh=seed_rel_thresh, free=free, prior=prior).seeds
            else:
                e = torch.empty(p.shape, device=dev, dtype=torch.float32).exponential_(generator=generator)  # (the draw of draw_seed_cells)
                rs = select_seeds(p.reshape(B, H // P, gw), K, P, shape=(H, W), radius=seed_radius, rel_thresh=seed_rel_thresh, free=free, e=e, prior=prior).seeds
            alive = (rs[..., 0] >= 0).reshape(B * K)
            flat = rs.reshape(B * K, 2).clamp(min=0)  # (a dead slot runs on pixel (0, 0) and its segment is cleared)
            segs, sc = [], []
            for lo in range(0, B * K, step):
                seg, frac = G.segment_spelke_object(rows_x[lo:lo + step], flat[lo:lo + step], generator=generator, **kwargs)
                seg = seg & alive[lo:lo + step, None, None]
                segs.append(seg)
                sc.append(segment_scores(seg, frac, score))
            cols = slice(r * K, (r + 1) * K)
            segments[:, cols] = torch.cat(segs).reshape(B, K, H, W)
            scores[:, cols] = torch.cat(sc).reshape(B, K)
            all_seeds[:, cols] = rs
            merged = G.segment_merge(segments[:, :(r + 1) * K], scores[:, :(r + 1) * K], **merge_kw)
            free = (merged.cover.reshape(B, -1) < free_below) if free_below is not None else (merged.cover.reshape(B, -1) == 0)
    return SceneSegmentation(labels=merged.labels, num_labels=merged.stats[:, 1].contiguous(), seeds=all_seeds, segments=segments, scores=scores,
                             owner=merged.owner, label_area=merged.label_area, cover=merged.cover, stats=merged.stats)
