"""Ego-motion counterfactuals read out as motion parallax (no counterpart in the reference, whose README lists "using counterfactuals to estimate other scene
properties" as coming).  Every other stage of the chain asks about objects moving in a fixed view; this one asks what the scene shows when the VIEWER moves:
under a translation of the viewer near things sweep across the image faster than far ones.  `ego_motion_flows` (`FlowGenerator.ego_motion_flows`) makes S flow
samples of one scene under S motions of the viewer -- a pan of anchored patches, or S head motions given to an IMU-conditioned predictor --, `measure` reduces
them to a parallax map (per pixel the motion along a reference motion as a multiple of it, the lower median over the samples, with its interquartile range and
the motion across the reference) and, with a slot map, to a histogram and a table of order statistics per slot; `depth_order` turns the table into who is
nearer than whom, and `agreement` sets that against the occlusion order of `object_motion.occlusion_order`, the project's other ordinal depth cue.  A pure
rotation of the viewer moves every pixel alike: the map is flat and `depth_order` stays silent.

The definition is the comment of `cwm_parallax` in include/cwm_hip.h: seven numbered steps, integer sums and correctly rounded float64 operations in a stated
order, a stable order where values tie.  Device tensors take the library call (`measure_device`: allocates the outputs, one call, nothing read back); CPU
tensors take the same definition in plain torch ops in that order (`measure_torch`), which equals the device bit for bit.  Whether a particular checkpoint
answers a pan or a head motion with depth-dependent flow has not been measured: the read-out is defined on flows."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib

SLOTS, BINS, MAX_PIXELS, MAX_SAMPLES, MAX_ROWS, MAX_REF_Q, MAX_DIR = 64, 256, 1 << 18, 64, 65535, 1 << 21, 4096
_SIDE = SLOTS + 1
REF_FIELDS = ("mu", "mv", "den", "live")
SLOT_FIELDS = ("n", "n_bad", "b_med", "b_q1", "b_q3", "b_min", "b_max", "zero")


class Parallax:
    """par, spread, off float32 [B,H,W] (the lower median over the samples of the motion along the reference motion, in units of that motion; the interquartile
    range of the same values; the lower median of the motion across it; NaN where fewer than min_samples samples count; spread / off None when not asked for);
    cnt uint8 [B,H,W] (the samples that count); ref float64 [B,S,4] (REF_FIELDS: the reference motion of each sample in 1/256 px, its squared length, 1.0 if
    the sample is live); with labels hist int32 [B,65,256] (pixels per slot and bin; a bin is 1/32 wide, bin 128 starts at 0) and slot_tab int32 [B,65,8]
    (SLOT_FIELDS: pixels with and without a parallax, the bins of the median, the quartiles, the minimum and the maximum, -1 for an empty slot), else None;
    `dirs` is the int32 [S,2] (dy, dx) tensor the call was made with, or None.  `FlowGenerator.parallax` also fills nearer and rank of `depth_order`"""
    __slots__ = ("par", "spread", "off", "cnt", "ref", "hist", "slot_tab", "dirs", "nearer", "rank")

    def __init__(self, par, spread, off, cnt, ref, hist, slot_tab, dirs=None, nearer=None, rank=None):
        self.par, self.spread, self.off, self.cnt, self.ref, self.hist, self.slot_tab, self.dirs = par, spread, off, cnt, ref, hist, slot_tab, dirs
        self.nearer, self.rank = nearer, rank


def _shape(t):
    return tuple(t.shape) if torch.is_tensor(t) else type(t)


def min_ref_q_of(min_ref) -> int:
    """the smallest reference motion in 1/256 px that the library takes"""
    return int(round(float(min_ref) * 256.0))


def _prepare(flows, dirs, labels, ref_slot, min_pixels, min_ref, min_samples):
    """What Python must refuse before it allocates the outputs; the library (csrc/parallax.hip) is the statement of the limits.  Returns the flows as a
    [B,2,H,W,S] float32 view in whatever strides they have, dirs int32 [S,2] or None, the maps as a [B,H,W] view with contiguous planes or None, and the
    checked scalars"""
    if not torch.is_tensor(flows) or flows.dim() != 5 or flows.shape[1] != 2:
        raise ValueError("parallax: flows must be [B,2,H,W,S], got %s" % (_shape(flows),))
    B, _, H, W, S = flows.shape
    if not 1 <= B <= MAX_ROWS:
        raise ValueError("parallax: flows of %d rows, 1 .. %d" % (B, MAX_ROWS))
    if H <= 0 or W <= 0 or H % 4 or W % 4 or H * W > MAX_PIXELS:
        raise ValueError("parallax: flows of H x W = %d x %d pixels: H and W positive multiples of 4, at most 2^18 pixels" % (H, W))
    if not 1 <= S <= MAX_SAMPLES:
        raise ValueError("parallax: S = %d samples, 1 .. %d" % (S, MAX_SAMPLES))
    dev = flows.device
    f = flows.to(torch.float32)
    if min(f.stride()) < 0:
        f = f.contiguous()
    if dirs is not None:
        dirs = torch.as_tensor(dirs)
        if dirs.numel() != 2 * S or dirs.is_floating_point() and not bool((dirs == dirs.round()).all()):
            raise ValueError("parallax: dirs must be [S,2] = (%d, 2) whole pixels (dy, dx), got %s" % (S, _shape(dirs)))
        if not dirs.is_cuda and bool((dirs.abs() > MAX_DIR).any()):  # (entries already on the device are not read back: the library states the limit)
            raise ValueError("parallax: dirs entries must be at most %d pixels in magnitude" % MAX_DIR)
        dirs = dirs.to(device=dev, dtype=torch.int32).reshape(S, 2).contiguous()
    if labels is not None:
        if not torch.is_tensor(labels) or tuple(labels.shape) != (B, H, W):
            raise ValueError("parallax: labels must be [B,H,W] = (%d, %d, %d), got %s" % (B, H, W, _shape(labels)))
        if labels.dtype == torch.bool:
            labels = labels.view(torch.uint8)
        if labels.dtype != torch.uint8:
            raise ValueError("parallax: labels must be uint8, got %s" % (labels.dtype,))
        if labels.device != dev:
            raise ValueError("parallax: flows are on %s and labels on %s" % (dev, labels.device))
        if labels.stride(-1) != 1 or labels.stride(-2) != W or labels.stride(0) < 0:
            labels = labels.contiguous()
    ref_slot, min_pixels, min_ref = int(ref_slot), int(min_pixels), float(min_ref)
    if not -1 <= ref_slot <= SLOTS or (ref_slot >= 0 and labels is None):
        raise ValueError("parallax: ref_slot = %d: -1, or 0 .. %d together with labels" % (ref_slot, SLOTS))
    if min_pixels < 1:
        raise ValueError("parallax: min_pixels = %d, at least 1" % min_pixels)
    if not math.isfinite(min_ref) or not 1 <= min_ref_q_of(min_ref) <= MAX_REF_Q:
        raise ValueError("parallax: min_ref = %r px, 1/256 .. 8192" % min_ref)
    min_samples = (S + 1) // 2 if min_samples is None else int(min_samples)
    if not 1 <= min_samples <= S:
        raise ValueError("parallax: min_samples = %d, 1 .. S = %d" % (min_samples, S))
    return f, dirs, labels, (B, H, W, S), ref_slot, min_pixels, min_ref_q_of(min_ref), min_samples


def measure_device(flows, dirs=None, labels=None, ref_slot=-1, min_pixels=1, min_ref=0.25, min_samples=None, want_spread=True, want_off=True) -> Parallax:
    """the library call on device tensors; asynchronous on the current stream, nothing is read back"""
    _lib.require_gpu()
    f, dirs, lab, (B, H, W, S), ref_slot, min_pixels, min_ref_q, min_samples = _prepare(flows, dirs, labels, ref_slot, min_pixels, min_ref, min_samples)
    dev = f.device
    if dev.type != "cuda":
        raise RuntimeError("measure_device needs device tensors")
    new = lambda shape, dtype: torch.empty((B,) + shape, device=dev, dtype=dtype)  # noqa: E731
    r = Parallax(new((H, W), torch.float32), new((H, W), torch.float32) if want_spread else None, new((H, W), torch.float32) if want_off else None,
                 new((H, W), torch.uint8), new((S, 4), torch.float64), new((_SIDE, BINS), torch.int32) if lab is not None else None,
                 new((_SIDE, 8), torch.int32) if lab is not None else None, dirs)
    a = _lib.new_parallax_args()
    _lib.fill_patch_args(a.base, geometry=(B, 1, 0, H, W, 0), stream=_lib.current_stream_handle(dev))
    a.flows_dev, a.S = f.data_ptr(), S
    for i in range(5):
        a.flow_strides[i] = f.stride(i)
    a.dirs_dev, a.labels_dev, a.labels_stride = _lib.ptr(dirs), _lib.ptr(lab), lab.stride(0) if lab is not None else 0
    a.ref_slot, a.min_pixels, a.min_ref_q, a.min_samples = ref_slot, min_pixels, min_ref_q, min_samples
    a.par_dev, a.spread_dev, a.off_dev, a.cnt_dev, a.ref_dev, a.hist_dev, a.slot_tab_dev = (_lib.ptr(t) for t in (r.par, r.spread, r.off, r.cnt, r.ref, r.hist, r.slot_tab))
    with torch.cuda.device(dev):
        _lib.check(_lib.get_lib().cwm_parallax(C.byref(a)))
    return r


def _order_statistics(vals, ok, n, ks):
    """the entries of rank k (each [B,H,W]) of the values that count, in the stable ascending order: what does not count is put last as +inf"""
    ordered = torch.sort(torch.where(ok, vals, torch.full_like(vals, float("inf"))), dim=-1, stable=True).values
    return [ordered.gather(-1, k[..., None])[..., 0] for k in ks]


def measure_torch(flows, dirs=None, labels=None, ref_slot=-1, min_pixels=1, min_ref=0.25, min_samples=None, want_spread=True, want_off=True) -> Parallax:
    """the same definition in plain torch, on the tensors' own device"""
    f, dirs, lab, (B, H, W, S), ref_slot, min_pixels, min_ref_q, min_samples = _prepare(flows, dirs, labels, ref_slot, min_pixels, min_ref, min_samples)
    dev, i64, f64 = f.device, torch.int64, torch.float64
    # 1 usable, 2 quantise
    u, v = f[:, 0], f[:, 1]  # [B,H,W,S]
    usable = (u.abs() <= 4096.0) & (v.abs() <= 4096.0)
    zf = torch.zeros_like(u)
    qu = torch.round(torch.where(usable, u, zf) * 256.0).to(i64)
    qv = torch.round(torch.where(usable, v, zf) * 256.0).to(i64)
    l = None
    if lab is not None:
        l = lab.to(i64)
        l = torch.where(l > SLOTS, torch.zeros_like(l), l)
    # 3 reference motion
    if dirs is not None:
        mu = (256 * dirs[:, 1].to(i64)).to(f64)[None].expand(B, S)
        mv = (256 * dirs[:, 0].to(i64)).to(f64)[None].expand(B, S)
        N = torch.full((B, S), H * W, dtype=i64, device=dev)
    else:
        member = usable if ref_slot < 0 else usable & (l == ref_slot)[..., None]
        zi = torch.zeros_like(qu)
        SU, SV, N = torch.where(member, qu, zi).sum((1, 2)), torch.where(member, qv, zi).sum((1, 2)), member.sum((1, 2))
        some = N > 0
        Nd = torch.where(some, N, torch.ones_like(N)).to(f64)
        zero = torch.zeros((B, S), dtype=f64, device=dev)
        mu, mv = torch.where(some, SU.to(f64) / Nd, zero), torch.where(some, SV.to(f64) / Nd, zero)
    uu, vv = mu * mu, mv * mv
    den = uu + vv
    live = (N >= min_pixels) & (den >= float(min_ref_q) * float(min_ref_q))
    ref = torch.stack([mu, mv, den, live.to(f64)], -1)
    # 4 projection
    ok = usable & live[:, None, None, :]
    mub, mvb = mu[:, None, None, :], mv[:, None, None, :]
    denb = torch.where(live, den, torch.ones_like(den))[:, None, None, :]
    fu, fv = qu.to(f64), qv.to(f64)
    a, b = fu * mub, fv * mvb
    p = (a + b) / denb
    # 5 order statistics
    n = ok.sum(-1)
    good = n >= min_samples
    m1 = (n - 1).clamp(min=0)
    k1, k2, k3 = m1 // 4, m1 // 2, (3 * m1) // 4
    q1, med, q3 = _order_statistics(p, ok, n, (k1, k2, k3))
    nan32 = torch.full((B, H, W), float("nan"), dtype=torch.float32, device=dev)
    zd = torch.zeros_like(med)
    med, q1, q3 = torch.where(good, med, zd), torch.where(good, q1, zd), torch.where(good, q3, zd)
    par = torch.where(good, med.to(torch.float32), nan32)
    spread = torch.where(good, (q3 - q1).to(torch.float32), nan32) if want_spread else None
    off = None
    if want_off:
        a, b = fu * mvb, fv * mub
        c = (a - b).abs() / denb
        cmed, = _order_statistics(c, ok, n, (k2,))
        off = torch.where(good, torch.where(good, cmed, zd).to(torch.float32), nan32)
    cnt = n.to(torch.uint8)
    hist = slot_tab = None
    if l is not None:
        # 6 histogram
        bins = (torch.floor(med * 32.0) + 128.0).clamp(0.0, 255.0).to(i64)
        cell = torch.arange(B, device=dev)[:, None, None] * _SIDE + l
        hist = torch.zeros(B * _SIDE * BINS, dtype=i64, device=dev).scatter_add_(0, (cell * BINS + bins).reshape(-1), good.to(i64).reshape(-1)).reshape(B, _SIDE, BINS)
        bad = torch.zeros(B * _SIDE, dtype=i64, device=dev).scatter_add_(0, cell.reshape(-1), (~good).to(i64).reshape(-1)).reshape(B, _SIDE)
        # 7 slot table: the lowest bin whose cumulative count exceeds k is the number of bins whose cumulative count does not
        cum = hist.cumsum(-1)
        ns = cum[..., -1]
        s1 = (ns - 1).clamp(min=0)
        bin_of = lambda k: (cum <= k[..., None]).sum(-1)  # noqa: E731
        cols = [bin_of(s1 // 2), bin_of(s1 // 4), bin_of((3 * s1) // 4), bin_of(torch.zeros_like(ns)), (cum < ns[..., None]).sum(-1)]
        none = torch.full_like(ns, -1)
        cols = [torch.where(ns > 0, c, none) for c in cols]
        slot_tab = torch.stack([ns, bad] + cols + [torch.zeros_like(ns)], -1).to(torch.int32)
        hist = hist.to(torch.int32)
    return Parallax(par, spread, off, cnt, ref, hist, slot_tab, dirs)


def measure(flows, dirs=None, labels=None, ref_slot=-1, min_pixels=1, min_ref=0.25, min_samples=None, want_spread=True, want_off=True) -> Parallax:
    """`flows` ([B,2,H,W,S]: S flow samples of each scene under S motions of the viewer, channel 0 horizontal, in pixels, in any strides -- the
    `_batch_to_samples` view is read in place), `dirs` ([S,2] whole pixels (dy, dx): the image motion each sample was asked for, which is then the reference
    motion; None: every sample is measured against its own mean flow over the row -- with `ref_slot` >= 0 over the pixels of that slot of `labels` only, e.g.
    0 for the background) and `labels` ([B,H,W] uint8 slots; with them the per-slot histogram and table are filled).  A sample is live if its reference motion
    rests on at least min_pixels pixels and is at least min_ref pixels long; a pixel has a parallax if at least min_samples (default (S + 1) // 2) of its samples
    are live and usable.  Device tensors: the library call; CPU tensors: the torch composition"""
    fn = measure_device if torch.is_tensor(flows) and flows.is_cuda else measure_torch
    return fn(flows, dirs=dirs, labels=labels, ref_slot=ref_slot, min_pixels=min_pixels, min_ref=min_ref, min_samples=min_samples, want_spread=want_spread,
              want_off=want_off)


# ---- host decisions: plain integer / bool torch on the tables' own device, in the manner of object_motion.occlusion_order ----
def _check_tab(who, slot_tab):
    if not torch.is_tensor(slot_tab) or slot_tab.dim() < 2 or tuple(slot_tab.shape[-2:]) != (_SIDE, 8) or slot_tab.is_floating_point():
        raise ValueError("%s: slot_tab must be an integer [..,65,8] table, got %s" % (who, _shape(slot_tab)))


def slot_values(slot_tab):
    """float32 [..,65,5]: the parallax at the centre of the bins b_med, b_q1, b_q3, b_min, b_max of every slot, (b - 127.5) / 32, NaN for -1 (an empty slot)"""
    _check_tab("slot_values", slot_tab)
    b = slot_tab[..., 2:7]
    return torch.where(b >= 0, (b.to(torch.float32) - 127.5) / 32.0, torch.full(b.shape, float("nan"), dtype=torch.float32, device=b.device))


def depth_order(slot_tab, min_pixels=16):
    """(nearer bool [..,65,65], rank int32 [..,65]).  nearer[a, b]: both slots have at least min_pixels pixels with a parallax and b_q1[a] > b_q3[b] -- the
    interquartile ranges of their parallax do not overlap, a's lies higher: a is nearer to the viewer than b.  Slot 0 (the background) is a slot like any other.
    rank[b] = the number of slots that are nearer than b.  Integer comparisons only"""
    _check_tab("depth_order", slot_tab)
    t = slot_tab.to(torch.int64)
    ok = t[..., 0] >= int(min_pixels)
    nearer = ok[..., :, None] & ok[..., None, :] & (t[..., 3][..., :, None] > t[..., 4][..., None, :])
    return nearer, nearer.sum(-2).to(torch.int32)


def agreement(nearer, behind):
    """int64 [..,3]: over the pairs (a, b) on which `behind` ([..,65,65] bool of `object_motion.occlusion_order`: a was hidden behind b) speaks, how many the
    parallax agrees with (nearer[b, a]), contradicts (nearer[a, b]) and is silent about"""
    if not (torch.is_tensor(nearer) and torch.is_tensor(behind)) or tuple(nearer.shape[-2:]) != (_SIDE, _SIDE) or nearer.shape != behind.shape:
        raise ValueError("agreement: nearer and behind must both be [..,65,65], got %s and %s" % (_shape(nearer), _shape(behind)))
    nearer, behind = nearer.bool(), behind.bool().to(nearer.device)
    agree, contra = behind & nearer.transpose(-1, -2), behind & nearer
    count = lambda m: m.flatten(-2).sum(-1)  # noqa: E731
    return torch.stack([count(agree), count(contra), count(behind & ~agree & ~contra)], -1)


# ---- the drivers ----
def lattice_anchors(gh, gw, num_anchors):
    """`num_anchors` cells of a gh x gw patch grid on an evenly spaced lattice: with a the smallest integer whose square is at least num_anchors, the lattice
    points (i, j), i, j < a, are the cells (((2 i + 1) gh) // (2 a), ((2 j + 1) gw) // (2 a)); the first num_anchors in row-major order, as indices y gw + x"""
    k = int(num_anchors)
    if k < 1 or k > gh * gw:
        raise ValueError("lattice_anchors: num_anchors = %d for a grid of %d x %d patches" % (k, gh, gw))
    a = math.isqrt(k - 1) + 1
    return [(((2 * i + 1) * gh) // (2 * a)) * gw + ((2 * j + 1) * gw) // (2 * a) for i in range(a) for j in range(a)][:k]


def ego_motion_flows(G, x, head_motions=None, shifts=None, num_samples=8, anchors=None, num_anchors=9, shift=2, mask=None, sample_batch_size=None, **kwargs):
    """`FlowGenerator.ego_motion_flows` (its docstring says what this does); G is the generator"""
    from . import segment_step as SS

    movie, _ = G._two_frame_movie(x, True)
    B, (H, W) = movie.shape[0], movie.shape[-2:]
    dev = movie.device
    with torch.random.fork_rng(devices=[]):  # the drivers rectangularise and draw masks on torch's global CPU generator; the caller's stream of draws is put back
        if head_motions is not None:
            if not hasattr(G, "predict_imu_video_and_flow"):
                raise ValueError("ego_motion_flows: head_motions need an IMU-conditioned generator (ImuConditionedFlowGenerator)")
            h = torch.as_tensor(head_motions).to(dev)
            if h.dim() == 3:
                h = h[None].expand(B, -1, -1, -1)
            if h.dim() != 4 or h.shape[0] != B or not 1 <= h.shape[1] <= MAX_SAMPLES:
                raise ValueError("ego_motion_flows: head_motions must be [S,C,L] or [B,S,C,L] with B = %d and 1 .. %d samples, got %s" % (B, MAX_SAMPLES, _shape(head_motions)))
            S = h.shape[1]
            h = h.reshape((B * S,) + tuple(h.shape[2:]))  # '(b s)' rows
            G.set_input(movie)
            m = G.generate_mask(movie) if mask is None else mask  # one mask per movie, whatever the chunking
            rows_x, rows_m = movie.repeat_interleave(S, 0), m.repeat_interleave(S, 0)
            step = int(sample_batch_size) if sample_batch_size else B * S
            parts = [G.predict_imu_video_and_flow(rows_x[lo:lo + step], mask=rows_m[lo:lo + step], head_motion=h[lo:lo + step], **kwargs)[1]
                     for lo in range(0, B * S, step)]
            flows = parts[0] if len(parts) == 1 else torch.cat(parts, 0)
            return G.batch_to_samples(flows, t=0, B=B), None
        P = G.patch_size[-1]
        gh, gw = H // P, W // P
        n = gh * gw
        pairs = SS.directions(num_samples, shift) if shifts is None else [(int(dy), int(dx)) for dy, dx in shifts]
        S = len(pairs)
        if not 1 <= S <= MAX_SAMPLES:
            raise ValueError("ego_motion_flows: %d samples, 1 .. %d" % (S, MAX_SAMPLES))
        if anchors is None:
            anchors = torch.tensor(lattice_anchors(gh, gw, num_anchors), dtype=torch.int64)[None].expand(B, -1)
        anchors = torch.as_tensor(anchors).to(device=dev, dtype=torch.int64)
        if anchors.dim() != 2 or anchors.shape[0] != B or bool(((anchors < 0) | (anchors >= n)).any()):
            raise ValueError("ego_motion_flows: anchors must be [B,n] patch indices of frame 1 in 0 .. %d, got %s" % (n - 1, _shape(anchors)))
        active = torch.ones((B, 2 * n), dtype=torch.bool, device=dev)  # 0 = moved: the layout of `SegmentStepResult.active`
        active[:, :n] = False
        active.scatter_(1, n + anchors, False)
        dirs = torch.tensor([(dy * P, dx * P) for dy, dx in pairs], dtype=torch.int32).to(dev)
        _, flows = G.predict_counterfactual_videos_and_flows(x, active.unsqueeze(-1).expand(-1, -1, S), mask, shifts=pairs, num_samples=S,
                                                             sample_batch_size=sample_batch_size, fix_passive=True, **kwargs)
        return G._batch_to_samples(flows), dirs


def parallax(G, x, labels=None, min_pixels=1, min_ref=0.25, min_samples=None, want_spread=True, want_off=True, order_min_pixels=16, **kwargs) -> Parallax:
    """`FlowGenerator.parallax` (its docstring says what this does); G is the generator"""
    flows, dirs = ego_motion_flows(G, x, **kwargs)
    if labels is not None:
        labels = labels.to(flows.device)
    r = measure(flows, dirs=dirs, labels=labels, ref_slot=0 if labels is not None else -1, min_pixels=min_pixels, min_ref=min_ref, min_samples=min_samples,
                want_spread=want_spread, want_off=want_off)
    if r.slot_tab is not None:
        r.nearer, r.rank = depth_order(r.slot_tab, min_pixels=order_min_pixels)
    return r
