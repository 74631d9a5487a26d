"""Scene segments through a movie: the label maps of `segment_scene` linked frame to frame by the backward flow (no counterpart in the reference, whose README
lists the segmentation algorithm itself as coming).  `segment_merge.py` ends at one frame pair: label m is the m-th best-scored object of THAT pair.  This module
gives objects an identity over time: the previous frame's track map is warped onto the current frame, its overlaps with the current labels are counted, tracks
and labels are linked one to one, unlinked tracks coast on the flow or end, unlinked labels are born under new ids.  A frame without a segmentation
(`cur_labels=None`) is carried by the flow alone, so a movie can be segmented every n-th frame.

The definition is the header comment of csrc/segment_track.hip (include/cwm_hip.h `cwm_segment_track`).  Device tensors take the library call
(`track_step_device`: one call, nothing read back); CPU tensors take the same definition composed in plain torch (`track_step_torch`; `torch.round` rounds half
to even as rintf does).  Every output is an integer, the warp is one float32 add per coordinate and the link test one float32 multiply and one compare, so both
give equal results.

`track_sequence` links a given sequence of label maps; `track_scene` is the loop on top of `FlowGenerator.segment_scene` and ONE backward flow call per movie.
Given the forward flows as well (`track_sequence(fwd_flows=...)`, `track_scene(occlusion=True)`), every step warps along the occlusion-masked backward flow of
`flow_consistency.check`."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

SLOTS, MAX_PIXELS = 64, 1 << 18
_SIDE = SLOTS + 1


class TrackState:
    """labels [B,H,W] uint8 (0: none, 1 .. 64: a slot) or None (no previous frame); track_id [B,64] int32 (0: the slot is free, otherwise its persistent id);
    age [B,64] int32 (frames since the slot was last linked); next_id [B] int32 (the id the next birth gets)"""
    __slots__ = ("labels", "track_id", "age", "next_id")

    def __init__(self, labels, track_id, age, next_id):
        self.labels, self.track_id, self.age, self.next_id = labels, track_id, age, next_id

    @classmethod
    def empty(cls, B, H, W, device="cpu"):
        z = lambda *s: torch.zeros(s, device=device, dtype=torch.int32)  # noqa: E731
        return cls(torch.zeros((B, H, W), device=device, dtype=torch.uint8), z(B, SLOTS), z(B, SLOTS), torch.ones((B,), device=device, dtype=torch.int32))


class TrackStepResult:
    """state: the new TrackState (its labels are `out` of the definition); area [B,64] int32; bbox [B,64,4] int32 (y0, x0, y1, x1) inclusive, (0, 0, -1, -1) for an
    empty slot; moments [B,64,2] int64 (sum y, sum x); slot_of_cur [B,64] int32 (the slot of label c at [c-1], or 0); linked_cur [B,64] int32 (the label linked to
    slot p at [p-1], or 0); stats [B,8] int32 (linked, born, coasting, ended, dropped labels, live slots, labelled pixels, 0); table [B,65,65] int32 and warped
    [B,H,W] uint8 on request, else None"""
    __slots__ = ("state", "area", "bbox", "moments", "slot_of_cur", "linked_cur", "stats", "table", "warped")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class TrackedScene:
    """labels [B,T,H,W] uint8 slots; track_id, age, area [B,T,64] int32; bbox [B,T,64,4] int32; moments [B,T,64,2] int64; stats [B,T,8] int32; next_id [B] int32
    after the last frame; segmentations: the per-frame SceneSegmentation objects (None for a carried frame) when `track_scene` was asked for them.  With
    `motion` (else None): motion [B,T,65,12] float64, motion_counts [B,T,65,4] int32 and occluders [B,T,65,65] int32 of `object_motion.measure`: entry t
    describes the pair (t, t+1) in the slots of frame t, which track_id[:, t] names (slot 0: everything that is no object, the camera's own motion); entry T-1
    is zeros.  With `points` (else None): points, the `point_track.PointTracks` (xy [B,T,K,2], state and under [B,T,K], owner [B,K]) of the query points
    through the movie"""
    __slots__ = ("labels", "track_id", "age", "area", "bbox", "moments", "stats", "next_id", "segmentations", "motion", "motion_counts", "occluders", "points")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _check(B, H, W, min_inter, min_area, max_age, carry):
    """What Python must refuse before it allocates the outputs; the library (csrc/segment_track.hip) is the statement of the limits and refuses everything else"""
    if B < 1 or B > 65535 or H <= 0 or W <= 0 or H % 4 or W % 4 or H * W > MAX_PIXELS:
        raise ValueError("segment_track: %d rows of %d x %d pixels: 1 .. 65535 rows, H and W positive multiples of 4, at most 2^18 pixels" % (B, H, W))
    if min_inter < 0 or min_area < 0 or max_age < 0:
        raise ValueError("segment_track: min_inter = %d, min_area = %d, max_age = %d must not be negative" % (min_inter, min_area, max_age))
    if carry not in (0, 1):
        raise ValueError("segment_track: carry = %r, 0 or 1" % (carry,))


def _maps(t, name, shape):
    """a [B,H,W] byte view whose H x W planes are contiguous, without a copy where the tensor already is one (a frame [:, t] of a [B,T,H,W] buffer stays a view)"""
    if t is None:
        return None
    if t.dim() != 3 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError("segment_track: %s must be [B,H,W]%s, got %s" % (name, "" if shape is None else " = %s" % (tuple(shape),), tuple(t.shape)))
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype != torch.uint8:
        raise ValueError("segment_track: %s must be uint8 (or bool), got %s" % (name, t.dtype))
    if t.stride(-1) != 1 or t.stride(-2) != t.shape[-1] or t.stride(0) < 0:
        t = t.contiguous()
    return t


def _flow(flow, shape, device):
    """a [B,2,H,W] float32 view whose H x W planes are contiguous (a pair [:, t] of a [B,T,2,H,W] tensor stays a view)"""
    if flow is None:
        return None
    B, H, W = shape
    if tuple(flow.shape) != (B, 2, H, W):
        raise ValueError("segment_track: flow must be [B,2,H,W] = (%d, 2, %d, %d), got %s" % (B, H, W, tuple(flow.shape)))
    flow = flow.to(device=device, dtype=torch.float32)
    if flow.stride(-1) != 1 or flow.stride(-2) != W or flow.stride(0) < 0 or flow.stride(1) < 0:
        flow = flow.contiguous()
    return flow


def _shape_of(state, cur_labels, flow, shape):
    for t in (None if state is None else state.labels, cur_labels):
        if t is not None:
            return tuple(t.shape)
    if flow is not None:
        return (flow.shape[0],) + tuple(flow.shape[-2:])
    if shape is None:
        raise ValueError("segment_track: no map and no flow gives the geometry: pass shape=(B, H, W)")
    return tuple(shape)


def work_bytes(B, H, W) -> int:
    return int(_lib.get_lib().cwm_segment_track_work_bytes(B, H, W))


def track_step_device(state, cur_labels, flow=None, *, iou_thresh=0.3, min_inter=1, min_area=1, max_age=2, carry=True, want_table=False, want_warped=False,
                      shape=None, out=None, work=None) -> TrackStepResult:
    """the library call on device tensors; asynchronous on the current stream.  state None: no previous frame and an empty state (every label is born).
    `out`: a [B,H,W] uint8 view with contiguous planes that takes the new track map (a frame of a [B,T,H,W] buffer; it must not overlap the inputs);
    `work`: a uint8 workspace of at least work_bytes(B, H, W) to reuse between calls on one stream"""
    _lib.require_gpu()
    shape = _shape_of(state, cur_labels, flow, shape)
    if len(shape) != 3:
        raise ValueError("segment_track: maps must be [B,H,W], got %s" % (shape,))
    B, H, W = shape
    min_inter, min_area, max_age, carry = int(min_inter), int(min_area), int(max_age), int(carry)
    _check(B, H, W, min_inter, min_area, max_age, carry)
    prev = _maps(None if state is None else state.labels, "state.labels", shape)
    cur = _maps(cur_labels, "cur_labels", shape)
    some = next((t for t in (prev, cur, flow, None if state is None else state.track_id) if t is not None), None)
    if some is None or some.device.type != "cuda":
        raise RuntimeError("track_step_device needs device tensors")
    dev = some.device
    flow = _flow(flow, shape, dev)
    lib = _lib.get_lib()
    i32 = lambda *s: torch.empty(s, device=dev, dtype=torch.int32)  # noqa: E731
    if out is None:
        out = torch.empty((B, H, W), device=dev, dtype=torch.uint8)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.stride(-1) != 1 or out.stride(-2) != W or (B > 1 and out.stride(0) < H * W):
        raise ValueError("segment_track: out must be a [B,H,W] uint8 view with contiguous planes")
    new = TrackState(out, i32(B, SLOTS), i32(B, SLOTS), i32(B))
    r = TrackStepResult(state=new, area=i32(B, SLOTS), bbox=i32(B, SLOTS, 4), moments=torch.empty((B, SLOTS, 2), device=dev, dtype=torch.int64),
                        slot_of_cur=i32(B, SLOTS), linked_cur=i32(B, SLOTS), stats=i32(B, 8), table=i32(B, _SIDE, _SIDE) if want_table else None,
                        warped=torch.empty((B, H, W), device=dev, dtype=torch.uint8) if want_warped else None)
    nbytes = int(lib.cwm_segment_track_work_bytes(B, H, W))
    if work is None:
        work = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    a = _lib.new_segment_track_args()
    _lib.fill_patch_args(a.base, geometry=(B, 1, 0, H, W, 0), stream=_lib.current_stream_handle(dev))
    if prev is not None:
        a.prev_dev, a.prev_stride = prev.data_ptr(), prev.stride(0)
    if cur is not None:
        a.cur_dev, a.cur_stride = cur.data_ptr(), cur.stride(0)
    if flow is not None:
        a.flow_dev = flow.data_ptr()
        a.flow_strides[0], a.flow_strides[1] = flow.stride(0), flow.stride(1)
    ins = []
    if state is not None:
        ins = [t.to(device=dev, dtype=torch.int32).contiguous() for t in (state.track_id, state.age, state.next_id)]
        if tuple(ins[0].shape) != (B, SLOTS) or tuple(ins[1].shape) != (B, SLOTS) or tuple(ins[2].shape) != (B,):
            raise ValueError("segment_track: state.track_id and state.age must be [B,64] and state.next_id [B]")
        a.track_id_in_dev, a.age_in_dev, a.next_id_in_dev = (t.data_ptr() for t in ins)
    a.iou_thresh, a.min_inter, a.min_area, a.max_age, a.carry = iou_thresh, min_inter, min_area, max_age, carry
    a.work_dev, a.work_bytes = work.data_ptr(), work.numel()
    a.out_dev, a.out_stride = out.data_ptr(), out.stride(0) if B > 1 else max(out.stride(0), H * W)
    a.track_id_out_dev, a.age_out_dev, a.next_id_out_dev = new.track_id.data_ptr(), new.age.data_ptr(), new.next_id.data_ptr()
    a.area_dev, a.bbox_dev, a.moments_dev = r.area.data_ptr(), r.bbox.data_ptr(), r.moments.data_ptr()
    a.slot_of_cur_dev, a.linked_cur_dev, a.stats_dev = r.slot_of_cur.data_ptr(), r.linked_cur.data_ptr(), r.stats.data_ptr()
    a.table_dev, a.warped_dev = _lib.ptr(r.table), _lib.ptr(r.warped)
    with torch.cuda.device(dev):
        _lib.check(lib.cwm_segment_track(C.byref(a)))
    return r


def track_step_torch(state, cur_labels, flow=None, *, iou_thresh=0.3, min_inter=1, min_area=1, max_age=2, carry=True, want_table=False, want_warped=False,
                     shape=None) -> TrackStepResult:
    """the same definition in plain torch, on the tensors' own device"""
    shape = _shape_of(state, cur_labels, flow, shape)
    if len(shape) != 3:
        raise ValueError("segment_track: maps must be [B,H,W], got %s" % (shape,))
    B, H, W = shape
    min_inter, min_area, max_age, carry = int(min_inter), int(min_area), int(max_age), int(carry)
    _check(B, H, W, min_inter, min_area, max_age, carry)
    prev = _maps(None if state is None else state.labels, "state.labels", shape)
    cur = _maps(cur_labels, "cur_labels", shape)
    some = next((t for t in (prev, cur, flow, None if state is None else state.track_id) if t is not None), None)
    dev = torch.device("cpu") if some is None else some.device
    flow = _flow(flow, shape, dev)
    i64 = torch.int64
    zeros = lambda *s: torch.zeros(s, device=dev, dtype=i64)  # noqa: E731
    rows = torch.arange(B, device=dev)
    if state is None:
        tid_in, age_in, next_in = zeros(B, SLOTS), zeros(B, SLOTS), torch.ones((B,), device=dev, dtype=i64)
    else:
        tid_in, age_in, next_in = (t.to(device=dev, dtype=i64) for t in (state.track_id, state.age, state.next_id))
    live = torch.cat([torch.zeros((B, 1), dtype=torch.bool, device=dev), tid_in != 0], 1)  # by slot 0 .. 64
    # 0 inputs, 1 warp
    c = zeros(B, H, W) if cur is None else cur.to(i64)
    c = torch.where(c > SLOTS, torch.zeros_like(c), c)
    w = zeros(B, H, W)
    if prev is not None:
        ys = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None].expand(B, H, W)
        xs = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :].expand(B, H, W)
        rx = torch.round(xs + flow[:, 0]) if flow is not None else xs
        ry = torch.round(ys + flow[:, 1]) if flow is not None else ys
        inside = (rx >= 0) & (rx <= float(W - 1)) & (ry >= 0) & (ry <= float(H - 1))
        src = torch.where(inside, ry, torch.zeros_like(ry)).to(i64) * W + torch.where(inside, rx, torch.zeros_like(rx)).to(i64)
        got = prev.reshape(B, H * W).to(i64).gather(1, src.reshape(B, H * W)).reshape(B, H, W)
        got = torch.where(inside & (got <= SLOTS), got, torch.zeros_like(got))
        w = torch.where(live.gather(1, got.reshape(B, -1)).reshape(B, H, W), got, torch.zeros_like(got))
    # 2 table
    pair = (c * _SIDE + w).reshape(B, -1) + rows[:, None] * (_SIDE * _SIDE)
    n = torch.bincount(pair.reshape(-1), minlength=B * _SIDE * _SIDE).reshape(B, _SIDE, _SIDE)
    area_cur, area_w = n.sum(2), n.sum(1)
    # 3 link: 64 rounds of arg-max over the candidates' (count, lower index first) words
    thr = torch.tensor(iou_thresh, dtype=torch.float32, device=dev)
    nn = n[:, 1:, 1:]
    union = area_cur[:, 1:, None] + area_w[:, None, 1:] - nn
    cand = (nn >= max(1, min_inter)) & (nn.to(torch.float32) > thr * union.to(torch.float32))
    idx = torch.arange(SLOTS * SLOTS, device=dev)
    word = torch.where(cand.reshape(B, -1), nn.reshape(B, -1) * (SLOTS * SLOTS) + (SLOTS * SLOTS - 1 - idx)[None], torch.full((1, 1), -1, dtype=i64, device=dev))
    slot_of, linked = zeros(B, _SIDE), zeros(B, _SIDE)
    for _ in range(SLOTS):
        best, at = word.max(1)
        hit = best >= 0
        ci, pi = torch.div(at, SLOTS, rounding_mode="floor") + 1, at % SLOTS + 1
        slot_of[rows, ci] = torch.where(hit, pi, slot_of[rows, ci])
        linked[rows, pi] = torch.where(hit, ci, linked[rows, pi])
        gone = hit[:, None] & ((torch.div(idx, SLOTS, rounding_mode="floor")[None] == (ci - 1)[:, None]) | ((idx % SLOTS)[None] == (pi - 1)[:, None]))
        word = torch.where(gone, torch.full_like(word, -1), word)
    # 4 coast or end
    is_live, is_linked = live[:, 1:], linked[:, 1:] > 0
    coast = is_live & ~is_linked & bool(carry) & (area_w[:, 1:] > 0) & (age_in + 1 <= max_age)
    ended = is_live & ~is_linked & ~coast
    # 5 births: the r-th wanting label (ascending) takes the r-th free slot (ascending)
    free = ~is_live | ended
    wants = (slot_of[:, 1:] == 0) & (area_cur[:, 1:] >= max(1, min_area))
    free_rank, want_rank = free.to(i64).cumsum(1) - 1, wants.to(i64).cumsum(1) - 1
    n_free, n_want = free.sum(1), wants.sum(1)
    born = free & (free_rank < n_want[:, None])
    n_born = torch.minimum(n_free, n_want)
    slots = torch.arange(1, _SIDE, device=dev)[None].expand(B, SLOTS)
    slot_by_rank = zeros(B, SLOTS + 1).scatter_(1, torch.where(free, free_rank, torch.full_like(free_rank, SLOTS)), slots)[:, :SLOTS]
    got_slot = wants & (want_rank < n_free[:, None])
    slot_of[:, 1:] = torch.where(got_slot, slot_by_rank.gather(1, want_rank.clamp(min=0)), slot_of[:, 1:])
    wrap = lambda v: ((v + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)  # noqa: E731
    tid_out = torch.where(is_linked | coast, tid_in, torch.where(born, next_in[:, None] + free_rank, torch.zeros_like(tid_in)))
    age_out = torch.where(coast, age_in + 1, torch.zeros_like(age_in))
    # 6 paint
    by_label = slot_of.gather(1, c.reshape(B, -1)).reshape(B, H, W)
    coast_lut = torch.cat([zeros(B, 1), torch.where(coast, slots, torch.zeros_like(slots))], 1)
    out = torch.where(by_label > 0, by_label, coast_lut.gather(1, w.reshape(B, -1)).reshape(B, H, W))
    # 7 read-outs
    flat = out.reshape(B, -1)
    yy = torch.arange(H, device=dev)[:, None].expand(H, W).reshape(1, -1).expand(B, -1)
    xx = torch.arange(W, device=dev)[None, :].expand(H, W).reshape(1, -1).expand(B, -1)
    area = zeros(B, _SIDE).scatter_add_(1, flat, torch.ones_like(flat))[:, 1:]
    sum_y, sum_x = zeros(B, _SIDE).scatter_add_(1, flat, yy)[:, 1:], zeros(B, _SIDE).scatter_add_(1, flat, xx)[:, 1:]
    big = torch.full((B, _SIDE), 1 << 30, dtype=i64, device=dev)
    y0, x0 = big.clone().scatter_reduce_(1, flat, yy, "amin")[:, 1:], big.clone().scatter_reduce_(1, flat, xx, "amin")[:, 1:]
    y1, x1 = (-big).scatter_reduce_(1, flat, yy, "amax")[:, 1:], (-big).scatter_reduce_(1, flat, xx, "amax")[:, 1:]
    some_px = area > 0
    z, m1 = torch.zeros_like(area), torch.full_like(area, -1)
    bbox = torch.stack([torch.where(some_px, y0, z), torch.where(some_px, x0, z), torch.where(some_px, y1, m1), torch.where(some_px, x1, m1)], -1)
    # 8 tables, 9 stats
    dropped = ((area_cur[:, 1:] >= 1) & (slot_of[:, 1:] == 0)).sum(1)
    tid32 = wrap(tid_out)
    stats = torch.stack([is_linked.sum(1), n_born, coast.sum(1), ended.sum(1), dropped, (tid32 != 0).sum(1), area.sum(1), torch.zeros_like(n_born)], 1)
    new = TrackState(out.to(torch.uint8), tid32, age_out.to(torch.int32), wrap(next_in + n_born))
    return TrackStepResult(state=new, area=area.to(torch.int32), bbox=bbox.to(torch.int32), moments=torch.stack([sum_y, sum_x], -1),
                           slot_of_cur=slot_of[:, 1:].to(torch.int32), linked_cur=linked[:, 1:].to(torch.int32), stats=stats.to(torch.int32),
                           table=n.to(torch.int32) if want_table else None, warped=w.to(torch.uint8) if want_warped else None)


def _is_cuda(state, cur_labels, flow):
    for t in (None if state is None else state.track_id, None if state is None else state.labels, cur_labels, flow):
        if t is not None:
            return t.is_cuda
    return False


def track_step(state, cur_labels, flow=None, **kw) -> TrackStepResult:
    """device tensors: the library call; CPU tensors: the torch composition"""
    return (track_step_device if _is_cuda(state, cur_labels, flow) else track_step_torch)(state, cur_labels, flow, **kw)


def track_sequence(label_maps, back_flows=None, fwd_flows=None, occ_alpha=0.01, occ_beta=0.5, motion=False, motion_kwargs=None, points=None, point_kwargs=None,
                   **kw) -> TrackedScene:
    """Links a given sequence.  label_maps: [B,T,H,W] uint8, or a list of T entries [B,H,W] / None (None: the frame is carried by the flow alone); back_flows
    [B,T,2,H,W] or None (zero motion): entry t is the flow from frame t to frame t - 1 on frame t's grid, entry 0 is not read.  Frame 0 has no previous frame
    and no flow: every label is born.  Frames and pairs are read in place and, on the device, written in place; nothing is read back in the loop.
    fwd_flows [B,T,2,H,W] (entry t: the flow from frame t - 1 to frame t on frame t - 1's grid, entry 0 is not read) makes the tracking occlusion-aware: step t
    gets the MASKED backward flow of `flow_consistency.check(back_flows[:, t], fwd_flows[:, t], occ_alpha, occ_beta)` -- NaN where the round trip fails --, so a
    disoccluded pixel warps nothing in and is 0 in a carried frame.  The masked flows of the whole movie come from ONE library call before the loop.
    motion=True (needs fwd_flows) also measures how every slot moves and who hides whom: the check before the loop runs in both directions, so that it gives
    the forward codes as well, and after the loop ONE `object_motion.measure(labels[:, :-1], fwd_flows[:, 1:], code=forward codes, other=labels[:, 1:],
    **motion_kwargs)` call over the T-1 pairs, all views read in place, fills `motion`, `motion_counts` and `occluders` of the result.
    points [B,K,2] (x, y) (needs fwd_flows and at least two frames) also follows these points through the movie: after the loop ONE
    `point_track.track(fwd_flows[:, 1:], points, bwd=back_flows[:, 1:], labels=labels, model=motion, **point_kwargs)` call -- the flows as given (not the masked
    ones) in pair order, the slot maps and, with motion=True, the models, all views read in place -- fills `points` of the result (keywords: start, alpha, beta,
    max_coast).  Without motion=True a hidden point coasts on its last believed flow vector."""
    if motion and fwd_flows is None:
        raise ValueError("track_sequence: motion=True needs fwd_flows (the forward flows carry the motion and the occlusion codes)")
    if points is not None and fwd_flows is None:
        raise ValueError("track_sequence: points need fwd_flows (a point follows the forward flows)")
    frames = [label_maps[:, t] for t in range(label_maps.shape[1])] if torch.is_tensor(label_maps) else list(label_maps)
    T = len(frames)
    first = next((f for f in frames if f is not None), None)
    if first is None or T < 1:
        raise ValueError("track_sequence: at least one frame must have a label map")
    if points is not None and T < 2:
        raise ValueError("track_sequence: points need at least two frames, got %d" % T)
    B, H, W = first.shape
    if back_flows is not None and tuple(back_flows.shape) != (B, T, 2, H, W):
        raise ValueError("track_sequence: back_flows must be [B,T,2,H,W] = (%d, %d, 2, %d, %d), got %s" % (B, T, H, W, tuple(back_flows.shape)))
    dev = first.device
    if fwd_flows is not None:
        if back_flows is None or tuple(fwd_flows.shape) != tuple(back_flows.shape):
            raise ValueError("track_sequence: fwd_flows needs back_flows of the same shape [B,T,2,H,W] = (%d, %d, 2, %d, %d), got %s" % (
                B, T, H, W, tuple(fwd_flows.shape)))
        if T > 1:
            from . import flow_consistency as FC

            fwd_pairs = fwd_flows[:, 1:].to(back_flows)  # (a view: entry t - 1 is the pair (t - 1, t))
            back_pairs = back_flows[:, 1:]  # (a view of the flows as given: entry t - 1 is the flow from frame t back to frame t - 1)
            if motion:
                fc = FC.check(back_flows[:, 1:], fwd_pairs, alpha=occ_alpha, beta=occ_beta, both=True, want_masked=True)
                masked, fwd_code = fc.masked[0], fc.code[1]  # (index 0: the backward flow checked; index 1: the forward flow checked)
            else:
                masked = FC.check(back_flows[:, 1:], fwd_pairs, alpha=occ_alpha, beta=occ_beta, want_masked=True).masked
            back_flows = torch.cat([masked[:, :1], masked], 1)  # (entry 0 is not read)
    _check(B, H, W, int(kw.get("min_inter", 1)), int(kw.get("min_area", 1)), int(kw.get("max_age", 2)), int(kw.get("carry", True)))
    labels = torch.empty((B, T, H, W), device=dev, dtype=torch.uint8)
    extra = dict(work=torch.empty((work_bytes(B, H, W),), device=dev, dtype=torch.uint8)) if dev.type == "cuda" else {}
    step = track_step_device if dev.type == "cuda" else track_step_torch
    state, res = None, []
    for t, cur in enumerate(frames):
        flow = None if t == 0 or back_flows is None else back_flows[:, t]
        if dev.type == "cuda":
            r = step(state, cur, flow, shape=(B, H, W), out=labels[:, t], **extra, **kw)
        else:
            r = step(state, cur, flow, shape=(B, H, W), **kw)
            labels[:, t] = r.state.labels
            r.state.labels = labels[:, t]
        res.append(r)
        state = r.state
    stack = lambda name: torch.stack([getattr(r, name) for r in res], 1)  # noqa: E731
    tracked = TrackedScene(labels=labels, track_id=torch.stack([r.state.track_id for r in res], 1), age=torch.stack([r.state.age for r in res], 1),
                           area=stack("area"), bbox=stack("bbox"), moments=stack("moments"), stats=stack("stats"), next_id=state.next_id)
    if motion:
        from . import object_motion as OM

        def padded(t):  # [B,T-1,...] -> [B,T,...]: entry T-1 is zeros
            return torch.cat([t, torch.zeros_like(t[:, :1])], 1)

        if T > 1:
            m = OM.measure(labels[:, :-1], fwd_pairs, code=fwd_code, other=labels[:, 1:], **(motion_kwargs or {}))
            tracked.motion, tracked.motion_counts, tracked.occluders = padded(m.model), padded(m.counts), padded(m.occluders)
        else:
            tracked.motion = torch.zeros((B, 1, _SIDE, 12), device=dev, dtype=torch.float64)
            tracked.motion_counts = torch.zeros((B, 1, _SIDE, 4), device=dev, dtype=torch.int32)
            tracked.occluders = torch.zeros((B, 1, _SIDE, _SIDE), device=dev, dtype=torch.int32)
    if points is not None:
        from . import point_track as PT

        tracked.points = PT.track(fwd_pairs, points.to(dev), bwd=back_pairs, labels=labels, model=tracked.motion, **(point_kwargs or {}))
    return tracked


def backward_pair_flows(G, x, flow_kwargs=None):
    """[B,T,2,H,W]: entry t >= 1 is the flow from frame t to frame t - 1 on frame t's grid, from ONE `G.predict_flow(x, backward=True)` call (which stores pair t
    at index T-2-t); entry 0 is zeros and is not read"""
    flows = G.predict_flow(x, backward=True, **(flow_kwargs or {}))  # [B,T-1,2,H,W]: index j is the pair (x[T-1-j], x[T-2-j])
    B, Tm1 = flows.shape[:2]
    if Tm1 != x.shape[1] - 1:
        raise ValueError("track_scene: predict_flow(backward=True) returned %d pairs for %d frames" % (Tm1, x.shape[1]))
    return torch.cat([torch.zeros_like(flows[:, :1]), flows.flip(1)], 1)


def forward_pair_flows(G, x, flow_kwargs=None):
    """[B,T,2,H,W]: entry t >= 1 is the flow from frame t - 1 to frame t on frame t - 1's grid, from ONE `G.predict_flow(x)` call; entry 0 is zeros and is not
    read"""
    flows = G.predict_flow(x, **(flow_kwargs or {}))  # [B,T-1,2,H,W]: index j is the pair (x[j], x[j+1])
    if flows.shape[1] != x.shape[1] - 1:
        raise ValueError("track_scene: predict_flow returned %d pairs for %d frames" % (flows.shape[1], x.shape[1]))
    return torch.cat([torch.zeros_like(flows[:, :1]), flows], 1)


def track_scene(G, x, segment_every=1, flow_kwargs=None, iou_thresh=0.3, min_inter=1, min_area=1, max_age=2, carry=True, return_segmentations=False,
                occlusion=False, occ_alpha=0.01, occ_beta=0.5, motion=False, motion_kwargs=None, points=None, point_kwargs=None, **segment_scene_kwargs):
    """`FlowGenerator.track_scene` (its docstring says what this does); G is the generator"""
    if motion and not occlusion:
        raise ValueError("track_scene: motion=True needs occlusion=True (the forward flows and their codes)")
    if points is not None and not occlusion:
        raise ValueError("track_scene: points need occlusion=True (the forward flows; motion=True as well for coasting on the objects' models)")
    segment_every, max_age = int(segment_every), int(max_age)
    if x.dim() != 5 or x.shape[1] < 2:
        raise ValueError("track_scene: x must be a movie [B,T,C,H,W] of at least two frames, got %s" % (tuple(x.shape),))
    if segment_every < 1:
        raise ValueError("track_scene: segment_every = %d, at least 1" % segment_every)
    if max_age < segment_every:
        raise ValueError("track_scene: max_age = %d < segment_every = %d: tracks would die between segmentations" % (max_age, segment_every))
    if not carry and segment_every > 1:
        raise ValueError("track_scene: carry is off with segment_every = %d: tracks would die between segmentations" % segment_every)
    T = x.shape[1]
    back = backward_pair_flows(G, x, flow_kwargs)
    occ = dict(fwd_flows=forward_pair_flows(G, x, flow_kwargs), occ_alpha=occ_alpha, occ_beta=occ_beta) if occlusion else {}
    if motion:
        occ.update(motion=True, motion_kwargs=motion_kwargs)
    if points is not None:
        occ.update(points=points, point_kwargs=point_kwargs)
    scenes = [G.segment_scene(x[:, t:t + 2], **segment_scene_kwargs) if t <= T - 2 and t % segment_every == 0 else None for t in range(T)]
    tracked = track_sequence([None if s is None else s.labels for s in scenes], back, iou_thresh=iou_thresh, min_inter=min_inter, min_area=min_area,
                             max_age=max_age, carry=carry, **occ)
    if return_segmentations:
        tracked.segmentations = scenes
    return tracked
