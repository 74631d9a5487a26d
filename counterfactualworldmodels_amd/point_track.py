"""Point tracks through a movie: where query points go over all frames and when they are hidden (no counterpart in the reference).  A point follows the forward
flow of its pair while it stands on the object it started on and the flow can be believed -- usable, inside the frame and, given the backward flow, consistent
by the forward-backward test of `flow_consistency` --; otherwise it coasts on the affine motion model of its object (`object_motion.measure`'s `model`, which
`TrackedScene.motion` holds: its first consumer in the pipeline) or, without one, on its last believed flow vector, and is picked up again when it stands on its
object once more.  A point that slides behind another object therefore does not adopt the occluder's flow.

The definition is the header comment of csrc/point_track.hip (include/cwm_hip.h `cwm_point_track`): five numbered steps per frame, fp32 operations in a stated
order and the coast as float64 operations.  Device tensors take the library call (`track_device`: allocates the outputs, ONE kernel launch for the whole movie,
K points by T frames, nothing read back); CPU tensors take the same definition in plain torch ops in that order (`track_torch`: a Python loop over the frames,
vectorised over rows and points), which equals the device bit for bit."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib

SLOTS, MAX_PIXELS, MAX_FRAMES, MAX_POINTS = 64, 1 << 18, 4096, 65536
_SIDE = SLOTS + 1
VISIBLE, HIDDEN, LEFT, LOST, NOT_STARTED = 0, 1, 2, 3, 255


class PointTracks:
    """xy [B,T,K,2] float32 (x, y) of every point in every frame, NaN for a terminal or not-started entry; state [B,T,K] uint8 (0 visible, 1 hidden and coasting,
    2 left the frame, 3 lost: hidden for more than max_coast consecutive frames, 255 not started yet; 2 and 3 hold to the last frame); under [B,T,K] uint8 (the
    slot the point stands on in that frame; 0 without labels); owner [B,K] uint8 (the slot it stood on in its start frame).  Frame-major: one frame's points are
    one slice"""
    __slots__ = ("xy", "state", "under", "owner")

    def __init__(self, xy, state, under, owner):
        self.xy, self.state, self.under, self.owner = xy, state, under, owner


def grid_points(H, W, stride, B=1, offset=None, device="cpu"):
    """[B,K,2] float32 (x, y): the pixels (offset + i stride, offset + j stride) inside an H x W frame in row-major order, K = rows x columns.  offset defaults
    to stride // 2; stride = 1 (offset 0) is every pixel"""
    H, W, stride, B = int(H), int(W), int(stride), int(B)
    offset = stride // 2 if offset is None else int(offset)
    if H < 1 or W < 1 or stride < 1 or B < 1 or offset < 0 or offset >= min(H, W):
        raise ValueError("grid_points: H = %d, W = %d, stride = %d, B = %d, offset = %d: all at least 1, 0 <= offset < min(H, W)" % (H, W, stride, B, offset))
    ys = torch.arange(offset, H, stride, dtype=torch.float32, device=device)
    xs = torch.arange(offset, W, stride, dtype=torch.float32, device=device)
    pts = torch.stack([xs[None, :].expand(len(ys), len(xs)), ys[:, None].expand(len(ys), len(xs))], -1).reshape(1, -1, 2)
    return pts.expand(B, -1, 2).contiguous()


def _shape(t):
    return tuple(t.shape) if torch.is_tensor(t) else type(t)


def _flows(t, name, shape):
    """a [B,T-1,2,H,W] float32 view whose H x W planes are contiguous, without a copy where the tensor already is one"""
    if not torch.is_tensor(t) or tuple(t.shape) != shape:
        raise ValueError("point_track: %s must be [B,T-1,2,H,W] = %s, got %s" % (name, shape, _shape(t)))
    if not t.dtype.is_floating_point:
        raise ValueError("point_track: %s must be a float tensor, got %s" % (name, t.dtype))
    t = t.to(torch.float32)
    if t.stride(-1) != 1 or t.stride(-2) != shape[-1] or min(t.stride()[:3]) < 0:
        t = t.contiguous()
    return t


def _prepare(fwd, points, bwd, labels, model, start, alpha, beta, max_coast):
    """What Python must refuse before it allocates the outputs; the library (csrc/point_track.hip) is the statement of the limits.  Returns the flows as
    [B,T-1,2,H,W] views, labels as a [B,T,H,W] view and model as a [B,T,65,12] view (slices [:, 1:] of larger tensors stay views), points [B,K,2] and start
    [B,K] contiguous"""
    if not torch.is_tensor(fwd) or fwd.dim() != 5 or fwd.shape[2] != 2:
        raise ValueError("point_track: fwd must be [B,T-1,2,H,W], got %s" % (_shape(fwd),))
    B, T, H, W = fwd.shape[0], fwd.shape[1] + 1, fwd.shape[3], fwd.shape[4]
    if B < 1 or B > 65535 or T < 2 or T > MAX_FRAMES or H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError("point_track: %d rows of %d frames of %d x %d pixels: 1 .. 65535 rows, 2 .. 4096 frames, at most 2^18 pixels" % (B, T, H, W))
    if not torch.is_tensor(points) or points.dim() != 3 or points.shape[0] != B or points.shape[2] != 2:
        raise ValueError("point_track: points must be [B,K,2] with B = %d, got %s" % (B, _shape(points)))
    K = points.shape[1]
    if K < 1 or K > MAX_POINTS:
        raise ValueError("point_track: K = %d points, 1 .. 65536" % K)
    if not points.dtype.is_floating_point:
        raise ValueError("point_track: points must be a float tensor, got %s" % (points.dtype,))
    if model is not None and labels is None:
        raise ValueError("point_track: model is given without labels (the model row of a point is that of the slot it started on)")
    dev = fwd.device
    for name, t in (("points", points), ("bwd", bwd), ("labels", labels), ("model", model), ("start", start)):
        if t is not None and torch.is_tensor(t) and t.device != dev:
            raise ValueError("point_track: fwd is on %s and %s on %s" % (dev, name, t.device))
    alpha, beta, max_coast = float(alpha), float(beta), int(max_coast)
    if not (math.isfinite(alpha) and alpha >= 0 and math.isfinite(beta) and beta >= 0):
        raise ValueError("point_track: alpha = %r and beta = %r must be finite and not negative" % (alpha, beta))
    if max_coast < 0 or max_coast > 2 ** 31 - 1:
        raise ValueError("point_track: max_coast = %d must not be negative" % max_coast)
    f = _flows(fwd, "fwd", (B, T - 1, 2, H, W))
    bw = None if bwd is None else _flows(bwd, "bwd", (B, T - 1, 2, H, W))
    lab = mod = st = None
    if labels is not None:
        if not torch.is_tensor(labels) or tuple(labels.shape) != (B, T, H, W):
            raise ValueError("point_track: labels must be [B,T,H,W] = %s, got %s" % ((B, T, H, W), _shape(labels)))
        lab = labels.view(torch.uint8) if labels.dtype == torch.bool else labels
        if lab.dtype != torch.uint8:
            raise ValueError("point_track: labels must be uint8, got %s" % (labels.dtype,))
        if lab.stride(-1) != 1 or lab.stride(-2) != W or lab.stride(0) < 0 or lab.stride(1) < 0:
            lab = lab.contiguous()
    if model is not None:
        if not torch.is_tensor(model) or tuple(model.shape) != (B, T, _SIDE, 12):
            raise ValueError("point_track: model must be [B,T,65,12] = %s, got %s" % ((B, T, _SIDE, 12), _shape(model)))
        if model.dtype != torch.float64:
            raise ValueError("point_track: model must be float64, got %s" % (model.dtype,))
        mod = model
        if mod.stride(-1) != 1 or mod.stride(-2) != 12 or mod.stride(0) < 0 or mod.stride(1) < 0:
            mod = mod.contiguous()
    if start is not None:
        if not torch.is_tensor(start) or tuple(start.shape) != (B, K):
            raise ValueError("point_track: start must be [B,K] = %s, got %s" % ((B, K), _shape(start)))
        if start.dtype not in (torch.int32, torch.int64):
            raise ValueError("point_track: start must be int32 or int64, got %s" % (start.dtype,))
        if dev.type == "cpu" and bool(((start < 0) | (start >= T)).any()):  # (seen only where it costs no read-back; the device call never starts such a point)
            raise ValueError("point_track: start must lie in 0 .. T-1 = %d" % (T - 1))
        st = start.to(torch.int32).contiguous()
    pts = points.to(torch.float32).contiguous()
    return f, bw, lab, mod, pts, st, (B, T, H, W, K), alpha, beta, max_coast


def track_device(fwd, points, bwd=None, labels=None, model=None, start=None, alpha=0.01, beta=0.5, max_coast=8) -> PointTracks:
    """the library call on device tensors: one kernel launch, asynchronous on the current stream, nothing is read back"""
    _lib.require_gpu()
    f, bw, lab, mod, pts, st, (B, T, H, W, K), alpha, beta, max_coast = _prepare(fwd, points, bwd, labels, model, start, alpha, beta, max_coast)
    if f.device.type != "cuda":
        raise RuntimeError("track_device needs device tensors")
    dev = f.device
    r = PointTracks(torch.empty((B, T, K, 2), device=dev, dtype=torch.float32), torch.empty((B, T, K), device=dev, dtype=torch.uint8),
                    torch.empty((B, T, K), device=dev, dtype=torch.uint8), torch.empty((B, K), device=dev, dtype=torch.uint8))
    a = _lib.new_point_track_args()
    _lib.fill_patch_args(a.base, geometry=(B, T, 0, H, W, 0), stream=_lib.current_stream_handle(dev))
    a.fwd_dev, a.bwd_dev, a.labels_dev, a.model_dev, a.points_dev, a.start_dev = (_lib.ptr(t) for t in (f, bw, lab, mod, pts, st))
    for strides, t, n in ((a.fwd_strides, f, 3), (a.bwd_strides, bw, 3), (a.labels_strides, lab, 2), (a.model_strides, mod, 2)):
        if t is not None:
            for i in range(n):
                strides[i] = t.stride(i)
    a.alpha, a.beta, a.K, a.max_coast = alpha, beta, K, max_coast
    a.xy_dev, a.state_dev, a.under_dev, a.owner_dev = (_lib.ptr(t) for t in (r.xy, r.state, r.under, r.owner))
    with torch.cuda.device(dev):
        _lib.check(_lib.get_lib().cwm_point_track(C.byref(a)))
    return r


def _sample(flow, px, py, W, H):
    """both channels of flow [B,2,H,W] at INSIDE points [B,K]: step 2 of cwm_flow_consistency, every line one float32 operation"""
    B = flow.shape[0]
    x0f, y0f = torch.floor(px), torch.floor(py)
    wx, wy = px - x0f, py - y0f
    ix0, iy0 = x0f.to(torch.int64), y0f.to(torch.int64)
    ix1, iy1 = (ix0 + 1).clamp(max=W - 1), (iy0 + 1).clamp(max=H - 1)
    out = []
    for c in range(2):
        plane = flow[:, c].reshape(B, H * W)
        o00, o01, o10, o11 = (plane.gather(1, iy * W + ix) for iy, ix in ((iy0, ix0), (iy0, ix1), (iy1, ix0), (iy1, ix1)))
        d = o01 - o00
        d = wx * d
        top = o00 + d
        d = o11 - o10
        d = wx * d
        bot = o10 + d
        d = bot - top
        d = wy * d
        out.append(top + d)
    return out


def track_torch(fwd, points, bwd=None, labels=None, model=None, start=None, alpha=0.01, beta=0.5, max_coast=8) -> PointTracks:
    """the same definition in plain torch, on the tensors' own device: a loop over the frames, rows and points at once"""
    f, bw, lab, mod, pts, st, (B, T, H, W, K), alpha, beta, max_coast = _prepare(fwd, points, bwd, labels, model, start, alpha, beta, max_coast)
    dev, f32, f64, i64 = f.device, torch.float32, torch.float64, torch.int64
    zf, zi = torch.zeros((B, K), dtype=f32, device=dev), torch.zeros((B, K), dtype=i64, device=dev)
    qnan = torch.full((), 0x7fc00000, dtype=torch.int32, device=dev).view(f32)
    al, be = torch.tensor(alpha, dtype=f32, device=dev), torch.tensor(beta, dtype=f32, device=dev)
    inside = lambda x, y: (x >= 0) & (x <= float(W - 1)) & (y >= 0) & (y <= float(H - 1))  # noqa: E731
    s = zi if st is None else st.to(i64)
    started = (s >= 0) & (s < T)
    px, py = pts[..., 0].clone(), pts[..., 1].clone()
    l0, l1, run, owner, term = zf, zf, zi, zi, zi
    coasted = torch.zeros((B, K), dtype=torch.bool, device=dev)
    xy, state, under = [], [], []
    for t in range(T):
        active = started & (s <= t) & (term == 0)
        # 1 inside
        ins = inside(px, py)
        term = torch.where(active & ~ins, torch.full_like(term, 2), term)
        live = active & ins
        # 2 under
        un = zi
        if lab is not None:
            rx, ry = torch.where(live, torch.round(px), zf).to(i64), torch.where(live, torch.round(py), zf).to(i64)
            un = lab[:, t].reshape(B, H * W).gather(1, ry * W + rx).to(i64)
            un = torch.where(live & (un <= SLOTS), un, zi)
        owner = torch.where(live & (s == t), un, owner)
        # 3 hidden
        hidden = live & ((un != owner) if lab is not None else coasted)
        run = torch.where(live, torch.where(hidden, run + 1, zi), run)
        lost = live & (run > max_coast)
        term = torch.where(lost, torch.full_like(term, 3), term)
        live = live & ~lost
        state.append(torch.where(~started | (s > t), torch.full_like(term, 255), torch.where(term != 0, term, hidden.to(i64))).to(torch.uint8))
        xy.append(torch.stack([torch.where(live, px, qnan), torch.where(live, py, qnan)], -1))
        under.append(torch.where(live, un, zi).to(torch.uint8))
        if t == T - 1:
            break
        # 4 flow (a point that does not take part samples at (0, 0); what it reads is discarded)
        tried = live & (un == owner)
        a0, a1 = _sample(f[:, t], torch.where(tried, px, zf), torch.where(tried, py, zf), W, H)
        usable = tried & (a0.abs() <= 4096.0) & (a1.abs() <= 4096.0)
        qx, qy = px + a0, py + a1
        qin = inside(qx, qy)
        leaves, believed = usable & ~qin, usable & qin
        if bw is not None:
            o0, o1 = _sample(bw[:, t], torch.where(believed, qx, zf), torch.where(believed, qy, zf), W, H)
            ru, rv = a0 + o0, a1 + o1
            ru2, rv2 = ru * ru, rv * rv
            res = ru2 + rv2
            aa0, aa1, oo0, oo1 = a0 * a0, a1 * a1, o0 * o0, o1 * o1
            m_a, m_o = aa0 + aa1, oo0 + oo1
            mag = m_a + m_o
            thr = al * mag
            thr = thr + be
            believed = believed & (res <= thr)
        l0, l1 = torch.where(believed, a0, l0), torch.where(believed, a1, l1)
        moved = leaves | believed
        # 5 coast
        c0, c1 = l0, l1
        if mod is not None:
            m = mod[:, t].gather(1, owner[..., None].expand(B, K, 12))
            dx, dy = px.to(f64) - m[..., 7], py.to(f64) - m[..., 8]
            e0, e1 = m[..., 3] * dx, m[..., 4] * dy
            cu = e0 + e1
            cu = m[..., 1] + cu
            e0, e1 = m[..., 5] * dx, m[..., 6] * dy
            cv = e0 + e1
            cv = m[..., 2] + cv
            f0, f1 = cu.to(f32), cv.to(f32)
            ok = (m[..., 0] >= 1.0) & torch.isfinite(f0) & torch.isfinite(f1)
            c0, c1 = torch.where(ok, f0, l0), torch.where(ok, f1, l1)
        coast = live & ~moved
        px, py = torch.where(moved, qx, torch.where(coast, px + c0, px)), torch.where(moved, qy, torch.where(coast, py + c1, py))
        coasted = coast
    return PointTracks(torch.stack(xy, 1), torch.stack(state, 1), torch.stack(under, 1), owner.to(torch.uint8))


def track(fwd, points, bwd=None, labels=None, model=None, start=None, alpha=0.01, beta=0.5, max_coast=8) -> PointTracks:
    """`fwd` [B,T-1,2,H,W] in PAIR order (entry t: the flow from frame t to frame t+1 on frame t's grid, channel 0 horizontal, in pixels: what `predict_flow`
    returns), `points` [B,K,2] (x, y) in pixels; optional `bwd` in pair order as `predict_flow_and_occlusion` returns it (entry t: from frame t+1 back to frame
    t on frame t+1's grid) with alpha and beta of the forward-backward test, `labels` [B,T,H,W] uint8 slot maps (`TrackedScene.labels`), `model` [B,T,65,12]
    float64 (`TrackedScene.motion`; needs labels) and `start` [B,K] int, the frame each point begins in (default 0; on CPU tensors a value outside 0 .. T-1 is
    refused, on the device such a point is never started).  A point hidden for more than max_coast consecutive frames is lost.  H and W need not be multiples
    of 4.  Device tensors: the library call; CPU tensors: the torch composition"""
    fn = track_device if torch.is_tensor(fwd) and fwd.is_cuda else track_torch
    return fn(fwd, points, bwd=bwd, labels=labels, model=model, start=start, alpha=alpha, beta=beta, max_coast=max_coast)
