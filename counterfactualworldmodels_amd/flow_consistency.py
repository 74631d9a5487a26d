"""Forward-backward flow consistency: whether a flow vector can be believed (no counterpart in the reference).  The checked flow is followed to the other frame,
the other frame's flow is sampled there bilinearly, and the squared round-trip residual is held against `alpha * (|a|^2 + |o|^2) + beta`.  Per pixel: a code
(0 consistent, 1 inconsistent -- occluded or wrong --, 2 the target lies outside the frame), the residual, and the MASKED flow: the checked flow where the code is
0 and NaN elsewhere, which `segment_track.track_step` reads as "falls outside", so that a disoccluded pixel warps nothing in.

The definition is the header comment of csrc/flow_consistency.hip (include/cwm_hip.h `cwm_flow_consistency`): seven numbered steps, every arithmetic step one
correctly rounded float32 operation in the stated order.  Device tensors take the library call (`check_device`: allocates the outputs, one call, nothing read
back); CPU tensors take the same definition in plain torch ops in that order (`check_torch`: no addcmul, no lerp, no grid_sample), which equals the device bit
for bit."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib

MAX_PIXELS = 1 << 18


class FlowConsistency:
    """code uint8 [B,H,W] (0 consistent, 1 inconsistent, 2 outside); stats int32 [B,4] (pixels with code 0, 1, 2, then 0); on request res float32 [B,H,W] (the
    squared residual, +inf for code 2 and for a NaN), masked float32 [B,2,H,W] (the checked flow, NaN where code != 0), cells float32 [B,H/P,W/P] (the fraction
    of a cell's pixels with code != 0), else None.  [B,T,...] inputs give [B,T,...] fields; with `both` every field has a leading dimension of 2: index 0 checks
    `flow` against `other`, index 1 `other` against `flow`"""
    __slots__ = ("code", "res", "masked", "cells", "stats")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _prepare(flow, other, alpha, beta, P, want_cells):
    """What Python must refuse before it allocates the outputs; the library (csrc/flow_consistency.hip) is the statement of the limits.  Returns the two flows as
    [R,2,H,W] float32 views with contiguous planes (a pair [:, t] of a larger tensor stays a view) and the leading shape"""
    if not torch.is_tensor(flow) or not torch.is_tensor(other) or flow.dim() not in (4, 5) or flow.shape[-3] != 2:
        raise ValueError("flow_consistency: flow must be [B,2,H,W] or [B,T,2,H,W], got %s" % (tuple(flow.shape) if torch.is_tensor(flow) else type(flow),))
    if tuple(other.shape) != tuple(flow.shape):
        raise ValueError("flow_consistency: other must have the shape of flow %s, got %s" % (tuple(flow.shape), tuple(other.shape)))
    if other.device != flow.device:
        raise ValueError("flow_consistency: flow is on %s and other on %s" % (flow.device, other.device))
    lead, (H, W) = tuple(flow.shape[:-3]), flow.shape[-2:]
    R = math.prod(lead)
    if R < 1 or R > 65535 or H <= 0 or W <= 0 or H % 4 or W % 4 or H * W > MAX_PIXELS:
        raise ValueError("flow_consistency: %d rows of %d x %d pixels: 1 .. 65535 rows, H and W positive multiples of 4, at most 2^18 pixels" % (R, H, W))
    alpha, beta = float(alpha), float(beta)
    if not (math.isfinite(alpha) and alpha >= 0 and math.isfinite(beta) and beta >= 0):
        raise ValueError("flow_consistency: alpha = %r and beta = %r must be finite and not negative" % (alpha, beta))
    if want_cells and (P not in (4, 8, 16) or H % P or W % P):
        raise ValueError("flow_consistency: want_cells needs P = %r in (4, 8, 16) and H = %d, W = %d multiples of it" % (P, H, W))

    def rows(t):
        t = t.to(torch.float32)
        if t.dim() == 5:
            t = t.reshape(R, 2, H, W)  # (a view where the strides allow it)
        if t.stride(-1) != 1 or t.stride(-2) != W or t.stride(0) < 0 or t.stride(1) < 0:
            t = t.contiguous()
        return t

    return rows(flow), rows(other), lead, R, H, W, alpha, beta


def _shaped(r, both, lead):
    """the fields [D,R,...] as the caller sees them: [B,...] or [B,T,...], with the leading direction dimension only with `both`"""
    def view(t):
        if t is None:
            return None
        t = t.reshape((t.shape[0],) + lead + tuple(t.shape[2:]))
        return t if both else t[0]

    return FlowConsistency(**{k: view(getattr(r, k)) for k in FlowConsistency.__slots__})


def check_device(flow, other, alpha=0.01, beta=0.5, P=0, both=False, want_res=False, want_masked=False, want_cells=False) -> FlowConsistency:
    """the library call on device tensors; asynchronous on the current stream, nothing is read back"""
    _lib.require_gpu()
    a, o, lead, R, H, W, alpha, beta = _prepare(flow, other, alpha, beta, P, want_cells)
    if a.device.type != "cuda":
        raise RuntimeError("check_device needs device tensors")
    dev, D = a.device, 2 if both else 1
    new = lambda shape, dtype: torch.empty(shape, device=dev, dtype=dtype)  # noqa: E731
    r = FlowConsistency(code=new((D, R, H, W), torch.uint8), stats=new((D, R, 4), torch.int32),
                        res=new((D, R, H, W), torch.float32) if want_res else None, masked=new((D, R, 2, H, W), torch.float32) if want_masked else None,
                        cells=new((D, R, H // P, W // P), torch.float32) if want_cells else None)
    args = _lib.new_flow_consistency_args()
    _lib.fill_patch_args(args.base, geometry=(R, 1, 0, H, W, int(P) if want_cells else 0), stream=_lib.current_stream_handle(dev))
    args.a_dev, args.o_dev = a.data_ptr(), o.data_ptr()
    args.a_strides[0], args.a_strides[1], args.o_strides[0], args.o_strides[1] = a.stride(0), a.stride(1), o.stride(0), o.stride(1)
    args.alpha, args.beta, args.both = alpha, beta, int(bool(both))
    args.code_dev, args.res_dev, args.masked_dev, args.cell_dev, args.stats_dev = (_lib.ptr(t) for t in (r.code, r.res, r.masked, r.cells, r.stats))
    with torch.cuda.device(dev):
        _lib.check(_lib.get_lib().cwm_flow_consistency(C.byref(args)))
    return _shaped(r, both, lead)


def _one_direction(a, o, alpha, beta, P, want_cells):
    """steps 1 to 7 for [R,2,H,W] float32 tensors, every line one float32 operation"""
    R, _, H, W = a.shape
    dev, f32 = a.device, torch.float32
    u, v = a[:, 0], a[:, 1]
    xs = torch.arange(W, device=dev, dtype=f32)[None, None, :].expand(R, H, W)
    ys = torch.arange(H, device=dev, dtype=f32)[None, :, None].expand(R, H, W)
    # 1 target
    fx, fy = xs + u, ys + v
    inside = (fx >= 0) & (fx <= float(W - 1)) & (fy >= 0) & (fy <= float(H - 1))
    # 2 sample (an outside pixel samples at its own place; what it reads is discarded)
    fx, fy = torch.where(inside, fx, xs), torch.where(inside, fy, ys)
    x0f, y0f = torch.floor(fx), torch.floor(fy)
    wx, wy = fx - x0f, fy - y0f
    ix0, iy0 = x0f.to(torch.int64), y0f.to(torch.int64)
    ix1, iy1 = (ix0 + 1).clamp(max=W - 1), (iy0 + 1).clamp(max=H - 1)
    s = []
    for c in range(2):
        plane = o[:, c].reshape(R, H * W)
        tap = lambda iy, ix: plane.gather(1, (iy * W + ix).reshape(R, H * W)).reshape(R, H, W)  # noqa: E731
        o00, o01, o10, o11 = tap(iy0, ix0), tap(iy0, ix1), tap(iy1, ix0), tap(iy1, ix1)
        d = o01 - o00
        d = wx * d
        top = o00 + d
        d = o11 - o10
        d = wx * d
        bot = o10 + d
        d = bot - top
        d = wy * d
        s.append(top + d)
    # 3 residual
    ru, rv = u + s[0], v + s[1]
    ru2, rv2 = ru * ru, rv * rv
    res = ru2 + rv2
    uu, vv, s00, s11 = u * u, v * v, s[0] * s[0], s[1] * s[1]
    m_a, m_s = uu + vv, s00 + s11
    mag = m_a + m_s
    thr = torch.tensor(alpha, dtype=f32, device=dev) * mag
    thr = thr + torch.tensor(beta, dtype=f32, device=dev)
    # 4 decision
    one, two = torch.ones((), dtype=torch.uint8, device=dev), torch.full((), 2, dtype=torch.uint8, device=dev)
    code = torch.where(inside, torch.where(res <= thr, torch.zeros_like(one), one), two)
    inf = torch.full((), float("inf"), dtype=f32, device=dev)
    res = torch.where(inside & (res == res), res, inf)
    # 5 masked
    qnan = torch.full((), 0x7fc00000, dtype=torch.int32, device=dev).view(f32)
    masked = torch.where((code == 0)[:, None], a, qnan)
    # 6 cells, 7 stats
    cells = None
    if want_cells:
        count = (code != 0).reshape(R, H // P, P, W // P, P).sum((2, 4))
        cells = count.to(f32) / float(P * P)
    stats = torch.stack([(code == k).sum((1, 2)) for k in range(3)] + [torch.zeros(R, dtype=torch.int64, device=dev)], 1).to(torch.int32)
    return code, res, masked, cells, stats


def check_torch(flow, other, alpha=0.01, beta=0.5, P=0, both=False, want_res=False, want_masked=False, want_cells=False) -> FlowConsistency:
    """the same definition in plain torch, on the tensors' own device"""
    a, o, lead, R, H, W, alpha, beta = _prepare(flow, other, alpha, beta, P, want_cells)
    outs = [_one_direction(a, o, alpha, beta, P, want_cells)] + ([_one_direction(o, a, alpha, beta, P, want_cells)] if both else [])
    stack = lambda i, want=True: torch.stack([d[i] for d in outs]) if want else None  # noqa: E731
    r = FlowConsistency(code=stack(0), res=stack(1, want_res), masked=stack(2, want_masked), cells=stack(3, want_cells), stats=stack(4))
    return _shaped(r, both, lead)


def check(flow, other, alpha=0.01, beta=0.5, P=0, both=False, want_res=False, want_masked=False, want_cells=False) -> FlowConsistency:
    """`flow` ([B,2,H,W] or [B,T,2,H,W]: one library call over the B T rows) checked against `other`, the flow of the other frame that points back; channel 0
    horizontal, channel 1 vertical, in pixels.  alpha = 0.01 and beta = 0.5 are the usual constants of this check.  Device tensors: the library call; CPU
    tensors: the torch composition"""
    fn = check_device if torch.is_tensor(flow) and flow.is_cuda else check_torch
    return fn(flow, other, alpha=alpha, beta=beta, P=P, both=both, want_res=want_res, want_masked=want_masked, want_cells=want_cells)
