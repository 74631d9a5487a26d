"""Per-object motion and occlusion order from tracked segments and flow (no counterpart in the reference, whose README lists read-outs of this kind as coming:
"using counterfactuals to estimate other scene properties").  One pass over the slot map of frame A, the flow from A to the other frame and -- where given -- the
codes of `flow_consistency.check` and the other frame's slot map gives, per slot: the pixel counts by class (believed, inconsistent, unusable or leaving the
frame), the integer sums of a least-squares affine fit, the fit itself -- translation, 2 x 2 matrix, centroid, flow variance: how the object translates, rotates
and looms -- and a 65 x 65 table of which slot was hidden where which other slot stands in the other frame.  Slot 0, everything that is no object, is measured
like any other: its model is the camera's own motion.  `occlusion_order` turns the table into a depth order among the objects, with no depth model.

The definition is the header comment of csrc/object_motion.hip (include/cwm_hip.h `cwm_object_motion`): six numbered steps, integer sums, and the model as
correctly rounded float64 operations in a stated order.  Device tensors take the library call (`measure_device`: allocates the outputs, one call, nothing read
back); CPU tensors take the same definition in plain torch ops in that order (`measure_torch`), which equals the device bit for bit."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib

SLOTS, MAX_PIXELS = 64, 1 << 18
_SIDE = SLOTS + 1
MODEL_FIELDS = ("valid", "tu", "tv", "a11", "a12", "a21", "a22", "mx", "my", "var_u", "var_v", "zero")


class ObjectMotion:
    """sums int64 [..,65,16] (1, x, y, xx, xy, yy, qu, qv, x qu, y qu, x qv, y qv, qu qu, qv qv over the believed pixels of a slot, q the flow in 1/256 px; then
    two zeros); counts int32 [..,65,4] (pixels of class 0 believed, 1 inconsistent, 2 unusable or leaving the frame; then 0); model float64 [..,65,12]
    (MODEL_FIELDS: valid 0 none / 1 translation / 2 affine, the translation, the matrix A, the centroid, the flow variance; the predicted flow of a pixel of the
    object is t + A ((x, y) - (mx, my))); occluders int32 [..,65,65] (row: the slot that was hidden, column: what stands there in the other frame) or None.
    The leading shape is that of the maps: [B] or [B,T]"""
    __slots__ = ("sums", "counts", "model", "occluders")

    def __init__(self, sums, counts, model, occluders=None):
        self.sums, self.counts, self.model, self.occluders = sums, counts, model, occluders


def _planes(t, name, lead, H, W, dtype):
    """a [B,T,H,W] view of a [B,H,W] or [B,T,H,W] map whose H x W planes are contiguous, without a copy where the tensor already is one"""
    if t is None:
        return None
    if not torch.is_tensor(t) or tuple(t.shape) != lead + (H, W):
        raise ValueError("object_motion: %s must be %s, got %s" % (name, lead + (H, W), tuple(t.shape) if torch.is_tensor(t) else type(t)))
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype != dtype:
        raise ValueError("object_motion: %s must be %s, got %s" % (name, dtype, t.dtype))
    if len(lead) == 1:
        t = t.unsqueeze(1)
    if t.stride(-1) != 1 or t.stride(-2) != W or t.stride(0) < 0 or t.stride(1) < 0:
        t = t.contiguous()
    return t


def _prepare(labels, flow, code, other, min_pixels, min_affine, min_det):
    """What Python must refuse before it allocates the outputs; the library (csrc/object_motion.hip) is the statement of the limits.  Returns the maps as
    [B,T,H,W] views and the flow as a [B,T,2,H,W] view, all with contiguous planes (slices [:, :-1] and [:, 1:] of a larger tensor stay views)"""
    if not torch.is_tensor(labels) or labels.dim() not in (3, 4):
        raise ValueError("object_motion: labels must be [B,H,W] or [B,T,H,W], got %s" % (tuple(labels.shape) if torch.is_tensor(labels) else type(labels),))
    lead, (H, W) = tuple(labels.shape[:-2]), labels.shape[-2:]
    R = math.prod(lead)
    if R < 1 or R > 65535 or H <= 0 or W <= 0 or H % 4 or W % 4 or H * W > MAX_PIXELS:
        raise ValueError("object_motion: %d rows of %d x %d pixels: 1 .. 65535 rows, H and W positive multiples of 4, at most 2^18 pixels" % (R, H, W))
    if not torch.is_tensor(flow) or tuple(flow.shape) != lead + (2, H, W):
        raise ValueError("object_motion: flow must be %s, got %s" % (lead + (2, H, W), tuple(flow.shape) if torch.is_tensor(flow) else type(flow)))
    for name, t in (("flow", flow), ("code", code), ("other", other)):
        if t is not None and torch.is_tensor(t) and t.device != labels.device:
            raise ValueError("object_motion: labels is on %s and %s on %s" % (labels.device, name, t.device))
    min_pixels, min_affine, min_det = int(min_pixels), int(min_affine), float(min_det)
    if min_pixels < 1 or min_affine < 3 or not (math.isfinite(min_det) and min_det > 0):
        raise ValueError("object_motion: min_pixels = %d (at least 1), min_affine = %d (at least 3), min_det = %r (finite and positive)" % (
            min_pixels, min_affine, min_det))
    lab = _planes(labels, "labels", lead, H, W, torch.uint8)
    cod = _planes(code, "code", lead, H, W, torch.uint8)
    oth = _planes(other, "other", lead, H, W, torch.uint8)
    f = flow.to(torch.float32)
    if len(lead) == 1:
        f = f.unsqueeze(1)
    if f.stride(-1) != 1 or f.stride(-2) != W or min(f.stride()[:3]) < 0:
        f = f.contiguous()
    return lab, f, cod, oth, lead, H, W, min_pixels, min_affine, min_det


def measure_device(labels, flow, code=None, other=None, min_pixels=1, min_affine=16, min_det=1.0) -> ObjectMotion:
    """the library call on device tensors; asynchronous on the current stream, nothing is read back"""
    _lib.require_gpu()
    lab, f, cod, oth, lead, H, W, min_pixels, min_affine, min_det = _prepare(labels, flow, code, other, min_pixels, min_affine, min_det)
    if lab.device.type != "cuda":
        raise RuntimeError("measure_device needs device tensors")
    dev, (B, T) = lab.device, lab.shape[:2]
    new = lambda shape, dtype: torch.empty(lead + shape, device=dev, dtype=dtype)  # noqa: E731
    r = ObjectMotion(new((_SIDE, 16), torch.int64), new((_SIDE, 4), torch.int32), new((_SIDE, 12), torch.float64),
                     new((_SIDE, _SIDE), torch.int32) if oth is not None else None)
    a = _lib.new_object_motion_args()
    _lib.fill_patch_args(a.base, geometry=(B, T, 0, H, W, 0), stream=_lib.current_stream_handle(dev))
    a.labels_dev, a.flow_dev, a.code_dev, a.other_dev = (_lib.ptr(t) for t in (lab, f, cod, oth))
    for strides, t in ((a.labels_strides, lab), (a.code_strides, cod), (a.other_strides, oth)):
        if t is not None:
            strides[0], strides[1] = t.stride(0), t.stride(1)
    a.flow_strides[0], a.flow_strides[1], a.flow_strides[2] = f.stride(0), f.stride(1), f.stride(2)
    a.min_pixels, a.min_affine, a.min_det = min_pixels, min_affine, min_det
    a.sums_dev, a.counts_dev, a.model_dev, a.occ_dev = (_lib.ptr(t) for t in (r.sums, r.counts, r.model, r.occluders))
    with torch.cuda.device(dev):
        _lib.check(_lib.get_lib().cwm_object_motion(C.byref(a)))
    return r


def model_torch(sums, min_pixels, min_affine, min_det):
    """step 6 on sums [..,16] int64: every line one float64 torch operation, in the order of the definition"""
    f64 = torch.float64
    S = [sums[..., i].to(f64) for i in range(14)]  # (round to nearest)
    N = sums[..., 0]
    some = N >= min_pixels
    n = torch.where(N > 0, S[0], torch.ones_like(S[0]))  # (an empty slot divides by 1; it is zeroed below)
    mx, my, mu, mv = S[1] / n, S[2] / n, S[6] / n, S[7] / n

    def cov(s, a, b):
        q = s / n
        return q - a * b

    cxx, cxy, cyy = cov(S[3], mx, mx), cov(S[4], mx, my), cov(S[5], my, my)
    cxu, cyu, cxv, cyv = cov(S[8], mx, mu), cov(S[9], my, mu), cov(S[10], mx, mv), cov(S[11], my, mv)
    d0, d1 = cxx * cyy, cxy * cxy
    det = d0 - d1
    affine = some & (N >= min_affine) & (det >= min_det)  # (a NaN det compares false)
    scale, scale2 = 2.0 ** -8, 2.0 ** -16

    def coef(p, q, r, s):
        e0, e1 = p * q, r * s
        e = e0 - e1
        e = e / det
        return e * scale

    zero = torch.zeros_like(det)
    a11, a12 = coef(cxu, cyy, cyu, cxy), coef(cyu, cxx, cxu, cxy)
    a21, a22 = coef(cxv, cyy, cyv, cxy), coef(cyv, cxx, cxv, cxy)
    valid = torch.where(affine, torch.full_like(det, 2.0), torch.where(some, torch.ones_like(det), zero))
    rows = [valid, mu * scale, mv * scale] + [torch.where(affine, a, zero) for a in (a11, a12, a21, a22)] + [
        mx, my, cov(S[12], mu, mu) * scale2, cov(S[13], mv, mv) * scale2, zero]
    return torch.stack([torch.where(some, v, zero) for v in rows], -1)


def measure_torch(labels, flow, code=None, other=None, min_pixels=1, min_affine=16, min_det=1.0) -> ObjectMotion:
    """the same definition in plain torch, on the tensors' own device"""
    lab, f, cod, oth, lead, H, W, min_pixels, min_affine, min_det = _prepare(labels, flow, code, other, min_pixels, min_affine, min_det)
    dev, R, i64, f32 = lab.device, math.prod(lead), torch.int64, torch.float32
    flat = lambda t: None if t is None else t.reshape(R, H, W)  # noqa: E731
    lab, cod, oth, f = flat(lab), flat(cod), flat(oth), f.reshape(R, 2, H, W)
    # 1 slot
    l = lab.to(i64)
    l = torch.where(l > SLOTS, torch.zeros_like(l), l)
    # 2 target
    u, v = f[:, 0], f[:, 1]
    xi = torch.arange(W, device=dev)[None, None, :].expand(R, H, W)
    yi = torch.arange(H, device=dev)[None, :, None].expand(R, H, W)
    usable = (u.abs() <= 4096.0) & (v.abs() <= 4096.0)
    fx, fy = xi.to(f32) + u, yi.to(f32) + v
    inside = (fx >= 0) & (fx <= float(W - 1)) & (fy >= 0) & (fy <= float(H - 1))
    # 3 class
    ok = usable & inside
    k = torch.where(ok, torch.zeros_like(l) if cod is None else (cod != 0).to(i64), torch.full_like(l, 2))
    row = torch.arange(R, device=dev)[:, None, None] * _SIDE
    counts = torch.bincount(((row + l) * 4 + k).reshape(-1), minlength=R * _SIDE * 4).reshape(R, _SIDE, 4)
    # 4 sums
    k0 = k == 0
    zf = torch.zeros_like(u)
    qu = torch.round(torch.where(k0, u, zf) * 256.0).to(i64)
    qv = torch.round(torch.where(k0, v, zf) * 256.0).to(i64)
    one = torch.ones_like(l)
    terms = [one, xi, yi, xi * xi, xi * yi, yi * yi, qu, qv, xi * qu, yi * qu, xi * qv, yi * qv, qu * qu, qv * qv]
    index = (row + l).reshape(-1)
    sums = torch.zeros((R * _SIDE, 16), dtype=i64, device=dev)
    for i, t in enumerate(terms):
        sums[:, i].scatter_add_(0, index, torch.where(k0, t, torch.zeros_like(t)).reshape(-1))
    sums = sums.reshape(R, _SIDE, 16)
    # 5 occluder
    occ = None
    if oth is not None:
        k1 = k == 1
        sx = torch.where(k1, torch.round(fx), zf).to(i64)
        sy = torch.where(k1, torch.round(fy), zf).to(i64)
        m = oth.reshape(R, H * W).to(i64).gather(1, (sy * W + sx).reshape(R, H * W)).reshape(R, H, W)
        m = torch.where(m > SLOTS, torch.zeros_like(m), m)
        occ = torch.bincount(((row + l) * _SIDE + m)[k1], minlength=R * _SIDE * _SIDE).reshape(R, _SIDE, _SIDE).to(torch.int32)
    # 6 model
    model = model_torch(sums, min_pixels, min_affine, min_det)
    shaped = lambda t: None if t is None else t.reshape(lead + tuple(t.shape[1:]))  # noqa: E731
    return ObjectMotion(shaped(sums), shaped(counts.to(torch.int32)), shaped(model), shaped(occ))


def measure(labels, flow, code=None, other=None, min_pixels=1, min_affine=16, min_det=1.0) -> ObjectMotion:
    """`labels` ([B,H,W] or [B,T,H,W] uint8 slots of frame A: one library call over the B T rows), `flow` ([B,2,H,W] or [B,T,2,H,W]: from A to the other frame on
    A's grid, channel 0 horizontal, in pixels), `code` (the codes of `flow_consistency.check` for this flow) and `other` (the slot map of the other frame; with
    it the result has `occluders`).  A slot needs min_pixels believed pixels for a model, and min_affine of them with a coordinate covariance of determinant at
    least min_det (px^4) for more than a translation.  Device tensors: the library call; CPU tensors: the torch composition"""
    fn = measure_device if torch.is_tensor(labels) and labels.is_cuda else measure_torch
    return fn(labels, flow, code=code, other=other, min_pixels=min_pixels, min_affine=min_affine, min_det=min_det)


def occlusion_order(occluders, min_count=8, ratio=2):
    """A depth order among the slots from the occluder table ([..,65,65], one pair of frames or a sum of tables over frames that the caller made).  Returns
    (behind, layer).  behind bool [..,65,65], indexed by slot: behind[a, b] holds for a != b in 1 .. 64 iff occ[a][b] >= min_count and
    occ[a][b] > ratio occ[b][a] -- enough pixels of a were hidden where b stands, and clearly more than the other way round; row and column 0 are False.
    layer int32 [..,64] (entry s-1 for slot s): 0 to begin with, then exactly 64 rounds of layer[b] = max(layer[b], max over a with behind[a, b] of
    layer[a] + 1), clamped to 63 -- the longest chain of objects behind b; defined for cyclic evidence as well.  Plain integer torch operations on the table's
    own device: the table is 64 x 64"""
    if not torch.is_tensor(occluders) or occluders.dim() < 2 or tuple(occluders.shape[-2:]) != (_SIDE, _SIDE):
        raise ValueError("occlusion_order: occluders must be [..,65,65], got %s" % (tuple(occluders.shape) if torch.is_tensor(occluders) else type(occluders),))
    o = occluders[..., 1:, 1:].to(torch.int64)
    off = ~torch.eye(SLOTS, dtype=torch.bool, device=o.device)
    rel = (o >= int(min_count)) & (o > int(ratio) * o.transpose(-1, -2)) & off
    behind = torch.zeros(occluders.shape, dtype=torch.bool, device=o.device)
    behind[..., 1:, 1:] = rel
    layer = torch.zeros(o.shape[:-1], dtype=torch.int64, device=o.device)
    for _ in range(SLOTS):
        above = torch.where(rel, (layer + 1)[..., :, None], torch.zeros_like(o)).amax(-2)
        layer = torch.maximum(layer, above).clamp(max=SLOTS - 1)
    return behind, layer.to(torch.int32)
