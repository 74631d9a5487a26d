"""Object interactions: which objects move when one is pushed (no counterpart in the reference, whose README describes the covariance this reads out at the level
of objects: "objects adjacent to one another tend to move together, as some motion counterfactuals include collisions between them").  Where
`segment_spelke_object` asks which pixels move with a seed, `measure` asks which slots of a slot map move with a pushed slot: from the S counterfactual flow samples
of each of K pushes per scene it gives, per push, sample and slot, a small integer table (pixels, how many moved, the flow sums in 1/256 px) and, over the
samples in which the pushed slot itself moved, per slot the share of pushes in which it moved too, its mean displacement along the push and its gain against the
pushed slot.  `relations` turns that into who moves whom, `groups` and `merge_labels` repair a slot map that split one rigid body into several labels, and
`object_interactions` (`FlowGenerator.object_interactions`) is the driver that makes the pushes.

The definition is the header comment of csrc/object_response.hip (include/cwm_hip.h `cwm_object_response`): eight numbered steps, integer sums, and the coupling
as correctly rounded float64 operations in a stated order.  Device tensors take the library call (`measure_device`: allocates the outputs, one call, nothing read
back); CPU tensors take the same definition in plain torch ops in that order (`measure_torch`), which equals the device bit for bit."""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn.functional as F

from . import _lib

SLOTS, MAX_PIXELS, MAX_SAMPLES, MAX_ROWS = 64, 1 << 18, 255, 65535
_SIDE = SLOTS + 1
TAB_FIELDS = ("n", "moved", "su", "sv", "moved_su", "moved_sv", "q2", "unusable")
AGG_FIELDS = ("N", "M", "A", "V")
COUPLING_FIELDS = ("vote", "moved", "along", "gain")


class ObjectResponse:
    """tab int64 [B,K,S,65,8] (TAB_FIELDS per sample and slot: usable pixels, how many of them moved, the flow sums in 1/256 px over all and over the moved ones,
    the sum of squared flows, the pixels whose flow is not usable); valid bool [B,K,S] (the pushed slot itself moved in sample s); agg int64 [B,K,65,4]
    (AGG_FIELDS over the valid samples: pixels, moved pixels, the flow summed along the push, the samples in which the slot moved); coupling float64 [B,K,65,4]
    (COUPLING_FIELDS: V / n_valid, M / N, the mean displacement along the push in pixels, that against the pushed slot's); stats int32 [B,K,4] (n_valid, the
    pushed slot or 0 for a dead row, its area, 0).  `dirs` is the int32 [S,2] (dy, dx) tensor the call was made with, or None"""
    __slots__ = ("tab", "valid", "agg", "coupling", "stats", "dirs")

    def __init__(self, tab, valid, agg, coupling, stats, dirs=None):
        self.tab, self.valid, self.agg, self.coupling, self.stats, self.dirs = tab, valid, agg, coupling, stats, dirs


def _shape(t):
    return tuple(t.shape) if torch.is_tensor(t) else type(t)


def min_q2_of(min_mag) -> int:
    """the squared motion threshold in (1/256 px)^2 that the library takes"""
    return int(round(float(min_mag) * 256.0)) ** 2


def _prepare(flows, labels, pushed, dirs, min_mag, min_pixels, self_frac, move_frac):
    """What Python must refuse before it allocates the outputs; the library (csrc/object_response.hip) is the statement of the limits.  Returns the flows as a
    [R,2,H,W,S] float32 view in whatever strides they have, the maps as a [B,K,H,W] view with contiguous planes (a [B,H,W] map with push stride 0), pushed int32
    [R], dirs int32 [S,2] or None, and the checked scalars"""
    if not torch.is_tensor(flows) or flows.dim() not in (5, 6) or flows.shape[-4] != 2:
        raise ValueError("object_response: flows must be [B,K,2,H,W,S] or [R,2,H,W,S], got %s" % (_shape(flows),))
    if not torch.is_tensor(labels) or labels.dim() not in (3, 4):
        raise ValueError("object_response: labels must be [B,H,W] or [B,K,H,W], got %s" % (_shape(labels),))
    H, W, S = flows.shape[-3:]
    R = math.prod(flows.shape[:-4])
    B = labels.shape[0]
    if tuple(labels.shape[-2:]) != (H, W):
        raise ValueError("object_response: labels are %d x %d and the flows %d x %d" % (tuple(labels.shape[-2:]) + (H, W)))
    if labels.dtype == torch.bool:
        labels = labels.view(torch.uint8)
    if labels.dtype != torch.uint8:
        raise ValueError("object_response: labels must be uint8, got %s" % (labels.dtype,))
    K = labels.shape[1] if labels.dim() == 4 else (flows.shape[1] if flows.dim() == 6 else (R // B if B else 0))
    if B < 1 or K < 1 or B * K != R or R > MAX_ROWS or (flows.dim() == 6 and tuple(flows.shape[:2]) != (B, K)):
        raise ValueError("object_response: %s flows for %s labels: B K rows of B scenes, 1 .. %d rows" % (_shape(flows), _shape(labels), MAX_ROWS))
    if H <= 0 or W <= 0 or H % 4 or W % 4 or H * W > MAX_PIXELS or not 1 <= S <= MAX_SAMPLES:
        raise ValueError("object_response: %d x %d pixels, %d samples: H and W positive multiples of 4, at most 2^18 pixels, 1 .. %d samples" % (H, W, S, MAX_SAMPLES))
    dev = flows.device
    if labels.device != dev:
        raise ValueError("object_response: flows are on %s and labels on %s" % (dev, labels.device))
    f = flows.to(torch.float32)
    if f.dim() == 6:
        f = f.flatten(0, 1)
    if min(f.stride()) < 0:
        f = f.contiguous()
    lab = labels.unsqueeze(1).expand(B, K, H, W) if labels.dim() == 3 else labels
    if lab.stride(-1) != 1 or lab.stride(-2) != W or lab.stride(0) < 0 or lab.stride(1) < 0:
        lab = lab.contiguous()
    pushed = torch.as_tensor(pushed)
    if pushed.numel() != R or pushed.is_floating_point():
        raise ValueError("object_response: pushed must be %d integers, got %s %s" % (R, _shape(pushed), pushed.dtype))
    pushed = pushed.to(device=dev, dtype=torch.int32).reshape(R).contiguous()
    if dirs is not None:
        dirs = torch.as_tensor(dirs)
        if dirs.numel() != 2 * S or dirs.is_floating_point() and not bool((dirs == dirs.round()).all()):
            raise ValueError("object_response: dirs must be [S,2] = (%d, 2) whole pixels (dy, dx), got %s" % (S, _shape(dirs)))
        dirs = dirs.to(device=dev, dtype=torch.int32).reshape(S, 2).contiguous()
    min_mag, min_pixels, self_frac, move_frac = float(min_mag), int(min_pixels), float(self_frac), float(move_frac)
    if not (math.isfinite(min_mag) and 0 <= min_mag <= 8192.0) or min_pixels < 1 or not 0 <= self_frac <= 1 or not 0 <= move_frac <= 1:
        raise ValueError("object_response: min_mag = %r (0 .. 8192 px), min_pixels = %d (at least 1), self_frac = %r and move_frac = %r (in [0, 1])" % (
            min_mag, min_pixels, self_frac, move_frac))
    return f, lab, pushed, dirs, (B, K, H, W, S), min_q2_of(min_mag), min_pixels, self_frac, move_frac


def measure_device(flows, labels, pushed, dirs=None, min_mag=1.0, min_pixels=1, self_frac=0.5, move_frac=0.5) -> ObjectResponse:
    """the library call on device tensors; asynchronous on the current stream, nothing is read back"""
    _lib.require_gpu()
    f, lab, pushed, dirs, (B, K, H, W, S), min_q2, min_pixels, self_frac, move_frac = _prepare(flows, labels, pushed, dirs, min_mag, min_pixels, self_frac, move_frac)
    dev = f.device
    if dev.type != "cuda":
        raise RuntimeError("measure_device needs device tensors")
    new = lambda shape, dtype: torch.empty((B, K) + shape, device=dev, dtype=dtype)  # noqa: E731
    r = ObjectResponse(new((S, _SIDE, 8), torch.int64), new((S,), torch.bool), new((_SIDE, 4), torch.int64), new((_SIDE, 4), torch.float64), new((4,), torch.int32), dirs)
    a = _lib.new_object_response_args()
    _lib.fill_patch_args(a.base, geometry=(B, K, 0, H, W, 0), stream=_lib.current_stream_handle(dev))
    a.flows_dev, a.S = f.data_ptr(), S
    for i in range(5):
        a.flow_strides[i] = f.stride(i)
    a.labels_dev, a.labels_strides[0], a.labels_strides[1] = lab.data_ptr(), lab.stride(0), lab.stride(1)
    a.pushed_dev, a.dirs_dev = pushed.data_ptr(), _lib.ptr(dirs)
    a.min_q2, a.min_pixels, a.self_frac, a.move_frac = min_q2, min_pixels, self_frac, move_frac
    a.tab_dev, a.valid_dev, a.agg_dev, a.coupling_dev, a.stats_dev = (t.data_ptr() for t in (r.tab, r.valid, r.agg, r.coupling, r.stats))
    with torch.cuda.device(dev):
        _lib.check(_lib.get_lib().cwm_object_response(C.byref(a)))
    return r


def measure_torch(flows, labels, pushed, dirs=None, min_mag=1.0, min_pixels=1, self_frac=0.5, move_frac=0.5) -> ObjectResponse:
    """the same definition in plain torch, on the tensors' own device"""
    f, lab, pushed, dirs, (B, K, H, W, S), min_q2, min_pixels, self_frac, move_frac = _prepare(flows, labels, pushed, dirs, min_mag, min_pixels, self_frac, move_frac)
    dev, R, i64, f64 = f.device, B * K, torch.int64, torch.float64
    # 1 slot
    l = lab.reshape(R, H, W).to(i64)
    l = torch.where(l > SLOTS, torch.zeros_like(l), l)[..., None].expand(R, H, W, S)
    # 2 usable
    u, v = f[:, 0], f[:, 1]  # [R,H,W,S]
    usable = (u.abs() <= 4096.0) & (v.abs() <= 4096.0)
    # 3 quantise
    zf = torch.zeros_like(u)
    qu = torch.round(torch.where(usable, u, zf) * 256.0).to(i64)
    qv = torch.round(torch.where(usable, v, zf) * 256.0).to(i64)
    q2 = qu * qu + qv * qv
    moved = usable & (q2 >= min_q2)
    # 4 table
    zi = torch.zeros_like(qu)
    row = torch.arange(R, device=dev)[:, None, None, None] * S + torch.arange(S, device=dev)
    index = (row * _SIDE + l).reshape(-1)
    terms = [usable.to(i64), moved.to(i64), qu, qv, torch.where(moved, qu, zi), torch.where(moved, qv, zi), q2, (~usable).to(i64)]
    tab = torch.zeros((R * S * _SIDE, 8), dtype=i64, device=dev)
    for i, t in enumerate(terms):
        tab[:, i].scatter_add_(0, index, t.reshape(-1))
    tab = tab.reshape(R, S, _SIDE, 8)
    # 5 valid samples
    a = pushed.to(i64)
    alive = (a >= 1) & (a <= SLOTS)
    a = torch.where(alive, a, torch.zeros_like(a))
    n, m, su, sv = (tab[..., i] for i in range(4))  # [R,S,65]
    pick = a[:, None, None].expand(R, S, 1)
    na, ma = n.gather(2, pick)[..., 0], m.gather(2, pick)[..., 0]  # [R,S]
    one = torch.ones_like(na)
    valid = alive[:, None] & (na >= min_pixels) & (ma.to(f64) / torch.where(na > 0, na, one).to(f64) >= self_frac)
    n_valid = valid.sum(1)
    # 6 aggregate
    vm = valid[:, :, None]
    zt = torch.zeros_like(n)
    N, M = torch.where(vm, n, zt).sum(1), torch.where(vm, m, zt).sum(1)
    if dirs is not None:
        dy, dx = dirs[:, 0].to(i64)[None, :, None], dirs[:, 1].to(i64)[None, :, None]
        A = torch.where(vm, su * dx + sv * dy, zt).sum(1)
    else:
        A = torch.zeros_like(N)
    V = (vm & (n > 0) & (m.to(f64) / torch.where(n > 0, n, torch.ones_like(n)).to(f64) >= move_frac)).sum(1)
    agg = torch.stack([N, M, A, V], -1)
    # 7 coupling
    zero = torch.zeros(N.shape, dtype=f64, device=dev)
    some = N != 0
    Nd = torch.where(some, N, torch.ones_like(N)).to(f64)
    mean = A.to(f64) / Nd
    c0 = torch.where((n_valid > 0)[:, None], V.to(f64) / n_valid.clamp(min=1).to(f64)[:, None], zero)
    c1 = torch.where(some, M.to(f64) / Nd, zero)
    c2 = torch.where(some, mean * 2.0 ** -8, zero)
    Na, Aa = N.gather(1, a[:, None]), A.gather(1, a[:, None])
    ok = some & (Na != 0) & (Aa != 0)
    den = Aa.to(f64) / torch.where(Na != 0, Na, torch.ones_like(Na)).to(f64)
    c3 = torch.where(ok, mean / torch.where(ok, den, torch.ones_like(den)), zero)
    coupling = torch.stack([c0, c1, c2, c3], -1)
    # 8 stats
    t0 = tab[:, 0].gather(1, a[:, None, None].expand(R, 1, 8))[:, 0]  # [R,8]: the pushed slot in sample 0
    area = torch.where(alive, t0[:, 0] + t0[:, 7], torch.zeros_like(a))
    stats = torch.stack([n_valid, a, area, torch.zeros_like(a)], 1).to(torch.int32)
    shaped = lambda t: t.reshape((B, K) + tuple(t.shape[1:]))  # noqa: E731
    return ObjectResponse(shaped(tab), shaped(valid), shaped(agg), shaped(coupling), shaped(stats), dirs)


def measure(flows, labels, pushed, dirs=None, min_mag=1.0, min_pixels=1, self_frac=0.5, move_frac=0.5) -> ObjectResponse:
    """`flows` ([B,K,2,H,W,S] or [R,2,H,W,S], R = B K: the S counterfactual flow samples of K pushes per scene, channel 0 horizontal, in pixels, in any strides --
    the `_batch_to_samples` view is read in place), `labels` ([B,H,W] uint8 slots, one map for all pushes of a scene and passed with push stride 0, or
    [B,K,H,W]), `pushed` (R integers: the slot pushed in each row; outside 1 .. 64 is a dead row) and `dirs` ([S,2] whole pixels (dy, dx), the shift of each
    sample; without it nothing is measured along the push).  A pixel moved if its flow, rounded to 1/256 px, is at least min_mag long; a sample is valid if at
    least self_frac of the pushed slot's usable pixels (and at least min_pixels of them exist) moved; a slot moved in a sample if move_frac of its pixels did.
    Device tensors: the library call; CPU tensors: the torch composition"""
    fn = measure_device if torch.is_tensor(flows) and flows.is_cuda else measure_torch
    return fn(flows, labels, pushed, dirs=dirs, min_mag=min_mag, min_pixels=min_pixels, self_frac=self_frac, move_frac=move_frac)


# ---- host decisions: plain integer / bool torch on the tables' own device, in the manner of object_motion.occlusion_order ----
def relations(resp: ObjectResponse, slots, min_vote=0.5, min_gain=0.25):
    """Who moves whom.  `slots` ([K] or [B,K]) are the slots pushed in the rows of `resp`.  Returns (moves, mutual, carries, tested), indexed by slot:
    tested bool [B,65]: a was pushed and at least one of its samples is valid; moves bool [B,65,65]: moves[b, a, l] holds iff a was tested, l >= 1, l != a,
    c0 >= min_vote (l moved in that share of the valid pushes of a) and c3 >= min_gain (and by that fraction of a's own displacement; skipped when the
    response was measured without dirs); mutual = moves & its transpose: two slots that each move when the other is pushed are one body;
    carries[a, l] = moves[a, l] & ~moves[l, a] & tested[l]: pushing a moves l while pushing l leaves a still -- l rides on a.  A slot pushed in several rows
    takes the union of them"""
    c, st = resp.coupling, resp.stats
    if c.dim() != 4 or tuple(c.shape[2:]) != (_SIDE, 4):
        raise ValueError("relations: coupling must be [B,K,65,4], got %s" % (_shape(c),))
    B, K = c.shape[:2]
    dev = c.device
    a = torch.as_tensor(slots).to(device=dev, dtype=torch.int64)
    if a.dim() == 1:
        a = a[None].expand(B, -1)
    if tuple(a.shape) != (B, K):
        raise ValueError("relations: slots must be [K] or [B,K] = (%d, %d), got %s" % (B, K, _shape(a)))
    ok = (a >= 1) & (a <= SLOTS) & (st[..., 0] > 0)  # [B,K]
    a = torch.where(ok, a, torch.zeros_like(a))
    l = torch.arange(_SIDE, device=dev)
    cond = ok[..., None] & (l >= 1) & (l != a[..., None]) & (c[..., 0] >= float(min_vote))
    if resp.dirs is not None:
        cond = cond & (c[..., 3] >= float(min_gain))
    rows = torch.arange(B, device=dev)[:, None].expand(B, K)
    moves = torch.zeros((B, _SIDE, _SIDE), dtype=torch.int32, device=dev).index_put_((rows, a), cond.to(torch.int32), accumulate=True) > 0
    tested = torch.zeros((B, _SIDE), dtype=torch.int32, device=dev).index_put_((rows, a), ok.to(torch.int32), accumulate=True) > 0
    back = moves.transpose(-1, -2)
    return moves, moves & back, moves & ~back & tested[:, None, :], tested


def groups(mutual):
    """int32 [B,65]: for every slot the lowest slot it reaches over mutual links ([B,65,65] bool, as `relations` returns them); exactly 64 rounds of minimum
    propagation, so nothing is read back to learn when it has settled.  Entry 0 is 0"""
    if not torch.is_tensor(mutual) or mutual.dim() != 3 or tuple(mutual.shape[1:]) != (_SIDE, _SIDE):
        raise ValueError("groups: mutual must be [B,65,65], got %s" % (_shape(mutual),))
    link = mutual.bool() | mutual.bool().transpose(-1, -2)
    g = torch.arange(_SIDE, device=mutual.device)[None].expand(mutual.shape[0], -1)
    for _ in range(SLOTS):
        g = torch.minimum(g, torch.where(link, g[:, None, :], torch.full_like(link, _SIDE, dtype=g.dtype)).amin(-1))
    return g.to(torch.int32)


def merge_labels(labels, groups):
    """the slot map with every slot replaced by its group ([B,H,W] or [B,T,H,W] uint8, slices of larger maps included; a byte above 64 reads as 0): a gather"""
    if not torch.is_tensor(labels) or labels.dim() not in (3, 4) or labels.dtype != torch.uint8:
        raise ValueError("merge_labels: labels must be [B,H,W] or [B,T,H,W] uint8, got %s" % (_shape(labels),))
    B = labels.shape[0]
    if tuple(groups.shape) != (B, _SIDE):
        raise ValueError("merge_labels: groups must be [B,65] = (%d, 65), got %s" % (B, _shape(groups)))
    l = labels.reshape(B, -1).to(torch.int64)
    l = torch.where(l > SLOTS, torch.zeros_like(l), l)
    return groups.to(device=labels.device, dtype=torch.uint8).gather(1, l).reshape(labels.shape)


# ---- the driver ----
class ObjectInteractions:
    """What `object_interactions` returns: the `ObjectResponse` fields tab, valid, agg, coupling, stats with leading shape [B,K]; slots int32 [B,K] (the slot
    pushed in each row as asked for) and the masks active / passive bool [B,K,2n] its counterfactuals were made with (0 = active, resp. 0 = passive and visible:
    the layout of `SegmentStepResult`); moves, mutual, carries [B,65,65] and tested [B,65] of `relations` at its defaults; dirs int32 [S,2]"""
    __slots__ = ObjectResponse.__slots__ + ("slots", "active", "passive", "moves", "mutual", "carries", "tested")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def push_masks(labels, slots, P, k_active=4, k_passive=4, ring_radius=1, keys=None):
    """The patches a push of each slot moves and pins.  labels [B,H,W] uint8, slots int [B,K], P the patch size; keys [B,K,n] float ranks the active picks among
    the cells the slot touches (None: by the slot's pixel count in the cell).  Active: the k_active cells with the most pixels of the slot (the higher count
    first, the lower index first: `masking.select_reveal`).  Passive: the first k_passive cells that hold no pixel of ANY slot and lie within ring_radius
    (Chebyshev) of a cell the slot touches -- a neighbouring object is never pinned: it must stay free to respond.  Returns (active, passive) bool [B,K,2n] in the
    layout of `SegmentStepResult` and pushed int32 [B,K]: the slot, or 0 for a dead row (a slot outside 1 .. 64 or without a pixel: nothing active, nothing
    passive).  Integer pooling on the labels' device, nothing read back"""
    from .masking import select_reveal

    B, H, W = labels.shape
    K, dev = slots.shape[1], labels.device
    gh, gw = H // P, W // P
    n, R = gh * gw, B * K
    slots = slots.to(device=dev, dtype=torch.int64)
    lab = labels.to(torch.int64)
    lab = torch.where(lab > SLOTS, torch.zeros_like(lab), lab)
    pool = lambda m: m.reshape(m.shape[:-2] + (gh, P, gw, P)).sum((-3, -1))  # noqa: E731
    count = pool((lab[:, None] == slots[:, :, None, None]) & (slots >= 1)[:, :, None, None] & (slots <= SLOTS)[:, :, None, None])  # [B,K,gh,gw]
    occupied = pool(lab > 0) > 0  # [B,gh,gw]
    touched = count > 0
    pushed = torch.where(touched.flatten(2).any(2), slots, torch.zeros_like(slots)).to(torch.int32)
    rad = min(int(ring_radius), max(gh, gw))
    near = F.max_pool2d(touched.reshape(R, 1, gh, gw).float(), 2 * rad + 1, stride=1, padding=rad).reshape(B, K, gh, gw) > 0
    ring = (near & ~occupied[:, None]).reshape(R, n)
    touched = touched.reshape(R, n)
    key = count.reshape(R, n).float() if keys is None else keys.to(device=dev, dtype=torch.float32).reshape(R, n)
    none = torch.zeros_like(touched)
    act = select_reveal(key, touched, none, int(k_active))
    pas = select_reveal(torch.zeros_like(key), ring, none, int(k_passive))
    rows = torch.arange(R, device=dev)[:, None]
    masks = []
    for cells in (act, pas):
        mk = torch.ones((R, 2 * n + 1), dtype=torch.bool, device=dev)  # (one spare column takes the -1 slots)
        mk[:, :n] = False
        mk[rows, torch.where(cells >= 0, n + cells, torch.full_like(cells, 2 * n))] = False
        masks.append(mk[:, :2 * n].reshape(B, K, 2 * n))
    return masks[0], masks[1], pushed


def object_interactions(G, x, labels, slots=None, num_slots=8, num_samples=8, shift=1, k_active=4, k_passive=4, ring_radius=1, sample=False, generator=None,
                        slot_batch_size=None, sample_batch_size=None, min_mag=1.0, self_frac=0.5, move_frac=0.5, **kwargs) -> ObjectInteractions:
    """`FlowGenerator.object_interactions` (its docstring says what this does); G is the generator"""
    from . import segment_step as SS

    movie, _ = G._two_frame_movie(x, True)
    B, (H, W) = movie.shape[0], movie.shape[-2:]
    P, S, dev = G.patch_size[-1], int(num_samples), movie.device
    if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or tuple(labels.shape) != (B, H, W):
        raise ValueError("object_interactions: labels must be [B,H,W] = (%d, %d, %d) uint8, got %s" % (B, H, W, _shape(labels)))
    if slots is None:
        slots = torch.arange(1, int(num_slots) + 1)
    slots = torch.as_tensor(slots).to(device=dev, dtype=torch.int32)
    if slots.dim() == 1:
        slots = slots[None].expand(B, -1)
    if slots.dim() != 2 or slots.shape[0] != B or slots.shape[1] < 1 or B * slots.shape[1] > MAX_ROWS:
        raise ValueError("object_interactions: slots must be [K] or [B,K] with 1 <= B K <= %d, got %s" % (MAX_ROWS, _shape(slots)))
    if int(k_active) < 1 or int(k_passive) < 0 or not 1 <= S <= MAX_SAMPLES or int(ring_radius) < 1:
        raise ValueError("object_interactions: k_active >= 1, k_passive >= 0, ring_radius >= 1 and 1 .. %d samples" % MAX_SAMPLES)
    slots = slots.contiguous()
    K, n = slots.shape[1], (H // P) * (W // P)
    labels = labels.to(dev)
    shifts = SS.directions(S, shift)
    dirs = torch.tensor([(dy * P, dx * P) for dy, dx in shifts], dtype=torch.int32).to(dev)
    keys = torch.rand((B, K, n), generator=generator, device=dev) if sample else None
    active, passive, pushed = push_masks(labels, slots, P, k_active=k_active, k_passive=k_passive, ring_radius=ring_radius, keys=keys)
    step = int(slot_batch_size) if slot_batch_size else K
    parts = []
    # the counterfactual driver rectangularises its masks on torch's global CPU generator; the caller's stream of draws is put back as it was
    with torch.random.fork_rng(devices=[]):
        for lo in range(0, K, step):
            hi = min(K, lo + step)
            rows = lambda t: t[:, lo:hi].reshape(B * (hi - lo), -1)  # noqa: E731
            _, flows = G.predict_counterfactual_videos_and_flows(x.repeat_interleave(hi - lo, 0), rows(active).unsqueeze(-1).expand(-1, -1, S),
                                                                 rows(passive).unsqueeze(-1).expand(-1, -1, S), shifts=shifts, num_samples=S,
                                                                 sample_batch_size=sample_batch_size, fix_passive=True, **kwargs)
            parts.append(measure(G._batch_to_samples(flows), labels, pushed[:, lo:hi], dirs=dirs, min_mag=min_mag, self_frac=self_frac, move_frac=move_frac))
    resp = ObjectResponse(*(torch.cat([getattr(p, k) for p in parts], 1) for k in ObjectResponse.__slots__[:5]), dirs)
    moves, mutual, carries, tested = relations(resp, pushed)
    return ObjectInteractions(tab=resp.tab, valid=resp.valid, agg=resp.agg, coupling=resp.coupling, stats=resp.stats, dirs=dirs, slots=slots, active=active,
                              passive=passive, moves=moves, mutual=mutual, carries=carries, tested=tested)
