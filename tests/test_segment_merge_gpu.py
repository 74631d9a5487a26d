"""`cwm_segment_merge` on a real MI355X through the C ABI against the NumPy restatement (tests/segment_merge_restatement.py), for EQUALITY: every output is an
integer or an integer divided by P P, and the two threshold tests are one float32 multiply and one compare on both sides.

Shapes: 8 x 12 P = 4 (the hand case: 96 pixels, three words), 20 x 12 P = 4 (240 pixels: a half last word, a partial wave), 24 x 40 P = 8, 64 x 64 P = 16; K in
{1, 2, 5, 33, 64}; B in {1, 3} with different content per row; one largest case 512 x 512, P = 16, K = 64.  Layouts: packed, a [:, :K] slice of a larger buffer
whose unread planes hold 1s, a base pointer one byte off a 16-byte address.  Every output sits between 64 guard bytes; the workspace is filled with 0xA5 before
every call and has guard bytes behind work_bytes."""
import ctypes

import numpy as np
import pytest
import torch

import segment_merge_restatement as MR
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
GUARD = 0xA5
OUT = ("labels", "owner", "area", "label_area", "inter", "cover", "stats")
FIELD = dict(labels="labels_dev", owner="owner_dev", area="area_dev", label_area="label_area_dev", inter="inter_dev", cover="cover_dev", stats="stats_dev")
LAYOUTS = ("packed", "slice", "offset")
SHAPES = ((8, 12, 4), (20, 12, 4), (24, 40, 8), (64, 64, 16))
KS = (1, 2, 5, 33, 64)


def lay_out(segs, layout):
    """a device view [B,K,H,W] uint8 equal to `segs` in the given layout"""
    t = torch.from_numpy(np.ascontiguousarray(segs))
    B, K, H, W = t.shape
    if layout == "packed":
        return t.cuda()
    if layout == "slice":  # the first K planes of a buffer of K + 3 per row; the planes behind them hold 1s
        wide = torch.ones((B, K + 3, H, W), dtype=torch.uint8)
        wide[:, :K] = t
        return wide.cuda()[:, :K]
    buf = torch.zeros(t.numel() + 1, dtype=torch.uint8, device="cuda")  # "offset": packed, one byte past an aligned address
    buf[1:] = t.reshape(-1).cuda()
    v = buf[1:].view(B, K, H, W)
    assert v.data_ptr() % 16 == 1
    return v


def guarded(shape, dtype):
    """(the buffer, its interior view): 64 guard bytes on either side"""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((nbytes + 128,), GUARD, dtype=torch.uint8, device="cuda")
    return buf, buf[64:64 + nbytes].view(dtype).view(*shape)


def guards_intact(buf):
    return bool((buf[:64] == GUARD).all()) and bool((buf[-64:] == GUARD).all())


def run(segs, scores, P, layout="packed", skip=(), expect=0, mutate=None, min_area=1, max_area=0, iou_thresh=0.5, contain_thresh=0.6, absorb=1):
    """one call; returns (dict of CPU arrays of the outputs not in `skip`, the message of a refusal); checks the guards around every output and the workspace"""
    sd = segs if torch.is_tensor(segs) else lay_out(segs, layout)
    B, K, H, W = sd.shape
    n = (H // P) * (W // P) if P > 0 and H % P == 0 and W % P == 0 else 1
    shapes = {"labels": ((B, H, W), torch.uint8), "owner": ((B, K), torch.int32), "area": ((B, K), torch.int32), "label_area": ((B, K), torch.int32),
              "inter": ((B, K, K), torch.int32), "cover": ((B, n), torch.float32), "stats": ((B, 4), torch.int32)}
    bufs = {k: guarded(*shapes[k]) for k in OUT if k not in skip}
    lib = _lib.get_lib()
    nbytes = int(lib.cwm_segment_merge_work_bytes(B, K, H, W)) or 4096
    assert nbytes % 16 == 0
    work = torch.full((nbytes + 128,), GUARD, dtype=torch.uint8, device="cuda")
    assert (work.data_ptr() + 64) % 16 == 0
    kd = None if scores is None else torch.from_numpy(np.ascontiguousarray(scores, np.float32)).cuda()
    a = _lib.new_segment_merge_args()
    _lib.fill_patch_args(a.base, geometry=(B, 2, 0, H, W, P), stream=_lib.current_stream_handle(torch.device("cuda:0")))
    a.K, a.segs_dev, a.scores_dev = K, sd.data_ptr(), _lib.ptr(kd)
    a.seg_strides[0], a.seg_strides[1] = sd.stride(0), sd.stride(1)
    a.min_area, a.max_area, a.iou_thresh, a.contain_thresh, a.absorb = min_area, max_area, iou_thresh, contain_thresh, absorb
    a.work_dev, a.work_bytes = work.data_ptr() + 64, nbytes
    for k in OUT:
        setattr(a, FIELD[k], bufs[k][1].data_ptr() if k in bufs else None)
    if mutate:
        mutate(a)
    rc = lib.cwm_segment_merge(ctypes.byref(a))
    torch.cuda.synchronize()
    msg = lib.cwm_last_error().decode()
    assert rc == expect, (rc, msg)
    assert guards_intact(work), "guard bytes around the workspace"
    out = {}
    for k, (buf, view) in bufs.items():
        assert guards_intact(buf), "guard bytes around %s" % k
        if expect:
            assert bool((buf == GUARD).all()), "%s written by a refused call" % k
        out[k] = view.cpu().numpy()
    return out, msg


def equal(got, want, what=""):
    for k, v in got.items():
        w = want[k].reshape(v.shape)
        if v.dtype == np.float32:
            assert np.array_equal(v.view(np.int32), w.astype(np.float32).view(np.int32)), (k, what)
        else:
            assert np.array_equal(v, w), (k, what)


_WANT = {}


def check(name, segs, scores, P, layout="packed", skip=(), **kw):
    """against the restatement, computed once per (name, keywords) and left unchanged"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _WANT:
        _WANT[key] = MR.merge(segs, scores, P, **kw)
    got, _ = run(segs, scores, P, layout, skip=skip, **kw)
    equal(got, _WANT[key], (name, layout))
    return _WANT[key]


@pytest.mark.parametrize("absorb", [1, 0])
def test_hand_worked_case(absorb):
    segs, scores, P, kw = MR.hand_worked()
    for layout in LAYOUTS:
        want = check("hand", segs, scores, P, layout, absorb=absorb, **kw)
    assert want["owner"].tolist() == MR.HAND["owner"] and want["stats"].tolist() == MR.HAND[absorb]["stats"]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("H,W,P", SHAPES)
def test_random_rectangles(H, W, P, K):
    for i, B in enumerate((1, 3)):
        segs, scores = MR.random_rects(100 * K + H + B, B, K, H, W)
        layout = LAYOUTS[(K + H + i) % 3]
        want = check(("rects", H, W, K, B), segs, scores, P, layout, iou_thresh=0.4, absorb=i)
        assert K < 5 or want["stats"][:, 1].max() >= 2, "the case has one label only"
        if B == 3:
            assert not np.array_equal(want["labels"][0], want["labels"][1])
    check(("rects-special", H, W, K), segs, MR.special_scores(3, K), P, "packed", iou_thresh=0.4)
    check(("rects-noscore", H, W, K), segs, None, P, "slice", min_area=3, max_area=H * W // 2)


@pytest.mark.parametrize("H,W,P", SHAPES)
def test_identical_and_empty_sets(H, W, P):
    for K in (2, 33, 64):
        want = check(("identical", H, W, K), MR.identical(2, K, H, W), MR.special_scores(2, K), P)
        assert want["stats"].tolist() == [[K, 1, (H - 2) * (W - 3), K - 1]] * 2
        want = check(("empty", H, W, K), np.zeros((2, K, H, W), np.uint8), MR.special_scores(2, K), P, "offset")
        assert not want["labels"].any() and want["stats"].tolist() == [[0, 0, 0, 0]] * 2


def test_thresholds_chain_and_area_bounds():
    half = MR.half_overlap()
    assert check("half", half, None, 4, iou_thresh=0.5, contain_thresh=1.0)["owner"].tolist() == [[1, 2]]  # I / U = 0.5 exactly: strict > does not absorb
    assert check("half", half, None, 4, iou_thresh=0.4999, contain_thresh=1.0)["owner"].tolist() == [[1, 1]]
    assert check("chain", MR.chain(), np.array([[3, 2, 1]], np.float32), 4, iou_thresh=0.9)["owner"].tolist() == [[1, 1, 1]]
    nan = float("nan")
    assert check("nan", MR.identical(1, 5, 8, 12), None, 4, iou_thresh=nan, contain_thresh=nan)["owner"].tolist() == [[1, 2, 3, 4, 5]]
    full = np.stack([np.ones((8, 12), np.uint8), MR.rect(8, 12, 0, 4, 0, 4), MR.rect(8, 12, 0, 1, 0, 1)])[None]
    assert check("full", full, None, 4, max_area=48, contain_thresh=2.0, iou_thresh=2.0)["owner"].tolist() == [[0, 1, 2]]
    assert check("full", full, None, 4, min_area=0, contain_thresh=2.0, iou_thresh=2.0)["owner"].tolist() == [[1, 2, 3]]
    assert check("full", full, None, 4, min_area=2, contain_thresh=2.0, iou_thresh=2.0)["owner"].tolist() == [[1, 2, 0]]


def test_every_optional_output_null_in_turn():
    segs, scores = MR.random_rects(7, 3, 5, 24, 40)
    for k in OUT:
        check("optional", segs, scores, 8, skip=(k,))
    check("optional", segs, scores, 8, skip=OUT)
    check("optional-noscore", segs, None, 8)


def test_two_calls_give_the_same_bits():
    segs, scores = MR.random_rects(8, 3, 33, 64, 64)
    a, _ = run(segs, scores, 16, "slice")
    b, _ = run(segs, scores, 16, "slice")
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in OUT)


def test_limits_are_refused_with_the_field_named():
    lib = _lib.get_lib()
    ok = np.zeros((1, 2, 8, 12), np.uint8)

    def refused(field, segs=ok, P=4, **kw):
        _, msg = run(segs, None, P, expect=-1, **kw)
        assert msg.startswith("cwm_segment_merge") and field in msg, (field, msg)

    refused("K = 0", mutate=lambda a: setattr(a, "K", 0))
    refused("K = 65", mutate=lambda a: setattr(a, "K", 65))
    refused("base.P = 5", torch.zeros((1, 2, 10, 10), dtype=torch.uint8, device="cuda"), 5)
    refused("base.H = 10", torch.zeros((1, 2, 10, 12), dtype=torch.uint8, device="cuda"), 4)
    refused("base.T = 3", mutate=lambda a: setattr(a.base, "T", 3))
    refused("base.H base.W", torch.zeros((1, 1, 512, 516), dtype=torch.uint8, device="cuda"), 4)
    refused("patches", torch.zeros((1, 1, 512, 512), dtype=torch.uint8, device="cuda"), 4)
    refused("absorb = 2", absorb=2)
    refused("min_area = -1", min_area=-1)
    refused("max_area = -1", max_area=-1)
    refused("work_dev", mutate=lambda a: setattr(a, "work_dev", None))
    refused("work_dev", mutate=lambda a: setattr(a, "work_dev", a.work_dev + 8))
    refused("work_bytes", mutate=lambda a: setattr(a, "work_bytes", a.work_bytes - 1))
    refused("struct_size", mutate=lambda a: setattr(a, "struct_size", a.struct_size - 8))
    refused("segs_dev", mutate=lambda a: setattr(a, "segs_dev", None))
    refused("seg_strides", mutate=lambda a: a.seg_strides.__setitem__(1, -96))
    assert lib.cwm_segment_merge_work_bytes(1, 2, 8, 12) > 0
    for B, K, H, W in ((0, 2, 8, 12), (1, 0, 8, 12), (1, 65, 8, 12), (1, 2, 0, 12), (1, 2, 8, -4), (1, 2, 10, 12), (1, 2, 512, 516), (70000, 2, 8, 12)):
        assert lib.cwm_segment_merge_work_bytes(B, K, H, W) == 0, (B, K, H, W)


def test_largest_case():
    """512 x 512 (2^18 pixels), P = 16, K = 64: 32 rectangles of 160 x 200 shifted by (9, 7), each twice.  Neighbours in the shift order overlap by 151 x 193 of
    160 x 200 (I / U = 0.84): with scores falling with the index, rectangle 0 is kept, its twin and the rectangles 1 .. i with I / U > 0.5 are absorbed, and so on.
    The areas and the first intersections are rectangle arithmetic; everything is also held against the restatement's loop, run once."""
    segs, scores = MR.shifted_pairs()
    want = check("largest", segs, scores, 16)
    assert want["area"][0].tolist() == [160 * 200] * 64 and want["inter"][0, 0, 1] == 160 * 200 and want["inter"][0, 0, 2] == 151 * 193
    assert want["inter"][0, 0, 63] == max(0, 160 - 9 * 31) * max(0, 200 - 7 * 31) and want["owner"][0, :4].tolist() == [1, 1, 1, 1]
    assert 2 <= want["stats"][0, 1] <= 16 and want["stats"][0, 0] == 64 and want["stats"][0, 2] == want["label_area"][0].sum() == np.count_nonzero(segs[0].any(0))
