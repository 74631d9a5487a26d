"""`cwm_segment_track` on a real MI355X through the C ABI against the NumPy restatement (tests/segment_track_restatement.py), for EQUALITY: every output is an
integer, the warp is one float32 add per coordinate and the link test one float32 multiply and one compare on both sides.

Shapes: 8 x 12 (the hand case: 96 pixels, six groups of 16, rows that are no multiple of 16), 20 x 12 (240 pixels: a partial wave), 24 x 40, 64 x 64 (more than
one workgroup per row is reached by the largest case, 512 x 512 with 64 labels and 64 slots).  Map layouts: packed, a frame [:, t] of a [B,T,H,W] buffer whose
other frames hold slot bytes, a base pointer one byte off a 16-byte address.  Flow layouts: packed, a pair [:, t] of a [B,T,2,H,W] tensor, a channel-strided
view, a base pointer four bytes off a 16-byte address, NULL.  Every output sits between 64 guard bytes; the workspace is filled with 0xA5 before every call and
has guard bytes behind work_bytes."""
import ctypes

import numpy as np
import pytest
import torch

import segment_track_restatement as TR
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
GUARD = 0xA5
OUT = ("out", "track_id", "age", "next_id", "area", "bbox", "moments", "slot_of_cur", "linked_cur", "table", "warped", "stats")
FIELD = dict(out="out_dev", track_id="track_id_out_dev", age="age_out_dev", next_id="next_id_out_dev", area="area_dev", bbox="bbox_dev", moments="moments_dev",
             slot_of_cur="slot_of_cur_dev", linked_cur="linked_cur_dev", table="table_dev", warped="warped_dev", stats="stats_dev")
MAP_LAYOUTS = ("packed", "frame", "offset")
FLOW_LAYOUTS = ("packed", "pair", "channel", "offset")
SHAPES = ((8, 12), (20, 12), (24, 40), (64, 64))


def lay_out_map(m, layout):
    """a device view [B,H,W] uint8 equal to `m` in the given layout"""
    t = torch.from_numpy(np.ascontiguousarray(m))
    B, H, W = t.shape
    if layout == "packed":
        return t.cuda()
    if layout == "frame":  # frame 1 of a [B,3,H,W] buffer; the frames around it hold slot bytes
        wide = torch.full((B, 3, H, W), 3, dtype=torch.uint8)
        wide[:, 1] = t
        return wide.cuda()[:, 1]
    buf = torch.zeros(t.numel() + 1, dtype=torch.uint8, device="cuda")  # "offset": packed, one byte past an aligned address
    buf[1:] = t.reshape(-1).cuda()
    v = buf[1:].view(B, H, W)
    assert v.data_ptr() % 16 == 1
    return v


def lay_out_flow(f, layout):
    """a device view [B,2,H,W] float32 equal to `f` in the given layout"""
    t = torch.from_numpy(np.ascontiguousarray(f, np.float32))
    B, _, H, W = t.shape
    if layout == "packed":
        return t.cuda()
    if layout == "pair":  # pair 1 of a [B,3,2,H,W] tensor; the pairs around it hold NaN
        wide = torch.full((B, 3, 2, H, W), float("nan"))
        wide[:, 1] = t
        return wide.cuda()[:, 1]
    if layout == "channel":  # channels 1 and 3 of a [B,5,H,W] tensor
        wide = torch.full((B, 5, H, W), float("nan"))
        wide[:, 1::2] = t
        v = wide.cuda()[:, 1::2]
        assert v.stride(1) == 2 * H * W
        return v
    buf = torch.zeros(t.numel() + 1, dtype=torch.float32, device="cuda")  # "offset": packed, four bytes past an aligned address
    buf[1:] = t.reshape(-1).cuda()
    v = buf[1:].view(B, 2, H, W)
    assert v.data_ptr() % 16 == 4
    return v


def guarded(shape, dtype):
    """(the buffer, its interior view): 64 guard bytes on either side"""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((nbytes + 128,), GUARD, dtype=torch.uint8, device="cuda")
    return buf, buf[64:64 + nbytes].view(dtype).view(*shape)


def guards_intact(buf):
    return bool((buf[:64] == GUARD).all()) and bool((buf[-64:] == GUARD).all())


def out_shapes(B, H, W):
    i32 = torch.int32
    return {"out": ((B, H, W), torch.uint8), "track_id": ((B, 64), i32), "age": ((B, 64), i32), "next_id": ((B,), i32), "area": ((B, 64), i32),
            "bbox": ((B, 64, 4), i32), "moments": ((B, 64, 2), torch.int64), "slot_of_cur": ((B, 64), i32), "linked_cur": ((B, 64), i32),
            "table": ((B, 65, 65), i32), "warped": ((B, H, W), torch.uint8), "stats": ((B, 8), i32)}


def device_state(state):
    return None if state is None else [torch.from_numpy(np.ascontiguousarray(state[k], np.int32)).cuda() for k in ("track_id", "age", "next_id")]


def run(prev, cur, flow, state, shape, layout="packed", flow_layout="packed", skip=(), expect=0, mutate=None, iou_thresh=0.3, min_inter=1, min_area=1, max_age=2,
        carry=1):
    """one call; prev / cur / flow are NumPy arrays (laid out here), device views, or None; state a dict of arrays, a list of device tensors, or None.  Returns
    (dict of CPU arrays of the outputs not in `skip`, the message of a refusal, the device buffers); checks the guards around every output and the workspace"""
    B, H, W = shape
    pd, cd = (m if m is None or torch.is_tensor(m) else lay_out_map(m, layout) for m in (prev, cur))
    fd = flow if flow is None or torch.is_tensor(flow) else lay_out_flow(flow, flow_layout)
    sd = state if state is None or isinstance(state, list) else device_state(state)
    shapes = out_shapes(B, H, W)
    bufs = {k: guarded(*shapes[k]) for k in OUT if k not in skip}
    lib = _lib.get_lib()
    nbytes = int(lib.cwm_segment_track_work_bytes(B, H, W)) or 4096
    assert nbytes % 16 == 0
    work = torch.full((nbytes + 128,), GUARD, dtype=torch.uint8, device="cuda")
    assert (work.data_ptr() + 64) % 16 == 0
    a = _lib.new_segment_track_args()
    _lib.fill_patch_args(a.base, geometry=(B, 1, 0, H, W, 0), stream=_lib.current_stream_handle(torch.device("cuda:0")))
    if pd is not None:
        a.prev_dev, a.prev_stride = pd.data_ptr(), pd.stride(0)
    if cd is not None:
        a.cur_dev, a.cur_stride = cd.data_ptr(), cd.stride(0)
    if fd is not None:
        a.flow_dev = fd.data_ptr()
        a.flow_strides[0], a.flow_strides[1] = fd.stride(0), fd.stride(1)
    if sd is not None:
        a.track_id_in_dev, a.age_in_dev, a.next_id_in_dev = (t.data_ptr() for t in sd)
    a.iou_thresh, a.min_inter, a.min_area, a.max_age, a.carry = iou_thresh, min_inter, min_area, max_age, carry
    a.work_dev, a.work_bytes = work.data_ptr() + 64, nbytes
    a.out_stride = H * W
    for k in OUT:
        setattr(a, FIELD[k], bufs[k][1].data_ptr() if k in bufs else None)
    if mutate:
        mutate(a)
    rc = lib.cwm_segment_track(ctypes.byref(a))
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
    return out, msg, {k: v[1] for k, v in bufs.items()}


def equal(got, want, what=""):
    for k, v in got.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), (k, what)


_WANT = {}


def check(name, prev, cur, flow, state, shape=None, layout="packed", flow_layout="packed", skip=(), **kw):
    """against the restatement, computed once per (name, keywords) and left unchanged"""
    shape = shape or next(m for m in (prev, cur) if m is not None).shape
    key = (name, tuple(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _WANT:
        _WANT[key] = TR.track(prev, cur, flow, state, shape, **kw)
    got, _, _ = run(prev, cur, flow, state, shape, layout, flow_layout, skip=skip, **kw)
    equal(got, _WANT[key], (name, layout, flow_layout))
    return _WANT[key]


def test_hand_worked_case_and_state_hand_over():
    """the output of call 1 is the input of call 2 ON THE DEVICE, against two restatement steps"""
    prev, cur, flow, state = TR.hand_worked()
    for layout in MAP_LAYOUTS:
        for flow_layout in FLOW_LAYOUTS:
            w1 = check("hand", prev, cur, flow, state, layout=layout, flow_layout=flow_layout, **TR.HAND_KW)
    assert w1["stats"].tolist() == TR.HAND[0]["stats"] and w1["track_id"][0, :3].tolist() == TR.HAND[0]["track_id"]
    w2 = TR.track(w1["out"], cur, None, TR.new_state(w1), (1, 8, 12), **TR.HAND_KW)
    assert w2["stats"].tolist() == TR.HAND[1]["stats"] and w2["track_id"][0, :3].tolist() == TR.HAND[1]["track_id"]
    g1, _, d1 = run(prev, cur, flow, state, (1, 8, 12), **TR.HAND_KW)
    g2, _, _ = run(d1["out"], cur, None, [d1["track_id"], d1["age"], d1["next_id"]], (1, 8, 12), **TR.HAND_KW)
    equal(g1, w1)
    equal(g2, w2)


@pytest.mark.parametrize("kind", ["int", "half", "frac", "special"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_random_rectangles(H, W, kind):
    for i, B in enumerate((1, 3)):
        prev, cur, state = TR.random_maps(H * 7 + W + B, B, H, W, n_prev=6, n_cur=7)
        flow = TR.flows(kind, H + W + B, B, H, W)
        j = H + len(kind) + i
        want = check(("rects", H, W, kind, B), prev, cur, flow, state, layout=MAP_LAYOUTS[j % 3], flow_layout=FLOW_LAYOUTS[j % 4], iou_thresh=0.25)
        if B == 3:
            assert not np.array_equal(want["out"][0], want["out"][1])
    check(("rects-strict", H, W, kind), prev, cur, flow, state, layout="frame", flow_layout="channel", iou_thresh=0.25, min_inter=3, min_area=5, max_age=1)
    check(("rects-noflow", H, W, kind), prev, cur, None, state, layout="offset", iou_thresh=0.25)


@pytest.mark.parametrize("H,W", SHAPES)
def test_many_tracks_and_labels(H, W):
    prev, cur, state = TR.random_maps(H + W, 2, H, W, n_prev=40, n_cur=64)
    want = check(("many", H, W), prev, cur, TR.flows("int", 9, 2, H, W), state, iou_thresh=0.1, flow_layout="pair")
    assert want["stats"][:, 0].max() >= 2


def test_bytes_above_64_full_table_and_garbage_state():
    prev, cur, state = TR.random_maps(5, 2, 24, 40, big_bytes=False)
    prev[:, :3], cur[:, -3:] = 65, 255
    check("big-bytes", prev, cur, None, state)
    prev, cur, state = TR.full_table(2, 8, 64)
    assert check("full", prev, cur, None, state, max_age=5)["stats"][:, :6].tolist() == [[0, 0, 64, 0, 2, 64]] * 2
    assert check("full", prev, cur, None, state, carry=0)["stats"][:, :6].tolist() == [[0, 2, 0, 64, 0, 2]] * 2
    prev, cur, _ = TR.random_maps(13, 3, 24, 40)
    check("garbage", prev, cur, TR.flows("special", 5, 3, 24, 40), TR.garbage_state(1, 3), max_age=3)


def test_thresholds_ages_and_missing_inputs():
    prev, cur, state = TR.random_maps(11, 2, 24, 40, n_prev=6, n_cur=6)
    flow = TR.flows("int", 3, 2, 24, 40)
    nan = float("nan")
    assert check("thr", prev, cur, flow, state, iou_thresh=0.0)["stats"][:, 0].min() >= 1
    assert check("thr", prev, cur, flow, state, iou_thresh=nan)["stats"][:, 0].tolist() == [0, 0]
    assert check("thr", prev, cur, flow, state, iou_thresh=nan, max_age=0)["stats"][:, 2].tolist() == [0, 0]
    assert check("thr", prev, cur, flow, state, iou_thresh=nan, max_age=9)["stats"][:, 2].min() >= 1
    assert check("thr", prev, cur, flow, state, iou_thresh=nan, max_age=9, carry=0)["stats"][:, 2].tolist() == [0, 0]
    check("thr", prev, cur, flow, state, iou_thresh=0.9, min_inter=0, min_area=0)
    check("no-cur", prev, None, flow, state)
    check("no-prev", None, cur, flow, state)
    a = check("null-state", None, cur, None, None)
    b = check("zero-state", None, cur, None, TR.empty_state(2))
    equal(a, b)
    check("prev-no-state", prev, cur, flow, None)
    check("nothing", None, None, None, state, shape=(2, 24, 40))


def test_every_optional_output_null_in_turn():
    prev, cur, state = TR.random_maps(7, 3, 24, 40)
    flow = TR.flows("frac", 7, 3, 24, 40)
    for k in OUT:
        check("optional", prev, cur, flow, state, skip=(k,))
    check("optional", prev, cur, flow, state, skip=OUT[1:])
    check("optional", prev, cur, flow, state, skip=OUT[:-1])


def test_two_calls_give_the_same_bits():
    prev, cur, state = TR.random_maps(8, 3, 64, 64, n_prev=30, n_cur=30)
    flow = TR.flows("frac", 8, 3, 64, 64)
    a, _, _ = run(prev, cur, flow, state, (3, 64, 64), "frame", "pair")  # (every call fills its workspace with 0xA5 first)
    b, _, _ = run(prev, cur, flow, state, (3, 64, 64), "frame", "pair")
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in OUT)


def test_out_is_written_into_a_frame_in_place():
    prev, cur, state = TR.random_maps(9, 2, 20, 12)
    want = TR.track(prev, cur, None, state, (2, 20, 12))
    movie = torch.full((2, 3, 20, 12), 77, dtype=torch.uint8, device="cuda")
    got, _, _ = run(prev, cur, None, state, (2, 20, 12), skip=("out",),
                    mutate=lambda a: (setattr(a, "out_dev", movie[:, 1].data_ptr()), setattr(a, "out_stride", movie.stride(0))))
    equal(got, want)
    assert np.array_equal(movie[:, 1].cpu().numpy(), want["out"]) and bool((movie[:, 0] == 77).all()) and bool((movie[:, 2] == 77).all())


def test_limits_are_refused_with_the_field_named():
    lib = _lib.get_lib()
    z = np.zeros((1, 8, 12), np.uint8)

    def refused(field, shape=(1, 8, 12), maps=z, **kw):
        _, msg, _ = run(maps, maps, None, None, shape, expect=-1, **kw)
        assert msg.startswith("cwm_segment_track") and field in msg, (field, msg)

    dev = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")  # noqa: E731
    refused("base.batch = 0", mutate=lambda a: setattr(a.base, "batch", 0))
    refused("base.batch = 65536", mutate=lambda a: setattr(a.base, "batch", 65536))
    refused("base.H = 10", (1, 10, 12), dev(1, 10, 12))
    refused("base.W = 10", (1, 12, 10), dev(1, 12, 10))
    refused("base.H = 0", mutate=lambda a: setattr(a.base, "H", 0))
    refused("base.W = -4", mutate=lambda a: setattr(a.base, "W", -4))
    refused("base.H base.W", (1, 512, 516), dev(1, 512, 516))
    refused("max_age = -1", max_age=-1)
    refused("min_inter = -1", min_inter=-1)
    refused("min_area = -1", min_area=-1)
    refused("carry = 2", carry=2)
    refused("carry = -1", carry=-1)
    refused("no output", skip=OUT)
    refused("work_dev", mutate=lambda a: setattr(a, "work_dev", None))
    refused("work_dev", mutate=lambda a: setattr(a, "work_dev", a.work_dev + 8))
    refused("work_bytes", mutate=lambda a: setattr(a, "work_bytes", a.work_bytes - 1))
    refused("struct_size", mutate=lambda a: setattr(a, "struct_size", a.struct_size - 8))
    refused("prev_stride", mutate=lambda a: setattr(a, "prev_stride", -96))
    refused("cur_stride", mutate=lambda a: setattr(a, "cur_stride", -96))
    refused("flow_strides", mutate=lambda a: a.flow_strides.__setitem__(1, -96))
    refused("out_stride", mutate=lambda a: setattr(a, "out_stride", 95))
    some = torch.zeros(64, dtype=torch.int32, device="cuda")
    refused("track_id_in_dev", mutate=lambda a: setattr(a, "track_id_in_dev", some.data_ptr()))
    assert lib.cwm_segment_track_work_bytes(1, 8, 12) > 0
    for B, H, W in ((0, 8, 12), (1, 0, 12), (1, 8, -4), (1, 10, 12), (1, 8, 10), (1, 512, 516), (70000, 8, 12)):
        assert lib.cwm_segment_track_work_bytes(B, H, W) == 0, (B, H, W)


def test_largest_case():
    """512 x 512 (2^18 pixels), 64 slots and 64 labels: an 8 x 8 grid of 48 x 48 squares; label 65 - s lies one pixel off slot s's warped square both ways, so
    each pair shares 47 x 47 pixels and is linked: slot_of_cur reverses the numbering and every id is kept.  Held against the restatement's loop, run once."""
    prev, cur, flow, state = TR.largest()
    want = check("largest", prev, cur, flow, state, iou_thresh=0.5)
    assert want["stats"][0].tolist() == [64, 0, 0, 0, 0, 64, 64 * 48 * 48, 0] and want["slot_of_cur"][0].tolist() == list(range(64, 0, -1))
    assert want["table"][0, 64, 1] == 47 * 47 and want["area"][0].tolist() == [48 * 48] * 64 and np.array_equal(want["track_id"], state["track_id"])
    assert want["moments"][0, 63].tolist() == [48 * sum(range(453, 501)), 48 * sum(range(454, 502))]
