"""`cwm_object_motion` on a real MI355X through the C ABI against the NumPy restatement (tests/object_motion_restatement.py), for EQUALITY: the integer tables by
value, the model as int64 bit patterns -- a fused multiply-add or a reciprocal anywhere in the fit shows here.

Shapes: 8 x 12 (the smallest legal plane with both sides different, one wave, most lanes past the plane), 64 x 64 with three rows (four workgroups per row),
24 x 40 (the last workgroup is partial), 512 x 512 once (the limit: 256 workgroups per row, sums beyond 2^32).  Label layouts: blocks with stray pixels (mixed
waves, runs that end inside a lane), whole image rows of one slot (every wave holds one slot: the wave sum alone; or two: the wave sum and per-lane adds), a label
change at every pixel with all 64 slots live (per-lane adds for all lanes but the first's).  Inputs packed,
as [:, :-1] / [:, 1:] slices of [2,3,..] buffers, and four bytes off their alignment (the narrow loads)."""
import ctypes

import numpy as np
import pytest
import torch

import object_motion_restatement as R
from counterfactualworldmodels_amd import _lib, object_motion as OM, segment_track as ST

pytestmark = pytest.mark.gpu
FIELD = dict(sums="sums_dev", counts="counts_dev", model="model_dev", occ="occ_dev")


def dev(a):
    return None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).cuda())


def as_bt(t):
    """[R,..] -> [R,1,..]: B = R rows of T = 1"""
    return None if t is None else t.unsqueeze(1)


def run(labels, flow, code=None, other=None, min_pixels=1, min_affine=16, min_det=1.0, expect=0, mutate=None, prefill=True, want_occ=None, outs=None):
    """one call on [B,T,H,W] / [B,T,2,H,W] device views (3- / 4-dimensional inputs are taken as T = 1).  Returns (dict of CPU arrays [R,..], the message)"""
    lab, fl, cod, oth = dev(labels), dev(flow), dev(code), dev(other)
    if lab.dim() == 3:
        lab, fl, cod, oth = as_bt(lab), as_bt(fl), as_bt(cod), as_bt(oth)
    B, T, H, W = lab.shape
    Rr = B * T
    if outs is None:
        i_fill, f_fill = (-9, float("nan")) if prefill else (0, 0.0)
        outs = {"sums": torch.full((Rr, 65, 16), i_fill, dtype=torch.int64, device="cuda"), "counts": torch.full((Rr, 65, 4), i_fill, dtype=torch.int32, device="cuda"),
                "model": torch.full((Rr, 65, 12), f_fill, dtype=torch.float64, device="cuda")}
        if (oth is not None) if want_occ is None else want_occ:
            outs["occ"] = torch.full((Rr, 65, 65), i_fill, dtype=torch.int32, device="cuda")
    before = {k: v.clone() for k, v in outs.items()}
    lib = _lib.get_lib()
    a = _lib.new_object_motion_args()
    _lib.fill_patch_args(a.base, geometry=(B, T, 0, H, W, 0), stream=_lib.current_stream_handle(torch.device("cuda:0")))
    a.labels_dev, a.flow_dev, a.code_dev, a.other_dev = (_lib.ptr(t) for t in (lab, fl, cod, oth))
    for strides, t in ((a.labels_strides, lab), (a.code_strides, cod), (a.other_strides, oth)):
        if t is not None:
            strides[0], strides[1] = t.stride(0), t.stride(1)
    a.flow_strides[0], a.flow_strides[1], a.flow_strides[2] = fl.stride(0), fl.stride(1), fl.stride(2)
    a.min_pixels, a.min_affine, a.min_det = min_pixels, min_affine, min_det
    for k, f in FIELD.items():
        setattr(a, f, outs[k].data_ptr() if k in outs else None)
    if mutate:
        mutate(a)
    rc = lib.cwm_object_motion(ctypes.byref(a))
    torch.cuda.synchronize()
    msg = lib.cwm_last_error().decode()
    assert rc == expect, (rc, msg)
    if expect:
        for k, v in outs.items():
            assert torch.equal(v.view(torch.int64) if k == "model" else v, before[k].view(torch.int64) if k == "model" else before[k]), "%s written by a refused call" % k
    return {k: v.cpu().numpy() for k, v in outs.items()}, msg


def equal(got, want, what=""):
    for k in R.NAMES:
        if want[k] is None:
            assert k not in got, (k, what)
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, what, got[k].dtype, got[k].shape)
        assert np.array_equal(R.bits(got[k]), R.bits(want[k])), (k, what, int((R.bits(got[k]) != R.bits(want[k])).sum()))


def check(labels, flow, code=None, other=None, what="", **kw):
    want = R.motion(labels, flow, code, other, **{k: v for k, v in kw.items() if k.startswith("min_")})
    got, _ = run(labels, flow, code, other, **kw)
    equal(got, want, what)
    return want


def test_smallest_plane():
    labels, flow, code, other = R.case_random(1, 8, 12, seed=11, reach=3.0)
    w = check(labels, flow, code, other, what="8x12")
    assert w["counts"].sum() == 96 and (w["counts"].sum(1) > 0)[0, :3].all()
    check(labels, flow, what="8x12 bare")


def test_random_labels_and_hostile_flows_with_and_without_code_and_other():
    labels, flow, code, other = R.case_random(3, 64, 64)
    assert (labels > 64).any() and np.isnan(flow).any() and np.isinf(flow).any() and (flow == 5000).any() and (flow == -4096.5).any()
    w = check(labels, flow, code, other, what="all")
    assert (w["counts"][:, :, :3].sum(1) > 100).all() and w["occ"].sum() == w["counts"][:, :, 1].sum() and (w["model"][..., 0] == 2).sum() > 50
    assert w["counts"][:, 0, 0].min() > 0 and (w["occ"][:, np.arange(65), np.arange(65)].sum() > 0)  # slot 0 is summed; the diagonal is counted
    for c, o in ((None, None), (code, None), (None, other)):
        w = check(labels, flow, c, o, what=(c is None, o is None))
        if c is None:
            assert not w["counts"][:, :, 1].any() and (o is None or not w["occ"].any())
    check(labels, flow, code, other, min_pixels=40, min_affine=60, min_det=300.0, what="thresholds")


def test_a_wave_of_one_slot_and_a_wave_of_sixty_four():
    labels, flow, code, other = R.case_rows(2, 64, 64)
    w = check(labels, flow, code, other, what="rows")
    assert (w["counts"][:, :32].sum(2) == 128).all()  # 64 columns: a wave holds four whole image rows, and the slot changes every two
    labels, flow, code, other = R.case_rows(2, 64, 256)
    labels = np.ascontiguousarray(labels[:, :16])
    check(labels, flow[:, :, :16], code[:, :16], other[:, :16], what="rows, 256 columns: every wave holds one slot")
    labels, flow, code, other = R.case_checker(2, 64, 64)
    w = check(labels, flow, code, other, what="checker")
    assert (w["counts"].sum(2) > 0).all() and (w["model"][..., 0] == 2).all()


def test_slices_of_larger_buffers_are_read_in_place():
    labels, _, _, _ = R.case_random(6, 64, 64, seed=21, top=64)
    labels = dev(labels.reshape(2, 3, 64, 64))
    _, flow, code, _ = R.case_random(6, 64, 64, seed=22)
    flow, code = dev(flow.reshape(2, 3, 2, 64, 64)), dev(code.reshape(2, 3, 64, 64))
    a, o, f, c = labels[:, :-1], labels[:, 1:], flow[:, 1:], code[:, 1:]
    assert not a.is_contiguous() and not o.is_contiguous() and not f.is_contiguous()
    got, _ = run(a, f, c, o)
    flat = lambda t: t.contiguous().reshape((4,) + tuple(t.shape[2:])).cpu().numpy()  # noqa: E731
    equal(got, R.motion(flat(a), flat(f), flat(c), flat(o)), "slices")
    packed, _ = run(a.contiguous(), f.contiguous(), c.contiguous(), o.contiguous())
    equal(got, {k: packed.get(k) for k in R.NAMES}, "slices against packed")


def test_inputs_off_their_alignment_take_the_narrow_loads():
    labels, flow, code, other = R.case_random(2, 24, 40, seed=31)

    def shifted(a, n):
        t = torch.from_numpy(a)
        buf = torch.zeros((t.numel() + 2 * n + 3,), dtype=t.dtype).cuda()
        buf[n:n + t.numel()] = t.reshape(-1).cuda()
        v = buf[n:n + t.numel()].view(*t.shape)
        return v

    fl, lab, cod = shifted(flow, 1), shifted(labels, 1), shifted(code, 2)
    assert fl.data_ptr() % 16 == 4 and lab.data_ptr() % 4 == 1
    want = R.motion(labels, flow, code, other)
    for L, F, C in ((lab, flow, code), (labels, fl, code), (labels, flow, cod), (lab, fl, cod)):
        got, _ = run(L, F, C, other)
        equal(got, want, "off alignment")


def test_the_limit_512_x_512():
    H = W = 512
    labels = np.ones((1, H, W), np.uint8)
    flow = np.empty((1, 2, H, W), np.float32)
    flow[:, 0], flow[:, 1] = 4096, -4096
    w = check(labels, flow, what="all outside")
    assert w["counts"][0, 1].tolist() == [0, 0, 1 << 18, 0] and not w["sums"].any() and not w["model"].any()
    flow[:, 0], flow[:, 1] = 0.00390625, 0
    w = check(labels, flow, what="one 256th")
    assert w["sums"][0, 1, 0] == (1 << 18) - H and w["sums"][0, 1, 6] == (1 << 18) - H and w["model"][0, 1, 1] == 0.00390625  # (the last column leaves the frame)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    flow[0, 0], flow[0, 1] = np.where(xs < 256, 511 - xs, -xs), np.where(ys < 256, 511 - ys, -ys)  # the largest flows that stay inside
    w = check(labels, flow, what="largest inside flow")
    assert w["counts"][0, 1, 0] == 1 << 18 and w["sums"][0, 1, 12] > 1 << 32 and abs(int(w["sums"][0, 1, 8])) > 1 << 32


def test_the_call_zeroes_its_own_outputs_and_two_calls_give_equal_bits():
    labels, flow, code, other = R.case_random(3, 64, 64, seed=9)
    fresh, _ = run(labels, flow, code, other, prefill=False)
    outs = {"sums": torch.full((3, 65, 16), -9, dtype=torch.int64, device="cuda"), "counts": torch.full((3, 65, 4), -9, dtype=torch.int32, device="cuda"),
            "model": torch.full((3, 65, 12), float("nan"), dtype=torch.float64, device="cuda"), "occ": torch.full((3, 65, 65), -9, dtype=torch.int32, device="cuda")}
    one, _ = run(labels, flow, code, other, outs=outs)
    two, _ = run(labels, flow, code, other, outs=outs)  # (into what the first call left)
    for k in R.NAMES:
        assert np.array_equal(R.bits(one[k]), R.bits(two[k])) and np.array_equal(R.bits(one[k]), R.bits(fresh[k])), k
    equal(one, R.motion(labels, flow, code, other))


def test_limits_are_refused_with_the_field_named():
    z = np.zeros((1, 8, 12), np.uint8)
    f = np.zeros((1, 2, 8, 12), np.float32)

    def refused(field, labels=z, flow=f, code=None, other=None, **kw):
        _, msg = run(labels, flow, code, other, expect=-1, **kw)
        assert msg.startswith("cwm_object_motion") and field in msg, (field, msg)

    refused("struct_size", mutate=lambda a: setattr(a, "struct_size", a.struct_size - 8))
    refused("base.H = 10", np.zeros((1, 10, 12), np.uint8), np.zeros((1, 2, 10, 12), np.float32))
    refused("base.W = 10", np.zeros((1, 12, 10), np.uint8), np.zeros((1, 2, 12, 10), np.float32))
    refused("base.H base.W", mutate=lambda a: (setattr(a.base, "H", 512), setattr(a.base, "W", 516)))
    refused("base.batch = 0", mutate=lambda a: setattr(a.base, "batch", 0))
    refused("base.T = 0", mutate=lambda a: setattr(a.base, "T", 0))
    refused("base.T = 65536", mutate=lambda a: setattr(a.base, "T", 65536))
    refused("labels_dev", mutate=lambda a: setattr(a, "labels_dev", None))
    refused("flow_dev", mutate=lambda a: setattr(a, "flow_dev", None))
    refused("occ_dev is given without other_dev", want_occ=True)
    refused("other_dev is given without occ_dev", other=z, want_occ=False)
    refused("min_pixels = 0", min_pixels=0)
    refused("min_affine = 2", min_affine=2)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("min_det", min_det=bad)
    refused("labels_strides", mutate=lambda a: a.labels_strides.__setitem__(0, -96))
    refused("flow_strides", mutate=lambda a: a.flow_strides.__setitem__(2, -96))
    refused("code_strides", code=z, mutate=lambda a: a.code_strides.__setitem__(1, -96))
    refused("other_strides", other=z, mutate=lambda a: a.other_strides.__setitem__(0, -96))
    refused("sums_dev", mutate=lambda a: setattr(a, "sums_dev", None))
    refused("counts_dev", mutate=lambda a: setattr(a, "counts_dev", None))
    refused("model_dev", mutate=lambda a: setattr(a, "model_dev", None))


def same_fields(d, c):
    for k in OM.ObjectMotion.__slots__:
        u, v = getattr(d, k), getattr(c, k)
        assert (u is None) == (v is None), k
        if u is not None:
            u = u.cpu()
            assert u.dtype == v.dtype and u.shape == v.shape, k
            assert torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u, v.view(torch.int64) if v.dtype == torch.float64 else v), k


def test_measure_on_the_device_equals_measure_on_the_cpu():
    labels, flow, code, other = (torch.from_numpy(a) for a in R.case_random(6, 64, 64, seed=13))
    labels, flow, code, other = labels.view(2, 3, 64, 64), flow.view(2, 3, 2, 64, 64), code.view(2, 3, 64, 64), other.view(2, 3, 64, 64)
    same_fields(OM.measure(labels.cuda(), flow.cuda(), code=code.cuda(), other=other.cuda()), OM.measure(labels, flow, code=code, other=other))
    same_fields(OM.measure(labels[:, 0].cuda(), flow[:, 0].cuda(), min_affine=40), OM.measure(labels[:, 0], flow[:, 0], min_affine=40))
    L = labels.cuda()
    d = OM.measure(L[:, :-1], flow.cuda()[:, 1:], code=code.cuda()[:, 1:], other=L[:, 1:])
    same_fields(d, OM.measure(labels[:, :-1], flow[:, 1:], code=code[:, 1:], other=labels[:, 1:]))
    assert tuple(d.model.shape) == (2, 2, 65, 12) and tuple(d.occluders.shape) == (2, 2, 65, 65)


def test_track_sequence_with_motion_on_the_device_equals_the_cpu():
    A, B, fwd, back = (torch.from_numpy(a) for a in R.translation_scene())
    backs, fwds = torch.stack([torch.zeros_like(back), back], 1), torch.stack([torch.zeros_like(fwd), fwd], 1)
    c = ST.track_sequence([A, B], backs, fwds, motion=True)
    d = ST.track_sequence([A.cuda(), B.cuda()], backs.cuda(), fwds.cuda(), motion=True)
    for k in ST.TrackedScene.__slots__:
        u, v = getattr(d, k), getattr(c, k)
        assert (u is None) == (v is None), k
        if u is not None:
            u = u.cpu()
            assert torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u, v.view(torch.int64) if v.dtype == torch.float64 else v), k
    assert int(d.occluders[0, 0, 1, 2]) == 64 and int(d.occluders[0, 0, 0, 1]) == 64 and d.motion[0, 0, 1, :3].tolist() == [2.0, 8.0, 0.0]
    assert not d.motion[:, 1].any() and not d.occluders[:, 1].any() and not d.motion_counts[:, 1].any()
