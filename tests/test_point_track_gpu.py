"""`cwm_point_track` on a real MI355X through the C ABI against the NumPy restatement (tests/point_track_restatement.py) and the torch composition, for EQUALITY:
state, under and owner by value, xy as int32 bit patterns, NaN included -- a fused multiply-add anywhere in the sample, the test or the coast shows here.

Shapes (B, T, H, W, K): (1,2,4,4,1) the smallest call (one thread of one wave, one step); (2,3,20,36,63) and (1,4,36,20,65) planes whose sides are no multiples
of 4 or of each other, one point short of a wave and one past it; (2,5,64,64,64) exactly one wave per row; (3,6,64,64,257) five workgroups per row, the last
with one live lane.  Every subset of the optional inputs, with max_coast 8, 1 and 0 in turn so that every state occurs.  The last shape also on [:, 1:] frame
slices of larger labels and model buffers, read in place, and on a points tensor four bytes off a 16-byte address."""
import ctypes

import numpy as np
import pytest
import torch

import point_track_restatement as R
from counterfactualworldmodels_amd import _lib, point_track as PT, segment_track as ST

pytestmark = pytest.mark.gpu
SHAPES = [(1, 2, 4, 4, 1), (2, 3, 20, 36, 63), (2, 5, 64, 64, 64), (1, 4, 36, 20, 65), (3, 6, 64, 64, 257)]
_CASES = {}


def case(shape):
    if shape not in _CASES:
        _CASES[shape] = R.case_passing() if shape == "passing" else R.case_random(*shape, seed=sum(shape))
    return _CASES[shape]


def dev(a):
    return None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).cuda())


def run(fwd, points, bwd=None, labels=None, model=None, start=None, alpha=0.01, beta=0.5, max_coast=8, expect=0, mutate=None, outs=None):
    """one call through the C ABI on device views.  Returns (dict of CPU arrays, the message)"""
    f, pts, bw, lab, mod, st = (dev(a) for a in (fwd, points, bwd, labels, model, start))
    B, T, H, W, K = f.shape[0], f.shape[1] + 1, f.shape[3], f.shape[4], pts.shape[1]
    if outs is None:
        outs = {"xy": torch.full((B, T, K, 2), -7.0, device="cuda"), "state": torch.full((B, T, K), 77, dtype=torch.uint8, device="cuda"),
                "under": torch.full((B, T, K), 77, dtype=torch.uint8, device="cuda"), "owner": torch.full((B, K), 77, dtype=torch.uint8, device="cuda")}
    before = {k: v.clone() for k, v in outs.items()}
    lib = _lib.get_lib()
    a = _lib.new_point_track_args()
    _lib.fill_patch_args(a.base, geometry=(B, T, 0, H, W, 0), stream=_lib.current_stream_handle(torch.device("cuda:0")))
    a.fwd_dev, a.bwd_dev, a.labels_dev, a.model_dev, a.points_dev, a.start_dev = (_lib.ptr(t) for t in (f, bw, lab, mod, pts, st))
    for strides, t, n in ((a.fwd_strides, f, 3), (a.bwd_strides, bw, 3), (a.labels_strides, lab, 2), (a.model_strides, mod, 2)):
        if t is not None:
            for i in range(n):
                strides[i] = t.stride(i)
    a.alpha, a.beta, a.K, a.max_coast = alpha, beta, K, max_coast
    a.xy_dev, a.state_dev, a.under_dev, a.owner_dev = (outs[k].data_ptr() for k in R.NAMES)
    if mutate:
        mutate(a)
    rc = lib.cwm_point_track(ctypes.byref(a))
    torch.cuda.synchronize()
    msg = lib.cwm_last_error().decode()
    assert rc == expect, (rc, msg)
    if expect:
        for k, v in outs.items():
            assert torch.equal(v, before[k]), "%s written by a refused call" % k
    return {k: v.cpu().numpy() for k, v in outs.items()}, msg


def equal(got, want, what=""):
    for k in R.NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, what, got[k].dtype, got[k].shape)
        assert np.array_equal(R.bits(got[k]), R.bits(want[k])), (k, what, np.argwhere(R.bits(got[k]) != R.bits(want[k]))[:4].tolist())


def fields(r):
    return {k: getattr(r, k).cpu().numpy() for k in R.NAMES}


@pytest.mark.parametrize("shape", ["passing"] + SHAPES)
def test_device_equals_restatement_equals_torch_with_each_subset_of_the_inputs(shape):
    c = case(shape)
    seen = np.zeros(256, np.int64)
    for i, sub in enumerate(R.SUBSETS):
        kw, mc = R.pick(c, **sub), (8, 1, 0)[i % 3]
        want = R.track(c["fwd"], c["points"], max_coast=mc, **kw)
        got, _ = run(c["fwd"], c["points"], max_coast=mc, **kw)
        equal(got, want, (sub, mc))
        seen += np.bincount(want["state"].ravel(), minlength=256)
    if shape != "passing" and shape[4] > 1:
        assert all(seen[v] > 0 for v in (0, 1, 2, 3, 255)), seen[[0, 1, 2, 3, 255]]
    # the module: the device call, the torch composition on the device and on the CPU
    on = {k: dev(v) for k, v in R.pick(c).items()}
    want = R.track(c["fwd"], c["points"], **R.pick(c))
    equal(fields(PT.track(dev(c["fwd"]), dev(c["points"]), **on)), want, "track")
    equal(fields(PT.track_torch(dev(c["fwd"]), dev(c["points"]), **on)), want, "track_torch on the device")
    equal(fields(PT.track(*(torch.from_numpy(c[k]) for k in ("fwd", "points")), **{k: None if v is None else v.cpu() for k, v in on.items()})), want, "cpu")


def test_passing_scene_on_the_device():
    c = case("passing")
    got, _ = run(c["fwd"], c["points"], **R.pick(c))
    assert got["state"][0, :, 0].tolist() == [0, 0, 0, 0, 0, 1, 1, 0] and got["xy"][0, :, 0, 0].tolist() == [12 + 4 * i for i in range(8)]
    got, _ = run(c["fwd"], c["points"])
    assert got["xy"][0, 5:, 0, 0].tolist() == [32, 32, 32] and not got["state"][0, :, 0].any()


def test_frame_slices_of_larger_buffers_are_read_in_place():
    shape = SHAPES[-1]
    c = case(shape)
    B, T, H, W, K = shape
    g = np.random.default_rng(5)
    labels = torch.from_numpy(np.concatenate([g.integers(0, 256, (B, 1, H, W)).astype(np.uint8), c["labels"]], 1)).cuda()
    model = torch.from_numpy(np.concatenate([g.uniform(-9, 9, (B, 1, 65, 12)), c["model"]], 1)).cuda()
    fwd = torch.from_numpy(np.concatenate([g.uniform(-9, 9, (B, 1, 2, H, W)).astype(np.float32), c["fwd"]], 1)).cuda()
    bwd = torch.from_numpy(np.concatenate([c["bwd"], g.uniform(-9, 9, (B, 1, 2, H, W)).astype(np.float32)], 1)).cuda()
    lab, mod, f, bw = labels[:, 1:], model[:, 1:], fwd[:, 1:], bwd[:, :-1]
    assert not lab.is_contiguous() and not mod.is_contiguous() and not f.is_contiguous() and not bw.is_contiguous()
    want = R.track(c["fwd"], c["points"], **R.pick(c))
    got, _ = run(f, c["points"], bwd=bw, labels=lab, model=mod, start=c["start"])
    equal(got, want, "slices")
    r = PT.track(f, dev(c["points"]), bwd=bw, labels=lab, model=mod, start=dev(c["start"]))
    equal(fields(r), want, "slices through the module")


def test_points_off_a_16_byte_address():
    c = case(SHAPES[-1])
    pts = torch.from_numpy(c["points"])
    buf = torch.zeros((pts.numel() + 8,), dtype=torch.float32).cuda()
    buf[1:1 + pts.numel()] = pts.reshape(-1).cuda()
    off = buf[1:1 + pts.numel()].view(*pts.shape)
    assert off.data_ptr() % 16 == 4
    want = R.track(c["fwd"], c["points"], **R.pick(c))
    got, _ = run(c["fwd"], off, **R.pick(c))
    equal(got, want, "off alignment")
    equal(fields(PT.track(dev(c["fwd"]), off, **{k: dev(v) for k, v in R.pick(c).items()})), want, "off alignment through the module")


def test_two_calls_give_equal_bits_and_every_output_byte_is_written():
    c = case(SHAPES[-1])
    one, _ = run(c["fwd"], c["points"], **R.pick(c))
    B, T, K = one["state"].shape
    outs = {"xy": torch.full((B, T, K, 2), 3.0, device="cuda"), "state": torch.full((B, T, K), 9, dtype=torch.uint8, device="cuda"),
            "under": torch.full((B, T, K), 9, dtype=torch.uint8, device="cuda"), "owner": torch.full((B, K), 9, dtype=torch.uint8, device="cuda")}
    two, _ = run(c["fwd"], c["points"], outs=outs, **R.pick(c))
    three, _ = run(c["fwd"], c["points"], outs=outs, **R.pick(c))  # (into what the second call left)
    equal(two, one)
    equal(three, one)
    # a device start outside 0 .. T-1: the point is never started
    start = c["start"].copy()
    start[:, 1], start[:, 2] = T, -1
    got, _ = run(c["fwd"], c["points"], **dict(R.pick(c), start=start))
    equal(got, R.track(c["fwd"], c["points"], **dict(R.pick(c), start=start)), "starts outside")
    assert (got["state"][:, :, 1:3] == 255).all() and not got["owner"][:, 1:3].any()


def test_limits_are_refused_with_the_field_named():
    c = case(SHAPES[1])
    full = R.pick(c)

    def refused(field, **kw):
        _, msg = run(c["fwd"], c["points"], expect=-1, **{**full, **kw})
        assert msg.startswith("cwm_point_track") and field in msg, (field, msg)

    refused("struct_size", mutate=lambda a: setattr(a, "struct_size", a.struct_size - 8))
    for name in ("xy_dev", "state_dev", "under_dev", "owner_dev", "fwd_dev", "points_dev"):
        refused(name, mutate=lambda a, name=name: setattr(a, name, None))
    refused("fwd_strides", mutate=lambda a: a.fwd_strides.__setitem__(1, -8))
    refused("bwd_strides", mutate=lambda a: a.bwd_strides.__setitem__(2, -8))
    refused("labels_strides", mutate=lambda a: a.labels_strides.__setitem__(0, -8))
    refused("model_strides", mutate=lambda a: a.model_strides.__setitem__(1, -8))
    refused("K = 0", mutate=lambda a: setattr(a, "K", 0))
    refused("K = 65537", mutate=lambda a: setattr(a, "K", 65537))
    refused("base.T = 1", mutate=lambda a: setattr(a.base, "T", 1))
    refused("base.T = 4097", mutate=lambda a: setattr(a.base, "T", 4097))
    refused("base.batch = 0", mutate=lambda a: setattr(a.base, "batch", 0))
    refused("base.H = 0", mutate=lambda a: setattr(a.base, "H", 0))
    refused("base.H base.W", mutate=lambda a: (setattr(a.base, "H", 512), setattr(a.base, "W", 513)))
    refused("model_dev is given without labels_dev", labels=None)
    refused("max_coast = -1", max_coast=-1)
    for bad in (-0.5, float("nan"), float("inf")):
        refused("alpha", alpha=bad)
        refused("beta", beta=bad)


def test_track_sequence_with_points_on_the_device_equals_the_cpu():
    c = case("passing")
    fwd, bwd, labels, pts = (torch.from_numpy(c[k]) for k in ("fwd", "bwd", "labels", "points"))
    z = torch.zeros_like(fwd[:, :1])
    backs, fwds = torch.cat([z, bwd], 1), torch.cat([z, fwd], 1)
    cpu = ST.track_sequence(labels, backs, fwds, motion=True, points=pts)
    d = ST.track_sequence(labels.cuda(), backs.cuda(), fwds.cuda(), motion=True, points=pts.cuda())
    for k in ST.TrackedScene.__slots__:
        u, v = getattr(d, k), getattr(cpu, k)
        assert (u is None) == (v is None), k
        if torch.is_tensor(u):
            u = u.cpu()
            assert torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u, v.view(torch.int64) if v.dtype == torch.float64 else v), k
    equal(fields(d.points), fields(cpu.points), "points")
    assert d.points.xy.is_cuda and d.points.state[0, :, 0].tolist() == [0, 0, 0, 0, 0, 1, 1, 0]
