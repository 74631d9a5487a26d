"""`cwm_parallax` on a real MI355X through the C ABI against the NumPy restatement (tests/parallax_restatement.py), for EQUALITY: the integer tables by value, the
float maps and the reference table as bit patterns, NaN positions included.

Shapes: 4 x 4 with S = 1 and R = 1 (the smallest plane: sixteen pixels of one wave), 8 x 12 with R = 3 (96 pixels: a partial last workgroup in every kernel form),
64 x 64 on every case x three flow layouts x S = 3, 8, 64 (the pixel kernel's (256, 8) and (64, 64) forms; S = 12 and 24 take the two in between), 512 x 512 once
at S = 8 (the limit).  Flows as the sample-outer view of a [(r s),1,2,H,W] tensor (wide loads in the reference kernel), packed [R,2,H,W,S], and a slice of a
larger buffer four bytes off its alignment (the scalar form).  Every output starts from garbage.  Then the Python layers on the device: `measure` against its CPU
copy, the drivers `ego_motion_flows` and `parallax` under a table flow model against the loop composed by hand, and one run with the package's RAFT at random
weights."""
import ctypes

import numpy as np
import pytest
import torch

import parallax_restatement as R
from counterfactualworldmodels_amd import _lib, parallax as PX

pytestmark = pytest.mark.gpu
FIELD = dict(par="par_dev", spread="spread_dev", off="off_dev", cnt="cnt_dev", ref="ref_dev", hist="hist_dev", slot_tab="slot_tab_dev")
DTYPE = dict(par=torch.float32, spread=torch.float32, off=torch.float32, cnt=torch.uint8, ref=torch.float64, hist=torch.int32, slot_tab=torch.int32)
INT_OF = {torch.float32: torch.int32, torch.float64: torch.int64}


def dev(a):
    return None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).cuda())


def new_outs(Rr, H, W, S, prefill=True):
    shape = dict(par=(Rr, H, W), spread=(Rr, H, W), off=(Rr, H, W), cnt=(Rr, H, W), ref=(Rr, S, 4), hist=(Rr, 65, 256), slot_tab=(Rr, 65, 8))
    fill = lambda k: (float("inf") if DTYPE[k].is_floating_point else (247 if k == "cnt" else -9)) if prefill else 0  # noqa: E731
    return {k: torch.full(shape[k], fill(k), dtype=DTYPE[k], device="cuda") for k in FIELD}


def as_bits(t):
    return t.view(INT_OF[t.dtype]) if t.dtype in INT_OF else t


def run(flows, dirs=None, labels=None, ref_slot=-1, min_pixels=1, min_ref=0.25, min_samples=None, expect=0, mutate=None, prefill=True, outs=None, drop=()):
    """one call: flows [R,2,H,W,S] in whatever strides they have, labels a [R,H,W] view with contiguous planes.  `drop`: outputs passed as NULL.  Returns (dict of
    CPU arrays -- None for what was dropped or, without labels, not written --, the message)"""
    fl, di, lab = dev(flows), dev(dirs), dev(labels)
    Rr, _, H, W, S = fl.shape
    if outs is None:
        outs = new_outs(Rr, H, W, S, prefill)
    before = {k: v.clone() for k, v in outs.items()}
    lib = _lib.get_lib()
    a = _lib.new_parallax_args()
    _lib.fill_patch_args(a.base, geometry=(Rr, 1, 0, H, W, 0), stream=_lib.current_stream_handle(torch.device("cuda:0")))
    a.flows_dev, a.S = fl.data_ptr(), S
    for i in range(5):
        a.flow_strides[i] = fl.stride(i)
    a.dirs_dev, a.labels_dev, a.labels_stride = _lib.ptr(di), _lib.ptr(lab), 0 if lab is None else lab.stride(0)
    a.ref_slot, a.min_pixels, a.min_ref_q, a.min_samples = ref_slot, min_pixels, R.min_ref_q_of(min_ref), (S + 1) // 2 if min_samples is None else min_samples
    for k, f in FIELD.items():
        setattr(a, f, None if k in drop else outs[k].data_ptr())
    if mutate:
        mutate(a)
    rc = lib.cwm_parallax(ctypes.byref(a))
    torch.cuda.synchronize()
    msg = lib.cwm_last_error().decode()
    assert rc == expect, (rc, msg)
    untouched = set(FIELD) if expect else set(drop) | ({"hist", "slot_tab"} if lab is None else set())
    for k in untouched:
        assert torch.equal(as_bits(outs[k]), as_bits(before[k])), "%s written by a call that may not write it" % k
    return {k: (None if k in untouched else v.cpu().numpy()) for k, v in outs.items()}, msg


def equal(got, want, what="", skip=()):
    for k in R.NAMES:
        if k in skip:
            continue
        if want[k] is None:
            assert got[k] is None, (k, what)
            continue
        assert got[k] is not None and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, what)
        assert np.array_equal(R.bits(got[k]), R.bits(want[k])), (k, what, int((R.bits(got[k]) != R.bits(want[k])).sum()))


def sample_outer(flows):
    """the `_batch_to_samples` view of a [(r s),1,2,H,W] device tensor holding flows [R,2,H,W,S]"""
    f = dev(flows)
    Rr, _, H, W, S = f.shape
    out = f.permute(0, 4, 1, 2, 3).contiguous().reshape(Rr * S, 1, 2, H, W)
    v = out[:, 0].reshape(Rr, S, 2, H, W).movedim(1, -1)
    assert v.data_ptr() == out.data_ptr() and v.stride() == (S * 2 * H * W, H * W, W, 1, 2 * H * W)
    return v


def sliced(t, n=1):
    """the same values and strides as a slice of a larger buffer, the base n elements off"""
    size = t.untyped_storage().nbytes() // t.element_size()
    buf = torch.zeros((size + n + 4,), dtype=t.dtype, device="cuda")
    buf[n:n + size] = torch.as_strided(t, (size,), (1,), 0)
    return torch.as_strided(buf, t.shape, t.stride(), n + t.storage_offset())


def layouts(flows):
    outer = sample_outer(flows)
    off = sliced(outer)
    assert outer.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    return (("sample-outer", outer), ("packed", dev(flows)), ("a slice off its alignment", off))


def check(flows, dirs=None, labels=None, what="", **kw):
    """the restatement once, then the three flow layouts against it"""
    want = R.parallax(flows, dirs, labels, **kw)
    for name, f in layouts(flows):
        got, _ = run(f, dirs, labels, **kw)
        equal(got, want, (what, name))
    return want


def hostile_dirs(S):
    d = R.dirs_of(S)
    d[S - 1] = 0  # a sample whose reference motion is zero
    return d


def test_smallest_plane():
    flows = np.zeros((1, 2, 4, 4, 1), np.float32)
    flows[0, 0, :, :, 0] = np.arange(16, dtype=np.float32).reshape(4, 4) / 2 - 3
    flows[0, 1, 1, 1, 0] = np.nan
    labels = np.zeros((1, 4, 4), np.uint8)
    labels[0, 2:] = 7
    w = check(flows, np.array([[0, 2]], np.int32), labels, what="4x4 dirs")
    assert int(w["cnt"].sum()) == 15 and w["slot_tab"][0, 7, 0] == 8 and w["slot_tab"][0, 0, :2].tolist() == [7, 1] and w["par"][0, 0, 0] == -1.5
    check(flows, None, labels, ref_slot=7, what="4x4 ref_slot")
    check(flows, None, None, what="4x4 bare")


def test_partial_last_workgroup():
    for S in (2, 12, 24):  # (12 and 24: the pixel kernel's (256, 16) and (128, 32) forms)
        flows, labels = R.case_random(3, 8, 12, S, seed=12)
        w = check(flows, R.dirs_of(S), labels, what="8x12 S=%d" % S)
        assert w["hist"].sum() + w["slot_tab"][:, :, 1].sum() == 3 * 96 and w["hist"].sum() > 0
        check(flows, None, labels, ref_slot=0, min_pixels=3, min_ref=0.5, min_samples=S, what="8x12 thresholds S=%d" % S)


@pytest.mark.parametrize("S", [3, 8, 64])
@pytest.mark.parametrize("case", ["random", "ties", "hostile", "planes"])
def test_64_x_64(case, S):
    Rr, H, W = 2, 64, 64
    if case == "planes":
        flows, labels, dirs = R.case_planes(Rr, H, W, S)
    else:
        flows, labels = getattr(R, "case_" + case)(Rr, H, W, S)
        dirs = hostile_dirs(S) if case == "hostile" else R.dirs_of(S) * np.where(np.arange(S) % 3 == 0, -1, 1)[:, None].astype(np.int32)
    w = check(flows, dirs, labels, what=(case, S, "dirs"))
    n = check(flows, None, labels, ref_slot=0 if case == "planes" else 3, min_samples=1, what=(case, S, "ref_slot"))
    if case == "planes":
        for x in (w, n):
            assert x["slot_tab"][:, :3, 2].tolist() == [[160, 192, 224]] * Rr and not x["spread"].any() and (x["cnt"] == S).all()
    elif case == "ties":
        zero = w["par"] == 0
        assert np.signbit(w["par"][zero]).any() and not np.signbit(w["par"][zero]).all()
    elif case == "hostile":
        assert np.isnan(w["par"][0]).all() and w["ref"][0, :, 3].sum() == S - 1 and w["ref"][1, S - 1, 3] == 0 and (labels > 64).any()
        assert n["ref"][0, :, 3].sum() == 0 and n["ref"][1, :, 3].sum() == 0  # an unusable row; a row without a pixel of slot 3
    else:
        assert w["hist"].sum() > 0.9 * Rr * H * W and (w["slot_tab"][:, :6, 0] > 0).all()


def test_the_limit_512_x_512():
    H = W = 512
    S = 8
    flows, labels, dirs = R.case_planes(1, H, W, S)
    flows[0, :, 100, 200:260, :5] = np.inf
    want = R.parallax(flows, None, labels, ref_slot=0)
    assert want["slot_tab"][0, :3, 2].tolist() == [160, 192, 224] and int(want["slot_tab"][0, :, 1].sum()) == 60 and int(want["hist"].sum()) == H * W - 60
    got, _ = run(sample_outer(flows), None, labels, ref_slot=0)
    equal(got, want, "512x512")


def test_every_optional_output_in_turn_and_labels_with_a_row_stride():
    Rr, H, W, S = 2, 24, 40, 5
    flows, labels = R.case_random(Rr, H, W, S, seed=14)
    want = R.parallax(flows, None, labels, ref_slot=1)
    f = sample_outer(flows)
    for drop in (("spread",), ("off",), ("cnt",), ("spread", "off", "cnt")):
        got, _ = run(f, None, labels, ref_slot=1, drop=drop)
        equal(got, want, drop, skip=drop)
    bare = R.parallax(flows, R.dirs_of(S))
    got, _ = run(f, R.dirs_of(S), None)  # without labels the tables are not touched (run() checks it)
    equal(got, bare, "no labels")
    big = torch.zeros((Rr, 3, H, W), dtype=torch.uint8, device="cuda")
    big[:, 1] = dev(labels)
    for name, lab in (("[:, 1] of a larger buffer", big[:, 1]), ("one byte off", sliced(dev(labels)))):
        assert lab.stride(0) in (3 * H * W, H * W)
        got, _ = run(f, None, lab, ref_slot=1)
        equal(got, want, name)


def test_the_call_zeroes_its_own_tables_and_two_calls_give_equal_bits():
    flows, labels = R.case_random(2, 64, 64, 5, seed=9)
    f = sample_outer(flows)
    fresh, _ = run(f, None, labels, ref_slot=2, prefill=False)
    outs = new_outs(2, 64, 64, 5, prefill=True)
    one, _ = run(f, None, labels, ref_slot=2, outs=outs)
    two, _ = run(f, None, labels, ref_slot=2, outs=outs)  # (into what the first call left)
    for k in R.NAMES:
        assert np.array_equal(R.bits(one[k]), R.bits(two[k])) and np.array_equal(R.bits(one[k]), R.bits(fresh[k])), k
    equal(one, R.parallax(flows, None, labels, ref_slot=2))


def test_limits_are_refused_with_the_field_named():
    flows, labels = R.case_random(1, 8, 12, 2, seed=1)

    def refused(field, labels=labels, **kw):
        _, msg = run(flows, R.dirs_of(2), labels, expect=-1, **kw)
        assert msg.startswith("cwm_parallax") and field in msg, (field, msg)

    refused("struct_size", mutate=lambda a: setattr(a, "struct_size", a.struct_size - 8))
    refused("base.batch = 0", mutate=lambda a: setattr(a.base, "batch", 0))
    refused("base.batch = 65536", mutate=lambda a: setattr(a.base, "batch", 65536))
    refused("base.H = 10", mutate=lambda a: setattr(a.base, "H", 10))
    refused("base.W = 10", mutate=lambda a: setattr(a.base, "W", 10))
    refused("base.H = 0", mutate=lambda a: setattr(a.base, "H", 0))
    refused("base.H base.W", mutate=lambda a: (setattr(a.base, "H", 512), setattr(a.base, "W", 516)))
    refused("S = 0", mutate=lambda a: setattr(a, "S", 0))
    refused("S = 65", mutate=lambda a: setattr(a, "S", 65))
    for i in range(5):
        refused("flow_strides[%d]" % i, mutate=lambda a, i=i: a.flow_strides.__setitem__(i, -4))
    refused("labels_stride", mutate=lambda a: setattr(a, "labels_stride", -96))
    for f in ("flows_dev", "par_dev", "ref_dev", "hist_dev", "slot_tab_dev"):
        refused(f, mutate=lambda a, f=f: setattr(a, f, None))
    refused("ref_dev", mutate=lambda a: setattr(a, "ref_dev", a.ref_dev + 4))
    refused("hist_dev", mutate=lambda a: setattr(a, "hist_dev", a.hist_dev + 4))
    refused("ref_slot = -2", ref_slot=-2)
    refused("ref_slot = 65", ref_slot=65)
    refused("ref_slot = 0 needs labels_dev", labels=None, ref_slot=0)
    refused("min_pixels = 0", min_pixels=0)
    refused("min_ref_q = 0", min_ref=0.0)
    refused("min_ref_q", min_ref=8192.01)
    refused("min_samples = 0", min_samples=0)
    refused("min_samples = 3", min_samples=3)
    got, _ = run(flows, R.dirs_of(2), labels, ref_slot=64, min_ref=8192.0, min_samples=2)  # (the ends of the ranges are accepted)
    equal(got, R.parallax(flows, R.dirs_of(2), labels, ref_slot=64, min_ref=8192.0, min_samples=2))


def same_fields(d, c):
    for k in R.NAMES:
        u, v = getattr(d, k), getattr(c, k)
        if v is None:
            assert u is None, k
            continue
        assert u.is_cuda and u.dtype == v.dtype and u.shape == v.shape, k
        assert torch.equal(as_bits(u.cpu()), as_bits(v)), k


def test_measure_on_the_device_equals_measure_on_the_cpu():
    Rr, H, W, S = 2, 64, 64, 5
    flows, labels = (torch.from_numpy(a) for a in R.case_hostile(Rr, H, W, S, seed=13))
    dirs = torch.from_numpy(hostile_dirs(S))
    same_fields(PX.measure(sample_outer(flows.cuda()), dirs.cuda(), labels.cuda()), PX.measure(flows, dirs, labels))
    same_fields(PX.measure(flows.cuda(), None, labels.cuda(), ref_slot=0, min_samples=1, min_ref=1.0), PX.measure(flows, None, labels, ref_slot=0, min_samples=1, min_ref=1.0))
    d, c = PX.measure(flows.cuda(), want_spread=False, want_off=False), PX.measure(flows, want_spread=False, want_off=False)
    assert d.spread is None and d.off is None and d.hist is None
    same_fields(d, c)
    flows, labels, dirs = (torch.from_numpy(a) for a in R.case_planes(Rr, H, W, S))
    d = PX.measure(flows.cuda(), dirs.cuda(), labels.cuda())
    for got, want in zip(PX.depth_order(d.slot_tab), PX.depth_order(PX.measure(flows, dirs, labels).slot_tab)):
        assert got.is_cuda and torch.equal(got.cpu(), want)
    assert PX.depth_order(d.slot_tab)[1][0, :3].tolist() == [2, 1, 0] and PX.slot_values(d.slot_tab).is_cuda


# ---- the drivers -------------------------------------------------------------------------------------------------------------------------------------------------
NS = 5


@pytest.fixture(scope="module")
def tiny():
    from counterfactualworldmodels_amd import synthetic as S
    from test_object_response_gpu import TableFlow, tiny_generator

    flows, labels, dirs = R.case_planes(2, 32, 32, NS)
    fm = TableFlow(flows)
    G, cfg = tiny_generator(fm)
    x = torch.from_numpy(S.synthetic_frames(2, cfg, 3)).cuda()
    return G, fm, x, flows, labels, dirs


def test_the_pan_equals_the_loop_composed_by_hand(tiny):
    from counterfactualworldmodels_amd import segment_step as SS

    G, fm, x, flows, labels, dirs = tiny
    lab = torch.from_numpy(labels).cuda()
    x0, lab0 = x.clone(), lab.clone()
    torch.manual_seed(11)
    state = torch.get_rng_state()
    fm.calls = 0
    res = G.parallax(x, lab, num_samples=NS, num_anchors=4, shift=1)
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(x, x0) and torch.equal(lab, lab0) and fm.calls == 1
    assert res.par.is_cuda and tuple(res.par.shape) == (2, 32, 32) and tuple(res.nearer.shape) == (2, 65, 65) and res.rank[:, :3].tolist() == [[2, 1, 0]] * 2
    assert res.dirs.tolist() == dirs.tolist() == [[8 * dy, 8 * dx] for dy, dx in SS.directions(NS, 1)]
    # by hand: the lattice's cells moved together through the public counterfactual driver, the restatement on the same flows
    anchors = PX.lattice_anchors(4, 4, 4)
    assert anchors == [5, 7, 13, 15]
    active = torch.ones((2, 32), dtype=torch.bool, device="cuda")
    active[:, :16] = False
    active[:, [16 + a for a in anchors]] = False
    fm.calls = 0
    with torch.random.fork_rng(devices=[]):
        _, f = G.predict_counterfactual_videos_and_flows(x, active.unsqueeze(-1).expand(-1, -1, NS), None, shifts=SS.directions(NS, 1), num_samples=NS,
                                                         sample_batch_size=None, fix_passive=True)
    hand = G._batch_to_samples(f).cpu().numpy()
    assert np.array_equal(hand, flows) and fm.calls == 1
    want = R.parallax(hand, dirs, labels, ref_slot=0)
    equal({k: getattr(res, k).cpu().numpy() for k in R.NAMES}, want, "pan")
    # ego_motion_flows alone: the view of the flow model's output, the given anchors and shifts, chunked -- equal bits
    fm.calls = 0
    fl, d = G.ego_motion_flows(x, num_samples=NS, anchors=torch.tensor([anchors, anchors]), shift=1, sample_batch_size=3)
    assert fm.calls == 1 and torch.equal(d, res.dirs) and fl.data_ptr() == fm.last.data_ptr() and np.array_equal(fl.cpu().numpy(), flows)
    table, fm.table = fm.table, fm.table[:, :2].contiguous()  # (the table flow model serves as many samples as its table holds)
    fl2, d2 = G.ego_motion_flows(x, shifts=[(0, 2), (-1, 0)], num_anchors=9)
    fm.table = table
    assert d2.tolist() == [[0, 16], [-8, 0]] and tuple(fl2.shape) == (2, 2, 32, 32, 2) and np.array_equal(fl2.cpu().numpy(), flows[..., :2])
    with pytest.raises(ValueError, match="anchors"):
        G.ego_motion_flows(x, anchors=torch.tensor([[16], [0]]))


def test_head_motions_equal_the_loop_composed_by_hand():
    """a tiny conjoined predictor under S head motions: one predict_imu_video_and_flow row per (movie, head motion), whatever the chunking"""
    from test_conj_oracle import TINY_CONJ
    from test_head_motion_cpu import TINY_FLOW2IMU
    from test_head_motion_gpu import weights
    from test_object_response_gpu import TableFlow

    from counterfactualworldmodels_amd import conjoined_vmae as CV, masking, segmentation

    pred = CV.ConjoinedPaddedVisionTransformer(TINY_CONJ)
    pred.load_state_dict(weights(TINY_CONJ, 1))
    f2i = CV.ConjoinedPretrainVisionTransformer(TINY_FLOW2IMU)
    f2i.load_state_dict(weights(TINY_FLOW2IMU, 2))
    gen = masking.RotatedTableUniformMaskingGenerator(input_size=pred.mask_size, mask_ratio=0.9, clumping_factor=2)
    H = W = 32
    S, B = 3, 2
    table, labels, _ = R.case_planes(B, H, W, S)
    fm = TableFlow(table)
    G = segmentation.ImuConditionedFlowGenerator(predictor=pred, head_motion_predictor=f2i, flow_model=fm, temporal_dim=2, imagenet_normalize_inputs=True,
                                                 mask_generator=gen, seed=0).to("cuda")
    x = torch.rand((B, 2, 3, H, W), generator=torch.Generator().manual_seed(3)).cuda()
    hm = torch.randn((S, G.head_motion_channels, G.head_tubelet_size * G.num_head_tokens), generator=torch.Generator().manual_seed(4)).cuda()
    x0, hm0 = x.clone(), hm.clone()
    torch.manual_seed(5)
    state = torch.get_rng_state()
    seen = []
    inner = G.predict_imu_video_and_flow

    def recording(xs, **kw):
        seen.append((xs.clone(), kw["mask"].clone(), kw["head_motion"].clone()))
        return inner(xs, **kw)

    G.predict_imu_video_and_flow = recording
    flows, dirs = G.ego_motion_flows(x, head_motions=hm)
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(x, x0) and torch.equal(hm, hm0) and dirs is None and fm.calls == 1 and len(seen) == 1
    assert tuple(flows.shape) == (B, 2, H, W, S) and flows.data_ptr() == fm.last.data_ptr() and np.array_equal(flows.cpu().numpy(), table)
    xs, ms, hs = seen[0]
    assert torch.equal(xs, x.repeat_interleave(S, 0)) and torch.equal(hs, hm.repeat(B, 1, 1))
    assert all(torch.equal(ms[b * S + s], ms[b * S]) for b in range(B) for s in range(S))  # one mask per movie
    # by hand: the same rows through the public call; the head motion reaches its row -- two rows of one movie and one mask differ by it alone
    with torch.random.fork_rng(devices=[]):
        y, none = inner(xs, mask=ms, head_motion=hs, return_flow=False)
    assert none is None and fm.calls == 1 and torch.isfinite(y).all() and torch.equal(y[:, 0], xs[:, 0]) and (y[0, 1] - y[1, 1]).abs().max() > 0
    # chunked: two rows per call, three calls -- equal bits -- and the read-out on top
    rows = []

    class Chunks(torch.nn.Module):
        """the table flow model asked for the '(b s)' rows two at a time"""

        def forward(self, video, backward=False, **kw):
            flat = fm.table.reshape(B * S, 1, 2, H, W)
            lo = sum(rows)
            rows.append(video.shape[0])
            return flat[lo:lo + video.shape[0]]

    G.flow_model = Chunks()
    state = torch.get_rng_state()
    res = G.parallax(x, torch.from_numpy(labels).cuda(), head_motions=hm, sample_batch_size=2, min_samples=1)
    G.predict_imu_video_and_flow, G.flow_model = inner, fm
    assert rows == [2, 2, 2] and len(seen) == 4 and res.dirs is None and torch.equal(torch.get_rng_state(), state)
    assert torch.equal(torch.cat([c[0] for c in seen[1:]]), xs) and torch.equal(torch.cat([c[2] for c in seen[1:]]), hs) and torch.equal(torch.cat([c[1] for c in seen[1:]]), ms)
    want = R.parallax(table, None, labels, ref_slot=0, min_samples=1)
    equal({k: getattr(res, k).cpu().numpy() for k in R.NAMES}, want, "head motions")
    assert res.rank[:, :3].tolist() == [[2, 1, 0]] * B


def test_with_raft_at_random_weights():
    """128 x 128, patch 8, S = 4, two RAFT iterations.  Equality with the restatement on the flows read back is exact: every step is an integer operation or a
    single correctly rounded binary64 operation"""
    from counterfactualworldmodels_amd import config as C, segmentation, synthetic as S
    from test_raft_fast_gpu import build
    from test_spelke_segment_gpu import Recorder, predictor

    cfg = C.VmaeConfig(name="tiny_128", img_size=(128, 128), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
    G = segmentation.FlowGenerator(predictor=predictor(cfg), flow_model=Recorder(build(0)), imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
    x = torch.from_numpy(S.synthetic_frames(1, cfg, 5)).cuda()
    labels = R.plane_labels(1, 128, 128)
    res = G.parallax(x, torch.from_numpy(labels).cuda(), num_samples=4, raft_iters=2, min_samples=1)
    assert tuple(res.par.shape) == (1, 128, 128) and res.par.is_cuda and tuple(res.hist.shape) == (1, 65, 256) and res.dirs.tolist() == [[0, 16], [16, 0], [0, -16], [-16, 0]]
    flows = G._batch_to_samples(G.flow_model.last).cpu().numpy()  # the very same flows, read back
    want = R.parallax(flows, res.dirs.cpu().numpy(), labels, ref_slot=0, min_samples=1)
    print("[raft] pixels per slot %s, median bins %s, spread up to %.3f" % (want["slot_tab"][0, :3, 0].tolist(), want["slot_tab"][0, :3, 2].tolist(), np.nanmax(want["spread"])))
    assert int(want["hist"].sum()) == 128 * 128 and np.isfinite(want["par"]).all()
    equal({k: getattr(res, k).cpu().numpy() for k in R.NAMES}, want, "raft")
    # and every sample against its own mean flow
    got = PX.measure(G._batch_to_samples(G.flow_model.last), None, torch.from_numpy(labels).cuda(), ref_slot=0, min_ref=1 / 256)
    equal({k: getattr(got, k).cpu().numpy() for k in R.NAMES}, R.parallax(flows, None, labels, ref_slot=0, min_ref=1 / 256), "raft, no dirs")
