"""The parallax read-out without a GPU: `parallax.measure_torch` against the NumPy restatement (tests/parallax_restatement.py) for EQUALITY of bit patterns, the
pinned numbers of a three-plane scene, the host decisions (`slot_values`, `depth_order`, `agreement`), the refusals, the binding, and the two drivers that ask
the question -- `predict_video_and_flow` and `predict_imu_video_and_flow` -- on stand-in predictors that record their calls."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import parallax_restatement as R
from counterfactualworldmodels_amd import _lib, parallax as PX, segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = (1, 2, 3, 4, 5, 8, 64)  # both parities and every residue of the quartile indices (n - 1) mod 4


def fields(r):
    return {k: (None if getattr(r, k) is None else getattr(r, k).cpu().numpy()) for k in R.NAMES}


def equal(got, want, what=""):
    for k in R.NAMES:
        if want[k] is None or got[k] is None:
            assert want[k] is None and got[k] is None, (k, what)
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, what, got[k].dtype, want[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(R.bits(got[k]), R.bits(want[k])), (k, what, int((R.bits(got[k]) != R.bits(want[k])).sum()))


def build(case, S, Rr=2, H=8, W=16):
    if case == "planes":
        flows, labels, _ = R.case_planes(Rr, 16, 24, S)
        return flows, labels
    return getattr(R, "case_" + case)(Rr, H, W, S)


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("case", ["random", "ties", "hostile", "planes"])
def test_measure_torch_equals_the_restatement(case, S):
    flows, labels = build(case, S)
    dirs = R.dirs_of(S)
    if case == "ties":
        dirs = -dirs if S == 1 else dirs * np.where(np.arange(S) % 3 == 0, -1, 1)[:, None].astype(np.int32)  # reference motions of both signs: -0.0 and +0.0
    if case == "hostile":
        dirs[S - 1] = 0  # a sample whose reference motion is zero
    f, l = torch.from_numpy(flows), torch.from_numpy(labels)
    seen_nan = False
    for d in (dirs, None):
        for ref_slot in ((-1,) if d is not None else (-1, 0, 3)):
            for ms in sorted({1, S}):
                want = R.parallax(flows, d, labels, ref_slot=ref_slot, min_samples=ms)
                got = PX.measure_torch(f, None if d is None else torch.from_numpy(d), l, ref_slot=ref_slot, min_samples=ms)
                equal(fields(got), want, (case, S, d is not None, ref_slot, ms))
                seen_nan |= bool(np.isnan(want["par"]).any())
    if case == "hostile":
        assert seen_nan
    # without labels: no tables, the same maps
    want = R.parallax(flows, dirs)
    got = PX.measure_torch(f, torch.from_numpy(dirs))
    assert got.hist is None and got.slot_tab is None
    equal(fields(got), want, (case, S, "no labels"))


def test_the_ties_case_really_orders_signed_zeros():
    """-0.0 and +0.0 in different sample positions of one pixel: the stable order decides which one the median is"""
    flows, labels = R.case_ties(1, 8, 16, 5)
    dirs = R.dirs_of(5) * np.array([-1, 1, 1, -1, 1], np.int32)[:, None]
    want = R.parallax(flows, dirs, labels, min_samples=1)
    zero = want["par"] == 0
    signs = np.signbit(want["par"][zero])
    assert signs.any() and not signs.all()
    got = PX.measure_torch(torch.from_numpy(flows), torch.from_numpy(dirs), torch.from_numpy(labels), min_samples=1)
    equal(fields(got), want)


def test_optional_outputs_and_default_min_samples():
    flows, labels = R.case_random(1, 8, 16, 5)
    f, l, d = torch.from_numpy(flows), torch.from_numpy(labels), torch.from_numpy(R.dirs_of(5))
    full = PX.measure(f, d, l)
    assert torch.equal(full.cnt, PX.measure(f, d, l, min_samples=3).cnt) and full.dirs.dtype == torch.int32
    part = PX.measure(f, d, l, want_spread=False, want_off=False)
    assert part.spread is None and part.off is None and torch.equal(part.par.view(torch.int32), full.par.view(torch.int32)) and torch.equal(part.hist, full.hist)


def test_three_planes_pinned():
    S = 8
    flows, labels, dirs = R.case_planes(2, 32, 40, S)
    f, l = torch.from_numpy(flows), torch.from_numpy(labels)
    for kw in (dict(dirs=torch.from_numpy(dirs)), dict(dirs=None, ref_slot=0)):
        r = PX.measure(f, labels=l, **kw)
        for slot, k in ((0, 1.0), (1, 2.0), (2, 3.0)):
            region = l == slot
            assert region.any() and (r.par[region] == k).all(), (slot, kw)
        assert (r.spread == 0).all() and (r.off == 0).all() and (r.cnt == S).all()
        assert r.ref[..., 3].min() == 1.0 and r.ref[0, 0].tolist() == [8 * 256.0, 0.0, (8 * 256.0) ** 2, 1.0]
        tab = r.slot_tab
        assert tab[:, :3, 2].tolist() == [[160, 192, 224]] * 2 and tab[:, :3, 1].tolist() == [[0, 0, 0]] * 2 and tab[:, 3:, 0].sum() == 0
        assert tab[:, :3, 0].sum(1).tolist() == [32 * 40] * 2 and (tab[:, 3:, 2:7] == -1).all() and (tab[:, :3, 2:7] == tab[:, :3, 2:3]).all()
        assert int(r.hist.sum()) == 2 * 32 * 40 and r.hist[0, 1, 192] == tab[0, 1, 0]
        vals = PX.slot_values(tab)
        assert vals[0, :3, 0].tolist() == [1.015625, 2.015625, 3.015625] and torch.isnan(vals[0, 3:]).all()
        nearer, rank = PX.depth_order(tab)
        assert np.argwhere(nearer[0].numpy()).tolist() == [[1, 0], [2, 0], [2, 1]] and rank[:, :4].tolist() == [[2, 1, 0, 0]] * 2 and rank.dtype == torch.int32
        assert not PX.depth_order(tab, min_pixels=10 ** 6)[0].any()
        # the other ordinal cue: slot 1 was hidden behind 2 (agrees), 2 behind 1 (contradicts), 1 behind 5, which has no pixel (silent)
        behind = torch.zeros((2, 65, 65), dtype=torch.bool)
        behind[:, 1, 2] = behind[:, 2, 1] = behind[:, 1, 5] = True
        assert PX.agreement(nearer, behind).tolist() == [[1, 1, 1]] * 2
        behind[1] = False
        behind[1, 1, 2] = True
        assert PX.agreement(nearer, behind).tolist() == [[1, 1, 1], [1, 0, 0]]


def test_a_rotation_gives_a_flat_map():
    """every pixel moves alike: one bin, nobody nearer than anybody"""
    S = 4
    flows, labels, dirs = R.case_planes(1, 16, 24, S)
    flows[:] = flows[:, :, :1, :1]
    r = PX.measure(torch.from_numpy(flows), None, torch.from_numpy(labels), ref_slot=0)
    assert (r.par == 1).all() and not PX.depth_order(r.slot_tab)[0].any()


def test_refusals_name_the_field():
    flows, labels = R.case_random(2, 8, 16, 4)
    f, l = torch.from_numpy(flows), torch.from_numpy(labels)

    def refused(word, *a, **kw):
        with pytest.raises(ValueError, match=word):
            PX.measure(*a, **kw)

    refused("flows must be", f[:, :1])
    refused("flows must be", f[0])
    refused("multiples of 4", f[:, :, :6])
    refused("multiples of 4", torch.zeros(1, 2, 512, 516, 1))
    refused("S = 65", torch.zeros(1, 2, 4, 4, 65))
    refused("dirs", f, torch.zeros(3, 2))
    refused("dirs", f, torch.full((4, 2), 0.5))
    refused("dirs entries", f, torch.tensor([[0, 8], [4097, 0], [0, 1], [1, 0]]))
    refused("dirs entries", f, [[0, 8], [0, -4097], [0, 1], [1, 0]])
    refused("labels must be", f, None, l[:1])
    refused("uint8", f, None, l.to(torch.int32))
    refused("ref_slot", f, None, None, 0)
    refused("ref_slot", f, None, l, 65)
    refused("min_pixels", f, min_pixels=0)
    refused("min_ref", f, min_ref=0.0)
    refused("min_ref", f, min_ref=float("nan"))
    refused("min_ref", f, min_ref=9000.0)
    refused("min_samples", f, min_samples=5)
    refused("min_samples", f, min_samples=0)
    for fn, word in ((PX.slot_values, "slot_tab"), (PX.depth_order, "slot_tab")):
        with pytest.raises(ValueError, match=word):
            fn(torch.zeros(2, 65, 7, dtype=torch.int32))
    with pytest.raises(ValueError, match="nearer and behind"):
        PX.agreement(torch.zeros(65, 65, dtype=torch.bool), torch.zeros(1, 65, 65, dtype=torch.bool))
    with pytest.raises(ValueError, match="num_anchors"):
        PX.lattice_anchors(4, 4, 17)
    # a view that torch can express is taken as it is; a bool map reads as bytes
    r = PX.measure(f.permute(0, 1, 3, 2, 4).contiguous().permute(0, 1, 3, 2, 4), None, l > 2, ref_slot=1)
    equal(fields(r), R.parallax(flows, None, (labels > 2).astype(np.uint8), ref_slot=1))


def test_lattice_anchors():
    assert PX.lattice_anchors(4, 4, 9) == [0, 2, 3, 8, 10, 11, 12, 14, 15] and PX.lattice_anchors(4, 4, 1) == [10] and PX.lattice_anchors(28, 28, 4) == [203, 217, 595, 609]
    assert len(set(PX.lattice_anchors(28, 28, 9))) == 9 and PX.lattice_anchors(3, 5, 5) == [0, 2, 4, 5, 7]


def test_binding_and_header():
    a = _lib.new_parallax_args()
    base = ctypes.sizeof(_lib.CwmPatchErrorArgs)
    assert a.struct_size == ctypes.sizeof(_lib.CwmParallaxArgs) and a.base.struct_size == base and _lib.CwmParallaxArgs.base.offset == 8
    names = [f[0] for f in _lib.CwmParallaxArgs._fields_]
    assert names[:2] == ["struct_size", "base"] and "stream" not in names  # the stream is base.stream
    assert "cwm_parallax" in _lib.SIGNATURES
    src = open(os.path.join(ROOT, "include", "cwm_hip.h")).read()
    body = src[src.index("typedef struct cwm_parallax_args"):src.index("} cwm_parallax_args;")]
    declared = [line.split(";")[0].split()[-1].split("[")[0].lstrip("*") for line in body.splitlines()[1:] if ";" in line and not line.lstrip().startswith(("*", "/*"))]
    assert declared == names, (declared, names)
    assert "TIES BROKEN BY THE SAMPLE INDEX" in src and "-0.0 and +0.0 compare equal" in src
    lib = _lib.get_lib()  # argument errors need no device
    a.struct_size -= 4
    assert lib.cwm_parallax(ctypes.byref(a)) != 0 and b"struct_size" in lib.cwm_last_error()
    a = _lib.new_parallax_args()
    a.base.batch, a.base.H, a.base.W, a.S = 1, 8, 10, 1
    assert lib.cwm_parallax(ctypes.byref(a)) != 0 and b"base.W = 10" in lib.cwm_last_error()


# ---- the drivers on stand-ins ------------------------------------------------------------------------------------------------------------------------------------
class VideoStub(torch.nn.Module):
    """a predictor of the geometry of a 32 x 32, patch 8, two-frame model; called as predictor(x [B,T,C,H,W], mask, **kw) it returns the video 10 x + 1 + t and
    records what it was given"""
    patch_size, image_size, num_frames, mask_size = (1, 8, 8), (32, 32), 2, (2, 4, 4)
    t_dim, c_dim = 1, 2

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, x, mask, *a, **kw):
        self.calls.append((x.clone(), mask.clone(), dict(kw)))
        return 10 * x + 1 + torch.arange(x.shape[1], dtype=x.dtype).view(1, -1, 1, 1, 1)


class HeadStub(VideoStub):
    """the flow -> IMU model: [B,4,12] from the movie, so that a static movie and a moving one give different head motions"""
    context_stream = types.SimpleNamespace(encoder=types.SimpleNamespace(num_tokens=4), patch_size=(2,))
    get_context_input = types.SimpleNamespace(num_channels=6)

    def forward(self, x, mask=None, **kw):
        self.calls.append((x.clone(), None if mask is None else mask.clone(), dict(kw)))
        motion = (x[:, 1] - x[:, 0]).mean((1, 2, 3)) + x[:, 0].mean((1, 2, 3))
        return motion.view(-1, 1, 1) + torch.arange(48, dtype=x.dtype).view(1, 4, 12)


class FlowStub:
    """flow_model(video [B,T,C,H,W], backward=...) -> [B,T-1,2,H,W]: the frame differences of two channels; records the videos and the keywords"""

    def __init__(self):
        self.calls, self.iters = [], None

    def set_iters(self, iters):
        self.iters = iters

    def __call__(self, video, backward=False, **kw):
        self.calls.append((video.clone(), backward, dict(kw)))
        return video[:, 1:, :2] - video[:, :-1, :2]


def movie(B, T, seed=0):
    return torch.rand((B, T, 3, 32, 32), generator=torch.Generator().manual_seed(seed))


def frame_mask(B):
    return (torch.arange(32) >= 16)[None].expand(B, -1).clone()  # frame 1 masked


def test_predict_video_and_flow():
    pred, fm = VideoStub(), FlowStub()
    G = segmentation.FlowGenerator(predictor=pred, flow_model=fm, temporal_dim=1)
    x, mask = movie(2, 4), frame_mask(2)
    x0 = x.clone()
    ctx = torch.ones(2, 3)
    y, f = G.predict_video_and_flow(x, mask, x_context=ctx, iters=5, flow_init="warm")
    assert torch.equal(x, x0) and tuple(y.shape) == (2, 4, 3, 32, 32) and tuple(f.shape) == (2, 3, 2, 32, 32)
    # frame slicing: window t is x[:, t:t+2], its frame 1 is the prediction; frame 0 of the result is the input's
    assert len(pred.calls) == 3 and all(torch.equal(c[0], x[:, t:t + 2]) and torch.equal(c[1], mask) for t, c in enumerate(pred.calls))
    assert torch.equal(y[:, 0], x[:, 0]) and all(torch.equal(y[:, t + 1], 10 * x[:, t + 1] + 2) for t in range(3))
    # keyword routing: the predictor sees x_context and no flow keyword, the flow model the other way round (iters goes through set_iters)
    assert all(set(c[2]) == {"x_context"} and torch.equal(c[2]["x_context"], ctx) for c in pred.calls)
    assert len(fm.calls) == 3 and all(c[2] == {"flow_init": "warm"} and c[1] is False for c in fm.calls) and fm.iters == 5
    # propagate_error=False: every pair is (the true frame t, the predicted frame t+1)
    for t, c in enumerate(fm.calls):
        assert torch.equal(c[0], torch.stack([x[:, t], y[:, t + 1]], 1))
        assert torch.equal(f[:, t], y[:, t + 1, :2] - x[:, t, :2])
    # propagate_error=True: ONE flow call on the predicted movie; raft_iters is iters; backward is passed on; the defaults are the generator's input and mask
    fm.calls.clear()
    G.set_input(x, mask=mask)
    y2, f2 = G.predict_video_and_flow(backward=True, propagate_error=True, raft_iters=7)
    assert torch.equal(y2, y) and len(fm.calls) == 1 and torch.equal(fm.calls[0][0], y) and fm.calls[0][1] is True and fm.calls[0][2] == {} and fm.iters == 7
    assert torch.equal(f2, y[:, 1:, :2] - y[:, :-1, :2])
    assert all(c[2] == {} for c in pred.calls[3:])


def imu_generator():
    pred, head, fm = VideoStub(), HeadStub(), FlowStub()
    draws = []

    def mask_generator(x):
        draws.append(x.shape[0])
        return frame_mask(x.shape[0])

    G = segmentation.ImuConditionedFlowGenerator(predictor=pred, head_motion_predictor=head, flow_model=fm, temporal_dim=1, mask_generator=mask_generator)
    return G, pred, head, fm, draws


def test_predict_imu_video_and_flow():
    G, pred, head, fm, draws = imu_generator()
    assert G.num_head_tokens == 4 and G.head_tubelet_size == 2 and G.head_motion_channels == 6
    x, mask = movie(2, 2, seed=3), frame_mask(2)
    static = x[:, :1].expand(-1, 2, -1, -1, -1)
    h_video, h_static = head.forward(x), head.forward(static)
    head.calls.clear()
    assert not torch.equal(h_video, h_static)
    reshaped = G.head_motion_generator.reshape_output
    given = torch.rand(2, 6, 8)
    # precedence 1: the argument, forwarded as it is; the head-motion predictor is not asked, static_head_motion does not matter
    y, f = G.predict_imu_video_and_flow(x, mask, head_motion=given, static_head_motion=True, iters=3)
    assert not head.calls and not draws and len(pred.calls) == 1 and len(fm.calls) == 1 and fm.iters == 3
    kw = pred.calls[0][2]
    assert set(kw) == {"x_context", "mask_context"} and torch.equal(kw["x_context"], given) and kw["mask_context"].dtype == torch.bool
    assert tuple(kw["mask_context"].shape) == (2, 4) and not kw["mask_context"].any() and torch.equal(pred.calls[0][1], mask)
    assert torch.equal(y, torch.cat([x[:, :1], 10 * x[:, 1:] + 2], 1)) and torch.equal(f, y[:, 1:, :2] - x[:, :1, :2]) and fm.calls[0][2] == {}
    assert G.forward(x, mask, head_motion=given, return_head_motion=True) is given and len(pred.calls) == 1
    # precedence 2: the static movie's head motion; 3: the movie's own.  Both go through reshape_output; return_head_motion returns them before it
    for static_flag, want, seen in ((True, h_static, static), (False, h_video, x)):
        pred.calls.clear(), head.calls.clear()
        h = G.predict_imu_video_and_flow(x, mask, static_head_motion=static_flag, return_head_motion=True)
        assert torch.equal(h, want) and not pred.calls and len(head.calls) == 1 and torch.equal(head.calls[0][0], seen)
        assert head.calls[0][2]["x_context"].abs().sum() == 0 and head.calls[0][2]["mask_context"].all() and head.calls[0][2]["output_context"] is True
        y2, _ = G(x, mask, static_head_motion=static_flag, timestamps="ts")
        assert torch.equal(pred.calls[0][2]["x_context"], reshaped(want)) and tuple(reshaped(want).shape) == (2, 6, 8) and pred.calls[0][2]["timestamps"] == "ts"
        # (the reference hands the timestamps to the estimate from the video, segmentation.py:908, and not to the static one, :906)
        assert head.calls[1][2]["timestamps"] == (None if static_flag else "ts") and torch.equal(y2, y)
    # mask_head_motion: an all-masked context; mask=None draws one mask; return_flow=False does not run the flow model
    pred.calls.clear(), fm.calls.clear()
    y3, f3 = G.predict_imu_video_and_flow(x, head_motion=given, mask_head_motion=True, return_flow=False, iters=9)
    assert draws == [2] and pred.calls[0][2]["mask_context"].all() and set(pred.calls[0][2]) == {"x_context", "mask_context"} and torch.equal(G.mask, mask)
    assert f3 is None and not fm.calls and torch.equal(y3, y)
    # the flow model never saw the predictor's keywords
    G.predict_imu_video_and_flow(x, mask, head_motion=given, flow_init="w")
    assert fm.calls[-1][2] == {"flow_init": "w"}


def test_ego_motion_flows_on_head_motions_composes_rows():
    """[S,C,L] head motions: '(b s)' rows of predict_imu_video_and_flow, chunked by sample_batch_size with equal results; the caller's RNG state is untouched"""
    G, pred, head, fm, draws = imu_generator()
    x = movie(2, 2, seed=5)
    hm = torch.rand(3, 6, 8)
    state = torch.get_rng_state()
    flows, dirs = G.ego_motion_flows(x, head_motions=hm)
    assert torch.equal(torch.get_rng_state(), state) and dirs is None and tuple(flows.shape) == (2, 2, 32, 32, 3) and draws == [2]
    assert len(pred.calls) == 1 and torch.equal(pred.calls[0][2]["x_context"], hm.repeat(2, 1, 1)) and torch.equal(pred.calls[0][0], x.repeat_interleave(3, 0))
    want = (10 * x[:, 1, :2] + 2 - x[:, 0, :2])[..., None].expand(-1, -1, -1, -1, 3)
    assert torch.equal(flows, want)
    pred.calls.clear()
    chunked, _ = G.ego_motion_flows(x, head_motions=hm[None].expand(2, -1, -1, -1), sample_batch_size=4)
    assert [c[0].shape[0] for c in pred.calls] == [4, 2] and torch.equal(chunked, flows)
    with pytest.raises(ValueError, match="head_motions"):
        G.ego_motion_flows(x, head_motions=torch.rand(3, 3, 6, 8))
    plain = segmentation.FlowGenerator(predictor=VideoStub(), flow_model=FlowStub(), temporal_dim=1)
    with pytest.raises(ValueError, match="IMU-conditioned"):
        plain.ego_motion_flows(x, head_motions=hm)
