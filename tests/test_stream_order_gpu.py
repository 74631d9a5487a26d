"""Stream ordering of every stream-taking entry point of include/cwm_hip.h: the protocols of tests/stream_order.py -- A late inputs and early
consumers on a side stream, B a busy null stream under a call that allocates and zero-fills, C two calls back to back, D two caller streams chained by the
caller -- on the smallest shapes that still take each path.  Every comparison is `torch.equal` against the plain run of the same case (default stream, device
synchronised on either side).  A missed ordering reads NaN or another VALID mask / table / length: a wrong number, never a wild access.

The table of cases (which entry points, which protocols, which calls the header documents as not synchronising the host) is `stream_order.CASES`; every case
has one runner here (`RUNNERS`, checked at the end of the module), and tests/test_stream_order_cpu.py holds the table against the header.

Not here, on purpose: the RCCL entry points (they need several ranks; collectives are not exercised this way on a shared machine) and capture into a hipGraph
(a separate piece of work)."""
import ctypes

import numpy as np
import pytest
import torch

import stream_order as SO
from counterfactualworldmodels_amd import _lib, flowstats as FS, masking, sampling, segmentation, synthetic as S
from counterfactualworldmodels_amd.raft import RAFT, _args as raft_args
from oracle import vmae_oracle as V
from test_conj_oracle import TINY_CONJ, conj_weights
from test_dec0_tables_gpu import NT, build as vit_build, frames as vit_frames, masks as vit_masks, weights as vit_weights

pytestmark = pytest.mark.gpu
MODES = ("parity", "fast")
DEV = torch.device("cuda:0")
RUNNERS = {}


def case(name):
    """registers the test function(s) that run the table's case `name`"""
    def deco(fn):
        RUNNERS.setdefault(name, []).append(fn.__name__)
        return fn
    return deco


def stream():
    return _lib.current_stream_handle(DEV)


def cuda(ts):
    return [t.cuda() for t in ts]


def nan_of(ts):
    return [SO.poison_like(t) for t in ts]


def plain2(call, truth):
    """the plain run, twice (the first pays one-off set-up: a workspace, a lazily created stream or table): (outputs, wall time of the second)"""
    first, _ = SO.plain(call, [t.clone() for t in truth])
    want, ms = SO.plain(call, [t.clone() for t in truth])
    assert SO.same(first, want), "the plain run is not bit-stable run to run"
    return want, ms


def run_a(name, call, truth, poison, extra="", poison_runs=True, second=None, asynchronous=None):
    """protocol A of a case on device tensors `truth` with `poison`; with `second` = (truth2, poison2) also protocol C"""
    asyn = SO.CASES[name][2] if asynchronous is None else asynchronous
    want, ms = plain2(call, truth)
    SO.check_poison(name + extra, truth, poison, want, call, poison_runs)
    SO.protocol_a(name, call, truth, poison, want, ms, asyn, extra)
    if second is not None:
        assert "C" in SO.CASES[name][1]
        truth2, poison2 = second
        want2, _ = plain2(call, truth2)
        assert not SO.same(want, want2), name + extra + ": the two back-to-back calls have the same result"
        SO.protocol_c(name, call, truth, truth2, poison, poison2, want, want2, ms, asyn, extra)
    else:
        assert "C" not in SO.CASES[name][1] or extra
    return want, ms


# ---- the ViT predictor -------------------------------------------------------------------------------------------------------------------------------------
VIT_B, VIT_NVIS = 4, 11
RAGGED_COUNTS, RAGGED_RANGE = (9, 12, 7, 11), (7, 12)


def lanes_of(B, n_vis, lanes, min_rows):
    """cwm_forward's lane count (csrc/model.hip)"""
    n = 1
    while n < lanes and n < B and (B // (n + 1)) * n_vis >= min_rows:
        n += 1
    return n


def ragged_masks(counts, seed):
    m = torch.ones(len(counts), NT, dtype=torch.bool)
    for b, n in enumerate(counts):
        m[b, torch.randperm(NT, generator=torch.Generator().manual_seed(seed + b))[:n]] = False
    return m.cuda()


def vit_call(m, kind, check):
    if kind == "video":
        return lambda x, mask: m.predict_video(x, mask, n_vis=VIT_NVIS, check=check)
    if kind == "forward":  # the model seam: [B, C, T, H, W] frames, tokens only
        return lambda x, mask: m(x.transpose(1, 2), mask, n_vis=VIT_NVIS, check=check)
    return lambda x, mask: m.predict_video(x, mask, check=check, ragged=True, n_vis_range=RAGGED_RANGE)


def vit_inputs(kind, seed):
    """(truth, poison): frames with NaN, masks with another valid mask of the same counts (ragged: the same multiset of counts, all inside the handle's range)"""
    x = vit_frames(VIT_B, seed)
    if kind == "ragged":
        mask, bad = ragged_masks(RAGGED_COUNTS, 40 + seed), ragged_masks(RAGGED_COUNTS[1:] + RAGGED_COUNTS[:1], 80 + seed)
    else:
        mask, bad = vit_masks(VIT_B, VIT_NVIS, seed), vit_masks(VIT_B, VIT_NVIS, 50 + seed)
    return [x, mask], [SO.poison_like(x), bad]


@pytest.fixture(scope="module")
def vit_models():
    out = {}
    for mode in MODES:
        m = vit_build(vit_weights(3), mode, min_lane_rows=1)
        m.predict_video(vit_frames(VIT_B, 1), vit_masks(VIT_B, VIT_NVIS, 1))  # (creates the handle: set_lanes needs one)
        out[mode] = m
    return out


@case("vit")
@pytest.mark.parametrize("kind", ["video", "forward", "ragged"])
@pytest.mark.parametrize("lanes", [2, 1])
@pytest.mark.parametrize("mode", MODES)
def test_vit_late_inputs_and_back_to_back(vit_models, mode, lanes, kind):
    m = vit_models[mode]
    m.set_lanes(lanes)
    n_vis = RAGGED_RANGE[1] if kind == "ragged" else VIT_NVIS
    assert lanes_of(VIT_B, n_vis, lanes, 1) == lanes  # the case runs on the lane count it names
    extra = " %s %s lanes=%d" % (mode, kind, lanes)
    truth, poison = vit_inputs(kind, 2)
    run_a("vit", vit_call(m, kind, False), truth, poison, extra + " check=0", second=vit_inputs(kind, 5))
    run_a("vit", vit_call(m, kind, True), truth, poison, extra + " check=1", asynchronous=False)
    m.set_lanes(2)


@case("vit")
@pytest.mark.parametrize("mode", MODES)
def test_vit_two_caller_streams(vit_models, mode):
    m = vit_models[mode]
    m.set_lanes(2)
    assert lanes_of(VIT_B, VIT_NVIS, 2, 1) == 2
    call = vit_call(m, "video", False)
    (t1, p1), (t2, p2) = vit_inputs("video", 2), vit_inputs("video", 5)
    w1, ms = plain2(call, t1)
    w2, _ = plain2(call, t2)
    SO.protocol_d("vit", call, t1, t2, p1, p2, w1, w2, ms, " " + mode)


@case("vit")
@pytest.mark.parametrize("mode", MODES)
def test_vit_fresh_buffers_under_a_busy_null_stream(mode):
    """the FIRST forward of a handle whose weights are uploaded (workspace, mask-token table, split-K slabs), the first forward of a larger batch (the workspace
    regrows) and the first forward after load_state_dict (the table is rebuilt), each on a fresh non-blocking stream while the null stream is busy"""
    sd, sd2 = vit_weights(3), vit_weights(6)
    ref, ref2 = vit_build(sd, mode, min_lane_rows=1), vit_build(sd2, mode, min_lane_rows=1)
    call = lambda m: (lambda x, mask: m.predict_video(x, mask, n_vis=VIT_NVIS, check=False))  # noqa: E731
    x, mask = vit_frames(VIT_B, 2), vit_masks(VIT_B, VIT_NVIS, 2)
    x8, mask8 = vit_frames(2 * VIT_B, 7), vit_masks(2 * VIT_B, VIT_NVIS, 7)
    want, ms = plain2(call(ref), [x, mask])
    want8, ms8 = plain2(call(ref), [x8, mask8])
    want2, _ = plain2(call(ref2), [x, mask])
    assert not SO.same(want, want2)
    m = vit_build(sd, mode, min_lane_rows=1)
    m.sync_weights(DEV)  # (the handle and its weights: the upload synchronises the device by itself; no workspace yet)
    SO.protocol_b("vit", call(m), [x, mask], want, ms, " %s first forward of a fresh handle" % mode)
    SO.protocol_b("vit", call(m), [x8, mask8], want8, ms8, " %s larger batch: the workspace regrows" % mode)
    m.load_state_dict(sd2)
    m.sync_weights(DEV)
    SO.protocol_b("vit", call(m), [x, mask], want2, ms, " %s after load_state_dict: the table is rebuilt" % mode)


# ---- the IMU-conditioned model ------------------------------------------------------------------------------------------------------------------------------
CONJ_B, CONJ_VIS, CONJ_VIS_C = 4, 70, 3


def conj_build(ctx_stream, seed=17):
    from counterfactualworldmodels_amd import conjoined_vmae as CV

    m = CV.ConjoinedPaddedVisionTransformer(TINY_CONJ, mode="parity")
    m.load_state_dict(conj_weights(TINY_CONJ, seed))
    m = m.cuda().eval()
    m.set_option("min_lane_rows", 1)
    m.set_option("conj_ctx_stream", ctx_stream)
    return m


def conj_inputs(seed):
    """(truth, poison) of [frames, mask, imu, context mask]: every row with CONJ_VIS visible main tokens and CONJ_VIS_C visible context tokens, so that the wrapper
    is told the counts and reads nothing back"""
    def tables(s):
        gen = torch.Generator().manual_seed(s)
        mask = torch.ones(CONJ_B, TINY_CONJ.main.num_tokens, dtype=torch.bool)
        mc = torch.ones(CONJ_B, TINY_CONJ.ctx_tokens, dtype=torch.bool)
        for b in range(CONJ_B):
            mask[b, torch.randperm(mask.shape[1], generator=gen)[:CONJ_VIS]] = False
            mc[b, torch.randperm(mc.shape[1], generator=gen)[:CONJ_VIS_C]] = False
        return mask.cuda(), mc.cuda()

    x = V.preprocess(torch.from_numpy(S.synthetic_frames(CONJ_B, TINY_CONJ.main, seed))).cuda()
    imu = torch.randn(CONJ_B, TINY_CONJ.ctx_in_chans, TINY_CONJ.ctx_seq_len, generator=torch.Generator().manual_seed(seed)).cuda()
    (mask, mc), (mask_p, mc_p) = tables(seed), tables(seed + 100)
    return [x, mask, imu, mc], [SO.poison_like(x), mask_p, SO.poison_like(imu), mc_p]


def conj_call(m, check):
    return lambda x, mask, imu, mc: m(x, mask, x_context=imu, mask_context=mc, output_main=True, output_context=True, check=check, n_vis=CONJ_VIS,
                                      n_vis_context=CONJ_VIS_C)


@case("conj")
@pytest.mark.parametrize("ctx_stream", [1, 0])
def test_conj_all_protocols(ctx_stream):
    assert CONJ_B >= 2 and (CONJ_B // 2) * CONJ_VIS >= 1  # two lanes under min_lane_rows = 1 (csrc/conj_model.hip cwm_conj_forward)
    extra = " ctx_stream=%d" % ctx_stream
    m = conj_build(ctx_stream)
    (t1, p1), (t2, p2) = conj_inputs(3), conj_inputs(4)
    want, ms = run_a("conj", conj_call(m, False), t1, p1, extra + " check=0", second=(t2, p2))
    run_a("conj", conj_call(m, True), t1, p1, extra + " check=1", asynchronous=False)
    want2, _ = plain2(conj_call(m, False), t2)
    SO.protocol_d("conj", conj_call(m, False), t1, t2, p1, p2, want, want2, ms, extra)
    fresh = conj_build(ctx_stream)
    fresh.sync_weights(DEV)
    SO.protocol_b("conj", conj_call(fresh, False), t1, want, ms, extra + " first forward of a fresh handle")


# ---- RAFT ---------------------------------------------------------------------------------------------------------------------------------------------------
RAFT_ITERS = 2


@pytest.fixture(scope="module")
def raft_models():
    def build(output_dim):
        m = RAFT(raft_args(output_dim=output_dim))
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(0, output_dim=output_dim).items()})
        return m.cuda().eval()
    return {"flow": build(None), "keypoint": build(1)}


def raft_frames(B, H, W, seed):
    return torch.from_numpy(S.raft_frames(B, H, W, seed)).cuda()


def raft_call(m):
    return lambda x: m(x, iters=RAFT_ITERS)


@case("raft")
@pytest.mark.parametrize("head", ["flow", "keypoint"])
@pytest.mark.parametrize("corr", ["all_pairs", "on_the_fly"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", [(128, 128), (128, 160)])
def test_raft_late_inputs_and_back_to_back(raft_models, H, W, B, mode, corr, head):
    m = raft_models[head].set_mode(mode).set_corr(corr)
    x1, x2 = raft_frames(B, H, W, 1), raft_frames(B, H, W, 2)
    run_a("raft", raft_call(m), [x1], nan_of([x1]), " %s %dx%dx%d %s %s" % (head, B, H, W, mode, corr), second=([x2], nan_of([x2])))


@case("raft")
def test_raft_warm_start_late_inputs(raft_models):
    """cwm_raft_forward_ex: the frames and the initial flow both arrive late; the poison of the initial flow is another finite field"""
    m = raft_models["flow"].set_mode("parity").set_corr("all_pairs")
    x = raft_frames(1, 128, 128, 3)
    g = torch.Generator().manual_seed(1)
    init, init_p = (2.0 * torch.randn(1, 2, 16, 16, generator=g)).cuda(), (2.0 * torch.randn(1, 2, 16, 16, generator=g)).cuda()
    run_a("raft", lambda x, f: m(x, iters=RAFT_ITERS, flow_init=f), [x, init], [SO.poison_like(x), init_p], " flow_init")


@case("raft")
def test_raft_fresh_buffers_under_a_busy_null_stream(raft_models):
    """the first forward of a fresh handle, the first at another frame size and the first after set_corr: each re-plans the workspace (csrc/raft_model.hip
    ensure_workspace) and runs on a fresh non-blocking stream while the null stream is busy"""
    ref = raft_models["flow"].set_mode("parity").set_corr("all_pairs")
    x, xw = raft_frames(1, 128, 128, 1), raft_frames(1, 128, 160, 1)
    want, ms = plain2(raft_call(ref), [x])
    want_w, ms_w = plain2(raft_call(ref), [xw])
    ref.set_corr("on_the_fly")
    want_o, ms_o = plain2(raft_call(ref), [xw])
    ref.set_corr("all_pairs")
    m = RAFT()
    m.load_state_dict(ref.state_dict())
    m = m.cuda().eval()
    m.sync_weights(DEV)
    SO.protocol_b("raft", raft_call(m), [x], want, ms, " first forward of a fresh handle")
    SO.protocol_b("raft", raft_call(m), [xw], want_w, ms_w, " the frame size changes")
    m.set_corr("on_the_fly")
    SO.protocol_b("raft", raft_call(m), [xw], want_o, ms_o, " after set_corr")


# ---- RAFT's stand-alone kernels -------------------------------------------------------------------------------------------------------------------------------
@case("raft_forward_interpolate")
def test_raft_forward_interpolate_late_inputs():
    lib = _lib.get_lib()
    P, h, w = 2, 16, 19
    g = torch.Generator().manual_seed(2)
    flow = (3.0 * torch.randn(P, 2, h, w, generator=g)).cuda()

    def call(f):
        out = torch.empty(P, 2, h, w, device="cuda")
        _lib.check(lib.cwm_raft_forward_interpolate(f.data_ptr(), f.stride(0), f.stride(1), P, h, w, out.data_ptr(), stream()))
        return out
    # (a NaN source is invalid: the poison's plain run is the cold start, zeros)
    run_a("raft_forward_interpolate", call, [flow], nan_of([flow]))


@case("raft_convex_upsample")
@pytest.mark.parametrize("channels", [2, 1])
def test_raft_convex_upsample_late_inputs(channels):
    from test_raft_gpu import CONVEX_SHAPES

    lib = _lib.get_lib()
    P, h, w = CONVEX_SHAPES[1]
    g = torch.Generator().manual_seed(4)
    field = (3.0 * torch.randn(*((P, 2, h, w) if channels == 2 else (P, h, w)), generator=g)).cuda()
    mask = (2.0 * torch.randn(P, h, w, 576, generator=g)).cuda()
    fn = lib.cwm_raft_convex_upsample if channels == 2 else lib.cwm_raft_convex_upsample1

    def call(f, k):
        out = torch.empty(P, channels, 8 * h, 8 * w, device="cuda")
        _lib.check(fn(f.data_ptr(), k.data_ptr(), P, h, w, out.data_ptr(), stream()))
        return out
    run_a("raft_convex_upsample", call, [field, mask], nan_of([field, mask]), " %d channel(s)" % channels)


@case("raft_head_project")
def test_raft_head_project_late_inputs():
    lib = _lib.get_lib()
    g = torch.Generator().manual_seed(5)
    M = 2 * 3 * 5 + 3
    hidden, wgt, bias = (2.0 * torch.randn(M, 256, generator=g)).cuda(), torch.randn(256, generator=g).cuda(), torch.tensor([0.37]).cuda()

    def call(hd, wt, b):
        out = torch.empty(M, device="cuda")
        _lib.check(lib.cwm_raft_head_project(hd.data_ptr(), wt.data_ptr(), b.data_ptr(), M, out.data_ptr(), stream()))
        return out
    run_a("raft_head_project", call, [hidden, wgt, bias], nan_of([hidden, wgt, bias]))


@case("raft_corr_lookup")
@pytest.mark.parametrize("form", ["all_pairs", "on_the_fly"])
def test_raft_corr_lookup_late_inputs(form):
    """the 1 x 17 x 19 case of tests/test_raft_corr_gpu.py; the coordinates are index-like: their poison is another finite field"""
    from test_raft_corr_gpu import lookup_case

    lib = _lib.get_lib()
    P, h, w = 1, 17, 19
    f1, f2, coords = lookup_case(P, h, w, 5)
    coords_p = lookup_case(P, h, w, 6)[2]
    fn = lib.cwm_raft_corr_lookup if form == "all_pairs" else lib.cwm_raft_corr_lookup_on_the_fly

    def call(a, b, c):
        out = torch.empty(P, h, w, 324, device="cuda")
        _lib.check(fn(a.data_ptr(), b.data_ptr(), c.data_ptr(), P, h, w, out.data_ptr(), stream()))
        return out
    run_a("raft_corr_lookup", call, [f1, f2, coords], nan_of([f1, f2]) + [coords_p], " " + form)


# ---- flow statistics ------------------------------------------------------------------------------------------------------------------------------------------
def flow_samples(seed):
    """B = 2, S = 37, 24 x 40, as the flow model emits them: the sample-major batch [(b s), 2, H, W]; the calls take its [B, 2, H, W, S] view"""
    return torch.randn(2 * 37, 2, 24, 40, generator=torch.Generator().manual_seed(seed)).cuda()


def samples_view(raw):
    v = raw.view(2, 37, 2, 24, 40).permute(0, 2, 3, 4, 1)
    assert not v.is_contiguous()
    return v


@case("flow_corrs")
def test_flow_corrs_with_a_prologue_that_needs_the_work_buffer():
    call = lambda raw: FS.compute_flow_corrs(samples_view(raw), downsample=2, use_covariance=True, zscore=True, normalize=True)  # noqa: E731
    a, b = flow_samples(3), flow_samples(4)
    run_a("flow_corrs", call, [a], nan_of([a]), second=([b], nan_of([b])))


@case("flow_motion_map")
def test_flow_mean_motion_map_normalised_per_sample():
    call = lambda raw: FS.compute_mean_motion_map(samples_view(raw), normalize_per_sample=True)  # noqa: E731
    a, b = flow_samples(3), flow_samples(4)
    run_a("flow_motion_map", call, [a], nan_of([a]), second=([b], nan_of([b])))


@case("flow_features")
def test_flow_features():
    call = lambda raw: FS.flow_features(samples_view(raw), 2)  # noqa: E731
    a, b = flow_samples(3), flow_samples(4)
    run_a("flow_features", call, [a], nan_of([a]), second=([b], nan_of([b])))


# ---- the flow filter (also the filter step of sample_counterfactual_motion_map, which calls FlowSampleFilter.forward) -----------------------------------------
def filter_case(B, Sn, seed):
    """the recipe of tests/test_motion_sampling_gpu.py::test_filter_sizes_against_restatement: (the '(b s) 1 c h w' batch, the active mask), with one active patch
    of frame 2 per sample"""
    rng = np.random.Generator(np.random.PCG64(seed))
    size, grid = 224, 28
    blobs = np.zeros((B, Sn, 1, 5), dtype=np.float32)
    active = np.ones((B, 2 * grid * grid, Sn), dtype=bool)
    active[:, : grid * grid] = False
    for b in range(B):
        for s in range(Sn):
            py, px = rng.integers(grid, size=2)
            active[b, grid * grid + py * grid + px, s] = False
            blobs[b, s, 0] = ((py + 0.5) * 8 - 0.5, (px + 0.5) * 8 - 0.5, rng.uniform(10, 150), rng.uniform(-25, 25), rng.uniform(-25, 25))
    f = torch.from_numpy(S.blob_flow_samples(size, Sn, blobs)).cuda()
    return f.permute(0, 4, 1, 2, 3).reshape(B * Sn, 1, 2, size, size).contiguous(), torch.from_numpy(active).cuda()


@case("flow_filter")
@pytest.mark.parametrize("B,Sn", [(1, 1), (2, 5)])
def test_flow_filter_late_inputs_and_back_to_back(B, Sn):
    """(1, 1) is the smallest case of the restatement test (a contiguous view: statistics + in-place zeroing); (2, 5) is a strided view: the packing pass too"""
    def call(batch, act):
        view = segmentation.FlowGenerator.batch_to_samples(batch, t=0, B=B)
        filt = sampling.FlowSampleFilter()
        out, _ = filt(view, act)
        st = filt.last_stats
        return out, st["patch_mag"], st["area_count"], st["corner_count"], st["reject"]
    (f1, a1), (f2, a2) = filter_case(B, Sn, 1), filter_case(B, Sn, 2)
    assert not torch.equal(a1, a2)
    run_a("flow_filter", call, [f1, a1], [SO.poison_like(f1), a2], " B=%d S=%d" % (B, Sn), second=([f2, a2], [SO.poison_like(f2), a1]))


# ---- prompts ----------------------------------------------------------------------------------------------------------------------------------------------------
@case("shift_prompts")
def test_shift_prompts_late_inputs():
    from test_prompt_kernels_gpu import SHIFT_CASES, shift_tables

    lib = _lib.get_lib()
    sc = SHIFT_CASES[0]
    B, S_, T, Cc, H, W, P, frame = sc
    x, passive, active, shifts = cuda(shift_tables(sc, 0))
    _, passive_p, active_p, shifts_p = cuda(shift_tables(sc, 1))  # other valid tables of the same geometry
    R, Nt = passive.shape

    def call(xd, pd, ad, sd):
        xo, mo = torch.empty(R, T, Cc, H, W, device="cuda"), torch.empty(R, Nt, dtype=torch.uint8, device="cuda")
        _lib.check(lib.cwm_shift_prompts(xd.data_ptr(), B, T, Cc, H, W, P, frame, S_, 2, ad.data_ptr(), pd.data_ptr(), sd.data_ptr(), xo.data_ptr(), mo.data_ptr(),
                                         stream()))
        return xo, mo
    run_a("shift_prompts", call, [x, passive, active, shifts], [SO.poison_like(x), passive_p, active_p, shifts_p])


@case("prompt_table_expand")
def test_prompt_table_expand_late_inputs():
    lib = _lib.get_lib()
    S_, T, gh, gw, frame = 9, 3, 2, 5, 1
    n = gh * gw
    table = torch.tensor([[0, 0, 1, -1], [1, 4, 0, 2], [0, 1, 3, 3], [0, 3, -2, 0], [1, 2, 5, 6], [1, 0, 0, -4], [0, 2, 7, 8], [1, 2, 2, 2], [1, 3, -9, 9]], dtype=torch.int32).cuda()
    poison = torch.stack([(table[:, 0] + 1) % gh, (table[:, 1] + 2) % gw, table[:, 3], table[:, 2]], 1).contiguous()  # other in-grid cells, other shifts

    def call(t):
        a, p = torch.empty(S_, T * n, dtype=torch.uint8, device="cuda"), torch.empty(S_, T * n, dtype=torch.uint8, device="cuda")
        s = torch.empty(S_, 2, dtype=torch.int32, device="cuda")
        _lib.check(lib.cwm_prompt_table_expand(t.data_ptr(), S_, T, gh, gw, frame, a.data_ptr(), p.data_ptr(), s.data_ptr(), stream()))
        return a, p, s
    run_a("prompt_table_expand", call, [table], [poison])


@case("multi_shift_prompts")
def test_multi_shift_prompts_late_inputs():
    from test_prompt_kernels_gpu import MULTI_CASES, distinct_frames, multi_tables

    lib = _lib.get_lib()
    mc = MULTI_CASES["p12_one_channel"]
    B, S_, T, Cc, H, W, P, frame, K, _ = mc
    points, masks, shifts, _ = multi_tables("p12_one_channel")
    R, _, Nt = points.shape
    max_abs = int(np.abs(shifts).max())
    x = torch.from_numpy(distinct_frames(B, T, Cc, H, W)).cuda()
    pd, md, sd = torch.from_numpy(points).cuda(), torch.from_numpy(masks).cuda(), torch.from_numpy(shifts.astype(np.int32)).cuda()
    # the poison tables: the rows' own tables in reversed row order, the shifts with the axes exchanged (|s| stays below max_abs + 1 <= min(H, W))
    poison = [SO.poison_like(x), pd.flip(0).contiguous(), md.flip(0).contiguous(), sd.flip(0).flip(-1).contiguous()]

    def call(xd, pts, msk, shf):
        xo, mo = torch.empty(R, T, Cc, H, W, device="cuda"), torch.empty(R, Nt, dtype=torch.uint8, device="cuda")
        _lib.check(lib.cwm_multi_shift_prompts(xd.data_ptr(), B, T, Cc, H, W, P, frame, S_, K, 0, pts.data_ptr(), msk.data_ptr(), msk.shape[1], shf.data_ptr(), max_abs,
                                               xo.data_ptr(), mo.data_ptr(), stream()))
        return xo, mo
    run_a("multi_shift_prompts", call, [x, pd, md, sd], poison)


# ---- patch error, un-embed ----------------------------------------------------------------------------------------------------------------------------------------
@case("patch_error")
def test_patch_error_late_inputs():
    from test_patch_error_gpu import GEOMETRIES, inputs, run_kernel

    B, T, Cc, H, W, P, nm, layout = GEOMETRIES["p4"]
    x, mask, y, target = inputs(B, T, Cc, H, W, P, nm, 100, layout)
    mask_p = inputs(B, T, Cc, H, W, P, nm, 101, layout)[1]  # another mask with the same count per row
    region = (torch.randint(0, 9, (B, T, H // P, W // P), generator=torch.Generator().manual_seed(7)).float() / 4).cuda()
    call = lambda yy, xx, mm, tt, rr: run_kernel(yy, xx, mm, P, 0, tt, rr)  # noqa: E731
    run_a("patch_error", call, [y, x, mask, target, region], nan_of([y, x]) + [mask_p] + nan_of([target, region]))


def unembed_inputs():
    from test_prompt_kernels_gpu import UNEMBED_CASES, unembed_case

    uc = UNEMBED_CASES[4]  # (2, 2, 1, 8, 12, 4, 3): the smallest
    x, y, mask, _ = unembed_case(uc)
    mask_p = mask.flip(0).contiguous()  # the rows' masks exchanged: the same count in every row, and the rows' masks differ
    return uc, cuda([y, x, mask]), [SO.poison_like(y).cuda(), SO.poison_like(x).cuda(), mask_p.cuda()]


def unembed_call(uc, rc_out=None):
    B, T, Cc, H, W, P, n_vis = uc
    lib = _lib.get_lib()

    def call(y, x, mask):
        out = torch.full((B, T, Cc, H, W), -7.0, device="cuda")
        rc = lib.cwm_unembed(y.data_ptr(), x.data_ptr(), mask.data_ptr(), B, T, Cc, H, W, P, n_vis, out.data_ptr(), stream())
        if rc_out is not None:
            rc_out.append(rc)
        else:
            _lib.check(rc)
        return out
    return call


@case("unembed")
def test_unembed_late_inputs():
    uc, truth, poison = unembed_inputs()
    run_a("unembed", unembed_call(uc), truth, poison)


@case("unembed")
def test_unembed_error_word_under_a_busy_null_stream():
    """the error word must be zero before the kernels of the call can set it, whatever the null stream is doing.  Each direction runs right after a plain call
    with the OTHER answer, whose freed scratch the allocator may hand out again: a good mask must still pass where the word last held an error, and a row with
    another count must still be reported"""
    uc, truth, _ = unembed_inputs()
    bad = [truth[0], truth[1], truth[2].clone()]
    bad[2][1, torch.nonzero(bad[2][1])[0, 0]] = False  # one more visible token in row 1: the rank of every masked token stays inside y
    want, ms = plain2(unembed_call(uc), truth)
    rcs = []
    want_bad, _ = SO.plain(unembed_call(uc, rcs), bad)
    assert rcs == [_lib.ERR_MASK]
    for name, prime, inputs, wanted, rc in (("good mask after a bad one", bad, truth, want, 0), ("bad mask after a good one", truth, bad, want_bad, _lib.ERR_MASK)):
        rcs = []
        SO.plain(unembed_call(uc, rcs), prime)
        SO.protocol_b("unembed", unembed_call(uc, rcs), inputs, wanted, ms, " " + name)
        assert rcs[1] == rc, "%s: cwm_unembed returned %d, not %d: its error word was not zero when the call began, or was cleared after it was set" % (name, rcs[1], rc)


# ---- the rectangulariser --------------------------------------------------------------------------------------------------------------------------------------------
def rect_masks(seed):
    """B = 8 rows of 64 tokens with unequal masked counts"""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(8, 64, dtype=torch.bool)
    for b, n in enumerate((30, 41, 30, 37, 52, 33, 30, 45)):
        m[b, torch.randperm(64, generator=g)[:n]] = True
    return m.cuda()


@case("rectangularize")
def test_rectangularize_masks_on_device():
    """the draws come from the global CPU generator: its seed is fixed before every run, plain or streamed.  Protocol C: two mask sets back to back through one
    object (the pinned pick table and its event)"""
    rect = masking.RectangularizeMasks("min")

    def call(m):
        torch.manual_seed(11)
        return rect(m).clone()
    a, b = rect_masks(1), rect_masks(2)
    pa, pb = a.roll(1, 1).contiguous(), b.roll(1, 1).contiguous()  # the same counts in other places
    want, _ = run_a("rectangularize", call, [a], [pa], second=([b], [pb]))
    assert (want[0].sum(1) == 30).all()


# ---- the stand-alone kernels ----------------------------------------------------------------------------------------------------------------------------------------
SPLIT_K_SHAPE = (130, 48, 4096)  # of tests/test_kernels_gpu.py::test_gemm_deep_ring_and_split_k_small_launches


def linear_call(mode, gelu, with_bias=True, with_resid=True):
    lib = _lib.get_lib()

    def call(a, w, *rest):
        rest = list(rest)
        bias = rest.pop(0) if with_bias else None
        resid = rest.pop(0) if with_resid else None
        out = torch.empty(a.shape[0], w.shape[0], device="cuda")
        _lib.check(lib.cwm_linear(a.data_ptr(), w.data_ptr(), _lib.ptr(bias), _lib.ptr(resid), out.data_ptr(), a.shape[0], w.shape[0], a.shape[1], int(gelu),
                                  _lib.mode_id(mode), stream()))
        return out
    return call


def linear_inputs(M, N, K, seed, with_bias=True, with_resid=True):
    g = torch.Generator().manual_seed(seed)
    t = [torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5]
    if with_bias:
        t.append(torch.randn(N, generator=g))
    if with_resid:
        t.append(torch.randn(M, N, generator=g))
    return cuda(t)


def splits_k(M, N, K, mode):
    """the default plan of the fp32-output launch (cwm_dev_gemm_plan, as tests/test_engine_kernels_gpu.py reads it)"""
    d = _lib.get_dev_lib()
    out = _lib.CwmDevGemmPlanOut()
    _lib.check(d.cwm_dev_gemm_plan(M, N, -(-K // 64) * 64, 0, _lib.mode_id(mode), 0, 0, 0, ctypes.byref(out)), d)
    return any(q.splitk > 1 for q in out.part[:out.nparts])


@case("linear")
@pytest.mark.parametrize("M,N,K", [SPLIT_K_SHAPE, (5, 16, 64)])
@pytest.mark.parametrize("mode", MODES)
def test_linear_late_inputs(mode, M, N, K):
    assert splits_k(M, N, K, mode) == ((M, N, K) == SPLIT_K_SHAPE)
    truth = linear_inputs(M, N, K, 31)
    run_a("linear", linear_call(mode, False), truth, nan_of(truth), " %s %dx%dx%d bias + residual" % (mode, M, N, K))
    truth = linear_inputs(M, N, K, 32, with_resid=False)
    run_a("linear", linear_call(mode, True, with_resid=False), truth, nan_of(truth), " %s %dx%dx%d bias + GELU" % (mode, M, N, K))


@case("linear")
@pytest.mark.parametrize("with_bias", [True, False])
def test_linear_bias_buffer_under_a_busy_null_stream(with_bias):
    """the bias scratch is zero-filled and then, with a bias, written on the caller's stream and read there.  Each form runs right after a plain call of the OTHER
    form on the same shape, whose freed scratch (a bias, or zeros) the allocator may hand out again"""
    M, N, K = SPLIT_K_SHAPE
    assert splits_k(M, N, K, "parity")
    full = linear_inputs(M, N, K, 33, with_bias=True, with_resid=False)
    truth, other = (full, full[:2]) if with_bias else (full[:2], full)
    call, other_call = linear_call("parity", False, with_bias=with_bias, with_resid=False), linear_call("parity", False, with_bias=not with_bias, with_resid=False)
    want, ms = plain2(call, truth)
    assert not SO.same(want, SO.plain(other_call, other)[0])  # (the bias changes the result; this call also leaves the other form's scratch behind)
    SO.protocol_b("linear", call, truth, want, ms, " with a bias, after a call without" if with_bias else " without a bias, after a call with one")


def attention_inputs(seed):
    return (torch.randn(2, 40, 3 * 2 * 64, generator=torch.Generator().manual_seed(seed))).cuda()


def attention_call(mode, ragged, rc_out=None):
    lib = _lib.get_lib()

    def call(qkv, key_len=None):
        out = torch.full((2, 40, 128), -7.0, device="cuda")
        if ragged:
            rc = lib.cwm_attention_ragged(qkv.data_ptr(), key_len.data_ptr(), out.data_ptr(), 2, 40, 2, _lib.mode_id(mode), stream())
        else:
            rc = lib.cwm_attention(qkv.data_ptr(), out.data_ptr(), 2, 40, 2, _lib.mode_id(mode), stream())
        if rc_out is not None:
            rc_out.append(rc)
        else:
            _lib.check(rc)
        return out
    return call


@case("attention")
@pytest.mark.parametrize("mode", MODES)
def test_attention_late_inputs(mode):
    qkv = attention_inputs(1)
    run_a("attention", attention_call(mode, False), [qkv], nan_of([qkv]), " " + mode)


@case("attention_ragged")
@pytest.mark.parametrize("mode", MODES)
def test_attention_ragged_late_inputs(mode):
    qkv = attention_inputs(1)
    key_len, key_len_p = torch.tensor([17, 40], dtype=torch.int32).cuda(), torch.tensor([33, 9], dtype=torch.int32).cuda()  # both inside [1, N]
    run_a("attention_ragged", attention_call(mode, True), [qkv, key_len], [SO.poison_like(qkv), key_len_p], " " + mode)


@case("attention_ragged")
def test_attention_ragged_error_word_under_a_busy_null_stream():
    """as the un-embed's error word: each direction right after a plain call with the other answer"""
    qkv, good, bad = attention_inputs(2), torch.tensor([17, 40], dtype=torch.int32).cuda(), torch.tensor([17, 41], dtype=torch.int32).cuda()
    want, ms = plain2(attention_call("parity", True), [qkv, good])
    rcs = []
    want_bad, _ = SO.plain(attention_call("parity", True, rcs), [qkv, bad])
    assert rcs == [_lib.ERR_INVALID] and bool((want_bad[0] == -7.0).all())
    for name, prime, key_len, wanted, rc in (("good lengths after a bad one", bad, good, want, 0), ("a length outside [1, N] after good ones", good, bad, want_bad, _lib.ERR_INVALID)):
        rcs = []
        SO.plain(attention_call("parity", True, rcs), [qkv, prime])
        SO.protocol_b("attention_ragged", attention_call("parity", True, rcs), [qkv, key_len], wanted, ms, " " + name)
        assert rcs[1] == rc, "%s: cwm_attention_ragged returned %d, not %d: its error word was not zero when the call began, or was cleared after it was set" % (name, rcs[1], rc)


@case("layernorm")
def test_layernorm_late_inputs():
    lib = _lib.get_lib()
    g = torch.Generator().manual_seed(3)
    truth = cuda([torch.randn(37, 40, generator=g), torch.randn(40, generator=g), torch.randn(40, generator=g)])

    def call(x, gamma, beta):
        out = torch.empty_like(x)
        _lib.check(lib.cwm_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), 37, 40, 1e-6, stream()))
        return out
    run_a("layernorm", call, truth, nan_of(truth))


def perm_call(rc_out):
    lib = _lib.get_lib()

    def call(mask):
        perm = torch.full(mask.shape, -7, dtype=torch.int32, device="cuda")
        rc_out.append(lib.cwm_mask_to_perm(mask.data_ptr(), mask.shape[0], mask.shape[1], VIT_NVIS, perm.data_ptr(), stream()))
        return perm
    return call


@case("mask_to_perm")
def test_mask_to_perm_late_inputs_good_and_bad_mask():
    good, other = vit_masks(3, VIT_NVIS, 4), vit_masks(3, VIT_NVIS, 5)
    bad = good.clone()
    bad[1, torch.nonzero(bad[1])[0, 0]] = False  # row 1 has one visible token too many
    rcs = []
    run_a("mask_to_perm", perm_call(rcs), [good], [other], " good mask")
    assert set(rcs) == {0}
    # the bad mask arrives late over a good one: it must be the bad one that is judged
    rcs = []
    run_a("mask_to_perm", perm_call(rcs), [bad], [other], " bad mask")
    assert rcs[0] == rcs[1] == rcs[-1] == _lib.ERR_MASK and rcs[2] == 0  # (plain, plain, the poison's plain run, protocol A)


@case("mask_to_perm")
def test_mask_to_perm_error_word_under_a_busy_null_stream():
    """as the un-embed's error word: each direction right after a plain call with the other answer"""
    good = vit_masks(3, VIT_NVIS, 4)
    bad = good.clone()
    bad[1, torch.nonzero(bad[1])[0, 0]] = False
    for name, prime, mask, rc in (("good mask after a bad one", bad, good, 0), ("bad mask after a good one", good, bad, _lib.ERR_MASK)):
        rcs = []
        want, ms = plain2(perm_call(rcs), [mask])
        SO.plain(perm_call(rcs), [prime])
        SO.protocol_b("mask_to_perm", perm_call(rcs), [mask], want, ms, " " + name)
        assert rcs[0] == rcs[1] == rc and rcs[2] != rc, (name, rcs)
        assert rcs[3] == rc, "%s: cwm_mask_to_perm returned %d, not %d: its error word was not zero when the call began, or was cleared after it was set" % (name, rcs[3], rc)


@case("split_bf16")
def test_split_bf16_late_inputs():
    lib = _lib.get_lib()
    x = torch.randn(1000, generator=torch.Generator().manual_seed(1)).cuda()

    def call(t):
        hi, lo = torch.empty(1000, dtype=torch.bfloat16, device="cuda"), torch.empty(1000, dtype=torch.bfloat16, device="cuda")
        _lib.check(lib.cwm_split_bf16(t.data_ptr(), 1000, hi.data_ptr(), lo.data_ptr(), stream()))
        return hi.view(torch.int16), lo.view(torch.int16)
    run_a("split_bf16", call, [x], [2.0 * x])  # (NaN splits into NaN planes, which compare unequal to themselves: the poison is another finite vector)


def test_every_case_of_the_table_has_a_runner():
    assert set(RUNNERS) == set(SO.CASES), (sorted(set(SO.CASES) - set(RUNNERS)), sorted(set(RUNNERS) - set(SO.CASES)))
    print("\n".join(SO.LOG))
