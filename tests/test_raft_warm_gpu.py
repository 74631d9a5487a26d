"""RAFT's warm start (`flow_init`) and per-iteration outputs (`test_mode=False`) on the GPU: `cwm_raft_forward_ex` (csrc/raft_model.hip,
`coords_init_flow_kernel` of csrc/raft_kernels.hip) and the Python surface around it (raft.py), against the reference's golden outputs
(tests/golden/make_golden_raft_warm.py) and against the plain forward, bit for bit.

Bounds.  Flows: 1e-2 px max-abs, TOL_24 of tests/test_raft_gpu.py, the project's parity bound for multi-iteration flows.  Keypoint maps: 1e-3 times
max |map|, as tests/test_keypoint_raft_gpu.py.  The fixtures' makers asserted on the reference that a warm start moves the output by >= 0.5 px (22.99 and
21.80 px here) and that successive list elements differ by >= 0.1 px (0.55 / 0.43 px), so neither bound is met by a build that ignores `flow_init` or
repeats the last prediction.  Everything else is an identity between two runs of the library and is asserted with `torch.equal`."""
import ctypes
import os

import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import _lib, config as C, segmentation, synthetic as S, vmae
from counterfactualworldmodels_amd.raft import RAFT, _args

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_24 = 1e-2   # px, max-abs (tests/test_raft_gpu.py)
TOL_MAP = 1e-3  # times max |map| (tests/test_keypoint_raft_gpu.py)
SENTINEL = -7.0


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def build(seed, multiframe=True, output_dim=None):
    m = RAFT(_args(output_dim=output_dim, multiframe=multiframe))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(seed, output_dim=output_dim).items()})
    return m.cuda().eval()


def frames(B, H, W, seed, **kw):
    return torch.from_numpy(S.raft_frames(B, H, W, seed, **kw)).cuda()


def check(name, got, want, tol, drift):
    err = float(np.abs(got - want).max())
    print(f"[{name}] max-abs {err:.3e} (bound {tol:.3e}, |reference| max {np.abs(want).max():.2f}, reference fp32 vs float64 {float(drift):.3e})")
    assert got.shape == want.shape
    assert err <= tol, (name, err, tol)


# ---- shared models and inputs (built once per module) -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case2():
    """128 x 128, B = 1, 3 iterations, with an init: the two-image flow model and keypoint model of the list fixture, their frames and init."""
    g = golden("raft_warm_list_128")
    x = frames(1, 128, 128, int(g["frames_seed"])) * 255.0
    return {"g": g, "flow": build(int(g["seed"]), multiframe=False), "kp": build(int(g["seed"]), multiframe=False, output_dim=1),
            "x1": x[:, 0].contiguous(), "x2": x[:, 1].contiguous(), "init": torch.from_numpy(g["init"]).cuda(), "iters": int(g["iters"])}


@pytest.fixture(scope="module")
def flow2():
    """A two-image flow model with 128 x 160 frames, B = 2, T = 3 (in [0, 255]) and a [2,2,16,20] init."""
    m = build(14, multiframe=False)
    x = frames(2, 128, 160, 31, shift=(2, -3), frames=3) * 255.0
    g = torch.Generator().manual_seed(7)
    init = (4.0 * torch.rand(2, 2, 16, 20, generator=g) - 2.0).cuda()
    return {"m": m, "x": x, "init": init}


# ---- parity against the reference -------------------------------------------------------------------------------------------------
def test_two_image_call_with_init_vs_reference():
    g = golden("raft_warm_136x152_b2")
    m = build(int(g["seed"]), multiframe=False)
    x = frames(2, 136, 152, int(g["frames_seed"]), shift=tuple(int(v) for v in g["shift"])) * 255.0
    low, up = m(x[:, 0], x[:, 1], iters=int(g["iters"]), flow_init=torch.from_numpy(g["init"]).cuda(), test_mode=True)
    assert float(g["warm_vs_cold"]) >= 0.5
    check("136x152 warm up", up.cpu().numpy(), g["up"], TOL_24, g["drift"])
    check("136x152 warm low", low.cpu().numpy(), g["low"], TOL_24, g["drift"])


def test_list_with_init_vs_reference(case2):
    g, n = case2["g"], case2["iters"]
    preds = case2["flow"](case2["x1"], case2["x2"], iters=n, flow_init=case2["init"], test_mode=False)
    assert isinstance(preds, list) and len(preds) == n and all(p.shape == (1, 2, 128, 128) for p in preds)
    for k in range(n):
        check("128 list flow %d" % k, preds[k].cpu().numpy(), g["preds"][k], TOL_24, g["drift"])
    maps = case2["kp"](case2["x1"], case2["x2"], iters=n, flow_init=case2["init"], test_mode=False)
    assert isinstance(maps, list) and len(maps) == n and all(p.shape == (1, 1, 128, 128) for p in maps)
    for k in range(n):
        check("128 list keypoint map %d" % k, maps[k].cpu().numpy(), g["kp_preds"][k], TOL_MAP * float(np.abs(g["kp_preds"][k]).max()), g["kp_drift"])


def test_multiframe_with_init_vs_reference():
    g = golden("raft_warm_128x160_t3")
    m = build(int(g["seed"]))
    x = frames(1, 128, 160, int(g["frames_seed"]), shift=tuple(int(v) for v in g["shift"]), frames=3)
    init = torch.from_numpy(g["init"]).cuda()
    assert tuple(init.shape) == (1, 2, 16, 20) and float(g["warm_vs_cold"]) >= 0.5
    yf = m(x, iters=int(g["iters"]), flow_init=init)
    yb = m(x, iters=int(g["iters"]), backward=True, flow_init=init)
    check("128x160 warm fwd", yf.cpu().numpy(), g["flow_fwd"], TOL_24, g["drift_fwd"])
    check("128x160 warm bwd", yb.cpu().numpy(), g["flow_bwd"], TOL_24, g["drift_bwd"])
    # test_mode is accepted and changes nothing: the reference keeps [-1] of what the pair's call returns
    assert torch.equal(m(x, iters=int(g["iters"]), flow_init=init, test_mode=False), yf)
    assert torch.equal(m(x, int(g["iters"]), init), yf)  # positionally, as the reference's *args[1:]


# ---- fast mode ----------------------------------------------------------------------------------------------------------------------
def test_fast_mode_list_is_the_fast_forwards(case2):
    n = case2["iters"]
    for key, ch in (("flow", 2), ("kp", 1)):
        m = case2[key]
        m.set_mode("fast")
        try:
            preds = m(case2["x1"], case2["x2"], iters=n, flow_init=case2["init"], test_mode=False)
            assert len(preds) == n and all(p.shape == (1, ch, 128, 128) and p.dtype == torch.float32 for p in preds)
            for k in range(n):
                _, up = m(case2["x1"], case2["x2"], iters=k + 1, flow_init=case2["init"], test_mode=True)
                assert torch.equal(preds[k], up), (key, k)
            m.set_mode("parity")
            parity = m(case2["x1"], case2["x2"], iters=n, flow_init=case2["init"], test_mode=False)
            assert not torch.equal(parity[-1], preds[-1])  # the mode reaches the per-iteration path
        finally:
            m.set_mode("parity")


# ---- identities between two runs of the library, bit for bit (parity mode) ------------------------------------------------------------
def test_zeros_init_is_no_init(flow2):
    m, x = flow2["m"], flow2["x"]
    low, up = m(x[:, 0], x[:, 1], iters=3)
    zeros = torch.zeros(2, 2, 16, 20, device="cuda")
    low0, up0 = m(x[:, 0], x[:, 1], iters=3, flow_init=zeros)
    assert torch.equal(low0, low) and torch.equal(up0, up)
    lowh, uph = m(x[:, 0], x[:, 1], iters=3, flow_init=zeros.half())  # any float dtype
    assert torch.equal(lowh, low) and torch.equal(uph, up)
    loww, upw = m(x[:, 0], x[:, 1], iters=3, flow_init=flow2["init"])
    assert not torch.equal(upw, up) and not torch.equal(loww, low)


def test_list_elements_are_the_shorter_forwards(case2):
    n, x1, x2, init = case2["iters"], case2["x1"], case2["x2"], case2["init"]
    for key in ("flow", "kp"):
        m = case2[key]
        cold = m(x1, x2, iters=n, test_mode=False)
        warm = m(x1, x2, iters=n, flow_init=init, test_mode=False)
        for k in range(n):
            assert torch.equal(cold[k], m(x1, x2, iters=k + 1)[1]), (key, k)  # the plain forward (cwm_raft_forward)
            assert torch.equal(warm[k], m(x1, x2, iters=k + 1, flow_init=init)[1]), (key, k)
        assert not torch.equal(warm[-1], cold[-1]) and not torch.equal(warm[-1], warm[-2])
    # self.iters, when set, decides the length
    m = case2["flow"]
    m.set_iters(2)
    try:
        short = m(x1, x2, iters=n, flow_init=init, test_mode=False)
    finally:
        m.set_iters(None)
    assert len(short) == 2 and torch.equal(short[1], warm_flow_at(case2, 2))


def warm_flow_at(case2, iters):
    return case2["flow"](case2["x1"], case2["x2"], iters=iters, flow_init=case2["init"])[1]


def test_multiframe_with_init_is_the_per_pair_two_image_calls(flow2):
    """B = 2, T = 3, forward and backward: the multi-frame call hands the same init to every pair (raft_model.py:297).  Both sides read frames in
    [0, 255] with input scale 1 (scale_inputs=False), so the inputs of the two paths are the same numbers."""
    m2, x, init = flow2["m"], flow2["x"], flow2["init"]
    mf = build(14)
    mf.scale_inputs = False
    for backward in (False, True):
        y = mf(x, iters=3, backward=backward, flow_init=init)
        assert y.shape == (2, 2, 2, 128, 160)
        for t in range(2):
            a, b = (x[:, t + 1], x[:, t]) if backward else (x[:, t], x[:, t + 1])
            _, up = m2(a, b, iters=3, flow_init=init)
            assert torch.equal(y[:, 1 - t if backward else t], up), (backward, t)


def test_one_field_for_all_batch_rows_is_the_expanded_field(flow2):
    m, x = flow2["m"], flow2["x"]
    one = flow2["init"][:1]
    low1, up1 = m(x[:, 0], x[:, 1], iters=2, flow_init=one)
    lowB, upB = m(x[:, 0], x[:, 1], iters=2, flow_init=one.expand(2, 2, 16, 20))  # stride 0 over the batch
    lowC, upC = m(x[:, 0], x[:, 1], iters=2, flow_init=one.expand(2, 2, 16, 20).contiguous())
    assert torch.equal(low1, lowB) and torch.equal(up1, upB) and torch.equal(low1, lowC) and torch.equal(up1, upC)
    # row 1 sees the field, not a second one read behind it
    _, up_row1 = m(x[1:, 0], x[1:, 1], iters=2, flow_init=one)
    assert (up1[1:] - up_row1).abs().max().item() <= TOL_24


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def _ex_args(x, iters=3):
    """x [B,2,3,H,W] in [0,1]: the pair (x[:,0], x[:,1])."""
    ex = _lib.new_raft_forward_ex_args()
    a = ex.base
    a.image1_dev, a.image2_dev = x.data_ptr(), x.data_ptr() + x.stride(1) * 4
    a.image1_stride_b = a.image2_stride_b = x.stride(0)
    a.image1_stride_c = a.image2_stride_c = x.stride(2)
    a.batch, a.pairs, a.height, a.width, a.input_scale, a.iters = x.shape[0], 1, x.shape[-2], x.shape[-1], 255.0, iters
    return ex


def test_ex_without_optional_fields_is_the_plain_forward():
    lib = _lib.get_lib()
    m = build(3)
    x = frames(2, 128, 160, 21)
    want = m(x, iters=3)  # cwm_raft_forward
    flow = torch.full((2, 1, 2, 128, 160), SENTINEL, device="cuda")
    low = torch.full((2, 2, 16, 20), SENTINEL, device="cuda")
    ex = _ex_args(x)
    ex.base.flow_dev, ex.base.flow_low_dev = flow.data_ptr(), low.data_ptr()
    ex.base.flow_stride_b, ex.base.flow_stride_c = flow.stride(0), flow.stride(2)
    _lib.check(lib.cwm_raft_forward_ex(m._handle, ctypes.byref(ex)))
    torch.cuda.synchronize()
    assert torch.equal(flow, want) and not (low == SENTINEL).any()


def test_head_and_flow_lists_in_one_call_are_the_separate_calls():
    """A keypoint model asked for both per-iteration outputs and both final outputs in one call: every buffer equals that of the call that asks for
    it alone, and the last list elements equal the final outputs."""
    lib = _lib.get_lib()
    kp = build(5, output_dim=1)
    x = frames(2, 128, 128, 23)
    n = 3
    kp(x, iters=1)  # creates the handle and uploads the weights

    def run(want_flow_iters, want_head_iters, want_final):
        bufs = {"flow_iters": torch.full((n, 2, 1, 2, 128, 128), SENTINEL, device="cuda"), "head_iters": torch.full((n, 2, 1, 1, 128, 128), SENTINEL, device="cuda"),
                "flow": torch.full((2, 1, 2, 128, 128), SENTINEL, device="cuda"), "head": torch.full((2, 1, 1, 128, 128), SENTINEL, device="cuda")}
        ex = _ex_args(x, iters=n)
        ex.base.flow_stride_b, ex.base.flow_stride_c = bufs["flow"].stride(0), bufs["flow"].stride(2)
        ex.base.head_stride_b, ex.base.head_stride_c = bufs["head"].stride(0), bufs["head"].stride(2)
        if want_flow_iters:
            ex.flow_iters_dev, ex.flow_iters_stride_i = bufs["flow_iters"].data_ptr(), bufs["flow_iters"].stride(0)
        if want_head_iters:
            ex.head_iters_dev, ex.head_iters_stride_i = bufs["head_iters"].data_ptr(), bufs["head_iters"].stride(0)
        if want_final:
            ex.base.flow_dev, ex.base.head_dev = bufs["flow"].data_ptr(), bufs["head"].data_ptr()
        _lib.check(lib.cwm_raft_forward_ex(kp._handle, ctypes.byref(ex)))
        torch.cuda.synchronize()
        return bufs

    both = run(True, True, True)
    only_flow, only_head = run(True, False, False), run(False, True, False)
    assert torch.equal(both["flow_iters"], only_flow["flow_iters"]) and torch.equal(both["head_iters"], only_head["head_iters"])
    assert not (both["flow_iters"] == SENTINEL).any() and not (both["head_iters"] == SENTINEL).any()
    # what a call does not ask for it does not write
    assert (only_flow["head_iters"] == SENTINEL).all() and (only_flow["flow"] == SENTINEL).all() and (only_flow["head"] == SENTINEL).all()
    assert (only_head["flow_iters"] == SENTINEL).all()
    # the final outputs beside the lists: the last elements, and the plain forward's
    assert torch.equal(both["flow"], both["flow_iters"][-1]) and torch.equal(both["head"], both["head_iters"][-1])
    assert torch.equal(both["head"], kp(x, iters=n))
    for k in range(n - 1):
        assert torch.equal(both["head_iters"][k], kp(x, iters=k + 1)), k


def test_pairs_with_a_per_pair_init_and_reversed_blocks_are_the_batched_pairs():
    """The strides only a direct caller sets: `pairs = 2` with an init of its own per pair (`flow_init_stride_t`) and a negative pair stride inside
    the per-iteration blocks and the final outputs, on a keypoint model asked for both lists.  The same two pairs as batch rows of a `pairs = 1`
    call (an init per row, blocks in order) are the same launches on the same rows, so every pair's output is equal bit for bit."""
    lib = _lib.get_lib()
    kp = build(5, output_dim=1)
    x = frames(1, 128, 128, 27, shift=(2, -3), frames=3)  # pairs (x0, x1) and (x1, x2)
    n = 2
    kp(x, iters=1)
    g = torch.Generator().manual_seed(9)
    init = (4.0 * torch.rand(2, 2, 16, 16, generator=g) - 2.0).cuda()

    def run(as_pairs):
        B, P = (1, 2) if as_pairs else (2, 1)
        bufs = {"flow_iters": torch.full((n, B, P, 2, 128, 128), SENTINEL, device="cuda"), "head_iters": torch.full((n, B, P, 1, 128, 128), SENTINEL, device="cuda"),
                "flow": torch.full((B, P, 2, 128, 128), SENTINEL, device="cuda"), "head": torch.full((B, P, 1, 128, 128), SENTINEL, device="cuda"),
                "low": torch.full((2, 2, 16, 16), SENTINEL, device="cuda")}
        ex = _lib.new_raft_forward_ex_args()
        a = ex.base
        a.image1_dev, a.image2_dev = x.data_ptr(), x.data_ptr() + x.stride(1) * 4
        a.image1_stride_c = a.image2_stride_c = x.stride(2)
        a.batch, a.pairs, a.height, a.width, a.input_scale, a.iters = B, P, 128, 128, 255.0, n
        ex.flow_init_dev, ex.flow_init_stride_c = init.data_ptr(), init.stride(1)
        flow, head = bufs["flow"], bufs["head"]
        a.flow_stride_b, a.flow_stride_c, a.head_stride_b, a.head_stride_c = flow.stride(0), flow.stride(2), head.stride(0), head.stride(2)
        off_f = off_h = 0
        if as_pairs:  # the frame stride walks the pairs; pair t is written at index 1 - t of every block
            a.image1_stride_t = a.image2_stride_t = x.stride(1)
            ex.flow_init_stride_t = init.stride(0)
            a.flow_stride_t, a.head_stride_t = -flow.stride(1), -head.stride(1)
            off_f, off_h = flow.stride(1) * 4, head.stride(1) * 4
        else:     # the batch stride walks the pairs
            a.image1_stride_b = a.image2_stride_b = x.stride(1)
            ex.flow_init_stride_b = init.stride(0)
        a.flow_dev, a.head_dev, a.flow_low_dev = flow.data_ptr() + off_f, head.data_ptr() + off_h, bufs["low"].data_ptr()
        ex.flow_iters_dev, ex.flow_iters_stride_i = bufs["flow_iters"].data_ptr() + off_f, bufs["flow_iters"].stride(0)
        ex.head_iters_dev, ex.head_iters_stride_i = bufs["head_iters"].data_ptr() + off_h, bufs["head_iters"].stride(0)
        _lib.check(lib.cwm_raft_forward_ex(kp._handle, ctypes.byref(ex)))
        torch.cuda.synchronize()
        assert not any((b == SENTINEL).any() for b in bufs.values())
        return bufs

    pairs, rows = run(True), run(False)
    assert torch.equal(pairs["low"], rows["low"])
    for t in range(2):
        for key in ("flow", "head"):
            assert torch.equal(pairs[key][0, 1 - t], rows[key][t, 0]), (key, t)
            assert torch.equal(pairs[key + "_iters"][:, 0, 1 - t], rows[key + "_iters"][:, t, 0]), (key, t)
    # the two pairs got different inits and are different frames: the order is observable
    assert not torch.equal(rows["flow"][0], rows["flow"][1])
    # and each pair saw ITS init: pair 1 with the inits swapped gives another flow
    assert (pairs["low"][1] - init[1]).abs().max() < (pairs["low"][1] - init[0]).abs().max()


def test_generator_predict_flow_passes_the_init():
    cfg = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
    raft = build(14)
    G = segmentation.FlowGenerator(predictor=vmae.PretrainVisionTransformer(cfg), flow_model=raft, imagenet_normalize_inputs=True, temporal_dim=2)
    vid = frames(1, 128, 160, 33)
    g = torch.Generator().manual_seed(8)
    init = (4.0 * torch.rand(1, 2, 16, 20, generator=g) - 2.0).cuda()
    got = G.predict_flow(vid, iters=2, flow_init=init)
    assert raft.iters == 2
    want = raft(vid, flow_init=init)
    assert got.shape == (1, 1, 2, 128, 160) and torch.equal(got, want)
    assert not torch.equal(got, G.predict_flow(vid))
    assert torch.equal(G.predict_flow(vid, backward=True, flow_init=init), raft(vid, backward=True, flow_init=init))


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_init_of_the_wrong_shape_or_device_raises(flow2):
    m, x = flow2["m"], flow2["x"]
    for bad in (torch.zeros(2, 2, 20, 16), torch.zeros(3, 2, 16, 20), torch.zeros(2, 1, 16, 20), torch.zeros(2, 16, 20), torch.zeros(2, 2, 128, 160)):
        with pytest.raises(RuntimeError, match=r"flow_init.*\[2,2,16,20\].*%s" % str(tuple(bad.shape)).replace("(", r"\(").replace(")", r"\)")):
            m(x[:, 0], x[:, 1], iters=2, flow_init=bad.cuda())
    with pytest.raises(RuntimeError, match=r"flow_init \(2, 2, 16, 20\) is on cpu"):
        m(x[:, 0], x[:, 1], iters=2, flow_init=torch.zeros(2, 2, 16, 20))
    with pytest.raises(RuntimeError, match="floating-point"):
        m(x[:, 0], x[:, 1], iters=2, flow_init=torch.zeros(2, 2, 16, 20, dtype=torch.int32).cuda())
    mf = build(14)
    with pytest.raises(RuntimeError, match=r"flow_init.*\(1, 2, 20, 16\)"):
        mf(x / 255.0, iters=2, flow_init=torch.zeros(1, 2, 20, 16).cuda())


def test_abi_errors_leave_the_outputs_untouched():
    lib = _lib.get_lib()
    m = build(3)
    x = frames(1, 128, 128, 22)
    m(x, iters=1)
    n = 2
    flow = torch.full((1, 1, 2, 128, 128), SENTINEL, device="cuda")
    flows = torch.full((n, 1, 1, 2, 128, 128), SENTINEL, device="cuda")
    heads = torch.full((n, 1, 1, 1, 128, 128), SENTINEL, device="cuda")

    def args():
        ex = _ex_args(x, iters=n)
        ex.base.flow_dev = flow.data_ptr()
        ex.base.flow_stride_b, ex.base.flow_stride_c = flow.stride(0), flow.stride(2)
        ex.flow_iters_dev, ex.flow_iters_stride_i = flows.data_ptr(), flows.stride(0)
        return ex

    def untouched():
        torch.cuda.synchronize()
        return bool((flow == SENTINEL).all() and (flows == SENTINEL).all() and (heads == SENTINEL).all())

    size = ctypes.sizeof(_lib.CwmRaftForwardExArgs)
    for bad in (0, size - 8, size + 8, ctypes.sizeof(_lib.CwmRaftForwardArgs), 5000):  # one size only: this is the first struct of its name
        ex = args()
        ex.struct_size = bad
        assert lib.cwm_raft_forward_ex(m._handle, ctypes.byref(ex)) == _lib.ERR_INVALID and b"struct_size" in lib.cwm_last_error()
        assert untouched()
    for bad in (0, _lib.CwmRaftForwardArgs.stream.offset, 5000):  # base keeps the size rules of cwm_raft_forward
        ex = args()
        ex.base.struct_size = bad
        assert lib.cwm_raft_forward_ex(m._handle, ctypes.byref(ex)) == _lib.ERR_INVALID and b"struct_size" in lib.cwm_last_error()
        assert untouched()
    # head_iters_dev on a flow model: the same error as head_dev
    ex = args()
    ex.head_iters_dev, ex.head_iters_stride_i = heads.data_ptr(), heads.stride(0)
    ex.base.head_stride_b = heads.stride(1)
    assert lib.cwm_raft_forward_ex(m._handle, ctypes.byref(ex)) == _lib.ERR_INVALID and b"output_block.0.weight" in lib.cwm_last_error()
    assert untouched()
    # no output requested
    ex = args()
    ex.base.flow_dev, ex.flow_iters_dev = None, None
    assert lib.cwm_raft_forward_ex(m._handle, ctypes.byref(ex)) == _lib.ERR_INVALID and b"no output" in lib.cwm_last_error()
    assert untouched()
    # the same arguments, valid: both buffers are written
    _lib.check(lib.cwm_raft_forward_ex(m._handle, ctypes.byref(args())))
    torch.cuda.synchronize()
    assert torch.equal(flow, m(x, iters=n)) and torch.equal(flows[-1], flow) and (heads == SENTINEL).all()
