"""The keypoint RAFT (`output_dim=1`: the output head of csrc/raft_model.hip, `head_project_kernel` / `convex_upsample_kernel<1>` of
csrc/raft_kernels.hip) on the GPU against the reference's golden outputs (tests/golden/make_golden_movability.py), its stand-alone kernels
against torch restatements, and the C ABI around it (optional weights, `struct_size` versions).

Bounds.  The low-resolution flow keeps the bounds of tests/test_raft_gpu.py (TOL_1, TOL_24).  The head map is held to the project's parity
contract: 1e-3 max-abs times max(1, max |reference|).  The keypoint distribution `((sigmoid v)^p - min) / range` through
`predict_keypoints_distribution(power=p)` is held to p * eps_map / R = 8e-3 / R with eps_map = 1e-3 and R the recorded range of (sigmoid v)^p:
d/dv (sigmoid v)^p = p (sigmoid v)^p (1 - sigmoid v) <= p / 4, so a value and the minimum each move by at most p/4 eps_map, the numerator by twice
that, and the range by twice that as well: |d (n / r)| <= (|dn| + (n / r) |dr|) / r <= 2 (p/2 eps_map) / R = p eps_map / R."""
import ctypes
import os

import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import _lib, synthetic as S
from counterfactualworldmodels_amd.prediction import PredictorBasedGenerator
from counterfactualworldmodels_amd.raft import RAFT, _args, load_raft_model
from test_raft_gpu import CONVEX_SHAPES, convex_case, padded_out, upsample_restated

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_24 = 1e-2  # px, max-abs at 24 iterations (tests/test_raft_gpu.py)
TOL_1 = 5e-3   # px, max-abs at 1 iteration
TOL_MAP = 1e-3  # the parity contract, times max(1, max |reference|)
HEAD_KEYS = ["output_block.0.weight", "output_block.0.bias", "output_block.2.weight", "output_block.2.bias"]


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def build(seed, multiframe=True):
    m = RAFT(_args(output_dim=1, multiframe=multiframe))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(seed, output_dim=1).items()})
    return m.cuda().eval()


def frames(B, H, W, seed, **kw):
    return torch.from_numpy(S.raft_frames(B, H, W, seed, **kw)).cuda()


def check_map(name, got, want, drift=None):
    tol = TOL_MAP * max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    print(f"[{name}] map max-abs {err:.3e} (bound {tol:.3e}, |map| max {np.abs(want).max():.2f}, std {want.std():.2f}"
          + (f", reference fp32 vs float64 {float(drift):.3e})" if drift is not None else ")"))
    assert got.shape == want.shape
    assert err <= tol, (name, err, tol)
    return tol


def check_low(name, got, want, tol):
    err = float(np.abs(got - want).max())
    print(f"[{name}] low-resolution flow max-abs {err:.3e} px (bound {tol:g})")
    assert got.shape == want.shape
    assert err <= tol, (name, err)


def test_224_b1_multiframe_and_two_image_calls_vs_reference():
    g = golden("raft_keypoint_224_b1")
    x = frames(1, 224, 224, int(g["frames_seed"]))
    m = build(int(g["seed"]))
    m2 = build(int(g["seed"]), multiframe=False)
    for iters, tol in ((24, TOL_24), (1, TOL_1)):
        y = m(x, iters=iters)
        assert y.shape == (1, 1, 1, 224, 224)
        check_map("224_b1 it%d" % iters, y.cpu().numpy(), g["map_it%d" % iters], g["drift_it%d" % iters])
        low, up = m2(x[:, 0] * 255.0, x[:, 1] * 255.0, iters=iters, test_mode=True)
        assert low.shape == (1, 2, 28, 28) and up.shape == (1, 1, 224, 224)
        # (the reference's second output equals its multi-frame map bit for bit: asserted by the fixture's maker)
        check_map("224_b1 two-image it%d" % iters, up.cpu().numpy(), g["map_it%d" % iters][:, 0], g["drift_two_it%d" % iters])
        check_low("224_b1 two-image it%d" % iters, low.cpu().numpy(), g["two_low_it%d" % iters], tol)
        assert torch.equal(up, y[:, 0])
    # T = 1: the frame is repeated (raft_model.py:287-288)
    y1 = m(x[:, :1], iters=24)
    assert y1.shape == (1, 1, 1, 224, 224)
    check_map("224_b1 T=1", y1.cpu().numpy(), g["map_t1"], g["drift_t1"])


def test_keypoints_distribution_vs_reference():
    g = golden("raft_keypoint_224_b1")
    power, R = int(g["power"]), float(g["R"])
    assert R >= 0.2
    m = build(int(g["seed"]))
    x = frames(1, 224, 224, int(g["frames_seed"]))

    class Keypoints:  # the two wrapper methods around the model, nothing else of the generator
        keypoint_predictor = m
        predict_keypoints_map = PredictorBasedGenerator.predict_keypoints_map
        predict_keypoints_distribution = PredictorBasedGenerator.predict_keypoints_distribution

    d = Keypoints().predict_keypoints_distribution(x, power=power).cpu().numpy()
    eps_map = TOL_MAP
    tol = power * eps_map / R
    err = float(np.abs(d - g["distribution"]).max())
    print(f"[keypoints distribution] max-abs {err:.3e} (bound {power} * {eps_map:.3e} / {R:.3f} = {tol:.3e})")
    assert d.shape == g["distribution"].shape == (1, 1, 224, 224)
    assert err <= tol


def test_128x160_t3_forward_and_backward_vs_reference():
    g = golden("raft_keypoint_128x160_t3")
    m = build(int(g["seed"]))
    x = frames(1, 128, 160, int(g["frames_seed"]), shift=tuple(int(v) for v in g["shift"]), frames=3)
    yf, yb = m(x, iters=24), m(x, iters=24, backward=True)
    assert yf.shape == yb.shape == (1, 2, 1, 128, 160)
    check_map("128x160 fwd", yf.cpu().numpy(), g["map_fwd"], g["drift_fwd"])
    check_map("128x160 bwd", yb.cpu().numpy(), g["map_bwd"], g["drift_bwd"])
    # backward=True is the two-image call with swapped images, the pairs in reversed order
    m2 = build(int(g["seed"]), multiframe=False)
    for t in range(2):
        _, up = m2(x[:, t + 1] * 255.0, x[:, t] * 255.0, iters=24, test_mode=True)
        err = (up - yb[:, 1 - t]).abs().max().item()
        print(f"[128x160 bwd pair {t}] multi-frame vs swapped two-image call {err:.3e}")
        assert err <= 1e-5 * max(1.0, up.abs().max().item())  # x * 255 here against the in-kernel input scale: one rounding of the input


def test_224_b2_vs_reference():
    g = golden("raft_keypoint_224_b2")
    m = build(int(g["seed"]))
    y = m(frames(2, 224, 224, int(g["frames_seed"])), iters=24)
    check_map("224_b2", y.cpu().numpy(), g["map"], g["drift"])


# ---- stand-alone kernels against torch restatements -----------------------------------------------------------------------
def test_head_project_kernel_vs_restatement():
    lib = _lib.get_lib()
    g = torch.Generator().manual_seed(5)
    M = 2 * 17 * 19 + 3  # not a multiple of the waves per workgroup
    hidden = (2.0 * torch.randn(M, 256, generator=g)).cuda()
    w = torch.randn(256, generator=g).cuda()
    b = torch.tensor([0.37]).cuda()
    out = torch.full((M + 8,), -77.0, device="cuda")
    _lib.check(lib.cwm_raft_head_project(hidden.data_ptr(), w.data_ptr(), b.data_ptr(), M, out.data_ptr(), None))
    torch.cuda.synchronize()
    ref = (hidden.double().relu() * w.double()).sum(1) + 0.37
    err = (out[:M].double() - ref).abs().max().item()
    # 256 fp32 products summed pairwise-ish in fp32: at most 256 * 2^-24 * sum |w_c relu(h_c)|
    bound = 256 * 2.0 ** -24 * (hidden.double().relu() * w.double().abs()).sum(1).max().item()
    print(f"[head project] max-abs vs float64 {err:.3e} (fp32 summation bound {bound:.3e}, values up to {ref.abs().max().item():.1f})")
    assert err <= bound
    assert (hidden < 0).any() and torch.all(out[M:] == -77.0)  # the ReLU matters; nothing is written past M


def test_convex_upsample1_kernel_vs_restatement():
    lib = _lib.get_lib()
    g = torch.Generator().manual_seed(6)
    for P, h, w in CONVEX_SHAPES:
        value, mask = convex_case(1, P, h, w, g)
        out, guard = padded_out(P, 1, h, w)
        _lib.check(lib.cwm_raft_convex_upsample1(value.data_ptr(), mask.data_ptr(), P, h, w, out.data_ptr(), None))
        torch.cuda.synchronize()
        err = (out - upsample_restated(value, mask)).abs().max().item()  # RAFT.upsample_flow (raft_model.py:177-188), C = 1
        print(f"[convex upsample, one channel {P}x{h}x{w}] max-abs {err:.3e}")
        assert err <= 1e-4
        assert torch.all(guard == -77.0)
        # one kernel is behind both entry points: channel 0 of the two-channel call on the same mask is the same bits
        two = torch.empty(P, 2, 8 * h, 8 * w, device="cuda")
        _lib.check(lib.cwm_raft_convex_upsample(value.expand(P, 2, h, w).contiguous().data_ptr(), mask.data_ptr(), P, h, w, two.data_ptr(), None))
        torch.cuda.synchronize()
        assert torch.equal(two[:, :1], out) and torch.equal(two[:, 1:], out)


# ---- the C ABI around the head ------------------------------------------------------------------------------------------------
def _raw_args(x, iters=3):
    a = _lib.new_raft_forward_args()
    a.image1_dev, a.image2_dev = x.data_ptr(), x.data_ptr() + x.stride(1) * 4
    a.image1_stride_b = a.image2_stride_b = x.stride(0)
    a.image1_stride_c = a.image2_stride_c = x.stride(2)
    a.batch, a.pairs, a.height, a.width, a.input_scale, a.iters = x.shape[0], 1, x.shape[-2], x.shape[-1], 255.0, iters
    return a


def test_flow_mode_is_unchanged_by_loaded_head_weights():
    """The flow of a model that has the head weights loaded equals, bit for bit, the flow of the model without them; and one forward may return
    both outputs."""
    sd = S.raft_state_dict(3, output_dim=1)
    flow_model = RAFT()
    flow_model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k not in HEAD_KEYS})
    flow_model = flow_model.cuda().eval()
    x = frames(2, 128, 160, 21)
    want = flow_model(x, iters=6)
    kp = build(3)
    head = kp(x, iters=6)
    lib = _lib.get_lib()
    flow = torch.empty(2, 1, 2, 128, 160, device="cuda")
    a = _raw_args(x, iters=6)
    a.flow_dev = flow.data_ptr()
    a.flow_stride_b, a.flow_stride_c = flow.stride(0), flow.stride(2)
    _lib.check(lib.cwm_raft_forward(kp._handle, ctypes.byref(a)))  # flow only, through the handle that has the head weights
    torch.cuda.synchronize()
    assert torch.equal(flow, want)
    both_flow, both_head = torch.empty_like(flow), torch.empty(2, 1, 1, 128, 160, device="cuda")
    a.flow_dev, a.head_dev = both_flow.data_ptr(), both_head.data_ptr()
    a.head_stride_b, a.head_stride_c = both_head.stride(0), both_head.stride(2)
    _lib.check(lib.cwm_raft_forward(kp._handle, ctypes.byref(a)))
    torch.cuda.synchronize()
    assert torch.equal(both_flow, want) and torch.equal(both_head, head)


def test_head_needs_its_weights_and_struct_size_versions():
    """Asking a flow model for the head names the first missing key; a caller that passes the size of the struct as it was before the head fields
    were appended (it ended at `stream`) gets the flow and the fields behind are not read; sizes that cannot be a cwm_raft_forward_args are refused."""
    lib = _lib.get_lib()
    flow_model = RAFT()
    flow_model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(0).items()})
    flow_model = flow_model.cuda().eval()
    x = frames(1, 128, 128, 22)
    want = flow_model(x, iters=3)
    buf = ctypes.create_string_buffer(256)
    assert lib.cwm_raft_missing_weights(flow_model._handle, buf, 256) == 0
    head = torch.full((1, 1, 1, 128, 128), -5.0, device="cuda")
    a = _raw_args(x)
    a.head_dev = head.data_ptr()
    a.head_stride_b = head.stride(0)
    assert lib.cwm_raft_forward(flow_model._handle, ctypes.byref(a)) == _lib.ERR_INVALID
    assert b"output_block.0.weight" in lib.cwm_last_error()
    # three of the four loaded: the message names the one that is not
    sd = S.raft_state_dict(0, output_dim=1)
    for k in HEAD_KEYS[:2] + HEAD_KEYS[3:]:
        t = torch.from_numpy(np.asarray(sd[k])).contiguous()
        shape = (ctypes.c_int64 * t.dim())(*t.shape)
        _lib.check(lib.cwm_raft_load_weight(flow_model._handle, k.encode(), t.data_ptr(), 0, shape, t.dim()))
    assert lib.cwm_raft_forward(flow_model._handle, ctypes.byref(a)) == _lib.ERR_INVALID
    assert b"output_block.2.weight" in lib.cwm_last_error()
    bad = torch.zeros(2, 256, 1, 1)
    assert lib.cwm_raft_load_weight(flow_model._handle, HEAD_KEYS[2].encode(), bad.data_ptr(), 0, (ctypes.c_int64 * 4)(2, 256, 1, 1), 4) == _lib.ERR_INVALID
    assert b"size mismatch" in lib.cwm_last_error()
    # neither output
    a.head_dev = None
    assert lib.cwm_raft_forward(flow_model._handle, ctypes.byref(a)) == _lib.ERR_INVALID
    # the old struct size: flow as before, the head pointer behind `stream` is not read
    old_size = _lib.CwmRaftForwardArgs.stream.offset + ctypes.sizeof(ctypes.c_void_p)
    assert old_size < ctypes.sizeof(_lib.CwmRaftForwardArgs)
    flow = torch.empty(1, 1, 2, 128, 128, device="cuda")
    a.flow_dev = flow.data_ptr()
    a.flow_stride_b, a.flow_stride_c = flow.stride(0), flow.stride(2)
    a.head_dev = head.data_ptr()
    a.struct_size = old_size
    _lib.check(lib.cwm_raft_forward(flow_model._handle, ctypes.byref(a)))
    torch.cuda.synchronize()
    assert torch.equal(flow, want) and torch.all(head == -5.0)
    for size in (0, old_size - 8, 5000):
        a.struct_size = size
        assert lib.cwm_raft_forward(flow_model._handle, ctypes.byref(a)) == _lib.ERR_INVALID and b"struct_size" in lib.cwm_last_error()


def test_notebook_construction_runs(capsys):
    m = load_raft_model(None, output_dim=1)
    assert "created a new RAFT with 5552961 parameters" in capsys.readouterr().out
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(7, output_dim=1).items()}
    m.load_state_dict(sd)
    m = m.cuda().eval()
    x = frames(1, 128, 128, 23)
    y = m(x, iters=4)
    assert y.shape == (1, 1, 1, 128, 128) and torch.isfinite(y).all()
    assert torch.equal(y, build(7)(x, iters=4))
