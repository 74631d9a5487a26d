"""RAFT-large on the GPU (csrc/raft_kernels.hip, csrc/raft_model.hip) against the reference's golden outputs (tests/golden/make_golden_raft.py),
its stand-alone lookup / upsampling kernels against torch restatements of the reference's semantics, and its use as the flow model of the
flow -> IMU head-motion predictor."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from counterfactualworldmodels_amd import _lib, config as C, conjoined_vmae as CV, synthetic as S
from counterfactualworldmodels_amd.raft import RAFT, load_raft_model

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_24 = 1e-2  # px, max-abs at 24 iterations
TOL_1 = 5e-3   # px, max-abs at 1 iteration


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def build(seed, multiframe=True):
    m = RAFT()
    m.multiframe = multiframe
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(seed).items()})
    return m.cuda().eval()


def frames(B, H, W, seed, **kw):
    return torch.from_numpy(S.raft_frames(B, H, W, seed, **kw)).cuda()


def check(name, got, want, tol):
    err = float(np.abs(got - want).max())
    print(f"[{name}] max-abs {err:.3e} px (bound {tol:g}, |flow| max {np.abs(want).max():.2f})")
    assert got.shape == want.shape
    assert err <= tol, (name, err)


def test_224_b2_forward_vs_reference():
    g = golden("raft_224_b2")
    m = build(int(g["seed"]))
    y = m(frames(2, 224, 224, int(g["frames_seed"])), iters=int(g["iters"])).cpu().numpy()
    print(f"reference fp32 vs float64: {float(g['drift']):.3e} px")
    check("224_b2", y, g["flow"], TOL_24)


def test_224_b1_two_image_call_vs_reference():
    g = golden("raft_224_b1")
    m = build(int(g["seed"]), multiframe=False)
    x = frames(1, 224, 224, int(g["frames_seed"])) * 255.0
    low, up = m(x[:, 0], x[:, 1], iters=1, test_mode=True)
    check("224_b1 it1 up", up.cpu().numpy(), g["flow_it1"], TOL_1)
    check("224_b1 it1 low", low.cpu().numpy(), g["flow_low_it1"], TOL_1)
    low, up = m(x[:, 1], x[:, 0], iters=24, test_mode=True)
    check("224_b1 bwd up", up.cpu().numpy(), g["flow_bwd"], TOL_24)
    check("224_b1 bwd low", low.cpu().numpy(), g["flow_low_bwd"], TOL_24)


def test_224_b1_multiframe_backward_matches_two_image_call():
    g = golden("raft_224_b1")
    m = build(int(g["seed"]))
    y = m(frames(1, 224, 224, int(g["frames_seed"])), iters=24, backward=True).cpu().numpy()
    check("224_b1 multiframe bwd", y[:, 0], g["flow_bwd"], TOL_24)


def test_128x160_t3_forward_and_backward_vs_reference():
    g = golden("raft_128x160_t3")
    m = build(int(g["seed"]))
    x = frames(1, 128, 160, int(g["frames_seed"]), shift=tuple(int(v) for v in g["shift"]), frames=3)
    check("128x160 fwd", m(x, iters=24).cpu().numpy(), g["flow_fwd"], TOL_24)
    check("128x160 bwd", m(x, iters=24, backward=True).cpu().numpy(), g["flow_bwd"], TOL_24)


def test_136x152_b2_odd_grid_vs_reference():
    """An odd 1/8 grid, 17 x 19: the floor-pooled pyramid 17/8/4/2 x 19/9/4/2 drops a row and a column at the first pooling and again at 9 -> 4, the
    7x7 / 3x3 borders fall on odd sides, and no row count is a multiple of a GEMM tile."""
    g = golden("raft_136x152_b2")
    m = build(int(g["seed"]))
    x = frames(2, 136, 152, int(g["frames_seed"]), shift=tuple(int(v) for v in g["shift"]))
    print(f"reference fp32 vs float64: {float(g['drift']):.3e} px (24 iterations), {float(g['drift_it1']):.3e} px (1 iteration)")
    check("136x152 it24", m(x, iters=24).cpu().numpy(), g["flow"], TOL_24)
    check("136x152 it1", m(x, iters=1).cpu().numpy(), g["flow_it1"], TOL_1)


# ---- stand-alone kernels against torch restatements --------------------------------------------------------------------
def lookup_restated(f1, f2, coords):
    """CorrBlock (corr.py:12-60) restated: all-pairs dot products / sqrt(256), 3 x avg_pool2d(2), and at level l the 9 x 9 window of
    grid_sample(align_corners=True) samples at (x / 2^l + a - 4, y / 2^l + b - 4), feature l*81 + a*9 + b."""
    P, h, w, D = f1.shape
    corr = torch.matmul(f1.reshape(P, h * w, D), f2.reshape(P, h * w, D).transpose(1, 2)) / 16.0
    lvl = corr.reshape(P * h * w, 1, h, w)
    c = coords.reshape(P * h * w, 1, 1, 2)
    d = torch.arange(-4, 5, device=f1.device, dtype=torch.float32)
    dx = d.view(9, 1).expand(9, 9)  # first window index moves x
    dy = d.view(1, 9).expand(9, 9)
    out = []
    for l in range(4):
        if l:
            lvl = F.avg_pool2d(lvl, 2, stride=2)
        H, W = lvl.shape[-2:]
        x = c[..., 0] / 2**l + dx
        y = c[..., 1] / 2**l + dy
        grid = torch.stack([2 * x / (W - 1) - 1, 2 * y / (H - 1) - 1], -1)
        out.append(F.grid_sample(lvl, grid, align_corners=True).reshape(P, h, w, 81))
    return torch.cat(out, -1)


def test_corr_lookup_kernel_vs_restatement():
    lib = _lib.get_lib()
    g = torch.Generator().manual_seed(3)
    P, h, w = 2, 20, 17
    f1 = torch.randn(P, h, w, 256, generator=g).cuda()
    f2 = torch.randn(P, h, w, 256, generator=g).cuda()
    base = torch.stack(torch.meshgrid(torch.arange(w, dtype=torch.float32), torch.arange(h, dtype=torch.float32), indexing="xy"), -1)
    coords = (base.unsqueeze(0) + 9.0 * (torch.rand(P, h, w, 2, generator=g) - 0.5)).cuda()  # fractional, partly outside the maps
    coords[0, 0, 0] = torch.tensor([-30.0, 50.0])
    out = torch.empty(P, h, w, 324, device="cuda")
    _lib.check(lib.cwm_raft_corr_lookup(f1.data_ptr(), f2.data_ptr(), coords.data_ptr(), P, h, w, out.data_ptr(), None))
    ref = lookup_restated(f1, f2, coords)
    err = (out - ref).abs().max().item()
    print(f"[corr lookup] max-abs {err:.3e} (values up to {ref.abs().max().item():.2f}, zeros {(ref == 0).float().mean().item():.3f})")
    assert err <= 1e-4 * max(1.0, ref.abs().max().item())
    assert (ref == 0).any()  # the test reaches the zero padding


def upsample_restated(field, mask):
    """RAFT.upsample_flow (raft_model.py:177-188) of a field [P, C, h, w] with the mask [P, h, w, 576], on the device of its inputs."""
    P, C, h, w = field.shape
    m = torch.softmax(mask.permute(0, 3, 1, 2).reshape(P, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(8 * field, [3, 3], padding=1).view(P, C, 9, 1, 1, h, w)
    return torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(P, C, 8 * h, 8 * w)


# 2 x 3 x 5: fourteen of the fifteen low-resolution pixels touch a border (every zero-padded neighbour pattern, the four corners included), and the 1920 outputs
# per channel are no multiple of 256: the last workgroup is partial
CONVEX_SHAPES = ((3, 16, 19), (2, 3, 5))


def convex_case(C, P, h, w, g):
    """Inputs of one convex-upsampling case on the GPU: the field [P, C, h, w] and the mask; the restatement is checked on the CPU first (finite, and no
    channel constant: at a shape this small a degenerate reference would pass anything)."""
    field = 3.0 * torch.randn(P, C, h, w, generator=g)
    mask = 2.0 * torch.randn(P, h, w, 576, generator=g)
    ref = upsample_restated(field, mask)
    assert ref.shape == (P, C, 8 * h, 8 * w) and torch.isfinite(ref).all() and (ref.flatten(2).std(dim=2) > 0).all()
    return field.cuda(), mask.cuda()


def padded_out(P, C, h, w):
    """An output buffer with 64 floats behind it that no launch may touch: (view, the guard)."""
    n = P * C * 64 * h * w
    buf = torch.full((n + 64,), -77.0, device="cuda")
    return buf[:n].view(P, C, 8 * h, 8 * w), buf[n:]


def test_convex_upsample_kernel_vs_restatement():
    lib = _lib.get_lib()
    g = torch.Generator().manual_seed(4)
    for P, h, w in CONVEX_SHAPES:
        flow, mask = convex_case(2, P, h, w, g)
        out, guard = padded_out(P, 2, h, w)
        _lib.check(lib.cwm_raft_convex_upsample(flow.data_ptr(), mask.data_ptr(), P, h, w, out.data_ptr(), None))
        torch.cuda.synchronize()
        err = (out - upsample_restated(flow, mask)).abs().max().item()
        print(f"[convex upsample {P}x{h}x{w}] max-abs {err:.3e}")
        assert err <= 1e-4
        assert torch.all(guard == -77.0)


# ---- integration, determinism, batching, errors ---------------------------------------------------------------------
def test_head_motion_predictor_with_raft_vs_reference(tmp_path):
    g = golden("head_motion_raft_b1")
    ckpt = str(tmp_path / "raft-synthetic.pth")  # a DataParallel-style checkpoint: load_raft_model strips `module.`
    torch.save({"module." + k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(int(g["raft_seed"])).items()}, ckpt)
    flow_model = load_raft_model(ckpt).cuda().eval()
    hm = CV.imu400_8x8patch_2frames_1tube_flowbackrgb01(flow_model=flow_model)
    hm.load_state_dict({k: torch.from_numpy(S.synthetic_tensor(k, shp, int(g["seed"]))) for k, shp in C.conj_state_dict_schema(hm.cfg).items()},
                       strict=False)
    hm = hm.cuda().eval()
    x01 = frames(1, 224, 224, int(g["frames_seed"])).transpose(1, 2)
    mean = torch.tensor(C.IMAGENET_MEAN, device="cuda").view(1, 3, 1, 1, 1)
    std = torch.tensor(C.IMAGENET_STD, device="cuda").view(1, 3, 1, 1, 1)
    n = hm.cfg.main.num_tokens
    y = hm((x01 - mean) / std, torch.zeros(1, 2 * n, dtype=torch.bool, device="cuda"), x_context=torch.zeros(1, 6, 400, device="cuda"),
           mask_context=torch.ones(1, 25, dtype=torch.bool, device="cuda"), output_main=False, output_context=True).cpu().numpy()
    err = float(np.abs(y - g["y_ctx"]).max())
    print(f"[head motion with RAFT] max-abs {err:.3e} (output std {g['y_ctx'].std():.3f})")
    assert err <= 1e-3


def test_forward_is_deterministic():
    m = build(0)
    x = frames(2, 128, 128, 9)
    a = m(x, iters=6)
    b = m(x, iters=6)
    assert torch.equal(a, b)


def test_batch_rows_agree_with_single_runs():
    m = build(1)
    for H, W in ((128, 160), (136, 152)):  # an even 16 x 20 grid and an odd 17 x 19 one
        x = frames(3, H, W, 10)
        y = m(x, iters=12)
        for b in range(3):
            y1 = m(x[b : b + 1].clone(), iters=12)
            err = (y[b : b + 1] - y1).abs().max().item()
            print(f"[batch row {b} of {H}x{W}] max-abs vs batch-1 run {err:.3e}")
            assert err <= TOL_24


@pytest.mark.parametrize("H,W,iters", [(100, 128, 4), (64, 64, 4), (128, 128, 0)])
def test_invalid_shapes_and_iterations_raise(H, W, iters):
    m = build(0)
    with pytest.raises(_lib.CwmHipError):
        m(torch.rand(1, 2, 3, H, W, device="cuda"), iters=iters)


def test_missing_weight_raises():
    import ctypes

    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(0).items()}
    lib = _lib.get_lib()
    hh = ctypes.c_void_p()
    _lib.check(lib.cwm_raft_create(ctypes.byref(hh)))
    try:
        for k, v in list(sd.items())[:-1]:  # everything but update_block.mask.2.bias
            t = v.float().contiguous()
            shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
            _lib.check(lib.cwm_raft_load_weight(hh.value, k.encode(), t.data_ptr(), 0, shape, t.dim()))
        buf = ctypes.create_string_buffer(256)
        assert lib.cwm_raft_missing_weights(hh.value, buf, 256) == 1
        assert buf.value.decode() == "update_block.mask.2.bias"
        x = torch.rand(1, 2, 3, 128, 128, device="cuda")
        out = torch.empty(1, 1, 2, 128, 128, device="cuda")
        a = _lib.new_raft_forward_args()
        a.image1_dev, a.image2_dev = x.data_ptr(), x.data_ptr() + x.stride(1) * 4
        a.image1_stride_b = a.image2_stride_b = x.stride(0)
        a.image1_stride_c = a.image2_stride_c = x.stride(2)
        a.batch, a.pairs, a.height, a.width, a.input_scale, a.iters = 1, 1, 128, 128, 255.0, 2
        a.flow_dev = out.data_ptr()
        a.flow_stride_b, a.flow_stride_c = out.stride(0), out.stride(2)
        with pytest.raises(_lib.CwmHipError, match="missing"):
            _lib.check(lib.cwm_raft_forward(hh.value, ctypes.byref(a)))
    finally:
        lib.cwm_raft_destroy(hh.value)


def test_iters_attribute_overrides_the_call():
    m = build(0)
    x = frames(1, 128, 128, 11)
    want = m(x, iters=3)
    m.set_iters(3)
    assert m.iters == 3
    assert torch.equal(m(x, iters=10), want)
    m.iters = None
    assert not torch.equal(m(x, iters=10), want)
