"""RAFT's fast (bf16-operand) mode on the GPU (csrc/raft_kernels.hip `im2col_kernel<1>` / `corr_lookup_kernel<1>`, csrc/raft_model.hip,
`cwm_raft_forward_args.mode`), through the Python module and through the raw argument struct.

Every bound comes from the reference alone: tests/golden/raft_fast_224_b2.npz (make_golden_raft_fast.py) holds the reference evaluated on the CPU with
the operands of every convolution rounded to bf16 (`flow_emul`, `kp_emul`: cnet's batch norms folded before the rounding, as the library does) and its
distance from the fp32 reference (`err_max`, `err_mean`).
  accuracy    max-abs(fast - fp32 reference) <= 2 x err_max and mean-abs <= 1.5 x err_mean: two valid bf16-operand evaluations differ by a draw (CPU
              re-draws with 1e-5 input noise moved the max by x1.15 and the mean by x1.03; the GPU also sums in another order).
  arithmetic  max-abs(fast - emulation) < err_max = max-abs(fp32 reference - emulation): the library is closer to the emulation than the fp32
              reference is.  An implementation that rounds more than the operands of the convolutions does not pass this.
Every measured maximum is printed (run with -s) and recorded in DESIGN.md §8.5.  Measured on an MI355X: flow 0.0704 max / 0.0167 mean px vs the fp32
reference (bounds 0.135 / 0.0249), 0.0178 vs the emulation (< 0.0676); keypoint map 0.0956 / 0.0322 (0.212 / 0.0458), 0.0434 (< 0.1061)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import _lib, config as C, conjoined_vmae as CV, segmentation, synthetic as S, vmae
from counterfactualworldmodels_amd.raft import RAFT, _args, load_raft_model

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_24 = 1e-2  # px: the parity bound of tests/test_raft_gpu.py at 24 iterations


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def build(seed, mode="parity", output_dim=None, multiframe=True):
    m = RAFT(_args(output_dim=output_dim, multiframe=multiframe, mixed_precision=(mode == "fast")))
    assert m.mode == mode
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(seed, output_dim=output_dim).items()})
    return m.cuda().eval()


def frames(B, H, W, seed, **kw):
    return torch.from_numpy(S.raft_frames(B, H, W, seed, **kw)).cuda()


def check_fast(name, got, ref, emul, err_max, err_mean):
    e_max, e_mean = float(np.abs(got - ref).max()), float(np.abs(got - ref).mean())
    d_emul = float(np.abs(got - emul).max())
    print(f"[{name}] fast vs fp32 reference: max-abs {e_max:.4f} (bound 2 x {err_max:.4f}), mean-abs {e_mean:.4f} (bound 1.5 x {err_mean:.4f}); "
          f"fast vs bf16-operand emulation: max-abs {d_emul:.4f} (bound < {err_max:.4f}); |reference| max {np.abs(ref).max():.2f}")
    assert got.shape == ref.shape == emul.shape
    assert e_max <= 2.0 * err_max, (name, e_max)
    assert e_mean <= 1.5 * err_mean, (name, e_mean)
    assert d_emul < err_max, (name, d_emul)


def test_224_b2_fast_flow_vs_reference_and_emulation():
    g, f = golden("raft_224_b2"), golden("raft_fast_224_b2")
    m = build(int(f["seed"]), "fast")
    y = m(frames(2, 224, 224, int(f["frames_seed"])), iters=int(f["iters"])).cpu().numpy()
    check_fast("224_b2 flow", y, g["flow"], f["flow_emul"], float(f["err_max"]), float(f["err_mean"]))


def test_224_b2_fast_keypoint_map_vs_reference_and_emulation():
    g, f = golden("raft_keypoint_224_b2"), golden("raft_fast_224_b2")
    m = load_raft_model(None, output_dim=1, mixed_precision=True)  # the notebook's construction
    assert m.mode == "fast"
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(int(f["kp_seed"]), output_dim=1).items()})
    y = m.cuda().eval()(frames(2, 224, 224, int(f["kp_frames_seed"])), iters=int(f["iters"])).cpu().numpy()
    check_fast("224_b2 keypoint map", y, g["map"], f["kp_emul"], float(f["kp_err_max"]), float(f["kp_err_mean"]))


def test_mode_changes_the_flow_and_leaves_parity_alone():
    g = golden("raft_224_b2")
    x = frames(2, 224, 224, int(g["frames_seed"]))
    fresh = build(int(g["seed"]))(x, iters=24)
    m = build(int(g["seed"]))
    before = m(x, iters=24)
    fast1 = m.set_mode("fast")(x, iters=24)
    fast2 = m(x, iters=24)
    after = m.set_mode("parity")(x, iters=24)
    diff = (fast1 - before).abs().max().item()
    err = float(np.abs(after.cpu().numpy() - g["flow"]).max())
    print(f"[mode] fast vs parity on one handle: max-abs {diff:.4f} px; parity after fast forwards vs fp32 reference {err:.3e} px (bound {TOL_24:g})")
    assert not torch.equal(fast1, before) and diff > 0
    assert torch.equal(fast1, fast2)  # two fast forwards
    assert torch.equal(before, fresh) and torch.equal(after, fresh)  # parity before and after fast forwards: a fresh parity handle's flow
    assert err <= TOL_24
    assert torch.equal(fast1, build(int(g["seed"]), "fast")(x, iters=24))  # ... and the fast flow does not depend on the handle's history either


def test_fast_backward_equals_swapped_two_image_call():
    g = golden("raft_128x160_t3")
    x = frames(1, 128, 160, int(g["frames_seed"]), shift=tuple(int(v) for v in g["shift"]), frames=3)
    m = build(int(g["seed"]), "fast")
    m2 = build(int(g["seed"]), "fast", multiframe=False)
    yb = m(x, iters=24, backward=True)
    assert yb.shape == (1, 2, 2, 128, 160)
    for t in range(2):  # pair (x[t+1], x[t]) is stored at index 1 - t
        _, up = m2(x[:, t + 1] * 255.0, x[:, t] * 255.0, iters=24, test_mode=True)
        print(f"[fast bwd pair {t}] multi-frame vs swapped two-image call: max-abs {(up - yb[:, 1 - t]).abs().max().item():.3e}")
        assert torch.equal(up, yb[:, 1 - t])
    err = float(np.abs(yb.cpu().numpy() - g["flow_bwd"]).max())
    print(f"[fast bwd] 128x160 T=3 vs fp32 reference: max-abs {err:.4f} px (|flow| max {np.abs(g['flow_bwd']).max():.2f})")


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def _raw_args(x, out, iters):
    a = _lib.new_raft_forward_args()
    a.image1_dev, a.image2_dev = x.data_ptr(), x.data_ptr() + x.stride(1) * 4
    a.image1_stride_b = a.image2_stride_b = x.stride(0)
    a.image1_stride_c = a.image2_stride_c = x.stride(2)
    a.batch, a.pairs, a.height, a.width, a.input_scale, a.iters = x.shape[0], 1, x.shape[-2], x.shape[-1], 255.0, iters
    a.flow_dev = out.data_ptr()
    a.flow_stride_b, a.flow_stride_c = out.stride(0), out.stride(2)
    return a


def test_raw_args_mode_values_and_struct_size_versions():
    lib = _lib.get_lib()
    x = frames(2, 128, 160, 31)
    m = build(5)
    parity = m(x, iters=6)
    fast = build(5, "fast")(x, iters=6)
    assert not torch.equal(parity, fast)

    def run(mode, struct_size=None):
        out = torch.full((2, 1, 2, 128, 160), -9.0, device="cuda")
        a = _raw_args(x, out, 6)
        a.mode = mode
        if struct_size is not None:
            a.struct_size = struct_size
        rc = lib.cwm_raft_forward(m._handle, ctypes.byref(a))
        torch.cuda.synchronize()
        return rc, out

    rc0, y0 = run(0)
    rcp, yp = run(_lib.MODE_PARITY)
    rcf, yf = run(_lib.MODE_FAST)
    assert rc0 == rcp == rcf == 0
    assert torch.equal(y0, yp) and torch.equal(y0, parity)  # 0 and CWM_MODE_PARITY: parity, bit for bit
    assert torch.equal(yf, fast)  # the raw call and the module agree on fast
    rc, y = run(7)
    assert rc == _lib.ERR_INVALID and b"mode" in lib.cwm_last_error() and torch.all(y == -9.0)
    # the 0.10.1 struct ended at head_stride_c: whatever lies behind it is not read, the call is a parity call
    size_0_10_1 = _lib.CwmRaftForwardArgs.head_stride_c.offset + 8
    assert size_0_10_1 == _lib.CwmRaftForwardArgs.mode.offset < ctypes.sizeof(_lib.CwmRaftForwardArgs)
    for garbage in (7, _lib.MODE_FAST, -1):
        rc, y = run(garbage, struct_size=size_0_10_1)
        assert rc == 0 and torch.equal(y, parity), garbage
    rc, y = run(_lib.MODE_FAST, struct_size=_lib.CwmRaftForwardArgs.stream.offset + ctypes.sizeof(ctypes.c_void_p))  # the 0.10.0 size
    assert rc == 0 and torch.equal(y, parity)


# ---- the pipeline inherits the mode ---------------------------------------------------------------------------------------------------------
def test_flow_generator_predict_flow_is_the_fast_models_forward():
    cfg = C.VmaeConfig(name="tiny_224", img_size=(224, 224), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
    p = vmae.PretrainVisionTransformer(cfg)
    p.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 3).items()})
    flow_model = build(0, "fast")
    G = segmentation.FlowGenerator(predictor=p.cuda().eval(), flow_model=flow_model, imagenet_normalize_inputs=True, temporal_dim=2, raft_iters=6)
    x = frames(1, 224, 224, 2)
    got = G.predict_flow(x)
    assert got.shape == (1, 1, 2, 224, 224)
    assert torch.equal(got, flow_model(x))
    assert not torch.equal(got, build(0).set_iters(6)(x))  # and it is the fast flow, not the parity one


def test_head_motion_predictor_with_fast_raft_vs_reference():
    g = golden("head_motion_raft_b1")
    flow_model = build(int(g["raft_seed"]), "fast")
    hm = CV.imu400_8x8patch_2frames_1tube_flowbackrgb01(flow_model=flow_model)
    hm.load_state_dict({k: torch.from_numpy(S.synthetic_tensor(k, shp, int(g["seed"]))) for k, shp in C.conj_state_dict_schema(hm.cfg).items()},
                       strict=False)
    hm = hm.cuda().eval()
    assert hm.flow_model.mode == "fast"
    x01 = frames(1, 224, 224, int(g["frames_seed"])).transpose(1, 2)
    mean = torch.tensor(C.IMAGENET_MEAN, device="cuda").view(1, 3, 1, 1, 1)
    std = torch.tensor(C.IMAGENET_STD, device="cuda").view(1, 3, 1, 1, 1)
    n = hm.cfg.main.num_tokens
    y = hm((x01 - mean) / std, torch.zeros(1, 2 * n, dtype=torch.bool, device="cuda"), x_context=torch.zeros(1, 6, 400, device="cuda"),
           mask_context=torch.ones(1, 25, dtype=torch.bool, device="cuda"), output_main=False, output_context=True).cpu().numpy()
    err = float(np.abs(y - g["y_ctx"]).max())
    print(f"[head motion with fast RAFT] max-abs {err:.3e} (bound 1e-1: DESIGN.md §8.1's fast-mode bound; output std {g['y_ctx'].std():.3f})")
    assert err <= 1e-1
