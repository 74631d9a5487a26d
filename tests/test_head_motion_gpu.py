"""The flow -> IMU head-motion predictor `imu400_8x8patch_2frames_1tube_flowbackrgb01` on the GPU (unpadded conjoined engine
variant, flow + RGB gather kernel, dummy IMU token) against the reference's golden outputs (tests/golden/make_golden_head_motion.py),
and its wiring into the IMU-conditioned driver."""
import os

import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import _lib, config as C, conjoined_vmae as CV, segmentation, synthetic as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "imu400_8x8patch_2frames_1tube_flowbackrgb01"
FRAMES = C.VmaeConfig(name="frames_224", patch=8)
N = 784


def weights(cfg, seed, sharp=False):
    sd = {k: S.synthetic_tensor(k, shp, seed) for k, shp in C.conj_state_dict_schema(cfg).items()}
    if sharp:
        sd = S.sharpen_state_dict(sd, seed)
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def build(seed, mode="parity", sharp=False):
    m = CV.imu400_8x8patch_2frames_1tube_flowbackrgb01(flow_model=S.SyntheticFlow(), mode=mode)
    m.load_state_dict(weights(m.cfg, seed, sharp), strict=False)
    return m.cuda().eval()


def frames(batch, seed):
    x = torch.from_numpy(S.synthetic_frames(batch, FRAMES, seed)).transpose(1, 2)
    mean = torch.tensor(C.IMAGENET_MEAN).view(1, 3, 1, 1, 1)
    std = torch.tensor(C.IMAGENET_STD).view(1, 3, 1, 1, 1)
    return ((x - mean) / std).cuda()


def imu_from_video_inputs(B):
    return (torch.zeros(B, 2 * N, dtype=torch.bool, device="cuda"), torch.zeros(B, 6, 400, device="cuda"),
            torch.ones(B, 25, dtype=torch.bool, device="cuda"))


@pytest.mark.parametrize("case,seed,sharp,B", [("head_motion_b2", 0, False, 2), ("head_motion_sharp_b1", 4, True, 1)])
def test_predict_imu_configuration_vs_reference(case, seed, sharp, B):
    """fixtures (a) and (c): all-visible 784-token main stream (decoder Nm = 0), a 1-token context encoder (only the dummy)."""
    g = np.load(os.path.join(GOLDEN, case + ".npz"))
    x = frames(B, int(g["frames_seed"]))
    mask, imu, mc = imu_from_video_inputs(B)
    for mode, tol in (("parity", 1e-3), ("fast", 1e-1)):
        m = build(seed, mode, sharp)
        y = m(x, mask, x_context=imu, mask_context=mc, output_main=False, output_context=True).cpu().numpy()
        assert y.shape == g["y_ctx"].shape
        err = np.abs(y - g["y_ctx"]).max()
        print(f"[{case}] {mode} max-abs vs reference {err:.3e} (output std {g['y_ctx'].std():.3f})")
        assert err <= tol, (mode, err)


def test_masked_both_outputs_vs_reference():
    """fixture (b): equal-count masked frame-1 tokens (frame-0 halves differ, and are ignored), a partly visible IMU."""
    g = np.load(os.path.join(GOLDEN, "head_motion_masked_b2.npz"))
    x = frames(2, int(g["frames_seed"]))
    mask, mc, imu = (torch.from_numpy(g[k]).cuda() for k in ("mask", "mask_context", "imu"))
    for mode, tol in (("parity", 1e-3), ("fast", 1e-1)):
        m = build(int(g["seed"]), mode)
        y, y_c = m(x, mask, x_context=imu, mask_context=mc, output_main=True, output_context=True)
        e_m = np.abs(y.cpu().numpy() - g["y_tokens"]).max()
        e_c = np.abs(y_c.cpu().numpy() - g["y_ctx"]).max()
        print(f"[head_motion_masked_b2] {mode} max-abs vs reference: main {e_m:.3e}, context {e_c:.3e}")
        assert y.shape == g["y_tokens"].shape and y_c.shape == g["y_ctx"].shape
        assert e_m <= tol and e_c <= tol, (mode, e_m, e_c)


def test_strided_flows_and_determinism():
    m = build(0)
    x = frames(2, 0)
    mask, imu, mc = imu_from_video_inputs(2)
    fwd, bwd = m.compute_flows(x)
    fwd, bwd = fwd.contiguous(), bwd.contiguous()
    y0 = m(x, mask, x_context=imu, mask_context=mc, output_main=False, output_context=True, flows=(fwd, bwd))
    y1 = m(x, mask, x_context=imu, mask_context=mc, output_main=False, output_context=True, flows=(fwd, bwd))
    assert torch.equal(y0, y1)  # two identical forwards
    y2 = m(x, mask, x_context=imu, mask_context=mc, output_main=False, output_context=True)  # flows through flow_model
    assert torch.equal(y0, y2)
    # non-contiguous batch / channel strides (channel slices of a wider tensor, batch-major interleaving): the kernel reads them in place
    big = torch.full((2, 6, 224, 224), float("nan"), device="cuda")
    big[:, 1:3], big[:, 4:6] = fwd, bwd
    inter = torch.empty((2, 2, 2, 224, 224), device="cuda")
    inter[:, 0], inter[:, 1] = fwd.transpose(0, 1), bwd.transpose(0, 1)  # [B][which][c] storage; the views below are [B,2,H,W] with channel stride 2*2*H*W
    f_s, b_s = big[:, 1:3], big[:, 4:6]
    assert not f_s.is_contiguous() and f_s.stride(0) == 6 * 224 * 224
    y3 = m(x, mask, x_context=imu, mask_context=mc, output_main=False, output_context=True, flows=(f_s, b_s))
    assert torch.equal(y0, y3)
    f_t, b_t = inter[:, 0].transpose(0, 1), inter[:, 1].transpose(0, 1)
    assert not f_t.is_contiguous() and f_t.stride(1) == 2 * 2 * 224 * 224
    y4 = m(x, mask, x_context=imu, mask_context=mc, output_main=False, output_context=True, flows=(f_t, b_t))
    assert torch.equal(y0, y4)


def test_unequal_visible_counts_are_rejected():
    m = build(0)
    x = frames(2, 0)
    mask, imu, mc = imu_from_video_inputs(2)
    mc_bad = mc.clone()
    mc_bad[0, 3] = False  # row 0 sees one IMU token more than row 1
    with pytest.raises(_lib.CwmHipError) as e:
        m(x, mask, x_context=imu, mask_context=mc_bad, output_main=False, output_context=True)
    assert e.value.code == -1  # CWM_ERR_INVALID
    mask_bad = mask.clone()
    mask_bad[1, N + 5] = True  # row 1 hides one frame-1 token
    with pytest.raises(_lib.CwmHipError):
        m(x, mask_bad, x_context=imu, mask_context=mc, output_main=False, output_context=True)
    # the model still works afterwards
    y = m(x, mask, x_context=imu, mask_context=mc, output_main=False, output_context=True)
    assert torch.isfinite(y).all()


def test_demo_construction_and_counterfactuals_with_predicted_head_motion():
    """The demo's construction (MovabilityAndMotionCovariance.ipynb:400-431) with the stand-in flow in place of RAFT and synthetic
    weights through load_state_dict(strict=False); counterfactuals with the head motion predicted from the video."""
    from counterfactualworldmodels_amd import masking

    flow2imu_model = CV.imu400_8x8patch_2frames_1tube_flowbackrgb01()
    print(flow2imu_model.load_state_dict(weights(flow2imu_model.cfg, 0), strict=False))
    imu_conditioned_model = CV.imu400_base_4x4patch_2frames_1tube()
    print(imu_conditioned_model.load_state_dict(weights(imu_conditioned_model.cfg, 1), strict=False))
    mask_generator_4x4 = masking.RotatedTableUniformMaskingGenerator(input_size=imu_conditioned_model.mask_size, mask_ratio=0.99, clumping_factor=2)
    PsiH = segmentation.ImuConditionedFlowGenerator(
        predictor=imu_conditioned_model, head_motion_predictor=flow2imu_model, temporal_dim=2, imagenet_normalize_inputs=True,
        mask_generator=mask_generator_4x4, seed=0, flow_model=S.SyntheticFlow(), raft_iters=24).requires_grad_(False).to("cuda")
    assert hasattr(PsiH, "head_motion_generator") and flow2imu_model.flow_model is PsiH.flow_model
    x = torch.from_numpy(S.synthetic_frames(1, FRAMES, 3)).cuda()  # a moving movie [B,T,C,H,W] in [0,1)
    h_video = PsiH.predict_imu_from_video(x)
    h_static = PsiH.get_static_imu(x)
    assert h_video.shape == h_static.shape == (1, 25, 96)
    assert not torch.equal(h_video, h_static)  # a moving movie gives a different flow, hence head motion, than a static one
    active = torch.zeros(1, 2 * 56 * 56, dtype=torch.bool, device="cuda")
    active[:, 56 * 56 + 20 * 56 + 20] = True
    active = ~active  # 0 = the active patch
    kw = dict(num_samples=2, shifts=[(1, 2), (-2, 1)], fix_passive=True)
    torch.manual_seed(6)
    y_moving, f_moving = PsiH.predict_counterfactual_videos_and_flows(x, active, static_head_motion=False, sample_batch_size=1, **kw)
    torch.manual_seed(6)
    y_static, _ = PsiH.predict_counterfactual_videos_and_flows(x, active, static_head_motion=True, sample_batch_size=2, **kw)
    assert y_moving.shape == y_static.shape and f_moving.shape[:2] == (2, 1)
    assert torch.isfinite(y_moving).all() and torch.isfinite(f_moving).all()
    # the predicted head motion is exactly what is passed as head_motion: the same result through the explicit argument
    h = PsiH.head_motion_generator.reshape_output(h_video)
    torch.manual_seed(6)
    y_explicit = PsiH.predict_counterfactual_videos(x, active, head_motion=h, sample_batch_size=1, **kw)
    assert torch.equal(y_explicit, y_moving)
    torch.manual_seed(6)
    y_explicit_s = PsiH.predict_counterfactual_videos(x, active, head_motion=PsiH.head_motion_generator.reshape_output(h_static), sample_batch_size=2, **kw)
    assert torch.equal(y_explicit_s, y_static)


def test_in_kernel_normalisation_of_frame_one():
    """normalize=True: raw [0,1] frames, frame 1 imagenet-normalised inside flow_rgb_gather_kernel, against the default path that reads the
    already normalised frame (the same network input up to the rounding of the normalisation)."""
    m = build(0)
    raw = torch.from_numpy(S.synthetic_frames(2, FRAMES, 5)).transpose(1, 2).cuda()
    mean = torch.tensor(C.IMAGENET_MEAN, device="cuda").view(1, 3, 1, 1, 1)
    std = torch.tensor(C.IMAGENET_STD, device="cuda").view(1, 3, 1, 1, 1)
    x = (raw - mean) / std
    mask, imu, mc = imu_from_video_inputs(2)
    flows = m.compute_flows(raw, normalized=False)
    y_n = m(x, mask, x_context=imu, mask_context=mc, output_main=False, output_context=True, flows=flows)
    y_r = m(raw, mask, x_context=imu, mask_context=mc, output_main=False, output_context=True, flows=flows, normalize=True)
    err = (y_n - y_r).abs().max().item()
    print(f"[normalize in-kernel] max-abs vs pre-normalised input {err:.3e}")
    assert err <= 1e-4
    # a wrong normalisation would show: the raw frames read as if normalised give a different result
    y_wrong = m(raw, mask, x_context=imu, mask_context=mc, output_main=False, output_context=True, flows=flows)
    assert (y_wrong - y_n).abs().max().item() > 1e-2


def test_driver_vs_reference():
    """fixture (d): the reference's ImuConditionedFlowGenerator on tiny models -- predict_imu_from_video, get_static_imu, and
    predict_counterfactual_videos_and_flows with static_head_motion True / False for two sample_batch_size values."""
    from test_conj_oracle import TINY_CONJ
    from test_head_motion_cpu import TINY_FLOW2IMU

    from counterfactualworldmodels_amd import masking

    g = np.load(os.path.join(GOLDEN, "head_motion_driver.npz"))
    pred = CV.ConjoinedPaddedVisionTransformer(TINY_CONJ)
    pred.load_state_dict(weights(TINY_CONJ, int(g["seed_pred"])))
    f2i = CV.ConjoinedPretrainVisionTransformer(TINY_FLOW2IMU)
    f2i.load_state_dict(weights(TINY_FLOW2IMU, int(g["seed_f2i"])))
    gen = masking.RotatedTableUniformMaskingGenerator(input_size=pred.mask_size, mask_ratio=0.9, clumping_factor=2)
    G = segmentation.ImuConditionedFlowGenerator(predictor=pred, head_motion_predictor=f2i, flow_model=S.SyntheticFlow(), temporal_dim=2,
                                                 imagenet_normalize_inputs=True, mask_generator=gen, seed=0).to("cuda")
    assert G.num_head_tokens == 4 and f2i.flow_model is G.flow_model
    x, act = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["active"]).cuda()
    shifts = [list(int(v) for v in r) for r in g["shifts"]]
    torch.manual_seed(7)
    e_v = np.abs(G.predict_imu_from_video(x).cpu().numpy() - g["imu_video"]).max()
    G.set_input(x)
    e_s = np.abs(G.get_static_imu().cpu().numpy() - g["imu_static"]).max()
    print(f"[driver] imu from video {e_v:.3e}, static imu {e_s:.3e}")
    assert e_v <= 3e-4 and e_s <= 3e-4
    for static in (True, False):
        for sbs in (64, 2):
            tag = "%s_sbs%d" % ("static" if static else "video", sbs)
            torch.manual_seed(6)
            ys, fs = G.predict_counterfactual_videos_and_flows(x, active_patches=act.clone(), shifts=shifts, num_samples=4, sample_batch_size=sbs,
                                                               static_head_motion=static)
            e_y = np.abs(ys.cpu().numpy() - g["ys_" + tag]).max()
            e_f = np.abs(fs.cpu().numpy() - g["flows_" + tag]).max()
            print(f"[driver {tag}] videos {e_y:.3e}, flows {e_f:.3e}")
            assert ys.shape == g["ys_" + tag].shape and fs.shape == g["flows_" + tag].shape
            assert e_y <= 3e-4 and e_f <= 4e-3, (tag, e_y, e_f)  # the stand-in flow scales frame differences by up to 12
