"""The flow -> IMU head-motion predictor `imu400_8x8patch_2frames_1tube_flowbackrgb01` on the host: state-dict schema against the
reference's (captured in tests/golden/head_motion_b2.npz), the factory's attribute surface, the IMU layout helpers, the stand-in
flow's contract and the errors.  No GPU needed."""
import json
import os

import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import config as C, conjoined_vmae as CV, segmentation, synthetic as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "imu400_8x8patch_2frames_1tube_flowbackrgb01"
# a tiny flow -> IMU model built as the reference factory builds the shipped one, paired with test_conj_oracle.TINY_CONJ (same frames and
# IMU length) in the driver fixture head_motion_driver.npz
TINY_FLOW2IMU = C.ConjConfig(
    name="tiny_flow2imu", main=C.VmaeConfig(name="tiny_flow2imu_main", img_size=(32, 32), patch=8, num_frames=1, in_chans=7, enc_dim=128,
                                            enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2),
    main_max_pad=0, ctx_seq_len=64, ctx_enc_dim=64, ctx_dec_dim=64, ctx_enc_heads=2, ctx_dec_heads=2, ctx_max_pad=0, enc_cross=(0, 1),
    dec_cross=(0,), padded=False, ctx_dummy_token=True, main_input="flowback_rgb01")


def test_schema_equals_the_reference_keys_shapes_and_order():
    keys = json.loads(str(np.load(os.path.join(GOLDEN, "head_motion_b2.npz"))["keys"]))
    sch = C.conj_state_dict_schema(C.CONJ_CONFIGS[NAME])
    assert [(k, list(v)) for k, v in sch.items()] == [(k, v) for k, v in keys]
    assert len(sch) == 583
    assert sum(int(np.prod(v)) for v in sch.values()) == 135_730_048
    assert list(sch).index("context_stream.encoder.dummy_token") == 219


def test_existing_conj_schema_unchanged():
    sch = C.conj_state_dict_schema(C.CONJ_CONFIGS["imu400_base_4x4patch_2frames_1tube"])
    assert len(sch) == 634
    assert "main_stream.null_token_enc" in sch and "context_stream.null_token_dec" in sch
    assert not any("dummy_token" in k for k in sch)
    cfg = C.CONJ_CONFIGS["imu400_base_4x4patch_2frames_1tube"]
    assert cfg.padded and not cfg.ctx_dummy_token and cfg.main_input == "rgb01"


def test_factory_attributes():
    m = CV.imu400_8x8patch_2frames_1tube_flowbackrgb01()
    assert m.mask_size == (2, 28, 28)
    assert m.context_stream.encoder.num_tokens == 25
    assert m.context_stream.patch_size == (16, 1, 1)
    assert m.get_context_input.num_channels == 6
    assert m.get_main_input.num_channels == 7
    assert not hasattr(m, "padding_mask")
    sd = m.state_dict()
    assert len(sd) == 583 and tuple(sd["main_stream.encoder.patch_embed.proj.weight"].shape) == (768, 7, 1, 8, 8)
    # load_state_dict(strict=False) as the demo notebook calls it, with a checkpoint that has extra and missing keys
    part = {k: torch.zeros(v.shape) for k, v in list(sd.items())[:5]}
    part["some.extra.key"] = torch.zeros(3)
    r = m.load_state_dict(part, strict=False)
    assert r.unexpected_keys == ["some.extra.key"] and len(r.missing_keys) == 578


def test_reshape_output_layout():
    m = CV.imu400_8x8patch_2frames_1tube_flowbackrgb01()
    G = segmentation.ImuGenerator(predictor=m, temporal_dim=2)
    y = torch.arange(2 * 25 * 96, dtype=torch.float32).reshape(2, 25, 96)
    h = G.reshape_output(y)
    assert h.shape == (2, 6, 400)
    # 'b t (pt c) -> b c (t pt)' (segmentation.py:645-649)
    for b, t, pt, c in ((0, 0, 0, 0), (1, 3, 5, 2), (1, 24, 15, 5)):
        assert h[b, c, t * 16 + pt] == y[b, t, pt * 6 + c]
    assert torch.equal(G.reshape_input(h), y)
    assert G.num_head_tokens == 25 and G._is_padded is False
    assert G.mask_generator(torch.zeros(2, 2, 3, 224, 224)).sum() == 0  # all visible


def test_synthetic_flow_contract():
    f = S.SyntheticFlow()
    g = np.random.Generator(np.random.PCG64(0))
    moving = torch.from_numpy(g.random((2, 2, 3, 32, 24), dtype=np.float32))
    static = moving[:, :1].expand(-1, 2, -1, -1, -1)
    fw, bw = f(moving, iters=24, backward=False), f(moving, iters=24, backward=True)
    assert fw.shape == bw.shape == (2, 1, 2, 32, 24)
    assert torch.equal(f(moving), fw)  # deterministic
    assert not torch.allclose(fw, f(static))  # content dependent
    assert not torch.allclose(fw[:, :, 0], fw[:, :, 1])  # x differs from y
    assert not torch.allclose(fw, bw) and not torch.allclose(fw, -bw)  # not a negation
    assert fw.abs().max() > 3.0 and bw.abs().max() > 3.0  # several pixels
    assert len(list(f.parameters())) == 0


def test_construction_without_flow_model_and_errors():
    m = CV.imu400_8x8patch_2frames_1tube_flowbackrgb01()
    assert m.flow_model is None
    with pytest.raises(RuntimeError, match="flow_model"):
        m.compute_flows(torch.zeros(1, 3, 2, 224, 224))
    with pytest.raises(RuntimeError, match="flow_model"):  # a forward without a flow model (checked before any device work)
        m(torch.zeros(1, 3, 2, 224, 224), torch.zeros(1, 2 * 784, dtype=torch.bool), x_context=torch.zeros(1, 6, 400), output_context=True)
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 3, 2, 224, 224), torch.zeros(1, 2 * 784, dtype=torch.bool), timestamps=torch.zeros(1, 2))
    # the IMU-conditioned driver without a head-motion predictor keeps its behaviour: no head_motion_generator attribute
    P = CV.imu400_base_4x4patch_2frames_1tube()
    G = segmentation.ImuConditionedFlowGenerator(predictor=P, temporal_dim=2, imagenet_normalize_inputs=True)
    assert not hasattr(G, "head_motion_generator")
    with pytest.raises(RuntimeError, match="head_motion"):
        G._conditioning_kwargs(torch.zeros(1, 2, 3, 224, 224), {})
    # with one, the generator's flow model is handed to the head-motion predictor
    flow = S.SyntheticFlow()
    G2 = segmentation.ImuConditionedFlowGenerator(predictor=P, head_motion_predictor=m, flow_model=flow, temporal_dim=2, imagenet_normalize_inputs=True)
    assert G2.head_motion_generator.predictor is m and m.flow_model is flow
    assert G2.num_head_tokens == 25 and G2.head_tubelet_size == 16 and G2.head_motion_channels == 6
    # the head-motion layout follows the head-motion predictor (segmentation.py:799-809), not the conditioned one
    from test_conj_oracle import TINY_CONJ

    G3 = segmentation.ImuConditionedFlowGenerator(predictor=CV.ConjoinedPaddedVisionTransformer(TINY_CONJ),
                                                  head_motion_predictor=CV.ConjoinedPretrainVisionTransformer(TINY_FLOW2IMU), flow_model=flow,
                                                  temporal_dim=2)
    assert G3._head_model() is G3.head_motion_generator.predictor
    assert G3.num_head_tokens == TINY_FLOW2IMU.ctx_tokens == 4
    h, h_mask = G3.get_fake_head_motion(torch.zeros(2, 2, 3, 32, 32))
    assert h.shape == (2, 6, 64) and h_mask.shape == (2, 4) and bool(h_mask.all())


def test_tiny_schema_equals_the_reference_keys():
    keys = json.loads(str(np.load(os.path.join(GOLDEN, "head_motion_driver.npz"))["keys"]))
    sch = C.conj_state_dict_schema(TINY_FLOW2IMU)
    assert [(k, list(v)) for k, v in sch.items()] == [(k, v) for k, v in keys]
