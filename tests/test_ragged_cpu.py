"""The ragged-batch fixtures (tests/golden/make_golden_ragged.py: every row predicted by the reference alone, at B = 1) against the CPU oracle run row by
row, and the new model entry point's argument checks that need no device."""
import ctypes as C_
import os

import numpy as np
import torch

import pytest

from counterfactualworldmodels_amd import _lib, config as C, conjoined_vmae as CV, dist, segmentation, synthetic as S, vmae
from oracle import vmae_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
TINY_SPEC = O.VmaeSpec(img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)


def test_oracle_row_by_row_reproduces_ragged_tiny():
    g = np.load(os.path.join(GOLDEN, "ragged_tiny.npz"))
    n_vis = g["n_vis"].tolist()
    assert len(set(n_vis)) >= 3 and ((~g["mask"]).sum(1) == g["n_vis"]).all()
    W = {k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(TINY, int(g["seed"])).items()}
    x, mask = torch.from_numpy(g["x"]), torch.from_numpy(g["mask"])
    rows = g["y_tokens"].shape[1]
    assert rows == TINY.num_tokens - min(n_vis)
    with torch.no_grad():
        for b, n in enumerate(n_vis):
            video, y = O.predict(W, TINY_SPEC, x[b:b + 1], mask[b:b + 1], frame=None, return_tokens=True)
            nm = TINY.num_tokens - n
            assert y.shape == (1, nm, 192)
            assert np.abs(y[0].numpy() - g["y_tokens"][b, rows - nm:]).max() <= 1e-5
            assert (g["y_tokens"][b, :rows - nm] == 0).all()
            assert np.abs(video[0].numpy() - g["video"][b]).max() <= 1e-5


def test_oracle_row_by_row_reproduces_ragged_base8():
    g = np.load(os.path.join(GOLDEN, "ragged_base8.npz"))
    cfg = C.CONFIGS["base_8x8patch_2frames_1tube"]
    assert g["n_vis"].tolist() == [785, 792, 824] and ((~g["mask"]).sum(1) == g["n_vis"]).all()
    spec = O.VmaeSpec(img_size=cfg.img_size, patch=cfg.patch, enc_dim=cfg.enc_dim, enc_depth=cfg.enc_depth, enc_heads=cfg.enc_heads, dec_dim=cfg.dec_dim,
                      dec_depth=cfg.dec_depth, dec_heads=cfg.dec_heads)
    W = {k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, int(g["seed"])).items()}
    x, mask = torch.from_numpy(S.synthetic_frames(3, cfg, int(g["seed"]))), torch.from_numpy(g["mask"])
    with torch.no_grad():
        for b in range(3):
            y = O.vmae_forward(W, spec, O.preprocess(x[b:b + 1]), mask[b:b + 1])
            assert np.abs(y[0, ::2].numpy() - g["y%d" % b]).max() <= 1e-5


def test_set_ragged_is_bound_and_refuses_a_null_handle():
    lib = _lib.get_lib()
    assert _lib.SIGNATURES["cwm_model_set_ragged"] == (C_.c_int, [C_.c_void_p, C_.c_int])
    assert lib.cwm_model_set_ragged(None, 5) == -1 and b"cwm_model_set_ragged" in lib.cwm_last_error()


def tiny_generator(**kw):
    m = vmae.PretrainVisionTransformer(TINY, mode="parity")
    return segmentation.FlowGenerator(predictor=m, imagenet_normalize_inputs=True, temporal_dim=2, **kw)


def test_prompt_fixture_is_ragged():
    g = np.load(os.path.join(GOLDEN, "ragged_prompts_tiny.npz"))
    assert g["masks"].shape[0] >= 6 and len(set(g["n_vis"].tolist())) >= 3 and ((~g["masks"]).sum(1) == g["n_vis"]).all()
    assert g["n_vis"].min() == 16  # a prompt whose only moved patch left the frame: nothing of frame 2 is visible


def test_ragged_host_step_leaves_masks_and_global_rng_alone():
    g = np.load(os.path.join(GOLDEN, "ragged_prompts_tiny.npz"))
    masks = torch.from_numpy(g["masks"])
    G = tiny_generator(ragged_batches=True)
    assert G.ragged_batches is True
    torch.manual_seed(11)
    state = torch.get_rng_state()
    out, n_masked, rng = G._equalise(masks.clone())
    assert torch.equal(out, masks) and n_masked is None
    assert rng == (int(g["n_vis"].min()), int(g["n_vis"].max()))
    assert torch.equal(torch.get_rng_state(), state)
    # the default: the reference's rectangulariser, which draws from the global generator and changes the longer rows
    G.ragged_batches = False
    out, n_masked, rng = G._equalise(masks.clone())
    assert rng is None and n_masked == 32 - int(g["n_vis"].max()) and not torch.equal(out, masks)
    assert ((~out).sum(1) == int(g["n_vis"].max())).all()
    assert not torch.equal(torch.get_rng_state(), state)


def test_ragged_batches_are_refused_where_they_cannot_run():
    G = tiny_generator(ragged_batches=True)
    x = torch.zeros(2, 2, 3, 32, 32)
    mask = torch.zeros(2, 32, dtype=torch.bool)
    mask[0, 17:] = True
    mask[1, 20:] = True
    with pytest.raises(RuntimeError, match="fused predict path"):  # predict_tokens is the predictor's plain forward
        G.predict_tokens(x, mask)
    with pytest.raises(RuntimeError, match="fused predict path"):  # extra predictor arguments leave the fused path
        G.predict(x, mask, -1, True, None)
    with pytest.raises(NotImplementedError, match="rectangular"):
        dist.prompt_hooks(G)
    main = C.VmaeConfig(name="tiny_conj_main", img_size=(32, 32), patch=4, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
    conj = C.ConjConfig(name="tiny_conj", main=main, main_max_pad=8, ctx_seq_len=64, ctx_enc_dim=64, ctx_dec_dim=64, ctx_enc_heads=2, ctx_dec_heads=2,
                        ctx_max_pad=4, enc_cross=(0,), dec_cross=(0,))
    Gc = segmentation.FlowGenerator(predictor=CV.ConjoinedPaddedVisionTransformer(conj), imagenet_normalize_inputs=True, temporal_dim=2, ragged_batches=True)
    with pytest.raises(RuntimeError, match="null-token padding"):
        Gc._equalise(torch.zeros(2, 128, dtype=torch.bool))
    G.ragged_batches = False
    dist.prompt_hooks(G)  # and with the option off the hooks are there as before
