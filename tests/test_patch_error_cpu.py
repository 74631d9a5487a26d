"""The patch-error surface without a GPU: the two static mask helpers against the reference's results, the float64 restatement of the error map and mean
(tests/patch_error_restatement.py) against what the reference computed from ITS tokens (tests/golden/patch_error.npz, make_golden_patch_error.py), and
the C-ABI binding of `cwm_patch_error`."""
import ctypes
import os

import numpy as np
import pytest
import torch

import patch_error_restatement as PR
from counterfactualworldmodels_amd import _lib, config as C, prediction, synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TINY = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
G = prediction.PredictorBasedGenerator


def golden():
    return np.load(os.path.join(GOLDEN, "patch_error.npz"))


def test_unmask_one_patch_equals_the_reference():
    g = golden()
    full = torch.ones(3, TINY.num_tokens, dtype=torch.bool)
    shape = (2, 4, 4)
    assert np.array_equal(G.unmask_one_patch(full, idx=21).numpy(), g["unmask_token"])
    assert np.array_equal(G.unmask_one_patch(full, idx=(1, 2), mask_shape=shape, frame=1).numpy(), g["unmask_hw"])
    assert np.array_equal(G.unmask_one_patch(full, idx=[1, 2, 3], mask_shape=shape).numpy(), g["unmask_thw"])
    assert np.array_equal(G.unmask_one_patch(full, idx=[2, 1, 0, 3], mask_shape=shape).numpy(), g["unmask_bthw"])
    assert full.all()  # inplace=False leaves the argument alone ...
    m = full.clone()
    assert G.unmask_one_patch(m, idx=21, inplace=True).data_ptr() == m.data_ptr() and not m[:, 21].any() and m.sum() == m.numel() - 3  # ... inplace=True does not
    assert g["unmask_token"].sum() == full.numel() - 3 and g["unmask_hw"].sum() == full.numel() - 3 and g["unmask_bthw"].sum() == full.numel() - 1


def test_patch_idx_list_from_mask_equals_the_reference():
    g = golden()
    mask = torch.from_numpy(g["mask"]).view(3, 2, 4, 4)
    got = G.patch_idx_list_from_mask(mask)
    assert isinstance(got, list) and all(isinstance(p, list) and len(p) == 4 for p in got)
    assert np.array_equal(np.array(got, dtype=np.int64), g["patch_idx_list"])
    assert len(got) == int((~mask).sum()) == 3 * (16 + 4)


def check(name, got, want, rel):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    excess = np.abs(got - want) - rel * np.maximum(np.abs(got), np.abs(want))
    print("%-12s max |restatement - reference| %.3e, largest value %.3e, bound - error >= %.3e" % (name, np.abs(got - want).max(), np.abs(want).max(), -excess.max()))
    assert (excess <= 0).all(), (name, excess.max())


def test_restatement_on_the_reference_tokens_equals_the_reference():
    """Fed the reference's own predicted tokens, the float64 restatement differs from the reference's fp32 results by the reference's rounding alone:
    (C P^2 + 2) 2^-24 of each patch value, plus (T h w + 2) 2^-24 for the mean."""
    g = golden()
    x = torch.from_numpy(S.synthetic_frames(3, TINY, int(g["seed"])))
    y, mask, target = torch.from_numpy(g["y_tokens"]), torch.from_numpy(g["mask"]), torch.from_numpy(g["target_x"])
    region = 1 - torch.from_numpy(g["target_mask"]).view(3, 2, 4, 4).double()
    assert 0 < region.sum() < region.numel() and not np.array_equal(g["mask"], g["target_mask"])
    mb, nb = PR.map_bound(3, 8), PR.mean_bound(3, 8, 2 * 4 * 4)
    for name, kw in (("default", {}), ("frame0", dict(frame=0)), ("each", dict(frame=None)), ("target", dict(target=target))):
        emap = PR.error_map(y, x, mask, 8, **kw)
        check(name + "_map", emap * region, g["map" if name == "default" else name + "_map"], mb)
        check(name, PR.error_mean(emap, region), g[name], nb)
    # frame 0 is fully visible: the predicted frame 0 IS x[:, 0], so its error against target frame 0 is exactly 0, against frame 1 it is not
    e0 = PR.error_map(y, x, mask, 8, frame=0)
    assert (e0[:, 0] == 0).all() and (e0[:, 1] > 0).all()
    # the per-pixel result of aggregate_over_patches=False pools to the map
    pooled = torch.from_numpy(g["pixels"]).double().reshape(3, 2, 4, 8, 4, 8).mean((3, 5))
    check("pixels", pooled, PR.error_map(y, x, mask, 8), mb)


def test_binding_and_header():
    a = _lib.new_patch_error_args()
    assert a.struct_size == ctypes.sizeof(_lib.CwmPatchErrorArgs) == 8 + 8 + 8 * 4 + 8 * 4 + 8 + 8 + 4 * 8 + 8 * 4
    assert [f[0] for f in _lib.CwmPatchErrorArgs._fields_][:2] == ["struct_size", "y_tokens_dev"] and _lib.CwmPatchErrorArgs._fields_[-1][0] == "stream"
    assert "cwm_patch_error" in _lib.SIGNATURES
    src = open(os.path.join(ROOT, "include", "cwm_hip.h")).read()
    assert "prediction.py:324-329" in src and "prediction.py:553-574" in src
    lib = _lib.get_lib()
    # argument checks need no device: a wrong struct_size and a missing output are refused before anything is launched
    a.struct_size = 8
    assert lib.cwm_patch_error(ctypes.byref(a)) == _lib.ERR_INVALID and b"struct_size" in lib.cwm_last_error()


def test_fill_patch_args_reads_pointers_and_strides_from_the_views():
    """[B,T,C,H,W]-shaped views over a [B,C,T,H,W] tensor and over one movie at batch stride 0: the (b, t, c) strides are the views' own, in that order"""
    B, T, Cc, H, W, P = 3, 2, 3, 16, 24, 8
    x = torch.zeros((B, Cc, T, H, W)).permute(0, 2, 1, 3, 4)
    target = torch.zeros((1, T, Cc, H, W)).expand(B, -1, -1, -1, -1)
    mask, region, y = torch.zeros((B, 12), dtype=torch.bool), torch.zeros((B, T, 2, 3)), torch.zeros((B, 5, P * P * Cc))
    emap, mean, scratch = torch.zeros((B, T, 2, 3)), torch.zeros((B,)), torch.zeros((B, T, 2, 3))
    for cls in (_lib.CwmPatchErrorArgs, _lib.CwmTokenResponseArgs, _lib.CwmUnmaskStepArgs, _lib.CwmSegmentStepArgs):
        a = _lib.new_args(cls)
        g = a if cls is _lib.CwmPatchErrorArgs else a.base
        assert a.struct_size == ctypes.sizeof(cls) and g.struct_size == ctypes.sizeof(_lib.CwmPatchErrorArgs)
        assert _lib.fill_patch_args(g, x=x, target=target, mask=mask, region=region, y=y, geometry=(B, T, Cc, H, W, P), n_vis=7, frame=1, map=emap, mean=mean,
                                    scratch=scratch, stream=1234) is g
        assert (g.x_dev, g.x_stride_b, g.x_stride_t, g.x_stride_c) == (x.data_ptr(), T * Cc * H * W, H * W, T * H * W) == (x.data_ptr(),) + x.stride()[:3]
        assert (g.target_dev, g.target_stride_b, g.target_stride_t, g.target_stride_c) == (target.data_ptr(), 0, Cc * H * W, H * W)
        assert (g.y_tokens_dev, g.mask_dev, g.region_dev) == (y.data_ptr(), mask.data_ptr(), region.data_ptr())
        assert (g.batch, g.T, g.C, g.H, g.W, g.P, g.n_vis, g.frame) == (B, T, Cc, H, W, P, 7, 1)
        assert (g.map_dev, g.mean_dev, g.scratch_dev, g.stream) == (emap.data_ptr(), mean.data_ptr(), scratch.data_ptr(), 1234)
        assert g.struct_size == ctypes.sizeof(_lib.CwmPatchErrorArgs)  # left alone
    # what is not given is NULL / 0, whatever the structure held before; frame defaults to -1 (each frame against its own)
    _lib.fill_patch_args(g, mask=mask, geometry=(B, T, 0, H, W, P), stream=None)
    assert (g.x_dev, g.x_stride_c, g.target_dev, g.target_stride_t, g.y_tokens_dev, g.map_dev, g.stream, g.n_vis, g.frame) == (None, 0, None, 0, None, None, None, 0, -1)
    assert _lib.new_segment_step_args().base.T == 2 and _lib.new_unmask_step_args().struct_size == ctypes.sizeof(_lib.CwmUnmaskStepArgs)
    for bad in (x[..., ::2], x.transpose(-1, -2), x[:, :, :, :, :W - 1], x[0]):  # rows that are not contiguous, or not five dimensions
        with pytest.raises(ValueError, match="contiguous image rows"):
            _lib.fill_patch_args(_lib.new_args(_lib.CwmPatchErrorArgs), x=bad, geometry=(B, T, Cc, H, W, P), stream=None)
    with pytest.raises(ValueError, match="target"):
        _lib.fill_patch_args(_lib.new_args(_lib.CwmPatchErrorArgs), x=x, target=x[..., ::2], geometry=(B, T, Cc, H, W, P), stream=None)


def test_greedy_golden_is_decided_by_the_frames():
    g = golden()
    assert (g["greedy_picks"] - TINY.tokens_per_frame).tolist() == [5, 10, 3, 12]
    assert (g["greedy_gaps"] >= 10 * g["greedy_bounds"]).all()
    final = g["greedy_mask"].copy()
    final[0, g["greedy_picks"]] = False
    assert np.array_equal(final, g["greedy_final_mask"])
