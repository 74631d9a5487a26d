"""Host side of the multi-shift prompts (no GPU): `perturbation.MultiShiftPatchesAndMask` normalises and draws shifts as the reference
class does (recorded in tests/golden/multi_shift.npz by make_golden_multi_shift.py), refuses CPU tensors, and the fixture itself is sound."""
import json
import os

import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import perturbation, segmentation, synthetic as S, vmae

from test_motion_sampling_cpu import GOLDEN, TINY

FIXTURE = os.path.join(GOLDEN, "multi_shift.npz")
REQUIRED_CASES = ["p8_random", "p4_random_frame0", "wide_k4", "border_subpatch", "negative_subpatch", "axis_and_zero_steps", "odd_sx", "sx_multiples_of_4",
                  "chain", "overlap", "leaves_frame", "frame_minus1", "no_points", "base_mask_2d", "k1", "k_max",
                  "p6_12x24", "p6_24x12", "p12_24x24"]


def load_cases():
    g = np.load(FIXTURE)
    return g, json.loads(str(g["cases"]))


def input_frames(B, H, W, T=2, Cc=3):
    """The kernel cases' input: every pixel a distinct positive integer (the maker's `frames`)."""
    return (np.arange(B * T * Cc * H * W, dtype=np.float32) + 1).reshape(B, T, Cc, H, W)


def test_shift_sequence_normalisation_matches_the_recorded_forms():
    g, _ = load_cases()
    forms = json.loads(str(g["shift_forms"]))
    assert {"pair", "pair_in_list", "list", "tensor_2xK", "tensor_2x1", "array_2xK"} <= set(forms)
    sh = perturbation.MultiShiftPatchesAndMask(patch_size=(1, 8, 8))
    for name, f in forms.items():
        arg = {"tensor": torch.tensor, "array": np.array, "list": lambda a: tuple(a) if name == "pair" else [tuple(p) for p in a]}[f["kind"]](f["arg"])
        sh.set_num_shifts(f["K"])
        got = sh._preprocess_shifts_sequence(arg)
        assert got == [tuple(p) for p in f["want"]] and len(got) == f["K"], name
        assert all(isinstance(v, int) for p in got for v in p)
    sh.set_num_shifts(3)
    for bad in ([(1, 2), (3, 4)], torch.zeros(3, 3, dtype=torch.long), torch.zeros(2, 2, dtype=torch.long), [(1, 2, 3)]):
        with pytest.raises(AssertionError):
            sh._preprocess_shifts_sequence(bad)
    with pytest.raises(ValueError, match="whole pixels"):
        sh._preprocess_shifts_sequence((1.5, 2))


def test_random_draws_equal_the_reference_stream():
    g, _ = load_cases()
    for tag, size in [("32x48", (32, 48)), ("224", (224, 224))]:
        sh = perturbation.MultiShiftPatchesAndMask(patch_size=(1, 8, 8), max_shift_fraction=0.15)
        sh.image_size = size
        sh.set_num_shifts(6)
        got = sh._preprocess_shifts_sequence(None) + sh._preprocess_shifts_sequence(None)
        assert np.array_equal(np.array(got), g["draws_" + tag]), tag
        assert all(dy + dx != 0 for dy, dx in got)
    # the generator's instance: built from the predictor's patch size and max_shift_fraction, a numpy stream of its own (seed 0) -- drawing from it
    # leaves the single-shift stream where it was
    m = vmae.PretrainVisionTransformer(TINY)
    G = segmentation.FlowGenerator(predictor=m, flow_model=S.SyntheticFlow(), imagenet_normalize_inputs=True, temporal_dim=2, max_shift_fraction=0.5)
    shifter = G.multi_patch_shifter
    assert isinstance(shifter, perturbation.MultiShiftPatchesAndMask) and shifter.max_shift_fraction == 0.5 and shifter.patch_size[-1] == 8
    G.inp_shape = (1, 2, 3, 32, 32)
    before = G._shift_rng.get_state()[1].copy()
    shifter.image_size = (32, 32)
    shifter.set_num_shifts(3)
    drawn = [shifter._preprocess_shifts_sequence(None) for _ in range(4)]
    assert np.array_equal(np.array(drawn), g["e2e_m0_shifts"]) and np.array_equal(G._shift_rng.get_state()[1], before)
    shifter.reset_shifts()
    assert shifter.shifts is None and shifter.num_shifts == 1


def test_cpu_tensors_are_refused():
    sh = perturbation.MultiShiftPatchesAndMask(patch_size=(1, 8, 8))
    x = torch.zeros(1, 2, 3, 32, 32)
    mask = torch.ones(1, 32, 2, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="built on the GPU"):
        sh(x, mask, ~mask, [(8, 0), (0, 8)], frame=1)
    with pytest.raises(RuntimeError, match="built on the GPU"):
        perturbation.multi_shift_rows(x, mask.permute(0, 2, 1), None, np.zeros((1, 2, 2)), 8, 1)
    assert sh(x, None) == (x, None)  # (the reference returns its input for mask_sequence=None)
    with pytest.raises(NotImplementedError):
        perturbation.MultiShiftPatchesAndMask(patch_size=(1, 8, 8), allow_fractional_shifts=False)


def test_fixture_shapes_and_non_vacuity():
    g, meta = load_cases()
    assert list(meta) == REQUIRED_CASES and int(g["max_steps"]) == perturbation.MAX_STEPS == meta["k_max"]["K"] >= 8 and meta["k1"]["K"] == 1
    assert os.path.getsize(FIXTURE) < 600 * 1024
    for tag, c in meta.items():
        H, W, P, K = c["H"], c["W"], c["P"], c["K"]
        Nt = 2 * (H // P) * (W // P)
        x = input_frames(2, H, W)
        x_p, mask_ps, masks, shifts = g["case_%s_x_p" % tag], g["case_%s_mask_ps" % tag], g["case_%s_masks" % tag], g["case_%s_shifts" % tag]
        assert (H, W) in ((32, 32), (32, 48), (12, 24), (24, 12), (24, 24)) and x_p.shape == x.shape and x_p.dtype == np.float32 and mask_ps.shape == (2, Nt) and mask_ps.dtype == bool, tag
        assert shifts.shape == (K, 2) and np.abs(shifts).max() < min(H, W) and masks.shape in ((2, Nt, K), (2, Nt)), tag
        assert (("case_%s_points" % tag) in g.files) == c["has_points"] and (not c["has_points"] or g["case_%s_points" % tag].shape == (2, Nt, K))
        f = c["frame"] % 2
        assert np.array_equal(x_p[:, 1 - f], x[:, 1 - f]), tag            # the other frame is a copy
        assert c["moved"] == int((x_p[:, f] != x[:, f]).sum()) > 0, tag    # no case is vacuous
        assert c["zeros"] == int((x_p == 0).sum()), tag
        assert np.isin(x_p, np.concatenate([[0.0], x.ravel()])).all(), tag  # copies and zeros only
    assert meta["wide_k4"]["W"] == 48 and meta["p4_random_frame0"]["P"] == 4 and meta["frame_minus1"]["frame"] == -1 and not meta["no_points"]["has_points"]
    assert g["case_base_mask_2d_masks"].ndim == 2
    assert sum(c["zeros"] for c in meta.values()) > 0 and meta["border_subpatch"]["zeros"] > 0
    assert sum(c["overlap"] for c in meta.values()) > 0 and meta["overlap"]["overlap"] > 0
    assert (g["case_odd_sx_shifts"][:, 1] % 2 == 1).any() and (g["case_sx_multiples_of_4_shifts"][:, 1] % 4 == 0).all()
    assert (g["case_negative_subpatch_shifts"] < 0).any() and np.abs(g["case_negative_subpatch_shifts"]).max() < 8
    assert [list(r) for r in g["case_axis_and_zero_steps_shifts"]] == [[0, 11], [-9, 0], [0, 0]]
    # leaves_frame: the token whose destination is outside the grid is gone, the other one arrived
    assert (~g["case_leaves_frame_mask_ps"]).sum(1).tolist() == [1, 1]
    # patch sizes the 16-byte path cannot assume, on non-square grids: K >= 2, an sx that is a multiple of 4 and one that is not, zeros from outside the
    # frame, a cell two steps write to
    assert [(meta[t]["H"], meta[t]["W"], meta[t]["P"]) for t in ("p6_12x24", "p6_24x12", "p12_24x24")] == [(12, 24, 6), (24, 12, 6), (24, 24, 12)]
    for t in ("p6_12x24", "p6_24x12", "p12_24x24"):
        sx = g["case_%s_shifts" % t][:, 1]
        assert meta[t]["K"] >= 2 and (sx % 4 == 0).any() and (sx % 4 != 0).any() and meta[t]["zeros"] > 0 and meta[t]["overlap"] > 0, t
    # the end-to-end record: two movies, S = 4 rows of K = 3 steps, rectangular masks
    for movie in (0, 1):
        t = "e2e_m%d_" % movie
        assert g[t + "active"].shape == (1, 32, 3, 4) and g[t + "shifts"].shape == (4, 3, 2) and g[t + "mask"].shape == (4, 32)
        assert g[t + "videos"].shape == (4, 2, 3, 32, 32) and g[t + "flows"].shape == (4, 1, 2, 32, 32) and len(set(g[t + "mask"].sum(1).tolist())) == 1
        assert (np.abs(g[t + "shifts"]) >= 8).any() and (g[t + "shifts"] % 8 != 0).any()
