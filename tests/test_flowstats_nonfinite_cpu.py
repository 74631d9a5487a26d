"""The case table of tests/flowstats_nonfinite_cases.py against the oracle (oracle/flowstats_oracle.py: torch's own amin / amax / clamp / cov / corrcoef): the facts
tests/test_flowstats_nonfinite_gpu.py relies on when it compares the kernels with the oracle on these cases.  If the table changed so that a poison no longer
reached the output, or reached all of it under every option, the GPU comparison would still pass and say nothing; here it fails.  No GPU needed."""
import pytest
import torch

import flowstats_nonfinite_cases as NC
from oracle import flowstats_oracle as FO


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("shape", list(NC.MOTION_SHAPES))
def test_motion_map_poisons_reach_the_output_as_tabulated(shape):
    _, _, S, H, W = NC.MOTION_SHAPES[shape]
    HW = H * W
    for C in NC.CHANNELS:
        clean = NC.clean_flows(C, H, W, S, 1000 + S + C)
        poisons = NC.motion_poisons(C, HW, S)
        assert len(poisons) == 14
        if S == 512:  # the second 256-sample piece of the whole-wave form holds poisoned samples
            assert sum(any(s is not None and s >= 256 for _, s, _, _ in pl) for pl in poisons.values()) >= 8
        assert HW - 64 * ((HW - 1) // 64) < 64 and NC.partial_pixel(HW) >= 64 * ((HW - 1) // 64)   # the last 64-pixel workgroup is partial and holds that pixel
        for nps, nm in NC.OPTION_PAIRS:
            ref_clean = FO.compute_mean_motion_map(clean, nps, nm)
            assert torch.isfinite(ref_clean).all()
            for name, placement in poisons.items():
                ref = FO.compute_mean_motion_map(NC.poisoned(clean, placement), nps, nm)
                isnan, isinf = NC.expected_pattern(placement, HW, nps, nm)
                key = (shape, C, name, nps, nm)
                assert torch.equal(torch.isnan(ref[0]).view(-1), isnan), key
                assert torch.equal(torch.isinf(ref[0]).view(-1), isinf), key
                assert _same_bits(ref[1], ref_clean[1]), key
                if (nps, nm) in NC.finite_pairs(placement):
                    nan_pix, inf_pix = NC.poisoned_pixels(placement, HW)
                    assert torch.isfinite(ref[0].view(-1)[~(nan_pix | inf_pix)]).all(), key
        for name, placement in poisons.items():
            assert NC.finite_pairs(placement), name


def test_issue_table_counts():
    """the counts of the table this work started from: [2, 2, 6, 10, 24], one poisoned value in batch row 0 -- 1 pixel or all 60"""
    clean = NC.clean_flows(2, 6, 10, 24, 7)
    for v, want in ((NC.NAN, {(False, False): (1, 0), (False, True): (60, 0), (True, False): (60, 0), (True, True): (60, 0)}),
                    (NC.INF, {(False, False): (0, 1), (False, True): (1, 0), (True, False): (1, 0), (True, True): (60, 0)}),
                    (-NC.INF, {(False, False): (0, 1), (False, True): (1, 0), (True, False): (1, 0), (True, True): (60, 0)}),
                    (3e19, {(False, False): (0, 1), (False, True): (1, 0), (True, False): (1, 0), (True, True): (60, 0)})):
        placement = [(17, 5, 1, v)]
        for (nps, nm), (n_nan, n_inf) in want.items():
            ref = FO.compute_mean_motion_map(NC.poisoned(clean, placement), nps, nm)
            assert (int(torch.isnan(ref[0]).sum()), int(torch.isinf(ref[0]).sum())) == (n_nan, n_inf), (v, nps, nm)
            assert torch.isfinite(ref[1]).all()
            isnan, isinf = NC.expected_pattern(placement, 60, nps, nm)
            assert (int(isnan.sum()), int(isinf.sum())) == (n_nan, n_inf)


@pytest.mark.parametrize("shape", list(NC.MOTION_SHAPES))
def test_flat_samples_take_the_eps_branch(shape):
    _, _, S, H, W = NC.MOTION_SHAPES[shape]
    for C in NC.CHANNELS:
        fl = NC.flat_flows("flat samples", C, H, W, S, 2000 + S + C)
        mags = fl.square().sum(1).sqrt().view(NC.BATCH, H * W, S)
        rng = mags.amax(1) - mags.amin(1)
        assert (rng[:, 0] == 0).all() and (rng[:, S - 1] > 0).all() and (rng[:, S - 1] < NC.EPS).all() and (rng[:, 1:S - 1] > 1.0).all()
        norm = FO.compute_flow_samples_magnitude(fl, True, eps=NC.EPS).view(NC.BATCH, H * W, S)
        assert (norm[..., 0] == 0).all() and abs(norm[..., S - 1].max().item() - 0.125) < 1e-3   # divided by eps, not by its range
        fl = NC.flat_flows("all flat", C, H, W, S, 3000 + S + C)
        mags = fl.square().sum(1).sqrt().view(NC.BATCH, H * W, S)
        assert ((mags.amax(1) - mags.amin(1)) < NC.EPS).all() and (mags.amax(1) > mags.amin(1)).all()
        mean = FO.compute_mean_motion_map(fl, False, False).view(NC.BATCH, -1)
        assert ((mean.amax(1) - mean.amin(1)) < NC.EPS).all() and ((mean.amax(1) - mean.amin(1)) > 0).all()
        assert FO.compute_mean_motion_map(fl, False, True).amax().item() < 0.999   # the map's own range: the finish divides by eps
        assert torch.equal(mags * 1024, (mags * 1024).round()) and mags.max().item() < 0.09   # multiples of 2^-10: sums of 512 are exact in fp32


@pytest.mark.parametrize("shape", list(NC.FINISH_SHAPES))
def test_finish_maps(shape):
    H, W = NC.FINISH_SHAPES[shape]
    HW = H * W
    assert {"registers 360": HW % 4 == 0 and HW <= 65536, "loop 63": HW % 4 != 0, "loop 66048": HW > 65536 and HW % 4 == 0}[shape]
    maps = NC.finish_maps(H, W, 40 + HW)
    ref_clean = FO.compute_mean_motion_map(maps["clean"])
    assert torch.isfinite(ref_clean).all()
    want = {"nan first": (HW, 0), "nan last": (HW, 0), "nan between": (HW, 0), "+inf between": (1, 0), "-inf between": (HW, 0),
            "+inf first and -inf last": (HW, 0), "flat": (0, 0), "clean": (0, 0)}
    assert set(want) == set(maps)
    for name, m in maps.items():
        ref = FO.compute_mean_motion_map(m)
        assert (int(torch.isnan(ref[0]).sum()), int(torch.isinf(ref[0]).sum())) == want[name], name
        assert _same_bits(ref[1], ref_clean[1]), name
    flat = maps["flat"][0]
    assert 0 < (flat.max() - flat.min()).item() < NC.EPS and FO.compute_mean_motion_map(maps["flat"])[0].max().item() < 0.999


@pytest.mark.parametrize("shape", list(NC.COV_SHAPES))
def test_covariance_poisons_zero_their_own_row_and_column_only(shape):
    H, W, ds, S, mode = NC.COV_SHAPES[shape]
    P = (H // ds) * (W // ds)
    assert NC.cov_mode(P, S) == mode and P % 128 == (0 if mode == 2 else 8)
    clean = NC.clean_flows(2, H, W, S, 500 + S + ds)
    x_clean = FO.flow_features(clean, ds)
    poisons = NC.cov_poisons(H, W, ds, S)
    assert len(poisons) == (10 if ds > 1 else 9)
    for use_cov in (True, False):
        ref_clean = FO.compute_flow_corrs(clean, ds, use_cov).reshape(NC.BATCH, P, P)
        assert torch.isfinite(ref_clean).all() and ref_clean[0].diagonal().abs().min().item() > 0
        for name, (placement, positions) in poisons.items():
            fl = NC.cov_poisoned(clean, placement)
            x = FO.flow_features(fl, ds)
            bad = ~torch.isfinite(x[0]).all(-1)
            assert bad.nonzero().view(-1).tolist() == positions, (name, "the features' poisoned positions")
            assert torch.isfinite(x[1]).all() and _same_bits(x[0][~bad], x_clean[0][~bad]) and _same_bits(x[1], x_clean[1])
            if name == "+inf and -inf in one cell":
                assert torch.isnan(x[0, positions[0], 3]) and not torch.isinf(x[0]).any()
            ref = FO.compute_flow_corrs(fl, ds, use_cov).reshape(NC.BATCH, P, P)
            assert torch.isfinite(ref).all(), name
            assert not ref[0][bad].any() and not ref[0][:, bad].any(), (name, use_cov)
            keep = ~bad[:, None] & ~bad[None, :]
            assert _same_bits(ref[0][keep], ref_clean[0][keep]) and _same_bits(ref[1], ref_clean[1]), (name, use_cov)
