"""NaN, Inf and flat flow samples through every kernel form of the motion maps, both paths of the finish kernel and the three load modes of the covariance kernel,
on a real MI355X against the CPU oracle (oracle/flowstats_oracle.py: torch's own amin / amax / clamp / cov / corrcoef).  The cases are
tests/flowstats_nonfinite_cases.py; tests/test_flowstats_nonfinite_cpu.py holds them against the oracle, so that a comparison here cannot be vacuous.  Every other
flow-statistics test draws finite random samples whose ranges are far above eps: nothing else reaches a NaN range, an infinite one, or the branch that divides by eps.

Each test walks its whole matrix of cases and reports every one that misses, by name."""
import pytest
import torch

import flowstats_nonfinite_cases as NC
from counterfactualworldmodels_amd import flowstats as FS
from oracle import flowstats_oracle as FO

pytestmark = pytest.mark.gpu
TOL = 1e-5  # tests/test_flowstats_gpu.py: fp32 statistics against torch's summation order


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _miss(out, ref, bound):
    """why `out` (device result, on the CPU) is not `ref` (the oracle's): the NaN pattern, the Inf pattern (with sign), or a finite value beyond `bound`; None if it is"""
    if out.shape != ref.shape:
        return "shape %s != %s" % (tuple(out.shape), tuple(ref.shape))
    if not torch.equal(torch.isnan(out), torch.isnan(ref)):
        return "isnan: %d of the oracle's %d" % (int(torch.isnan(out).sum()), int(torch.isnan(ref).sum()))
    if not torch.equal(torch.isinf(out), torch.isinf(ref)) or not torch.equal(out[torch.isinf(ref)], ref[torch.isinf(ref)]):
        return "isinf: %d of the oracle's %d" % (int(torch.isinf(out).sum()), int(torch.isinf(ref).sum()))
    fin = torch.isfinite(ref)
    err = (out[fin] - ref[fin]).abs().max().item() if fin.any() else 0.0
    return None if err <= bound else "error %.3e > %.3e" % (err, bound)


def _device_map(dev, nps, nm):
    """the motion map through the split entry points, which must be what the one call gives, bit for bit"""
    S = dev.shape[-1]
    total = FS.motion_map_sum(dev, nps)
    out = FS.finish_motion_map(total, S, nm)
    whole = FS.compute_mean_motion_map(dev, normalize_per_sample=nps, normalize=nm)
    assert _same_bits(out, whole), "motion_map_sum + finish_motion_map != compute_mean_motion_map"
    return out.cpu()


def _assert_form(dev, form):
    B, C, H, W, S = dev.shape
    got = NC.motion_form(dev.stride(), B, C, H, W, S, dev.data_ptr())
    assert got == form, "the case is meant for the %s form and takes %s" % (form, got)


@pytest.mark.parametrize("shape", list(NC.MOTION_SHAPES))
def test_motion_map_non_finite_samples(shape):
    """Every placement of NC.motion_poisons x both channel counts x the four option pairs, in the form the shape is meant for (asserted): the NaN and Inf patterns are the
    oracle's, the rest is within the bound of test_motion_map_kernel_forms_match_oracle, batch row 1 is bit-identical to the device result for the unpoisoned input (the
    range replicas and atomics are indexed by b), and a packed case agrees with the sample-major view of the same samples (the strided kernels)."""
    form, layout, S, H, W = NC.MOTION_SHAPES[shape]
    HW = H * W
    bad = []
    for C in NC.CHANNELS:
        clean = NC.clean_flows(C, H, W, S, 1000 + S + C)
        clean_dev = NC.as_layout(clean, layout).cuda()
        _assert_form(clean_dev, form)
        clean_out = {pair: _device_map(clean_dev, *pair) for pair in NC.OPTION_PAIRS}
        for name, placement in NC.motion_poisons(C, HW, S).items():
            fl = NC.poisoned(clean, placement)
            dev = NC.as_layout(fl, layout).cuda()
            _assert_form(dev, form)
            view = NC.as_layout(fl, "view").cuda() if layout == "packed" else None
            if view is not None:
                _assert_form(view, "STRIDED")
            for nps, nm in NC.OPTION_PAIRS:
                ref = FO.compute_mean_motion_map(fl, nps, nm)
                bound = NC.motion_bound(S, ref)
                out = _device_map(dev, nps, nm)
                why = _miss(out, ref, bound)
                if why is None and not _same_bits(out[1], clean_out[(nps, nm)][1]):
                    why = "batch row 1 differs from the unpoisoned run"
                if why is None and view is not None:
                    why = _miss(_device_map(view, nps, nm), out, bound)
                    why = why and "sample-major view against packed: " + why
                if why:
                    bad.append((C, name, "nps=%d nm=%d" % (nps, nm), why))
    assert not bad, "%d cases miss:\n%s" % (len(bad), "\n".join(map(str, bad)))


@pytest.mark.parametrize("shape", list(NC.MOTION_SHAPES))
def test_motion_map_flat_samples(shape):
    """Finite input whose ranges are below eps (NC.flat_flows): a sample of zeros and a sample of range 0.00125 among ordinary ones, and every sample flat so that the map's
    own range is below eps in the finish kernel -- the clamp's other branch in every form."""
    form, layout, S, H, W = NC.MOTION_SHAPES[shape]
    bad = []
    for C in NC.CHANNELS:
        for kind in NC.FLAT_KINDS:
            fl = NC.flat_flows(kind, C, H, W, S, (2000 if kind == "flat samples" else 3000) + S + C)
            dev = NC.as_layout(fl, layout).cuda()
            _assert_form(dev, form)
            view = NC.as_layout(fl, "view").cuda() if layout == "packed" else None
            for nps, nm in NC.OPTION_PAIRS:
                ref = FO.compute_mean_motion_map(fl, nps, nm)
                assert torch.isfinite(ref).all()
                bound = NC.motion_bound(S, ref)
                out = _device_map(dev, nps, nm)
                why = _miss(out, ref, bound)
                if why is None and view is not None:
                    why = _miss(_device_map(view, nps, nm), out, bound)
                    why = why and "sample-major view against packed: " + why
                if why:
                    bad.append((C, kind, "nps=%d nm=%d" % (nps, nm), why))
    assert not bad, "%d cases miss:\n%s" % (len(bad), "\n".join(map(str, bad)))


@pytest.mark.parametrize("shape", list(NC.FINISH_SHAPES))
def test_finish_kernel_paths(shape):
    """flow_map_finish_kernel alone: the register path (a multiple of 4 pixels, at most 65536) and the loop path (63 pixels; 66048 pixels), as the 4-D form of
    compute_mean_motion_map and through finish_motion_map with the normalisation on and off; the second map of the batch is clean and must not change by a bit."""
    H, W = NC.FINISH_SHAPES[shape]
    maps = NC.finish_maps(H, W, 40 + H * W)
    quarter = torch.tensor(0.25)
    clean_dev = maps["clean"].cuda()
    clean_out = {"4d": FS.compute_mean_motion_map(clean_dev).cpu(), True: FS.finish_motion_map(clean_dev, 4, True).cpu(),
                 False: FS.finish_motion_map(clean_dev, 4, False).cpu()}
    bad = []
    for name, m in maps.items():
        dev = m.cuda()
        runs = {"4d": (FS.compute_mean_motion_map(dev).cpu(), FO.compute_mean_motion_map(m)),
                True: (FS.finish_motion_map(dev, 4, True).cpu(), FO.compute_mean_motion_map(m * quarter)),   # (x 1/4: exact, as the kernel's scale)
                False: (FS.finish_motion_map(dev, 4, False).cpu(), m * quarter)}
        assert _same_bits(dev.cpu(), m), "finish_motion_map works on a copy"
        for how, (out, ref) in runs.items():
            why = _miss(out, ref, NC.motion_bound(1, ref))
            if why is None and not _same_bits(out[1], clean_out[how][1]):
                why = "map 1 differs from the unpoisoned run"
            if why:
                bad.append((name, "normalize=%s" % how, why))
    assert not bad, "%d cases miss:\n%s" % (len(bad), "\n".join(map(str, bad)))


@pytest.mark.parametrize("shape", list(NC.COV_SHAPES))
def test_features_and_covariance_non_finite(shape):
    """A non-finite flow value through flow_features (16-byte and scalar form) and the three load modes of flow_cov_kernel, whole matrix (symmetric grid, mirrored writes)
    and row slabs: the poisoned position's row and column are exactly 0 (NaN -> 0, segmentation.py:541), nothing else moves by a bit, and nothing is non-finite."""
    H, W, ds, S, mode = NC.COV_SHAPES[shape]
    P = (H // ds) * (W // ds)
    assert NC.cov_mode(P, S) == mode
    clean = NC.clean_flows(2, H, W, S, 500 + S + ds)
    clean_dev = clean.cuda()
    x_clean = FS.flow_features(clean_dev, ds)
    clean_full = {uc: FS.feature_cov_rows(x_clean, 0, P, uc) for uc in (True, False)}
    bad = []
    for name, (placement, positions) in NC.cov_poisons(H, W, ds, S).items():
        fl = NC.cov_poisoned(clean, placement)
        dev, view = fl.cuda(), NC.as_layout(fl, "view").cuda()
        assert NC.features_form(dev.stride(), *dev.shape, dev.data_ptr()) == ("VEC4" if S % 4 == 0 else "SCALAR")
        assert NC.features_form(view.stride(), *view.shape, view.data_ptr()) == "SCALAR"
        x_ref = FO.flow_features(fl, ds)
        x = FS.flow_features(dev, ds)
        for what, got in (("features", x), ("features of the sample-major view", FS.flow_features(view, ds))):
            why = _miss(got.cpu(), x_ref, 1e-6)
            if why:
                bad.append((name, what, why))
        poisoned = torch.zeros(P, dtype=torch.bool)
        poisoned[positions] = True
        keep = (~poisoned[:, None] & ~poisoned[None, :]).cuda()
        for uc in (True, False):
            key = (name, "cov" if uc else "corr")
            full = FS.feature_cov_rows(x, 0, P, uc)
            ref = FO.compute_flow_corrs(fl, ds, uc).reshape(NC.BATCH, P, P)
            if not torch.isfinite(full).all():
                bad.append(key + ("a non-finite output",))
            if full[0][poisoned.cuda()].any() or full[0][:, poisoned.cuda()].any():
                bad.append(key + ("the poisoned row / column is not 0",))
            if not _same_bits(full[0][keep], clean_full[uc][0][keep]) or not _same_bits(full[1], clean_full[uc][1]):
                bad.append(key + ("an entry outside the poisoned row / column differs from the unpoisoned run",))
            err = (full.cpu() - ref).abs().max().item()
            if not err <= TOL * max(1.0, ref.abs().max().item()):
                bad.append(key + ("error %.3e against the oracle" % err,))
            for row0, nrows in NC.cov_slabs(P):
                if not _same_bits(FS.feature_cov_rows(x, row0, nrows, uc), full[:, row0:row0 + nrows]):
                    bad.append(key + ("slab (%d, %d) differs from the whole matrix" % (row0, nrows),))
            whole = FS.compute_flow_corrs(dev, downsample=ds, use_covariance=uc)
            if not _same_bits(whole.reshape(NC.BATCH, P, P), full):
                bad.append(key + ("compute_flow_corrs differs from flow_features + feature_cov_rows",))
    assert not bad, "%d cases miss:\n%s" % (len(bad), "\n".join(map(str, bad)))
