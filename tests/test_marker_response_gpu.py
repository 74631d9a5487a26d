"""Marker counterfactuals through the predictor on a real MI355X: `predict_marker_responses` on its fused path (tokens -> `cwm_token_response`, no predicted
video) against its composed path (`predict` -> squared difference -> statistics in torch) and against the float64 restatement
(tests/response_restatement.py) on the tokens the predictor returns, and `predict_perturbation_flow` on top of it.

Both paths are run with the SAME chunking, so the predictor sees the same GEMM shapes and returns the same tokens; what is compared is then the read-out
alone, and its bounds are the restatement's (operation counts, sums of non-negative terms).  Peak indices are equal: in every row the largest response leads
the second by more than twice the pixel bound (asserted, no row left out).

Measured on an MI355X (run with -s), relative to the value, either path: maps 1.2e-7 (bound 3.0e-7), mass 7.6e-8 (6.1e-5 at 32 x 32, 3.0e-3 at
224 x 224), centroid 2.1e-7 (1.8e-4 / 9.1e-3); the largest response leads the second by at least 2.8e-3 of its value in every row (needed: 6.0e-7)."""
import numpy as np
import pytest
import torch

import response_restatement as RR
from counterfactualworldmodels_amd import perturbation, prediction, segmentation, synthetic as S
from test_patch_error_gpu import BASE8, TINY, generator, no_video

pytestmark = pytest.mark.gpu
SEED = 3
ALL16 = [[i, j] for i in range(4) for j in range(4)]


def composed_like(G):
    c = prediction.PredictorBasedGenerator(predictor=G.predictor, imagenet_normalize_inputs=True, temporal_dim=2)
    c._responses_take_fused_path = lambda *a, **k: False
    return c


def fused_like(G):
    return no_video(prediction.PredictorBasedGenerator(predictor=G.predictor, imagenet_normalize_inputs=True, temporal_dim=2))


def exact_responses(G, x, patches_thw, mask, frame, chunk):
    """float64 responses [K,H,W] from the tokens the predictor returns for the marked rows, predicted in chunks of `chunk`, and for the clean row"""
    _, T, Cc, H, W = x.shape
    P = G.patch_size[-1]
    K = len(patches_thw)
    markers = perturbation.AddMarkers(P).sample_markers(K, x)
    where = torch.tensor(patches_thw, device=x.device)
    rows = x.expand(K, -1, -1, -1, -1).clone()
    perturbation.paint_markers(rows, markers, torch.arange(K, device=x.device), where[:, 0], where[:, 1], where[:, 2], (P, P))
    clean = G.predictor.predict_video(x, mask, normalize=True)[0]
    out = []
    for r0 in range(0, K, chunk):
        xs = rows[r0:r0 + chunk]
        y = G.predictor.predict_video(xs, mask.expand(len(xs), -1), normalize=True)[0]
        out.append(RR.response(y.cpu(), clean.cpu(), mask.expand(len(xs), -1).cpu(), T, Cc, H, W, P, frame % T))
    return torch.cat(out)


def within(name, got, want, rel):
    got, want = torch.as_tensor(got).double().cpu(), want.double().cpu()
    err = (got - want).abs()
    print("%-40s max error %.3e of values up to %.3e (relative bound %.3e)" % (name, err.max().item(), want.abs().max().item(), rel))
    assert bool((err <= rel * want.abs()).all()), (name, (err - rel * want.abs()).max().item())


def paths_against_restatement(G, x, patches, mask, chunk, label):
    _, T, Cc, H, W = x.shape
    thw = [[0] + list(p) for p in patches]
    m = G.get_zeros_mask(x, frame=-1) if mask is None else mask
    r = exact_responses(G, x, thw, m.reshape(1, -1).contiguous(), -1, chunk or len(patches))
    gap, top = RR.index_gap(r)
    print("%s: relative lead of the largest response over the second >= %.3e (needed %.3e)" % (label, float((gap / top).min()), 2 * RR.pixel_bound(Cc)))
    assert bool((gap > 2 * RR.pixel_bound(Cc) * top).all())
    want_idx, want = RR.statistics(r)
    results = {}
    for name, gen in (("fused", fused_like(G)), ("composed", composed_like(G))):
        res = gen.predict_marker_responses(x, patches, mask=mask, sample_batch_size=chunk, return_maps=True)
        assert res.peak_yx.shape == (len(patches), 2) and res.peak_yx.dtype == np.int64 and res.centroid.shape == (len(patches), 2)
        assert res.maps.shape == (len(patches), H, W) and res.maps.is_cuda
        assert (res.peak_yx[:, 0] * W + res.peak_yx[:, 1]).tolist() == want_idx.tolist(), (label, name)
        within("%s %s maps" % (label, name), res.maps, r, RR.pixel_bound(Cc))
        within("%s %s peak" % (label, name), res.peak, want[:, 0], RR.pixel_bound(Cc))
        within("%s %s mass" % (label, name), res.mass, want[:, 1], RR.mass_bound(Cc, H, W))
        within("%s %s centroid" % (label, name), res.centroid, want[:, 2:], RR.centroid_bound(Cc, H, W))
        without = gen.predict_marker_responses(x, patches, mask=mask, sample_batch_size=chunk)
        assert without.maps is None and np.array_equal(without.peak_yx, res.peak_yx) and np.array_equal(without.mass, res.mass)
        results[name] = res
    return results


@pytest.fixture(scope="module")
def tiny():
    G = generator(TINY, SEED)
    x = torch.from_numpy(S.synthetic_frames(1, TINY, SEED)).cuda()
    return G, x


@pytest.mark.parametrize("chunk", [None, 3])
def test_fused_path_equals_composed_path_without_a_video(tiny, chunk):
    G, x = tiny
    rng = torch.get_rng_state()
    paths_against_restatement(G, x, ALL16, None, chunk, "tiny chunks of %s" % chunk)
    assert torch.equal(rng, torch.get_rng_state())  # nothing is drawn


def test_a_mask_with_visible_patches_in_the_predicted_frame(tiny):
    G, x = tiny
    mask = G.get_zeros_mask(x, frame=-1).clone()
    mask[0, [16 + 5, 16 + 6, 16 + 15]] = False  # three patches of frame 1 are given
    mask[0, [3, 12]] = True                      # two of frame 0 are hidden -- not marked ones
    patches = [p for p in ALL16 if p not in ([0, 3], [3, 0])]
    res = paths_against_restatement(G, x, patches, mask, 5, "tiny, mixed mask")["fused"]
    given = torch.zeros((4, 4), dtype=torch.bool)
    given.view(-1)[[5, 6, 15]] = True
    up = given.repeat_interleave(8, 0).repeat_interleave(8, 1).cuda()
    assert bool((res.maps[:, up] == 0).all()) and bool((res.maps[:, ~up] > 0).any())


def test_chunk_sizes_give_the_same_indices(tiny):
    G, x = tiny
    F = fused_like(G)
    runs = [F.predict_marker_responses(x, ALL16, sample_batch_size=c) for c in (1, 3, 16, None)]
    for r in runs[1:]:
        assert np.array_equal(r.peak_yx, runs[0].peak_yx)
    assert np.array_equal(runs[2].peak, runs[3].peak) and np.array_equal(runs[2].centroid, runs[3].centroid)  # K rows and "all rows" are one chunk
    again = F.predict_marker_responses(x, ALL16, sample_batch_size=3)
    assert np.array_equal(again.peak, runs[1].peak) and np.array_equal(again.mass, runs[1].mass) and np.array_equal(again.centroid, runs[1].centroid)


def test_markers_of_another_kind_and_patch_entries(tiny):
    G, x = tiny
    F = fused_like(G)
    a = F.predict_marker_responses(x, [[1, 2], [3, 3]])
    b = F.predict_marker_responses(x, [[0, 1, 2], torch.tensor([0, 0, 3, 3])], marker=perturbation.AddMarkers(8))
    assert np.array_equal(a.peak_yx, b.peak_yx) and np.array_equal(a.peak, b.peak)
    cross = perturbation.AddMarkers(8, marker_shapes=["cross"], marker_color=[0, 0, 1])
    c = F.predict_marker_responses(x, [[1, 2], [3, 3]], marker=cross)
    assert not np.array_equal(a.peak, c.peak)
    black = F.predict_marker_responses(x, [[1, 2]], marker=perturbation.AddMarkers(8, marker_color=[0, 0, 0]))  # paints nothing: the clean row again
    assert black.peak.tolist() == [0.0] and black.mass.tolist() == [0.0] and black.peak_yx.tolist() == [[0, 0]] and black.centroid.tolist() == [[0.0, 0.0]]


def test_refusals(tiny):
    G, x = tiny
    mask = G.get_zeros_mask(x, frame=-1).clone()
    mask[0, 5] = True
    with pytest.raises(ValueError, match="visible"):
        G.predict_marker_responses(x, [[0, 0], [1, 1]], mask=mask)  # patch (1, 1) of frame 0 is token 5
    with pytest.raises(ValueError, match="another frame"):
        G.predict_marker_responses(x, [[1, 0, 0]])  # a marker in the frame the response is read in
    with pytest.raises(ValueError, match="ONE movie"):
        G.predict_marker_responses(x.expand(2, -1, -1, -1, -1), [[0, 0]])
    with pytest.raises(ValueError, match="grid"):
        G.predict_marker_responses(x, [[0, 4]])
    with pytest.raises(ValueError, match="marker's patches"):
        G.predict_marker_responses(x, [[0, 0]], marker=perturbation.AddMarkers(4))
    with pytest.raises(ValueError):
        G.predict_marker_responses(x, [[0, 0]], frame=None)


def test_ragged_generator_runs_fused_and_conjoined_predictor_composed():
    R = no_video(generator(TINY, SEED, ragged_batches=True))  # all rows share the clean row's mask: there is nothing ragged about them
    x = torch.from_numpy(S.synthetic_frames(1, TINY, SEED)).cuda()
    a = R.predict_marker_responses(x, ALL16[:6], sample_batch_size=4)
    b = no_video(generator(TINY, SEED)).predict_marker_responses(x, ALL16[:6], sample_batch_size=4)
    assert np.array_equal(a.peak_yx, b.peak_yx) and np.array_equal(a.peak, b.peak) and np.array_equal(a.centroid, b.centroid)

    import os

    from counterfactualworldmodels_amd import conjoined_vmae as CV
    from test_conj_oracle import TINY_CONJ, conj_weights

    c = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conj_tiny.npz"))
    m = CV.ConjoinedPaddedVisionTransformer(TINY_CONJ)
    m.load_state_dict(conj_weights(TINY_CONJ, int(c["seed"])))
    Gc = prediction.PredictorBasedGenerator(predictor=m.cuda().eval(), imagenet_normalize_inputs=True, temporal_dim=2)
    xc, imu, mask = torch.from_numpy(c["x"]).cuda()[:1], torch.from_numpy(c["imu"]).cuda()[:1], torch.from_numpy(c["mask_eq"]).cuda()[:1]
    mc = torch.zeros(1, TINY_CONJ.ctx_tokens, dtype=torch.bool, device="cuda")
    assert not Gc._responses_take_fused_path(xc, dict(x_context=imu, mask_context=mc)) and not Gc._responses_take_fused_path(xc, {})
    P = Gc.patch_size[-1]
    hh, ww = xc.shape[-2] // P, xc.shape[-1] // P
    vis = (~mask[0, :hh * ww]).nonzero()[:, 0].tolist()[:2]
    patches = [[v // ww, v % ww] for v in vis]
    assert len(patches) == 2
    res = Gc.predict_marker_responses(xc, patches, mask=mask, x_context=imu, mask_context=mc, return_maps=True)
    rows = xc.expand(2, -1, -1, -1, -1).clone()
    where = torch.tensor(patches, device="cuda")
    perturbation.paint_markers(rows, perturbation.AddMarkers(P).sample_markers(2, xc), torch.arange(2, device="cuda"), torch.zeros(2, dtype=torch.long, device="cuda"),
                               where[:, 0], where[:, 1], (P, P))
    video = Gc.predict(rows, mask.expand(2, -1).clone(), x_context=imu.expand(2, *imu.shape[1:]), mask_context=mc.expand(2, -1))
    clean = Gc.predict(xc, mask.clone(), x_context=imu, mask_context=mc)
    r = ((video - clean) ** 2).sum(2)[:, 0]
    assert torch.equal(res.maps, r) and bool((r > 0).any())
    idx, stats = RR.statistics(r.double().cpu())
    assert (res.peak_yx[:, 0] * r.shape[-1] + res.peak_yx[:, 1]).tolist() == idx.tolist() and np.array_equal(res.peak, stats[:, 0].float().numpy())


def test_perturbation_flow(tiny):
    G, x = tiny
    F = segmentation.FlowGenerator(predictor=G.predictor, imagenet_normalize_inputs=True, temporal_dim=2)
    no_video(F)
    res = F.predict_marker_responses(x, ALL16)
    flow = F.predict_perturbation_flow(x, points=ALL16)
    assert flow.shape == (16, 2) and flow.is_cuda and flow.dtype == torch.float32
    centre = np.array(ALL16) * 8 + 3.5
    assert np.array_equal(flow.cpu().numpy(), np.stack([res.peak_yx[:, 1] - centre[:, 1], res.peak_yx[:, 0] - centre[:, 0]], 1).astype(np.float32))
    soft = F.predict_perturbation_flow(x, points=torch.tensor(ALL16), use_centroid=True, sample_batch_size=16)
    assert np.array_equal(soft.cpu().numpy(), np.stack([res.centroid[:, 1] - centre[:, 1], res.centroid[:, 0] - centre[:, 0]], 1).astype(np.float32))
    field, valid = F.predict_perturbation_flow(x, grid_stride=2)
    assert field.shape == (2, 2, 2) and valid.shape == (2, 2) and valid.dtype == torch.bool and bool(valid.all())
    sub = flow.view(4, 4, 2)[::2, ::2].permute(2, 0, 1)
    assert torch.equal(field, sub)  # the same prompts, four of them: chunks of 4 rows against chunks of 16 -- equal only where the peaks are (they are)
    median = float(np.median(res.mass))
    _, strict = F.predict_perturbation_flow(x, grid_stride=1, min_mass=median)
    assert strict.shape == (4, 4) and strict.view(-1).tolist() == (res.mass > median).tolist() and 0 < int(strict.sum()) < 16
    with pytest.raises(ValueError):
        F.predict_perturbation_flow(x)
    with pytest.raises(ValueError):
        F.predict_perturbation_flow(x, points=ALL16, grid_stride=2)


def test_full_geometry_fused_equals_composed():
    """ViT-B/8 at 224 x 224: 28 x 28 patches per frame, 28 workgroups of 448 items per row, K = 4 markers in one chunk"""
    G = generator(BASE8, 0)
    x = torch.from_numpy(S.synthetic_frames(1, BASE8, 0)).cuda()
    paths_against_restatement(G, x, [[0, 0], [13, 14], [27, 27], [5, 20]], None, None, "base8")
