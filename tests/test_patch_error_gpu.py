"""Patch-error maps straight from the predicted tokens on a real MI355X: the kernel (`cwm_patch_error`) against the float64 restatement
(tests/patch_error_restatement.py), the wrapper's fused path against the reference's results (tests/golden/patch_error.npz) and against its own composed
path, and the error-guided search `greedy_unmask`.

Bounds.  Kernel against restatement: the rounding of ANY fp32 evaluation, (C P^2 + 2) 2^-24 of each patch value, plus (T h w + 2) 2^-24 for the mean
(patch_error_restatement.map_bound / mean_bound).  Wrapper against the reference: a predicted pixel is within tau = 1e-3 of the reference's (the project's
parity bound on tokens), so (p + e - t)^2 - (p - t)^2 = 2 (p - t) e + e^2 is at most 2 dmax tau + tau^2 per pixel and channel, with dmax the largest
|prediction - target| of the case (stored in the golden); the patch average of the channel sums is then within C (2 dmax tau + tau^2), and so is any
mean of patch values with non-negative weights.

Measured on an MI355X (run with -s): kernel against restatement at most 1.2e-6 on values up to 6.7 (bound 1.2e-5 relative); fused path against
the reference 1.2e-5 (map) / 1.7e-6 (mean) against bounds of 6.0e-3 - 2.2e-2; greedy scores 2.9e-6 from the reference's against bounds of 5.3e-2 - 6.5e-2."""
import ctypes
import os

import numpy as np
import pytest
import torch
from torch import nn

import patch_error_restatement as PR
from counterfactualworldmodels_amd import _lib, config as C, prediction, synthetic as S, vmae

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
BASE8 = C.CONFIGS["base_8x8patch_2frames_1tube"]
TAU = 1e-3  # tests/test_model_gpu.py: parity-mode tokens against the reference


def stream():
    return _lib.current_stream_handle(torch.device("cuda:0"))


def run_kernel(y, x, mask, P, frame, target=None, region=None, want_map=True, want_mean=True):
    """`cwm_patch_error` on device tensors; x / target are [B,T,C,H,W]-shaped views of any (b, t, c) strides.  Returns (map, mean), None where not asked for."""
    B, T, Cc, H, W = x.shape
    h, w = H // P, W // P
    emap = torch.full((B, T, h, w), float("nan"), device="cuda") if want_map else None
    mean = torch.full((B,), float("nan"), device="cuda") if want_mean else None
    scratch = torch.empty((B, T, h, w), device="cuda") if want_mean and not want_map else None
    a = _lib.fill_patch_args(_lib.new_patch_error_args(), x=x, target=target, mask=mask, region=region, y=y, geometry=(B, T, Cc, H, W, P),
                             n_vis=T * h * w - (0 if y is None else y.shape[1]), frame=-1 if frame is None else frame, map=emap, mean=mean, scratch=scratch, stream=stream())
    _lib.check(_lib.get_lib().cwm_patch_error(ctypes.byref(a)))
    return emap, mean


def inputs(B, T, Cc, H, W, P, n_masked, seed, layout="btchw"):
    """frames (a [B,T,C,H,W]-shaped view: contiguous, of a [B,C,T,H,W] tensor, one movie shared at batch stride 0, or off the 16-byte grid), masks with
    `n_masked` masked tokens per row in both frames, tokens, and another movie as target"""
    g = torch.Generator().manual_seed(seed)
    if layout == "bcthw":
        x = torch.rand((B, Cc, T, H, W), generator=g).cuda().permute(0, 2, 1, 3, 4)
    elif layout == "stride0":
        x = torch.rand((1, T, Cc, H, W), generator=g).cuda().expand(B, -1, -1, -1, -1)
    elif layout == "offset":
        x = torch.rand((B * T * Cc * H * W + 1,), generator=g).cuda()[1:].view(B, T, Cc, H, W)
    else:
        x = torch.rand((B, T, Cc, H, W), generator=g).cuda()
    Nt = T * (H // P) * (W // P)
    mask = torch.zeros((B, Nt), dtype=torch.bool)
    for b in range(B):
        mask[b, torch.randperm(Nt, generator=g)[:n_masked]] = True
    y = torch.randn((B, n_masked, P * P * Cc), generator=g).cuda() if n_masked else None
    target = torch.rand((B, T, Cc, H, W), generator=g).cuda()
    return x, mask.cuda(), y, target


def within(name, got, want, rel):
    got, want = got.double().cpu(), want.double().cpu()
    err = (got - want).abs()
    print("%-28s max error %.3e of values up to %.3e (relative bound %.3e)" % (name, err.max().item(), want.abs().max().item(), rel))
    assert bool((err <= rel * want.abs()).all()), (name, (err - rel * want.abs()).max().item())


# (B, T, C, H, W, P, masked tokens per row, layout): a 4 x 6 grid that is not square; the three patch sizes; the generic kernel (C != 3, frames off the 16-byte
# grid); strided and shared frames; 8 * 136 / 4 = 272 items for the 256 lanes of a workgroup: a second, partly filled pass; 3 * 2 * 5 = 30 workgroups
GEOMETRIES = {
    "grid4x6": (3, 2, 3, 32, 48, 8, 17, "btchw"),
    "p4": (2, 2, 3, 16, 16, 4, 13, "btchw"),
    "p16": (2, 2, 3, 32, 32, 16, 3, "btchw"),
    "bcthw": (3, 2, 3, 32, 48, 8, 17, "bcthw"),
    "stride0": (3, 2, 3, 32, 48, 8, 17, "stride0"),
    "two_channels": (2, 2, 2, 16, 32, 8, 5, "btchw"),
    "offset": (2, 2, 3, 32, 48, 8, 17, "offset"),
    "second_pass": (3, 2, 3, 40, 136, 8, 61, "btchw"),
    "three_frames": (2, 3, 3, 16, 16, 8, 5, "btchw"),
}


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_kernel_equals_the_restatement(name):
    B, T, Cc, H, W, P, nm, layout = GEOMETRIES[name]
    x, mask, y, target = inputs(B, T, Cc, H, W, P, nm, 100 + len(name), layout)
    h, w = H // P, W // P
    mb, nb = PR.map_bound(Cc, P), PR.mean_bound(Cc, P, T * h * w)
    g = torch.Generator().manual_seed(7)
    weights = torch.randint(0, 9, (B, T, h, w), generator=g).float() / 4  # float weights in [0, 2]
    weights[B - 1] = 0  # one row whose region is empty: mean 0 through the clamp
    for frame in (0, T - 1, None):
        for tgt in (None, target):
            for region in (None, weights.cuda()):
                emap, mean = run_kernel(y, x, mask, P, frame, tgt, region)
                want = PR.error_map(y.cpu(), x.cpu(), mask.cpu(), P, None if tgt is None else tgt.cpu(), frame)
                tag = "%s frame %s%s%s" % (name, frame, " target" if tgt is not None else "", " region" if region is not None else "")
                within(tag + " map", emap, want, mb)
                within(tag + " mean", mean, PR.error_mean(want, None if region is None else region.cpu()), nb)
                if region is not None:
                    assert mean[B - 1].item() == 0.0
                if tgt is None and frame is None:  # a visible patch compared with itself
                    vis = ~mask.view(B, T, h, w)
                    assert bool((emap[vis] == 0).all()) and bool((emap[~vis] > 0).all())


def test_each_output_alone_and_two_calls_are_bit_equal():
    B, T, Cc, H, W, P, nm, _ = GEOMETRIES["grid4x6"]
    x, mask, y, target = inputs(B, T, Cc, H, W, P, nm, 5)
    region = (torch.arange(B * T * 4 * 6).view(B, T, 4, 6) % 5).float().cuda() / 2
    both = run_kernel(y, x, mask, P, 1, target, region)
    again = run_kernel(y, x, mask, P, 1, target, region)
    assert torch.equal(both[0], again[0]) and torch.equal(both[1], again[1]) and not both[0].isnan().any() and not both[1].isnan().any()
    only_map = run_kernel(y, x, mask, P, 1, target, region, want_mean=False)
    only_mean = run_kernel(y, x, mask, P, 1, target, region, want_map=False)
    assert only_map[1] is None and only_mean[0] is None
    assert torch.equal(only_map[0], both[0]) and torch.equal(only_mean[1], both[1])
    # arguments that cannot be run are refused, naming what is wrong
    a = _lib.fill_patch_args(_lib.new_patch_error_args(), x=x, mask=mask, geometry=(B, T, Cc, H, W, P), n_vis=T * 24, frame=0, stream=None)
    lib = _lib.get_lib()
    assert lib.cwm_patch_error(ctypes.byref(a)) == _lib.ERR_INVALID and b"neither output" in lib.cwm_last_error()
    a.mean_dev = both[1].data_ptr()
    assert lib.cwm_patch_error(ctypes.byref(a)) == _lib.ERR_INVALID and b"scratch" in lib.cwm_last_error()
    a.map_dev, a.P = both[0].data_ptr(), 12
    assert lib.cwm_patch_error(ctypes.byref(a)) == _lib.ERR_INVALID and b"P = 12" in lib.cwm_last_error()


def test_nothing_masked():
    """n_vis = Nt: there are no predicted tokens; the prediction is the input, so its error against itself is 0 and against another target it is not"""
    B, T, Cc, H, W, P, _, _ = GEOMETRIES["grid4x6"]
    x, mask, y, target = inputs(B, T, Cc, H, W, P, 0, 9)
    assert y is None and not mask.any()
    emap, mean = run_kernel(None, x, mask, P, None)
    assert bool((emap == 0).all()) and bool((mean == 0).all())
    emap, mean = run_kernel(None, x, mask, P, 1)  # frame 1 against frames 0 and 1
    assert bool((emap[:, 1] == 0).all()) and bool((emap[:, 0] > 0).all())
    emap, mean = run_kernel(None, x, mask, P, None, target)
    want = PR.error_map(None, x.cpu(), mask.cpu(), P, target.cpu(), None)
    within("nothing masked, target map", emap, want, PR.map_bound(Cc, P))
    within("nothing masked, target mean", mean, PR.error_mean(want), PR.mean_bound(Cc, P, T * 24))


# ---- the wrapper ------------------------------------------------------------------------------------------------------------------------------------
def build(cfg, seed, mode="parity"):
    m = vmae.PretrainVisionTransformer(cfg, mode=mode)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, seed).items()})
    return m.to("cuda:0").eval()


def generator(cfg, weights_seed, **kw):
    return prediction.PredictorBasedGenerator(predictor=build(cfg, weights_seed), imagenet_normalize_inputs=True, temporal_dim=2, **kw)


def no_video(G):
    """make `predict` (the composed path) an error: what runs afterwards is the fused path"""
    def refuse(*a, **k):
        raise AssertionError("the composed path ran")
    G.predict = refuse
    return G


@pytest.fixture(scope="module")
def tiny():
    g = np.load(os.path.join(GOLDEN, "patch_error.npz"))
    G = generator(TINY, int(g["seed"]))
    x = torch.from_numpy(S.synthetic_frames(3, TINY, int(g["seed"]))).cuda()
    return G, g, x, torch.from_numpy(g["mask"]).cuda(), torch.from_numpy(g["target_mask"]).cuda(), torch.from_numpy(g["target_x"]).cuda()


CASES = {"default": {}, "frame0": dict(frame=0), "each": dict(frame=None), "target": dict(target=True)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_path_equals_the_reference(tiny, name):
    G, g, x, mask, target_mask, target = tiny
    kw = dict(CASES[name])
    if kw.pop("target", False):
        kw["target"] = target
    bound = 3 * (2 * float(g["dmax_" + name]) * TAU + TAU * TAU)
    fused = no_video(generator(TINY, int(g["seed"])))
    rng = torch.get_rng_state()
    emap = fused.get_error_on_target_region(x, mask.clone(), target_mask, average_error=False, **kw)
    mean = fused.get_error_on_target_region(x, mask.clone(), target_mask, **kw)
    assert torch.equal(rng, torch.get_rng_state())  # rows of equal counts: nothing is drawn
    want_map, want_mean = g["map" if name == "default" else name + "_map"], g[name]
    assert emap.shape == want_map.shape == (3, 2, 4, 4) and mean.shape == want_mean.shape == (3,)
    e_map, e_mean = np.abs(emap.cpu().numpy() - want_map).max(), np.abs(mean.cpu().numpy() - want_mean).max()
    print("%s: fused path against the reference: map %.3e, mean %.3e (bound %.3e, dmax %.3f)" % (name, e_map, e_mean, bound, float(g["dmax_" + name])))
    assert e_map <= bound and e_mean <= bound
    # a target mask given as the [B,T,h,w] region complement, and float weights given as such
    m4 = fused.get_error_on_target_region(x, mask.clone(), target_mask.view(3, 2, 4, 4), **kw)
    assert torch.equal(m4, mean)
    half = fused.get_error_on_target_region(x, mask.clone(), 1 - 0.5 * (~target_mask).view(3, 2, 4, 4).float(), average_error=False, **kw)
    assert torch.equal(half, 0.5 * emap)


def test_composed_paths_equal_the_reference_and_torch(tiny):
    G, g, x, mask, target_mask, _ = tiny
    bound = 3 * (2 * float(g["dmax_default"]) * TAU + TAU * TAU)
    pixels = G.get_error_on_target_region(x, mask.clone(), target_mask, aggregate_over_patches=False)
    assert pixels.shape == g["pixels"].shape == (3, 2, 1, 32, 32) and np.abs(pixels.cpu().numpy() - g["pixels"]).max() <= bound
    G.set_input(x)
    ewm = G.error_with_mask(mask.clone())
    assert ewm.shape == g["error_with_mask"].shape == (3, 1, 1, 32, 32) and np.abs(ewm.cpu().numpy() - g["error_with_mask"]).max() <= bound
    assert torch.equal(G.predict_with_mask(mask.clone()), G.predict(x, mask.clone()))
    assert torch.equal(G.predict_with_mask(~mask, invert_mask=True, frame=None), G.predict(x, mask.clone(), frame=None))
    # another patch size pools the per-pixel error differently: composed
    coarse = G.get_error_on_target_region(x, mask.clone(), torch.zeros(3, 2, 2, 2, device="cuda"), average_error=False, patch_size=(1, 16, 16))
    assert torch.allclose(coarse, nn.functional.avg_pool3d(pixels.transpose(1, 2), (1, 16, 16)).squeeze(1), rtol=1e-6, atol=0)
    # a custom error function: composed, and what torch computes from the predicted video
    L1 = prediction.PredictorBasedGenerator(predictor=G.predictor, imagenet_normalize_inputs=True, temporal_dim=2, error_func=nn.L1Loss(reduction="none"))
    got = L1.get_error_on_target_region(x, mask.clone(), target_mask, frame=None)
    video = L1.predict(x, mask.clone(), frame=None)
    region = 1 - target_mask.view(3, 2, 4, 4).float()
    want = nn.functional.avg_pool3d((video - x).abs().sum(2, True).transpose(1, 2), (1, 8, 8), stride=(1, 8, 8)).squeeze(1)
    want = (want * region).sum((1, 2, 3)) / region.sum((1, 2, 3)).clamp(min=1)
    assert torch.equal(got, want)


def paths_against_restatement(G, x, mask, target_mask, label, **kw):
    """fused and composed path on the same inputs, each within the summation bound of the float64 restatement on the tokens the predictor returns"""
    Cc, P = x.shape[2], G.patch_size[-1]
    B, T, h, w = x.shape[0], x.shape[1], x.shape[-2] // P, x.shape[-1] // P
    y, video = G.predictor.predict_video(x, mask, normalize=True)
    exact = PR.error_map(y.cpu(), x.cpu(), mask.cpu(), P, frame=kw.get("frame", -1))
    region = 1 - target_mask.view(B, T, h, w).double().cpu()
    composed = generator_like(G)
    composed._error_takes_fused_path = lambda *a, **k: False
    fused = no_video(generator_like(G))
    for name, gen in (("fused", fused), ("composed", composed)):
        emap = gen.get_error_on_target_region(x, mask.clone(), target_mask, average_error=False, **kw)
        mean = gen.get_error_on_target_region(x, mask.clone(), target_mask, **kw)
        within("%s %s map" % (label, name), emap, exact * region, PR.map_bound(Cc, P))
        within("%s %s mean" % (label, name), mean, PR.error_mean(exact, region), PR.mean_bound(Cc, P, T * h * w))


def generator_like(G):
    return prediction.PredictorBasedGenerator(predictor=G.predictor, imagenet_normalize_inputs=True, temporal_dim=2)


@pytest.mark.parametrize("frame", [-1, None])
def test_fused_path_equals_composed_path(tiny, frame):
    G, g, x, mask, target_mask, _ = tiny
    paths_against_restatement(G, x, mask, target_mask, "tiny frame %s" % frame, frame=frame)


def test_full_geometry_fused_equals_composed():
    """ViT-B/8 at 224 x 224, B = 2: 28 x 28 patches per frame, 28 patch rows of 448 items per (b, t)"""
    G = generator(BASE8, 0)
    x = torch.from_numpy(S.synthetic_frames(2, BASE8, 0)).cuda()
    mask = torch.from_numpy(S.synthetic_masks(2, BASE8, 8, 0)).cuda()
    target_mask = torch.from_numpy(S.synthetic_masks(2, BASE8, 300, 1)).cuda()
    paths_against_restatement(G, x, mask, target_mask, "base8")


def test_ragged_generator_and_conjoined_predictor_take_the_composed_path():
    g = np.load(os.path.join(GOLDEN, "ragged_tiny.npz"))
    R = generator(TINY, int(g["seed"]), ragged_batches=True)
    x, mask = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["mask"]).cuda()
    assert len(set((~mask).sum(1).tolist())) >= 3
    tm = torch.zeros_like(mask)
    tm[:, :16] = True
    got = R.get_error_on_target_region(x, mask.clone(), tm, average_error=False)  # rows of different counts: the ragged predict
    video = R.predict(x, mask.clone())
    want = nn.functional.avg_pool3d(nn.MSELoss(reduction="none")(video, x).sum(2, True).transpose(1, 2), (1, 8, 8), stride=(1, 8, 8)).squeeze(1) * (1 - tm.view(4, 2, 4, 4).float())
    assert torch.equal(got, want)
    same = mask[:1].expand(2, -1).contiguous()  # rows that agree run fused, ragged generator or not
    a = no_video(generator(TINY, int(g["seed"]), ragged_batches=True)).get_error_on_target_region(x[:2], same.clone(), tm[:2])
    b = no_video(generator(TINY, int(g["seed"]))).get_error_on_target_region(x[:2], same.clone(), tm[:2])
    assert torch.equal(a, b)

    from counterfactualworldmodels_amd import conjoined_vmae as CV
    from test_conj_oracle import TINY_CONJ, conj_weights

    c = np.load(os.path.join(GOLDEN, "conj_tiny.npz"))
    m = CV.ConjoinedPaddedVisionTransformer(TINY_CONJ)
    m.load_state_dict(conj_weights(TINY_CONJ, int(c["seed"])))
    Gc = prediction.PredictorBasedGenerator(predictor=m.cuda().eval(), imagenet_normalize_inputs=True, temporal_dim=2)
    xc, imu, mask_eq = torch.from_numpy(c["x"]).cuda()[:2], torch.from_numpy(c["imu"]).cuda()[:2], torch.from_numpy(c["mask_eq"]).cuda()
    mc = torch.zeros(2, TINY_CONJ.ctx_tokens, dtype=torch.bool, device="cuda")
    ps = Gc._patch3()
    hh, ww = xc.shape[-2] // ps[-2], xc.shape[-1] // ps[-1]
    tmc = torch.zeros(2, 2 * hh * ww, dtype=torch.bool, device="cuda")
    tmc[:, :hh * ww] = True
    got = Gc.get_error_on_target_region(xc, mask_eq.clone(), tmc, x_context=imu, mask_context=mc)
    video = Gc.predict(xc, mask_eq.clone(), x_context=imu, mask_context=mc)
    want = nn.functional.avg_pool3d(nn.MSELoss(reduction="none")(video, xc).sum(2, True).transpose(1, 2), ps, stride=ps).squeeze(1) * (1 - tmc.view(2, 2, hh, ww).float())
    assert got.shape == (2,) and torch.equal(got, want.sum((1, 2, 3)) / (hh * ww))


# ---- greedy_unmask -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def greedy():
    g = np.load(os.path.join(GOLDEN, "patch_error.npz"))
    return g, torch.from_numpy(g["greedy_x"]).cuda(), torch.from_numpy(g["greedy_mask"]).cuda()


@pytest.mark.parametrize("sbs", [None, 4])
def test_greedy_unmask_equals_the_reference_search(greedy, sbs):
    g, x, mask = greedy
    G = no_video(generator(TINY, int(g["seed"])))
    rng = torch.get_rng_state()
    start = mask.clone()
    out, picks, scores, trace = G.greedy_unmask(x, mask, num_steps=4, sample_batch_size=sbs, return_scores=True)
    assert torch.equal(rng, torch.get_rng_state()) and torch.equal(mask, start)
    assert picks.tolist() == g["greedy_picks"].tolist() and np.array_equal(out.cpu().numpy(), g["greedy_final_mask"])
    err = np.abs(scores - g["greedy_scores"])
    print("greedy (chunks of %s): picks %s, scores against the reference %s (bounds %s)" % (sbs, picks.tolist(), err, g["greedy_bounds"]))
    assert (err <= g["greedy_bounds"]).all()
    # every step: the candidates are the still-masked tokens of frame 1, the scores are those of a direct call on the same rows in the same chunks, and the
    # pick is the first minimum
    D = no_video(generator(TINY, int(g["seed"])))
    region_mask = torch.ones_like(mask)
    region_mask[:, 16:] = False
    cur = start.clone()
    for step, (cand, s) in enumerate(trace):
        assert cand.tolist() == [t for t in range(16, 32) if bool(cur[0, t])]
        rows = cur.expand(len(cand), -1).clone()
        rows[torch.arange(len(cand)), torch.from_numpy(cand).cuda()] = False
        k = len(cand) if sbs is None else sbs
        direct = torch.cat([D.get_error_on_target_region(x.expand(len(r), -1, -1, -1, -1), r, region_mask.expand(len(r), -1)) for r in rows.split(k)])
        assert np.array_equal(direct.cpu().numpy(), s)
        assert picks[step] == cand[int(np.flatnonzero(s == s.min())[0])] and scores[step] == s.min()
        cur[0, picks[step]] = False
    assert torch.equal(cur, out)


def test_greedy_unmask_candidates_and_errors(greedy):
    g, x, mask = greedy
    draws = []
    for _ in range(2):
        G = generator(TINY, int(g["seed"]), seed=11)
        out, picks, scores, trace = G.greedy_unmask(x, mask, num_steps=2, num_candidates=5, return_scores=True)
        assert all(len(c) == 5 and (np.diff(c) > 0).all() for c, _ in trace) and picks[0] in trace[0][0] and picks[1] not in (picks[0],)
        draws.append([c.tolist() for c, _ in trace])
    assert draws[0] == draws[1]
    # given candidates: only they are tried, and a picked one is not tried again
    G = generator(TINY, int(g["seed"]))
    out, picks, scores, trace = G.greedy_unmask(x, mask, num_steps=2, candidates=[28, 19, 17], return_scores=True)
    assert trace[0][0].tolist() == [17, 19, 28] and picks[0] == 19 and trace[1][0].tolist() == [17, 28] and picks[1] == 28
    assert len(G.greedy_unmask(x, mask, candidates=[19])) == 3
    with pytest.raises(ValueError):
        G.greedy_unmask(x.expand(2, -1, -1, -1, -1), mask.expand(2, -1))
    with pytest.raises(ValueError):
        G.greedy_unmask(x, mask, num_steps=2, candidates=[19])
    # another target, another frame's region: same code path, scored against the given target
    tgt = torch.from_numpy(g["target_x"]).cuda()[:1]
    _, p2, s2, t2 = G.greedy_unmask(x, mask, target=tgt, candidates=[17, 19], return_scores=True)
    rows = mask.expand(2, -1).clone()
    rows[0, 17] = rows[1, 19] = False
    region_mask = torch.ones_like(mask)
    region_mask[:, 16:] = False
    direct = G.get_error_on_target_region(x.expand(2, -1, -1, -1, -1), rows, region_mask.expand(2, -1), target=tgt.expand(2, -1, -1, -1, -1))
    assert np.array_equal(direct.cpu().numpy(), t2[0][1])
