"""Ragged batches through the predictor on a real MI355X: rows with different visible-token counts run as ONE batch (cwm_model_set_ragged;
`forward(..., ragged=True)`), each predicted from exactly its own visible tokens -- what the reference computes for the row alone at B = 1
(tests/golden/make_golden_ragged.py), where in a batch it would first un-mask random masked patches until the counts agree."""
import os

import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import config as C, prediction, segmentation, synthetic as S, vmae
from oracle import vmae_oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
BASE8 = C.CONFIGS["base_8x8patch_2frames_1tube"]
PARITY_TOL = 1e-3   # tests/test_model_gpu.py
REASSOC_TOL = 5e-5  # what tests/test_model_gpu.py holds the re-association of fp32 sums to (other tilings, lanes, batch sizes)


def build(cfg, seed, mode="parity"):
    m = vmae.PretrainVisionTransformer(cfg, mode=mode)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, seed).items()})
    return m.to("cuda:0").eval()


def own_rows(y, n_vis, Nt):
    """row b's predictions out of a ragged result: its last Nt - Nv_b rows"""
    return [y[b, y.shape[1] - (Nt - int(n)):] for b, n in enumerate(n_vis)]


@pytest.fixture(scope="module")
def base8():
    """model, preprocessed frames and masks of ragged_base8.npz, and the fixture"""
    g = np.load(os.path.join(GOLDEN, "ragged_base8.npz"))
    assert len(set(g["n_vis"].tolist())) >= 3 and g["n_vis"].tolist() == [785, 792, 824]  # (824 = 6 * 128 + 56)
    m = build(BASE8, int(g["seed"]))
    x = torch.from_numpy(S.synthetic_frames(3, BASE8, int(g["seed"]))).cuda()
    mask = torch.from_numpy(g["mask"]).cuda()
    assert ((~mask).sum(1).cpu().numpy() == g["n_vis"]).all()
    return m, x, O.preprocess(x.cpu()).cuda(), mask, g


@pytest.mark.parametrize("fused", [1, 0])
def test_ragged_tiny_golden(fused):
    g = np.load(os.path.join(GOLDEN, "ragged_tiny.npz"))
    n_vis = g["n_vis"].tolist()
    assert len(set(n_vis)) >= 3
    m = build(TINY, int(g["seed"]))
    m.set_option("index_fused", fused)
    G = prediction.PredictorBasedGenerator(predictor=m, imagenet_normalize_inputs=True, temporal_dim=2)
    x, mask = torch.from_numpy(g["x"]), torch.from_numpy(g["mask"])
    xd, md = x.cuda(), mask.cuda()
    for rng in (None, (min(n_vis), max(n_vis))):
        y = m(G._preprocess(xd), md, ragged=True, n_vis_range=rng).cpu().numpy()
        assert y.shape == g["y_tokens"].shape
        err = np.abs(y - g["y_tokens"]).max()  # (the rows before a row's predictions are zero on both sides)
        print("ragged tiny, index_fused=%d, range %s: tokens max-abs vs the reference row by row %.3e" % (fused, rng, err))
        assert err <= 2e-4
    _, video = m.predict_video(xd, md, ragged=True)
    video = video.cpu()
    assert (video - torch.from_numpy(g["video"])).abs().max().item() <= 2e-4
    vis_pix = O.patches_to_video((~mask)[..., None].expand(-1, -1, 192).float(), 2, 3, 32, 32, 8).bool()
    assert torch.equal(video[vis_pix], x[vis_pix])  # visible patches are bit-exact copies of the input


def test_ragged_base8_golden_parity_fast_and_own_batch1(base8):
    m, x, xp, mask, g = base8
    Nt, n_vis = BASE8.num_tokens, g["n_vis"].tolist()
    m.mode = "parity"
    y = m(xp, mask, ragged=True, n_vis_range=(785, 824))
    assert y.shape == (3, Nt - 785, 192)
    _, video = m.predict_video(x, mask, ragged=True, n_vis_range=(785, 824))
    for b, yb in enumerate(own_rows(y, n_vis, Nt)):
        err = np.abs(yb[::2].cpu().numpy() - g["y%d" % b]).max()
        alone = m(xp[b:b + 1], mask[b:b + 1])[0]  # the library's own rectangular forward of the row
        d = (yb - alone).abs().max().item()
        print("ragged base8 parity row %d (n_vis %d): vs reference %.3e, vs own batch-1 forward %.3e" % (b, n_vis[b], err, d))
        assert err <= PARITY_TOL and d <= REASSOC_TOL
        assert (y[b, :y.shape[1] - yb.shape[0]] == 0).all()
    rows = video[:, 1, :, :: BASE8.img_size[0] // 8].cpu().numpy()
    assert np.abs(rows - g["video_frame1_rows"]).max() <= PARITY_TOL
    m.mode = "fast"
    try:
        yf = m(xp, mask, ragged=True, n_vis_range=(785, 824))
        for b, yb in enumerate(own_rows(yf, n_vis, Nt)):
            e = np.abs(yb[::2].cpu().numpy() - g["y%d" % b])
            print("ragged base8 fast row %d: max %.3e mean %.3e" % (b, e.max(), e.mean()))
            assert e.max() <= 5e-2 and e.mean() <= 1.5e-2  # the bound of test_base8_golden_parity_and_fast
    finally:
        m.mode = "parity"


def test_equal_counts_with_ragged_on_match_ragged_off(base8):
    m, _, _, _, _ = base8
    x = O.preprocess(torch.from_numpy(S.synthetic_frames(4, BASE8, 5))).cuda()
    mask = torch.from_numpy(S.synthetic_masks(4, BASE8, 8, 5)).cuda()
    off = m(x, mask)
    on = m(x, mask, ragged=True)
    assert on.shape == off.shape
    d = (on - off).abs().max().item()
    print("equal counts, ragged on vs off: %.3e" % d)
    assert d <= REASSOC_TOL
    assert torch.equal(m(x, mask), off)  # and off again is what it was


def ragged16():
    ks = [1, 8, 40, 3, 8, 17, 40, 2, 9, 1, 33, 8, 5, 40, 12, 7]
    x = O.preprocess(torch.from_numpy(S.synthetic_frames(16, BASE8, 7))).cuda()
    mask = torch.from_numpy(np.stack([S.synthetic_masks(1, BASE8, k, 7 + r)[0] for r, k in enumerate(ks)])).cuda()
    return x, mask, [784 + k for k in ks]


def test_ragged_batch16_two_lanes_match_one_lane(base8):
    m, _, _, _, _ = base8
    x, mask, n_vis = ragged16()
    try:
        m.set_lanes(1)
        one = m(x, mask, ragged=True)
        m.set_lanes(2)
        two = m(x, mask, ragged=True)
    finally:
        m.set_lanes(2)
    assert one.shape == (16, BASE8.num_tokens - 785, 192) and torch.isfinite(one).all()
    d = (one - two).abs().max().item()
    print("ragged batch 16, two lanes vs one: %.3e" % d)
    assert d <= REASSOC_TOL
    # row 5 alone, rectangular: the batch did not leak into it
    alone = m(x[5:6], mask[5:6])[0]
    assert (own_rows(two, n_vis, BASE8.num_tokens)[5] - alone).abs().max().item() <= REASSOC_TOL


@pytest.mark.parametrize("row", [1, 14])  # a row of either lane (16 rows: 8 + 8)
def test_ragged_rows_outside_the_range_are_refused(base8, row):
    m, _, _, _, _ = base8
    x, mask, n_vis = ragged16()
    lo, hi = min(n_vis), max(n_vis)
    above = mask.clone()
    above[row, 784:784 + 60] = False       # more visible tokens than the cap
    below = mask.clone()
    below[row, :100] = True                # fewer than n_vis_min
    empty = mask.clone()
    empty[row] = True                      # none at all
    for bad in (above, below, empty):
        with pytest.raises(RuntimeError, match="between %d" % lo):
            m(x, bad, ragged=True, n_vis_range=(lo, hi))
    y = m(x, mask, ragged=True, n_vis_range=(lo, hi))  # the handle works afterwards
    assert torch.isfinite(y).all()
    with pytest.raises(RuntimeError, match="do not all have n_vis"):  # ragged off: unequal rows are refused as ever
        m(x, mask)
    with pytest.raises(RuntimeError):
        m(x, mask, ragged=True, n_vis_range=(hi + 1, hi))


def test_generator_runs_counterfactual_prompts_as_ragged_batches():
    """ragged_prompts_tiny.npz: 7 prompts built by the reference's shifter, masks before its rectangulariser (16 ... 19 visible tokens), every row
    predicted by the reference alone.  With ragged_batches=True the wrapper builds those very masks, draws nothing from torch's global generator, and
    predicts every row as the reference does alone -- whatever the chunking."""
    g = np.load(os.path.join(GOLDEN, "ragged_prompts_tiny.npz"))
    assert g["masks"].shape[0] >= 6 and len(set(g["n_vis"].tolist())) >= 3
    m = build(TINY, int(g["seed"]))
    G = segmentation.FlowGenerator(predictor=m, imagenet_normalize_inputs=True, temporal_dim=2, ragged_batches=True)
    x = torch.from_numpy(g["x"]).cuda()
    active, passive = torch.from_numpy(g["active"]).cuda(), torch.from_numpy(g["passive"]).cuda()
    shifts = [[int(v) for v in row] for row in g["shifts"]]
    Sn = len(shifts)
    torch.manual_seed(5)
    state = torch.get_rng_state()
    G.set_input(x)
    _, masks = G.create_motion_counterfactuals(x, masks=passive, active_patches=active, shifts=shifts, num_samples=Sn, fix_passive=True, reset_shifts=True)
    assert np.array_equal(masks.cpu().numpy(), g["masks"])  # bit-equal to the reference's masks before rectangularisation
    outs = {}
    for chunk in (None, 2, 6):
        y = G.predict_counterfactual_videos(x, active, passive_patches=passive, shifts=shifts, num_samples=Sn, sample_batch_size=chunk, fix_passive=True,
                                            frame=1)
        assert y.shape == g["videos"].shape
        err = np.abs(y.cpu().numpy() - g["videos"]).max()
        print("ragged prompts, sample_batch_size=%s: videos max-abs vs the reference row by row %.3e" % (chunk, err))
        assert err <= 2e-4
        outs[chunk] = y
    assert (outs[2] - outs[6]).abs().max().item() <= REASSOC_TOL and (outs[2] - outs[None]).abs().max().item() <= REASSOC_TOL
    assert torch.equal(torch.get_rng_state(), state)  # nothing was drawn
    # the default still rectangularises: every row ends up with the smallest masked count, on the global generator
    G.ragged_batches = False
    _, rect = G.create_motion_counterfactuals(x, masks=passive, active_patches=active, shifts=shifts, num_samples=Sn, fix_passive=True, reset_shifts=True)
    assert len(set((~rect).sum(1).tolist())) == 1 and not torch.equal(torch.get_rng_state(), state)


def test_generator_predict_on_unequal_rows():
    """`G.predict` on the four rows of ragged_tiny.npz: with ragged_batches the reference's row-by-row videos and untouched masks; by default the
    rectangulariser equalises the rows first (and the rows that were shown an extra patch differ from their own prediction)."""
    g = np.load(os.path.join(GOLDEN, "ragged_tiny.npz"))
    m = build(TINY, int(g["seed"]))
    x, mask = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["mask"]).cuda()
    G = prediction.PredictorBasedGenerator(predictor=m, imagenet_normalize_inputs=True, temporal_dim=2, ragged_batches=True)
    md = mask.clone()
    video = G.predict(x, md, frame=None)
    assert torch.equal(md, mask)
    assert (video.cpu() - torch.from_numpy(g["video"])).abs().max().item() <= 2e-4
    assert torch.equal(G.predict(x, mask.clone()), video[:, 1:2])  # frame=-1: the last frame
    G.ragged_batches = False
    md = mask.clone()
    torch.manual_seed(0)
    rect = G.predict(x, md, frame=None)
    assert len(set((~md).sum(1).tolist())) == 1 and not torch.equal(md, mask)
    assert torch.isfinite(rect).all() and (rect.cpu() - torch.from_numpy(g["video"])).abs().max().item() > 2e-4


# ---- properties of the ragged forward that the fixtures cannot see (TINY, ragged_tiny.npz) --------------------------------------------------------------
MODES = ("parity", "fast")


@pytest.fixture(scope="module")
def tiny():
    """frames, masks and counts of ragged_tiny.npz on the device, and one model per mode"""
    g = np.load(os.path.join(GOLDEN, "ragged_tiny.npz"))
    n_vis = g["n_vis"].tolist()
    assert len(set(n_vis)) >= 3 and max(n_vis) < TINY.num_tokens - 1
    models = {mode: build(TINY, int(g["seed"]), mode) for mode in MODES}
    return models, torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["mask"]).cuda(), n_vis


def masked_pixels(mask):
    """bool [B, T, C, H, W] of the TINY geometry: the pixels of the masked patches"""
    return O.patches_to_video(mask.cpu()[..., None].expand(-1, -1, 192).float(), 2, 3, 32, 32, 8).bool()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("mode", MODES)
def test_ragged_fused_and_unfused_index_prologue_give_the_same_bits(tiny, mode):
    """The two forms differ in what the padding rows [count, cap) of the embed operand hold (zeros / masked tokens); every launch that reads those rows
    is row-wise and planned alike, and the attention never stages them: each row's predictions and the video agree bit for bit."""
    models, x, mask, n_vis = tiny
    m = models[mode]
    out = {}
    try:
        for fused in (1, 0):
            m.set_option("index_fused", fused)
            out[fused] = m.predict_video(x, mask, ragged=True)
    finally:
        m.set_option("index_fused", 1)
    for a, b in zip(own_rows(out[1][0], n_vis, TINY.num_tokens), own_rows(out[0][0], n_vis, TINY.num_tokens)):
        assert a.shape[0] > 0 and torch.isfinite(a).all() and same_bits(a, b), (mode, (a - b).abs().max().item())
    assert same_bits(out[1][1], out[0][1])


@pytest.mark.parametrize("mode", MODES)
def test_nan_under_the_mask_never_reaches_a_prediction(tiny, mode):
    """The raw pixels of every masked patch are NaN.  Ragged, fused: they are never read.  Ragged, unfused: the patch gather reads perm[count .. cap), masked
    tokens, into the padding rows, which are NaN from there on.  Rectangular (equal counts): never read.  Tokens and the masked part of the video are
    bitwise what the clean input gives, and the video holds no NaN."""
    models, x, mask, n_vis = tiny
    m = models[mode]
    Nt = TINY.num_tokens
    eq_mask = torch.from_numpy(S.synthetic_masks(4, TINY, 4, 11)).cuda()
    assert len(set((~eq_mask).sum(1).tolist())) == 1
    cases = [("ragged fused", mask, dict(ragged=True), 1), ("ragged unfused", mask, dict(ragged=True), 0), ("rectangular", eq_mask, {}, 1)]
    try:
        for name, mk, kw, fused in cases:
            hidden = masked_pixels(mk)
            xn = x.clone()
            xn[hidden.cuda()] = float("nan")
            assert torch.isnan(xn).any() and hidden.any() and not hidden.all()
            m.set_option("index_fused", fused)
            y0, v0 = m.predict_video(x, mk, **kw)
            y1, v1 = m.predict_video(xn, mk, **kw)
            assert not torch.isnan(v1).any(), (mode, name, "NaN in the video")
            assert torch.isfinite(y0).all() and same_bits(y1, y0), (mode, name, "tokens")
            assert same_bits(v1.cpu()[hidden], v0.cpu()[hidden]), (mode, name, "masked part of the video")
            assert same_bits(v1.cpu()[~hidden], x.cpu()[~hidden]), (mode, name, "visible part of the video")
    finally:
        m.set_option("index_fused", 1)
    assert Nt - max(n_vis) > 0


@pytest.mark.parametrize("mode", MODES)
def test_ragged_cap_above_every_count(tiny, mode):
    """n_vis_range = (lo, Nt - 1): every sample carries padding rows, the encoder's M grows from 4 x 22 to 4 x 31 rows -- other tilings at most, which the
    file holds to REASSOC_TOL."""
    models, x, mask, n_vis = tiny
    m = models[mode]
    Nt, lo, hi = TINY.num_tokens, min(n_vis), max(n_vis)
    xp = O.preprocess(x.cpu()).cuda()
    tight = m(xp, mask, ragged=True, n_vis_range=(lo, hi))
    loose = m(xp, mask, ragged=True, n_vis_range=(lo, Nt - 1))
    assert tight.shape == loose.shape == (4, Nt - lo, 192)
    for b, (a, c) in enumerate(zip(own_rows(tight, n_vis, Nt), own_rows(loose, n_vis, Nt))):
        d = (a - c).abs().max().item()
        print("ragged tiny %s row %d: cap %d against cap %d: %.3e" % (mode, b, hi, Nt - 1, d))
        assert torch.isfinite(c).all() and d <= REASSOC_TOL, (mode, b, d)


@pytest.mark.parametrize("mode", MODES)
def test_ragged_batch_on_a_dirty_workspace_equals_a_fresh_handle(tiny, mode):
    """A rectangular batch with large-magnitude inputs -- more samples and more visible tokens than the ragged batch needs, so the workspace is not
    re-allocated -- leaves every shared buffer full of stale rows; the ragged batch after it is bitwise what a fresh handle computes."""
    models, x, mask, n_vis = tiny
    m = models[mode]
    fresh = build(TINY, 3, mode)
    y_fresh, v_fresh = fresh.predict_video(x, mask, ragged=True)
    big = 1e4 * O.preprocess(torch.from_numpy(S.synthetic_frames(6, TINY, 9))).cuda()
    big_mask = torch.from_numpy(S.synthetic_masks(6, TINY, 8, 9)).cuda()
    assert int((~big_mask[0]).sum()) > max(n_vis) and big.abs().max().item() > 1e4
    m(big, big_mask)
    y, v = m.predict_video(x, mask, ragged=True)
    assert torch.isfinite(y_fresh).all() and same_bits(y, y_fresh) and same_bits(v, v_fresh), (mode, (y - y_fresh).abs().max().item())
