"""Counterfactual motion-map sampling on the device: the flow-sample filter kernels (`cwm_flow_filter_stats` / `_apply` / `_pack`) against goldens
recorded from the reference's `FlowSampleFilter` (tests/golden/make_golden_motion_sampling.py) and `FlowGenerator.sample_counterfactual_motion_map`
end to end against the reference's own run.

Filter cases (motion_filter.npz), B=2, S=12 at 224^2 with 28^2 and 56^2 patches and at 96^2 with 10^2 (ratio 9.6: the general bilinear formula).
Per sample: 0 kept; 1 kept, clumped 2x2 active set; 2 rejected by patch_magnitude alone; 3 by flow_area alone; 4 by num_corners alone; 5 empty
active set; 6 kept, active patches on the last grid row and column; 7 NaN pixels, one under an active patch's tap; 8 rejected by flow_area and
num_corners; 9 kept, two active patches; 10 rejected by patch_magnitude alone (noise only); 11 kept.

Bounds.  Decisions and the integer counts are compared exactly: the maker asserts that no pixel magnitude lies within 1e-6 (relative) of the
threshold and no per-sample statistic within 1e-3.  patch_mag: relative, the larger of 8 x the reference's recorded fp32-vs-float64 difference
and (4 n_active + 4) 2^-23 (`patch_mag_bound`); both are >= 30 times inside the 1e-3 guard band.

Measured on an MI355X: patch_mag 7.4e-8 / 1.0e-7 / 9.5e-7 relative to the reference's float64 evaluation for the three cases (bounds
2.4e-6 / 2.4e-6 / 6.8e-6), identical in the three layouts; end-to-end flows 2.5e-4 px max-abs against the reference (bound 4e-4)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import _lib, raft, sampling, segmentation, synthetic as S, vmae

import flow_filter_restatement as R
from test_motion_sampling_cpu import FILTER_CASES, GOLDEN, TINY, load_filter_case, patch_mag_bound

pytestmark = pytest.mark.gpu
# the patch_mag bound for one active patch at 224^2 / 28^2 (the tests without a golden): the larger of 8 x the rounding the fixture of that geometry
# records for the reference itself and the floor (4 n_active + 4) 2^-23
ONE_PATCH_BOUND = max(8.0 * float(np.load(os.path.join(GOLDEN, "motion_filter.npz"))["f224_g28_patch_mag_rounding"]), 8 * 2.0 ** -23)


def layouts(flows_np):
    """name -> a [B,2,H,W,S] CUDA tensor with the golden's values: the sample-outermost view of a '(b s) 1 c h w' batch, the packed layout, and
    a slice along W of a larger sample-outermost tensor (arbitrary strides)."""
    f = torch.from_numpy(flows_np).cuda()
    B, Cc, H, W, Sn = f.shape
    batch = f.permute(0, 4, 1, 2, 3).reshape(B * Sn, 1, Cc, H, W).contiguous()
    view = segmentation.FlowGenerator.batch_to_samples(batch, t=0, B=B)
    assert view.data_ptr() == batch.data_ptr() and (Sn == 1 or not view.is_contiguous())
    wide = torch.full((B, Sn, Cc, H, W + 5), 1e6, device="cuda")
    wide[..., 3:W + 3] = f.permute(0, 4, 1, 2, 3)
    return {"view": view, "packed": f.contiguous(), "strided": wide[..., 3:W + 3].permute(0, 2, 3, 4, 1)}


def rel_err(got, want):
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok)
    return float((np.abs(got[ok].astype(np.float64) - want[ok]) / np.maximum(np.abs(want[ok]), 1e-30)).max())


@pytest.mark.parametrize("tag", FILTER_CASES)
def test_filter_statistics_decisions_and_zeroing_vs_reference(tag):
    g = np.load(os.path.join(GOLDEN, "motion_filter.npz"))
    flows_np, active = load_filter_case(g, tag)
    thr, area_thr, corner_thr = (float(v) for v in g["thresholds"])
    act = torch.from_numpy(active).cuda()
    subsets = json.loads(str(g["subsets"]))
    bound = patch_mag_bound(g, tag, active)
    first = None
    for name, f in layouts(flows_np).items():
        before = f.clone()
        filt = sampling.FlowSampleFilter(subsets[-1], thr, area_thr, int(corner_thr))
        out, mask = filt(f, act)
        st = {k: v.cpu().numpy() for k, v in filt.last_stats.items()}
        err = rel_err(st["patch_mag"], g[tag + "_patch_mag64"])
        print("%s %s: patch_mag rel err vs float64 %.3e (bound %.3e), vs the reference's fp32 %.3e" % (tag, name, err, bound, rel_err(st["patch_mag"], g[tag + "_patch_mag"].astype(np.float64))))
        assert np.array_equal(st["reject"], g[tag + "_reject"][-1]), name
        assert np.array_equal(st["area_count"], g[tag + "_area_count"]) and np.array_equal(st["corner_count"], g[tag + "_corner_count"]), name
        assert st["area_count"].dtype == np.int32 and st["reject"].dtype == bool
        assert err <= bound, (name, err, bound)
        # rejected samples all zero, kept samples bitwise unchanged, in place; contiguous result; expanded mask
        rej = filt.last_stats["reject"]
        for b in range(f.shape[0]):
            assert (f[b][..., rej[b]] == 0).all() and torch.equal(f[b][..., ~rej[b]].view(torch.int32), before[b][..., ~rej[b]].view(torch.int32)), name
        assert out.is_contiguous() and out.shape == f.shape and torch.equal(out.view(torch.int32), f.contiguous().view(torch.int32))
        assert (out.data_ptr() == f.data_ptr()) == (name == "packed")
        assert mask.shape == f.shape and mask.dtype == torch.bool and mask.stride()[1:4] == (0, 0, 0) and torch.equal(mask.amax((1, 2, 3)), rej)
        if name == "strided":  # nothing outside the slice was written
            base = f._base if f._base is not None else f
            assert (base[..., :3] == 1e6).all() and (base[..., -2:] == 1e6).all()
        # layouts and repeated runs agree bitwise
        again = sampling.FlowSampleFilter(subsets[-1], thr, area_thr, int(corner_thr)).compute_stats(before, act)
        for k in st:
            assert np.array_equal(again[k].cpu().numpy(), st[k], equal_nan=True), (name, k)
        if first is None:
            first = st
        for k in st:
            assert np.array_equal(first[k].view(np.uint8), st[k].view(np.uint8)), (name, k)
    # each method alone and each pair
    view = layouts(flows_np)["view"]
    for sub, want in zip(subsets, g[tag + "_reject"]):
        got = sampling.FlowSampleFilter(sub, thr, area_thr, int(corner_thr)).compute_stats(view, act)["reject"]
        assert np.array_equal(got.cpu().numpy(), want), sub
    # a uint8 mask with a strided sample axis takes the byte-wise mask path: same bits
    act8 = torch.ones(active.shape[0], active.shape[1], 2 * active.shape[2], dtype=torch.uint8, device="cuda")[..., ::2]
    act8.copy_(act)
    got = sampling.FlowSampleFilter(subsets[-1], thr, area_thr, int(corner_thr)).compute_stats(view, act8)
    assert np.array_equal(got["patch_mag"].cpu().numpy().view(np.uint32), first["patch_mag"].view(np.uint32))


@pytest.mark.parametrize("B,Sn", [(1, 1), (1, 256), (2, 5)])
def test_filter_sizes_against_restatement(B, Sn):
    """B=1 S=1, S=256 and an odd S (the scalar kernels): against the torch restatement on seeded blobs, outside the guard bands."""
    rng = np.random.Generator(np.random.PCG64(B * 1000 + Sn))
    size, grid = 224, 28
    blobs = np.zeros((B, Sn, 1, 5), dtype=np.float32)
    active = np.ones((B, 2 * grid * grid, Sn), dtype=bool)
    active[:, : grid * grid] = False
    for b in range(B):
        for s in range(Sn):
            py, px = rng.integers(grid, size=2)
            active[b, grid * grid + py * grid + px, s] = False
            blobs[b, s, 0] = ((py + 0.5) * 8 - 0.5 + rng.integers(-30, 30) * (s % 3 == 0), (px + 0.5) * 8 - 0.5, rng.uniform(10, 150), rng.uniform(-25, 25), rng.uniform(-25, 25))
    flows_np = S.blob_flow_samples(size, Sn, blobs)
    act = torch.from_numpy(active).cuda()
    ref64 = R.flow_filter_stats(torch.from_numpy(flows_np).double(), torch.from_numpy(active), 5.0)
    mag64 = ref64[3].numpy()
    in_band = np.abs(mag64 / 5.0 - 1) < 1e-6
    safe = (np.abs(ref64[0].numpy() / 5.0 - 1) >= 1e-3) & (np.abs(ref64[1].numpy() / (size * size) / 0.75 - 1) >= 1e-3) & (in_band.sum((1, 2)) == 0)
    _, _, dec = R.flow_filter_forward(torch.from_numpy(flows_np).clone(), torch.from_numpy(active))
    for name, f in layouts(flows_np).items():
        filt = sampling.FlowSampleFilter()
        before = f.clone()
        out, mask = filt(f, act)
        st = {k: v.cpu().numpy() for k, v in filt.last_stats.items()}
        assert rel_err(st["patch_mag"], ref64[0].numpy()) <= ONE_PATCH_BOUND
        assert (np.abs(st["area_count"] - ref64[1].numpy()) <= in_band.sum((1, 2))).all()
        assert np.array_equal(st["reject"][safe], dec.numpy()[safe]) and safe.mean() >= 0.5  # (not vacuous: at least half of the samples are outside the guard bands)
        rej = filt.last_stats["reject"]
        assert torch.equal(out, torch.where(rej.view(B, 1, 1, 1, Sn), torch.zeros_like(before), before)) and out.is_contiguous()


def test_invalid_arguments_are_returned_not_faulted():
    lib = _lib.get_lib()
    f = torch.zeros(1, 2, 16, 16, 4, device="cuda")
    act = torch.ones(1, 2 * 16, 4, dtype=torch.bool, device="cuda")
    pm, rj = torch.empty(1, 4, device="cuda"), torch.empty(1, 4, dtype=torch.uint8, device="cuda")
    ac, cc = torch.empty(1, 4, dtype=torch.int32, device="cuda"), torch.empty(1, 4, dtype=torch.int32, device="cuda")
    fs, as_ = (C.c_int64 * 5)(*f.stride()), (C.c_int64 * 3)(*act.stride())
    stream = _lib.current_stream_handle(f.device)

    def stats(flows=f.data_ptr(), Cc=2, H=16, W=16, Sn=4, a=act.data_ptr(), Np=32, methods=7, out=pm.data_ptr()):
        return lib.cwm_flow_filter_stats(flows, fs, 1, Cc, H, W, Sn, a, as_, Np, methods, 5.0, 0.75, 2.0, out, ac.data_ptr(), cc.data_ptr(), rj.data_ptr(), stream)

    assert stats() == 0
    for kw, word in [({"Cc": 3}, "C=2"), ({"H": 8}, "H="), ({"Np": 31}, "Np=31"), ({"Np": 30}, "Np=30"), ({"flows": None}, "null"), ({"a": None}, "null"),
                     ({"out": None}, "null"), ({"Sn": 0}, "S=0"), ({"methods": 8}, "methods")]:
        assert stats(**kw) == -1, kw  # CWM_ERR_INVALID
        assert word in lib.cwm_last_error().decode(), (kw, lib.cwm_last_error())
    assert lib.cwm_flow_filter_apply(f.data_ptr(), fs, 1, 3, 16, 16, 4, rj.data_ptr(), stream) == -1
    assert lib.cwm_flow_filter_apply(f.data_ptr(), fs, 1, 2, 16, 16, 4, None, stream) == -1
    assert lib.cwm_flow_filter_apply(None, fs, 1, 2, 16, 16, 4, rj.data_ptr(), stream) == -1
    assert lib.cwm_flow_filter_pack(f.data_ptr(), fs, 1, 2, 16, 16, 4, rj.data_ptr(), pm.data_ptr(), stream) == -1 and b"contiguous" in lib.cwm_last_error()
    torch.cuda.synchronize()
    with pytest.raises(_lib.CwmHipError):
        sampling.FlowSampleFilter()(torch.zeros(1, 2, 16, 8, 4, device="cuda"), act)
    assert lib.cwm_version().decode().startswith("cwm_hip 0.10.")


def tiny_generator(**kw):
    m = vmae.PretrainVisionTransformer(TINY)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(TINY, 3).items()})
    return segmentation.FlowGenerator(predictor=m.cuda().eval(), flow_model=S.SyntheticFlow(), imagenet_normalize_inputs=True, temporal_dim=2, **kw)


def test_sample_counterfactual_motion_map_vs_reference():
    """The reference's own `sample_counterfactual_motion_map` (B = 1 per call: its prompt loop does not run at B > 1) on the tiny predictor and the
    stand-in flow, two movies, two sample_batch_sizes, filter on and off: patches bit-equal, decisions equal, flows within the 4e-4 of the driver
    test (tests/test_prompts_gpu.py), results across the sample_batch_sizes within its 1e-5."""
    g = np.load(os.path.join(GOLDEN, "motion_sampling_e2e.npz"))
    params = json.loads(str(g["filter_params"]))
    x = torch.from_numpy(g["x"]).cuda()
    for movie in (0, 1):
        outs = {}
        for sbs in (8, 3):
            for do_filter in (True, False):
                tag = "m%d_sbs%d_%s" % (movie, sbs, "filter" if do_filter else "raw")
                G = tiny_generator(seed=movie, flow_sample_filter_params=params)
                flows, active, passive = G.sample_counterfactual_motion_map(x[movie:movie + 1], num_samples=8, sample_batch_size=sbs, do_filter=do_filter)
                assert np.array_equal(active.cpu().numpy(), g["active_" + tag]) and np.array_equal(passive.cpu().numpy(), g["passive_" + tag]), tag
                assert np.array_equal(np.array(G.shifts), g["shifts_" + tag]), tag
                assert flows.shape == (1, 2, 32, 32, 8) and (flows.is_contiguous() or not do_filter)
                err = np.abs(flows.cpu().numpy() - g["flows_" + tag]).max()
                print(tag, "flows max-abs vs reference %.3e" % err)
                assert err <= 4e-4, (tag, err)
                if do_filter:
                    assert np.array_equal(G.flow_sample_filter.last_stats["reject"].cpu().numpy(), g["reject_m%d_sbs%d_raw" % (movie, sbs)]), tag
                    pm = G.flow_sample_filter.last_stats["patch_mag"].cpu().numpy()
                    # flows within 4e-4 px per component -> magnitudes within sqrt(2) 4e-4; the bilinear weights and the mean are convex
                    assert np.abs(pm - g["patch_mag_m%d_sbs%d_raw" % (movie, sbs)]).max() <= 2 ** 0.5 * 4e-4 + 1e-5
                outs[(sbs, do_filter)] = flows
        for do_filter in (True, False):
            assert (outs[(8, do_filter)] - outs[(3, do_filter)]).abs().max().item() <= 1e-5
        assert not torch.equal(outs[(8, True)], outs[(8, False)])
        # flow_sample_filter=None returns the unfiltered flows, like do_filter=False
        G = tiny_generator(seed=movie, flow_sample_filter=None)
        flows, _, _ = G.sample_counterfactual_motion_map(x[movie:movie + 1], num_samples=8, sample_batch_size=8)
        assert torch.equal(flows, outs[(8, False)])
    # B = 2 in one call: every movie's S prompts share the S shifts; shapes, and the filter's decisions against the restatement
    G = tiny_generator(seed=0, flow_sample_filter_params=params)
    raw, active, passive = G.sample_counterfactual_motion_map(x, num_samples=8, sample_batch_size=5, do_filter=False)
    G = tiny_generator(seed=0, flow_sample_filter_params=params)
    flows, active2, _ = G.sample_counterfactual_motion_map(x, num_samples=8, sample_batch_size=5)
    assert flows.shape == (2, 2, 32, 32, 8) and torch.equal(active, active2) and active.shape == (2, 32, 8)
    want, _, dec = R.flow_filter_forward(raw.clone(), active, **params)
    assert torch.equal(G.flow_sample_filter.last_stats["reject"], dec) and torch.equal(flows, want)


def test_real_path_smoke_raft_flow_model():
    """Our RAFT (synthetic weights) as the flow model at 224^2, S=4, no golden: shapes, finiteness, and the filter against the torch restatement on the
    same flows.  Random weights give no control over the guard bands, so decisions are compared where the restatement's statistics are outside them."""
    from counterfactualworldmodels_amd import config as Cfg

    cfg = Cfg.VmaeConfig(name="tiny_224", img_size=(224, 224), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
    m = vmae.PretrainVisionTransformer(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 3).items()})
    flow_model = raft.RAFT()
    flow_model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(0).items()})
    thr = 1.0
    G = segmentation.FlowGenerator(predictor=m.cuda().eval(), flow_model=flow_model.cuda().eval(), imagenet_normalize_inputs=True, temporal_dim=2, raft_iters=6,
                                   flow_sample_filter_params={"flow_magnitude_threshold": thr, "flow_area_threshold": 0.75, "num_corners_threshold": 2})
    x = torch.from_numpy(S.raft_frames(1, 224, 224, seed=2)).cuda()
    raw, active, passive = G.sample_counterfactual_motion_map(x, num_samples=4, sample_batch_size=4, do_filter=False)
    assert raw.shape == (1, 2, 224, 224, 4) and torch.isfinite(raw).all() and active.shape == (1, 2 * 28 * 28, 4) and not raw.is_contiguous()
    f = raw.clone()
    out, mask = G.flow_sample_filter(f, active)
    st = {k: v.cpu().numpy() for k, v in G.flow_sample_filter.last_stats.items()}
    pm64, area64, corners64, mag64 = (v.cpu().numpy() for v in R.flow_filter_stats(raw.double(), active, thr))
    in_band = (np.abs(mag64 / thr - 1) < 1e-6).sum((1, 2))
    print("real path: patch_mag", st["patch_mag"], "area", st["area_count"] / 224 ** 2, "corners", st["corner_count"], "reject", st["reject"], "px in band", in_band)
    assert rel_err(st["patch_mag"], pm64) <= ONE_PATCH_BOUND
    assert (np.abs(st["area_count"] - area64) <= in_band).all()
    _, _, dec = R.flow_filter_forward(raw.clone(), active, flow_magnitude_threshold=thr)
    safe = (np.abs(pm64 / thr - 1) >= 1e-3) & (np.abs(area64 / 224 ** 2 / 0.75 - 1) >= 1e-3) & (in_band == 0)
    assert np.array_equal(st["reject"][safe], dec.cpu().numpy()[safe])
    assert out.is_contiguous() and out.shape == raw.shape and mask.shape == raw.shape
