"""Multi-shift prompts on the device (`cwm_multi_shift_prompts`): K groups of patches per prompt, each moved by its own pixel shift.

Every case of tests/golden/multi_shift.npz (recorded from the reference's `MultiShiftPatchesAndMask.forward`, see make_golden_multi_shift.py for
what each case is for) through the generator's `multi_patch_shifter` and through the raw C ABI: frames and masks bit-equal.  K = 1 with a
whole-patch shift against the single-shift kernel, bitwise.  The batch driver against the reference's own end-to-end run: masks and shifts equal,
videos and flows within the 4e-4 that tests/test_prompts_gpu.py and test_motion_sampling_gpu.py use for this predictor-plus-flow chain, two
sample_batch_sizes within their 1e-5.  The IMU-conditioned generator, and the argument errors of the entry point."""
import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import _lib, conjoined_vmae as CV, perturbation, segmentation, synthetic as S, vmae

from test_motion_sampling_cpu import GOLDEN, TINY
from test_multi_shift_cpu import REQUIRED_CASES, input_frames, load_cases

pytestmark = pytest.mark.gpu
CWM_ERR_INVALID = -1


def tiny_generator(cls=segmentation.FlowGenerator, **kw):
    m = vmae.PretrainVisionTransformer(TINY)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(TINY, 3).items()})
    return cls(predictor=m.cuda().eval(), flow_model=S.SyntheticFlow(), imagenet_normalize_inputs=True, temporal_dim=2, **kw)


@pytest.fixture(scope="module")
def generator():
    return tiny_generator()


def raw_call(x, points, masks, shifts, P, frame, S_=1, fix_passive=0, frames=True, masks_out=True, K=None, max_abs=None, W=None):
    """The C entry point itself on step-major tables (points [R,K,Nt], masks [R,Km,Nt] or None, shifts [R,K,2]); returns (status, x_out, mask_out)."""
    B, T, Cc, H, Wx = x.shape
    R, Kp, Nt = points.shape
    sh = torch.as_tensor(np.ascontiguousarray(shifts), dtype=torch.int32).cuda().contiguous()
    x_out = torch.full((R, T, Cc, H, Wx), -7.0, device="cuda") if frames else None
    m_out = torch.full((R, Nt), 3, dtype=torch.uint8, device="cuda") if masks_out else None
    st = _lib.get_lib().cwm_multi_shift_prompts(
        x.data_ptr(), B, T, Cc, H, Wx if W is None else W, P, frame % T, S_, Kp if K is None else K, fix_passive, points.data_ptr(), _lib.ptr(masks),
        0 if masks is None else masks.shape[1], sh.data_ptr(), int(np.abs(shifts).max()) if max_abs is None else max_abs, _lib.ptr(x_out), _lib.ptr(m_out),
        _lib.current_stream_handle(x.device))
    return st, x_out, m_out


@pytest.mark.parametrize("tag", REQUIRED_CASES)
def test_golden_case_bit_equal_through_the_shifter_and_the_raw_abi(tag, generator):
    g, meta = load_cases()
    c = meta[tag]
    x_np = input_frames(2, c["H"], c["W"])
    x = torch.from_numpy(x_np).cuda()
    masks = torch.from_numpy(g["case_%s_masks" % tag]).cuda()
    points = torch.from_numpy(g["case_%s_points" % tag]).cuda() if c["has_points"] else None
    shifts = [tuple(int(v) for v in r) for r in g["case_%s_shifts" % tag]]
    want_x, want_m = g["case_%s_x_p" % tag], g["case_%s_mask_ps" % tag]
    shifter = generator.multi_patch_shifter if c["P"] == 8 else perturbation.MultiShiftPatchesAndMask(patch_size=(1, c["P"], c["P"]))
    masks_before = masks.clone()
    x_p, mask_ps = shifter(x, masks, points, shifts, frame=c["frame"])
    assert x_p.dtype == torch.float32 and mask_ps.dtype == torch.bool and mask_ps.shape == (2, masks.shape[1])
    assert np.array_equal(x_p.cpu().numpy().view(np.uint32), want_x.view(np.uint32)), tag
    assert np.array_equal(mask_ps.cpu().numpy(), want_m), tag
    assert torch.equal(masks, masks_before) and shifter.shifts == shifts and shifter.num_shifts == c["K"]
    # list-of-tensors sequences and the [2,K] tensor of shifts: the same call
    if c["has_points"] and masks.dim() == 3:
        x_l, m_l = shifter(x, [masks[..., k] for k in range(c["K"])], tuple(points[..., k] for k in range(c["K"])), torch.tensor(shifts).T, frame=c["frame"])
        assert torch.equal(x_l, x_p) and torch.equal(m_l, mask_ps)
    # the raw ABI on step-major tables, both outputs / frames only / masks only
    m3 = masks if masks.dim() == 3 else masks.unsqueeze(-1)
    pts = (points if c["has_points"] else ~m3).permute(0, 2, 1).contiguous()
    base = m3.permute(0, 2, 1).contiguous() if c["has_points"] else None
    table = np.broadcast_to(np.array(shifts)[None], (2, c["K"], 2))
    st, xo, mo = raw_call(x, pts, base, table, c["P"], c["frame"])
    assert st == 0, _lib.get_lib().cwm_last_error()
    assert np.array_equal(xo.cpu().numpy().view(np.uint32), want_x.view(np.uint32)) and np.array_equal(mo.cpu().numpy().astype(bool), want_m), tag
    st, xo2, none_m = raw_call(x, pts, base, table, c["P"], c["frame"], masks_out=False)
    st2, none_x, mo2 = raw_call(x, pts, base, table, c["P"], c["frame"], frames=False)
    assert st == 0 and st2 == 0 and none_m is None and none_x is None and torch.equal(xo2, xo) and torch.equal(mo2, mo)


@pytest.mark.parametrize("fix_passive", [0, 1])
def test_one_whole_patch_step_equals_the_single_shift_kernel(fix_passive, generator):
    """K = 1 with a shift of whole patches is `cwm_shift_prompts`: B S = 6 rows (2 movies x 3 samples) with per-row shifts, some leaving the frame,
    fix_passive 0 and 1, both outputs and each one alone."""
    G = generator
    gen = torch.Generator().manual_seed(17 + fix_passive)
    B, S_, n, P = 2, 3, 16, 8
    x = torch.rand(B, 2, 3, 32, 32, generator=gen).cuda()
    R = B * S_
    passive = (torch.rand(R, 2 * n, generator=gen) < 0.6).cuda()
    active = (torch.rand(R, 2 * n, generator=gen) < 0.7).cuda()      # 0 = moved: about five patches per frame and row
    patch_shifts = torch.tensor([[1, 0], [0, -1], [-2, 1], [3, 3], [0, 0], [-1, -3]], dtype=torch.int32)
    G.inp_shape = tuple(x.shape)
    want_x, want_m = G._shift_rows(x, passive, active, patch_shifts, 1, bool(fix_passive), samples_per_movie=S_)
    assert not torch.equal(want_x[:, 1], x[:, 0 if fix_passive else 1].repeat_interleave(S_, 0))  # something moved
    pixel = (patch_shifts * P).numpy().reshape(R, 1, 2)
    got_x, got_m = perturbation.multi_shift_rows(x, ~active[:, None], passive[:, None], pixel, P, 1, fix_passive=fix_passive, samples_per_movie=S_)
    assert torch.equal(got_x.view(torch.int32), want_x.view(torch.int32)) and torch.equal(got_m, want_m)
    only_x, none_m = perturbation.multi_shift_rows(x, ~active[:, None], passive[:, None], pixel, P, 1, fix_passive=fix_passive, samples_per_movie=S_, masks_out=False)
    none_x, only_m = perturbation.multi_shift_rows(x, ~active[:, None], passive[:, None], pixel, P, 1, fix_passive=fix_passive, samples_per_movie=S_, frames=False)
    assert none_m is None and none_x is None and torch.equal(only_x, want_x) and torch.equal(only_m, want_m)


def test_driver_reproduces_the_reference_end_to_end():
    g, _ = load_cases()
    x = torch.from_numpy(g["e2e_x"]).cuda()
    frac = float(g["e2e_max_shift_fraction"])
    for movie in (0, 1):
        t = "e2e_m%d_" % movie
        active = torch.from_numpy(g[t + "active"]).cuda()
        outs = {}
        for sbs in (4, 3):
            G = tiny_generator(seed=movie, max_shift_fraction=frac)
            torch.manual_seed(int(g["e2e_seed"]) + movie)
            ys, fs = G.predict_multi_shift_counterfactual_videos_and_flows(x[movie:movie + 1], active, shifts=None, sample_batch_size=sbs)
            assert np.array_equal(np.array(G.shifts), g[t + "shifts"]), "the drawn shifts differ from the reference's"
            assert ys.shape == (4, 2, 3, 32, 32) and fs.shape == (4, 1, 2, 32, 32)
            ev, ef = np.abs(ys.cpu().numpy() - g[t + "videos"]).max(), np.abs(fs.cpu().numpy() - g[t + "flows"]).max()
            print("movie %d sample_batch_size %d: videos %.3e, flows %.3e max-abs vs the reference" % (movie, sbs, ev, ef))
            assert ev <= 4e-4 and ef <= 4e-4, (movie, sbs, ev, ef)
            outs[sbs] = (ys, fs)
        assert (outs[4][0] - outs[3][0]).abs().max().item() <= 1e-5 and (outs[4][1] - outs[3][1]).abs().max().item() <= 1e-5
        # the prompts themselves: frames bit-equal, masks equal after the one rectangulariser call; explicit shifts in each accepted form
        G = tiny_generator(seed=movie, max_shift_fraction=frac)
        torch.manual_seed(int(g["e2e_seed"]) + movie)
        batch = G._multi_shift_batch(x[movie:movie + 1], active, g[t + "shifts"].tolist(), None, 8, True, 1, {})
        assert np.array_equal(batch.x.cpu().numpy(), g[t + "x_p"]) and np.array_equal(batch.mask.cpu().numpy(), g[t + "mask"])
        assert batch.n_masked == int(g[t + "mask"][0].sum())
        torch.manual_seed(int(g["e2e_seed"]) + movie)
        as_tensor = torch.from_numpy(g[t + "shifts"]).permute(2, 1, 0)  # [2,K,S]
        y_t = G.predict_multi_shift_counterfactual_videos(x[movie:movie + 1], active, shifts=as_tensor, sample_batch_size=4)
        assert (y_t - outs[4][0]).abs().max().item() <= 1e-5
    # [B,Nt,K] patches shared by the samples, K pairs shared by the samples, two movies in one call: '(b s)' rows
    G = tiny_generator()
    torch.manual_seed(1)
    shared = torch.from_numpy(g["e2e_m0_active"][..., 0]).cuda().expand(2, -1, -1)
    ys = G.predict_multi_shift_counterfactual_videos(x, shared, shifts=[(8, 0), (3, -9), (-16, 8)], num_samples=2, sample_batch_size=None)
    assert ys.shape == (4, 2, 3, 32, 32) and len(G.shifts) == 4 and (ys[0] - ys[1]).abs().max().item() <= 1e-5 and not torch.equal(ys[0], ys[2])
    assert torch.equal(ys[:, 0], x[:, 0].repeat_interleave(2, 0))  # frame 0 is visible everywhere: the input comes back


def test_imu_conditioned_generator_one_whole_patch_step():
    """`ImuConditionedFlowGenerator` through the multi-shift driver: K = 1 with whole-patch shifts is `predict_counterfactual_videos` with the same
    head motion (the IMU stream goes through `_conditioning_kwargs` and follows each movie's prompts), on the tiny conjoined fixtures."""
    import os

    from test_conj_oracle import TINY_CONJ, conj_weights

    g = np.load(os.path.join(GOLDEN, "wrapper_conj.npz"))
    m = CV.ConjoinedPaddedVisionTransformer(TINY_CONJ)
    m.load_state_dict(conj_weights(TINY_CONJ, int(g["seed"])))
    G = segmentation.ImuConditionedFlowGenerator(predictor=m.cuda().eval(), flow_model=S.SyntheticFlow(), imagenet_normalize_inputs=True, temporal_dim=2)
    img, imu, act = (torch.from_numpy(g[k]).cuda() for k in ("img", "imu", "active"))
    shifts = [[int(v) for v in r] for r in g["shifts"]]
    P = G.patch_size[-1]
    torch.manual_seed(6)
    want = G.predict_counterfactual_videos(img, act.clone(), shifts=shifts, num_samples=4, sample_batch_size=3, head_motion=imu)
    torch.manual_seed(6)
    got = G.predict_multi_shift_counterfactual_videos(img, act.clone().unsqueeze(2), shifts=[[(dy * P, dx * P)] for dy, dx in shifts], num_samples=4,
                                                      sample_batch_size=3, head_motion=imu)
    assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-5
    assert not hasattr(m, "padding_mask")
    with pytest.raises(RuntimeError, match="head_motion"):
        G.predict_multi_shift_counterfactual_videos(img, act.clone().unsqueeze(2), shifts=[(P, 0)], num_samples=4)


def test_argument_errors_are_returned_and_nothing_is_launched():
    lib = _lib.get_lib()
    x = torch.rand(1, 2, 3, 32, 32, device="cuda")
    pts = torch.zeros(1, 2, 32, dtype=torch.bool, device="cuda")
    pts[0, :, 16 + 5] = True
    shifts = np.array([[[8, 0], [0, -8]]])
    st, xo, mo = raw_call(x, pts, None, shifts, 8, 1)
    assert st == 0 and not (xo == -7.0).any() and not (mo == 3).any()
    big = torch.zeros(1, perturbation.MAX_STEPS + 1, 32, dtype=torch.bool, device="cuda")
    for kw, word in [(dict(K=0), "K=0"), (dict(points=big, shifts=np.zeros((1, perturbation.MAX_STEPS + 1, 2), dtype=np.int64)), "K=%d" % (perturbation.MAX_STEPS + 1)),
                     (dict(max_abs=32), "min(H=32"), (dict(W=30), "W=30"), (dict(frames=False, masks_out=False), "null outputs")]:
        args = dict(points=pts, shifts=shifts)
        args.update(kw)
        st, xo, mo = raw_call(x, args.pop("points"), None, args.pop("shifts"), 8, 1, **args)
        assert st == CWM_ERR_INVALID, kw
        assert word in lib.cwm_last_error().decode(), (kw, lib.cwm_last_error())
        torch.cuda.synchronize()
        # nothing was launched: the outputs still hold their fill values
        assert (xo is None or (xo == -7.0).all()) and (mo is None or (mo == 3).all()), kw
    # the host wrapper raises the library's message
    with pytest.raises(_lib.CwmHipError, match="min"):
        perturbation.multi_shift_rows(x, pts, None, np.array([[[32, 0], [0, 0]]]), 8, 1)
    with pytest.raises(_lib.CwmHipError, match="K=9"):
        perturbation.MultiShiftPatchesAndMask((1, 8, 8))(x, torch.ones(1, 32, 9, dtype=torch.bool, device="cuda"), None, (1, 0))
    assert lib.cwm_version().decode().startswith("cwm_hip 0.10.")
