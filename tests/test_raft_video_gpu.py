"""RAFT's video warm start on the GPU: `forward_interpolate` (csrc/raft_kernels.hip `forward_interpolate_kernel`, `cwm_raft_forward_interpolate`) and the
chain `RAFT.forward(x, warm_start=True)` drives with it (raft.py).

What is compared with what.  The kernel against scipy, bit for bit on every element: the fields of tests/golden/make_golden_raft_video.py, which have
no ties (their maker asserted a gap >= 1e-9 between the best and the second-best squared distance; the kernel's distances are the same float64
expression).  What scipy does not define -- ties, no valid source -- and the validity rule's edges against tests/raft_video_restatement.py, bit for bit:
the maker asserted that restatement equal to scipy on every stored field.  The chain against its own composition (two-image calls fed
`forward_interpolate` of the previous low-resolution flow), bit for bit.  The reference's chain pair by pair with the golden's init given to the GPU
(teacher-forced) within 1e-2 px, TOL_24 of tests/test_raft_gpu.py; the free-running chain's distance from the reference's is printed, not asserted:
the nearest-source choice is discontinuous, so a 1e-4 px difference in a low-resolution flow may legitimately pick another source."""
import ctypes
import os

import numpy as np
import pytest
import torch

import raft_video_restatement as R
from counterfactualworldmodels_amd import _lib, synthetic as S
from counterfactualworldmodels_amd import raft as raft_mod
from counterfactualworldmodels_amd.raft import RAFT, _args

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_24 = 1e-2      # px, max-abs (tests/test_raft_gpu.py)
WARM_MIN_PX = 0.5  # the margin tests/golden/make_golden_raft_video.py asserted on the reference
SENTINEL = -7.0


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def build(seed, multiframe=True, output_dim=None):
    m = RAFT(_args(output_dim=output_dim, multiframe=multiframe))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(seed, output_dim=output_dim).items()})
    return m.cuda().eval()


def finterp(f):
    """numpy field(s) -> the device's forward_interpolate as numpy"""
    return raft_mod.forward_interpolate(torch.from_numpy(np.ascontiguousarray(f)).cuda()).cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- 1: the kernel against scipy ----------------------------------------------------------------------------------------------------------
def test_kernel_vs_scipy_golden_fields():
    g = golden("raft_finterp_fields")
    names = [str(n) for n in g["names"]]
    assert sorted(names) == ["16x16_a1", "16x16_a6", "16x16_t", "17x19_a3", "28x28_a3", "40x56_a8"]
    for n in names:  # each alone, [2,h,w]; 40x56 = 2240 sources is three LDS chunks and nine workgroups, 17x19 has odd sides, 16x16 is RAFT's smallest grid
        got = finterp(g[n + "_in"])
        assert same_bits(got, g[n + "_out"]), (n, int((got != g[n + "_out"]).sum()))
    trio = ["16x16_a1", "16x16_a6", "16x16_t"]
    want = np.stack([g[n + "_out"] for n in trio])
    fields = np.stack([g[n + "_in"] for n in trio])
    assert same_bits(finterp(fields), want)  # one P = 3 call
    # a non-contiguous view, read in place: rows contiguous, arbitrary field and channel strides, NaN between the planes
    flat = torch.full((4096,), float("nan"), device="cuda")
    view = torch.as_strided(flat, (3, 2, 16, 16), (1100, 300, 16, 1), 7)
    view.copy_(torch.from_numpy(fields))
    assert not view.is_contiguous()
    assert same_bits(raft_mod.forward_interpolate(view).cpu().numpy(), want)
    # the same view through the C entry point with a negative field stride: the fields come out in reversed order
    out = torch.full((3, 2, 16, 16), SENTINEL, device="cuda")
    _lib.check(_lib.get_lib().cwm_raft_forward_interpolate(view[2].data_ptr(), -1100, 300, 3, 16, 16, out.data_ptr(), None))
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), want[::-1])
    # half and double inputs are cast to fp32 first
    a = torch.from_numpy(g["17x19_a3_in"]).cuda()
    assert same_bits(raft_mod.forward_interpolate(a.double()).cpu().numpy(), g["17x19_a3_out"])
    assert same_bits(raft_mod.forward_interpolate(a.half()).cpu().numpy(), R.forward_interpolate(a.half().float().cpu().numpy()))


def test_kernel_vs_scipy_on_the_chain_fields():
    """the low-resolution flows the reference's chain interpolated (16 x 20, a few tenths of a pixel: most sources land next to their own pixel)"""
    g = golden("raft_video_128x160_t4")
    for d in ("fwd", "bwd"):
        for k in (0, 1):
            assert same_bits(finterp(g["%s_low_%d" % (d, k)]), g["%s_init_%d" % (d, k + 1)]), (d, k)


# ---- 2: the rules scipy leaves open, against the restatement ---------------------------------------------------------------------------------
def rule_fields():
    rng = np.random.Generator(np.random.PCG64(5))
    out = {}
    for h, w in ((16, 16), (17, 19)):  # integer-valued flows: landing points on the grid, exact ties
        out["ties_%dx%d" % (h, w)] = rng.integers(-3, 4, (2, h, w)).astype(np.float32)
    # column 0 with dx = 0 and row 0 with dy = 0 land ON the open boundary: invalid.  Were they valid (a `>=`), each would land at distance < 0.5 of its
    # own grid point and win it with its own value, and those values are distinct from every other pixel's
    f = rng.uniform(-0.4, 0.4, (2, 12, 20)).astype(np.float32)
    f[0, :, 0] = 0.0
    f[1, 0, :] = 0.0
    f[1, :, 0] = np.linspace(0.11, 0.39, 12, dtype=np.float32)
    f[0, 0, :] = np.linspace(0.12, 0.38, 20, dtype=np.float32)
    f[:, 0, 0] = 0.0
    out["open_boundary"] = f
    f = rng.uniform(-0.4, 0.4, (2, 16, 16)).astype(np.float32)
    f[0, 5, 14] = 2.0    # x1 = 16 = w8 exactly
    f[1, 13, 3] = 3.0    # y1 = 16 = h8 exactly
    out["far_boundary"] = f
    f = rng.uniform(-2.0, 2.0, (2, 16, 18)).astype(np.float32)
    f[0, 3, 4], f[1, 7, 7], f[0, 9, 2], f[1, 11, 12], f[0, 12, 12] = np.nan, np.inf, -np.inf, np.nan, np.inf
    out["nonfinite"] = f
    f = np.full((2, 16, 16), 1e6, dtype=np.float32)
    f[:, 9, 4] = (0.25, -1.5)
    out["one_valid"] = f
    out["none_valid"] = np.full((2, 16, 17), -1e6, dtype=np.float32)
    out["all_nan"] = np.full((2, 3, 5), np.nan, dtype=np.float32)
    f = rng.uniform(-1.5, 1.5, (2, 1, 7)).astype(np.float32)
    f[1] = np.array([0.5, 0.25, 0.0, -0.5, 0.75, 1.0, 0.125], dtype=np.float32).reshape(1, 7)
    out["1x7"] = f
    out["1x1_valid"] = np.array([0.3, 0.6], dtype=np.float32).reshape(2, 1, 1)
    out["1x1_zero_flow"] = np.zeros((2, 1, 1), dtype=np.float32)
    return out


def test_rules_vs_restatement():
    fields = rule_fields()
    # the cases are what they claim to be, on the restatement
    for n in ("ties_16x16", "ties_17x19"):
        assert R.min_gap(fields[n]) == 0.0
    f = fields["open_boundary"]
    valid = R.landing_points(f)[2].reshape(12, 20)
    assert not valid[:, 0].any() and not valid[0, :].any() and valid[1:, 1:].all()
    wrong = f.copy()  # what a `>=` would give: the boundary sources nudged inside win their own grid points
    wrong[0, :, 0] = 1e-6
    wrong[1, 0, :] = 1e-6
    assert not np.array_equal(R.forward_interpolate(wrong)[:, 1:, 0], R.forward_interpolate(f)[:, 1:, 0])
    valid = R.landing_points(fields["far_boundary"])[2].reshape(16, 16)
    assert not valid[5, 14] and not valid[13, 3] and valid[1:-1, 1:-1].sum() == 14 * 14 - 2
    assert R.landing_points(fields["nonfinite"])[2].sum() < 16 * 18 - 4
    assert R.landing_points(fields["one_valid"])[2].sum() == 1
    valid = R.landing_points(fields["1x7"])[2]
    assert valid.any() and not valid[[2, 3, 5]].any()  # y1 = 0, -0.5 and 1 = h8 are outside (0, 1)
    for n, f in fields.items():
        want = R.forward_interpolate(f)
        assert np.isfinite(want).all(), n
        got = finterp(f)
        assert same_bits(got, want), (n, int((got != want).sum()))
    assert (finterp(fields["none_valid"]) == 0).all() and (finterp(fields["all_nan"]) == 0).all() and (finterp(fields["1x1_zero_flow"]) == 0).all()
    one = finterp(fields["one_valid"])
    assert (one[0] == 0.25).all() and (one[1] == -1.5).all()
    assert same_bits(finterp(fields["1x1_valid"]), fields["1x1_valid"])


# ---- 3: the chain is the composition ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def movie():
    """B = 2, T = 4, 128 x 160 frames in [0, 255], a multi-frame model reading them with input scale 1 and the two-image model of the same weights (the
    inputs of the two paths are then the same numbers), and a [2,2,16,20] init."""
    mf = build(14)
    mf.scale_inputs = False
    x = torch.from_numpy(S.raft_frames(2, 128, 160, 41, shift=(2, -3), frames=4)).cuda() * 255.0
    gen = torch.Generator().manual_seed(11)
    init = (4.0 * torch.rand(2, 2, 16, 20, generator=gen) - 2.0).cuda()
    return {"mf": mf, "m2": build(14, multiframe=False), "x": x, "init": init}


def composed(m2, x, backward, flow_init=None, iters=3):
    """the chain written out with two-image calls: [B,T-1,C,H,W] in the multi-frame call's order"""
    T = x.shape[1]
    ups, init = [None] * (T - 1), flow_init
    for k in range(T - 1):
        t = T - 2 - k if backward else k
        a, b = (x[:, t + 1], x[:, t]) if backward else (x[:, t], x[:, t + 1])
        low, up = m2(a, b, iters=iters, flow_init=init)
        ups[T - 2 - t if backward else t] = up
        init = raft_mod.forward_interpolate(low)
    return torch.stack(ups, dim=1)


def test_chain_is_the_composition(movie):
    mf, m2, x, init = movie["mf"], movie["m2"], movie["x"], movie["init"]
    cold = mf(x, iters=3)
    for backward in (False, True):
        y = mf(x, iters=3, backward=backward, warm_start=True)
        assert y.shape == (2, 3, 2, 128, 160) and torch.equal(y, composed(m2, x, backward))
        yi = mf(x, iters=3, backward=backward, warm_start=True, flow_init=init)
        assert torch.equal(yi, composed(m2, x, backward, flow_init=init)) and not torch.equal(yi, y)
        # a given init starts the first pair of the chain only.  (Against the call that batches all pairs the first pair is compared within the parity
        # bound, not bitwise: another row count may choose another GEMM tile.)
        first, every = 0, mf(x, iters=3, backward=backward, flow_init=init)  # (backward: the chain's first pair is the last one, stored at index 0)
        assert (yi[:, first] - every[:, first]).abs().max().item() <= TOL_24
        assert min((yi[:, k] - every[:, k]).abs().max().item() for k in range(3) if k != first) > 10 * TOL_24
        one = mf(x, iters=3, backward=backward, warm_start=True, flow_init=init[:1])  # [1,2,h8,w8]: one field for all batch rows of the first pair
        assert torch.equal(one[0], yi[0]) and not torch.equal(one[1], yi[1])
    assert torch.equal(mf(x, iters=3, warm_start=False), cold) and torch.equal(mf(x, iters=3), cold)
    assert (mf(x, iters=3, warm_start=True)[:, 0] - cold[:, 0]).abs().max().item() <= TOL_24  # without an init the first pair is cold
    x2 = x[:, :2]
    assert torch.equal(mf(x2, iters=3, warm_start=True), mf(x2, iters=3))
    assert torch.equal(mf(x2, iters=3, warm_start=True, flow_init=init, backward=True), mf(x2, iters=3, flow_init=init, backward=True))
    assert torch.equal(mf(x[:, :1], iters=3, warm_start=True), mf(x[:, :1], iters=3))
    mf.set_iters(3)  # self.iters overrides the call's, in the chain as elsewhere
    try:
        assert torch.equal(mf(x, iters=7, warm_start=True), composed(m2, x, False))
    finally:
        mf.set_iters(None)
    assert torch.equal(mf(x, iters=3, warm_start=True, test_mode=False), composed(m2, x, False))


def test_keypoint_model_runs_the_same_chain(movie):
    x = movie["x"][:1]
    kf = build(5, output_dim=1)
    kf.scale_inputs = False
    y = kf(x, iters=2, warm_start=True)
    assert y.shape == (1, 3, 1, 128, 160)
    assert torch.equal(y, composed(build(5, multiframe=False, output_dim=1), x, False, iters=2))
    assert not torch.equal(y[:, 1:], kf(x, iters=2)[:, 1:])


# ---- 4, 5: against the reference ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_case():
    g = golden("raft_video_128x160_t4")
    x = torch.from_numpy(S.raft_frames(1, 128, 160, int(g["frames_seed"]), shift=tuple(int(v) for v in g["shift"]), frames=4)).cuda()
    return {"g": g, "x": x, "mf": build(int(g["seed"])), "m2": build(int(g["seed"]), multiframe=False), "iters": int(g["iters"])}


def test_warm_start_is_not_ignored(ref_case):
    """Fails on a build that swallows the keyword: pairs after the first of a chain differ from the cold call by the margin the maker proved."""
    g, x, mf, n = ref_case["g"], ref_case["x"], ref_case["mf"], ref_case["iters"]
    for d, backward in (("fwd", False), ("bwd", True)):
        assert (g["warm_vs_cold_" + d][1:] >= WARM_MIN_PX).all()
        cold = mf(x, iters=n, backward=backward)
        warm = mf(x, iters=n, backward=backward, warm_start=True)
        for k in range(3):  # chain step k is stored at index k in both directions: the backward chain starts at the last pair, which comes first
            diff = (warm[:, k] - cold[:, k]).abs().max().item()
            print("[warm vs cold %s step %d] %.3f px (reference %.3f px)" % (d, k, diff, float(g["warm_vs_cold_" + d][k])))
            assert diff <= TOL_24 if k == 0 else diff >= WARM_MIN_PX, (d, k, diff)  # the first pair of a chain is cold


def test_chain_vs_reference_teacher_forced(ref_case):
    g, x, mf, m2, n = ref_case["g"], ref_case["x"], ref_case["mf"], ref_case["m2"], ref_case["iters"]
    x255 = x * 255.0
    for d, backward in (("fwd", False), ("bwd", True)):
        free = mf(x, iters=n, backward=backward, warm_start=True)
        for k in range(3):
            t = 2 - k if backward else k
            a, b = (x255[:, t + 1], x255[:, t]) if backward else (x255[:, t], x255[:, t + 1])
            init = None if k == 0 else torch.from_numpy(g["%s_init_%d" % (d, k)]).cuda()  # step 0 is cold; later steps take the REFERENCE's init
            low, up = m2(a, b, iters=n, flow_init=init)
            err_low = float(np.abs(low.cpu().numpy() - g["%s_low_%d" % (d, k)]).max())
            print("[%s step %d] low max-abs %.3e (bound %.1e, reference fp32 vs float64 %.3e)" % (d, k, err_low, TOL_24, float(g["drift_" + d][k])))
            assert err_low <= TOL_24, (d, k, err_low)
            if not backward:
                err_up = float(np.abs(up.cpu().numpy() - g["fwd_up_%d" % k]).max())
                dev = float(np.abs(free[:, k].cpu().numpy() - g["fwd_up_%d" % k]).max())
                print("[fwd step %d] up max-abs %.3e (bound %.1e); free-running chain vs the reference's chain %.3e px (not asserted)" % (k, err_up, TOL_24, dev))
                assert err_up <= TOL_24, (k, err_up)


# ---- 6: refusals are errors, not faults ------------------------------------------------------------------------------------------------------
def test_refusals_then_a_correct_call():
    lib = _lib.get_lib()
    g = golden("raft_finterp_fields")
    with pytest.raises(RuntimeError, match=r"forward_interpolate needs a CUDA/HIP tensor \(no CPU fallback\); got cpu"):
        raft_mod.forward_interpolate(torch.zeros(2, 16, 16))
    for bad in (torch.zeros(3, 16, 16), torch.zeros(4, 3, 16, 16), torch.zeros(16, 16), torch.zeros(1, 1, 2, 16, 16), torch.zeros(2, 0, 16)):
        with pytest.raises(RuntimeError, match=r"forward_interpolate expects.*%s" % str(tuple(bad.shape)).replace("(", r"\(").replace(")", r"\)")):
            raft_mod.forward_interpolate(bad.cuda())
    with pytest.raises(RuntimeError, match="floating-point"):
        raft_mod.forward_interpolate(torch.zeros(2, 16, 16, dtype=torch.int32).cuda())
    buf = torch.full((4, 2, 16, 16), SENTINEL, device="cuda")
    buf[:2].copy_(torch.from_numpy(np.stack([g["16x16_a1_in"], g["16x16_a6_in"]])))
    fn = lib.cwm_raft_forward_interpolate
    N = 256
    overlapping = [(buf.data_ptr(), 2 * N, N, 2, buf.data_ptr()),                # in place
                   (buf.data_ptr(), 2 * N, N, 2, buf.data_ptr() + 4 * (4 * N - 1)),  # out begins on the last element read
                   (buf.data_ptr() + 4 * 2 * N, 2 * N, N, 2, buf.data_ptr() + 4),    # out ends one element into what is read
                   (buf[1].data_ptr(), -2 * N, N, 2, buf.data_ptr())]                # a negative field stride reaches back over out
    for src, sp, sc, P, dst in overlapping:
        assert fn(src, sp, sc, P, 16, 16, dst, None) == _lib.ERR_INVALID and b"overlaps" in lib.cwm_last_error()
    for args, word in (((None, 2 * N, N, 1, 16, 16, buf[2].data_ptr(), None), b"null"), ((buf.data_ptr(), 2 * N, N, 1, 16, 16, None, None), b"null"),
                       ((buf.data_ptr(), 2 * N, N, 0, 16, 16, buf[2].data_ptr(), None), b"bad argument"),
                       ((buf.data_ptr(), 2 * N, N, 1, 0, 16, buf[2].data_ptr(), None), b"bad argument"),
                       ((buf.data_ptr(), 0, 0, 1, 300, 300, buf[2].data_ptr(), None), b"65536")):
        assert fn(*args) == _lib.ERR_INVALID and word in lib.cwm_last_error(), word
    torch.cuda.synchronize()
    assert (buf[2:] == SENTINEL).all() and same_bits(buf[0].cpu().numpy(), g["16x16_a1_in"])  # nothing was written
    # adjacent, not overlapping: accepted, and right
    _lib.check(fn(buf.data_ptr(), 2 * N, N, 2, 16, 16, buf[2].data_ptr(), None))
    torch.cuda.synchronize()
    assert same_bits(buf[2:].cpu().numpy(), np.stack([g["16x16_a1_out"], g["16x16_a6_out"]]))


# ---- 7: determinism ---------------------------------------------------------------------------------------------------------------------------
def test_two_runs_of_the_chain_are_bit_equal(movie):
    mf, x, init = movie["mf"], movie["x"], movie["init"]
    for backward in (False, True):
        a = mf(x, iters=3, backward=backward, warm_start=True, flow_init=init)
        b = mf(x, iters=3, backward=backward, warm_start=True, flow_init=init)
        assert torch.equal(a, b)
