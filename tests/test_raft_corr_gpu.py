"""RAFT's on-the-fly correlation on the GPU (`fmap_pool_kernel` / `corr_lookup_on_the_fly_kernel` of csrc/raft_kernels.hip, the `corr` option of
csrc/raft_model.hip, `cwm_raft_set_corr` / `cwm_raft_workspace_bytes` / `cwm_raft_corr_lookup_on_the_fly`, `RAFT.set_corr`): the stand-alone lookup
against the torch restatement of `CorrBlock` and against the all-pairs lookup, its operand form, the committed goldens end to end with
`corr="on_the_fly"`, the fast mode, one handle switched back and forth, the workspace, and the error paths.

Bounds.  None is new: the lookup keeps `1e-4 * max(1, max |ref|)` of tests/test_raft_gpu.py::test_corr_lookup_kernel_vs_restatement, the flows TOL_24 = 1e-2 px
and TOL_1 = 5e-3 px, the keypoint maps TOL_MAP = 1e-3 times max(1, max |map|), the fast mode the three rules of tests/test_raft_fast_gpu.py::check_fast with
the bounds stored in raft_fast_224_b2.npz.  Pooling is linear, so "pool fmap2, then dot" is "dot, then pool" up to fp32 summation order: the two lookups
were found to differ by 5e-6 on values up to 3.4 on the CPU, and the reference with an fp32 restatement of the on-the-fly lookup reproduces these goldens
to 6e-6 px.  The workspace bound is the issue's: the pyramid is gone and at most one more copy of fmap2's levels has appeared.
Every measured maximum is printed (run with -s) and recorded in DESIGN.md §8.12.  Measured on an MI355X: lookup vs the restatement 8.9e-6 (2x20x17, bound
3.4e-4) and 1.2e-5 (1x17x19, bound 3.0e-4), vs the all-pairs lookup 1.9e-6 / 1.7e-6; 136x152 9.0e-5 px at 24 iterations and 6.4e-6 px at 1; 128x160 T=3 9.5e-5 /
7.6e-5 px; 224_b2 1.21e-4 px; warm 136x152 3.6e-5 px (up) / 4.3e-6 px (low); the list 3.6e-5 px (flows) / 8.9e-5 (keypoint maps, bound 1.1e-2); keypoint
128x160 9.7e-5 / 1.10e-4 (bound 1.22e-2); fast mode 0.0696 max / 0.0166 mean px vs the fp32 reference (bounds 0.135 / 0.0249), 0.0196 vs the emulation
(< 0.0676); on the fly vs all-pairs on one handle 7.7e-6 px; workspace at 256x384 211,292,160 -> 199,274,496 bytes (bound 200,847,360)."""
import ctypes

import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import _lib, synthetic as S
from counterfactualworldmodels_amd.raft import RAFT, _args
from gpu_utils import new_operand
from test_keypoint_raft_gpu import TOL_MAP  # 1e-3, times max(1, max |map|)
from test_raft_fast_gpu import check_fast
from test_raft_gpu import TOL_1, TOL_24, check, frames, golden, lookup_restated
from test_raft_kernels_gpu import MODES, check_operand

pytestmark = pytest.mark.gpu
OTF = "on_the_fly"


def build(seed, corr=OTF, multiframe=True, output_dim=None, mode="parity"):
    m = RAFT(_args(output_dim=output_dim, multiframe=multiframe, corr=corr, mixed_precision=(mode == "fast")))
    assert m.corr == corr and m.mode == mode
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(seed, output_dim=output_dim).items()})
    return m.cuda().eval()


def check_map(name, got, want):
    check(name, got, want, TOL_MAP * max(1.0, float(np.abs(want).max())))


# ---- 1, 2: the stand-alone lookup and its operand form ---------------------------------------------------------------------------------------
def lookup_case(P, h, w, seed):
    """The recipe of tests/test_raft_gpu.py::test_corr_lookup_kernel_vs_restatement: fractional coordinates up to 4.5 pixels off the grid (partly outside
    the maps) and one far outside every level."""
    g = torch.Generator().manual_seed(seed)
    f1 = torch.randn(P, h, w, 256, generator=g).cuda()
    f2 = torch.randn(P, h, w, 256, generator=g).cuda()
    base = torch.stack(torch.meshgrid(torch.arange(w, dtype=torch.float32), torch.arange(h, dtype=torch.float32), indexing="xy"), -1)
    coords = (base.unsqueeze(0) + 9.0 * (torch.rand(P, h, w, 2, generator=g) - 0.5)).cuda()
    coords[0, 0, 0] = torch.tensor([-30.0, 50.0])
    return f1, f2, coords


@pytest.fixture(scope="module")
def lookups():
    """name -> (P, h, w, f1, f2, coords, the restatement, the all-pairs lookup): 2 x 20 x 17 with seed 3 are that test's own inputs; 1 x 17 x 19 is an odd
    grid whose floor-pooled levels are 17/8/4/2 x 19/9/4/2."""
    lib = _lib.get_lib()
    out = {}
    for name, (P, h, w, seed) in {"2x20x17": (2, 20, 17, 3), "1x17x19": (1, 17, 19, 5)}.items():
        f1, f2, coords = lookup_case(P, h, w, seed)
        all_pairs = torch.empty(P, h, w, 324, device="cuda")
        _lib.check(lib.cwm_raft_corr_lookup(f1.data_ptr(), f2.data_ptr(), coords.data_ptr(), P, h, w, all_pairs.data_ptr(), None))
        out[name] = (P, h, w, f1, f2, coords, lookup_restated(f1, f2, coords), all_pairs)
    return out


@pytest.mark.parametrize("name", ["2x20x17", "1x17x19"])
def test_on_the_fly_lookup_vs_restatement_and_all_pairs_lookup(lookups, name):
    lib = _lib.get_lib()
    P, h, w, f1, f2, coords, ref, all_pairs = lookups[name]
    buf = torch.full((P * h * w * 324 + 64,), -77.0, device="cuda")
    out = buf[:P * h * w * 324].view(P, h, w, 324)
    _lib.check(lib.cwm_raft_corr_lookup_on_the_fly(f1.data_ptr(), f2.data_ptr(), coords.data_ptr(), P, h, w, out.data_ptr(), None))
    bound = 1e-4 * max(1.0, ref.abs().max().item())
    err, err_ap = (out - ref).abs().max().item(), (out - all_pairs).abs().max().item()
    print(f"[on-the-fly lookup {name}] max-abs vs restatement {err:.3e}, vs the all-pairs lookup {err_ap:.3e} (bound {bound:.3e}, values up to "
          f"{ref.abs().max().item():.2f}, zeros {(ref == 0).float().mean().item():.3f})")
    assert torch.isfinite(out).all() and torch.all(buf[P * h * w * 324:] == -77.0)
    assert err <= bound
    assert err_ap <= bound
    assert (ref == 0).any()  # the reference reaches the zero padding
    assert torch.all(out[0, 0, 0] == 0)  # the row whose windows lie outside every level
    again = torch.empty_like(out)
    _lib.check(lib.cwm_raft_corr_lookup_on_the_fly(f1.data_ptr(), f2.data_ptr(), coords.data_ptr(), P, h, w, again.data_ptr(), None))
    assert torch.equal(again, out)  # a fixed summation order


@pytest.mark.parametrize("mode", list(MODES))
def test_on_the_fly_operand_equals_its_fp32_lookup(lookups, mode):
    """tests/test_raft_kernels_gpu.py::test_lookup_operand_equals_the_fp32_lookup for the on-the-fly kernel: the operand convc1 reads holds the fp32
    form's values, fast bitwise after one bf16 rounding, parity within 2^-16 |v|; features 324 .. 383 are 0."""
    dev = _lib.get_dev_lib()
    planes = MODES[mode][1]
    for name, (P, h, w, f1, f2, coords, _, _) in lookups.items():
        M = P * h * w
        out = torch.empty(M, 324, device="cuda")
        _lib.check(dev.cwm_raft_corr_lookup_on_the_fly(f1.data_ptr(), f2.data_ptr(), coords.data_ptr(), P, h, w, out.data_ptr(), None), dev)
        A = new_operand(M, 384, planes)
        _lib.check(dev.cwm_dev_raft_corr_lookup_on_the_fly_operand(f1.data_ptr(), f2.data_ptr(), coords.data_ptr(), P, h, w, MODES[mode][0], A.data_ptr(),
                                                                   None), dev)
        ref = out.cpu().double()
        assert (ref == 0).any() and ref.abs().max() > 1
        check_operand("on-the-fly lookup " + name, A, ref, mode, arithmetic=False)


# ---- 3: the committed goldens, end to end ----------------------------------------------------------------------------------------------------
def test_136x152_b2_odd_grid_vs_reference():
    g = golden("raft_136x152_b2")
    m = build(int(g["seed"]))
    x = frames(2, 136, 152, int(g["frames_seed"]), shift=tuple(int(v) for v in g["shift"]))
    check("on-the-fly 136x152 it24", m(x, iters=24).cpu().numpy(), g["flow"], TOL_24)
    check("on-the-fly 136x152 it1", m(x, iters=1).cpu().numpy(), g["flow_it1"], TOL_1)


def test_128x160_t3_forward_and_backward_vs_reference():
    g = golden("raft_128x160_t3")
    m = build(int(g["seed"]))
    x = frames(1, 128, 160, int(g["frames_seed"]), shift=tuple(int(v) for v in g["shift"]), frames=3)
    check("on-the-fly 128x160 fwd", m(x, iters=24).cpu().numpy(), g["flow_fwd"], TOL_24)
    check("on-the-fly 128x160 bwd", m(x, iters=24, backward=True).cpu().numpy(), g["flow_bwd"], TOL_24)


def test_224_b2_vs_reference():
    g = golden("raft_224_b2")
    m = build(int(g["seed"]))
    check("on-the-fly 224_b2", m(frames(2, 224, 224, int(g["frames_seed"])), iters=int(g["iters"])).cpu().numpy(), g["flow"], TOL_24)


def test_two_image_call_with_init_vs_reference():
    g = golden("raft_warm_136x152_b2")
    m = build(int(g["seed"]), multiframe=False)
    x = frames(2, 136, 152, int(g["frames_seed"]), shift=tuple(int(v) for v in g["shift"])) * 255.0
    low, up = m(x[:, 0], x[:, 1], iters=int(g["iters"]), flow_init=torch.from_numpy(g["init"]).cuda(), test_mode=True)
    check("on-the-fly 136x152 warm up", up.cpu().numpy(), g["up"], TOL_24)
    check("on-the-fly 136x152 warm low", low.cpu().numpy(), g["low"], TOL_24)


def test_list_with_init_vs_reference():
    g = golden("raft_warm_list_128")
    n = int(g["iters"])
    x = frames(1, 128, 128, int(g["frames_seed"])) * 255.0
    x1, x2, init = x[:, 0].contiguous(), x[:, 1].contiguous(), torch.from_numpy(g["init"]).cuda()
    preds = build(int(g["seed"]), multiframe=False)(x1, x2, iters=n, flow_init=init, test_mode=False)
    assert isinstance(preds, list) and len(preds) == n
    for k in range(n):
        check("on-the-fly 128 list flow %d" % k, preds[k].cpu().numpy(), g["preds"][k], TOL_24)
    maps = build(int(g["seed"]), multiframe=False, output_dim=1)(x1, x2, iters=n, flow_init=init, test_mode=False)
    assert isinstance(maps, list) and len(maps) == n
    for k in range(n):
        check("on-the-fly 128 list keypoint map %d" % k, maps[k].cpu().numpy(), g["kp_preds"][k], TOL_MAP * float(np.abs(g["kp_preds"][k]).max()))


def test_keypoint_head_128x160_t3_vs_reference():
    g = golden("raft_keypoint_128x160_t3")
    m = build(int(g["seed"]), output_dim=1)
    x = frames(1, 128, 160, int(g["frames_seed"]), shift=tuple(int(v) for v in g["shift"]), frames=3)
    yf, yb = m(x, iters=24), m(x, iters=24, backward=True)
    assert yf.shape == yb.shape == (1, 2, 1, 128, 160)
    check_map("on-the-fly keypoint 128x160 fwd", yf.cpu().numpy(), g["map_fwd"])
    check_map("on-the-fly keypoint 128x160 bwd", yb.cpu().numpy(), g["map_bwd"])


# ---- 4: fast mode ------------------------------------------------------------------------------------------------------------------------------
def test_224_b2_fast_flow_vs_reference_and_emulation():
    g, f = golden("raft_224_b2"), golden("raft_fast_224_b2")
    m = build(int(f["seed"]), mode="fast")
    y = m(frames(2, 224, 224, int(f["frames_seed"])), iters=int(f["iters"])).cpu().numpy()
    check_fast("on-the-fly 224_b2 flow", y, g["flow"], f["flow_emul"], float(f["err_max"]), float(f["err_mean"]))


# ---- 5: one handle, switched ---------------------------------------------------------------------------------------------------------------------
def test_one_handle_switched_there_and_back():
    x = frames(2, 136, 152, 23, shift=(3, -2))
    fresh = build(4, corr="all_pairs")(x, iters=6)
    m = build(4, corr="all_pairs")
    before = m(x, iters=6)
    ws_all_pairs = m.workspace_bytes()
    otf1 = m.set_corr(OTF)(x, iters=6)
    ws_on_the_fly = m.workspace_bytes()
    otf2 = m(x, iters=6)
    rows = [m(x[b:b + 1].clone(), iters=6) for b in range(2)]
    after = m.set_corr("all_pairs")(x, iters=6)
    diff = (otf1 - before).abs().max().item()
    row_diff = max((otf1[b:b + 1] - rows[b]).abs().max().item() for b in range(2))
    print(f"[switch] on-the-fly vs all-pairs on one handle: max-abs {diff:.3e} px; batch 2 vs two batch-1 forwards (on the fly): max-abs {row_diff:.3e} px; "
          f"workspace {ws_all_pairs} -> {ws_on_the_fly} -> {m.workspace_bytes()} bytes")
    assert torch.equal(before, fresh) and torch.equal(after, fresh)  # all-pairs before and after on-the-fly forwards: a fresh handle's flow
    assert torch.equal(otf1, otf2)
    assert torch.equal(otf1, build(4)(x, iters=6))  # ... and the on-the-fly flow does not depend on the handle's history either
    assert all(torch.equal(otf1[b:b + 1], rows[b]) for b in range(2))
    assert not torch.equal(otf1, before)  # the option is not ignored
    assert diff <= TOL_24
    assert ws_on_the_fly < ws_all_pairs == m.workspace_bytes()  # switching re-plans the workspace, both ways


# ---- 6: the workspace ------------------------------------------------------------------------------------------------------------------------------
def test_workspace_drops_the_pyramid():
    H, W, P = 256, 384, 1
    x = frames(1, H, W, 7)
    ws = {}
    for corr in ("all_pairs", OTF):
        m = build(0, corr=corr)
        assert m.workspace_bytes() == 0
        m(x, iters=1)
        ws[corr] = m.workspace_bytes()
    sides = [((H // 8) >> l, (W // 8) >> l) for l in range(4)]
    levels = sum(h * w for h, w in sides)
    M = P * sides[0][0] * sides[0][1]
    assert (M, levels) == (1536, 2040)
    bound = ws["all_pairs"] - 4 * M * levels + 4 * 256 * P * levels
    print(f"[workspace 256x384] all-pairs {ws['all_pairs']} bytes, on-the-fly {ws[OTF]} bytes (bound {bound}; the pyramid is {4 * M * levels} bytes, "
          f"fmap2's levels {4 * 256 * P * levels})")
    assert 0 < ws[OTF] <= bound


# ---- 7: errors ---------------------------------------------------------------------------------------------------------------------------------------
def _raw_args(x, out, iters):
    a = _lib.new_raft_forward_args()
    a.image1_dev, a.image2_dev = x.data_ptr(), x.data_ptr() + x.stride(1) * 4
    a.image1_stride_b = a.image2_stride_b = x.stride(0)
    a.image1_stride_c = a.image2_stride_c = x.stride(2)
    a.batch, a.pairs, a.height, a.width, a.input_scale, a.iters = x.shape[0], 1, x.shape[-2], x.shape[-1], 255.0, iters
    a.flow_dev = out.data_ptr()
    a.flow_stride_b, a.flow_stride_c = out.stride(0), out.stride(2)
    return a


def test_invalid_corr_values_leave_the_handle_as_it_was():
    lib = _lib.get_lib()
    x = frames(1, 128, 160, 31)
    m = build(5)
    want = m(x, iters=3)
    all_pairs = build(5, corr="all_pairs")(x, iters=3)
    assert not torch.equal(want, all_pairs)

    def raw():
        out = torch.full((1, 1, 2, 128, 160), -9.0, device="cuda")
        rc = lib.cwm_raft_forward(m._handle, ctypes.byref(_raw_args(x, out, 3)))
        torch.cuda.synchronize()
        return rc, out

    for bad in (2, -1):
        assert lib.cwm_raft_set_corr(m._handle, bad) == _lib.ERR_INVALID and b"cwm_raft_set_corr" in lib.cwm_last_error()
        rc, y = raw()
        assert rc == 0 and torch.equal(y, want), bad  # still on the fly
    assert lib.cwm_raft_set_corr(m._handle, _lib.RAFT_CORR_ALL_PAIRS) == 0
    rc, y = raw()
    assert rc == 0 and torch.equal(y, all_pairs)
    n = ctypes.c_uint64()
    assert lib.cwm_raft_workspace_bytes(m._handle, None) == _lib.ERR_INVALID
    assert lib.cwm_raft_workspace_bytes(m._handle, ctypes.byref(n)) == 0 and n.value == m.workspace_bytes() > 0


def test_stand_alone_call_refuses_null_arguments(lookups):
    lib = _lib.get_lib()
    P, h, w, f1, f2, coords, _, _ = lookups["1x17x19"]
    out = torch.full((P, h, w, 324), -5.0, device="cuda")
    good = [f1.data_ptr(), f2.data_ptr(), coords.data_ptr(), P, h, w, out.data_ptr(), None]
    for i in (0, 1, 2, 6):
        args = list(good)
        args[i] = None
        assert lib.cwm_raft_corr_lookup_on_the_fly(*args) == _lib.ERR_INVALID, i
        assert b"cwm_raft_corr_lookup_on_the_fly" in lib.cwm_last_error()
    for i, v in ((3, 0), (4, 7), (5, 7)):  # the checks of cwm_raft_corr_lookup: P > 0, h8 >= 8, w8 >= 8
        args = list(good)
        args[i] = v
        assert lib.cwm_raft_corr_lookup_on_the_fly(*args) == _lib.ERR_INVALID, i
    torch.cuda.synchronize()
    assert torch.all(out == -5.0)
