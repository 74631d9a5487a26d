"""Marker counterfactuals without a GPU: `AddMarkers` against what the reference returns (tests/golden/markers.npz, make_golden_markers.py, on the cases of
tests/marker_cases.py), the float64 restatement of the response (tests/response_restatement.py) on cases worked out by hand, the C-ABI binding of
`cwm_token_response` with its argument refusals, the torch statistics of the composed path, and the displacement arithmetic of `predict_perturbation_flow`."""
import ctypes
import os

import numpy as np
import pytest
import torch

import marker_cases as MC
import response_restatement as RR
from counterfactualworldmodels_amd import _lib, perturbation, prediction, segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run_case(name):
    ctor, call = MC.CASES[name]
    call = {k: v for k, v in call.items() if k != "as4"}
    if call.pop("points", False):
        call["perturbation_points"] = torch.from_numpy(MC.points())
    x, mask = torch.from_numpy(MC.frames()), torch.from_numpy(MC.mask())
    x0, m0 = x.clone(), mask.clone()
    xm, mm = perturbation.AddMarkers((1, MC.P, MC.P), **ctor)(x, mask, **call)
    assert torch.equal(x, x0) and torch.equal(mask, m0)  # the arguments are left alone
    return xm, mm


# ---- AddMarkers -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_add_markers_equals_the_reference(name):
    g = np.load(os.path.join(GOLDEN, "markers.npz"))
    xm, mm = run_case(name)
    assert xm.dtype == torch.float32 and mm.dtype == torch.bool
    assert torch.equal(xm, torch.from_numpy(g[name + "_x"])), name
    assert torch.equal(mm, torch.from_numpy(g[name + "_mask"])), name


def test_the_golden_shows_what_it_is_there_for():
    g = np.load(os.path.join(GOLDEN, "markers.npz"))
    x, mask = MC.frames(), MC.mask()
    grid = lambda m: m.reshape(MC.B, *MC.GRID)  # noqa: E731
    assert set(g.files) == {n + s for n in MC.CASES for s in ("_x", "_mask")}
    # neither a list nor random patches: nothing is marked, the mask is returned unchanged
    assert np.array_equal(g["empty_default_x"], x) and np.array_equal(g["empty_default_mask"], mask)
    assert np.array_equal(g["frame_none_empty_x"], x) and np.array_equal(g["frame_none_empty_mask"], mask)
    # frame 0 visible at the marked patches: the mask is returned unchanged, the frames are not
    assert np.array_equal(g["full_fixed_mask"], mask) and not np.array_equal(g["full_fixed_x"], x)
    assert (g["full_fixed_x"][0, 0, :, 4:8, 8:12] == np.array([1, 0, 0], dtype=np.float32)[:, None, None]).all()
    # a marked patch that was masked comes back visible
    assert mask.reshape(MC.B, *MC.GRID)[1, 0, 1, 1] and not grid(g["masked_source_mask"])[1, 0, 1, 1] and not grid(g["masked_source_mask"])[1, 0, 3, 5]
    assert int((g["masked_source_mask"] != mask).sum()) == 2
    # a marker without colour replaces nothing, and still un-masks
    assert np.array_equal(g["black_marker_x"], x) and int((g["black_marker_mask"] != mask).sum()) == 1
    # a cross keeps the image between its arms: patch (0, 0) of row 0 keeps its corners
    cross = g["cross_fixed_x"][0, 0, :, 0:4, 0:4]
    assert np.array_equal(cross[:, 0, 0], x[0, 0, :, 0, 0]) and (cross[:, 1, 0] == np.array([0, 1, 0.5], dtype=np.float32)).all()
    # frame=None marks any frame, and un-masks there; frame=1 counts a 4-entry index from frame 1
    assert not grid(g["frame_none_mask"])[1, 1, 2, 3] and not grid(g["frame_none_mask"])[0, 1, 3, 5] and int((g["frame_none_mask"] != mask).sum()) == 2
    assert not np.array_equal(g["frame_one_x"][:, 1], x[:, 1]) and np.array_equal(g["frame_one_x"][:, 0], x[:, 0])
    assert not grid(g["frame_one_mask"])[1, 1, 1, 2] and not grid(g["frame_one_mask"])[0, 1, 0, 5]
    # random patches: one per row and round, in frame 0 / in any frame
    assert not np.array_equal(g["random_patches_x"][:, 0], x[:, 0]) and np.array_equal(g["random_patches_x"][:, 1], x[:, 1])
    assert not np.array_equal(g["random_patches_any_frame_x"], x)


def test_marker_shapes_and_draw_order():
    M = perturbation.MarkerShape((4, 4))
    assert M("full").tolist() == np.ones((4, 4)).tolist()
    assert M("cross").tolist() == [[0, 1, 1, 0], [1, 1, 1, 1], [1, 1, 1, 1], [0, 1, 1, 0]]
    assert perturbation.MarkerShape((5, 3))("cross").tolist() == [[0, 1, 0], [0, 1, 0], [1, 1, 1], [0, 1, 0], [0, 1, 0]]  # |k - (s - 1) / 2| < 1: one line for an odd size, two for an even
    with pytest.raises(NotImplementedError):
        M("disc")
    # per marker: the shape first, then the colour -- the same stream replayed by hand
    A = perturbation.AddMarkers((1, 4, 4), marker_shapes=["full", "cross"], marker_color=None, seed=5)
    rng = np.random.RandomState(5)
    for _ in range(3):
        shape = rng.choice(["full", "cross"])
        colour = rng.random((3))
        assert np.array_equal(A.sample_marker(), M(shape)[None] * colour[:, None, None])
    assert perturbation.AddMarkers(4).patch_size == (1, 4, 4) and perturbation.AddMarkers((8, 8)).patch_size == (1, 8, 8)


def test_add_markers_refusals():
    x, mask = torch.from_numpy(MC.frames()), torch.from_numpy(MC.mask())
    A = perturbation.AddMarkers((1, MC.P, MC.P))
    with pytest.raises(NotImplementedError):  # a mask on a coarser grid than the patches: the reference's stride branch
        A(x, mask.view(MC.B, MC.T, 4, 6)[:, :, ::2, ::2].reshape(MC.B, -1), patch_idx_list=[[0, 0, 1, 2]])
    with pytest.raises(ValueError):
        A(x, None, patch_idx_list=[[0, 0, 1, 2]])
    with pytest.raises(IndexError):  # frame 0 is the only marked frame: its index is 0 (or -1)
        A(x, mask, patch_idx_list=[[0, 1, 1, 2]])
    with pytest.raises(IndexError):
        A(x, mask, patch_idx_list=[[0, 0, 4, 2]])
    with pytest.raises(AssertionError):
        A(x, mask, patch_idx_list=[[0, 0, 0, 1, 2]])
    with pytest.raises(AssertionError):  # a fixed colour has one entry per channel
        perturbation.AddMarkers((1, MC.P, MC.P), marker_color=[1, 0])(x, mask, patch_idx_list=[[0, 0, 1, 2]])


def test_add_markers_on_other_layouts():
    """frames that are a permuted view, float masks: the same pixels, the mask's own dtype"""
    x, mask = torch.from_numpy(MC.frames()), torch.from_numpy(MC.mask())
    A = perturbation.AddMarkers((1, MC.P, MC.P), marker_shapes=["cross"])
    want_x, want_m = A(x, mask, patch_idx_list=[[1, 0, 2, 2]])
    xv = x.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)
    got_x, got_m = A(xv, mask.float(), patch_idx_list=[[1, 0, 2, 2]])
    assert torch.equal(got_x, want_x) and got_m.dtype == torch.float32 and torch.equal(got_m.bool(), want_m)


def test_paint_markers_one_marker_per_row():
    """what `predict_marker_responses` builds: row k of K copies of a movie with marker k in its own patch -- equal to K calls of the class"""
    x = torch.from_numpy(MC.frames())[:1]
    mask = torch.from_numpy(MC.mask())[:1]
    A = perturbation.AddMarkers((1, MC.P, MC.P), marker_shapes=["full", "cross"], marker_color=None, seed=1)
    Bm = perturbation.AddMarkers((1, MC.P, MC.P), marker_shapes=["full", "cross"], marker_color=None, seed=1)
    where = [(0, 1, 2), (1, 3, 5), (0, 0, 0), (0, 1, 2)]
    markers = A.sample_markers(len(where), x)
    rows = x.expand(len(where), -1, -1, -1, -1).clone()
    idx = torch.tensor(where)
    perturbation.paint_markers(rows, markers, torch.arange(len(where)), idx[:, 0], idx[:, 1], idx[:, 2], (MC.P, MC.P))
    for k, (t, h, w) in enumerate(where):
        one, _ = Bm(x, mask, patch_idx_list=[[0, 0, h, w]], frame=t)
        assert torch.equal(rows[k:k + 1], one), k


# ---- the restatement, on cases worked out by hand -----------------------------------------------------------------------------------------------------------
def hand_case():
    """T = 2, C = 2, 8 x 8, P = 4: four patches per frame; row 0 masks frame 1 but its patch 1, row 1 masks all of frame 1 and patch 0 of frame 0"""
    T, Cc, H, W, P = 2, 2, 8, 8, 4
    mask = torch.zeros((2, 8), dtype=torch.bool)
    mask[0, [4, 6, 7]] = True
    mask[1, [0, 4, 5]] = True  # (three masked tokens in either row, as rows of one batch have)
    y = torch.zeros((2, 3, P, P, Cc))
    ref = torch.zeros((1, 3, P, P, Cc))
    y[0, 1, 2, 3] = torch.tensor([3.0, 4.0])    # row 0, its 2nd masked token = token 6 = frame 1 patch (1, 0), pixel (2, 3) of it: image (6, 3); 9 + 16 = 25
    y[0, 2, 0, 0] = torch.tensor([0.0, 2.0])    # token 7 = patch (1, 1), pixel (0, 0): image (4, 4); 4
    ref[0, 2, 0, 0] = torch.tensor([1.0, 2.0])  # ... against (1, 2): 1 + 0 = 1
    y[1, 0, 1, 1] = torch.tensor([9.0, 9.0])    # row 1, token 0: frame 0 -- not in frame 1
    y[1, 2, 3, 3] = torch.tensor([1.0, 1.0])    # row 1, its 3rd masked token = token 5 = frame 1 patch (0, 1), pixel (3, 3): image (3, 7); against ref 0: 2
    return y.view(2, 3, -1), ref.view(1, 3, -1), mask, (T, Cc, H, W, P)


def test_restatement_by_hand():
    y, ref, mask, (T, Cc, H, W, P) = hand_case()
    r = RR.response(y, ref, mask, T, Cc, H, W, P, 1)
    want = torch.zeros((2, 8, 8), dtype=torch.float64)
    want[0, 6, 3], want[0, 4, 4] = 25.0, 1.0
    want[1, 3, 7] = 2.0
    want[1, 0, 4] = 1.0 + 4.0  # the shared reference's (1, 2) sits in ITS token row 2, which for row 1 is patch (0, 1): pixel (0, 0) of it, image (0, 4); y is 0 there
    assert torch.equal(r, want)
    assert torch.equal(RR.patch_map(r, P), torch.tensor([[[0, 0], [25 / 16, 1 / 16]], [[0, 7 / 16], [0, 0]]], dtype=torch.float64))
    idx, stats = RR.statistics(r)
    assert idx.tolist() == [6 * 8 + 3, 0 * 8 + 4]
    assert stats[0].tolist() == [25.0, 26.0, (25 * 6 + 4) / 26, (25 * 3 + 4) / 26]
    assert stats[1].tolist() == [5.0, 7.0, (2 * 3) / 7, (5 * 4 + 2 * 7) / 7]
    # frame 0: row 0 has nothing masked there, row 1 its token 0
    r0 = RR.response(y, ref, mask, T, Cc, H, W, P, 0)
    idx0, stats0 = RR.statistics(r0)
    assert idx0.tolist() == [0, 1 * 8 + 1] and stats0[0].tolist() == [0.0, 0.0, 0.0, 0.0] and stats0[1].tolist() == [162.0, 162.0, 1.0, 1.0]
    # equal responses: the first; a NaN: the maximum
    tie = torch.zeros((1, 8, 8), dtype=torch.float64)
    tie[0, 5, 1] = tie[0, 2, 6] = 3.0
    assert RR.statistics(tie)[0].tolist() == [2 * 8 + 6]
    tie[0, 7, 0] = float("nan")
    idx, stats = RR.statistics(tie)
    assert idx.tolist() == [56] and bool(stats.isnan().all())
    gap, top = RR.index_gap(want)
    assert gap.tolist() == [24.0, 3.0] and top.tolist() == [25.0, 5.0]


def test_bounds_are_operation_counts():
    assert RR.EPS == 2.0 ** -24 and RR.gamma(1) > RR.EPS
    assert RR.pixel_bound(3) == RR.gamma(5) and RR.map_bound(3, 8) == RR.gamma(3 * 64 + 2) and RR.mass_bound(3, 16, 16) == RR.gamma(3 + 2 + 255)
    assert RR.centroid_bound(3, 16, 16) == RR.gamma((3 + 3 + 255) + 2 * (3 + 2 + 255) + 1)
    # a plain fp32 evaluation, in another order than any kernel's, lies within them
    g = torch.Generator().manual_seed(0)
    y, ref = torch.randn((4, 16, 48), generator=g), torch.randn((1, 16, 48), generator=g)
    mask = torch.zeros((4, 32), dtype=torch.bool)
    mask[:, 16:] = True
    r = RR.response(y, ref, mask, 2, 3, 16, 16, 4, 1)
    d = (y - ref).view(4, 4, 4, 4, 4, 3).flip(-1)
    r32 = (d * d).sum(-1).permute(0, 1, 3, 2, 4).reshape(4, 16, 16)
    assert bool(((r32.double() - r).abs() <= RR.pixel_bound(3) * r).all())
    assert bool(((r32.sum((1, 2)).double() - r.sum((1, 2))).abs() <= RR.mass_bound(3, 16, 16) * r.sum((1, 2))).all())


def test_the_gpu_cases_are_decided_by_their_inputs():
    """the condition under which tests/test_token_response_gpu.py asks for EQUAL peak indices, checked here on every case it runs"""
    import test_token_response_gpu as TG

    leads = []
    for name in sorted(TG.GEOMETRIES):
        T, Cc, H, W, P, _ = TG.GEOMETRIES[name]
        for B, shared, frame, seed in TG.cases(name):
            y, ref, mask = TG.inputs(name, B, shared, frame, seed)
            ok, lead = TG.decided(RR.response(y, ref, mask, T, Cc, H, W, P, frame), Cc)
            assert ok, (name, B, shared, frame, lead)
            leads.append(lead)
    print("relative lead of the largest response over the second: at least %.3e (needed: %.3e)" % (min(leads), 2 * RR.pixel_bound(4)))
    assert len(leads) == 6 * 8


# ---- the binding ----------------------------------------------------------------------------------------------------------------------------------------------
def test_binding_header_and_refusals():
    a = _lib.new_token_response_args()
    base = ctypes.sizeof(_lib.CwmPatchErrorArgs)
    assert a.struct_size == ctypes.sizeof(_lib.CwmTokenResponseArgs) == 8 + base + 5 * 8 and a.base.struct_size == base
    assert [f[0] for f in _lib.CwmTokenResponseArgs._fields_] == ["struct_size", "base", "y_ref_dev", "y_ref_stride_b", "pixel_map_dev", "peak_index_dev", "stats_dev"]
    assert _lib.CwmTokenResponseArgs.base.offset == 8 and _lib.CwmTokenResponseArgs.y_ref_dev.offset == 8 + base
    assert _lib.SIGNATURES["cwm_token_response"] == (ctypes.c_int, [ctypes.POINTER(_lib.CwmTokenResponseArgs)])
    src = open(os.path.join(ROOT, "include", "cwm_hip.h")).read()
    assert "perturbation.py:356-476" in src and "cwm_token_response_args" in src
    body = src[src.index("typedef struct cwm_token_response_args"):src.index("} cwm_token_response_args;")]
    assert "stream" not in body.replace("scratch_dev, stream", "")  # the stream is base.stream: the struct has no stream field of its own
    lib = _lib.get_lib()
    assert lib.cwm_version().decode() == "cwm_hip 0.10.4 gfx950"

    # argument checks need no device: everything below is refused before anything is launched (the pointers are never followed)
    def refused(what):
        assert lib.cwm_token_response(ctypes.byref(a)) == _lib.ERR_INVALID and what in lib.cwm_last_error(), lib.cwm_last_error()

    fake = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(fake)
    g = a.base
    g.y_tokens_dev = g.mask_dev = a.y_ref_dev = addr
    g.batch, g.T, g.C, g.H, g.W, g.P, g.n_vis, g.frame = 2, 2, 3, 16, 16, 4, 16, 1
    a.struct_size = 8
    refused(b"struct_size")
    a.struct_size = ctypes.sizeof(_lib.CwmTokenResponseArgs)
    refused(b"no output requested")
    a.stats_dev = addr
    refused(b"scratch")
    a.stats_dev, a.peak_index_dev = None, addr
    refused(b"scratch")
    g.scratch_dev, g.frame = addr, -1
    refused(b"frame = -1")
    g.frame = 2
    refused(b"frame = 2 of 2")
    g.frame, g.P = 1, 12
    refused(b"P = 12")
    g.P, a.y_ref_dev = 4, None
    refused(b"y_ref_dev")
    a.y_ref_dev, a.y_ref_stride_b = addr, -48
    refused(b"y_ref_stride_b")
    a.y_ref_stride_b, g.n_vis = 0, 33
    refused(b"n_vis = 33")


# ---- the composed path's statistics, the patch list, the displacements ------------------------------------------------------------------------------------------
def test_torch_statistics_follow_the_contract():
    G = prediction.PredictorBasedGenerator
    g = torch.Generator().manual_seed(3)
    r = torch.rand((5, 12, 20), generator=g) ** 4
    r[1] = 0  # no response at all: index 0, the centroid is the peak position
    r[2, 7, 9] = r[2, 3, 15] = 2.0  # equal maxima: the first
    r[3] = 0
    r[3, 11, 19] = 0.5
    idx, stats = G._response_statistics(r)
    want_idx, want = RR.statistics(r)
    assert torch.equal(idx, want_idx) and idx[1].item() == 0 and idx[2].item() == 3 * 20 + 15 and idx[3].item() == 239
    assert stats.dtype == torch.float32 and stats[1].tolist() == [0.0, 0.0, 0.0, 0.0] and stats[3].tolist() == [0.5, 0.5, 11.0, 19.0]
    assert torch.equal(stats[:, 0].double(), want[:, 0])
    assert bool(((stats[:, 1].double() - want[:, 1]).abs() <= RR.gamma(240) * want[:, 1]).all())
    assert bool(((stats[:, 2:].double() - want[:, 2:]).abs() <= RR.gamma(3 * 241) * want[:, 2:]).all())
    bad = r.clone()
    bad[0, 4, 4] = float("nan")
    idx, stats = G._response_statistics(bad)
    assert idx[0].item() == 4 * 20 + 4 and bool(stats[0].isnan().all()) and not stats[1:].isnan().any()


def test_marker_patches():
    P_ = prediction.PredictorBasedGenerator._marker_patches
    assert P_([[1, 2], (0, 3)]).tolist() == [[0, 1, 2], [0, 0, 3]]
    assert P_([[1, 1, 2]]).tolist() == [[1, 1, 2]]
    assert P_([torch.tensor([0, 1, 2, 3]), np.array([0, 0, 0, 1])]).tolist() == [[1, 2, 3], [0, 0, 1]]
    assert P_([[1, 2], [1, 1, 2]]).tolist() == [[0, 1, 2], [1, 1, 2]]
    for bad in ([], [[1]], [[1, 0, 2, 3]], [[1, 2], [0, 1, 2, 3, 4]]):
        with pytest.raises(ValueError):
            P_(bad)


def test_displacements_from_statistics():
    res = prediction.MarkerResponses(peak_yx=np.array([[5, 9], [0, 0], [31, 31]]), peak=np.ones(3, np.float32), mass=np.array([2.0, 0.0, 1.0], np.float32),
                                     centroid=np.array([[4.25, 10.5], [0.0, 0.0], [30.0, 29.5]], np.float32))
    patches = [[0, 1], [0, 0], [3, 3]]  # centres (3.5, 11.5), (3.5, 3.5), (27.5, 27.5) at P = 8
    F = segmentation.FlowGenerator.marker_displacements
    flow = F(patches, res, 8)
    assert flow.dtype == np.float32 and flow.tolist() == [[9 - 11.5, 5 - 3.5], [-3.5, -3.5], [3.5, 3.5]]  # (dx, dy)
    assert F(patches, res, 8, use_centroid=True).tolist() == [[10.5 - 11.5, 4.25 - 3.5], [-3.5, -3.5], [2.0, 2.5]]
    assert F([[2, 5]], prediction.MarkerResponses(np.array([[10, 22]]), None, None, None), 4).tolist() == [[22 - 21.5, 10 - 9.5]]
