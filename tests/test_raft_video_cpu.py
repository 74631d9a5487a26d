"""RAFT's video warm start without a GPU: the entry point `cwm_raft_forward_interpolate` in the header and the ctypes binding, the Python surface, and the
guards and sizes recorded in the fixtures of tests/golden/make_golden_raft_video.py, including that the numpy restatement of `forward_interpolate`
(tests/raft_video_restatement.py) reproduces every stored scipy result bit for bit without scipy."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import raft_video_restatement as R
from counterfactualworldmodels_amd import _lib, raft, segmentation
from counterfactualworldmodels_amd.raft import RAFT

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
HEADER = os.path.join(os.path.dirname(HERE), "include", "cwm_hip.h")
FIELDS = {"16x16_a1": (16, 16), "16x16_a6": (16, 16), "16x16_t": (16, 16), "17x19_a3": (17, 19), "28x28_a3": (28, 28), "40x56_a8": (40, 56)}
GAP_MIN = 1e-9


def test_entry_point_is_declared_cited_and_bound():
    with open(HEADER) as fh:
        text = fh.read()
    decl = ("CWM_API int cwm_raft_forward_interpolate(const float* flow_dev, int64_t stride_p, int64_t stride_c, int P, int h8, int w8, float* out_dev, "
            "void* stream);")
    assert decl in text
    comment = text[text.index("RAFT's forward interpolation on the device"):text.index(decl)]
    assert re.search(r"replaces:.*raft/utils\.py:28-56", comment)
    for word in ("x1 > 0 && x1 < w8 && y1 > 0 && y1 < h8", "lowest i wins", "zeros", "overlaps", "does not synchronise"):
        assert word in comment, word
    res, argtypes = _lib.SIGNATURES["cwm_raft_forward_interpolate"]
    assert res is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert hasattr(_lib.get_lib(), "cwm_raft_forward_interpolate")
    # the forward's structs are as they were: the chain is driven from Python over cwm_raft_forward_ex
    assert len(_lib.CwmRaftForwardArgs._fields_) == 26 and len(_lib.CwmRaftForwardExArgs._fields_) == 10


def test_python_surface():
    sig = inspect.signature(RAFT._forward_multiframe)
    assert sig.parameters["warm_start"].default is False
    assert list(sig.parameters)[:7] == ["self", "x", "iters", "flow_init", "upsample", "test_mode", "backward"]  # positional order as before
    assert callable(raft.forward_interpolate) and list(inspect.signature(raft.forward_interpolate).parameters) == ["flow"]
    assert "warm_start" in (segmentation.FlowGenerator.predict_flow.__doc__ or "")
    with pytest.raises(RuntimeError, match=r"forward_interpolate needs a CUDA/HIP tensor \(no CPU fallback\); got cpu"):
        raft.forward_interpolate(torch.zeros(2, 16, 16))
    for mod in (raft, R):  # neither needs scipy
        assert not re.search(r"^\s*(import|from) scipy", inspect.getsource(mod), re.M)


def test_field_fixture_guards_and_restatement():
    limit = os.path.getsize(os.path.join(GOLDEN, "base8_k8_b2.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "raft_finterp_fields.npz")) <= limit
    g = np.load(os.path.join(GOLDEN, "raft_finterp_fields.npz"))
    assert sorted(str(n) for n in g["names"]) == sorted(FIELDS)
    for name, (h, w) in FIELDS.items():
        f, y = g[name + "_in"], g[name + "_out"]
        assert f.shape == y.shape == (2, h, w) and f.dtype == y.dtype == np.float32
        index, gap = R.nearest_sources(f)
        assert float(g[name + "_gap"]) >= GAP_MIN and gap.min() == float(g[name + "_gap"])
        assert np.array_equal(R.forward_interpolate(f).view(np.int32), y.view(np.int32)), name  # scipy's result, every element
        valid = R.landing_points(f)[2]
        assert 0.03 <= 1.0 - valid.mean() < 0.5 and (np.abs(y - f).max(axis=0) > 0).mean() >= 0.5
        assert index.min() >= 0 and valid[index].all()
    a, t = g["16x16_a6_in"], g["16x16_t_in"]
    assert np.array_equal(t, np.stack([a[1].T, a[0].T]))
    assert np.array_equal(g["16x16_t_out"], np.stack([g["16x16_a6_out"][1].T, g["16x16_a6_out"][0].T]))  # the operation commutes with the transposition


def test_video_fixture_guards_and_restatement():
    limit = os.path.getsize(os.path.join(GOLDEN, "base8_k8_b2.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "raft_video_128x160_t4.npz")) <= limit
    g = np.load(os.path.join(GOLDEN, "raft_video_128x160_t4.npz"))
    assert int(g["iters"]) == 3 and list(g["shift"]) == [2, -3]
    for d in ("fwd", "bwd"):
        assert g["cold_" + d].shape == (1, 3, 2, 16, 20)
        assert g["warm_vs_cold_" + d].shape == g["drift_" + d].shape == (3,)
        assert g["warm_vs_cold_" + d][0] == 0.0 and (g["warm_vs_cold_" + d][1:] >= 0.5).all()
        assert (g["drift_" + d] > 0).all() and (g["drift_" + d] <= 1e-4).all()
        for k in range(3):
            low = g["%s_low_%d" % (d, k)]
            assert low.shape == (1, 2, 16, 20) and low.dtype == np.float32
            if k == 0:
                assert np.array_equal(low, g["cold_" + d][:, 0])  # the first pair of a chain is cold
                assert "%s_init_0" % d not in g.files
            else:
                init = g["%s_init_%d" % (d, k)]
                assert init.shape == (1, 2, 16, 20) and init.dtype == np.float32
                assert float(g["%s_gap_%d" % (d, k - 1)]) >= GAP_MIN
                prev = g["%s_low_%d" % (d, k - 1)]
                assert R.min_gap(prev[0]) == float(g["%s_gap_%d" % (d, k - 1)])
                assert np.array_equal(R.forward_interpolate(prev).view(np.int32), init.view(np.int32)), (d, k)
                assert float(np.abs(low - g["cold_" + d][:, k]).max()) > 1e-2  # the init moved the low-resolution flow too
        if d == "fwd":
            assert all(g["fwd_up_%d" % k].shape == (1, 2, 128, 160) and g["fwd_up_%d" % k].dtype == np.float32 for k in range(3))
        else:
            assert not any(n.startswith("bwd_up") for n in g.files)
    assert not np.array_equal(g["fwd_low_0"], g["bwd_low_0"])


def test_restatement_rules():
    """what the restatement fixes beyond scipy: the lowest index among equal distances, zeros without a valid source, strict validity"""
    f = np.zeros((2, 4, 4), dtype=np.float32)  # every interior source lands on its own grid point; the border (x1 = 0 or y1 = 0) is invalid
    index, gap = R.nearest_sources(f)
    assert list(index.reshape(4, 4)[0]) == [5, 5, 6, 7] and list(index.reshape(4, 4)[:, 0]) == [5, 5, 9, 13]
    assert gap.min() == 1.0 and (R.forward_interpolate(f) == 0).all()
    f[0, 1, 1] = 1.0  # source 5 now lands on (2, 1), where source 6 lands too: target 6 sees both at distance 0 and takes the lower index
    index, gap = R.nearest_sources(f)
    assert index[6] == 5 and gap[6] == 0.0 and R.forward_interpolate(f)[0, 1, 2] == 1.0
    f = np.full((2, 3, 3), 9.0, dtype=np.float32)
    assert (R.nearest_sources(f)[0] == -1).all() and (R.forward_interpolate(f) == 0).all()
    f = np.full((2, 3, 3), np.nan, dtype=np.float32)
    f[:, 1, 1] = (0.5, -0.5)
    assert (R.nearest_sources(f)[0] == 4).all() and (R.forward_interpolate(f)[0] == 0.5).all() and (R.forward_interpolate(f)[1] == -0.5).all()
    f = np.zeros((2, 1, 3), dtype=np.float32)
    f[1] = 0.5
    f[0, 0, 2] = 1.0  # x1 = 3 = w: invalid
    assert list(R.landing_points(f)[2]) == [False, True, False]
    P = np.stack([f, f[:, :, ::-1].copy()])
    assert R.forward_interpolate(P).shape == (2, 2, 1, 3) and np.array_equal(R.forward_interpolate(P)[0], R.forward_interpolate(f))
