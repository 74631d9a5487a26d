"""RAFT's on-the-fly correlation without a GPU: the new entry points in the header and the ctypes binding, the Python surface (`corr=`, `set_corr`,
`workspace_bytes`), the FLOP accounting, and `InputPadder` against the reference's class (tests/golden/make_golden_raft_padder.py), bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import _lib, config as C
from counterfactualworldmodels_amd.raft import RAFT, InputPadder, _args, load_raft_model

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")


def header(name="cwm_hip.h"):
    with open(os.path.join(INCLUDE, name)) as fh:
        return fh.read()


def test_new_symbols_are_declared_bound_and_cite_the_reference():
    text = header()
    assert re.search(r"CWM_API int cwm_raft_set_corr\(cwm_raft_model\* m, int corr\);", text)
    assert re.search(r"CWM_API int cwm_raft_workspace_bytes\(cwm_raft_model\* m, uint64_t\* out\);", text)
    assert re.search(r"CWM_API int cwm_raft_corr_lookup_on_the_fly\(const float\* fmap1_dev, const float\* fmap2_dev, const float\* coords_dev, int P, int h8, "
                     r"int w8, float\* out_dev,\s+void\* stream\);", text)
    assert re.search(r"#define CWM_RAFT_CORR_ALL_PAIRS 0\b", text) and re.search(r"#define CWM_RAFT_CORR_ON_THE_FLY 1\b", text)
    comment = text[text.index("The correlation computed at lookup time"):text.index("#define CWM_RAFT_CORR_ALL_PAIRS")]
    assert "raft/corr.py:63-91" in comment and "replaces:" in comment and "added after 0.10.4" in comment
    for name in ("cwm_raft_set_corr", "cwm_raft_workspace_bytes", "cwm_raft_corr_lookup_on_the_fly"):
        assert name in comment, name
    dev = header("cwm_hip_dev.h")
    assert "raft/corr.py:63-91" in dev[:dev.index("cwm_dev_raft_corr_lookup_on_the_fly_operand(")][-400:]
    assert _lib.SIGNATURES["cwm_raft_set_corr"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    res, argtypes = _lib.SIGNATURES["cwm_raft_workspace_bytes"]
    assert res is ctypes.c_int and argtypes[1]._type_ is ctypes.c_uint64
    assert _lib.SIGNATURES["cwm_raft_corr_lookup_on_the_fly"] == _lib.SIGNATURES["cwm_raft_corr_lookup"]
    assert _lib.DEV_SIGNATURES["cwm_dev_raft_corr_lookup_on_the_fly_operand"] == _lib.DEV_SIGNATURES["cwm_dev_raft_corr_lookup_operand"]
    lib, dev_lib = _lib.get_lib(), _lib.get_dev_lib()
    for name in ("cwm_raft_set_corr", "cwm_raft_workspace_bytes", "cwm_raft_corr_lookup_on_the_fly"):
        assert hasattr(lib, name) and hasattr(dev_lib, name), name
    assert hasattr(dev_lib, "cwm_dev_raft_corr_lookup_on_the_fly_operand")
    assert not hasattr(ctypes.CDLL(_lib.library_path()), "cwm_dev_raft_corr_lookup_on_the_fly_operand")
    assert (_lib.RAFT_CORR_ALL_PAIRS, _lib.RAFT_CORR_ON_THE_FLY) == (0, 1)
    assert lib.cwm_version().decode() == "cwm_hip 0.10.4 gfx950"  # the version string stays
    assert RAFT._ABI["set_corr"] == "cwm_raft_set_corr" and RAFT._ABI["workspace_bytes"] == "cwm_raft_workspace_bytes"


def test_set_corr_refuses_null_and_unknown_values_without_a_device():
    """argument checks that come before any use of the handle or the device"""
    lib = _lib.get_lib()
    assert lib.cwm_raft_set_corr(None, 1) == _lib.ERR_INVALID
    n = ctypes.c_uint64(7)
    assert lib.cwm_raft_workspace_bytes(None, ctypes.byref(n)) == _lib.ERR_INVALID and n.value == 7
    assert lib.cwm_raft_corr_lookup_on_the_fly(None, None, None, 1, 16, 16, None, None) == _lib.ERR_INVALID
    assert b"cwm_raft_corr_lookup_on_the_fly" in lib.cwm_last_error()


def test_corr_keyword_attribute_and_setter():
    assert _args().corr == "all_pairs" and RAFT().corr == "all_pairs"
    m = load_raft_model(None, output_dim=1, corr="on_the_fly")
    assert m.corr == "on_the_fly" and m.args.corr == "on_the_fly"
    assert m.set_corr("all_pairs") is m and m.corr == "all_pairs"
    assert m.set_corr("on_the_fly").corr == "on_the_fly"
    assert m.workspace_bytes() == 0  # no handle yet
    for bad in ("alternate", "", None, 1):
        with pytest.raises(ValueError, match="corr"):
            m.set_corr(bad)
        assert m.corr == "on_the_fly"
    with pytest.raises(ValueError, match="corr"):
        RAFT(_args(corr="volume"))
    with pytest.raises(ValueError, match="corr"):
        load_raft_model(None, output_dim=1, corr="volume")


def test_alternate_corr_still_raises_and_points_to_the_keyword():
    with pytest.raises(NotImplementedError, match="on_the_fly"):
        load_raft_model(None, output_dim=1, alternate_corr=True)
    with pytest.raises(NotImplementedError):
        RAFT(_args(alternate_corr=True, corr="on_the_fly"))


def test_algorithmic_flops_of_both_forms():
    base = C.raft_algorithmic_flops(224, 224, 24)
    assert abs(base / 1e9 - 122.17) < 0.005
    assert C.raft_algorithmic_flops(224, 224, 24, corr="all_pairs") == base
    for H, W, iters in ((224, 224, 24), (440, 1024, 24), (1080, 1920, 12), (136, 152, 1)):
        hw = (H // 8) * (W // 8)
        all_pairs, on_the_fly = C.raft_algorithmic_flops(H, W, iters), C.raft_algorithmic_flops(H, W, iters, corr="on_the_fly")
        want = all_pairs - 2.0 * 256 * hw * hw + iters * 204800.0 * hw
        assert abs(on_the_fly - want) <= 1e-12 * want, (H, W, iters)
    # 4 levels x 100 neighbours x 2 x 256 per pixel and iteration against 2 x 256 x hw once: equal at hw = 400 x iters = 9600 for 24 iterations
    assert C.raft_algorithmic_flops(640, 960, 24, corr="on_the_fly") == pytest.approx(C.raft_algorithmic_flops(640, 960, 24), rel=1e-12)
    assert C.raft_algorithmic_flops(1080, 1920, 24, corr="on_the_fly") < C.raft_algorithmic_flops(1080, 1920, 24)
    assert C.raft_algorithmic_flops(224, 224, 24, corr="on_the_fly") > base
    with pytest.raises(ValueError):
        C.raft_algorithmic_flops(224, 224, 24, corr="alternate")


def test_input_padder_equals_the_reference_bit_for_bit():
    g = np.load(os.path.join(GOLDEN, "raft_input_padder.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "raft_input_padder.npz")) < 16384
    sizes = [tuple(int(v) for v in s) for s in g["sizes"]]
    assert sizes == [(436, 1024), (375, 1242), (224, 224), (129, 130), (7, 9)]
    for mode in ("sintel", "kitti"):
        for (h, w), pad in zip(sizes, g["pad_" + mode]):
            p = InputPadder((2, 3, h, w), mode=mode)
            assert p._pad == [int(v) for v in pad], (mode, h, w)
            assert (h + p._pad[2] + p._pad[3]) % 8 == 0 and (w + p._pad[0] + p._pad[1]) % 8 == 0
        x = torch.from_numpy(g["x"])
        p = InputPadder(x.shape, mode=mode)
        out = p.pad(x)
        assert isinstance(out, list) and len(out) == 1
        assert out[0].dtype == torch.float32 and np.array_equal(out[0].numpy(), g["padded_" + mode])
        assert np.array_equal(p.unpad(out[0]).numpy(), g["unpadded_" + mode]) and torch.equal(p.unpad(out[0]), x)
    assert InputPadder((7, 9))._pad == InputPadder((7, 9), "sintel")._pad  # the default mode
    assert not np.array_equal(g["pad_sintel"], g["pad_kitti"])


def test_input_padder_takes_any_leading_dimensions():
    g = np.load(os.path.join(GOLDEN, "raft_input_padder.npz"))
    x = torch.from_numpy(g["x"])  # [1,3,7,9]
    p = InputPadder(x.shape)
    want = torch.from_numpy(g["padded_sintel"])
    movie = torch.stack([x, 2 * x], 1)  # [1,2,3,7,9]: the multi-frame call's input
    a, b, c = p.pad(movie, x[0], x[0, 0])
    assert a.shape == (1, 2, 3, 8, 16) and torch.equal(a[:, 0], want) and torch.equal(a[:, 1], 2 * want)
    assert b.shape == (3, 8, 16) and torch.equal(b, want[0])
    assert c.shape == (8, 16) and torch.equal(c, want[0, 0])
    assert torch.equal(p.unpad(a), movie)
