"""RAFT's fast (bf16-operand) mode without a GPU: how the Python surface chooses the mode (`mixed_precision`, `set_mode`), the `mode` field of
`cwm_raft_forward_args` in the ctypes mirror and in the header, and the self-consistency of the reference-only fixture raft_fast_224_b2.npz
(tests/golden/make_golden_raft_fast.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from counterfactualworldmodels_amd import _lib
from counterfactualworldmodels_amd.raft import RAFT, _args, load_raft_model

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
HEADER = os.path.join(os.path.dirname(HERE), "include", "cwm_hip.h")


def test_default_mode_is_parity():
    assert RAFT().mode == "parity"
    assert RAFT(_args(mixed_precision=False)).mode == "parity"


def test_mixed_precision_selects_fast():
    assert RAFT(_args(mixed_precision=True)).mode == "fast"
    m = load_raft_model(None, output_dim=1, mixed_precision=True)
    assert m.mode == "fast" and m.output_dim == 1


def test_set_mode_round_trips_and_validates():
    m = RAFT()
    assert m.set_mode("fast") is m and m.mode == "fast"
    assert m.set_mode("parity").mode == "parity"
    with pytest.raises(ValueError, match="fast.*parity"):
        m.set_mode("half")
    assert m.mode == "parity"  # a refused mode changes nothing


def test_forward_args_mode_field():
    names = [f[0] for f in _lib.CwmRaftForwardArgs._fields_]
    assert names[-1] == "mode" and names[-2] == "head_stride_c"
    S = _lib.CwmRaftForwardArgs
    assert S.mode.offset == S.head_stride_c.offset + 8 and S.mode.size == 4
    assert ctypes.sizeof(S) == S.mode.offset + 8  # int32 + tail padding to the struct's 8-byte alignment
    a = _lib.new_raft_forward_args()
    assert a.struct_size == ctypes.sizeof(S)
    assert a.mode == 0
    assert 0 not in (_lib.MODE_FAST, _lib.MODE_PARITY)  # 0 is a value of its own: "not given", which is parity


def test_header_declares_the_field_and_documents_zero_as_parity():
    with open(HEADER) as fh:
        text = fh.read()
    body = re.search(r"typedef struct cwm_raft_forward_args \{(.*?)\} cwm_raft_forward_args;", text, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.search(r"head_stride_c;\s*int32_t mode;\s*$", fields)
    comment = body[body.index("appended in 0.10.2"):]
    assert re.search(r"0 or CWM_MODE_PARITY: parity", comment) and "CWM_MODE_FAST" in comment and "CWM_ERR_INVALID" in comment


def test_fixture_scalars_are_self_consistent():
    g = np.load(os.path.join(GOLDEN, "raft_fast_224_b2.npz"))
    ref = {"": np.load(os.path.join(GOLDEN, "raft_224_b2.npz"))["flow"], "kp_": np.load(os.path.join(GOLDEN, "raft_keypoint_224_b2.npz"))["map"]}
    base = {"": np.load(os.path.join(GOLDEN, "raft_224_b2.npz")), "kp_": np.load(os.path.join(GOLDEN, "raft_keypoint_224_b2.npz"))}
    assert int(g["seed"]) == int(base[""]["seed"]) and int(g["frames_seed"]) == int(base[""]["frames_seed"]) and int(g["iters"]) == 24
    assert int(g["kp_seed"]) == int(base["kp_"]["seed"]) and int(g["kp_frames_seed"]) == int(base["kp_"]["frames_seed"])
    for pre, emul in (("", "flow_emul"), ("kp_", "kp_emul")):
        y = g[emul]
        assert y.dtype == np.float32 and y.shape == ref[pre].shape
        err_max, err_mean, spread = float(g[pre + "err_max"]), float(g[pre + "err_mean"]), float(g[pre + "spread_max"])
        # the scalars are those of the stored array against the stored fp32 reference
        assert abs(float(np.abs(y - ref[pre]).max()) - err_max) < 1e-6 and abs(float(np.abs(y - ref[pre]).mean()) - err_mean) < 1e-6
        assert abs(float(np.abs(ref[pre]).max()) - float(g[pre + "ref_max"])) < 1e-6
        assert err_max >= err_mean > 0
        assert float(g[pre + "err_max_A"]) >= float(g[pre + "err_mean_A"]) > 0
        assert spread < err_max
    # the bf16-operand error is small against the flow itself: below 2 % of the fp32 flow's max-abs
    assert float(g["err_max"]) < 0.02 * float(np.abs(ref[""]).max())
    assert os.path.getsize(os.path.join(GOLDEN, "raft_fast_224_b2.npz")) <= os.path.getsize(os.path.join(GOLDEN, "raft_224_b2.npz"))
