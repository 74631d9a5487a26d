"""RAFT's warm start and per-iteration outputs without a GPU: `cwm_raft_forward_ex_args` in the ctypes mirror against the header text, the
Python surface's argument handling, and the guards and sizes recorded in the fixtures of tests/golden/make_golden_raft_warm.py."""
import ctypes
import inspect
import os
import re

import numpy as np

from counterfactualworldmodels_amd import _lib
from counterfactualworldmodels_amd.raft import RAFT

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
HEADER = os.path.join(os.path.dirname(HERE), "include", "cwm_hip.h")
CTYPE_OF = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def header_fields(name):
    """[(field, ctypes type or struct name)] of `typedef struct <name> {...} <name>;` in the header, in order (pointers: c_void_p)."""
    with open(HEADER) as fh:
        text = fh.read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    out = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = re.match(r"((?:const )?[A-Za-z_0-9]+\s*\*?)\s*(.*)$", decl, re.S).groups()
        typ = typ.replace("const ", "").strip()
        for n in names.split(","):
            out.append((n.strip(), ctypes.c_void_p if typ.endswith("*") else CTYPE_OF.get(typ, typ)))
    return out


def test_ex_args_mirror_matches_the_header():
    fields = header_fields("cwm_raft_forward_ex_args")
    mirror = list(_lib.CwmRaftForwardExArgs._fields_)
    assert [f[0] for f in fields] == [f[0] for f in mirror] == [
        "struct_size", "base", "flow_init_dev", "flow_init_stride_b", "flow_init_stride_t", "flow_init_stride_c", "flow_iters_dev", "flow_iters_stride_i",
        "head_iters_dev", "head_iters_stride_i"]
    for (name, htype), (_, ctype) in zip(fields, mirror):
        if name == "base":
            assert htype == "cwm_raft_forward_args" and ctype is _lib.CwmRaftForwardArgs
        else:
            assert htype is ctype, name
    S = _lib.CwmRaftForwardExArgs
    assert S.base.offset == 8 and S.base.size == ctypes.sizeof(_lib.CwmRaftForwardArgs)
    assert S.flow_init_dev.offset == 8 + ctypes.sizeof(_lib.CwmRaftForwardArgs)
    assert ctypes.sizeof(S) == S.head_iters_stride_i.offset + 8 == 8 + ctypes.sizeof(_lib.CwmRaftForwardArgs) + 8 * 8


def test_base_is_the_unchanged_forward_args():
    """A freeze guard, not evidence for the feature (it passes without it): `cwm_raft_forward_args`, which the ex struct embeds, stays as 0.10.2 left it."""
    fields = header_fields("cwm_raft_forward_args")
    mirror = list(_lib.CwmRaftForwardArgs._fields_)
    assert [f[0] for f in fields] == [f[0] for f in mirror]
    assert all(h is c for (_, h), (_, c) in zip(fields, mirror))
    assert mirror[-1][0] == "mode" and len(mirror) == 26  # as 0.10.2 left it: what is new is in the ex struct


def test_new_ex_args_sets_both_sizes():
    a = _lib.new_raft_forward_ex_args()
    assert a.struct_size == ctypes.sizeof(_lib.CwmRaftForwardExArgs)
    assert a.base.struct_size == ctypes.sizeof(_lib.CwmRaftForwardArgs) == _lib.new_raft_forward_args().struct_size
    assert not a.flow_init_dev and not a.flow_iters_dev and not a.head_iters_dev and a.base.mode == 0
    a.base.iters = 5  # `base` is a view of the struct, not a copy
    assert a.base.iters == 5


def test_entry_point_is_declared_bound_and_versioned():
    with open(HEADER) as fh:
        text = fh.read()
    assert re.search(r"CWM_API int cwm_raft_forward_ex\(cwm_raft_model\* m, const cwm_raft_forward_ex_args\* args\);", text)
    comment = text[text.index("The same forward with RAFT's warm start"):text.index("typedef struct cwm_raft_forward_ex_args")]
    assert "raft_model.py:241-242" in comment and "raft_model.py:244-274" in comment and "replaces:" in comment
    res, argtypes = _lib.SIGNATURES["cwm_raft_forward_ex"]
    assert res is ctypes.c_int and argtypes[1]._type_ is _lib.CwmRaftForwardExArgs
    lib = _lib.get_lib()
    assert lib.cwm_version().decode() == "cwm_hip 0.10.4 gfx950"
    assert RAFT._ABI["forward_ex"] == "cwm_raft_forward_ex"


def test_python_signature_mirrors_the_reference():
    sig = inspect.signature(RAFT._forward_two_images)
    assert list(sig.parameters)[:7] == ["self", "image1", "image2", "iters", "flow_init", "upsample", "test_mode"]
    assert sig.parameters["iters"].default == 24 and sig.parameters["flow_init"].default is None
    assert sig.parameters["upsample"].default is True and sig.parameters["test_mode"].default is True
    src = inspect.getsource(RAFT)
    assert "NotImplementedError(\"flow_init" not in src and "test_mode=False (the per-iteration" not in src


def test_fixture_guards_and_sizes():
    limit = os.path.getsize(os.path.join(GOLDEN, "base8_k8_b2.npz"))
    for name in ("raft_warm_136x152_b2", "raft_warm_list_128", "raft_warm_128x160_t3"):
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= limit, name
    g = np.load(os.path.join(GOLDEN, "raft_warm_136x152_b2.npz"))
    assert g["up"].shape == (2, 2, 136, 152) and g["low"].shape == g["init"].shape == (2, 2, 17, 19) and int(g["iters"]) == 4
    assert g["up"].dtype == g["low"].dtype == g["init"].dtype == np.float32
    assert 1.0 < float(np.abs(g["init"]).max()) <= 3.0
    assert float(g["warm_vs_cold"]) >= 0.5 and 0 < float(g["drift"]) <= 1e-4
    g = np.load(os.path.join(GOLDEN, "raft_warm_list_128.npz"))
    assert g["preds"].shape == (3, 1, 2, 128, 128) and g["kp_preds"].shape == (3, 1, 1, 128, 128) and g["init"].shape == (1, 2, 16, 16) and int(g["iters"]) == 3
    steps = [float(np.abs(g["preds"][k] - g["preds"][k - 1]).max()) for k in (1, 2)]
    assert np.allclose(steps, g["steps"]) and min(steps) >= 0.1  # a build that repeats a prediction misses the 1e-2 px bound
    assert all(float(np.abs(g["kp_preds"][k] - g["kp_preds"][k - 1]).max()) > 10 * 1e-3 * float(np.abs(g["kp_preds"][k]).max()) for k in (1, 2))
    assert 0 < float(g["drift"]) <= 1e-4 and 0 < float(g["kp_drift"]) <= 1e-4
    g = np.load(os.path.join(GOLDEN, "raft_warm_128x160_t3.npz"))
    assert g["flow_fwd"].shape == g["flow_bwd"].shape == (1, 2, 2, 128, 160) and g["init"].shape == (1, 2, 16, 20) and int(g["iters"]) == 3
    assert float(g["warm_vs_cold"]) >= 0.5 and 0 < float(g["drift_fwd"]) <= 1e-4 and 0 < float(g["drift_bwd"]) <= 1e-4
    # after 3 warm-started iterations the init still dominates every flow; the direction and the pair order each move it by ten times the GPU test's
    # 1e-2 px bound all the same, so a wrong direction or an un-reversed backward order misses that bound
    for a, b in ((g["flow_fwd"], g["flow_bwd"]), (g["flow_fwd"], g["flow_bwd"][:, ::-1]), (g["flow_bwd"], g["flow_bwd"][:, ::-1])):
        assert float(np.abs(a - b).max()) >= 0.1
