"""cwm_attention_ragged without a device: the symbol, its binding, its documentation and the argument checks that run before any HIP call."""
import os
import re

from counterfactualworldmodels_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CWM_ERR_INVALID = -1


def test_ragged_attention_is_exported_bound_and_documented():
    lib = _lib.get_lib()
    assert hasattr(lib, "cwm_attention_ragged") and hasattr(_lib.get_dev_lib(), "cwm_attention_ragged")
    ret, args = _lib.SIGNATURES["cwm_attention_ragged"]
    assert len(args) == len(_lib.SIGNATURES["cwm_attention"][1]) + 1  # cwm_attention's arguments + the key counts
    src = open(os.path.join(ROOT, "include", "cwm_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*CWM_API int cwm_attention_ragged\(const float\* qkv_dev, const int32_t\* key_len_dev, float\* o_dev, int B, int N, int H, int mode, void\* stream\);", src, flags=re.S)
    assert m, "the header declares cwm_attention_ragged under a comment"
    comment = m.group(1)
    # what the reference does instead, and where
    assert "prediction.py:421" in comment and "vmae.py:167" in comment
    assert "CWM_ERR_INVALID" in comment and "attn_tail" in comment and "attn_ksplit" in comment


def test_ragged_attention_refuses_null_pointers_and_bad_modes_before_any_launch():
    lib = _lib.get_lib()
    for (qkv, lens, out, B, N, H, mode) in [(0, 8, 8, 1, 64, 1, 1), (8, 0, 8, 1, 64, 1, 1), (8, 8, 0, 1, 64, 1, 1), (8, 8, 8, 0, 64, 1, 1), (8, 8, 8, 1, 0, 1, 1),
                                            (8, 8, 8, 1, 64, 0, 1), (8, 8, 8, 1, 64, 1, 77)]:
        assert lib.cwm_attention_ragged(qkv, lens, out, B, N, H, mode, None) == CWM_ERR_INVALID
        assert b"cwm_attention_ragged" in lib.cwm_last_error()
