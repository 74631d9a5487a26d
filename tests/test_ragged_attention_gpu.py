"""cwm_attention_ragged on a real MI355X: attention with a key count per batch row (AttnParams.key_len; csrc/attention.hip, attention_pipe.hip).

Batch row b attends to keys [0, len[b]) of its N rows and only its query rows [0, len[b]) are written.  Checked against a dense fp32 softmax over the
valid keys, against cwm_attention on every row alone, bit for bit against cwm_attention when every length is N, with NaN in everything past the
lengths, and for lengths the entry point has to refuse.  Both kernels are reached in both modes: the 4-wave kernel below 160 (parity) / 512 (fast)
tokens, the software-pipelined one from there."""
import ctypes as C

import pytest
import torch

from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu

TOL = {"parity": 3e-4, "fast": 3e-2}  # tests/test_kernels_gpu.py test_attention_matches_dense_softmax
SENTINEL = -12345.0
CWM_ERR_INVALID = -1

# (B, N, H), lengths.  The third has an XCD-mapped grid (B * H = 8) and a last query tile of <= 32 rows for some rows only (792, 785, 784, 769 ...)
DENSE_CASES = [
    ((4, 200, 2), [200, 1, 64, 65]),
    ((4, 128, 1), [128, 127, 63, 33]),
    ((8, 792, 1), [792, 785, 784, 769, 768, 705, 129, 8]),
]
# 25 query tiles x 21 (batch, head) = 525 work items on 512 workgroup slots: the rectangular launch of this shape cuts the 13 items of its last round
# into key ranges (attention_pipe.hip launch_pipe); the ragged launch must not
KSPLIT_CASE = ((3, 3168, 7), [3168, 3140, 2049])


def _bind(lib):
    lib.cwm_attention_ragged.restype = C.c_int
    lib.cwm_attention_ragged.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _bind(_lib.get_lib())


@pytest.fixture(scope="module")
def dlib():
    """the development library: the same objects + cwm_debug_set (thread-local options of that shared object)"""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _bind(_lib.get_dev_lib())


def stream():
    return _lib.current_stream_handle(torch.device("cuda:0"))


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def ragged(lib, qkv, lens, H, mode):
    """(status, O on the CPU); O starts as SENTINEL everywhere"""
    B, N, _ = qkv.shape
    q_d = qkv.cuda().contiguous()
    l_d = torch.tensor(lens, dtype=torch.int32).cuda()
    out = torch.full((B, N, H * 64), SENTINEL, device="cuda", dtype=torch.float32)
    rc = lib.cwm_attention_ragged(q_d.data_ptr(), l_d.data_ptr(), out.data_ptr(), B, N, H, _lib.mode_id(mode), stream())
    return rc, out.cpu()


def rect(lib, qkv, H, mode):
    B, N, _ = qkv.shape
    q_d = qkv.cuda().contiguous()
    out = torch.empty(B, N, H * 64, device="cuda", dtype=torch.float32)
    _lib.check(lib.cwm_attention(q_d.data_ptr(), out.data_ptr(), B, N, H, _lib.mode_id(mode), stream()), lib)
    return out.cpu()


def dense_masked(qkv, lens, H):
    """fp32 softmax(q k^T / 8) v over the first lens[b] keys of row b (rows of the result past lens[b] mean nothing)"""
    B, N, _ = qkv.shape
    q, k, v = qkv.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q * 0.125) @ k.transpose(-2, -1)
    dead = torch.arange(N)[None, :] >= torch.tensor(lens)[:, None]  # [B, N] keys
    s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B, N, H * 64)


@pytest.fixture(scope="module")
def dense_inputs():
    """inputs and dense references of DENSE_CASES, made once"""
    made = []
    for (B, N, H), lens in DENSE_CASES:
        qkv = rnd(B, N, 3 * H * 64, seed=N + 11)
        made.append(((B, N, H), lens, qkv, dense_masked(qkv, lens, H)))
    return made


def check_unwritten(out, lens):
    for b, n in enumerate(lens):
        assert (out[b, n:] == SENTINEL).all(), ("rows past the length were written", b, n)


@pytest.mark.parametrize("mode", ["parity", "fast"])
def test_ragged_attention_matches_dense_softmax_over_the_valid_keys(lib, dense_inputs, mode):
    for (B, N, H), lens, qkv, ref in dense_inputs:
        rc, out = ragged(lib, qkv, lens, H, mode)
        _lib.check(rc, lib)
        for b, n in enumerate(lens):
            assert torch.isfinite(out[b, :n]).all(), (mode, B, N, H, b, n)
            err = (out[b, :n] - ref[b, :n]).abs().max().item()
            print("ragged vs dense", mode, (B, N, H), "row", b, "len", n, "err %.3e" % err)
            assert err <= TOL[mode], (err, mode, B, N, H, b, n)
        check_unwritten(out, lens)


@pytest.mark.parametrize("mode", ["parity", "fast"])
def test_ragged_attention_where_the_rectangular_launch_splits_its_last_round(lib, mode):
    """every row against cwm_attention on that row alone, at N = its length"""
    (B, N, H), lens = KSPLIT_CASE
    assert (-(-N // 128) * B * H) % 512 == 13  # the shape still is what the comment above says it is
    qkv = rnd(B, N, 3 * H * 64, seed=N + 12)
    rc, out = ragged(lib, qkv, lens, H, mode)
    _lib.check(rc, lib)
    for b, n in enumerate(lens):
        alone = rect(lib, qkv[b:b + 1, :n], H, mode)
        err = (out[b, :n] - alone[0]).abs().max().item()
        print("ragged vs row alone", mode, "row", b, "len", n, "err %.3e" % err)
        assert err <= TOL[mode], (err, mode, b, n)
    check_unwritten(out, lens)


@pytest.mark.parametrize("mode", ["parity", "fast"])
def test_ragged_attention_with_full_lengths_is_bitwise_the_rectangular_attention(dlib, mode):
    """Ragged launches run the regular schedule (no key-split last query tile, no key-split last round: DESIGN.md 8.14), so the rectangular side is
    taken with "attn_tail" = 0 and "attn_ksplit" = 0, through the development library."""
    try:
        _lib.check(dlib.cwm_debug_set(b"attn_tail", 0), dlib)
        _lib.check(dlib.cwm_debug_set(b"attn_ksplit", 0), dlib)
        for (B, N, H) in [c for c, _ in DENSE_CASES] + [(2, 792, 4), KSPLIT_CASE[0]]:
            qkv = rnd(B, N, 3 * H * 64, seed=N + 13)
            ref = rect(dlib, qkv, H, mode)
            rc, out = ragged(dlib, qkv, [N] * B, H, mode)
            _lib.check(rc, dlib)
            assert torch.equal(out, ref), (mode, B, N, H, (out - ref).abs().max().item())
    finally:
        _lib.check(dlib.cwm_debug_set(b"attn_tail", 1), dlib)
        _lib.check(dlib.cwm_debug_set(b"attn_ksplit", 1), dlib)


@pytest.mark.parametrize("mode", ["parity", "fast"])
def test_ragged_attention_ignores_nan_past_the_lengths(lib, dense_inputs, mode):
    """q, k and v rows at and past each length hold NaN: the valid output rows stay finite and do not change by a bit (a zero weight would not do:
    0 x NaN is NaN -- those keys must never be staged)"""
    for (B, N, H), lens, qkv, _ in dense_inputs:
        rc, clean = ragged(lib, qkv, lens, H, mode)
        _lib.check(rc, lib)
        poisoned = qkv.clone()
        for b, n in enumerate(lens):
            poisoned[b, n:] = float("nan")
        rc, out = ragged(lib, poisoned, lens, H, mode)
        _lib.check(rc, lib)
        for b, n in enumerate(lens):
            assert torch.isfinite(out[b, :n]).all(), (mode, B, N, H, b, n)
            assert torch.equal(out[b, :n], clean[b, :n]), (mode, B, N, H, b, n)
        check_unwritten(out, lens)


@pytest.mark.parametrize("mode", ["parity", "fast"])
@pytest.mark.parametrize("N", [128, 200, 792])
def test_ragged_attention_refuses_bad_lengths(lib, mode, N):
    B, H = 3, 1
    qkv = rnd(B, N, 3 * H * 64, seed=N + 14)
    for lens in ([N, 0, 5], [N + 1, N, N], [7, N, -3]):
        rc, out = ragged(lib, qkv, lens, H, mode)
        assert rc == CWM_ERR_INVALID, (mode, N, lens, rc)
        assert b"key count" in lib.cwm_last_error()
        assert (out == SENTINEL).all(), (mode, N, lens)
    rc, out = ragged(lib, qkv, [N, 1, 5], H, mode)  # and the entry point works afterwards
    _lib.check(rc, lib)
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1, :1]).all()
