"""The half-height instance of the 256x256 8-phase GEMM tile (csrc/gemm.hip gemm8p_tile<PLANES, false, true>): a last row tile with at most 128 rows stages
A0 | W0 | W1 only and runs the two quadrants that hold rows.  Rows keep their product sequence, so every output must equal, bit for bit,

  * the full tile ("gemm_debug" bit 2048 takes the instance away), and
  * the 128x128 kernel ("gemm_tile" 1: DESIGN.md section 4.1, one product sequence per accumulator in both kernels),

with the 8-phase kernel forced ("gemm_tile" 4), in both modes, with all four epilogues, in the LDS-staged, the direct and the per-fragment form.
M: 1, 127, 128 (one half-height tile), 129 (a ragged FULL tile: 129 rows need the second quadrant row), 256 + 1, 256 + 128 (a full tile and a half-height
one), 256 + 129, 3 * 256 + 128.  N: 256 and 384 -- 384 ends in a half-width column tile, so the ragged row and the half-width column meet in one tile (that
tile runs as the half-width instance).  The Q/K/V scatter needs N = 3 * heads * head_dim: 384 and 768 there.  K: 64 (one K tile in fast mode: prologue
only) and 384.  Random N(0, 1) operands; outputs compared whole, sentinel included: a store outside the launch's rows would show.
Then the same comparison through the engine's row maps: the kept rows of a pruned block in place, and the residual row map of to_decoder."""
import contextlib
import ctypes

import pytest
import torch

from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu

MODES = ("parity", "fast")
F32, GELU, BF16, QKV = 0, 1, 2, 3
EPI_NAMES = {F32: "f32", GELU: "gelu", BF16: "bf16", QKV: "qkv"}
FORMS = ((1, 0), (1, 2), (0, 0))  # (gemm_staged, gemm_direct): LDS-staged, direct (fp32 outputs too), per-fragment
MS = (1, 127, 128, 129, 256 + 1, 256 + 128, 256 + 129, 3 * 256 + 128)
KS = (64, 384)
NO_HALF_HEIGHT = 2048
SENT = -12345.75
DEFAULTS = {"gemm_tile": 0, "gemm_debug": 0, "gemm_staged": 1, "gemm_direct": 1}


@pytest.fixture(scope="module")
def gu():
    import gpu_utils

    return gpu_utils


@pytest.fixture(scope="module")
def d():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.get_dev_lib()


@contextlib.contextmanager
def switches(d, **kw):
    try:
        for k, v in kw.items():
            _lib.check(d.cwm_debug_set(k.encode(), int(v)), d)
        yield
    finally:
        for k in kw:
            d.cwm_debug_set(k.encode(), DEFAULTS[k])


def rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda().contiguous()


def run_gemm(d, gu, mode, epi, a, w, bias, **fields):
    g = _lib.new_dev_conj_args(_lib.CwmDevGemmArgs)
    g.mode, g.epi = _lib.mode_id(mode), epi
    g.a, g.w, g.bias = a.data_ptr(), w.data_ptr(), _lib.ptr(bias)
    (g.M, g.K), g.N = a.shape, w.shape[0]
    for k, v in fields.items():
        setattr(g, k, v.data_ptr() if torch.is_tensor(v) else v)
    forms = (ctypes.c_int32 * 2)(-1, -1)
    g.plan_forms = forms
    g.stream = gu.stream()
    _lib.check(d.cwm_dev_gemm(ctypes.byref(g)), d)


def launch(d, gu, mode, epi, a, w, bias, resid):
    """one launch of the epilogue form `epi` into fresh sentinel-filled outputs -> the list of raw output buffers"""
    planes = 2 if mode == "parity" else 1
    M, N = a.shape[0], w.shape[0]
    if epi == F32:
        C = torch.full((M + 3, N), SENT, device="cuda")
        run_gemm(d, gu, mode, epi, a, w, bias, C=C, ldc=N, resid=resid, ldr=N)
        return [C]
    if epi == QKV:
        D, guard = N // 3, 192
        count = M * D
        bufs = [torch.full((planes, count + guard), gu.NAN_BF16, dtype=torch.int16, device="cuda") for _ in range(3)]
        run_gemm(d, gu, mode, epi, a, w, bias, rows_in=M, rows_out=M, map_stride=M, q_out=bufs[0], k_out=bufs[1], v_out=bufs[2], qk_plane=count + guard,
                 heads=D // 64, head_dim=64, n_tok=M, q_scale=0.125)
        return bufs
    out = gu.new_operand(M + 3, N, planes)
    run_gemm(d, gu, mode, epi, a, w, bias, out=out, ldo=N)
    return [out]


def same(xs, ys):
    return all(torch.equal(x.view(torch.int16) if x.element_size() == 2 else x.view(torch.int32), y.view(torch.int16) if y.element_size() == 2 else y.view(torch.int32))
               for x, y in zip(xs, ys))


@pytest.mark.parametrize("epi", [F32, GELU, BF16, QKV], ids=[EPI_NAMES[e] for e in (F32, GELU, BF16, QKV)])
@pytest.mark.parametrize("mode", MODES)
def test_half_height_tile_equals_the_full_tile_and_the_128_kernel(d, gu, mode, epi):
    for N in ((384, 768) if epi == QKV else (256, 384)):
        for K in KS:
            w, bias = rnd(N, K, seed=N + K, scale=K ** -0.5), rnd(N, seed=N + K + 1)
            for M in MS:
                a = rnd(M, K, seed=M + K)
                resid = rnd(M, N, seed=M + N + 2) if epi == F32 else None
                with switches(d, gemm_tile=1):
                    ref = launch(d, gu, mode, epi, a, w, bias, resid)
                assert all((r != (gu.NAN_BF16 if r.element_size() == 2 else SENT)).any() for r in ref)  # (every output was written)
                for st, dr in FORMS:
                    with switches(d, gemm_tile=4, gemm_staged=st, gemm_direct=dr):
                        new = launch(d, gu, mode, epi, a, w, bias, resid)
                    with switches(d, gemm_tile=4, gemm_staged=st, gemm_direct=dr, gemm_debug=NO_HALF_HEIGHT):
                        full = launch(d, gu, mode, epi, a, w, bias, resid)
                    assert same(new, full), ("half-height != full tile", mode, EPI_NAMES[epi], (M, N, K), (st, dr))
                    assert same(new, ref), ("8-phase != 128x128", mode, EPI_NAMES[epi], (M, N, K), (st, dr))


@pytest.mark.parametrize("mode", MODES)
def test_half_height_tile_with_the_engines_row_maps(d, gu, mode):
    """(a) residual_gemm of a pruned block: B = 3 samples of n_tok = 197 rows keep their last 100, x[kept rows] += A W^T + bias in place -- 300 rows, the
    second row tile holds 44; (b) to_decoder: 2 x 190 rows into samples of 200 slots, the residual a table row picked by a permutation -- 380 rows, the
    second row tile holds 124.  Rows the launch does not own keep their value."""
    K = 384
    for N in (256, 384):
        w, bias = rnd(N, K, seed=N, scale=K ** -0.5), rnd(N, seed=N + 1)
        # (a)
        B, n_tok, n_out = 3, 197, 100
        a, x0 = rnd(B * n_out, K, seed=3), rnd(B * n_tok, N, seed=4)
        # (b)
        Bb, n_vis, slots = 2, 190, 200
        ab, table = rnd(Bb * n_vis, K, seed=5), rnd(slots, N, seed=6)
        perm = torch.stack([torch.randperm(slots, generator=torch.Generator().manual_seed(7 + b)) for b in range(Bb)]).to(torch.int32).cuda().contiguous()

        def both():
            x = x0.clone()
            run_gemm(d, gu, mode, F32, a, w, bias, C=x, ldc=N, resid=x, ldr=N, rows_in=n_out, rows_out=n_tok, out_row_offset=n_tok - n_out)
            C = torch.full((Bb * slots, N), SENT, device="cuda")
            run_gemm(d, gu, mode, F32, ab, w, None, C=C, ldc=N, resid=table, ldr=N, rows_in=n_vis, rows_out=slots, map_stride=slots, resid_rowmap=perm)
            return [x, C]

        with switches(d, gemm_tile=1):
            ref = both()
        kept = torch.zeros(B * n_tok, dtype=torch.bool)
        for b in range(B):
            kept[b * n_tok + n_tok - n_out:(b + 1) * n_tok] = True
        assert torch.equal(ref[0][~kept.cuda()], x0[~kept.cuda()]) and (ref[0][kept.cuda()] != x0[kept.cuda()]).any()
        assert (ref[1].view(Bb, slots, N)[:, n_vis:] == SENT).all() and (ref[1].view(Bb, slots, N)[:, :n_vis] != SENT).all()
        for st, dr in FORMS:
            with switches(d, gemm_tile=4, gemm_staged=st, gemm_direct=dr):
                new = both()
            with switches(d, gemm_tile=4, gemm_staged=st, gemm_direct=dr, gemm_debug=NO_HALF_HEIGHT):
                full = both()
            assert same(new, full) and same(new, ref), (mode, N, (st, dr))
