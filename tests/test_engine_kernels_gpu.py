"""The ViT engine's own launch forms one launch at a time, on a real MI355X, through the development library (include/cwm_hip_dev.h cwm_dev_gemm,
cwm_dev_attention, cwm_dev_layernorm, cwm_dev_fill_mask_tokens) against tests/engine_rows_restatement.py (float64; pinned to the model's semantics
by tests/test_engine_rows_cpu.py):

  GEMM       the Q/K/V scatter (EPI_QKV), EPI_BF16, the kept rows of the pruned last decoder block (rows_in / rows_out / out_row_offset, in place),
             the residual row map of embed_stream / to_decoder (resid_rowmap / map_stride), ldc > N -- over the tile configurations, the three
             epilogue forms and the small-launch kernels.  Small-integer operands make every fp32 result exact: equality, not a tolerance.
  attention  the query window (q_off, n_q) of the pruned block against the same rows of the full run and the dense softmax
  LayerNorm  the bf16 operand every consumer GEMM reads, the one-plane instantiation, mapped rows, D that is no multiple of 32
  fill_mask_tokens

Every output buffer is pre-filled with a sentinel and compared WHOLE: what must be written is right and everything else still holds the sentinel.
Every GEMM launch is preceded by a read-out of its plan (cwm_dev_gemm_plan under the switches the case set), held against the restated launcher
(tests/gemm_plan_restatement.py) and, for the default options, against the kernel / split-K count the case names."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import engine_rows_restatement as R
import gemm_plan_restatement as PR
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu

MODES = ("parity", "fast")
TOL = {"parity": 2e-4, "fast": 6e-2}  # tests/test_kernels_gpu.py: max-abs on O(1) outputs
F32, GELU, BF16, QKV = PR.EPI_F32, PR.EPI_BF16_GELU, PR.EPI_BF16, PR.EPI_QKV
K128, DEEP128, DEEP64, P8 = PR.KERNEL_128, PR.KERNEL_DEEP128, PR.KERNEL_DEEP64, PR.KERNEL_8PHASE
KERNEL_NAMES = {K128: "128x128", DEEP128: "deep128", DEEP64: "deep64", P8: "8phase"}
CUS = 256                # MI355X: what the named plans are stated for
SENT = -12345.75         # fp32 sentinel (exact in fp32): no sum of small integers and no O(1) random output equals it
DEFAULTS = {"gemm_tile": 0, "gemm_debug": 0, "gemm_staged": 1, "gemm_direct": 1, "attn_kernel": 0, "attn_tail": 1, "attn_ksplit": 1}
FORMS = ((0, 0), (1, 0), (1, 1), (1, 2))  # (gemm_staged, gemm_direct): per-fragment, LDS-staged, direct for bf16 outputs (default), direct everywhere


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
    """this thread's options of the development library for the duration of the block; the defaults afterwards, whatever happened inside"""
    try:
        for k, v in kw.items():
            _lib.check(d.cwm_debug_set(k.encode(), int(v)), d)
        yield
    finally:
        for k in kw:
            d.cwm_debug_set(k.encode(), DEFAULTS[k])


def planes_of(mode):
    return 2 if mode == "parity" else 1


def ints(*shape, seed, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def cuda(t):
    return None if t is None else t.cuda().contiguous()


def raw_equal(got, want):
    """bit equality of a device buffer and its expected image (any dtype of the same width)"""
    return torch.equal(got.view(torch.int16) if got.element_size() == 2 else got.view(torch.int32),
                       want.to(got.device).view(torch.int16) if want.element_size() == 2 else want.to(got.device).view(torch.int32))


# ---- the split-bf16 operand --------------------------------------------------------------------------------------------------------------------------
def operand_image(values, rows_total, ld, planes, gu):
    """expected raw image [rows_total][planes * ld] int16 of an operand buffer whose first values.shape[0] rows hold `values` (fp32 [rows][n], n <= ld) in
    columns [0, n), split exactly; everything else the sentinel of gpu_utils.new_operand"""
    rows, n = values.shape
    img = torch.full((rows_total, planes * ld), gu.NAN_BF16, dtype=torch.int16)
    hi, lo = R.split_bf16(values)
    hi_pos, lo_pos = R.operand_positions(ld, planes)
    img[:rows, torch.from_numpy(hi_pos[:n])] = gu.bits(hi)
    if planes == 2:
        img[:rows, torch.from_numpy(lo_pos[:n])] = gu.bits(lo)
    return img


def operand_values(raw, ld, planes, n, gu):
    """fp64 [rows][n] = hi (+ lo) of the first n columns of a raw operand buffer"""
    hi, lo = gu.decode(raw, planes, ld)
    v = hi.double()
    return (v + lo.double() if planes == 2 else v)[:, :n]


def test_bf16_conversion_is_round_to_nearest_even_like_torch(d, gu):
    """The claim the bitwise operand checks below rest on: common.h `(bf16)v` = torch's `.to(torch.bfloat16)`, and lo = bf16(v - hi) -- on ties, integers,
    values across the exponent range and random ones, through cwm_split_bf16"""
    g = torch.Generator().manual_seed(11)
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 255.5, 256.5, 257.5, -3.0078125, 1e-30, -3e30, 0.0, 65280.0, 65408.0])
    x = torch.cat([ties, torch.arange(-600, 601).float(), torch.randn(20000, generator=g), torch.randn(5000, generator=g) * 1e-3, torch.randn(5000, generator=g) * 6144,
                   torch.arange(-4 * 6144, 4 * 6144 + 1).float() * 0.125])
    xd = x.cuda()
    hi, lo = (torch.full((x.numel(),), gu.NAN_BF16, dtype=torch.int16, device="cuda") for _ in range(2))
    _lib.check(d.cwm_split_bf16(xd.data_ptr(), x.numel(), hi.data_ptr(), lo.data_ptr(), gu.stream()), d)
    torch.cuda.synchronize()
    want_hi, want_lo = R.split_bf16(x)
    assert raw_equal(hi, gu.bits(want_hi)) and raw_equal(lo, gu.bits(want_lo))


# ---- GEMM ----------------------------------------------------------------------------------------------------------------------------------------------
PLAN_LOG = []  # (case, mode, tile, debug, cfg, [(kernel, splitk)]) of every launch, printed once per test (pytest -s / -rP)


def expect_plan(d, what, M, N, K, epi, mode, tile=0, debug=0, want=None, nparts=None):
    """The plan the library reports for the launch about to be made (this thread's options are already set): equal to the restated launcher at 256 CUs
    and, where the case names them, to the kernels / split-K counts `want` = [(kernel, splitk or None = at least 3), ...]"""
    out = _lib.CwmDevGemmPlanOut()
    Kp = -(-K // 64) * 64
    _lib.check(d.cwm_dev_gemm_plan(M, N, Kp, epi, _lib.mode_id(mode), 0, 0, 0, ctypes.byref(out)), d)
    got = (out.cfg, [(q.kernel, q.splitk) for q in out.part[:out.nparts]])
    cfg, parts = PR.plan(M, N, Kp, epi, planes_of(mode), 0, CUS, tile, debug)
    assert got == (cfg, [(q[2], q[3]) for q in parts]), (what, mode, tile, debug, got)
    if want is not None:
        assert len(want) == len(got[1]) and all(k == wk and (s >= 3 if ws is None else s == ws) for (k, s), (wk, ws) in zip(got[1], want)), (what, mode, got, want)
    if nparts is not None and tile == 6:
        assert out.nparts == nparts, (what, mode, tile, got)
    PLAN_LOG.append((what, mode, tile, debug, got[0], got[1]))
    return got


def print_plans(title):
    seen = {}
    for what, mode, tile, debug, cfg, parts in PLAN_LOG:
        seen.setdefault((what, mode, cfg, tuple(parts)), []).append((tile, debug))
    for (what, mode, cfg, parts), opts in seen.items():
        print("PLAN %s | %s %s | cfg %d %s | (gemm_tile, gemm_debug) %s" % (title, what, mode, cfg, " + ".join("%s x%d" % (KERNEL_NAMES[k], s) for k, s in parts),
                                                                               sorted(set(opts))))
    del PLAN_LOG[:]


def run_gemm(d, gu, mode, epi, a, w, bias, **fields):
    """one cwm_dev_gemm call on device tensors; the other cwm_dev_gemm_args fields by name (tensors as pointers).  Returns the plan's (staged, direct)"""
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
    return forms[0], forms[1]


def variants(M, N, extra=()):
    """(gemm_tile, gemm_staged, gemm_direct, gemm_debug): the default; every tile configuration x every epilogue form; for a small launch (no more 128x128
    tiles than CUs) the double-buffered kernel, the deep ring without split-K, its 128-row form; `extra`"""
    out = [(0, 1, 1, 0)] + [(t, s, dr, 0) for t in (1, 4, 6) for s, dr in FORMS]
    if -(-M // 128) * -(-N // 128) <= CUS:
        out += [(1, s, dr, dbg) for dbg in (4, 32, 32 + 256) for s, dr in ((0, 0), (1, 1))]
    return out + list(extra)


def qkv_case(d, gu, mode, B, n_tok, H, hd, K, seed, var, want=None, nparts=None, staged=None):
    """EPI_QKV on exact operands under every variant: the three [B * H, n_tok, hd] outputs (hi, and lo in parity mode) equal the exact split of the
    float64 result bit for bit, the guard elements behind them still hold the sentinel"""
    planes, D = planes_of(mode), H * hd
    M, N, guard = B * n_tok, 3 * D, 192
    a, w, bias = ints(M, K, seed=seed), ints(N, K, seed=seed + 1), ints(N, seed=seed + 2, lo=-9, hi=9)
    y = R.linear64(a, w, bias).float()
    assert (y.double() == R.linear64(a, w, bias)).all()  # exact in fp32
    count = M * D
    want_img = []
    for t in R.qkv_scatter(y, B, n_tok, H, hd, 0.125):
        img = torch.full((planes, count + guard), gu.NAN_BF16, dtype=torch.int16)
        hi, lo = R.split_bf16(t.reshape(-1))
        img[0, :count] = gu.bits(hi)
        if planes == 2:
            img[1, :count] = gu.bits(lo)
        want_img.append(img.cuda())
    ad, wd, bd = cuda(a), cuda(w), cuda(bias)
    what = "qkv B=%d n_tok=%d D=%d hd=%d K=%d" % (B, n_tok, D, hd, K)
    for tile, st, dr, dbg in var:
        with switches(d, gemm_tile=tile, gemm_staged=st, gemm_direct=dr, gemm_debug=dbg):
            expect_plan(d, what, M, N, K, QKV, mode, tile, dbg, want if (tile, dbg) == (0, 0) else None, nparts)
            bufs = [torch.full((planes, count + guard), gu.NAN_BF16, dtype=torch.int16, device="cuda") for _ in range(3)]
            forms = run_gemm(d, gu, mode, QKV, ad, wd, bd, rows_in=n_tok, rows_out=n_tok, map_stride=n_tok, q_out=bufs[0], k_out=bufs[1], v_out=bufs[2],
                             qk_plane=count + guard, heads=H, head_dim=hd, n_tok=n_tok, q_scale=0.125)
            if staged is not None:
                assert forms[0] == (staged and st), (what, forms)
            for name, got, img in zip("qkv", bufs, want_img):
                assert raw_equal(got, img), (what, mode, name, (tile, st, dr, dbg), (got != img).nonzero()[:4].tolist())


# D, H, head_dim, and the plan the default options must reach per (B, n_tok) in (parity, fast): [(kernel, splitk)]
QKV_ROWS = [(5, 40), (3, 197), (1, 792), (2, 1100)]
QKV_SHAPES = [
    (64, 1, 64, {(5, 40): [(DEEP64, 1)], (3, 197): [(DEEP64, 1)], (1, 792): [(DEEP64, 1)], (2, 1100): [(DEEP64, 1)]}),
    (192, 3, 64, {(5, 40): [(DEEP64, 1)], (3, 197): [(DEEP64, 1)], (1, 792): [(DEEP64, 1)], (2, 1100): [(DEEP64, 1)]}),
    (320, 5, 64, {(5, 40): [(DEEP64, 1)], (3, 197): [(DEEP64, 1)], (1, 792): [(DEEP64, 1)], (2, 1100): [(DEEP128, 1)]}),
    (384, 6, 64, {(5, 40): [(DEEP64, 1)], (3, 197): [(DEEP64, 1)], (1, 792): [(DEEP64, 1)], (2, 1100): [(DEEP128, 1)]}),
    (96, 3, 32, {(5, 40): [(DEEP64, 1)], (3, 197): [(DEEP64, 1)], (1, 792): [(DEEP64, 1)], (2, 1100): [(DEEP64, 1)]}),
    (48, 3, 16, {(5, 40): [(DEEP64, 1)], (3, 197): [(DEEP64, 1)], (1, 792): [(DEEP64, 1)], (2, 1100): [(DEEP64, 1)]}),
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D,H,hd,wants", QKV_SHAPES, ids=["D%d_hd%d" % (s[0], s[2]) for s in QKV_SHAPES])
def test_gemm_qkv_scatter_is_exact(d, gu, mode, D, H, hd, wants):
    """The first GEMM of every block.  D = 192: the 128-column tile 128..255 straddles the Q / K boundary; D = 320, 384: a last column tile of 192 / 128
    columns in the 8-phase kernel (the half-width instance for 128; "gemm_debug" 1024 takes it away); head_dim 32 is staged, head_dim 16 must take the
    per-fragment form; rows such that tiles straddle samples"""
    for B, n_tok in QKV_ROWS:
        extra = [(4, 1, 1, 1024), (0, 1, 1, 1024)] if D in (320, 384) else []
        qkv_case(d, gu, mode, B, n_tok, H, hd, D, 100 + D, variants(B * n_tok, 3 * D, extra), want=wants[(B, n_tok)], staged=(hd % 32 == 0))
    print_plans("qkv")


@pytest.mark.parametrize("mode", MODES)
def test_gemm_qkv_scatter_mixed_tiling_is_exact(d, gu, mode):
    """22064 rows = 87 row tiles of 256: one whole round of 8-phase tiles on 256 CUs (3 column tiles: 85 row tiles) and a remainder on 128x128 tiles, samples
    of 197 rows straddling every tile and the seam between the two launches"""
    var = [(6, 1, 1, 0), (6, 0, 0, 0), (6, 1, 0, 0), (1, 1, 1, 0)]  # (the last: 865 tiles of 128x128 on the 2-stage ring, two workgroups per CU)
    qkv_case(d, gu, mode, 112, 197, 3, 64, 192, 77, var, nparts=2)
    assert {k for _, _, tile, _, _, parts in PLAN_LOG for k, _ in parts} == {P8, DEEP64, K128}
    print_plans("qkv mixed")


KEPT = [(3, 197, 100), (2, 792, 396), (5, 40, 1), (1, 1568, 784), (9, 300, 129)]
KEPT_WANT = {  # (M, N) -> the default plan, the same in both modes at K = 128
    (300, 384): [(DEEP64, 1)], (792, 384): [(DEEP64, 1)], (5, 384): [(DEEP128, 1)], (784, 384): [(DEEP64, 1)], (1161, 384): [(DEEP64, 1)],
    (300, 768): [(DEEP64, 1)], (792, 768): [(DEEP64, 1)], (5, 768): [(DEEP128, 1)], (784, 768): [(DEEP64, 1)], (1161, 768): [(DEEP64, 1)],
}


def f32_case(d, gu, mode, what, a, w, bias, C0, resid, var, K, want=None, in_place=False, **fields):
    """EPI_F32 on exact operands under every variant: the whole output surface equals R.gemm_f32 of its initial state (rows and columns the launch does
    not own unchanged).  `in_place`: resid is the output buffer itself"""
    M, N = a.shape[0], w.shape[0]
    rows = {k: fields[k] for k in ("rows_in", "rows_out", "out_row_offset", "map_stride") if k in fields}
    rowmap = fields.get("resid_rowmap")
    want_C = R.gemm_f32(a, w, bias, C0, resid=C0 if in_place else resid, resid_rowmap=None if rowmap is None else rowmap.numpy(), **rows)
    assert (want_C.float().double() == want_C).all()
    want_C = want_C.float().cuda()
    ad, wd, bd, C0d = cuda(a), cuda(w), cuda(bias), cuda(C0)
    rd = None if in_place or resid is None else cuda(resid)
    dev_fields = dict(fields)
    if rowmap is not None:
        dev_fields["resid_rowmap"] = rowmap.to(torch.int32).cuda()
    for tile, st, dr, dbg in var:
        with switches(d, gemm_tile=tile, gemm_staged=st, gemm_direct=dr, gemm_debug=dbg):
            expect_plan(d, what, M, N, K, F32, mode, tile, dbg, want if (tile, dbg) == (0, 0) else None)
            Cd = C0d.clone()
            run_gemm(d, gu, mode, F32, ad, wd, bd, C=Cd, resid=Cd if in_place else rd, **dev_fields)
            assert torch.equal(Cd, want_C), (what, mode, (tile, st, dr, dbg), (Cd != want_C).nonzero()[:4].tolist())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", [384, 768])
def test_gemm_kept_rows_in_place_are_exact(d, gu, mode, N):
    """residual_gemm of the pruned last decoder block: x[kept rows] += A W^T + bias with C == resid; rows [0, first) of every sample bit-unchanged"""
    K = 128
    for B, n_tok, n_out in KEPT:
        a, w, bias = ints(B * n_out, K, seed=n_tok), ints(N, K, seed=n_tok + 1), ints(N, seed=n_tok + 2, lo=-9, hi=9)
        x = ints(B * n_tok, N, seed=n_tok + 3, lo=-50, hi=50)
        f32_case(d, gu, mode, "kept B=%d n_tok=%d n_out=%d N=%d K=%d" % (B, n_tok, n_out, N, K), a, w, bias, x, None, variants(B * n_out, N), K,
                 want=KEPT_WANT[(B * n_out, N)], in_place=True, ldc=N, ldr=N, **R.kept_rows(n_tok, n_out))
    print_plans("kept rows")


@pytest.mark.parametrize("mode", MODES)
def test_gemm_kept_rows_deep_ring_split_k_is_exact(d, gu, mode):
    """the same form on the kernel the batch-1 decoder takes: 64x128 tiles of the 4-stage ring with K cut in at least three ranges (integers stay exact under
    the re-associated sum), and with the split switched off"""
    B, n_tok, n_out, N, K = 2, 197, 100, 384, 2304
    a, w, bias = ints(B * n_out, K, seed=5), ints(N, K, seed=6), ints(N, seed=7, lo=-9, hi=9)
    x = ints(B * n_tok, N, seed=8, lo=-50, hi=50)
    var = [(0, 1, 1, 0), (0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 2, 0), (0, 1, 1, 256), (0, 1, 1, 32), (0, 1, 1, 4)]
    f32_case(d, gu, mode, "kept split-K B=%d n_tok=%d n_out=%d N=%d K=%d" % (B, n_tok, n_out, N, K), a, w, bias, x, None, var, K, want=[(DEEP64, None)],
             in_place=True, ldc=N, ldr=N, **R.kept_rows(n_tok, n_out))
    print_plans("kept rows split-K")


@pytest.mark.parametrize("mode", MODES)
def test_gemm_kept_rows_column_slice_is_exact(d, gu, mode):
    """ldc = ldr > N with mapped rows (the RAFT slice test covers identity rows): columns [N, ldc) of every row keep the sentinel"""
    B, n_tok, n_out, N, K, ld = 3, 197, 100, 384, 128, 384 + 64
    a, w, bias = ints(B * n_out, K, seed=15), ints(N, K, seed=16), ints(N, seed=17, lo=-9, hi=9)
    x = torch.full((B * n_tok, ld), SENT)
    x[:, :N] = ints(B * n_tok, N, seed=18, lo=-50, hi=50)
    f32_case(d, gu, mode, "kept slice ldc=%d N=%d" % (ld, N), a, w, bias, x, None, variants(B * n_out, N), K, want=[(DEEP64, 1)], in_place=True, ldc=ld, ldr=ld,
             **R.kept_rows(n_tok, n_out))
    print_plans("kept rows, ldc > N")


ROWMAP = [(3, 100, 197, 16), (2, 396, 792, 40), (5, 13, 40, 8)]  # B, n_vis, n_tok, pad slots
ROWMAP_WANT = {(300, 384): [(DEEP64, 1)], (792, 384): [(DEEP64, 1)], (65, 384): [(DEEP64, 1)]}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("to_decoder", [False, True], ids=["embed_stream", "to_decoder"])
def test_gemm_residual_row_map_is_exact(d, gu, mode, to_decoder):
    """The positional-table gather: out[b][i] = a w^T + table[perm[b][i]], perm a random permutation of the n_tok + pad slots of an extended table (some
    visible entries point at pad slots).  embed_stream: rows_out == rows_in; to_decoder: rows_out = the slot count, rows [n_vis, slots) of every sample untouched"""
    N, K = 384, 192
    for B, n_vis, n_tok, pad in ROWMAP:
        slots = n_tok + pad
        g = torch.Generator().manual_seed(n_tok)
        perm = torch.stack([torch.randperm(slots, generator=g) for _ in range(B)])
        perm[0, 0] = slots - 1  # a pad slot, and the table's last row
        assert (perm[:, :n_vis] >= n_tok).any() and slots > n_vis
        a, w = ints(B * n_vis, K, seed=n_tok + 1), ints(N, K, seed=n_tok + 2)
        table = ints(slots, N, seed=n_tok + 3, lo=-50, hi=50)
        rows_out = slots if to_decoder else n_vis
        C0 = torch.full((B * rows_out, N), SENT)
        f32_case(d, gu, mode, "rowmap %s B=%d n_vis=%d slots=%d" % ("to_decoder" if to_decoder else "embed", B, n_vis, slots), a, w, None, C0, table,
                 variants(B * n_vis, N), K, want=ROWMAP_WANT[(B * n_vis, N)], ldc=N, ldr=N, rows_in=n_vis, rows_out=rows_out, map_stride=slots,
                 resid_rowmap=perm.reshape(-1))
    print_plans("residual row map")


@pytest.mark.parametrize("mode", MODES)
def test_gemm_bf16_operand_output_is_exact(d, gu, mode):
    """EPI_BF16 (Engine::linear_operand) with identity and kept rows, ldo = N and N + 32 -- and, in fast mode, an ldo that is no multiple of 8, which must take the
    per-fragment form: the operand equals the exact split bit for bit, the pad columns and the rows behind the last hold the sentinel"""
    planes = planes_of(mode)
    for (M, N, K, rows, R_total) in [(300, 384, 128, {}, 304), (200, 288, 192, R.kept_rows(197, 100), 2 * 197 + 3), (792, 768, 64, {}, 792)]:
        a, w, bias = ints(M, K, seed=M), ints(N, K, seed=M + 1), ints(N, seed=M + 2, lo=-9, hi=9)
        y = R.linear64(a, w, bias).float()
        out_rows, _ = R.row_maps(M, **rows)
        ad, wd, bd = cuda(a), cuda(w), cuda(bias)
        for ldo in (N, N + 32) + ((N + 4,) if mode == "fast" else ()):
            full = torch.zeros(R_total, N)
            full[out_rows] = y
            img = operand_image(full, R_total, ldo, planes, gu)
            untouched = torch.ones(R_total, dtype=torch.bool)
            untouched[out_rows] = False
            img[untouched] = gu.NAN_BF16
            img = img.cuda()
            what = "bf16 M=%d N=%d K=%d ldo=%d%s" % (M, N, K, ldo, " kept rows" if rows else "")
            for tile, st, dr, dbg in variants(M, N):
                with switches(d, gemm_tile=tile, gemm_staged=st, gemm_direct=dr, gemm_debug=dbg):
                    expect_plan(d, what, M, N, K, BF16, mode, tile, dbg)
                    out = gu.new_operand(R_total, ldo, planes)
                    forms = run_gemm(d, gu, mode, BF16, ad, wd, bd, out=out, ldo=ldo, **rows)
                    assert forms[0] == (st if ldo % 8 == 0 else 0), (what, forms)
                    assert raw_equal(out, img), (what, mode, (tile, st, dr, dbg), (out != img).nonzero()[:4].tolist())
    print_plans("bf16 operand")


def test_gemm_refuses_before_launching(d, gu):
    """what cwm_dev_gemm and the plan refuse comes back as an error with the output untouched"""
    a, w = cuda(ints(40, 64, seed=1)), cuda(ints(48, 64, seed=2))
    C0 = torch.full((80, 48), SENT, device="cuda")
    out = gu.new_operand(40, 40, 2)
    for mode, epi, fields, text in [
        ("parity", F32, dict(C=C0, ldc=48, rows_in=7, rows_out=7), b"samples of 7 rows"),           # M % rows_in
        ("parity", F32, dict(C=C0, ldc=48, rows_in=20, rows_out=30, out_row_offset=11), b"offset"),  # the offset rows leave the sample
        ("parity", F32, dict(C=C0, ldc=32), b"at least N columns"),
        ("parity", F32, dict(C=C0, ldc=48, out_row_offset=3), b"rows_in > 0"),
        ("parity", BF16, dict(out=out, ldo=48 + 8), b"multiple of 32"),                              # gemm_plan's own refusal
        ("fast", QKV, dict(q_out=out, k_out=out, v_out=out, heads=1, head_dim=16, n_tok=7, rows_in=8, rows_out=8), b"whole samples"),
    ]:
        with pytest.raises(_lib.CwmHipError) as e:
            run_gemm(d, gu, mode, epi, a, w, None, **fields)
        assert text in str(e.value).encode(), (fields, str(e.value))
    torch.cuda.synchronize()
    assert (C0 == SENT).all() and (out == gu.NAN_BF16).all()


@pytest.mark.parametrize("mode", MODES)
def test_gemm_row_maps_on_random_data(d, gu, mode):
    """The same row maps on N(0, 1) data against float64, at the tolerances of tests/test_kernels_gpu.py; EPI_BF16_GELU with a row offset; across tile
    configurations and epilogue forms the outputs are bit-identical; with and without split-K they are deterministic under repetition"""
    planes = planes_of(mode)
    # ---- fp32: kept rows in place, and the residual row map into a wider sample ----
    for (B, n_tok, n_out, N, K) in [(3, 197, 100, 384, 384), (2, 792, 396, 768, 192), (9, 300, 129, 384, 768)]:
        M = B * n_out
        a, w, bias = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3)
        x = rnd(B * n_tok, N, seed=4)
        rows = R.kept_rows(n_tok, n_out)
        ref = R.gemm_f32(a, w, bias, x, resid=x, **rows)
        ad, wd, bd, xd = cuda(a), cuda(w), cuda(bias), cuda(x)
        first = None
        for tile, st, dr, dbg in [(0, 1, 1, 32)] + [(t, s, r, 32) for t in (1, 4, 6) for s, r in FORMS]:   # (no split-K: a split re-associates the fp32 sum)
            with switches(d, gemm_tile=tile, gemm_staged=st, gemm_direct=dr, gemm_debug=dbg):
                expect_plan(d, "random kept M=%d N=%d K=%d" % (M, N, K), M, N, K, F32, mode, tile, dbg)
                C = xd.clone()
                run_gemm(d, gu, mode, F32, ad, wd, bd, C=C, ldc=N, resid=C, ldr=N, **rows)
                first = C if first is None else first
                assert torch.equal(C, first), (mode, M, N, K, (tile, st, dr, dbg))
        err = (first.cpu().double() - ref).abs().max().item()
        print("random kept rows M=%d N=%d K=%d %s: max-abs error %.3e" % (M, N, K, mode, err))
        assert err <= TOL[mode], (mode, M, N, K, err)
    # ---- split-K on / off: deterministic, both within the tolerance ----
    B, n_tok, n_out, N, K = 2, 197, 100, 384, 2304
    M = B * n_out
    a, w, bias, x = rnd(M, K, seed=5), rnd(N, K, seed=6, scale=K ** -0.5), rnd(N, seed=7), rnd(B * n_tok, N, seed=8)
    rows = R.kept_rows(n_tok, n_out)
    ref = R.gemm_f32(a, w, bias, x, resid=x, **rows)
    ad, wd, bd, xd = cuda(a), cuda(w), cuda(bias), cuda(x)
    for dbg, want in ((0, [(DEEP64, None)]), (32, [(DEEP64, 1)])):
        with switches(d, gemm_debug=dbg):
            expect_plan(d, "random kept split-K M=%d N=%d K=%d" % (M, N, K), M, N, K, F32, mode, 0, dbg, want)
            outs = []
            for rep in range(4):
                C = xd.clone()
                run_gemm(d, gu, mode, F32, ad, wd, bd, C=C, ldc=N, resid=C, ldr=N, **rows)
                outs.append(C)
            assert all(torch.equal(o, outs[0]) for o in outs[1:]), (mode, dbg, "not deterministic")
            err = (outs[0].cpu().double() - ref).abs().max().item()
            print("random kept rows split-K gemm_debug=%d %s: max-abs error %.3e" % (dbg, mode, err))
            assert err <= TOL[mode], (mode, dbg, err)
    # ---- the residual row map ----
    B, n_vis, n_tok, pad, N, K = 3, 100, 197, 16, 384, 192
    slots = n_tok + pad
    perm = torch.stack([torch.randperm(slots, generator=torch.Generator().manual_seed(b)) for b in range(B)])
    a, w, table = rnd(B * n_vis, K, seed=9), rnd(N, K, seed=10, scale=K ** -0.5), rnd(slots, N, seed=11)
    C0 = torch.full((B * slots, N), SENT)
    ref = R.gemm_f32(a, w, None, C0, resid=table, rows_in=n_vis, rows_out=slots, resid_rowmap=perm.reshape(-1).numpy(), map_stride=slots)
    ad, wd, td, pd = cuda(a), cuda(w), cuda(table), perm.reshape(-1).to(torch.int32).cuda()
    first = None
    for tile, st, dr, dbg in [(0, 1, 1, 32)] + [(t, s, r, 32) for t in (1, 4) for s, r in FORMS]:
        with switches(d, gemm_tile=tile, gemm_staged=st, gemm_direct=dr, gemm_debug=dbg):
            expect_plan(d, "random rowmap M=%d N=%d K=%d" % (B * n_vis, N, K), B * n_vis, N, K, F32, mode, tile, dbg)
            C = cuda(C0)
            run_gemm(d, gu, mode, F32, ad, wd, None, C=C, ldc=N, resid=td, ldr=N, rows_in=n_vis, rows_out=slots, map_stride=slots, resid_rowmap=pd)
            first = C if first is None else first
            assert torch.equal(C, first), (mode, "rowmap", (tile, st, dr, dbg))
    got = first.cpu().double()
    assert (got - ref).abs().max().item() <= TOL[mode] and (got.reshape(B, slots, N)[:, n_vis:] == SENT).all()
    # ---- EPI_BF16_GELU with a row offset, and the Q/K/V scatter ----
    B, n_tok, n_out, N, K = 3, 197, 100, 768, 384
    M = B * n_out
    a, w, bias = rnd(M, K, seed=12), rnd(N, K, seed=13, scale=K ** -0.5), rnd(N, seed=14)
    rows = R.kept_rows(n_tok, n_out)
    out_rows, _ = R.row_maps(M, **rows)
    ref = R.gelu64(R.linear64(a, w, bias))
    ad, wd, bd = cuda(a), cuda(w), cuda(bias)
    first = None
    for tile, st, dr, dbg in [(0, 1, 1, 32)] + [(t, s, r, 32) for t in (1, 4) for s, r in FORMS]:
        with switches(d, gemm_tile=tile, gemm_staged=st, gemm_direct=dr, gemm_debug=dbg):
            expect_plan(d, "random gelu M=%d N=%d K=%d" % (M, N, K), M, N, K, GELU, mode, tile, dbg)
            out = gu.new_operand(B * n_tok, N + 32, planes)
            run_gemm(d, gu, mode, GELU, ad, wd, bd, out=out, ldo=N + 32, **rows)
            first = out if first is None else first
            assert torch.equal(out, first), (mode, "gelu", (tile, st, dr, dbg))
    raw = first.cpu()
    err = (operand_values(raw, N + 32, planes, N, gu)[out_rows] - ref).abs().max().item()
    print("random gelu kept rows %s: max-abs error %.3e" % (mode, err))
    assert err <= TOL[mode], (mode, err)
    untouched = torch.ones(B * n_tok, dtype=torch.bool)
    untouched[out_rows] = False
    assert (raw[untouched] == gu.NAN_BF16).all()
    hi_pos, lo_pos = R.operand_positions(N + 32, planes)
    pad_cols = np.concatenate([hi_pos[N:]] + ([lo_pos[N:]] if planes == 2 else []))
    assert (raw[:, torch.from_numpy(pad_cols)] == gu.NAN_BF16).all()
    B, n_tok, H = 3, 197, 3
    D, M = 64 * H, B * n_tok
    a, w, bias = rnd(M, D, seed=15), rnd(3 * D, D, seed=16, scale=D ** -0.5), rnd(3 * D, seed=17)
    want = R.qkv_scatter(R.linear64(a, w, bias), B, n_tok, H, 64, 0.125)
    ad, wd, bd = cuda(a), cuda(w), cuda(bias)
    first = None
    for tile, st, dr, dbg in [(0, 1, 1, 32)] + [(t, s, r, 32) for t in (1, 4) for s, r in FORMS]:
        with switches(d, gemm_tile=tile, gemm_staged=st, gemm_direct=dr, gemm_debug=dbg):
            expect_plan(d, "random qkv M=%d D=%d" % (M, D), M, 3 * D, D, QKV, mode, tile, dbg)
            bufs = [torch.full((planes, M * D), gu.NAN_BF16, dtype=torch.int16, device="cuda") for _ in range(3)]
            run_gemm(d, gu, mode, QKV, ad, wd, bd, rows_in=n_tok, rows_out=n_tok, map_stride=n_tok, q_out=bufs[0], k_out=bufs[1], v_out=bufs[2], qk_plane=M * D,
                     heads=H, head_dim=64, n_tok=n_tok, q_scale=0.125)
            first = bufs if first is None else first
            assert all(torch.equal(x_, y_) for x_, y_ in zip(bufs, first)), (mode, "qkv", (tile, st, dr, dbg))
    for got, ref in zip(first, want):
        v = got.cpu().view(torch.bfloat16).double().sum(0).reshape(ref.shape)  # hi + lo
        assert (v - ref).abs().max().item() <= TOL[mode], (mode, "qkv")
    print_plans("random data")


# ---- attention: the query window ---------------------------------------------------------------------------------------------------------------------
def run_attention(d, gu, mode, qkv_d, B, N, H, q_off, n_q, ldo, rows_total):
    planes = planes_of(mode)
    o = gu.new_operand(rows_total, ldo, planes)
    g = _lib.new_dev_conj_args(_lib.CwmDevAttentionArgs)
    g.mode, g.qkv, g.B, g.N, g.H, g.q_off, g.n_q = _lib.mode_id(mode), qkv_d.data_ptr(), B, N, H, q_off, n_q
    g.o, g.ldo, g.stream = o.data_ptr(), ldo, gu.stream()
    _lib.check(d.cwm_dev_attention(ctypes.byref(g)), d)
    return o


def window_schedule(mode, kern, N, n_q, items):
    """what launch_attention does with the window under the default switches (csrc/attention.hip, attention_pipe.hip): (ragged-tile key split, key-split round)"""
    nqb = -(-n_q // 128)
    last = n_q - (nqb - 1) * 128
    tail = nqb > 1 and last <= 32 and N > 128
    rem = items % (2 * CUS)
    parts = min(8, (2 * CUS) // rem) if rem else 0
    nkt = -(-N // 64)
    while parts > 1 and nkt // parts < 6:
        parts -= 1
    ksplit = kern == 3 and items >= 2 * CUS and 0 < rem <= 2 * CUS // 4 and not tail and parts >= 2
    return tail, ksplit


# B, N, H, q_off, n_q.  n_q = 1 (3, 200, 1, 199, 1); n_q < 128 (100); n_q % 128 in 1..32 -- 129, 396 = 3 x 128 + 12, 784 = 6 x 128 + 16: the ragged-tile
# key split -- and in 33..127 (600, 680: not); n_q % 128 == 0 (256); q_off no multiple of 16 (171, 199, 500, 344, 88); q_off + n_q == N (all but two);
# q_off = 0 with n_q < N; a chip-filling grid (8, 792, 12); and (43, 768, 2, 88, 680): 6 query tiles x 86 (batch, head) pairs = 516 work items = one round of
# 512 slots + 4, the last tile 40 rows, 12 key tiles -> the key-split round of the pipelined kernel (2 ranges of 6 tiles)
WINDOWS = [(2, 300, 2, 171, 129), (1, 792, 3, 396, 396), (3, 200, 1, 199, 1), (2, 1100, 2, 500, 600), (1, 1568, 2, 784, 784), (2, 300, 2, 0, 100),
           (2, 600, 1, 344, 256), (8, 792, 12, 396, 396), (43, 768, 2, 88, 680)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,N,H,q_off,n_q", WINDOWS, ids=["-".join(map(str, c)) for c in WINDOWS])
def test_attention_query_window(d, gu, mode, B, N, H, q_off, n_q):
    """The pruned block's attention: queries [q_off, q_off + n_q) of every sample against all N keys, O as [B * n_q] compact operand rows.  For both kernels:
    on the regular schedule the rows are bit-identical to the same rows of the full run (the engine's claim at run_block); with the default schedule -- the
    window decides which rows form the ragged last tile and how many work items the last round holds -- within the bounds of
    test_attention_key_split_of_the_ragged_last_tile; always within the dense-softmax bound; rows and columns outside the window's hold the sentinel"""
    planes, D = planes_of(mode), 64 * H
    ldo, extra_rows = D + 32, 5
    qkv = rnd(B, N, 3 * D, seed=N + n_q)
    spike_q = q_off + min(7, n_q - 1)
    qkv[0, N - 5, D:D + 64] = qkv[0, spike_q, :64] * 6.0  # a late spike, in the last key tile, for a query inside the window (head 0)
    ref = R.attention_window(qkv, H, q_off, n_q)
    qd = cuda(qkv)
    hi_pos, lo_pos = R.operand_positions(ldo, planes)
    used = torch.from_numpy(np.concatenate([hi_pos[:D]] + ([lo_pos[:D]] if planes == 2 else [])))
    pad = torch.from_numpy(np.concatenate([hi_pos[D:]] + ([lo_pos[D:]] if planes == 2 else [])))
    for kern in (1, 3):
        with switches(d, attn_kernel=kern, attn_tail=0, attn_ksplit=0):
            full = run_attention(d, gu, mode, qd, B, N, H, 0, 0, ldo, B * N)
            win = run_attention(d, gu, mode, qd, B, N, H, q_off, n_q, ldo, B * n_q + extra_rows)
        want = full.view(B, N, planes * ldo)[:, q_off:q_off + n_q].reshape(B * n_q, planes * ldo)
        assert torch.equal(win[:B * n_q], want), (mode, kern, (win[:B * n_q] != want).nonzero()[:4].tolist())
        assert (win[B * n_q:] == gu.NAN_BF16).all() and (win[:, pad] == gu.NAN_BF16).all() and (win[:B * n_q][:, used] != gu.NAN_BF16).any()
        with switches(d, attn_kernel=kern):
            dflt = run_attention(d, gu, mode, qd, B, N, H, q_off, n_q, ldo, B * n_q + extra_rows)
            again = run_attention(d, gu, mode, qd, B, N, H, q_off, n_q, ldo, B * n_q + extra_rows)
        assert torch.equal(dflt, again), (mode, kern, "not deterministic")
        assert (dflt[B * n_q:] == gu.NAN_BF16).all() and (dflt[:, pad] == gu.NAN_BF16).all()
        v_reg = operand_values(win.cpu()[:B * n_q], ldo, planes, D, gu)
        v_def = operand_values(dflt.cpu()[:B * n_q], ldo, planes, D, gu)
        diff = (v_def - v_reg).abs().reshape(B, n_q, D)
        changed = (diff.amax(-1) > 0)
        assert diff.max().item() <= (1e-4 if mode == "parity" else 1e-2), (mode, kern, diff.max().item())
        items = -(-n_q // 128) * B * H
        tail, ksplit = window_schedule(mode, kern, N, n_q, items)
        tail0 = (n_q - 1) // 128 * 128
        print("WINDOW %s kernel %d (B, N, H, q_off, n_q) = %s: ragged-tile key split %s, key-split round %s; %d rows differ from the regular schedule (max %.2e)"
              % (mode, kern, (B, N, H, q_off, n_q), tail, ksplit, int(changed.sum()), diff.max().item()))
        if tail:
            assert not changed[:, :tail0].any(), (mode, kern, "rows of whole tiles changed")   # only the ragged tile runs the other schedule ...
            assert changed.any() or mode == "fast" or n_q - tail0 == 1                          # ... and it really ran (a re-associated sum seldom keeps every bit)
        elif ksplit:
            assert 0 < int(changed.sum()) <= (items % (2 * CUS)) * 128, (mode, kern, int(changed.sum()))
        else:
            assert not changed.any(), (mode, kern, "no split applies to this window, yet rows differ")
        for name, v in (("regular", v_reg), ("default", v_def)):
            err = (v.reshape(B, n_q, D) - ref).abs().max().item()
            print("WINDOW %s kernel %d %s schedule: max-abs error against the dense softmax %.3e" % (mode, kern, name, err))
            assert err <= (3e-4 if mode == "parity" else 3e-2), (mode, kern, name, err)


def test_attention_window_refusals(d, gu):
    qd = cuda(rnd(1, 40, 192, seed=1))
    for mode, q_off, n_q, ldo in [("parity", 30, 11, 64), ("parity", 0, 8, 72), ("fast", 0, 8, 48), ("parity", 5, 0, 64)]:
        with pytest.raises(_lib.CwmHipError):
            run_attention(d, gu, mode, qd, 1, 40, 1, q_off, n_q, ldo, 40)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------------------------
LN_MAPS = [(0, 0, 0, 37), (100, 197, 97, 300), (1, 40, 39, 5), (396, 792, 396, 396)]  # rows_out_per_b, rows_in_per_b, in_offset, rows (37, 5: no multiple of 4)


def run_layernorm(d, gu, mode, xd, gd, bd, D, ldx, rows, rowmap, ldo, rows_total, with_f32):
    planes = planes_of(mode)
    out = gu.new_operand(rows_total, ldo, planes)
    f32 = torch.full((rows_total, D), SENT, device="cuda") if with_f32 else None
    g = _lib.new_dev_conj_args(_lib.CwmDevLayernormArgs)
    g.mode, g.x, g.ldx, g.gamma, g.beta, g.eps = _lib.mode_id(mode), xd.data_ptr(), ldx, gd.data_ptr(), bd.data_ptr(), 1e-6
    g.D, g.rows, (g.rows_out_per_b, g.rows_in_per_b, g.in_offset) = D, rows, rowmap
    g.out, g.ldo, g.out_f32, g.stream = out.data_ptr(), ldo, _lib.ptr(f32), gu.stream()
    rc = d.cwm_dev_layernorm(ctypes.byref(g))
    return rc, out, f32


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [8, 40, 200, 384, 520, 768, 1000, 1024])
def test_layernorm_operand_and_row_map(d, gu, mode, D):
    """launch_layernorm as run_mlp / head_rows call it.  The fp32 copy is within 5e-6 of the float64 LayerNorm of the MAPPED input rows; the bf16 operand --
    what every consumer GEMM reads -- is the exact split of that copy bit for bit, with and without the copy, in two planes and in one; columns [D, ldo)
    and the rows behind the last hold the sentinel.  D = 520: lane 0 alone owns a second chunk.  A split row is made of whole [32 hi | 32 lo] blocks: rows
    whose ldo is no multiple of 32 (D + 32 for D = 8, 40, 200, 520, 1000) cannot hold one and must be refused, not written"""
    planes, ldx, extra = planes_of(mode), D + 4, 3
    gam, bet = 1 + 0.1 * rnd(D, seed=1), 0.1 * rnd(D, seed=2)
    gd, bd = cuda(gam), cuda(bet)
    for rows_out_per_b, rows_in_per_b, in_offset, rows in LN_MAPS:
        rowmap = (rows_out_per_b, rows_in_per_b, in_offset)
        in_rows = rows if rows_out_per_b == 0 else rows // rows_out_per_b * rows_in_per_b
        x = rnd(in_rows, ldx, seed=D + rows) * 3 + 1
        xd = cuda(x)
        ref = R.layernorm_rows(x, gam, bet, 1e-6, D, rows, rows_out_per_b=rows_out_per_b, rows_in_per_b=rows_in_per_b, in_offset=in_offset)
        for ldo in (-(-D // 32) * 32, D + 32):
            rc, out, f32 = run_layernorm(d, gu, mode, xd, gd, bd, D, ldx, rows, rowmap, ldo, rows + extra, True)
            if planes == 2 and ldo % 32:
                assert rc != 0 and b"multiple of 32" in d.cwm_last_error(), (D, ldo)
                torch.cuda.synchronize()
                assert (out == gu.NAN_BF16).all() and (f32 == SENT).all(), (D, ldo, "a refused launch wrote")
                continue
            _lib.check(rc, d)
            y = f32.cpu()
            err = (y[:rows].double() - ref).abs().max().item()
            print("LAYERNORM %s D=%d ldo=%d row map %s: max-abs error of the fp32 copy %.3e" % (mode, D, ldo, rowmap, err))
            assert err <= 5e-6, (mode, D, rowmap, ldo, err)
            assert (y[rows:] == SENT).all()
            img = operand_image(y[:rows], rows + extra, ldo, planes, gu)
            assert raw_equal(out, img), (mode, D, rowmap, ldo, (out.cpu() != img).nonzero()[:4].tolist())
            rc, out2, _ = run_layernorm(d, gu, mode, xd, gd, bd, D, ldx, rows, rowmap, ldo, rows + extra, False)
            _lib.check(rc, d)
            assert torch.equal(out2, out), (mode, D, rowmap, ldo, "the operand depends on out_f32")


def test_stand_alone_layernorm_accepts_widths_that_are_no_multiple_of_32(gu):
    """cwm_layernorm stages its (discarded) operand in rows of round_up(D, 32): D = 40 and 200 ran over the end of a [rows][2 D] buffer before"""
    _lib.get_lib()
    for D in (40, 200, 8):
        x = rnd(37, D, seed=D) * 3 + 1
        g_, b_ = 1 + 0.1 * rnd(D, seed=1), 0.1 * rnd(D, seed=2)
        ref = R.layernorm_rows(x, g_, b_, 1e-6, D, 37)
        assert (gu.layernorm(x, g_, b_).double() - ref).abs().max().item() <= 5e-6


# ---- fill_mask_tokens ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Nt,n_vis,D", [(2, 40, 13, 128), (3, 197, 196, 384), (1, 64, 0, 96), (2, 40, 40, 128)])
def test_fill_mask_tokens(d, gu, B, Nt, n_vis, D):
    """x_full[b][n_vis + j] = mask_token + pos[perm[b][n_vis + j]]: one fp32 add, so bit-exact; visible rows untouched; n_vis == Nt writes nothing"""
    g = torch.Generator().manual_seed(Nt)
    tok, pos = rnd(D, seed=1), rnd(Nt + 5, D, seed=2)
    perm = torch.stack([torch.randperm(Nt + 5, generator=g)[:Nt] for _ in range(B)])
    x0 = torch.full((B, Nt, D), SENT)
    want = R.fill_mask_tokens(x0, tok, pos, perm, n_vis)
    xd, td, pd, permd = cuda(x0), cuda(tok), cuda(pos), perm.to(torch.int32).cuda()
    _lib.check(d.cwm_dev_fill_mask_tokens(xd.data_ptr(), td.data_ptr(), pd.data_ptr(), permd.data_ptr(), B, Nt, n_vis, D, gu.stream()), d)
    assert raw_equal(xd, want)
    assert (xd[:, :n_vis] == SENT).all() and (n_vis == Nt or (xd[:, n_vis:] != SENT).all())
