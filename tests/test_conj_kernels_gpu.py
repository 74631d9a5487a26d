"""The attention and padding kernels of the IMU-conditioned (conjoined) predictor one call at a time, through the development library
(include/cwm_hip_dev.h cwm_dev_conj_cross_attention / cwm_dev_conj_small_attention / cwm_dev_conj_pad):

  csrc/conj_attention.hip  cross_attn_mfma_kernel roles A and B, cross_attn_combine_kernel, small_attn_mfma_kernel          ("MFMA" below)
  csrc/conj_kernels.hip    the fp32 VALU forms of the same operations and the padding bookkeeping                          ("VALU" below)

The reference is tests/conj_attention_restatement.py -- float64, computed from the same fp32 inputs (tests/test_conj_kernels_cpu.py ties it to the
oracles) -- never the other kernel form, except in the tests that are by name a comparison of the two forms.  Every output buffer is pre-filled with a
NaN pattern and carries 8 guard rows: every element of the rows the call owns must have been written, the guard rows must still hold the pattern.
B = 2 and 3 heads throughout (different data per batch element and head), both modes.

Bounds (max-abs on O(1) outputs of randn inputs, scale = head_dim^-0.5):
  MFMA forms   3e-4 parity / 3e-2 fast, 5e-4 / 5e-2 for the "late spike" variants: what tests/test_kernels_gpu.py holds the 64-wide flash attention to
               (the same split-bf16 / bf16 products with fp32 accumulation).  Worst measured (MI355X): 5.9e-5 parity (head_dim 192) and 2.2e-2 fast (head_dim 96), spike cases
               4.8e-5 / 2.9e-2, small attention 2.0e-5 / 1.2e-2: no instance needs more, so no bound here comes from an emulation.
  VALU forms   |err| <= rel |ref| + FLOOR with rel = 2^-16 parity / 2^-8 fast, the operand format's own bound (tests/test_gather_kernels_gpu.py); FLOOR
               covers the fp32 softmax and accumulation: the worst |err| - rel |ref| measured over the cases below (MI355X) is 2.513e-6 (parity, the
               context update of the head_dim 192 spike case; 1.126e-6 without the spike cases, 2.58e-7 in the small attention, 4.09e-7 in fast mode),
               120 x below the MFMA parity bound; FLOOR = 4 x 2.513e-6 = 1.005e-5 (the kernels are deterministic: the margin is for other seeds).
  MFMA against VALU   the sum of the two bounds.
  selection cases, determinism, roles, bookkeeping   bitwise.

Which case launches which MFMA instance cross_attn_mfma_kernel<PLANES, NDB, MT, role> (PLANES 2 parity / 1 fast: every case runs both; NDB =
head_dim / 32; MT = 1 for M <= 32, 2 above; both roles per case) -- CROSS_CASES rows by (head_dim, M, N):
  <*, 1, 1>  (32, 1, 33) (32, 5, 1) (32, 5, 31) (32, 5, 32) (32, 25, 512) (32, 32, 63) (32, 31, 65) (32, 25, 1031)      spike (32, 25, 1100)
  <*, 1, 2>  (32, 33, 1) (32, 33, 31) (32, 33, 65) (32, 50, 513) (32, 63, 33) (32, 64, 63) (32, 50, 1100)                spike (32, 50, 1100)   selection (32, 64, 545)
  <*, 3, 1>  (96, 1, 31) (96, 5, 33) (96, 5, 63) (96, 25, 513) (96, 32, 65) (96, 25, 1100)                                spike (96, 25, 1100)
  <*, 3, 2>  (96, 33, 32) (96, 33, 33) (96, 33, 63) (96, 50, 512) (96, 64, 31) (96, 50, 1031) (96, 63, 65)                spike (96, 50, 1031)   selection (96, 50, 33)
  <*, 6, 1>  (192, 1, 65) (192, 5, 31) (192, 5, 65) (192, 25, 512) (192, 32, 33) (192, 25, 1031) (192, 31, 63)            spike (192, 25, 1031)  selection (192, 32, 1031)
  <*, 1, 1> and <*, 3, 1> have their selection case in (32, 25, 97) and (96, 32, 545).
  VALU only (head_dim 192 beyond M = 32): (192, 33, 33) (192, 50, 513) (192, 63, 65), selection (192, 50, 65); M = 64 there is refused (LDS).
N < 512 leaves role-B shares without a chunk (their -1e30 maximum must weigh 0 in the combine), N = 512 gives every share exactly one chunk, 513 gives
share 0 a second chunk of one token, 1031 / 1100 several chunks per share and a ragged tail; below N = 1024 half of role A's 32 shares are idle.
Tried on scratch builds of conj_attention.hip (not part of the tree): without role B's `ragged` mask 66 of the 98 cross cases (float64 + spike +
selection) fail, without role A's `m >= M` mask 66, with two entries of ctx_pos exchanged 84 (every selection case among them).
small_attn_mfma_kernel<PLANES, NT>: NT = 1 for n_tok in {1, 8, 26, 31, 32}, NT = 2 for {33, 51, 64}; selection cases at n_tok 33 and 64 (NT = 2) and 26
(NT = 1)."""
import ctypes
import functools

import pytest
import torch

import conj_attention_restatement as R
from counterfactualworldmodels_amd import _lib
from gpu_utils import NAN_BF16, bits, decode, new_operand
from oracle import conj_oracle as O

pytestmark = pytest.mark.gpu

MODES = {"parity": (_lib.MODE_PARITY, 2), "fast": (_lib.MODE_FAST, 1)}
IMPLS = {"valu": _lib.DEV_CONJ_VALU, "mfma": _lib.DEV_CONJ_MFMA}
B, HEADS, GUARD = 2, 3, 8
MFMA_TOL = {"parity": 3e-4, "fast": 3e-2}
MFMA_SPIKE_TOL = {"parity": 5e-4, "fast": 5e-2}
REL = {"parity": 2.0 ** -16, "fast": 2.0 ** -8}
# worst |err| - rel |ref| of the VALU forms over every float64 comparison of this module (cross, spike and small cases; MI355X), and the floor: 4 x
VALU_EXCESS_MEASURED = 2.513e-6
FLOOR = 4 * VALU_EXCESS_MEASURED
assert 10 * VALU_EXCESS_MEASURED <= MFMA_TOL["parity"]  # (else the "exact fp32" forms would not be what conj_kernels.hip says they are)

CROSS_CASES = [  # (head_dim, M, N)
    (32, 1, 33), (32, 5, 1), (32, 5, 31), (32, 5, 32), (32, 25, 512), (32, 32, 63), (32, 31, 65), (32, 25, 1031),
    (32, 33, 1), (32, 33, 31), (32, 33, 65), (32, 50, 513), (32, 63, 33), (32, 64, 63), (32, 50, 1100),
    (96, 1, 31), (96, 5, 33), (96, 5, 63), (96, 25, 513), (96, 32, 65), (96, 25, 1100),
    (96, 33, 32), (96, 33, 33), (96, 33, 63), (96, 50, 512), (96, 64, 31), (96, 50, 1031), (96, 63, 65),
    (192, 1, 65), (192, 5, 31), (192, 5, 65), (192, 25, 512), (192, 32, 33), (192, 25, 1031), (192, 31, 63),
    (192, 33, 33), (192, 50, 513), (192, 63, 65),
]
SPIKE_CASES = [(32, 25, 1100), (32, 50, 1100), (96, 25, 1100), (96, 50, 1031), (192, 25, 1031)]  # one per MFMA instance
BOTH_FORMS_CASES = [(32, 25, 1031), (32, 50, 1100), (96, 25, 1100), (96, 50, 1031), (192, 25, 1031)]
SELECTION = R.SELECTION_SHAPES


def mfma_ok(hd, M):
    return hd in (32, 96, 192) and 1 <= M <= (32 if hd == 192 else 64)


def valu_ok(hd, M):
    """the corrected precondition of launch_cross_attention: the LDS request (3 M hd + 64 (M + 1)) * 4 within 160 KiB"""
    return 1 <= M <= 64 and hd % 32 == 0 and 0 < hd <= 256 and (3 * M * hd + 64 * (M + 1)) * 4 <= 160 * 1024


def impls_of(hd, M):
    return [i for i, ok in (("valu", valu_ok(hd, M)), ("mfma", mfma_ok(hd, M))) if ok]


MFMA_CASES = [c for c in CROSS_CASES if mfma_ok(c[0], c[1])]
assert all(valu_ok(hd, M) for hd, M, _ in CROSS_CASES) and len(MFMA_CASES) == len(CROSS_CASES) - 3
for _ndb, _mt in [(1, 1), (1, 2), (3, 1), (3, 2), (6, 1)]:  # every MFMA instance: M at both ends of its range, an N < 32, a ragged N, an N > 512
    _c = [(M, N) for hd, M, N in MFMA_CASES if hd == 32 * _ndb and (M > 32) == (_mt == 2)]
    assert {M for M, _ in _c} >= ({1, 32} if _mt == 1 else {33, 64}) and any(N < 32 for _, N in _c) and any(N % 32 for _, N in _c) and any(N > 512 for _, N in _c)
    assert any(hd == 32 * _ndb and (M > 32) == (_mt == 2) and mfma_ok(hd, M) for hd, M, _ in SELECTION)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.get_dev_lib()


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- inputs and float64 references, computed once per case and left unchanged ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cross_case(hd, M, N, spike=False):
    D, g = HEADS * hd, gen(1000 * hd + 17 * M + N)
    qk, v = torch.randn(B, N, 2 * D, generator=g), torch.randn(B, N, D, generator=g)
    qk_src, v_src = torch.randn(B, M, 2 * D, generator=g), torch.randn(B, M, D, generator=g)
    if spike:
        # role B (softmax over the tokens): the key of a token in the SECOND chunk of its share (token >= 512) far above the rest for context row m1,
        # a key in chunk 0 for row m2 -- the running maximum jumps late / stays; role A (softmax over the context): the key of row m3 for a few tokens
        assert N > 600 and M >= 8
        q4, s4 = qk.view(B, N, HEADS, 2, hd), qk_src.view(B, M, HEADS, 2, hd)
        m1, m2, m3 = 3, M - 1, 5
        q4[:, 530 + 32 * (hd // 32), :, 1] = 6.0 * s4[:, m1, :, 1]
        q4[:, 7, :, 1] = 6.0 * s4[:, m2, :, 1]
        for n in (2, 601, N - 1):
            q4[:, n, :, 0] = 6.0 * s4[:, m3, :, 0]
    ref = R.cross(qk, v, qk_src, v_src, HEADS, hd ** -0.5)
    return tuple(t.cuda() for t in (qk, v, qk_src, v_src)), ref


def cross_outputs(mode, N, M, D):
    planes = MODES[mode][1]
    return new_operand(B * N + GUARD, D, planes), new_operand(B * M + GUARD, D, planes)


def cross_call(dev, impl, mode, inputs, hd, M, N, y, y_src, roles=3, heads=HEADS, batch=B, scale=None, expect_error=False):
    a = _lib.new_dev_conj_args(_lib.CwmDevConjCrossAttentionArgs)
    a.mode, a.impl, a.roles = MODES[mode][0], IMPLS[impl], roles
    a.qk, a.v, a.qk_src, a.v_src = (_lib.ptr(t) for t in inputs)
    a.B, a.N, a.M, a.heads, a.head_dim = batch, N, M, heads, hd
    a.scale = hd ** -0.5 if scale is None else scale
    a.y, a.y_src, a.stream = _lib.ptr(y), _lib.ptr(y_src), None
    rc = dev.cwm_dev_conj_cross_attention(ctypes.byref(a))
    if expect_error:
        return rc
    _lib.check(rc, dev)


def untouched(A):
    return bool((A == NAN_BF16).all().item())


def read_operand(name, A, rows, mode, cols=None):
    """-> (hi, lo) of rows [0, rows): every element written (no NaN left), the guard rows behind them still the pattern; cols: only these columns of the
    row are the call's (the others must hold the pattern)"""
    planes = MODES[mode][1]
    width = A.shape[1] // planes
    assert A.shape[0] == rows + GUARD
    assert untouched(A[rows:]), (name, mode, "guard rows overwritten")
    hi, lo = decode(A[:rows], planes, width)
    for p in (hi, lo):
        if p is not None:
            if cols is not None:
                assert (bits(p[:, cols:]) == NAN_BF16).all(), (name, mode, "columns beyond the output written")
            assert not torch.isnan(p[:, :cols].float()).any(), (name, mode, "elements left unwritten")
    return hi[:, :cols], (lo[:, :cols] if lo is not None else None)


def value(hi, lo):
    return hi.double() + (lo.double() if lo is not None else 0.0)


def check_float64(name, impl, mode, got, ref, tol=None):
    """MFMA: max-abs <= tol; VALU: |err| <= rel |ref| + FLOOR elementwise.  Prints the worst figure before asserting."""
    ref = ref.reshape(got.shape)
    err = (got - ref).abs()
    if impl == "mfma":
        tol = (tol or MFMA_TOL)[mode]
        print(f"[conj {name} mfma {mode}] max-abs {err.max().item():.3e} (bound {tol:.0e})")
        assert err.max().item() <= tol, (name, mode, err.max().item())
    else:
        excess = (err - REL[mode] * ref.abs()).max().item()
        print(f"[conj {name} valu {mode}] max-abs {err.max().item():.3e}, worst |err| - rel |ref| {excess:.3e} (floor {FLOOR:.1e})")
        assert excess <= FLOOR, (name, mode, excess)


def run_cross(dev, impl, mode, hd, M, N, spike=False, roles=3):
    inputs, _ = cross_case(hd, M, N, spike)
    y, y_src = cross_outputs(mode, N, M, HEADS * hd)
    cross_call(dev, impl, mode, inputs, hd, M, N, y, y_src, roles)
    return y, y_src


def case_id(c):
    return "hd%d-M%d-N%d" % c


# ---- a. cross attention against float64, both forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CROSS_CASES, ids=case_id)
@pytest.mark.parametrize("mode", list(MODES))
def test_cross_attention_matches_float64(dev, mode, case):
    hd, M, N = case
    _, (ref_y, ref_ys) = cross_case(hd, M, N)
    for impl in impls_of(hd, M):
        y, y_src = run_cross(dev, impl, mode, hd, M, N)
        check_float64(f"{case_id(case)} y", impl, mode, value(*read_operand("y", y, B * N, mode)), ref_y)
        check_float64(f"{case_id(case)} y_src", impl, mode, value(*read_operand("y_src", y_src, B * M, mode)), ref_ys)


@pytest.mark.parametrize("case", SPIKE_CASES, ids=case_id)
@pytest.mark.parametrize("mode", list(MODES))
def test_cross_attention_late_spike(dev, mode, case):
    """the online-softmax rescale of role B across a share's chunks with the maximum arriving in the second chunk (and in chunk 0), and a dominant context
    key in role A: tests/test_kernels_gpu.py test_attention_online_softmax_rescale_branch for these kernels"""
    hd, M, N = case
    _, (ref_y, ref_ys) = cross_case(hd, M, N, True)
    for impl in impls_of(hd, M):
        y, y_src = run_cross(dev, impl, mode, hd, M, N, spike=True)
        check_float64(f"spike {case_id(case)} y", impl, mode, value(*read_operand("y", y, B * N, mode)), ref_y, MFMA_SPIKE_TOL)
        check_float64(f"spike {case_id(case)} y_src", impl, mode, value(*read_operand("y_src", y_src, B * M, mode)), ref_ys, MFMA_SPIKE_TOL)


@pytest.mark.parametrize("case", BOTH_FORMS_CASES, ids=case_id)
@pytest.mark.parametrize("mode", list(MODES))
def test_cross_attention_mfma_against_valu(dev, mode, case):
    hd, M, N = case
    _, refs = cross_case(hd, M, N)
    outs = {impl: run_cross(dev, impl, mode, hd, M, N) for impl in ("valu", "mfma")}
    for i, (name, rows) in enumerate((("y", B * N), ("y_src", B * M))):
        a, b = (value(*read_operand(name, outs[impl][i], rows, mode)) for impl in ("valu", "mfma"))
        bound = MFMA_TOL[mode] + REL[mode] * refs[i].reshape(a.shape).abs() + FLOOR
        print(f"[conj {case_id(case)} {name} mfma - valu {mode}] max-abs {(a - b).abs().max().item():.3e}")
        assert ((a - b).abs() <= bound).all(), (name, mode, (a - b).abs().max().item())


# ---- b. selection cases: bitwise ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def selection_case(hd, M, N):
    qk, v, qk_src, v_src, sel_a, sel_b = R.selection_cross(B, N, M, HEADS, hd)
    return tuple(t.cuda() for t in (qk, v, qk_src, v_src)), v_src[:, sel_a].reshape(B * N, -1), v[:, sel_b].reshape(B * M, -1)


def assert_selected(name, A, rows, mode, want, cols=None):
    hi, lo = read_operand(name, A, rows, mode, cols)
    assert torch.equal(bits(hi), bits(want.to(torch.bfloat16))), (name, mode, "hi != bf16(selected V row)")
    if lo is not None:
        assert (bits(lo) == 0).all(), (name, mode, "lo != 0")


@pytest.mark.parametrize("case", SELECTION, ids=case_id)
@pytest.mark.parametrize("mode", list(MODES))
def test_cross_attention_selection_is_bitwise(dev, mode, case):
    """one-hot softmaxes (tests/conj_attention_restatement.py selection_cross, checked on the CPU in test_conj_kernels_cpu.py): main token n must return
    V_src row (7 n + 3) % M, context row m the V row of token t(m) -- token 0, the last token of the ragged chunk, tokens of a share's second chunk --
    bit for bit.  Catches a wrong ctx_pos, transposed V read, share merge or (batch, head) index exactly.  It cannot see a dropped mask: a padded context
    row scores 0 and a clamped token repeats a row that is selected or scores 0, either way with weight exactly 0 or cancelling in O / l -- the float64
    cases above are what fails then (module docstring)."""
    hd, M, N = case
    inputs, want_y, want_ys = selection_case(hd, M, N)
    for impl in impls_of(hd, M):
        y, y_src = cross_outputs(mode, N, M, HEADS * hd)
        cross_call(dev, impl, mode, inputs, hd, M, N, y, y_src)
        assert_selected(f"{impl} y", y, B * N, mode, want_y)
        assert_selected(f"{impl} y_src", y_src, B * M, mode, want_ys)


# ---- c. determinism and roles ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MFMA_CASES, ids=case_id)
@pytest.mark.parametrize("mode", list(MODES))
def test_cross_attention_mfma_is_deterministic_and_roles_compose(dev, mode, case):
    hd, M, N = case
    y, y_src = run_cross(dev, "mfma", mode, hd, M, N)
    y2, y_src2 = run_cross(dev, "mfma", mode, hd, M, N)
    assert torch.equal(y, y2) and torch.equal(y_src, y_src2), "two launches differ"  # (the combine merges the shares in a fixed order)
    ya, ysa = run_cross(dev, "mfma", mode, hd, M, N, roles=1)
    assert untouched(ysa), "roles = 1 wrote y_src"
    assert torch.equal(ya, y)
    inputs, _ = cross_case(hd, M, N)
    cross_call(dev, "mfma", mode, inputs, hd, M, N, ya, ysa, roles=2)  # ... then role B into the same buffers
    assert torch.equal(ya, y) and torch.equal(ysa, y_src), "roles 1 then 2 != roles 3"
    yb, ysb = run_cross(dev, "mfma", mode, hd, M, N, roles=2)
    assert untouched(yb), "roles = 2 wrote y"
    assert torch.equal(ysb, y_src)


# ---- d. small self-attention -------------------------------------------------------------------------------------------------------------------------------
N_TOK = [1, 8, 26, 31, 32, 33, 51, 64]


@functools.lru_cache(maxsize=None)
def small_case(hd, heads, n):
    qkv = torch.randn(B, n, 3 * heads * hd, generator=gen(100 * hd + 7 * heads + n))
    return qkv.cuda(), R.small(qkv, heads).reshape(B * n, heads * hd)


def round_up32(x):
    return (x + 31) // 32 * 32


def small_call(dev, impl, mode, qkv, heads, hd, n, o, ldo, expect_error=False):
    a = _lib.new_dev_conj_args(_lib.CwmDevConjSmallAttentionArgs)
    a.mode, a.impl, a.qkv = MODES[mode][0], IMPLS[impl], _lib.ptr(qkv)
    a.B, a.n_tok, a.heads, a.head_dim = B, n, heads, hd
    a.o, a.ldo, a.stream = _lib.ptr(o), ldo, None
    rc = dev.cwm_dev_conj_small_attention(ctypes.byref(a))
    if expect_error:
        return rc
    _lib.check(rc, dev)


@pytest.mark.parametrize("n", N_TOK)
@pytest.mark.parametrize("hd,heads", [(32, 3), (32, 12), (16, 3), (48, 3), (64, 3)])
@pytest.mark.parametrize("mode", list(MODES))
def test_small_attention_matches_float64(dev, mode, hd, heads, n):
    """both forms where both apply (head_dim 32), ldo = D (rounded up to the operand's 32-column blocks) and 32 more (the extra columns stay untouched),
    and the two forms against each other"""
    qkv, ref = small_case(hd, heads, n)
    D = heads * hd
    got = {}
    for impl in ["valu"] + (["mfma"] if hd == 32 else []):
        for ldo in (round_up32(D), round_up32(D) + 32):
            o = new_operand(B * n + GUARD, ldo, MODES[mode][1])
            small_call(dev, impl, mode, qkv, heads, hd, n, o, ldo)
            got[impl] = value(*read_operand(f"{impl} ldo {ldo}", o, B * n, mode, cols=D))
            check_float64(f"small hd{hd} heads{heads} n{n} ldo{ldo}", impl, mode, got[impl], ref)
    if len(got) == 2:
        d = (got["mfma"] - got["valu"]).abs()
        assert (d <= MFMA_TOL[mode] + REL[mode] * ref.abs() + FLOOR).all(), ("mfma - valu", mode, d.max().item())


@pytest.mark.parametrize("n", [26, 33, 64])
@pytest.mark.parametrize("hd", [32, 48, 64])
@pytest.mark.parametrize("mode", list(MODES))
def test_small_attention_selection_is_bitwise(dev, mode, hd, n):
    qkv, sel = R.selection_small(B, n, HEADS, hd)
    D = HEADS * hd
    want = qkv[:, :, 2 * D:][:, sel].reshape(B * n, D)
    for impl in ["valu"] + (["mfma"] if hd == 32 else []):
        ldo = round_up32(D) + 32
        o = new_operand(B * n + GUARD, ldo, MODES[mode][1])
        small_call(dev, impl, mode, qkv.cuda(), HEADS, hd, n, o, ldo)
        assert_selected(f"small {impl} hd{hd} n{n}", o, B * n, mode, want, cols=D)


# ---- e. refusals: an error from the entry's / the launcher's precondition, before any launch ------------------------------------------------------
def test_valu_cross_precondition_counts_the_lds():
    """the shapes whose LDS request overflowed the 160 KiB the launcher sets itself: head_dim 192 at M = 64 (164,096 B), 256 from M = 50, 224 from M = 56"""
    assert not valu_ok(192, 64) and valu_ok(192, 63) and not valu_ok(256, 50) and valu_ok(256, 49) and not valu_ok(224, 56) and valu_ok(224, 55)
    assert (3 * 64 * 192 + 64 * 65) * 4 == 164096


@pytest.mark.parametrize("impl,hd,M,roles,null", [("mfma", 64, 8, 3, None), ("mfma", 32, 65, 3, None), ("mfma", 192, 33, 3, None), ("valu", 192, 64, 3, None),
                                                   ("valu", 256, 50, 3, None), ("mfma", 32, 8, 0, None), ("valu", 32, 8, 0, None), ("valu", 32, 8, 1, None),
                                                   ("mfma", 32, 8, 3, "y_src"), ("valu", 32, 8, 3, "qk"), ("mfma", 32, 8, 3, "v_src")])
@pytest.mark.parametrize("mode", list(MODES))
def test_cross_attention_refusals_write_nothing(dev, mode, impl, hd, M, roles, null):
    N, heads, batch = 40, 1, 1
    D = heads * hd
    inputs = [torch.zeros(batch * N, 2 * D), torch.zeros(batch * N, D), torch.zeros(batch * M, 2 * D), torch.zeros(batch * M, D)]
    inputs = [t.cuda() for t in inputs]
    planes = MODES[mode][1]
    y, y_src = new_operand(batch * N + GUARD, D, planes), new_operand(batch * M + GUARD, D, planes)
    names = ("qk", "v", "qk_src", "v_src")
    if null in names:
        inputs[names.index(null)] = None
    rc = cross_call(dev, impl, mode, inputs, hd, M, N, y, None if null == "y_src" else y_src, roles=roles, heads=heads, batch=batch, expect_error=True)
    assert rc != 0 and dev.cwm_last_error(), (impl, hd, M, roles, null)
    torch.cuda.synchronize()
    assert untouched(y) and untouched(y_src)
    if (impl, hd, M) == ("valu", 192, 64):
        assert b"164096" in dev.cwm_last_error()  # (the message states the bytes)


@pytest.mark.parametrize("impl,hd,n,ldo_extra", [("mfma", 64, 8, 0), ("mfma", 32, 65, 0), ("valu", 32, 65, 0), ("mfma", 32, 8, 16), ("valu", 32, 8, 16), ("valu", 96, 8, 0)])
@pytest.mark.parametrize("mode", list(MODES))
def test_small_attention_refusals_write_nothing(dev, mode, impl, hd, n, ldo_extra):
    D = HEADS * hd
    ldo = D + ldo_extra
    qkv = torch.zeros(B * n, 3 * D).cuda()
    o = torch.full((B * n + GUARD, MODES[mode][1] * (ldo + 32)), NAN_BF16, dtype=torch.int16, device="cuda")
    rc = small_call(dev, impl, mode, qkv, HEADS, hd, n, o, ldo, expect_error=True)
    assert rc != 0 and dev.cwm_last_error()
    torch.cuda.synchronize()
    assert untouched(o)


# ---- f. padding bookkeeping: exact ---------------------------------------------------------------------------------------------------------------------------
def pad_args(kind, batch):
    a = _lib.new_dev_conj_args(_lib.CwmDevConjPadArgs)
    a.kind, a.B, a.stream = kind, batch, None
    return a


def pad_mask_call(dev, mask_u8, P, vmax):
    batch, N = mask_u8.shape
    ext = torch.full((batch * (N + P) + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    a = pad_args(_lib.DEV_CONJ_PAD_MASK, batch)
    mask_d = mask_u8.cuda()
    a.mask, a.N, a.P, a.vmax, a.ext_mask = mask_d.data_ptr(), N, P, vmax, ext.data_ptr()
    _lib.check(dev.cwm_dev_conj_pad(ctypes.byref(a)), dev)
    ext = ext.cpu()
    assert (ext[batch * (N + P):] == 0xAA).all(), "written past ext_mask"
    return ext[:batch * (N + P)].reshape(batch, N + P)


@pytest.mark.parametrize("N", [25, 256, 257, 784, 3136])
@pytest.mark.parametrize("P", [0, 25, 64])
def test_pad_mask_matches_the_oracle(dev, N, P):
    """rows with vmax - visible = 0 (the fully visible row), in the middle, = P, >= P and the fully masked row, against oracle.conj_oracle.padding_masks;
    then with a vmax BELOW a row's count (vmax - visible < 0: no pad slot visible), against the kernel's own statement j < vmax - visible"""
    g = gen(N + P)
    counts = [N, max(N - P // 2, 0), max(N - P, 0), max(N - P - 3, 0), 0, N // 3]
    mask = torch.ones(len(counts), N, dtype=torch.bool)
    for b, c in enumerate(counts):
        mask[b, torch.randperm(N, generator=g)[:c]] = False
    full, _ = O.padding_masks(mask, P)
    mask_u8 = mask.to(torch.uint8) * torch.randint(1, 256, mask.shape, generator=g).to(torch.uint8)  # any non-zero byte is "masked"
    assert torch.equal(mask_u8 != 0, mask)
    ext = pad_mask_call(dev, mask_u8, P, N)
    assert torch.equal(ext, full.to(torch.uint8))
    vmax = N // 2
    want = torch.cat([mask, ~(torch.arange(P)[None] < (vmax - (~mask).sum(-1, keepdim=True)))], -1).to(torch.uint8)
    assert (vmax - torch.tensor(counts) < 0).any()
    assert torch.equal(pad_mask_call(dev, mask_u8, P, vmax), want)


def mixed_perm(batch, stride, n_real, seed):
    """[batch][stride] slots drawn from [0, n_real + 9): real tokens and pad slots mixed"""
    return torch.randint(0, n_real + 9, (batch, stride), generator=gen(seed)).to(torch.int32)


@pytest.mark.parametrize("D", [64, 192])
def test_fix_pad_rows_and_zero_pad_out_rows(dev, D):
    batch, n_rows, stride, n_real, n_vis = 3, 11, 29, 20, 13
    perm = mixed_perm(batch, stride, n_real, D)
    x = torch.randn(batch * n_rows + GUARD, D, generator=gen(D + 1))
    token = torch.randn(D, generator=gen(D + 2))
    pad = perm[:, :n_rows].reshape(-1) >= n_real
    assert pad.any() and not pad.all() and not torch.equal(perm[0, :n_rows], perm[1, :n_rows])
    x_d, t_d, p_d = x.cuda(), token.cuda(), perm.cuda()
    a = pad_args(_lib.DEV_CONJ_FIX_PAD_ROWS, batch)
    a.x, a.perm, a.perm_stride, a.n_rows, a.n_real, a.D, a.token = x_d.data_ptr(), p_d.data_ptr(), stride, n_rows, n_real, D, t_d.data_ptr()
    _lib.check(dev.cwm_dev_conj_pad(ctypes.byref(a)), dev)
    want = x.clone()
    want[:batch * n_rows][pad] = token
    assert torch.equal(x_d.cpu().view(torch.int32), want.view(torch.int32))  # (the other rows and the guard rows: bitwise unchanged)
    # zero_pad_out_rows: row j of the sample's n_out output rows is slot perm[b][n_vis + j]
    n_out = stride - n_vis - 2
    pad_o = perm[:, n_vis:n_vis + n_out].reshape(-1) >= n_real
    assert pad_o.any() and not pad_o.all()
    y = torch.randn(batch * n_out + GUARD, D, generator=gen(D + 3))
    y_d = y.cuda()
    a = pad_args(_lib.DEV_CONJ_ZERO_PAD_OUT_ROWS, batch)
    a.x, a.perm, a.perm_stride, a.n_rows, a.n_vis, a.n_real, a.D = y_d.data_ptr(), p_d.data_ptr(), stride, n_out, n_vis, n_real, D
    _lib.check(dev.cwm_dev_conj_pad(ctypes.byref(a)), dev)
    want = y.clone()
    want[:batch * n_out][pad_o] = 0.0
    assert torch.equal(y_d.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("batch,C,L,T,n", [(2, 6, 400, 16, 25), (3, 5, 37, 3, 7)])
def test_imu_append_dummy_is_bitwise(dev, batch, C, L, T, n):
    g = gen(L)
    imu, dummy = torch.randn(batch, C, L, generator=g), torch.randn(C, T, generator=g)
    mask = torch.randint(0, 2, (batch, n), generator=g).to(torch.uint8)
    out = torch.full((batch * C * (L + T) + 64,), float("nan"), device="cuda")
    ext = torch.full((batch * (n + 1) + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    a = pad_args(_lib.DEV_CONJ_IMU_APPEND_DUMMY, batch)
    imu_d, dummy_d, mask_d = imu.cuda(), dummy.cuda(), mask.cuda()
    a.imu, a.dummy, a.mask = imu_d.data_ptr(), dummy_d.data_ptr(), mask_d.data_ptr()
    a.C, a.L, a.T, a.N, a.out, a.ext_mask = C, L, T, n, out.data_ptr(), ext.data_ptr()
    _lib.check(dev.cwm_dev_conj_pad(ctypes.byref(a)), dev)
    out, ext = out.cpu(), ext.cpu()
    want = torch.cat([imu, dummy[None].expand(batch, -1, -1)], -1)
    assert torch.equal(out[:want.numel()].view(torch.int32), want.reshape(-1).view(torch.int32)) and torch.isnan(out[want.numel():]).all()
    want_m = torch.cat([mask, torch.zeros(batch, 1, dtype=torch.uint8)], -1)
    assert torch.equal(ext[:want_m.numel()], want_m.reshape(-1)) and (ext[want_m.numel():] == 0xAA).all()
