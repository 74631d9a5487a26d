"""Decoder block 0 of the plain predictor takes LN1 and Q / K / V of its mask-token rows from a per-position table (csrc/engine.hip Engine::dec0_table,
option "mask_token_tables") instead of computing them for every sample of every call.  The table is made by the forward's own kernels, whose rows are
independent, so every output must be bit-identical with the option off -- on the tiny model of tests/test_model_gpu.py (32 tokens, one decoder block, which
is therefore also the pruned last block), in both modes, through `predict_video` (tokens and frames) unless the case says otherwise.
Also here: the launch form the table path adds -- the Q/K/V scatter over the first rows_in <= n_tok tokens of every sample -- one launch at a time."""
import contextlib
import ctypes

import pytest
import torch

from counterfactualworldmodels_amd import _lib, config as C, synthetic as S, vmae

pytestmark = pytest.mark.gpu
MODES = ("parity", "fast")
TINY = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
NT = 32
OPT = "mask_token_tables"


def weights(seed):
    return {k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(TINY, seed).items()}


def build(sd, mode, **options):
    m = vmae.PretrainVisionTransformer(TINY, mode=mode)
    m.load_state_dict(sd)
    for k, v in options.items():
        m.set_option(k, v)  # (before the first forward: applied when the handle is created)
    return m.to("cuda:0").eval()


def frames(B, seed):
    return torch.from_numpy(S.synthetic_frames(B, TINY, seed)).cuda()


def masks(B, n_vis, seed):
    """bool [B, NT], True = masked: a different random set of n_vis visible tokens in every row"""
    g = torch.Generator().manual_seed(seed)
    m = torch.ones(B, NT, dtype=torch.bool)
    for b in range(B):
        m[b, torch.randperm(NT, generator=g)[:n_vis]] = False
    assert B == 1 or n_vis in (0, NT) or not all(torch.equal(m[0], m[b]) for b in range(1, B))
    return m.cuda()


def same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def on_off(m, x, mask, **kw):
    """(outputs with the table, outputs without) of one live handle"""
    m.set_option(OPT, 1)
    on = m.predict_video(x, mask, **kw)
    m.set_option(OPT, 0)
    off = m.predict_video(x, mask, **kw)
    m.set_option(OPT, 1)
    return on, off


@pytest.fixture(scope="module")
def parent():
    """mode -> a handle that never had the option on (created with it off): what the library computed before the table existed"""
    sd = weights(3)
    return {mode: build(sd, mode, **{OPT: 0}) for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
def test_table_rows_equal_computed_rows(mode, parent):
    """B = 1, 2, 3 with a different mask per row; exactly one masked token; one visible token -- against the option off on the same handle and against a
    handle created with it off"""
    m = build(weights(3), mode)
    for B, n_vis in [(1, 9), (2, 9), (3, 9), (3, 16), (2, NT - 1), (3, 1)]:
        x, mask = frames(B, 10 + B), masks(B, n_vis, 20 + n_vis)
        on, off = on_off(m, x, mask)
        ref = parent[mode].predict_video(x, mask)
        assert on[0].shape == (B, NT - n_vis, 192) and torch.isfinite(on[0]).all()
        assert same(on, off) and same(on, ref), (mode, B, n_vis, (on[0] - ref[0]).abs().max().item())


@pytest.mark.parametrize("mode", MODES)
def test_nothing_masked_and_ragged_batches_keep_the_computed_path(mode, parent):
    """nothing masked (the decoder returns every token; no table row is used) and a ragged batch (rows with different visible counts): the path of before runs,
    with the option on or off, and the outputs are the parent's"""
    m = build(weights(3), mode)
    x = frames(3, 5).transpose(1, 2).contiguous()  # the model seam takes [B, C, T, H, W]
    none = torch.zeros(3, NT, dtype=torch.bool, device="cuda")
    m.set_option(OPT, 1)
    on = m(x, none)
    m.set_option(OPT, 0)
    off = m(x, none)
    assert on.shape == (3, NT, 192) and torch.equal(on, off) and torch.equal(on, parent[mode](x, none))
    rag = torch.ones(3, NT, dtype=torch.bool)
    for b, n in enumerate((5, 9, 7)):
        rag[b, torch.randperm(NT, generator=torch.Generator().manual_seed(40 + b))[:n]] = False
    rag = rag.cuda()
    m.set_option(OPT, 1)
    on = m(x, rag, ragged=True)
    m.set_option(OPT, 0)
    off = m(x, rag, ragged=True)
    assert torch.equal(on, off) and torch.equal(on, parent[mode](x, rag, ragged=True))
    # ... and the rectangular call after the ragged one is back on the table
    mask = masks(3, 9, 1)
    xv = frames(3, 5)
    on, off = on_off(m, xv, mask)
    assert same(on, off) and same(on, parent[mode].predict_video(xv, mask))


@pytest.mark.parametrize("mode", MODES)
def test_one_lane_and_two_lanes(mode):
    """a batch of 4 as one lane and as two (the table is built before the lanes fork and read by both): on == off at either lane count"""
    m = build(weights(4), mode, min_lane_rows=1)
    x, mask = frames(4, 2), masks(4, 11, 2)
    m.predict_video(x, mask)  # (creates the handle: set_lanes needs one)
    for lanes in (2, 1, 2):
        m.set_lanes(lanes)
        on, off = on_off(m, x, mask)
        assert same(on, off), (mode, lanes)


def test_one_table_per_mode_on_one_handle(parent):
    """parity, then fast, then parity on one handle: each mode reads its own table"""
    m = build(weights(3), "parity")
    x, mask = frames(2, 8), masks(2, 12, 8)
    outs = []
    for mode in ("parity", "fast", "parity", "fast"):
        m.mode = mode
        outs.append(m.predict_video(x, mask))
        assert same(outs[-1], parent[mode].predict_video(x, mask)), mode
    assert same(outs[0], outs[2]) and same(outs[1], outs[3]) and not torch.equal(outs[0][0], outs[1][0])


@pytest.mark.parametrize("mode", MODES)
def test_reloaded_weights_rebuild_the_table(mode):
    """decoder.blocks.0.norm1.weight, then the qkv weight, then mask_token are changed on a live handle whose table exists: each changes the output, to that of a
    fresh model (table off) with those weights"""
    sd = weights(6)
    m = build(sd, mode)
    x, mask = frames(2, 9), masks(2, 10, 9)
    prev = m.predict_video(x, mask)
    g = torch.Generator().manual_seed(1)
    for key in ("decoder.blocks.0.norm1.weight", "decoder.blocks.0.attn.qkv.weight", "mask_token"):
        new = sd[key] + 0.05 * torch.randn(sd[key].shape, generator=g)
        sd = dict(sd, **{key: new})
        with torch.no_grad():
            m.state_dict(keep_vars=True)[key].copy_(new)
        got = m.predict_video(x, mask)
        want = build(sd, mode, **{OPT: 0}).predict_video(x, mask)
        assert same(got, want), (mode, key, (got[0] - want[0]).abs().max().item())
        assert not torch.equal(got[0], prev[0]), (mode, key)
        prev = got


def test_table_rows_on_the_headline_model():
    """ViT-B/8 at batch 2 (1568 tokens, 792 visible; block 0 is not the pruned last block here, and the table's GEMM launch -- 1568 rows -- takes another
    kernel than the forward's): both modes on one handle, the default tile rule and each kernel forced, with and without pruning: on == off"""
    cfg = C.CONFIGS["base_8x8patch_2frames_1tube"]
    m = vmae.PretrainVisionTransformer(cfg, mode="parity")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 1).items()})
    m = m.to("cuda:0").eval()
    x = torch.from_numpy(S.synthetic_frames(2, cfg, 1)).cuda()
    mask = torch.from_numpy(S.synthetic_masks(2, cfg, 8, 1, 1)).cuda()
    for mode in MODES:
        m.mode = mode
        for tile, prune in [(0, 1), (4, 1), (1, 0)]:
            m.set_option("gemm_tile", tile)
            m.set_option("prune_last_block", prune)
            on, off = on_off(m, x, mask)
            assert on[0].shape == (2, 776, 192) and same(on, off), (mode, tile, prune)


# ---- the relaxed Q/K/V launch form, one launch at a time --------------------------------------------------------------------------------------------
F32, QKV = 0, 3
NAN_BF16 = 0x7FC0
DEFAULTS = {"gemm_tile": 0, "gemm_staged": 1, "gemm_direct": 1}


@contextlib.contextmanager
def switches(d, **kw):
    try:
        for k, v in kw.items():
            _lib.check(d.cwm_debug_set(k.encode(), int(v)), d)
        yield
    finally:
        for k in kw:
            d.cwm_debug_set(k.encode(), DEFAULTS[k])


def qkv_launch(d, mode, a, w, bias, B, rows_in, n_tok, H):
    import gpu_utils as gu

    planes = 2 if mode == "parity" else 1
    count, guard = B * H * n_tok * 64, 192
    bufs = [torch.full((planes, count + guard), NAN_BF16, dtype=torch.int16, device="cuda") for _ in range(3)]
    g = _lib.new_dev_conj_args(_lib.CwmDevGemmArgs)
    g.mode, g.epi = _lib.mode_id(mode), QKV
    g.a, g.w, g.bias = a.data_ptr(), w.data_ptr(), bias.data_ptr()
    (g.M, g.K), g.N = a.shape, w.shape[0]
    g.rows_in, g.rows_out, g.map_stride = rows_in, n_tok, n_tok
    g.q_out, g.k_out, g.v_out = (b.data_ptr() for b in bufs)
    g.qk_plane, g.heads, g.head_dim, g.n_tok, g.q_scale = count + guard, H, 64, n_tok, 0.125
    forms = (ctypes.c_int32 * 2)(-1, -1)
    g.plan_forms = forms
    g.stream = gu.stream()
    _lib.check(d.cwm_dev_gemm(ctypes.byref(g)), d)
    return [b[:, :count].view(planes, B, H, n_tok, 64) for b in bufs], [b[:, count:] for b in bufs]


@pytest.mark.parametrize("mode", MODES)
def test_qkv_scatter_over_the_first_rows_of_every_sample(mode):
    """rows_in in {1, 24, 129} tokens of samples of n_tok in {rows_in + 1, 200}, two samples, staged / direct / per-fragment epilogue, the default tile rule and
    the forced 8-phase kernel: rows [0, rows_in) of every (sample, head) equal the full launch's, the rows behind them and the guard keep the sentinel"""
    d = _lib.get_dev_lib()
    B, H, K = 2, 2, 128
    g = torch.Generator().manual_seed(5)
    w, bias = (torch.randn(3 * H * 64, K, generator=g) * K ** -0.5).cuda(), torch.randn(3 * H * 64, generator=g).cuda()
    for rows_in in (1, 24, 129):
        for n_tok in sorted({rows_in + 1, 200}):
            full_a = torch.randn(B, n_tok, K, generator=g).cuda()
            part_a = full_a[:, :rows_in].contiguous()
            full, _ = qkv_launch(d, mode, full_a.view(-1, K), w, bias, B, n_tok, n_tok, H)
            for tile, st, dr in [(0, 1, 0), (0, 1, 1), (0, 0, 0), (4, 1, 1), (4, 1, 0), (1, 1, 1)]:
                with switches(d, gemm_tile=tile, gemm_staged=st, gemm_direct=dr):
                    part, guards = qkv_launch(d, mode, part_a.view(-1, K), w, bias, B, rows_in, n_tok, H)
                for name, p, f, gd in zip("qkv", part, full, guards):
                    assert torch.equal(p[:, :, :, :rows_in], f[:, :, :, :rows_in]), (mode, name, rows_in, n_tok, (tile, st, dr))
                    assert (p[:, :, :, rows_in:] == NAN_BF16).all() and (gd == NAN_BF16).all(), (mode, name, rows_in, n_tok, (tile, st, dr))
    # more rows per sample than the sample has tokens is refused before anything is launched
    with pytest.raises(_lib.CwmHipError):
        qkv_launch(d, mode, torch.randn(2 * 9, K).cuda(), w, bias, 2, 9, 8, H)
