"""The ledger of the kernel timers (tests/timer_ledger.py) against itself: the CPU oracle's FLOP count plus the named terms must equal the closed form of the
schedule, for every option and every kind of call, before tests/test_timer_ledger_gpu.py holds the library's books against it.  No GPU."""
import itertools
import os

import numpy as np
import pytest
import torch

import timer_ledger as L
from counterfactualworldmodels_amd import config as C, synthetic as S
from test_conj_oracle import TINY_CONJ, TINY_MAIN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)  # tests/test_model_gpu.py
TINY16 = C.VmaeConfig(name="tiny_16x16", img_size=(64, 64), patch=16, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
CASES = {"tiny8": (TINY, 3, 4), "tiny4": (TINY_MAIN, 2, 5), "tiny16": (TINY16, 2, 3)}  # configuration, batch, visible frame-1 patches (synthetic_masks)


def rect_mask(cfg, B, n_vis):
    """a rectangular mask with n_vis visible tokens per row (the count depends on nothing else)"""
    mask = torch.ones(B, cfg.num_tokens, dtype=torch.bool)
    mask[:, :n_vis] = False
    return mask


@pytest.fixture(scope="module")
def oracle_counts():
    """one oracle run per (case, visible count), shared by the tests below"""
    cache = {}

    def get(name, n_vis):
        if (name, n_vis) not in cache:
            cfg, B, _ = CASES[name]
            cache[(name, n_vis)] = L.vmae_oracle_flops(cfg, rect_mask(cfg, B, n_vis))
        return cache[(name, n_vis)]

    return get


def true_k_flops(gemms):
    return sum(2 * g.M * g.N * g.K for g in gemms)


def test_anchor_tiny8(oracle_counts):
    """TINY, B = 3, synthetic_masks(3, TINY, 4, 0, 1): Nt = 32, Nv = 20, Nm = 12.  The oracle's per-op counts, the closed form of the forward with the patch
    embed over the visible rows only, and their difference -- the reference embeds all Nt patches and then gathers."""
    mask = torch.from_numpy(S.synthetic_masks(3, TINY, 4, 0, 1))
    n_vis = int((~mask[0]).sum())
    assert mask.shape == (3, 32) and ((~mask).sum(1) == 20).all() and n_vis == 20
    o = L.vmae_oracle_flops(TINY, mask)
    assert o == oracle_counts("tiny8", 20)  # the count depends on the shapes only
    assert o["by_op"] == {"addmm": 91_422_720, "mm": 1_966_080, "bmm": 2_801_664}
    B, Nt, Nv, Nm, H = 3, 32, 20, 12, 2
    plain = L.VmaeCall(TINY, B, Nv, prune_last_block=0, mask_token_tables=0)
    closed = true_k_flops(L.vmae_gemms(plain))
    assert closed == 91_619_328
    assert o["matmul"] - closed == 1_769_472 == 2 * B * Nm * 192 * 128 == -L.term_embed_visible_rows(plain)
    assert o["bmm"] == 2 * 4 * B * H * Nv * Nv * 64 + 4 * B * H * Nt * Nt * 64


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_plus_terms_is_the_schedule(name, oracle_counts):
    """For every setting of the two options that change the rows computed, with masked tokens and without, rectangular and ragged: oracle + named terms ==
    the sum over the schedule's launches, GEMM and attention, and the launch counts are those of the schedule (one launch per GEMM on 128x128 tiles)."""
    cfg, B, k_vis = CASES[name]
    Nt = cfg.num_tokens
    n_vis = cfg.tokens_per_frame + k_vis
    assert (~torch.from_numpy(S.synthetic_masks(B, cfg, k_vis, 0, 1))).sum(1).tolist() == [n_vis] * B
    calls = [(n_vis, 0), (Nt, 0), (n_vis, n_vis - 3), (Nt, Nt - 2)]  # (cap, ragged minimum)
    for (cap, n_min), prune, tables in itertools.product(calls, (1, 0), (1, 0)):
        c = L.VmaeCall(cfg, B, cap, n_vis_min=n_min, prune_last_block=prune, mask_token_tables=tables)
        rows = L.vmae_flop_ledger(c, oracle_counts(name, cap))
        books = L.vmae_books(c)
        print(L.format_ledger("%s B=%d n_vis=%d ragged_min=%d prune=%d tables=%d" % (name, B, cap, n_min, prune, tables), rows,
                              (books["GEMM"][1], books["ATTENTION"][1])))
        assert rows[-1][1] == books["GEMM"][1] and rows[-1][2] == books["ATTENTION"][1]
        assert books["GEMM"][0] == 4 * (cfg.enc_depth + cfg.dec_depth) + 3 and books["ATTENTION"][0] == cfg.enc_depth + cfg.dec_depth
        assert books["GEMM_WIDE"] == (0, 0) and books["GEMM_NARROW"] == books["GEMM"]
        assert books["LAYERNORM"][0] == 2 * (cfg.enc_depth + cfg.dec_depth) + 2
        assert books["FILL_MASK"][0] == (1 if c.Nm > 0 else 0) + (1 if c.tables else 0)


def test_padded_k_term():
    """K = 192 (patch 8) and 768 (patch 16) are whole tiles; the patch-4 embed's K = 48 is booked as 64"""
    for name, extra_k in (("tiny8", 0), ("tiny16", 0), ("tiny4", 16)):
        cfg, B, k_vis = CASES[name]
        c = L.VmaeCall(cfg, B, cfg.tokens_per_frame + k_vis)
        assert L.term_padded_k(L.vmae_gemms(c)) == 2 * B * c.n_vis * cfg.enc_dim * extra_k


def test_terms_are_zero_when_their_skip_is_off():
    for cfg, B, _ in CASES.values():
        Nt = cfg.num_tokens
        full = L.VmaeCall(cfg, B, Nt)  # nothing masked: Nm = 0
        assert full.Nm == 0 and full.n_ret == Nt and not full.pruned and not full.tables
        for term in (L.term_embed_visible_rows, L.term_mask_token_tables, L.term_pruned_block_gemms, L.term_pruned_block_attention, L.term_ragged_head_rows):
            assert term(full) == 0, term.__name__
        off = L.VmaeCall(cfg, B, Nt // 2 + 1, prune_last_block=0, mask_token_tables=0)
        for term in (L.term_mask_token_tables, L.term_pruned_block_gemms, L.term_pruned_block_attention, L.term_ragged_head_rows):
            assert term(off) == 0, term.__name__
        assert L.term_embed_visible_rows(off) < 0
        on = L.VmaeCall(cfg, B, Nt // 2 + 1)
        assert L.term_mask_token_tables(on) < 0 and L.term_pruned_block_gemms(on) < 0 and L.term_pruned_block_attention(on) < 0
        ragged = L.VmaeCall(cfg, B, Nt // 2 + 1, n_vis_min=Nt // 2)
        assert L.term_mask_token_tables(ragged) == 0 and L.term_ragged_head_rows(ragged) == 2 * B * cfg.dec_dim * cfg.out_dim  # no tables; one more row


def test_bytes_and_lanes_of_the_schedule():
    """the byte classes restate the header: spot values for TINY (B = 3, Nv = 20, parity and fast), and two lanes book the FLOPs and bytes of one"""
    for planes in (2, 1):
        c = L.VmaeCall(TINY, 3, 20, planes=planes, video=True)
        b = L.vmae_books(c)
        w = 4 + 2 * planes
        ln_rows = 5 * 3 * 20 + 3 * 20 + 3 * 12 + 3 * 12  # LN1/LN2 of two encoder blocks + encoder.norm; decoder block 0: LN1 on B*Nv (table), LN2 on B*Nm (pruned); norm
        assert b["LAYERNORM"] == (8, ln_rows * 128 * w)
        assert b["PATCH_GATHER"] == (1, 3 * 20 * 192 * w + 3 * 32 * (1 + 4 + 4))
        assert b["FILL_MASK"] == (2, 3 * 12 * 128 * 4 + 3 * 12 * 3 * 128 * 2 * planes)
        assert b["UNEMBED"] == (1, 3 * 2 * 3 * 32 * 32 * 8)
        unfused = L.vmae_books(L.VmaeCall(TINY, 3, 20, planes=planes, index_fused=0))
        assert unfused["PATCH_GATHER"] == (1, 3 * 20 * 192 * w) and unfused["UNEMBED"] == (0, 0)
        assert L.vmae_books(L.VmaeCall(TINY, 3, 20, planes=planes))["PATCH_GATHER"] == (1, 3 * 20 * 192 * w + 3 * 32 * 5)
        two = L.vmae_books(c, lanes=2)
        assert L.lane_batches(3, 2) == [2, 1]
        for k in b:
            assert two[k] == (2 * b[k][0], b[k][1]), k


def test_tiny_conjoined_ledger():
    """the tiny padded IMU-conditioned model on the inputs of tests/golden/conj_tiny.npz: oracle + terms == the schedule, for the matrix products and for the
    three attention classes together; the cross attention needs no term (the reference computes two similarity matrices, transformer.py:357-365)"""
    g = np.load(os.path.join(GOLDEN, "conj_tiny.npz"))
    mask, mc = torch.from_numpy(g["mask"]), torch.from_numpy(g["mask_context"])
    B = mask.shape[0]
    vm, vc = int((~mask).sum(1).max()), int((~mc).sum(1).max())
    for ctx_out in (False, True):
        o = L.conj_oracle_flops(TINY_CONJ, tuple(g["x"].shape[:1]) + (3, 2, 32, 32), mask, tuple(g["imu"].shape), mc, output_context=ctx_out)
        c = L.ConjCall(TINY_CONJ, B, vm, vc, ctx_out=ctx_out)
        rows = L.conj_flop_ledger(c, o)
        gemm = sum(x.flops for x in L.conj_gemms(c))
        attn = L.conj_main_attn_flops(c) + L.conj_cross_attn_flops(c) + L.conj_small_attn_flops(c)
        print(L.format_ledger("tiny conjoined B=%d vm=%d vc=%d ctx_out=%d" % (B, vm, vc, ctx_out), rows, (gemm, attn)))
        assert rows[-1][1] == gemm and rows[-1][2] == attn
    assert L.conj_cross_attn_flops(c) == 8 * B * (vm * vc + c.Nx * c.Mx) * 128  # one encoder and one decoder cross block, width 128
