"""`gemm_plan` (csrc/gemm.hip), read out through the development library's `cwm_dev_gemm_plan`, against tests/gemm_plan_restatement.py -- the launch
layout as the launcher and the engine decided it before there was a plan -- over the GEMM shapes of the models, every tile option and every
`gemm_debug` bit that reaches the rule, at the MI355X's 256 compute units and at 304.  No GPU needed: a plan is host arithmetic."""
import ctypes
import itertools

import pytest

import gemm_plan_restatement as R
from counterfactualworldmodels_amd import _lib

F32, GELU, QKV = R.EPI_F32, R.EPI_BF16_GELU, R.EPI_QKV
BATCHES = list(range(1, 13)) + [16, 20, 24, 32, 48]
TILES = (0, 1, 4, 6)
DEBUG_BITS = (4, 32, 128, 256, 512, 1024)


def sweep_shapes():
    """(M, N, K, epi) of every launch the sweep covers"""
    out = []
    vit_b = [(2304, 768, QKV), (768, 768, F32), (3072, 768, GELU), (768, 3072, F32), (384, 768, F32), (1152, 384, QKV), (384, 384, F32), (1536, 384, GELU),
             (384, 1536, F32), (192, 384, F32)]
    vit_l = [(3072, 1024, QKV), (1024, 1024, F32), (4096, 1024, GELU), (1024, 4096, F32), (512, 1024, F32), (1536, 512, QKV), (512, 512, F32),
             (2048, 512, GELU), (512, 2048, F32)]
    for rows, nke in (((792, 1568), vit_b), ((784, 3136), vit_l)):
        out += [(B * r, N, K, epi) for B in BATCHES for r in rows for N, K, epi in nke]
    update = [(256, 384), (192, 2304), (128, 128), (64, 1152), (128, 2304), (256, 1920), (128, 1920), (256, 1152), (16, 2304), (576, 256)]
    out += [(P * r, N, K, F32) for P in (1, 2, 4, 8) for r in (256, 320, 323, 784) for N, K in update]
    encoder = [(12544, [(64, 192), (64, 576)]), (3136, [(96, 576), (96, 896)]), (784, [(128, 896), (128, 1152), (256, 128)])]
    out += [(2 * P * r, N, K, F32) for P in (1, 2, 4, 8) for r, nk in encoder for N, K in nk]
    return out


def library_plan(d, M, N, K, epi, mode, overlapped, cus, forced_cfg=0):
    out = _lib.CwmDevGemmPlanOut()
    _lib.check(d.cwm_dev_gemm_plan(M, N, K, epi, _lib.mode_id(mode), overlapped, forced_cfg, cus, ctypes.byref(out)), d)
    assert all(v == 0 for i in range(out.nparts, 2) for v in (out.part[i].m_offset, out.part[i].M, out.part[i].kernel, out.part[i].splitk))
    return out.cfg, [(q.m_offset, q.M, q.kernel, q.splitk) for q in out.part[:out.nparts]]


@pytest.fixture(scope="module")
def plans():
    """{cus: {(shape, mode, overlapped, gemm_tile, gemm_debug): (library's plan, restated plan)}}, computed once"""
    d = _lib.get_dev_lib()
    shapes = sweep_shapes()
    assert len(shapes) == 834
    shapes = sorted(set(shapes))  # (B x 1568 = 2B x 792 and the like: 762 distinct launches)
    res = {256: {}, 304: {}}
    try:
        for tile, dbg in itertools.product(TILES, (0,) + DEBUG_BITS):
            _lib.check(d.cwm_debug_set(b"gemm_tile", tile), d)
            _lib.check(d.cwm_debug_set(b"gemm_debug", dbg), d)
            for cus, shape, mode, ovl in itertools.product(res, shapes, ("parity", "fast"), (0, 1)):
                planes = 2 if mode == "parity" else 1
                res[cus][(shape, mode, ovl, tile, dbg)] = (library_plan(d, *shape, mode, ovl, cus), R.plan(*shape[:3], shape[3], planes, ovl, cus, tile, dbg))
    finally:
        d.cwm_debug_set(b"gemm_tile", 0)
        d.cwm_debug_set(b"gemm_debug", 0)
    return res


@pytest.mark.parametrize("cus", [256, 304])
def test_plan_equals_the_restated_launcher(plans, cus):
    bad = [(k, got, want) for k, (got, want) in plans[cus].items() if got != want]
    assert not bad, "%d of %d plans differ, first: %s" % (len(bad), len(plans[cus]), bad[:3])
    for (shape, *_), ((cfg, parts), _) in plans[cus].items():  # and every plan covers the rows once, in order
        assert parts[0][0] == 0 and sum(q[1] for q in parts) == shape[0] and all(a[0] + a[1] == b[0] for a, b in zip(parts, parts[1:]))
        assert (cfg == 6) == (len(parts) == 2)


def test_sweep_reaches_every_outcome(plans):
    """at 256 CUs: the three configurations, the four kernels, split-K of three parts and more, every gemm_debug bit, and a 6 that has no whole round"""
    got = {k: v[0] for k, v in plans[256].items()}
    default = {k: v for k, v in got.items() if k[3] == 0 and k[4] == 0}
    assert len(default) == 762 * 4
    assert {cfg for cfg, _ in default.values()} == {1, 4, 6}
    assert {q[2] for _, parts in default.values() for q in parts} == {R.KERNEL_128, R.KERNEL_DEEP128, R.KERNEL_DEEP64, R.KERNEL_8PHASE}
    assert {q[3] for _, parts in default.values() for q in parts} >= {1, 3, 4, 5, 6}
    for bit in DEBUG_BITS:
        assert any(got[k[:4] + (bit,)] != v for k, v in default.items()), "gemm_debug %d changes no plan" % bit
    forced6 = [v for k, v in got.items() if k[3] == 6 and k[4] == 0]
    assert any(cfg == 6 for cfg, _ in forced6)
    assert any(cfg == 1 and parts[0][2] != R.KERNEL_8PHASE for cfg, parts in forced6)


def test_forced_configuration_stands_for_the_gemm_tile_option(plans):
    """the read-out's forced_cfg argument (what a caller of gemm_plan may pass) = the same value of "gemm_tile" """
    d = _lib.get_dev_lib()
    for (shape, mode, ovl, tile, dbg), (got, _) in plans[256].items():
        if tile and dbg == 0 and ovl == 0:
            assert library_plan(d, *shape, mode, ovl, 256, forced_cfg=tile) == got


def test_plan_refuses_what_the_launcher_refused():
    d = _lib.get_dev_lib()
    out = _lib.CwmDevGemmPlanOut()
    assert d.cwm_dev_gemm_plan(792, 768, 100, F32, _lib.mode_id("fast"), 0, 0, 256, ctypes.byref(out)) != 0 and b"multiple of 64" in d.cwm_last_error()
    assert d.cwm_dev_gemm_plan(792, 768, 768, F32, _lib.mode_id("fast"), 0, 5, 256, ctypes.byref(out)) != 0 and b"unknown tile configuration" in d.cwm_last_error()
