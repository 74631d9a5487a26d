"""The books the kernel timers (cwm_timing_enable / cwm_timing_collect, cwm_conj_timing_*; include/cwm_hip.h CWM_KCLASS_*) must hold after a forward,
stated once and independently of csrc/engine.hip.

FLOPs come from the REFERENCE ARITHMETIC: the CPU oracle (oracle/vmae_oracle.py, oracle/conj_oracle.py) run under torch's FlopCounterMode -- its `bmm` count is
the attention work, everything else (`addmm`, `mm`, convolutions) the matrix-product work -- plus a list of NAMED TERMS, each a closed form in the configuration
and the call and each tied to a documented skip or surplus of the library (rows it does not compute, K it pads).  `expected = oracle + sum(terms)`; a remainder
nobody named is a finding.  Bytes (classes 4-7) and launch counts restate the header's formulas over the schedule of one forward (csrc/model.hip forward_lane:
index prologue, embed, encoder blocks, encoder.norm + encoder_to_decoder + mask tokens, decoder blocks, norm + head, un-embed).

Everything here is an integer far below 2^53: the tests compare with ==.  tests/test_timer_ledger_cpu.py checks the ledger against itself (oracle + terms ==
the schedule's closed form, for every option), so that a GPU failure points at the library's books."""
from collections import OrderedDict
from dataclasses import dataclass

import torch
from torch.utils.flop_counter import FlopCounterMode

import gemm_plan_restatement as GP
from oracle import conj_oracle as CO, vmae_oracle as VO

KCLASS_NAMES = {0: "GEMM", 1: "ATTENTION", 2: "GEMM_WIDE", 3: "GEMM_NARROW", 4: "LAYERNORM", 5: "PATCH_GATHER", 6: "FILL_MASK", 7: "UNEMBED", 8: "CROSS_ATTN",
                9: "SMALL_ATTN"}


def round_up(a, b):
    return (a + b - 1) // b * b


def spec_of(cfg):
    """the oracle's VmaeSpec of a VmaeConfig"""
    return VO.VmaeSpec(img_size=tuple(cfg.img_size), patch=cfg.patch, num_frames=cfg.num_frames, in_chans=cfg.in_chans, enc_dim=cfg.enc_dim,
                       enc_depth=cfg.enc_depth, enc_heads=cfg.enc_heads, dec_dim=cfg.dec_dim, dec_depth=cfg.dec_depth, dec_heads=cfg.dec_heads,
                       mlp_ratio=cfg.mlp_ratio)


def conj_spec_of(cfg):
    return CO.ConjSpec(main=spec_of(cfg.main), main_max_pad=cfg.main_max_pad, ctx_in_chans=cfg.ctx_in_chans, ctx_seq_len=cfg.ctx_seq_len,
                       ctx_tubelet=cfg.ctx_tubelet, ctx_enc_dim=cfg.ctx_enc_dim, ctx_dec_dim=cfg.ctx_dec_dim, ctx_enc_heads=cfg.ctx_enc_heads,
                       ctx_dec_heads=cfg.ctx_dec_heads, ctx_max_pad=cfg.ctx_max_pad, enc_cross=tuple(cfg.enc_cross), dec_cross=tuple(cfg.dec_cross),
                       cross_heads=cfg.cross_heads, cross_mlp_ratio=float(cfg.cross_mlp_ratio))


# ---- the oracle's own count --------------------------------------------------------------------------------------------------------------------------------
def count_flops(fn):
    """{"matmul": FLOPs of every matrix product that is not a batched one, "bmm": FLOPs of the batched ones (attention), "by_op": per aten op} of fn()"""
    with torch.no_grad(), FlopCounterMode(display=False) as fc:
        fn()
    by_op = {str(op).replace("aten.", ""): int(n) for op, n in fc.get_flop_counts()["Global"].items()}
    bmm = sum(n for op, n in by_op.items() if op.startswith("bmm") or op.startswith("baddbmm"))
    return {"matmul": sum(by_op.values()) - bmm, "bmm": bmm, "by_op": by_op}


def _zero_weights(schema):
    return {k: torch.zeros(tuple(shp)) for k, shp in schema.items()}


def vmae_oracle_flops(cfg, mask):
    """FLOPs of `vmae_forward` for this configuration and (rectangular) mask; the count depends on shapes only, so weights and frames are zeros.
    Nothing masked: the reference's forward cannot build its empty mask-token block (`pos[mask].reshape(B, -1, C)` of no element), and its decoder then
    returns head(norm(x)) of every token (vmae.py:250-253): the same oracle pieces, composed without that block."""
    from counterfactualworldmodels_amd import config as C

    spec, B = spec_of(cfg), mask.shape[0]
    W = _zero_weights(C.state_dict_schema(cfg))
    x = torch.zeros(B, cfg.in_chans, cfg.num_frames, *cfg.img_size)
    if bool(mask.any()):
        return count_flops(lambda: VO.vmae_forward(W, spec, x, mask))

    def all_visible():
        x_vis = torch.nn.functional.linear(VO.encoder_forward(W, spec, x, mask), W["encoder_to_decoder.weight"])
        return VO.decoder_forward(W, spec, x_vis + VO.sinusoid_table(mask.shape[1], spec.dec_dim)[None], 0)

    return count_flops(all_visible)


def conj_oracle_flops(cfg, x_shape, mask, imu_shape, mask_context, output_context=False):
    from counterfactualworldmodels_amd import config as C

    W = _zero_weights(C.conj_state_dict_schema(cfg))
    return count_flops(lambda: CO.conj_forward(W, conj_spec_of(cfg), torch.zeros(*x_shape), mask, torch.zeros(*imu_shape), mask_context, output_context))


# ---- one call of the plain predictor -------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class VmaeCall:
    """What decides the books of one cwm_forward: the configuration, the batch, the cap of the visible counts (`n_vis`), the handle's ragged minimum (0: a
    rectangular batch), the mode's planes, whether y_video_dev is set, and the three options that change which rows are computed or how they are launched."""
    cfg: object
    B: int
    n_vis: int
    n_vis_min: int = 0
    planes: int = 2
    video: bool = False
    prune_last_block: int = 1
    mask_token_tables: int = 1
    index_fused: int = 1

    @property
    def Nt(self):
        return self.cfg.num_tokens

    @property
    def Nm(self):  # the rows the decoder returns (model.hip forward_lane: from the least visible count on)
        return self.Nt - (self.n_vis_min if self.n_vis_min > 0 else self.n_vis)

    @property
    def n_ret(self):  # nothing masked: every token (vmae.py:250-253)
        return self.Nm if self.Nm > 0 else self.Nt

    @property
    def pruned(self):
        return self.Nm > 0 and bool(self.prune_last_block)

    @property
    def tables(self):  # a rectangular batch with masked tokens (model.hip cwm_forward)
        return bool(self.mask_token_tables) and self.Nt - self.n_vis > 0 and self.n_vis_min == 0

    @property
    def k_embed(self):
        return self.cfg.in_chans * self.cfg.patch * self.cfg.patch

    def lane(self, B):
        return VmaeCall(self.cfg, B, self.n_vis, self.n_vis_min, self.planes, self.video, self.prune_last_block, self.mask_token_tables, self.index_fused)


# ---- named terms: what the library computes less (or more) than the reference -------------------------------------------------------------------------------
def term_embed_visible_rows(c):
    """the reference embeds all Nt patches and then gathers the visible ones (vmae.py:162-167); the library gathers first"""
    return -2 * c.B * (c.Nt - c.n_vis) * c.k_embed * c.cfg.enc_dim


def term_mask_token_tables(c):
    """"mask_token_tables": decoder block 0's Q/K/V projection runs on the B * n_vis rows that are no mask tokens; the others are copied from a table"""
    return -2 * c.B * (c.Nt - c.n_vis) * c.cfg.dec_dim * 3 * c.cfg.dec_dim if c.tables else 0


def term_pruned_block_gemms(c):
    """"prune_last_block": proj, fc1 and fc2 of the last decoder block on the B * Nm rows the head reads"""
    Dd, hid = c.cfg.dec_dim, c.cfg.mlp_ratio * c.cfg.dec_dim
    return -2 * c.B * (c.Nt - c.Nm) * (Dd * Dd + 2 * Dd * hid) if c.pruned else 0


def term_pruned_block_attention(c):
    """"prune_last_block": the last decoder block's attention computes Nm query rows against all Nt keys"""
    return -4 * c.B * c.cfg.dec_heads * (c.Nt - c.Nm) * c.Nt * 64 if c.pruned else 0


def term_ragged_head_rows(c):
    """a ragged handle returns the rows from the LEAST visible count on (y_tokens is [B, Nt - n_vis_min, out]); the reference, run at the cap, returns Nt - n_vis"""
    oracle_rows = c.Nt - c.n_vis if c.Nt > c.n_vis else c.Nt
    return 2 * c.B * (c.n_ret - oracle_rows) * c.cfg.dec_dim * c.cfg.out_dim


def term_padded_k(gemms):
    """GEMMs are booked with K rounded up to 64 (the zero-padded operand tiles the hardware executes): + 2 M N (Kpad - K) per GEMM"""
    return sum(2 * g.M * g.N * (round_up(g.K, 64) - g.K) for g in gemms)


# ---- the schedule of one lane ----------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Gemm:
    name: str
    M: int
    N: int
    K: int
    epi: int

    @property
    def flops(self):  # as booked: K rounded up to 64
        return 2 * self.M * self.N * round_up(self.K, 64)


def _block_gemms(pre, rows_qkv, rows_out, D, hidden):
    return [Gemm(pre + "qkv", rows_qkv, 3 * D, D, GP.EPI_QKV), Gemm(pre + "proj", rows_out, D, D, GP.EPI_F32),
            Gemm(pre + "fc1", rows_out, hidden, D, GP.EPI_BF16_GELU), Gemm(pre + "fc2", rows_out, D, hidden, GP.EPI_F32)]


def vmae_gemms(c):
    """every GEMM of one lane of c.B samples, in launch order"""
    cfg, B = c.cfg, c.B
    g = [Gemm("embed", B * c.n_vis, cfg.enc_dim, c.k_embed, GP.EPI_F32)]
    for i in range(cfg.enc_depth):
        g += _block_gemms("enc%d." % i, B * c.n_vis, B * c.n_vis, cfg.enc_dim, cfg.mlp_ratio * cfg.enc_dim)
    g.append(Gemm("encoder_to_decoder", B * c.n_vis, cfg.dec_dim, cfg.enc_dim, GP.EPI_F32))
    for i in range(cfg.dec_depth):
        n_in = c.n_vis if (i == 0 and c.tables) else c.Nt
        n_out = c.Nm if (i == cfg.dec_depth - 1 and c.pruned) else c.Nt
        g += _block_gemms("dec%d." % i, B * n_in, B * n_out, cfg.dec_dim, cfg.mlp_ratio * cfg.dec_dim)
    g.append(Gemm("head", B * c.n_ret, cfg.out_dim, cfg.dec_dim, GP.EPI_F32))
    return g


def vmae_attention(c):
    """(query rows, keys, heads) of every attention launch of one lane.  A ragged handle is booked by launch extent: n_vis rows and keys per sample."""
    cfg = c.cfg
    a = [(c.n_vis, c.n_vis, cfg.enc_heads)] * cfg.enc_depth
    for i in range(cfg.dec_depth):
        a.append((c.Nm if (i == cfg.dec_depth - 1 and c.pruned) else c.Nt, c.Nt, cfg.dec_heads))
    return a


def vmae_layernorm_rows(c):
    """(rows, D) of every LayerNorm launch of one lane"""
    cfg, B = c.cfg, c.B
    r = [(B * c.n_vis, cfg.enc_dim)] * (2 * cfg.enc_depth) + [(B * c.n_vis, cfg.enc_dim)]  # LN1, LN2 of every encoder block; encoder.norm
    for i in range(cfg.dec_depth):
        r.append((B * (c.n_vis if (i == 0 and c.tables) else c.Nt), cfg.dec_dim))                   # LN1 (block 0 with the table: the visible rows)
        r.append((B * (c.Nm if (i == cfg.dec_depth - 1 and c.pruned) else c.Nt), cfg.dec_dim))      # LN2 (the pruned block: the kept rows)
    r.append((B * c.n_ret, cfg.dec_dim))                                                            # decoder.norm
    return r


def gemm_parts(g, planes, overlapped, cus, gemm_tile=0, gemm_debug=0):
    """the launches of one GEMM as tests/gemm_plan_restatement.py lays them out: [(rows, runs the 256x256 8-phase kernel)]"""
    _, parts = GP.plan(g.M, g.N, round_up(g.K, 64), g.epi, planes, overlapped, cus, gemm_tile, gemm_debug)
    return [(M, kernel == GP.KERNEL_8PHASE) for _, M, kernel, _ in parts]


def lane_batches(B, lanes):
    """cwm_forward: lane l owns batch rows [ceil(B l / n), ceil(B (l + 1) / n))"""
    first = [(B * l + lanes - 1) // lanes for l in range(lanes + 1)]
    return [first[l + 1] - first[l] for l in range(lanes)]


def vmae_books(c, lanes=1, cus=256, gemm_tile=1, gemm_debug=0):
    """{class name: (launches, total_flops)} of one cwm_forward run as `lanes` lanes, from the schedule alone.  `gemm_tile` = 1: every GEMM is one launch;
    other values take the parts (and the wide / narrow split) from the plan restatement with `cus` compute units."""
    books = OrderedDict((n, [0, 0]) for n in ("GEMM", "ATTENTION", "GEMM_WIDE", "GEMM_NARROW", "LAYERNORM", "PATCH_GATHER", "FILL_MASK", "UNEMBED"))

    def book(name, work):
        books[name][0] += 1
        books[name][1] += work

    cfg = c.cfg
    for Bl in lane_batches(c.B, lanes):
        l = c.lane(Bl)
        for g in vmae_gemms(l):
            for rows, wide in gemm_parts(g, c.planes, lanes >= 2, cus, gemm_tile, gemm_debug):
                fl = 2 * rows * g.N * round_up(g.K, 64)
                book("GEMM", fl)
                book("GEMM_WIDE" if wide else "GEMM_NARROW", fl)
        for n_q, n, heads in vmae_attention(l):
            book("ATTENTION", 4 * n_q * n * 64 * heads * Bl)
        for rows, D in vmae_layernorm_rows(l):
            book("LAYERNORM", rows * D * (4 + 2 * c.planes))
        gather = Bl * c.n_vis * c.k_embed * (4 + 2 * c.planes)
        # the fused prologue also reads the mask row and writes the permutation (and its inverse when the un-embed will read it); of the four launches of
        # "index_fused" = 0 (memset, mask_to_perm, patch_gather, perm_to_rank) the gather alone is booked
        book("PATCH_GATHER", gather + (Bl * c.Nt * (1 + 4 + (4 if c.video else 0)) if c.index_fused else 0))
        if c.Nm > 0:
            book("FILL_MASK", Bl * c.Nm * cfg.dec_dim * 4)
        if c.tables:
            book("FILL_MASK", Bl * (c.Nt - c.n_vis) * 3 * cfg.dec_dim * 2 * c.planes)
        if c.video:
            book("UNEMBED", Bl * cfg.num_frames * cfg.in_chans * cfg.img_size[0] * cfg.img_size[1] * 8)
    return OrderedDict((k, tuple(v)) for k, v in books.items())


def vmae_flop_ledger(c, oracle):
    """The itemised FLOP books of one call: [(item, GEMM FLOPs, attention FLOPs)], the oracle's count first, then every named term; the last row is the sum --
    what CWM_KCLASS_GEMM and CWM_KCLASS_ATTENTION must hold.  `oracle`: vmae_oracle_flops of the call's configuration at a rectangular mask of c.n_vis visible
    tokens per row."""
    rows = [("oracle (addmm + mm | bmm)", oracle["matmul"], oracle["bmm"]),
            ("patch embed on the visible rows only", term_embed_visible_rows(c), 0),
            ("mask-token tables: decoder block 0's QKV on B*n_vis rows", term_mask_token_tables(c), 0),
            ("pruned last decoder block: proj, fc1, fc2 on B*Nm rows", term_pruned_block_gemms(c), 0),
            ("pruned last decoder block: attention of Nm query rows", 0, term_pruned_block_attention(c)),
            ("ragged handle: head rows from the least visible count on", term_ragged_head_rows(c), 0),
            ("K rounded up to 64 (zero-padded operand tiles)", term_padded_k(vmae_gemms(c)), 0)]
    rows.append(("expected books", sum(r[1] for r in rows), sum(r[2] for r in rows)))
    return rows


def format_ledger(title, rows, booked=None):
    out = ["[ledger] %s" % title] + ["    %-62s %16d %16d" % r for r in rows]
    if booked is not None:
        out.append("    %-62s %16d %16d" % (("booked by the library",) + tuple(int(b) for b in booked)))
    return "\n".join(out)


# ---- the conjoined (IMU-conditioned) predictor ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ConjCall:
    cfg: object
    B: int
    vm: int   # n_vis_max: visible main-stream slots per row (pad slots included)
    vc: int   # n_vis_ctx_max
    planes: int = 2
    main_out: bool = True
    ctx_out: bool = False

    @property
    def Nt(self):
        return self.cfg.main.num_tokens

    @property
    def Nx(self):  # slots of the main stream
        return self.Nt + self.cfg.main_max_pad

    @property
    def Mt(self):
        return self.cfg.ctx_tokens

    @property
    def Mx(self):
        return self.Mt + self.cfg.ctx_max_pad

    @property
    def k_main(self):
        return self.cfg.main.in_chans * self.cfg.main.patch * self.cfg.main.patch

    @property
    def k_ctx(self):
        return self.cfg.ctx_in_chans * self.cfg.ctx_tubelet


def conj_cross_blocks(c):
    """(N, M, width) of every cross block in launch order: the encoder's on the visible slots, the decoder's on all slots"""
    cfg = c.cfg
    return [(c.vm, c.vc, cfg.main.enc_dim) for _ in cfg.enc_cross] + [(c.Nx, c.Mx, cfg.main.dec_dim) for _ in cfg.dec_cross]


def conj_gemms(c):
    """every GEMM of one conjoined forward in launch order (csrc/conj_model.hip conj_forward_lane, run_cross)"""
    cfg, m, B = c.cfg, c.cfg.main, c.B
    F32 = GP.EPI_F32

    def cross(pre, N, ci, M, cs):
        D, r = ci, cfg.cross_mlp_ratio
        return [Gemm(pre + "qk", B * N, 2 * D, ci, F32), Gemm(pre + "v", B * N, D, ci, F32), Gemm(pre + "qk_src", B * M, 2 * D, cs, F32),
                Gemm(pre + "v_src", B * M, D, cs, F32), Gemm(pre + "proj", B * N, ci, D, F32), Gemm(pre + "mlp_trg0", B * N, r * ci, ci, GP.EPI_BF16_GELU),
                Gemm(pre + "mlp_trg2", B * N, ci, r * ci, F32), Gemm(pre + "proj_src", B * M, cs, D, F32),
                Gemm(pre + "mlp_src0", B * M, r * cs, cs, GP.EPI_BF16_GELU), Gemm(pre + "mlp_src2", B * M, cs, r * cs, F32)]

    g = [Gemm("main embed", B * c.vm, m.enc_dim, c.k_main, F32), Gemm("context embed", B * c.vc, cfg.ctx_enc_dim, c.k_ctx, F32)]
    for i in range(m.enc_depth):
        if i in cfg.enc_cross:
            g += cross("enc_cross%d." % i, c.vm, m.enc_dim, c.vc, cfg.ctx_enc_dim)
        g += _block_gemms("enc%d." % i, B * c.vm, B * c.vm, m.enc_dim, m.mlp_ratio * m.enc_dim)
        g += _block_gemms("ctx_enc%d." % i, B * c.vc, B * c.vc, cfg.ctx_enc_dim, m.mlp_ratio * cfg.ctx_enc_dim)
    g += [Gemm("encoder_to_decoder", B * c.vm, m.dec_dim, m.enc_dim, F32), Gemm("ctx encoder_to_decoder", B * c.vc, cfg.ctx_dec_dim, cfg.ctx_enc_dim, F32)]
    for i in range(m.dec_depth):
        g += _block_gemms("dec%d." % i, B * c.Nx, B * c.Nx, m.dec_dim, m.mlp_ratio * m.dec_dim)
        g += _block_gemms("ctx_dec%d." % i, B * c.Mx, B * c.Mx, cfg.ctx_dec_dim, m.mlp_ratio * cfg.ctx_dec_dim)
        if i in cfg.dec_cross:
            g += cross("dec_cross%d." % i, c.Nx, m.dec_dim, c.Mx, cfg.ctx_dec_dim)
    if c.ctx_out:
        g.append(Gemm("ctx head", B * (c.Mx - c.vc), c.k_ctx, cfg.ctx_dec_dim, F32))
    if c.main_out and c.Nx > c.vm:
        g.append(Gemm("head", B * (c.Nx - c.vm), m.out_dim, m.dec_dim, F32))
    return g


def conj_cross_attn_flops(c):
    """CWM_KCLASS_CROSS_ATTN: both directions, each a score product and a P.V product -- 2 * (4 N M hd) per head, hd = width / cross_heads.  The reference
    (transformer.py:357-371 with shared_similarity=False, the shipped factories' setting) and the oracle compute the same four products: no term."""
    return sum(8 * c.B * N * M * D for N, M, D in conj_cross_blocks(c))  # heads * hd = D


def conj_small_attn_flops(c):
    """CWM_KCLASS_SMALL_ATTN: the context stream's self-attention, 4 n^2 hd per head: the encoder's on vc slots, the decoder's on all Mx"""
    cfg = c.cfg
    return cfg.main.enc_depth * 4 * c.B * c.vc * c.vc * cfg.ctx_enc_dim + cfg.main.dec_depth * 4 * c.B * c.Mx * c.Mx * cfg.ctx_dec_dim


def conj_main_attn_flops(c):
    m = c.cfg.main
    return m.enc_depth * 4 * c.B * c.vm * c.vm * m.enc_dim + m.dec_depth * 4 * c.B * c.Nx * c.Nx * m.dec_dim


def conj_flop_ledger(c, oracle):
    """as vmae_flop_ledger; the attention column is CWM_KCLASS_ATTENTION + CROSS_ATTN + SMALL_ATTN together.  Pad slots, null tokens and the context stream's
    blocks are in the oracle's run; the library embeds the visible slots of both streams only and pads both embeds' K (48 -> 64, 96 -> 128)."""
    cfg = c.cfg
    embeds = [Gemm("main embed", c.B * c.vm, cfg.main.enc_dim, c.k_main, GP.EPI_F32), Gemm("context embed", c.B * c.vc, cfg.ctx_enc_dim, c.k_ctx, GP.EPI_F32)]
    rows = [("oracle (addmm + mm | bmm)", oracle["matmul"], oracle["bmm"]),
            ("main patch embed on the visible slots only", -2 * c.B * (c.Nt - c.vm) * c.k_main * cfg.main.enc_dim, 0),
            ("context embed on the visible slots only", -2 * c.B * (c.Mt - c.vc) * c.k_ctx * cfg.ctx_enc_dim, 0),
            ("main head not requested", 0 if c.main_out else -2 * c.B * (c.Nx - c.vm) * cfg.main.dec_dim * cfg.main.out_dim, 0),
            ("cross attention: four products in the reference too", 0, 0),
            ("K rounded up to 64 (zero-padded operand tiles)", term_padded_k(embeds), 0)]
    rows.append(("expected books", sum(r[1] for r in rows), sum(r[2] for r in rows)))
    return rows
