"""Model shapes and state-dict schema of the VMAE predictors this package accelerates.

Mirrors the constructor arguments / factory functions of the reference
(`cwm/models/VideoMAE/vmae.py:257-384`, factories `:563-619`) so that published
checkpoints load unchanged (key names and shapes: SURVEY.md Appendix B).
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Tuple  # noqa: F401

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
LN_EPS = 1e-6


@dataclass(frozen=True)
class VmaeConfig:
    name: str = "base_8x8patch_2frames_1tube"
    img_size: Tuple[int, int] = (224, 224)
    patch: int = 8
    num_frames: int = 2
    in_chans: int = 3
    enc_dim: int = 768
    enc_depth: int = 12
    enc_heads: int = 12
    dec_dim: int = 384
    dec_depth: int = 4
    dec_heads: int = 6
    mlp_ratio: int = 4

    @property
    def tokens_per_frame(self) -> int:
        return (self.img_size[0] // self.patch) * (self.img_size[1] // self.patch)

    @property
    def num_tokens(self) -> int:
        return self.tokens_per_frame * self.num_frames

    @property
    def patch_dim(self) -> int:
        return self.in_chans * self.patch * self.patch

    @property
    def out_dim(self) -> int:
        return self.in_chans * self.patch * self.patch

    def with_image_size(self, hw) -> "VmaeConfig":
        from dataclasses import replace

        return replace(self, img_size=(int(hw[0]), int(hw[1])))


CONFIGS: Dict[str, VmaeConfig] = {
    "base_8x8patch_2frames_1tube": VmaeConfig(),  # vmae.py:605
    "base_16x16patch_2frames_1tube": VmaeConfig(name="base_16x16patch_2frames_1tube", patch=16),  # vmae.py:597
    "large_4x4patch_2frames_1tube": VmaeConfig(  # vmae.py:613
        name="large_4x4patch_2frames_1tube",
        patch=4,
        enc_dim=1024,
        enc_depth=24,
        enc_heads=16,
        dec_dim=512,
        dec_depth=12,
        dec_heads=8,
    ),
}


def _block_schema(pre: str, d: int, hidden: int, out: "OrderedDict[str, tuple]") -> None:
    out[pre + "norm1.weight"] = (d,)
    out[pre + "norm1.bias"] = (d,)
    out[pre + "attn.q_bias"] = (d,)
    out[pre + "attn.v_bias"] = (d,)
    out[pre + "attn.qkv.weight"] = (3 * d, d)
    out[pre + "attn.proj.weight"] = (d, d)
    out[pre + "attn.proj.bias"] = (d,)
    out[pre + "norm2.weight"] = (d,)
    out[pre + "norm2.bias"] = (d,)
    out[pre + "mlp.fc1.weight"] = (hidden, d)
    out[pre + "mlp.fc1.bias"] = (hidden,)
    out[pre + "mlp.fc2.weight"] = (d, hidden)
    out[pre + "mlp.fc2.bias"] = (d,)


def state_dict_schema(cfg: VmaeConfig) -> "OrderedDict[str, tuple]":
    """Parameter names -> shapes, in the reference's registration order."""
    s: "OrderedDict[str, tuple]" = OrderedDict()
    s["mask_token"] = (1, 1, cfg.dec_dim)
    s["encoder.patch_embed.proj.weight"] = (cfg.enc_dim, cfg.in_chans, 1, cfg.patch, cfg.patch)
    s["encoder.patch_embed.proj.bias"] = (cfg.enc_dim,)
    for i in range(cfg.enc_depth):
        _block_schema(f"encoder.blocks.{i}.", cfg.enc_dim, cfg.mlp_ratio * cfg.enc_dim, s)
    s["encoder.norm.weight"] = (cfg.enc_dim,)
    s["encoder.norm.bias"] = (cfg.enc_dim,)
    for i in range(cfg.dec_depth):
        _block_schema(f"decoder.blocks.{i}.", cfg.dec_dim, cfg.mlp_ratio * cfg.dec_dim, s)
    s["decoder.norm.weight"] = (cfg.dec_dim,)
    s["decoder.norm.bias"] = (cfg.dec_dim,)
    s["decoder.head.weight"] = (cfg.out_dim, cfg.dec_dim)
    s["decoder.head.bias"] = (cfg.out_dim,)
    s["encoder_to_decoder.weight"] = (cfg.dec_dim, cfg.enc_dim)
    return s


def num_parameters(cfg: VmaeConfig) -> int:
    n = 0
    for shp in state_dict_schema(cfg).values():
        k = 1
        for v in shp:
            k *= v
        n += k
    return n


def algorithmic_flops(cfg: VmaeConfig, n_vis: int) -> float:
    """GEMM + attention FLOPs (2*MAC) per frame pair, SURVEY.md §8(d)."""
    Nt, De, Dd = cfg.num_tokens, cfg.enc_dim, cfg.dec_dim
    Nm = Nt - n_vis
    f = 2.0 * Nt * cfg.patch_dim * De
    f += cfg.enc_depth * (24.0 * n_vis * De * De + 4.0 * n_vis * n_vis * De)
    f += 2.0 * n_vis * De * Dd
    f += cfg.dec_depth * (24.0 * Nt * Dd * Dd + 4.0 * Nt * Nt * Dd)
    f += 2.0 * Nm * Dd * cfg.out_dim
    return f


# ---------------------------------------------------------------------------------------------
# IMU-conditioned conjoined padded predictor (BASELINE configs[4])
# `imu400_base_4x4patch_2frames_1tube` (cwm/models/VideoMAE/conjoined_vmae.py:1230-1243)
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ConjConfig:
    name: str = "imu400_base_4x4patch_2frames_1tube"
    main: VmaeConfig = VmaeConfig(name="imu400_main_4x4", patch=4)
    main_max_pad: int = 64
    ctx_in_chans: int = 6
    ctx_seq_len: int = 400
    ctx_tubelet: int = 16
    ctx_enc_dim: int = 384
    ctx_dec_dim: int = 192
    ctx_enc_heads: int = 12
    ctx_dec_heads: int = 6
    ctx_max_pad: int = 25
    enc_cross: Tuple[int, ...] = (0, 3, 6, 9)
    dec_cross: Tuple[int, ...] = (0, 1, 2, 3)
    cross_heads: int = 4
    cross_mlp_ratio: int = 2
    # the unpadded flow -> IMU variant (ConjoinedPretrainVisionTransformer, conjoined_vmae.py:212-887); the defaults are the padded model
    padded: bool = True
    ctx_dummy_token: bool = False  # ImuEncoder(concat_dummy_token=True): a learned, always visible 26th IMU token (:1013-1147)
    main_input: str = "rgb01"      # or "flowback_rgb01" (preprocessor.py:208-277, 356): 7 channels from two flows and frame 1

    @property
    def ctx_tokens(self) -> int:
        return self.ctx_seq_len // self.ctx_tubelet

    @property
    def ctx_out_dim(self) -> int:
        return self.ctx_in_chans * self.ctx_tubelet


CONJ_CONFIGS: Dict[str, ConjConfig] = {
    "imu400_base_4x4patch_2frames_1tube": ConjConfig(),
    # the flow -> IMU head-motion predictor (conjoined_vmae.py:1218-1228): one 7-channel frame of 784 tokens, cross blocks before
    # encoder layers 0 and 11 (conjoin_encoder_layers=[0, -1]) and after every decoder layer
    "imu400_8x8patch_2frames_1tube_flowbackrgb01": ConjConfig(
        name="imu400_8x8patch_2frames_1tube_flowbackrgb01",
        main=VmaeConfig(name="flow2imu_main_8x8", patch=8, num_frames=1, in_chans=7),
        main_max_pad=0,
        ctx_max_pad=0,
        enc_cross=(0, 11),
        dec_cross=(0, 1, 2, 3),
        padded=False,
        ctx_dummy_token=True,
        main_input="flowback_rgb01",
    ),
}


def _cross_schema(pre: str, ci: int, cs: int, ratio: int, out: "OrderedDict[str, tuple]") -> None:
    d = ci  # inner width D = heads * (in_dim // heads) = in_dim (transformer.py:272, 300-303)
    out[pre + "norm1_cross.weight"] = (ci,)
    out[pre + "norm1_cross.bias"] = (ci,)
    out[pre + "norm1_src_cross.weight"] = (cs,)
    out[pre + "norm1_src_cross.bias"] = (cs,)
    out[pre + "norm2.weight"] = (ci,)
    out[pre + "norm2.bias"] = (ci,)
    out[pre + "norm2_src.weight"] = (cs,)
    out[pre + "norm2_src.bias"] = (cs,)
    out[pre + "cross_attention.qk.weight"] = (2 * d, ci)
    out[pre + "cross_attention.qk_src.weight"] = (2 * d, cs)
    out[pre + "cross_attention.v.weight"] = (d, ci)
    out[pre + "cross_attention.v_src.weight"] = (d, cs)
    out[pre + "cross_attention.projection.weight"] = (ci, d)
    out[pre + "cross_attention.projection.bias"] = (ci,)
    out[pre + "cross_attention.projection_src.weight"] = (cs, d)
    out[pre + "cross_attention.projection_src.bias"] = (cs,)
    out[pre + "mlp.trg.layers.0.weight"] = (ratio * ci, ci)
    out[pre + "mlp.trg.layers.0.bias"] = (ratio * ci,)
    out[pre + "mlp.trg.layers.2.weight"] = (ci, ratio * ci)
    out[pre + "mlp.trg.layers.2.bias"] = (ci,)
    out[pre + "mlp.src.layers.0.weight"] = (ratio * cs, cs)
    out[pre + "mlp.src.layers.0.bias"] = (ratio * cs,)
    out[pre + "mlp.src.layers.2.weight"] = (cs, ratio * cs)
    out[pre + "mlp.src.layers.2.bias"] = (cs,)


def conj_state_dict_schema(cfg: ConjConfig) -> "OrderedDict[str, tuple]":
    """Parameter names -> shapes in the reference's order (634 tensors)."""
    s: "OrderedDict[str, tuple]" = OrderedDict()
    m = cfg.main
    main = state_dict_schema(m)
    s["main_stream.mask_token"] = main["mask_token"]
    if cfg.padded:
        s["main_stream.null_token_enc"] = (1, 1, m.enc_dim)
        s["main_stream.null_token_dec"] = (1, 1, m.dec_dim)
    for k, v in main.items():
        if k != "mask_token":
            s["main_stream." + k] = v
    c = "context_stream."
    s[c + "mask_token"] = (1, 1, cfg.ctx_dec_dim)
    if cfg.padded:
        s[c + "null_token_enc"] = (1, 1, cfg.ctx_enc_dim)
        s[c + "null_token_dec"] = (1, 1, cfg.ctx_dec_dim)
    if cfg.ctx_dummy_token:
        s[c + "encoder.dummy_token"] = (1, cfg.ctx_in_chans, cfg.ctx_tubelet, 1, 1)
    s[c + "encoder.patch_embed.proj.weight"] = (cfg.ctx_enc_dim, cfg.ctx_in_chans, cfg.ctx_tubelet, 1, 1)
    s[c + "encoder.patch_embed.proj.bias"] = (cfg.ctx_enc_dim,)
    for i in range(m.enc_depth):
        _block_schema(f"{c}encoder.blocks.{i}.", cfg.ctx_enc_dim, m.mlp_ratio * cfg.ctx_enc_dim, s)
    s[c + "encoder.norm.weight"] = (cfg.ctx_enc_dim,)
    s[c + "encoder.norm.bias"] = (cfg.ctx_enc_dim,)
    for i in range(m.dec_depth):
        _block_schema(f"{c}decoder.blocks.{i}.", cfg.ctx_dec_dim, m.mlp_ratio * cfg.ctx_dec_dim, s)
    s[c + "decoder.norm.weight"] = (cfg.ctx_dec_dim,)
    s[c + "decoder.norm.bias"] = (cfg.ctx_dec_dim,)
    s[c + "decoder.head.weight"] = (cfg.ctx_out_dim, cfg.ctx_dec_dim)
    s[c + "decoder.head.bias"] = (cfg.ctx_out_dim,)
    s[c + "encoder_to_decoder.weight"] = (cfg.ctx_dec_dim, cfg.ctx_enc_dim)
    # present in the checkpoints, never used on this path (spacetime_separable_pos_embed=True, vmae.py:368-369)
    s[c + "pos_embed_encoder.weight"] = (cfg.ctx_dec_dim, 2 * cfg.ctx_dec_dim)
    s[c + "pos_embed_encoder.bias"] = (cfg.ctx_dec_dim,)
    for i in cfg.enc_cross:
        _cross_schema(f"encoder_conjoining_blocks.{i}-{i}.", m.enc_dim, cfg.ctx_enc_dim, cfg.cross_mlp_ratio, s)
    for i in cfg.dec_cross:
        _cross_schema(f"decoder_conjoining_blocks.{i}-{i}.", m.dec_dim, cfg.ctx_dec_dim, cfg.cross_mlp_ratio, s)
    return s


# ---- RAFT-large optical flow (cwm/models/raft/raft_model.py:103-161, extractor.py:6-57, 118-192, update.py:6-137) ----------------------
RAFT_HIDDEN = 128  # hidden_dim = context_dim of RAFT-large
RAFT_CORR_LEVELS = 4
RAFT_CORR_RADIUS = 4
RAFT_BN_EPS = 1e-5
RAFT_IN_EPS = 1e-5


def _raft_encoder_schema(pre: str, norm: str, out_dim: int, out: "OrderedDict[str, tuple]") -> None:
    def conv(name, n, c, k):
        out[pre + name + ".weight"] = (n, c, k, k)
        out[pre + name + ".bias"] = (n,)

    def bn(name, c):
        if norm == "batch":
            for p in ("weight", "bias", "running_mean", "running_var"):
                out[pre + name + "." + p] = (c,)
            out[pre + name + ".num_batches_tracked"] = ()

    bn("norm1", 64)  # BasicEncoder registers norm1 before conv1
    conv("conv1", 64, 3, 7)
    cin = 64
    for li, dim in ((1, 64), (2, 96), (3, 128)):
        for bi in range(2):
            b = "layer%d.%d." % (li, bi)
            stride = 2 if (bi == 0 and li > 1) else 1
            conv(b + "conv1", dim, cin, 3)
            conv(b + "conv2", dim, dim, 3)
            bn(b + "norm1", dim)
            bn(b + "norm2", dim)
            if stride != 1:
                bn(b + "norm3", dim)  # the same module as downsample.1: the state dict lists it twice
                conv(b + "downsample.0", dim, cin, 1)
                bn(b + "downsample.1", dim)
            cin = dim
    conv("conv2", out_dim, 128, 1)


def raft_state_dict_schema(output_dim=None) -> "OrderedDict[str, tuple]":
    """State-dict names -> shapes of RAFT-large in the reference's order (179 tensors, `num_batches_tracked` included); with `output_dim`
    the four tensors of `output_block` (raft_model.py:152-159: the keypoint head) follow, 183 in all."""
    s: "OrderedDict[str, tuple]" = OrderedDict()
    _raft_encoder_schema("fnet.", "instance", 256, s)
    _raft_encoder_schema("cnet.", "batch", 2 * RAFT_HIDDEN, s)
    cor_planes = RAFT_CORR_LEVELS * (2 * RAFT_CORR_RADIUS + 1) ** 2
    for name, n, c, kh, kw in (("encoder.convc1", 256, cor_planes, 1, 1), ("encoder.convc2", 192, 256, 3, 3), ("encoder.convf1", 128, 2, 7, 7),
                               ("encoder.convf2", 64, 128, 3, 3), ("encoder.conv", 126, 256, 3, 3),
                               ("gru.convz1", 128, 384, 1, 5), ("gru.convr1", 128, 384, 1, 5), ("gru.convq1", 128, 384, 1, 5),
                               ("gru.convz2", 128, 384, 5, 1), ("gru.convr2", 128, 384, 5, 1), ("gru.convq2", 128, 384, 5, 1),
                               ("flow_head.conv1", 256, 128, 3, 3), ("flow_head.conv2", 2, 256, 3, 3),
                               ("mask.0", 256, 128, 3, 3), ("mask.2", 576, 256, 1, 1)):
        s["update_block." + name + ".weight"] = (n, c, kh, kw)
        s["update_block." + name + ".bias"] = (n,)
    if output_dim is not None:
        s["output_block.0.weight"] = (256, RAFT_HIDDEN, 3, 3)
        s["output_block.0.bias"] = (256,)
        s["output_block.2.weight"] = (int(output_dim), 256, 1, 1)
        s["output_block.2.bias"] = (int(output_dim),)
    return s


def raft_algorithmic_flops(height: int, width: int, iters: int, corr: str = "all_pairs") -> float:
    """FLOPs one frame pair costs on this package's path (2*M*N*K per convolution and for the correlation; the mask head and the
    convex upsampling run once, after the last iteration).  `corr="on_the_fly"` (RAFT.set_corr) books, in place of the all-pairs product, the
    dot products a lookup needs: 4 levels x 100 integer neighbours x 2 * 256 = 204.8 kFLOP per 1/8-resolution pixel and iteration."""
    if corr not in ("all_pairs", "on_the_fly"):
        raise ValueError("corr must be 'all_pairs' or 'on_the_fly', got %r" % (corr,))
    def conv(hw, n, c, k):
        return 2.0 * hw * n * c * k

    h2, h4, h8 = (height // 2) * (width // 2), (height // 4) * (width // 4), (height // 8) * (width // 8)
    enc = conv(h2, 64, 3, 49) + 4 * conv(h2, 64, 64, 9)
    enc += conv(h4, 96, 64, 9) + conv(h4, 96, 96, 9) * 3 + conv(h4, 96, 64, 1)
    enc += conv(h8, 128, 96, 9) + conv(h8, 128, 128, 9) * 3 + conv(h8, 128, 96, 1) + conv(h8, 256, 128, 1)
    upd = (conv(h8, 256, 324, 1) + conv(h8, 192, 256, 9) + conv(h8, 128, 2, 49) + conv(h8, 64, 128, 9) + conv(h8, 126, 256, 9)
           + 6 * conv(h8, 128, 384, 5) + conv(h8, 256, 128, 9) + conv(h8, 2, 256, 9))
    mask = conv(h8, 256, 128, 9) + conv(h8, 576, 256, 1)
    if corr == "on_the_fly":
        return 3 * enc + iters * (upd + RAFT_CORR_LEVELS * 100 * 2.0 * 256 * h8) + mask
    return 3 * enc + 2.0 * h8 * h8 * 256 + iters * upd + mask
