"""Host-side mirror of the reference VMAE predictor classes, backed by libcwm_hip.so.

`PretrainVisionTransformer` keeps the reference's class surface -- constructor semantics of the
factories (`cwm/models/VideoMAE/vmae.py:563-619`), parameter names/shapes (state-dict compatible with
the published checkpoints), attributes read by the wrapper/UI (`patch_size`, `image_size`,
`num_frames`, `mask_size`, `encoder.patch_embed.proj.kernel_size`, ...) and
`forward(x[B,C,T,H,W], mask[B,Nt]) -> [B,Nm,C*P*P]` (`vmae.py:539-560`) -- but holds no compute:
the forward pass is one call into the C ABI (`include/cwm_hip.h: cwm_forward`), which runs the
hand-written HIP kernels.  There is no PyTorch fallback path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
import torch.nn as nn

from . import _lib
from ._handle import LibraryModule, _NoForward
from .config import CONFIGS, LN_EPS, VmaeConfig


def trunc_normal_(tensor, mean=0.0, std=1.0):
    # vmae.py:25-26 (timm's trunc_normal_ == torch.nn.init.trunc_normal_)
    return nn.init.trunc_normal_(tensor, mean=mean, std=std, a=-std, b=std)


def _init_weights(m):
    # vmae.py:100-107 / :212-219
    if isinstance(m, nn.Linear):
        nn.init.xavier_uniform_(m.weight)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.LayerNorm):
        nn.init.constant_(m.bias, 0)
        nn.init.constant_(m.weight, 1.0)


class Attention(_NoForward):
    """Parameter layout of VideoMAE/utils.py:57-85 (fused qkv without bias, separate q/v bias)."""

    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=False)
        self.q_bias = nn.Parameter(torch.zeros(dim))
        self.v_bias = nn.Parameter(torch.zeros(dim))
        self.proj = nn.Linear(dim, dim)


class Mlp(_NoForward):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class Block(_NoForward):
    def __init__(self, dim, num_heads, mlp_ratio):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=LN_EPS)
        self.attn = Attention(dim, num_heads)
        self.norm2 = nn.LayerNorm(dim, eps=LN_EPS)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))


class PatchEmbed(_NoForward):
    def __init__(self, cfg: VmaeConfig):
        super().__init__()
        self.patch_size = (cfg.patch, cfg.patch)
        self.tubelet_size = 1
        self.num_frames = cfg.num_frames
        self.num_patches = cfg.num_tokens
        self.embed_dim = cfg.enc_dim
        self.proj = nn.Conv3d(cfg.in_chans, cfg.enc_dim, kernel_size=(1, cfg.patch, cfg.patch), stride=(1, cfg.patch, cfg.patch))


class PretrainVisionTransformerEncoder(_NoForward):
    def __init__(self, cfg: VmaeConfig):
        super().__init__()
        self.embed_dim = self.num_features = cfg.enc_dim
        self.patch_size = (1, cfg.patch, cfg.patch)
        self.pt, self.ph, self.pw = self.patch_size
        self.patch_embed = PatchEmbed(cfg)
        self.image_size = cfg.img_size[0]
        self.num_patches = cfg.num_tokens
        self.num_frames = cfg.num_frames
        self.blocks = nn.ModuleList([Block(cfg.enc_dim, cfg.enc_heads, cfg.mlp_ratio) for _ in range(cfg.enc_depth)])
        self.norm = nn.LayerNorm(cfg.enc_dim, eps=LN_EPS)
        self.head = nn.Identity()
        self.timestamps = None
        self.apply(_init_weights)


class PretrainVisionTransformerDecoder(_NoForward):
    def __init__(self, cfg: VmaeConfig):
        super().__init__()
        self.embed_dim = self.num_features = cfg.dec_dim
        self.num_classes = cfg.out_dim
        self.patch_size = (cfg.patch, cfg.patch)
        self.blocks = nn.ModuleList([Block(cfg.dec_dim, cfg.dec_heads, cfg.mlp_ratio) for _ in range(cfg.dec_depth)])
        self.norm = nn.LayerNorm(cfg.dec_dim, eps=LN_EPS)
        self.head = nn.Linear(cfg.dec_dim, cfg.out_dim)
        self.apply(_init_weights)


class PretrainVisionTransformer(LibraryModule):
    """Drop-in for `cwm.models.VideoMAE.vmae.PretrainVisionTransformer` (main_input=None models)."""

    def __init__(self, cfg: VmaeConfig, mode: str = "parity", use_flash_attention: bool = True, **unused):
        super().__init__()
        self.cfg = cfg
        self.mode = mode
        _lib.mode_id(mode)
        self.get_main_input = None
        self.encoder = PretrainVisionTransformerEncoder(cfg)
        self.decoder = PretrainVisionTransformerDecoder(cfg)
        self.encoder_to_decoder = nn.Linear(cfg.enc_dim, cfg.dec_dim, bias=False)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, cfg.dec_dim))
        trunc_normal_(self.mask_token, std=0.02)
        self.timestamps = None
        self.num_frames = cfg.num_frames
        self.num_patches = cfg.num_tokens
        self.num_patches_per_frame = cfg.tokens_per_frame
        self.patch_size = self.encoder.patch_size
        self.image_size = tuple(cfg.img_size)
        self.default_cfg = {}

    # ---- reference attribute surface -------------------------------------------------------------
    @property
    def mask_size(self):  # vmae.py:386-390
        return (
            self.num_frames // self.patch_size[0],
            self.image_size[-2] // self.patch_size[-2],
            self.image_size[-1] // self.patch_size[-1],
        )

    def get_num_layers(self):
        return len(self.encoder.blocks)

    # ---- C-ABI plumbing (the handle, sync_weights and the options live in _handle.LibraryModule) -------
    _ABI = {"destroy": "cwm_model_destroy", "load_weight": "cwm_model_load_weight", "forward": "cwm_forward", "set_option": "cwm_model_set_option",
            "set_lanes": "cwm_model_set_lanes", "set_ragged": "cwm_model_set_ragged", "timing_enable": "cwm_timing_enable", "timing_collect": "cwm_timing_collect"}

    def _create(self, lib, h):
        c = self.cfg
        ccfg = _lib.CwmConfig(
            c.img_size[0], c.img_size[1], c.patch, c.num_frames, c.in_chans, c.enc_dim, c.enc_depth, c.enc_heads,
            c.dec_dim, c.dec_depth, c.dec_heads, c.mlp_ratio, LN_EPS,
        )
        return lib.cwm_model_create(C.byref(ccfg), C.byref(h))

    def _run(self, x, strides, normalize, mask, n_vis, want_video, xraw=None, check=True, out_tokens=None, out_video=None, weights_synced=False,
             ragged=False, n_vis_range=None):
        _lib.require_gpu()
        if not x.is_cuda:
            raise RuntimeError("PretrainVisionTransformer.forward needs a CUDA/HIP tensor (no CPU fallback); got %s" % x.device)
        dev = x.device
        if not weights_synced or self._handle is None or self._handle_device != dev:
            self.sync_weights(dev)
        c = self.cfg
        B = x.shape[0]
        Nt = c.num_tokens
        mask = mask.to(device=dev, dtype=torch.bool).reshape(B, -1).contiguous()
        if mask.shape[1] != Nt:
            raise RuntimeError("mask has %d tokens per row, model expects %d" % (mask.shape[1], Nt))
        n_vis_min = 0
        if ragged:
            # rows with different visible counts as ONE batch (cwm_model_set_ragged): `hi` is the cap the encoder runs at, `lo` sizes the output
            vis = Nt - mask.sum(1, dtype=torch.int32)  # (device; read back only when the caller gave no range)
            if n_vis_range is None:
                lo, hi = (int(v) for v in torch.stack([vis.min(), vis.max()]).tolist())
            else:
                lo, hi = (int(v) for v in n_vis_range)
            if not 0 < lo <= hi <= Nt:
                raise RuntimeError("n_vis_range=(%d, %d): need 0 < lo <= hi <= %d tokens" % (lo, hi, Nt))
            n_vis, n_vis_min = hi, lo
        elif n_vis_range is not None:
            raise RuntimeError("n_vis_range goes with ragged=True")
        if n_vis is None:
            n_vis = Nt - int(mask[0].sum().item())
        Nm = Nt - (n_vis_min if ragged else n_vis)
        # nothing masked: the reference returns head(norm(x)) for all Nt tokens (vmae.py:250-253)
        y = self._out_buffer(out_tokens, (B, Nm if Nm > 0 else Nt, c.out_dim), dev)
        video = self._out_buffer(out_video, (B, c.num_frames, c.in_chans, c.img_size[0], c.img_size[1]), dev) if want_video else None
        args = _lib.CwmForwardArgs(
            C.sizeof(_lib.CwmForwardArgs), x.data_ptr(), strides[0], strides[1], strides[2], int(normalize), mask.data_ptr(), B, n_vis, y.data_ptr(),
            _lib.ptr(video), _lib.ptr(xraw), _lib.mode_id(self.mode), int(check), _lib.current_stream_handle(dev),
        )
        with torch.cuda.device(dev):
            if ragged or self.__dict__.get("_ragged_set"):  # (a handle that never ran a ragged batch is never told about them)
                self._check(self._fn["set_ragged"](self._handle, n_vis_min))
                self.__dict__["_ragged_set"] = bool(ragged)
            self._check(self._fn["forward"](self._handle, C.byref(args)))
        if ragged and Nm > 0:
            # row b's predictions are its last Nt - Nv_b rows; what the library leaves before them is unspecified: zeroed (on the device, no read-back)
            lead = (vis - n_vis_min).clamp_(min=0)
            y.masked_fill_((torch.arange(y.shape[1], device=dev)[None, :] < lead[:, None])[:, :, None], 0.0)
        return y, video

    @staticmethod
    def _out_buffer(given, shape, dev):
        """The caller's output tensor (a row slice of a larger result: lets a chunked driver assemble its result without a
        concatenation pass) or a fresh one."""
        if given is None:
            return torch.empty(shape, device=dev, dtype=torch.float32)
        if tuple(given.shape) != tuple(shape) or given.dtype != torch.float32 or given.device != dev or not given.is_contiguous():
            raise RuntimeError("output buffer must be a contiguous float32 tensor of shape %s on %s" % (tuple(shape), dev))
        return given

    @staticmethod
    def _frame_strides(x: torch.Tensor, c_dim: int, t_dim: int):
        """(tensor, (stride_b, stride_c, stride_t)) with H,W contiguous; copies only if needed."""
        if x.dtype != torch.float32:
            x = x.float()
        H, W = x.shape[-2:]
        if x.stride(-1) != 1 or x.stride(-2) != W:
            x = x.contiguous()
        return x, (x.stride(0), x.stride(c_dim), x.stride(t_dim))

    # ---- reference forward: vmae.py:539-560 ------------------------------------------------------
    @torch.no_grad()
    def forward(self, x, mask, timestamps=None, *args, n_vis: Optional[int] = None, check: bool = True, ragged: bool = False, n_vis_range=None, **kwargs):
        """x: float[B,C,T,H,W] (already pre-processed by the caller, any strides), mask: bool[B,Nt]
        with equal visible counts per row.  Returns float[B,Nm,C*P*P].

        ragged=True: the rows of `mask` may have different visible counts, between `lo` and `hi` = n_vis_range (without it one read-back of the
        counts' minimum and maximum).  Every row is predicted from exactly its own visible tokens, as it would be alone at batch 1.  Returns
        float[B, Nt - lo, C*P*P]: row b's predictions are its LAST Nt - Nv_b rows (ascending token order), the rows before them are zero."""
        if x.dim() != 5 or x.shape[1] != self.cfg.in_chans or x.shape[2] != self.cfg.num_frames:
            raise RuntimeError("expected x of shape [B,%d,%d,H,W], got %s" % (self.cfg.in_chans, self.cfg.num_frames, tuple(x.shape)))
        if tuple(x.shape[-2:]) != tuple(self.cfg.img_size):
            raise RuntimeError("input image size %s does not match the model's %s" % (tuple(x.shape[-2:]), self.cfg.img_size))
        x, strides = self._frame_strides(x, 1, 2)
        y, _ = self._run(x, strides, False, mask, n_vis, False, check=check, ragged=ragged, n_vis_range=n_vis_range)
        return y

    @torch.no_grad()
    def predict_video(self, x_btchw, mask, normalize: bool = True, n_vis: Optional[int] = None, check: bool = True,
                      out_tokens: Optional[torch.Tensor] = None, out_video: Optional[torch.Tensor] = None, weights_synced: bool = False,
                      ragged: bool = False, n_vis_range=None):
        """Fused wrapper path: raw [B,T,C,H,W] frames in [0,1] -> (tokens [B,Nm,C*P*P], video
        [B,T,C,H,W]) = `_preprocess` + forward + `pred_patches_to_video`
        (prediction.py:304-312, :419-422, :245-259) in one library call.  ragged / n_vis_range: as `forward` (tokens [B, Nt - lo, C*P*P])."""
        if x_btchw.dim() != 5 or x_btchw.shape[2] != self.cfg.in_chans or x_btchw.shape[1] != self.cfg.num_frames:
            raise RuntimeError("expected x of shape [B,%d,%d,H,W], got %s" % (self.cfg.num_frames, self.cfg.in_chans, tuple(x_btchw.shape)))
        x, strides = self._frame_strides(x_btchw, 2, 1)
        # (weights_synced: the caller has just run sync_weights() itself -- the wrapper does, BEFORE its mask read-back, so that the walk over the
        # parameters overlaps the previous call's kernels instead of delaying this call's first launch)
        return self._run(x, strides, normalize, mask, n_vis, True, xraw=x, check=check, out_tokens=out_tokens, out_video=out_video,
                         weights_synced=weights_synced, ragged=ragged, n_vis_range=n_vis_range)


# ---- factories (same names / defaults as vmae.py:597-619) -------------------------------------------
def base_16x16patch_2frames_1tube(**kwargs):
    return PretrainVisionTransformer(CONFIGS["base_16x16patch_2frames_1tube"], **kwargs)


def base_8x8patch_2frames_1tube(**kwargs):
    return PretrainVisionTransformer(CONFIGS["base_8x8patch_2frames_1tube"], **kwargs)


def large_4x4patch_2frames_1tube(**kwargs):
    return PretrainVisionTransformer(CONFIGS["large_4x4patch_2frames_1tube"], **kwargs)
