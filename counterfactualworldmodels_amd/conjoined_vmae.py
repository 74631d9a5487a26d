"""Host-side mirror of the IMU-conditioned conjoined padded predictor, backed by libcwm_hip.so.

`ConjoinedPaddedVisionTransformer` / `imu400_base_4x4patch_2frames_1tube` keep the reference's surface
(`cwm/models/VideoMAE/conjoined_vmae.py:889-1011, 1230-1243`): the 634 state-dict keys and shapes of
the published checkpoint, `forward(x, mask, timestamps=None, x_context=None,
mask_context=None, output_main=None, output_context=None)` returning the main-stream tokens
`[B, Nt + 64 - max_visible, 48]` with rows at masked pad slots zeroed, and the attributes the wrapper
reads (`main_stream`, `context_stream`, `max_padding_tokens`, `min_padding_tokens`, `padding_mask`,
`_reset_padding_mask`, `get_current_inputs`, `patch_size`, `image_size`, `num_frames`, `mask_size`).
The parameter tree holds no compute: the forward pass is one `cwm_conj_forward` call.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
import torch.nn as nn

from . import _lib
from ._handle import LibraryModule, _NoForward
from .config import CONJ_CONFIGS, IMAGENET_MEAN, IMAGENET_STD, LN_EPS, ConjConfig, conj_state_dict_schema


def _init_param(name: str, p: torch.Tensor) -> None:
    if "norm" in name and name.endswith("weight"):
        nn.init.ones_(p)
    elif name.endswith("bias"):
        nn.init.zeros_(p)
    elif "token" in name:
        nn.init.trunc_normal_(p, std=0.02, a=-0.02, b=0.02)
    elif p.dim() >= 2:
        nn.init.xavier_uniform_(p.view(p.shape[0], -1))
    else:
        nn.init.zeros_(p)


def _build_tree(root: nn.Module, schema) -> None:
    for key, shape in schema.items():
        node = root
        parts = key.split(".")
        for part in parts[:-1]:
            if part not in node._modules:
                node.add_module(part, _NoForward())
            node = node._modules[part]
        p = nn.Parameter(torch.empty(shape))
        _init_param(key, p.data)
        node.register_parameter(parts[-1], p)


class ConjoinedPaddedVisionTransformer(LibraryModule):
    def __init__(self, cfg: ConjConfig, mode: str = "parity", **unused):
        super().__init__()
        self.cfg = cfg
        self.mode = mode
        _lib.mode_id(mode)
        _build_tree(self, conj_state_dict_schema(cfg))
        m = cfg.main
        ms, cs = self.main_stream, self.context_stream
        ms.max_padding_tokens, ms.min_padding_tokens = cfg.main_max_pad, 0
        cs.max_padding_tokens, cs.min_padding_tokens = cfg.ctx_max_pad, 0
        ms.patch_size = (1, m.patch, m.patch)
        ms.image_size = tuple(m.img_size)
        ms.num_frames = m.num_frames
        ms.num_patches = m.num_tokens
        ms.padding_mask = ms.full_input_mask = ms.null_mask = None
        ms._reset_padding_mask = lambda: self._reset_stream(ms)
        cs.patch_size = (cfg.ctx_tubelet, 1, 1)
        cs.image_size = (1, 1)
        cs.num_frames = 0
        cs.padding_mask = cs.full_input_mask = cs.null_mask = None
        cs._reset_padding_mask = lambda: self._reset_stream(cs)
        cs.encoder.num_tokens = cfg.ctx_tokens
        cs.encoder.sequence_length = cfg.ctx_seq_len
        self.num_frames = m.num_frames
        self.get_context_input = type("IMU", (), {"num_channels": cfg.ctx_in_chans, "num_frames": None})()
        self.get_main_input = type("RGB01", (), {"num_channels": m.in_chans, "num_frames": m.num_frames})()
        self._output_main, self._output_context = True, False
        self.default_cfg = {}

    # ---- reference attribute surface ---------------------------------------------------------------
    @staticmethod
    def _reset_stream(s):
        s.padding_mask = s.full_input_mask = s.null_mask = None

    def _reset_padding_mask(self):
        self._reset_stream(self.main_stream)
        self._reset_stream(self.context_stream)

    @property
    def patch_size(self):
        return self.main_stream.patch_size

    @property
    def image_size(self):
        return self.main_stream.image_size

    @image_size.setter
    def image_size(self, v):
        self.main_stream.image_size = tuple(v)

    @property
    def padding_mask(self):
        # the reference's __getattr__ falls through to the main stream and raises while it is None
        # (conjoined_vmae.py:347-354), so hasattr(model, 'padding_mask') is False before a forward
        if self.main_stream.padding_mask is None:
            raise AttributeError("no attr padding_mask in the module or the main transformer stream")
        return self.main_stream.padding_mask

    @property
    def max_padding_tokens(self):
        return self.main_stream.max_padding_tokens

    @property
    def min_padding_tokens(self):
        return self.main_stream.min_padding_tokens

    @property
    def mask_size(self):  # conjoined_vmae.py:356-360
        ps = self.main_stream.patch_size
        return (self.num_frames // ps[0], self.main_stream.image_size[-2] // ps[-2], self.main_stream.image_size[-1] // ps[-1])

    def get_current_inputs(self, x, mask, *args, **kwargs):
        """conjoined_vmae.py:722-732 with output_main only: the main stream sees (x, mask) unchanged ('rgb01')."""
        return ((x, mask, None),)

    # ---- C-ABI plumbing (the handle, sync_weights and the options live in _handle.LibraryModule) -------
    _ABI = {role: "cwm_conj_" + role for role in ("destroy", "load_weight", "forward", "set_option", "set_lanes", "timing_enable", "timing_collect")}

    def _conj_config(self):
        c, m = self.cfg, self.cfg.main
        cc = _lib.CwmConjConfig()
        cc.main = _lib.CwmConfig(m.img_size[0], m.img_size[1], m.patch, m.num_frames, m.in_chans, m.enc_dim, m.enc_depth, m.enc_heads,
                                 m.dec_dim, m.dec_depth, m.dec_heads, m.mlp_ratio, LN_EPS)
        cc.main_max_pad = c.main_max_pad
        cc.ctx_in_chans, cc.ctx_seq_len, cc.ctx_tubelet = c.ctx_in_chans, c.ctx_seq_len, c.ctx_tubelet
        cc.ctx_enc_dim, cc.ctx_dec_dim, cc.ctx_enc_heads, cc.ctx_dec_heads = c.ctx_enc_dim, c.ctx_dec_dim, c.ctx_enc_heads, c.ctx_dec_heads
        cc.ctx_max_pad = c.ctx_max_pad
        cc.n_enc_cross, cc.n_dec_cross = len(c.enc_cross), len(c.dec_cross)
        for i, v in enumerate(c.enc_cross):
            cc.enc_cross[i] = v
        for i, v in enumerate(c.dec_cross):
            cc.dec_cross[i] = v
        cc.cross_heads, cc.cross_mlp_ratio = c.cross_heads, c.cross_mlp_ratio
        return cc

    def _create(self, lib, h):
        return lib.cwm_conj_create(C.byref(self._conj_config()), C.byref(h))

    # ---- reference forward: conjoined_vmae.py:852-887 ----------------------------------------------
    @torch.no_grad()
    def forward(self, x, mask, timestamps=None, x_context=None, mask_context=None, output_main=None, output_context=None,
                *args, normalize: bool = False, check: bool = True, n_vis: Optional[int] = None, n_vis_context: Optional[int] = None,
                **kwargs):
        """`n_vis` / `n_vis_context`: the caller knows that every row of `mask` / `mask_context` has exactly this many visible
        tokens (a rectangularised batch; `mask_context=None` means all visible): skips the host read-back of the row counts."""
        _lib.require_gpu()
        # `_set_decoder_outputs` (conjoined_vmae.py:589-593): a flag that is given replaces the model's setting and STAYS replaced
        if output_main is not None:
            self._output_main = bool(output_main)
        if output_context is not None:
            self._output_context = bool(output_context)
        want_main, want_ctx = self._output_main, self._output_context
        if not want_main and not want_ctx:  # "return all the tokens from both streams" (:1010-1011): the same tuple in the padded model
            want_main = want_ctx = True
        if x_context is None:
            raise RuntimeError("the IMU-conditioned predictor needs x_context [B,%d,%d]" % (self.cfg.ctx_in_chans, self.cfg.ctx_seq_len))
        if not x.is_cuda:
            raise RuntimeError("ConjoinedPaddedVisionTransformer.forward needs CUDA/HIP tensors (no CPU fallback); got %s" % x.device)
        c, m = self.cfg, self.cfg.main
        if x.dim() != 5 or x.shape[1] != m.in_chans or x.shape[2] != m.num_frames or tuple(x.shape[-2:]) != tuple(m.img_size):
            raise RuntimeError("expected x of shape [B,%d,%d,%d,%d], got %s" % (m.in_chans, m.num_frames, m.img_size[0], m.img_size[1], tuple(x.shape)))
        dev, B, Nt = x.device, x.shape[0], m.num_tokens
        self.sync_weights(dev)
        if x.dtype != torch.float32:
            x = x.float()
        if x.stride(-1) != 1 or x.stride(-2) != x.shape[-1]:
            x = x.contiguous()
        mask = mask.to(device=dev, dtype=torch.bool).reshape(B, -1).contiguous()
        if mask.shape[1] != Nt:
            raise RuntimeError("mask has %d tokens per row, model expects %d" % (mask.shape[1], Nt))
        ctx = x_context.to(device=dev, dtype=torch.float32).reshape(B, c.ctx_in_chans, c.ctx_seq_len).contiguous()
        mask_context_given = mask_context is not None
        if mask_context is None:
            mask_context = torch.zeros(B, c.ctx_tokens, dtype=torch.bool, device=dev)
        mc = mask_context.to(device=dev, dtype=torch.bool).reshape(B, c.ctx_tokens).contiguous()
        vis = (~mask).sum(-1)
        vis_c = (~mc).sum(-1)
        if not mask_context_given:
            n_vis_context = c.ctx_tokens
        if n_vis is not None and n_vis_context is not None:
            vmax = vmin = int(n_vis)
            vcmax = vcmin = int(n_vis_context)
        else:
            vmax, vmin, vcmax, vcmin = (int(v) for v in torch.stack([vis.max(), vis.min(), vis_c.max(), vis_c.min()]).tolist())
        if vmax - vmin > c.main_max_pad or vcmax - vcmin > c.ctx_max_pad:
            raise RuntimeError("visible-token counts differ by more than max_padding_tokens (%d / %d)" % (c.main_max_pad, c.ctx_max_pad))
        if vmax < 1 or vcmax < 1:
            raise RuntimeError("every stream needs at least one visible token")
        n_out = Nt + c.main_max_pad - vmax
        y = torch.empty((B, n_out, m.out_dim), device=dev, dtype=torch.float32)
        # the context stream's predictions: head(norm(x_c[:, -n:])) * ~null_mask over its masked + pad slots (conjoined_vmae.py:990-1002)
        y_ctx = torch.empty((B, c.ctx_tokens + c.ctx_max_pad - vcmax, c.ctx_out_dim), device=dev, dtype=torch.float32) if want_ctx else None
        args_ = _lib.CwmConjForwardArgs(
            C.sizeof(_lib.CwmConjForwardArgs),
            x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), int(normalize), mask.data_ptr(), B, vmax, ctx.data_ptr(), mc.data_ptr(),
            vcmax, y.data_ptr(), _lib.mode_id(self.mode), int(check), _lib.current_stream_handle(dev), _lib.ptr(y_ctx))
        with torch.cuda.device(dev):
            self._check(self._fn["forward"](self._handle, C.byref(args_)))
        self._record_padding_state(mask, vis, vmax, mc, vis_c, vcmax)
        if want_main and want_ctx:
            return y, y_ctx
        return y if want_main else y_ctx

    def _record_padding_state(self, mask, vis, vmax, mask_ctx=None, vis_ctx=None, vmax_ctx=None):
        """The padding attributes the reference leaves set on BOTH streams after a forward until the wrapper resets them
        (prediction.py:451-452; conjoined_vmae.py:49-116): `padding_mask` (pad slot j of row b is masked unless
        j < max visible - visible(b)), `full_input_mask` = [mask | padding_mask], `null_mask` = [zeros(min masked) | padding_mask]."""
        def record(stream, m, v, vm, max_pad):
            B, N = m.shape
            pad = torch.arange(max_pad, device=m.device)[None] >= (vm - v)[:, None]
            stream.padding_mask = pad
            stream.full_input_mask = torch.cat([m, pad], -1)
            stream.null_mask = torch.cat([torch.zeros(B, N - vm, dtype=torch.bool, device=m.device), pad], -1)

        record(self.main_stream, mask, vis, vmax, self.cfg.main_max_pad)
        if mask_ctx is not None:
            record(self.context_stream, mask_ctx, vis_ctx, vmax_ctx, self.cfg.ctx_max_pad)


def imu400_base_4x4patch_2frames_1tube(**kwargs):
    """conjoined_vmae.py:1230-1243"""
    return ConjoinedPaddedVisionTransformer(CONJ_CONFIGS["imu400_base_4x4patch_2frames_1tube"], **kwargs)


class ConjoinedPretrainVisionTransformer(ConjoinedPaddedVisionTransformer):
    """The unpadded conjoined model of the flow -> IMU head-motion predictor (`ConjoinedPretrainVisionTransformer`,
    conjoined_vmae.py:212-887; factory `imu400_8x8patch_2frames_1tube_flowbackrgb01` :1218-1228).

    Same surface as the reference: the 583 state-dict keys, `forward(x, mask, timestamps=None, x_context=None, mask_context=None,
    output_main=None, output_context=None)` on the imagenet-normalised frames [B,3,2,H,W] and a mask over both frames
    (`mask_size` (2, 28, 28); the main stream reads its frame-1 half).  The main stream's 7 input channels (`FlowBackRGB01`,
    preprocessor.py:208-277) come from `flow_model` -- any module with RAFT's multi-frame call signature, run in PyTorch on the
    un-normalised frames -- and frame 1; scaling, normalisation and the patch gather happen in-kernel.  Every row must have the same
    visible count in each stream (the reference reshapes `x[~mask]`).  The context stream appends its learned dummy token (always
    visible), so an entirely masked IMU leaves the context encoder one token.  `output_context=True` returns the context stream's
    predictions [B, 25 - visible IMU tokens, 96]."""

    def __init__(self, cfg: ConjConfig, mode: str = "parity", flow_model=None, raft_iters: int = 24, **unused):
        assert not cfg.padded and cfg.ctx_dummy_token and cfg.main_input == "flowback_rgb01", cfg
        super().__init__(cfg, mode=mode)
        self.num_frames = 2  # mask_size covers both input frames (conjoined_vmae.py:356-360)
        self.get_main_input = type("FlowBackRGB01", (), {"num_channels": cfg.main.in_chans, "num_frames": 1, "frames_list": [0, 1]})()
        # a plain attribute, not a submodule: the flow model's parameters are not part of this model's state dict
        object.__setattr__(self, "flow_model", flow_model)
        self.raft_iters = raft_iters
        for stream in (self.main_stream, self.context_stream):  # the unpadded streams have no padding state (hasattr is False)
            for k in ("padding_mask", "full_input_mask", "null_mask", "_reset_padding_mask", "max_padding_tokens", "min_padding_tokens"):
                stream.__dict__.pop(k, None)

    def _reset_padding_mask(self):
        pass

    @property
    def max_padding_tokens(self):
        return 0

    @property
    def min_padding_tokens(self):
        return 0

    def set_flow_model(self, flow_model):
        object.__setattr__(self, "flow_model", flow_model)

    def _create(self, lib, h):
        v = _lib.CwmConjVariant(C.sizeof(_lib.CwmConjVariant), 0, 1, _lib.CONJ_INPUT_FLOWBACK_RGB01)
        return lib.cwm_conj_create_ex(C.byref(self._conj_config()), C.byref(v), C.byref(h))

    @property
    def padding_mask(self):
        raise AttributeError("the unpadded conjoined model has no padding_mask")

    def get_current_inputs(self, x, mask, *args, **kwargs):  # pragma: no cover - the reference's training helper
        raise NotImplementedError("get_current_inputs is not provided for the flow -> IMU model")

    def _require_flow_model(self):
        if self.flow_model is None:
            raise RuntimeError("this flow -> IMU model has no flow_model: pass flow_model= (RAFT, or any module called as "
                               "flow_model(x[B,2,3,H,W] in [0,1], iters=..., backward=...) -> [B,1,2,H,W]) to the factory, or set_flow_model()")

    def compute_flows(self, x, normalized: bool = True):
        """(forward, backward) flow of frames 0 -> 1, each [B,2,H,W] in pixels, from the frames x [B,3,2,H,W]: imagenet-normalised
        (`FramePairFlow.get_flow` on `imagenet_unnormalize(x)`, preprocessor.py:226-277) or, with normalized=False, in [0,1]."""
        self._require_flow_model()
        x01 = x[:, :, :2]
        if normalized:
            mean = torch.tensor(IMAGENET_MEAN, device=x.device, dtype=x.dtype).view(1, 3, 1, 1, 1)
            std = torch.tensor(IMAGENET_STD, device=x.device, dtype=x.dtype).view(1, 3, 1, 1, 1)
            x01 = x01 * std + mean
        x01 = x01.transpose(1, 2)
        fwd = self.flow_model(x01, iters=self.raft_iters, backward=False)
        bwd = self.flow_model(x01, iters=self.raft_iters, backward=True)
        return fwd[:, 0], bwd[:, 0]

    @staticmethod
    def _flow_operand(f, B, H, W):
        f = f.to(dtype=torch.float32)
        if tuple(f.shape) != (B, 2, H, W):
            raise RuntimeError("expected a flow of shape [B,2,H,W] = %s, got %s" % ((B, 2, H, W), tuple(f.shape)))
        if f.stride(-1) != 1 or f.stride(-2) != W or f.stride(0) % 4 or f.stride(1) % 4 or f.data_ptr() % 16:
            f = f.contiguous()
        return f

    @torch.no_grad()
    def forward(self, x, mask, timestamps=None, x_context=None, mask_context=None, output_main=None, output_context=None,
                *args, flows=None, normalize: bool = False, check: bool = True, **kwargs):
        """`flows`: (forward, backward) [B,2,H,W] pixel flows instead of calling flow_model (any strides with contiguous rows).
        `normalize=True`: x holds the frames in [0,1] (the flow model's input as it is) and frame 1 is imagenet-normalised in-kernel,
        as the padded model's `normalize`; by default x is imagenet-normalised, as the reference's forward takes it."""
        if timestamps is not None:
            raise NotImplementedError("timestamps are not supported (the IMU-conditioned path ignores them as well)")
        if flows is None:
            self._require_flow_model()
        _lib.require_gpu()
        if output_main is not None:
            self._output_main = bool(output_main)
        if output_context is not None:
            self._output_context = bool(output_context)
        want_main, want_ctx = self._output_main, self._output_context
        if not want_main and not want_ctx:
            want_main = want_ctx = True
        c, m = self.cfg, self.cfg.main
        H, W = m.img_size
        if x_context is None:
            raise RuntimeError("the flow -> IMU model needs x_context [B,%d,%d] (an all-masked zero IMU to predict it from the video)"
                               % (c.ctx_in_chans, c.ctx_seq_len))
        if not x.is_cuda:
            raise RuntimeError("ConjoinedPretrainVisionTransformer.forward needs CUDA/HIP tensors (no CPU fallback); got %s" % x.device)
        if x.dim() != 5 or x.shape[1] != 3 or x.shape[2] < 2 or tuple(x.shape[-2:]) != (H, W):
            raise RuntimeError("expected x of shape [B,3,2,%d,%d], got %s" % (H, W, tuple(x.shape)))
        dev, B, Nt = x.device, x.shape[0], m.num_tokens
        if flows is None:
            flows = self.compute_flows(x, normalized=not normalize)
        fwd, bwd = (self._flow_operand(f.to(dev), B, H, W) for f in flows)
        self.sync_weights(dev)
        if x.dtype != torch.float32:
            x = x.float()
        if x.stride(-1) != 1 or x.stride(-2) != W or x.stride(0) % 4 or x.stride(1) % 4 or x.data_ptr() % 16:
            x = x.contiguous()
        frame1 = x[:, :, 1]
        mask = mask.to(device=dev, dtype=torch.bool).reshape(B, -1)
        if mask.shape[1] != 2 * Nt:
            raise RuntimeError("mask has %d tokens per row, model expects %d (both frames)" % (mask.shape[1], 2 * Nt))
        mask_m = mask[:, Nt:].contiguous()  # the main stream reads the frame-1 half (get_stream_inputs :430-486)
        ctx = x_context.to(device=dev, dtype=torch.float32).reshape(B, c.ctx_in_chans, c.ctx_seq_len).contiguous()
        if mask_context is None:
            mask_context = torch.zeros(B, c.ctx_tokens, dtype=torch.bool, device=dev)
        mc = mask_context.to(device=dev, dtype=torch.bool).reshape(B, c.ctx_tokens).contiguous()
        # the largest visible counts; the library rejects rows that differ (CWM_ERR_INVALID)
        vm, vc = (int(v) for v in torch.stack([(~mask_m).sum(-1).max(), (~mc).sum(-1).max()]).tolist())
        vc += 1  # the dummy token
        n_out, n_out_c = Nt - vm, c.ctx_tokens + 1 - vc
        y = torch.empty((B, n_out, m.out_dim), device=dev, dtype=torch.float32) if want_main else None
        y_ctx = torch.empty((B, n_out_c, c.ctx_out_dim), device=dev, dtype=torch.float32) if want_ctx else None
        args_ = _lib.CwmConjForwardArgs()
        args_.struct_size = C.sizeof(_lib.CwmConjForwardArgs)
        args_.x_dev, args_.x_stride_b, args_.x_stride_c, args_.normalize = frame1.data_ptr(), frame1.stride(0), frame1.stride(1), int(normalize)
        args_.mask_dev, args_.batch, args_.n_vis_max = mask_m.data_ptr(), B, vm
        args_.ctx_dev, args_.ctx_mask_dev, args_.n_vis_ctx_max = ctx.data_ptr(), mc.data_ptr(), vc
        args_.y_tokens_dev = y.data_ptr() if (y is not None and n_out > 0) else None
        args_.y_ctx_tokens_dev = _lib.ptr(y_ctx)
        args_.mode, args_.check, args_.stream = _lib.mode_id(self.mode), int(check), _lib.current_stream_handle(dev)
        args_.flow_fwd_dev, args_.flow_fwd_stride_b, args_.flow_fwd_stride_c = fwd.data_ptr(), fwd.stride(0), fwd.stride(1)
        args_.flow_bwd_dev, args_.flow_bwd_stride_b, args_.flow_bwd_stride_c = bwd.data_ptr(), bwd.stride(0), bwd.stride(1)
        if args_.y_tokens_dev is None and args_.y_ctx_tokens_dev is None:
            return y  # nothing to compute: every main token visible and no context output asked for
        with torch.cuda.device(dev):
            self._check(self._fn["forward"](self._handle, C.byref(args_)))
        if want_main and want_ctx:
            return y, y_ctx
        return y if want_main else y_ctx


def imu400_8x8patch_2frames_1tube_flowbackrgb01(flow_model=None, **kwargs):
    """conjoined_vmae.py:1218-1228: the flow -> IMU head-motion predictor.  `flow_model` (RAFT in the reference) may be set later."""
    return ConjoinedPretrainVisionTransformer(CONJ_CONFIGS["imu400_8x8patch_2frames_1tube_flowbackrgb01"], flow_model=flow_model, **kwargs)
