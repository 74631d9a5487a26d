"""RAFT-large optical flow on the GPU: drop-in for `cwm.models.raft.raft_model.load_raft_model` / `RAFT` (raft_model.py:55-300).

The module keeps the reference's parameter tree (179 state-dict tensors: `fnet`, `cnet`, `update_block`), so checkpoints load unchanged,
and runs its forward pass in libcwm_hip.so (`cwm_raft_forward`; `cwm_raft_forward_ex` for a warm start or the per-iteration list): HIP kernels and GEMMs in parity (split-bf16) arithmetic by default or,
with `mixed_precision=True` / `set_mode("fast")`, with bf16 operands; no PyTorch operator and no CPU fallback.  The configuration is the reference's inference one:
BasicEncoder fnet (instance norm) and cnet (eval batch norm), 4 correlation levels of radius 4, BasicUpdateBlock with SepConvGRU, convex
upsampling.

    from counterfactualworldmodels_amd.raft import load_raft_model
    flow_model = load_raft_model("raft-large.pth").cuda().eval()
    flows = flow_model(x, iters=24)              # x [B,T,3,H,W] in [0,1] -> [B,T-1,2,H,W] pixels
    flows_back = flow_model(x, backward=True)    # pairs (x[t+1], x[t]), in reversed order
    flows_warm = flow_model(x, flow_init=f8)     # f8 [B or 1,2,H/8,W/8]: RAFT's warm start, e.g. the previous pair's low-resolution flow
    flows_video = flow_model(x, warm_start=True) # each pair started from forward_interpolate(low-resolution flow of the pair before), on the device

With `output_dim=1` the model owns the reference's `output_block` (raft_model.py:152-159; 183 state-dict tensors) and returns its convex-upsampled
value in place of the flow: the keypoint predictor of the demo notebook,

    keypoint_predictor = load_raft_model(None, output_dim=1)   # then load_state_dict(checkpoint['model'])
    keypoints = keypoint_predictor.cuda()(x)                   # [B,T-1,1,H,W]

The reference's `--mixed_precision` is the fast mode: `load_raft_model(path, mixed_precision=True)`, or `model.set_mode("fast")` at any time.

For large frames and long movies, `load_raft_model(path, corr="on_the_fly")` or `model.set_corr("on_the_fly")` computes the correlations a lookup needs
when it needs them (the reference's `AlternateCorrBlock`, raft/corr.py:63-91) instead of building the all-pairs volume, which grows with the square of
the frame area; `model.workspace_bytes()` tells what a forward holds.  Frames whose sides are no multiple of 8 go through `InputPadder`:

    padder = InputPadder(x.shape)                # raft/utils.py:9-26
    flows = padder.unpad(flow_model(*padder.pad(x)))

`load_raft_model(path, share_frames=True)` or `model.set_share_frames(True)` runs the two encoders once per distinct frame of a call instead of once
per pair: the interior frames of a movie, a single repeated frame, and the first frame that S counterfactual samples share,

    flows = flow_model.flow_pairs(x0.expand(B, S, 3, H, W), predicted)   # [B,S,2,H,W]; fnet on B * (S + 1) images, cnet on B
    flow_model.last_encoder_images                                       # (fnet images, cnet images) of the last forward
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._handle import LibraryModule, _NoForward
from .config import RAFT_CORR_LEVELS, RAFT_CORR_RADIUS, RAFT_HIDDEN

default_raft_ckpt = "../../../checkpoints/raft_checkpoints/raft-large.pth"


class ResidualBlock(_NoForward):
    def __init__(self, in_planes: int, planes: int, norm_fn: str, stride: int = 1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        norm = nn.BatchNorm2d if norm_fn == "batch" else nn.InstanceNorm2d
        self.norm1 = norm(planes)
        self.norm2 = norm(planes)
        if stride != 1:
            self.norm3 = norm(planes)
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, kernel_size=1, stride=stride), self.norm3)
        else:
            self.downsample = None


class BasicEncoder(_NoForward):
    def __init__(self, output_dim: int, norm_fn: str):
        super().__init__()
        self.norm_fn = norm_fn
        self.norm1 = nn.BatchNorm2d(64) if norm_fn == "batch" else nn.InstanceNorm2d(64)
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3)
        self.relu1 = nn.ReLU(inplace=True)
        self.in_planes = 64
        self.layer1 = self._make_layer(64, 1)
        self.layer2 = self._make_layer(96, 2)
        self.layer3 = self._make_layer(128, 2)
        self.conv2 = nn.Conv2d(128, output_dim, kernel_size=1)
        self.dropout = None

    def _make_layer(self, dim: int, stride: int) -> nn.Sequential:
        layers = (ResidualBlock(self.in_planes, dim, self.norm_fn, stride), ResidualBlock(dim, dim, self.norm_fn, 1))
        self.in_planes = dim
        return nn.Sequential(*layers)


class BasicMotionEncoder(_NoForward):
    def __init__(self):
        super().__init__()
        cor_planes = RAFT_CORR_LEVELS * (2 * RAFT_CORR_RADIUS + 1) ** 2
        self.convc1 = nn.Conv2d(cor_planes, 256, 1, padding=0)
        self.convc2 = nn.Conv2d(256, 192, 3, padding=1)
        self.convf1 = nn.Conv2d(2, 128, 7, padding=3)
        self.convf2 = nn.Conv2d(128, 64, 3, padding=1)
        self.conv = nn.Conv2d(64 + 192, 128 - 2, 3, padding=1)


class SepConvGRU(_NoForward):
    def __init__(self, hidden_dim: int = 128, input_dim: int = 192 + 128):
        super().__init__()
        for i, (k, p) in enumerate((((1, 5), (0, 2)), ((5, 1), (2, 0))), 1):
            for g in "zrq":
                setattr(self, "conv%s%d" % (g, i), nn.Conv2d(hidden_dim + input_dim, hidden_dim, k, padding=p))


class FlowHead(_NoForward):
    def __init__(self, input_dim: int = 128, hidden_dim: int = 256):
        super().__init__()
        self.conv1 = nn.Conv2d(input_dim, hidden_dim, 3, padding=1)
        self.conv2 = nn.Conv2d(hidden_dim, 2, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)


class BasicUpdateBlock(_NoForward):
    def __init__(self, hidden_dim: int = 128):
        super().__init__()
        self.encoder = BasicMotionEncoder()
        self.gru = SepConvGRU(hidden_dim=hidden_dim, input_dim=128 + hidden_dim)
        self.flow_head = FlowHead(hidden_dim, hidden_dim=256)
        self.mask = nn.Sequential(nn.Conv2d(128, 256, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(256, 64 * 9, 1, padding=0))


def _args(**kw) -> argparse.Namespace:
    a = argparse.Namespace(corr_levels=RAFT_CORR_LEVELS, corr_radius=RAFT_CORR_RADIUS, output_dim=None, iters=None, dropout=0.0, mixed_precision=False,
                           small=False, gpus=[0], multiframe=True, scale_inputs=True, alternate_corr=False, corr="all_pairs", share_frames=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _forward_interpolate_into(src: torch.Tensor, dst: torch.Tensor) -> None:
    """`cwm_raft_forward_interpolate` of src [P,2,h,w] (fp32, rows contiguous, any field and channel strides) into dst [P,2,h,w] (fp32, contiguous), on the
    current stream of src's device; nothing is synchronised."""
    P, _, h, w = src.shape
    with torch.cuda.device(src.device):
        _lib.check(_lib.get_lib().cwm_raft_forward_interpolate(src.data_ptr(), src.stride(0), src.stride(1), P, h, w, dst.data_ptr(),
                                                               _lib.current_stream_handle(src.device)))


class InputPadder:
    """raft/utils.py:9-26: pads frames so that both sides are multiples of 8, which the forward requires (436 x 1024 -> 440 x 1024), and crops a result
    back.  `dims` is a shape ending in (H, W); mode "sintel" splits both paddings between the two borders, any other mode ("kitti") puts the vertical one
    below.  `pad` replicates the border pixels of tensors with any number of leading dimensions ([B,3,H,W] or the multi-frame [B,T,3,H,W]) and returns
    a list; `unpad` is a view of the last two dimensions."""

    def __init__(self, dims, mode="sintel"):
        h, w = int(dims[-2]), int(dims[-1])
        add_h, add_w = -h % 8, -w % 8  # what each side lacks to the next multiple of 8
        left = add_w // 2
        top = add_h // 2 if mode == "sintel" else 0
        self.ht, self.wd = h, w
        self._pad = [left, add_w - left, top, add_h - top]  # F.pad's order: left, right, top, bottom

    def pad(self, *inputs):
        out = []
        for x in inputs:  # F.pad's replicate mode takes 3 or 4 dimensions: fold the leading ones into one
            y = F.pad(x.reshape(1, -1, x.shape[-2], x.shape[-1]), self._pad, mode="replicate")
            out.append(y.reshape(*x.shape[:-2], y.shape[-2], y.shape[-1]))
        return out

    def unpad(self, x):
        left, right, top, bottom = self._pad
        return x[..., top:x.shape[-2] - bottom, left:x.shape[-1] - right]


@torch.no_grad()
def forward_interpolate(flow: torch.Tensor) -> torch.Tensor:
    """raft/utils.py:28-56 on the device: the flow [2,h,w] (or P of them, [P,2,h,w]; channel 0 = x) carried along itself.  Pixel (x0, y0) lands at
    (x0 + dx, y0 + dy); every grid point takes the flow of the source that lands nearest to it, among those landing strictly inside (0, w) x (0, h).
    This is what RAFT's warm start feeds to the next pair as `flow_init`.  Any float dtype; a strided view is read in place when its rows are
    contiguous.  Returns fp32 of the same shape on the same device, on the current stream, without a host synchronisation.
    Not the reference's: equal distances go to the lowest source index (scipy's KD-tree order is its own), and a field with no valid source gives
    zeros, a cold start (scipy returns NaN or raises)."""
    if not torch.is_tensor(flow) or not flow.is_floating_point():
        raise RuntimeError("forward_interpolate needs a floating-point tensor [2,h,w] or [P,2,h,w], got %r"
                           % (type(flow).__name__ if not torch.is_tensor(flow) else flow.dtype,))
    if not flow.is_cuda:
        raise RuntimeError("forward_interpolate needs a CUDA/HIP tensor (no CPU fallback); got %s" % flow.device)
    if flow.dim() not in (3, 4) or flow.shape[-3] != 2 or flow.numel() == 0:
        raise RuntimeError("forward_interpolate expects a flow [2,h,w] or [P,2,h,w], got %s" % (tuple(flow.shape),))
    f = flow.detach().float()
    f = f.unsqueeze(0) if f.dim() == 3 else f
    if f.stride(-1) != 1 or f.stride(-2) != f.shape[-1]:
        f = f.contiguous()
    out = torch.empty(f.shape, dtype=torch.float32, device=f.device)
    _forward_interpolate_into(f, out)
    return out if flow.dim() == 4 else out[0]


class RAFT(LibraryModule):
    """Drop-in for the reference's `RAFT` (large, inference).  Calls:
    - multiframe (default): `model(x[B,T,3,H,W], iters=24, backward=False)` -> [B,T-1,2,H,W] pixel flows (flow_up of the last iteration);
      x is in [0,1] with scale_inputs=True (in [0,255] otherwise); backward=True computes the pairs (x[t+1], x[t]) and returns them in
      reversed order, as the reference's `flows.insert(0, ...)`.
    - multiframe=False: `model(image1, image2, iters=24, flow_init=None, upsample=True, test_mode=True)` on [B,3,H,W] images in [0,255] ->
      (coords1 - coords0 [B,2,H/8,W/8], flow_up [B,2,H,W]); with `test_mode=False` the list of every iteration's flow_up (`iters` tensors [B,2,H,W],
      views of one buffer; the last equals the flow_up above).  `upsample` is ignored, as in the reference.
    - `flow_init` (both calls; raft_model.py:241-242): RAFT's warm start, a flow [B,2,H/8,W/8] or [1,2,H/8,W/8] in 1/8-resolution pixels (channel 0 = x)
      added to the initial coordinates; any float dtype (cast to fp32), on the frames' device.  The multi-frame call gives the same field to every
      pair, also with backward=True, and accepts `test_mode` (its result is the last iteration's flow_up either way, raft_model.py:297).
    - `warm_start=True` (multi-frame call): the pairs run as a chain, each started from `forward_interpolate` (this module; raft/utils.py:28-56) of the
      low-resolution flow of the pair before it; `flow_init` then starts the first pair of the chain only (`_forward_multiframe`).
    Without `flow_init` and with test_mode=True a call is `cwm_raft_forward`: the mask head and the upsampling run once.  Otherwise it is
    `cwm_raft_forward_ex`; only test_mode=False makes them run in every iteration.
    `self.iters`, when set, overrides the call's `iters`.  H and W must be multiples of 8 with H/8, W/8 >= 16.
    With `args.output_dim == 1` the 2-channel flow_up above is the 1-channel upsampled `output_block(net)` (raft_model.py:257-267): [B,T-1,1,H,W],
    and (coords1 - coords0, up [B,1,H,W]) from the two-image call.
    Arithmetic: `self.mode` is "parity" (split-bf16 convolutions, the default) or "fast" (every convolution with bf16 operands and fp32 accumulation;
    norm statistics, correlation, lookup, coordinates, GRU update and upsampling stay fp32: the reference's autocast split, raft_model.py:218-252).
    It is "fast" when `args.mixed_precision` is true and changes with `set_mode`; nothing else chooses it.  In particular fp16 / bf16 frames do NOT turn
    the fast mode on (the reference's autocast does, raft_model.py:219): they are upcast to fp32 and run in the model's mode.
    Correlation: `self.corr` is "all_pairs" (the default: the volume of `CorrBlock`, built once per forward) or "on_the_fly" (the taps of every lookup
    computed from the two feature maps, `AlternateCorrBlock` of raft/corr.py:63-91: no volume, so the workspace grows with the frame area and not with
    its square).  It comes from `args.corr` and changes with `set_corr`; both give the same flow up to fp32 summation order, in either mode.
    Shared frames: with `self.share_frames` (False by default; `args.share_frames`, `set_share_frames`) a forward runs fnet once per distinct frame and
    cnet once per distinct first image of the call.  What repeats is read off the strides of the two image views the call hands to the library: a view
    expanded over the pairs or over the batch (stride 0), a movie's `x[:, :-1]` / `x[:, 1:]` (T frames per row through fnet in place of 2 (T - 1)), a
    single repeated frame.  The multi-frame call needs nothing more than the flag; `flow_pairs` takes the two views directly.  The result agrees with
    the unshared one as one pair does between batches of different sizes (fp32 summation order), not bit for bit.  `warm_start=True` runs pair by pair
    and shares nothing between its calls.  `last_encoder_images` tells what the last forward ran."""

    def __init__(self, args: Optional[argparse.Namespace] = None):
        super().__init__()
        self.args = args if args is not None else _args()
        if getattr(self.args, "small", False):
            raise NotImplementedError("RAFT-small (SmallEncoder / SmallUpdateBlock) is not provided: only RAFT-large runs on the GPU")
        self.output_dim = getattr(self.args, "output_dim", None)
        if self.output_dim is not None and self.output_dim != 1:
            raise NotImplementedError("the output_dim head of RAFT is provided for output_dim = 1 only (the keypoint predictor), got %r" % (self.output_dim,))
        if getattr(self.args, "alternate_corr", False):
            raise NotImplementedError("alternate_corr (the alt_cuda_corr extension) is not provided: the all-pairs correlation runs in the library; "
                                      "the library's own on-the-fly correlation is chosen with corr=\"on_the_fly\"")
        self.corr = getattr(self.args, "corr", "all_pairs")
        _lib.raft_corr_id(self.corr)
        self.share_frames = bool(getattr(self.args, "share_frames", False))
        self.multiframe = getattr(self.args, "multiframe", True)
        self.scale_inputs = getattr(self.args, "scale_inputs", True)
        self.hidden_dim = RAFT_HIDDEN
        self.context_dim = RAFT_HIDDEN
        self._iters = getattr(self.args, "iters", None)
        self.mode = "fast" if getattr(self.args, "mixed_precision", False) else "parity"
        self.fnet = BasicEncoder(output_dim=256, norm_fn="instance")
        self.cnet = BasicEncoder(output_dim=self.hidden_dim + self.context_dim, norm_fn="batch")
        self.update_block = BasicUpdateBlock(hidden_dim=self.hidden_dim)
        if self.output_dim is not None:  # raft_model.py:152-159
            self.output_block = nn.Sequential(nn.Conv2d(RAFT_HIDDEN, 256, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(256, self.output_dim, 1, padding=0))
        else:
            self.output_block = None

    # ---- reference attribute surface -------------------------------------------------------------
    @property
    def iters(self):
        return getattr(self, "_iters", None)

    @iters.setter
    def iters(self, value=None):
        self._iters = value

    def set_iters(self, value=None):
        self.iters = value
        return self

    def set_mode(self, mode: str):
        """"fast" or "parity" for the forwards that follow (the packed weights hold both forms: nothing is re-packed)."""
        _lib.mode_id(mode)
        self.mode = mode
        return self

    def set_corr(self, corr: str):
        """"all_pairs" or "on_the_fly" for the forwards that follow (the first one after a change re-plans the workspace)."""
        _lib.raft_corr_id(corr)
        self.corr = corr
        return self

    def set_share_frames(self, on: bool = True):
        """Run the encoders once per distinct frame (True) or once per pair (False, the default) in the forwards that follow."""
        self.share_frames = bool(on)
        return self

    @property
    def last_encoder_images(self):
        """(fnet images, cnet images) of the last forward; (0, 0) before the first."""
        if self._handle is None:
            return (0, 0)
        f, c = C.c_int(), C.c_int()
        self._check(self._fn["encoder_images"](self._handle, C.byref(f), C.byref(c)))
        return (int(f.value), int(c.value))

    def workspace_bytes(self) -> int:
        """Bytes of activation workspace the library handle holds: what the last forward's shape and `corr` asked for (0 before the first forward)."""
        if self._handle is None:
            return 0
        n = C.c_uint64()
        self._check(self._fn["workspace_bytes"](self._handle, C.byref(n)))
        return int(n.value)

    def freeze_bn(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()

    # ---- C-ABI plumbing (the handle and sync_weights live in _handle.LibraryModule; the library folds the batch norms and packs the
    # convolutions at the next forward.  cwm_raft_* has no lanes or kernel timing: the arithmetic mode travels with each call, and the one per-handle
    # options, the form of the correlation and the sharing of frames, are set before each forward) -------
    _ABI = {role: "cwm_raft_" + role for role in ("destroy", "load_weight", "forward", "forward_ex", "set_corr", "workspace_bytes", "set_share_frames",
                                                  "encoder_images")}

    def _create(self, lib, h):
        return lib.cwm_raft_create(C.byref(h))

    def _run(self, x1, x2, B, pairs, H, W, scale, iters, out, out_strides, flow_low=None, flow_init=None, per_iteration=None, share=None):
        """One library forward.  `out` = (pointer,) of the last iteration's output, addressed with `out_strides` (b, t, c), or None.  Without
        `flow_init` and `per_iteration` the call is `cwm_raft_forward`; with either, `cwm_raft_forward_ex`: `flow_init` [B or 1, 2, H/8, W/8] fp32
        goes to every pair, `per_iteration` = (pointer, stride between iterations) receives every iteration's output, addressed inside an
        iteration's block with `out_strides`.  `share`: the call's sharing of frames (None: the model's)."""
        dev = x1.device
        self.sync_weights(dev)
        extended = flow_init is not None or per_iteration is not None
        ex = _lib.new_raft_forward_ex_args() if extended else None
        a = ex.base if extended else _lib.new_raft_forward_args()
        a.image1_dev, a.image2_dev = x1.data_ptr(), x2.data_ptr()
        a.image1_stride_b, a.image1_stride_t, a.image1_stride_c = x1.stride(0), x1.stride(1), x1.stride(2)
        a.image2_stride_b, a.image2_stride_t, a.image2_stride_c = x2.stride(0), x2.stride(1), x2.stride(2)
        a.batch, a.pairs, a.height, a.width = B, pairs, H, W
        a.input_scale = float(scale)
        a.iters = int(iters)
        a.mode = _lib.mode_id(self.mode)
        if self.output_dim is None:
            a.flow_dev = out[0] if out is not None else None
            a.flow_stride_b, a.flow_stride_t, a.flow_stride_c = out_strides
        else:  # the head's value is what is upsampled; the flow's own upsampling is not asked for
            a.head_dev = out[0] if out is not None else None
            a.head_stride_b, a.head_stride_t, a.head_stride_c = out_strides
        a.flow_low_dev = _lib.ptr(flow_low)
        a.stream = _lib.current_stream_handle(dev)
        if flow_init is not None:  # one field for every pair (stride_t = 0), and for every batch row when its batch is 1
            ex.flow_init_dev = flow_init.data_ptr()
            ex.flow_init_stride_b = flow_init.stride(0) if flow_init.shape[0] > 1 else 0
            ex.flow_init_stride_t, ex.flow_init_stride_c = 0, flow_init.stride(1)
        if per_iteration is not None:
            if self.output_dim is None:
                ex.flow_iters_dev, ex.flow_iters_stride_i = per_iteration
            else:
                ex.head_iters_dev, ex.head_iters_stride_i = per_iteration
        self._check(self._fn["set_corr"](self._handle, _lib.raft_corr_id(self.corr)))
        self._check(self._fn["set_share_frames"](self._handle, int(bool(self.share_frames if share is None else share))))
        with torch.cuda.device(dev):
            if extended:
                self._check(self._fn["forward_ex"](self._handle, C.byref(ex)))
            else:
                self._check(self._fn["forward"](self._handle, C.byref(a)))

    @staticmethod
    def _frames(x: torch.Tensor) -> torch.Tensor:
        _lib.require_gpu()
        if not x.is_cuda:
            raise RuntimeError("RAFT.forward needs a CUDA/HIP tensor (no CPU fallback); got %s" % x.device)
        if x.dtype != torch.float32:
            x = x.float()
        if x.stride(-1) != 1 or x.stride(-2) != x.shape[-1]:
            x = x.contiguous()
        return x

    @staticmethod
    def _flow_init(flow_init, B: int, H: int, W: int, device) -> Optional[torch.Tensor]:
        """The warm start as the library reads it: fp32 [B or 1, 2, H/8, W/8] on the frames' device with contiguous rows; None stays None."""
        if flow_init is None:
            return None
        want = "[%d,2,%d,%d] or [1,2,%d,%d]" % (B, H // 8, W // 8, H // 8, W // 8)
        if not torch.is_tensor(flow_init) or not flow_init.is_floating_point():
            raise RuntimeError("flow_init must be a floating-point tensor %s, got %r" % (want, type(flow_init).__name__ if not torch.is_tensor(flow_init) else flow_init.dtype))
        if flow_init.dim() != 4 or flow_init.shape[0] not in (1, B) or tuple(flow_init.shape[1:]) != (2, H // 8, W // 8):
            raise RuntimeError("flow_init must be %s for frames [%d,3,%d,%d], got %s" % (want, B, H, W, tuple(flow_init.shape)))
        if flow_init.device != device:
            raise RuntimeError("flow_init %s is on %s but the frames [%d,3,%d,%d] are on %s" % (tuple(flow_init.shape), flow_init.device, B, H, W, device))
        f = flow_init.detach().float()
        if f.stride(-1) != 1 or f.stride(-2) != f.shape[-1]:
            f = f.contiguous()
        return f

    @torch.no_grad()
    def _forward_two_images(self, image1, image2, iters=24, flow_init=None, upsample=True, test_mode=True, **kwargs):
        """raft_model.py:199-274: for images in [0,255], (coords1 - coords0, flow_up) with test_mode=True and the list of every iteration's flow_up
        with test_mode=False; `flow_init` [B or 1, 2, H/8, W/8] (1/8-resolution pixels) is added to the initial coordinates."""
        if self.iters is not None:
            iters = self.iters
        x1, x2 = self._frames(image1), self._frames(image2)
        if x1.dim() != 4 or x1.shape != x2.shape or x1.shape[1] != 3:
            raise RuntimeError("expected two [B,3,H,W] images of one shape, got %s and %s" % (tuple(image1.shape), tuple(image2.shape)))
        B, _, H, W = x1.shape
        init = self._flow_init(flow_init, B, H, W, x1.device)
        v1, v2 = x1.unsqueeze(1), x2.unsqueeze(1)
        if not test_mode:  # every iteration's prediction: one buffer [iters,B,C,H,W], returned as the list of its views
            ups = torch.empty(max(int(iters), 0), B, self.output_dim or 2, H, W, device=x1.device)
            self._run(v1, v2, B, 1, H, W, 1.0, iters, None, (ups.stride(1), 0, ups.stride(2)), flow_init=init, per_iteration=(ups.data_ptr(), ups.stride(0)))
            return list(ups.unbind(0))
        up = torch.empty(B, self.output_dim or 2, H, W, device=x1.device)
        low = torch.empty(B, 2, H // 8, W // 8, device=x1.device)
        self._run(v1, v2, B, 1, H, W, 1.0, iters, (up.data_ptr(),), (up.stride(0), 0, up.stride(1)), flow_low=low, flow_init=init)
        return low, up

    @torch.no_grad()
    def flow_pairs(self, first, second, iters=24, flow_init=None, backward=False, share=None):
        """The flows of the pairs (first[b, s], second[b, s]): `first` and `second` [B,S,3,H,W] in the model's input range (in [0,1] with
        scale_inputs=True) -> [B,S,C,H,W], C = 2 or `output_dim`.  `backward=True` computes the pairs (second[b, s], first[b, s]), in the same order.
        Either argument may be an expanded view, with stride 0 over S or over B: with sharing on (`share`; None = the model's `share_frames`) such a
        frame goes through the encoders once, e.g. `flow_pairs(x0.expand(-1, S, -1, -1, -1), predicted, share=True)` for S samples of one first frame.
        With sharing off every pair is computed in full, as by the multi-frame call.
        A tensor that is not fp32 must be converted BEFORE it is expanded: converting an expanded view materialises the copies, and the call is then
        correct but shares nothing.  `flow_init` [B or 1, 2, H/8, W/8] starts every pair, as in the multi-frame call."""
        if self.iters is not None:
            iters = self.iters
        if first.dim() != 5 or first.shape != second.shape or first.shape[2] != 3:
            raise RuntimeError("flow_pairs expects two [B,S,3,H,W] tensors of one shape, got %s and %s" % (tuple(first.shape), tuple(second.shape)))
        x1, x2 = self._frames(first), self._frames(second)
        if x1.device != x2.device:
            raise RuntimeError("flow_pairs: first is on %s, second on %s" % (x1.device, x2.device))
        B, S, _, H, W = x1.shape
        init = self._flow_init(flow_init, B, H, W, x1.device)
        if backward:
            x1, x2 = x2, x1
        out = torch.empty(B, S, self.output_dim or 2, H, W, device=x1.device)
        self._run(x1, x2, B, S, H, W, 255.0 if self.scale_inputs else 1.0, iters, (out.data_ptr(),), (out.stride(0), out.stride(1), out.stride(2)),
                  flow_init=init, share=share)
        return out

    @torch.no_grad()
    def forward(self, *args, **kwargs):
        if not self.multiframe:
            return self._forward_two_images(*args, **kwargs)
        return self._forward_multiframe(*args, **kwargs)

    def _forward_multiframe(self, x, iters=24, flow_init=None, upsample=True, test_mode=True, backward=False, warm_start=False, **kwargs):
        """raft_model.py:276-300: the reference hands everything after x to every pair's two-image call (:297), so the arguments are those of
        `_forward_two_images`, plus `backward`.
        `warm_start=True` (not in the reference's forward: RAFT's video protocol, raft/utils.py:28-56) runs the pairs one after another, all B rows per
        library call, and starts each pair from `forward_interpolate` of the low-resolution flow of the pair before it in the chain, a field per batch row.
        With `backward` the chain runs from the last pair to the first (the flow of (x[t+1], x[t]) lives on frame t+1's grid and is carried to frame
        t's); the outputs keep their order.  `flow_init` then starts the first pair of the chain only; without it that pair is cold.  Nothing in the chain
        synchronises with the host.  With T <= 2 there is no chain: the call is the one without the keyword."""
        if self.iters is not None:
            iters = self.iters
        if x.dim() != 5:
            raise RuntimeError("RAFT (multiframe) expects x [B,T,3,H,W], got %s" % (tuple(x.shape),))
        x = self._frames(x)
        B, T, Cc, H, W = x.shape
        if Cc != 3:
            raise RuntimeError("RAFT expects 3-channel frames, got %s" % (tuple(x.shape),))
        # test_mode: either way the reference keeps `[-1]` of what the pair's call returns, the last iteration's flow_up: nothing to choose here
        init = self._flow_init(flow_init, B, H, W, x.device)  # the same field for every pair, forward or backward
        scale = 255.0 if self.scale_inputs else 1.0
        if T == 1:  # a single frame is repeated (raft_model.py:287-288): the pair (x0, x0)
            first, second, pairs = x, x, 1
        else:
            first, second, pairs = x[:, :-1], x[:, 1:], T - 1
        out = torch.empty(B, pairs, self.output_dim or 2, H, W, device=x.device)
        if warm_start and pairs > 1:
            # two [B,2,H/8,W/8] buffers: a pair's coords1 - coords0 (the flow, also under the output head) and its forward interpolation, the next init
            low, carried = torch.empty(2, B, 2, H // 8, W // 8, device=x.device).unbind(0)
            strides = (out.stride(0), 0, out.stride(2))
            for k in range(pairs):  # step k of the chain is pair t, stored at index `at`
                t = pairs - 1 - k if backward else k
                at = pairs - 1 - t if backward else t
                a, b = (x[:, t + 1:t + 2], x[:, t:t + 1]) if backward else (x[:, t:t + 1], x[:, t + 1:t + 2])
                self._run(a, b, B, 1, H, W, scale, iters, (out[:, at].data_ptr(),), strides, flow_low=low if k + 1 < pairs else None, flow_init=init)
                if k + 1 < pairs:
                    _forward_interpolate_into(low, carried)
                    init = carried
            return out
        if backward:  # pairs (x[t+1], x[t]), stored at index pairs - 1 - t
            first, second = second, first
            ptr = out.data_ptr() + (pairs - 1) * out.stride(1) * out.element_size()
            self._run(first, second, B, pairs, H, W, scale, iters, (ptr,), (out.stride(0), -out.stride(1), out.stride(2)), flow_init=init)
        else:
            self._run(first, second, B, pairs, H, W, scale, iters, (out.data_ptr(),), (out.stride(0), out.stride(1), out.stride(2)), flow_init=init)
        return out


def load_raft_model(load_path=default_raft_ckpt, ignore_prefix=None, multiframe=True, scale_inputs=True, output_dim=None, share_frames=False, **kwargs):
    """raft_model.py:55-101: builds RAFT-large and loads a checkpoint (`module.` and `ignore_prefix` stripped from the keys, strict=False);
    with `output_dim=1` and no path, a freshly initialised keypoint model.  `share_frames=True`: the encoders once per distinct frame of a call
    (`RAFT.set_share_frames`); the other keywords (`mixed_precision`, `corr`, ...) go to the model's `args`."""
    if ((load_path is None) or (not os.path.exists(load_path))) and (output_dim is None):
        print("%s is not a valid raft checkpoint" % load_path)
        raise ValueError("You must download RAFT checkpoints with cwm/models/raft/download_raft_checkpoints.sh\n"
                         + "Checkpoints will be downloaded to CounterfactualWorldModels/checkpoints/raft_checkpoints/")
    args = _args(**kwargs)
    args.multiframe, args.scale_inputs, args.output_dim, args.share_frames = multiframe, scale_inputs, output_dim, bool(share_frames)
    model = RAFT(args)
    if load_path is None:
        print("created a new %s with %d parameters" % (type(model).__name__, sum([v.numel() for v in model.parameters()])))
        return model
    weight_dict = torch.load(load_path, map_location=torch.device("cpu"))
    new_dict = {}
    for k in weight_dict.keys():
        new_dict[k.replace("module.", "") if "module" in k else k] = weight_dict[k]
    if ignore_prefix is not None:
        new_dict = {k.replace(ignore_prefix, ""): v for k, v in new_dict.items()}
    did_load = model.load_state_dict(new_dict, strict=False)
    print(did_load, type(model).__name__, load_path)
    return model
