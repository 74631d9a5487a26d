"""`PredictorBasedGenerator`: the wrapper surface the notebooks / UI drive (reference: cwm/models/prediction.py:17-850),
re-built around the HIP predictor.

Same method names, argument meaning and error behaviour as the reference class, so code written against it runs on a
`counterfactualworldmodels_amd.vmae` / `.conjoined_vmae` predictor.  What differs is how the work is organised:

* a prediction is ONE library call (normalise + forward + un-embed fused, `cwm_forward`); the wrapper never touches
  pixels or tokens itself, and there is no CPU path
* batches are described once -- frames, masks and the number of masked tokens per row (`_RectBatch`) -- and then cut
  into row ranges that are fed to the library back to back with no host synchronisation in between
  (`_run_rect_batch`); the only host round trip of a multi-row call is the mask rectangulariser's single read-back
* per-sample tiling (`sample_tile*`, `predict_per_sample`) is expressed as index arithmetic on the batch description
  instead of materialised `expand().reshape()` copies wherever the library can take strided rows
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _lib
from .config import IMAGENET_MEAN, IMAGENET_STD
from . import masking
from .masking import RectangularizeMasks, upsample_masks
from .perturbation import AddMarkers, MultiShiftPatchesAndMask, paint_markers
from .conjoined_vmae import ConjoinedPaddedVisionTransformer
from .vmae import PretrainVisionTransformer


def imagenet_normalize(x, temporal_dim=1):
    """(x - mean_c) / std_c with the channel axis at 2 (temporal_dim=1) or 1 (temporal_dim=2); cwm/models/utils.py:15-21."""
    shape = [1, 1, 1, 1, 1]
    shape[2 if temporal_dim == 1 else 1] = 3
    mean = torch.tensor(IMAGENET_MEAN, dtype=x.dtype, device=x.device).view(shape)
    std = torch.tensor(IMAGENET_STD, dtype=x.dtype, device=x.device).view(shape)
    return (x - mean) / std


def _region_of(target_mask, x, h, w):
    """The region an error is read on, `1 - target_mask` in x's dtype: the patches VISIBLE in a [B,Nt] mask, viewed as [B,T,h,w], or one
    minus any tensor of weights of that shape"""
    return 1 - (target_mask.view(x.shape[0], -1, h, w) if target_mask.dim() == 2 else target_mask).to(x)


@dataclass
class _RectBatch:
    """R independent prediction rows: frames [R,T,C,H,W] in [0,1], masks [R,Nt] whose rows all mask `n_masked` tokens
    (None: not known on the host; the library then counts row 0 and verifies the others), and per-row keyword tensors
    for the predictor (the IMU stream of the conjoined model)."""

    x: torch.Tensor
    mask: torch.Tensor
    n_masked: Optional[int]
    row_kwargs: Dict[str, object] = field(default_factory=dict)
    weights_synced: bool = False          # `_as_rect` ran the predictor's sync_weights() already (before the mask read-back)
    out: Optional[torch.Tensor] = None    # output video allocated there too (fused path)
    n_vis_range: Optional[tuple] = None   # ragged batch (`ragged_batches`): the rows' visible counts lie in [lo, hi]; the masks are as they were built

    @property
    def rows(self) -> int:
        return self.x.shape[0]


@dataclass
class MarkerResponses:
    """What `predict_marker_responses` returns for K markers: where each response peaks, how strong it is and where its weight lies.  Host arrays, but `maps`."""

    peak_yx: np.ndarray    # [K,2] int64: (Y, X) of the first maximum of the response
    peak: np.ndarray       # [K] float32: the response there
    mass: np.ndarray       # [K] float32: the response summed over the frame
    centroid: np.ndarray   # [K,2] float32: (Y, X) weighted by the response; the peak position where mass == 0
    maps: Optional[torch.Tensor] = None  # [K,H,W] on the device, with return_maps


class PredictorBasedGenerator(nn.Module):
    """Factual / counterfactual predictions from a masked predictor (reference class: prediction.py:17)."""

    def __init__(self, predictor=None, predictor_load_path=None, keypoint_predictor=None, keypoint_predictor_load_path=None,
                 error_func=None, imagenet_normalize_inputs=False, temporal_dim=2, seed=0, mask_generator=None, raft_iters=None,
                 max_shift_fraction=0.15, ragged_batches=False, **kwargs):
        super().__init__()
        # True: rows with different visible-token counts run as ONE ragged batch per library call (vmae.py forward(..., ragged=True)) where the
        # reference -- and the default here -- first un-masks random masked patches of the rows with fewer visible tokens until the counts agree
        # (`mask_rectangularizer`).  Masks then stay exactly as they were built, nothing is drawn from torch's global RNG, and a batched row is
        # predicted as it would be alone.
        self.ragged_batches = bool(ragged_batches)
        self.set_predictor(predictor, predictor_load_path)
        self.error_func = error_func if error_func is not None else nn.MSELoss(reduction="none")
        self.imagenet_normalize_inputs = bool(imagenet_normalize_inputs)
        self.set_temporal_dim(temporal_dim)
        # RNG streams in the reference's construction order (prediction.py:43-45, perturbation.py:26-28): the wrapper seeds
        # numpy + the GLOBAL torch generator, then each perturbation module seeds the global generator with its own default 0
        self.seed = seed
        self.rng = np.random.RandomState(seed=seed)
        self.torch_rng = torch.manual_seed(seed)
        self._shift_rng = np.random.RandomState(seed=0)
        torch.manual_seed(0)
        self.mask_generator = mask_generator
        self.mask_rectangularizer = RectangularizeMasks("min")
        self.max_shift_fraction = max_shift_fraction
        # prediction.py:59-64: pixel shifts, several patch groups per prompt; its numpy stream is its own (seed 0), its torch.manual_seed(0) the one above
        self.multi_patch_shifter = MultiShiftPatchesAndMask(patch_size=self.patch_size, max_shift_fraction=max_shift_fraction, padding_mode="constant",
                                                            allow_fractional_shifts=True)
        # the default marker of `predict_marker_responses` (perturbation.py:356-368: 'full', colour [1,0,0]); its torch.manual_seed(0) is again the one above
        self.marker = AddMarkers(patch_size=self.patch_size)
        self.keypoint_predictor = keypoint_predictor
        if keypoint_predictor is not None:
            self.load_predictor(keypoint_predictor_load_path, model=keypoint_predictor)
        self.shifts = None
        self.x = self.mask = self.timestamps = None

    # ---- predictor management (prediction.py:75-107) ---------------------------------------------------------------
    def set_predictor(self, net, predictor_load_path=None):
        if net is None:
            raise ValueError("There is no predictor set for this generator and no model to load to")
        self.predictor = net
        self.load_predictor(predictor_load_path)
        self.x = self.mask = self.inp_shape = None

    def load_predictor(self, load_path=None, model=None, map_location="cpu"):
        target = model if model is not None else getattr(self, "predictor", None)
        if target is None:
            raise ValueError("There is no predictor set for this generator and no model to load to")
        if load_path is None:
            inherited = getattr(self.predictor, "_predictor_load_path", None)
            if inherited is not None:
                self._predictor_load_path = inherited
            return
        state = torch.load(load_path, map_location=torch.device(map_location))
        state = state["model"] if "model" in state else state
        report = target.load_state_dict(state)
        if model is None:
            self._predictor_load_path = load_path
        print(report, load_path)

    # ---- geometry (prediction.py:131-207) --------------------------------------------------------------------------
    @property
    def patch_size(self):
        p = self.predictor
        return p.patch_size if hasattr(p, "patch_size") else p.encoder.patch_embed.proj.kernel_size

    @property
    def image_size(self):
        return self.predictor.image_size

    @property
    def sequence_length(self):
        p = self.predictor
        return p.sequence_length if hasattr(p, "sequence_length") else getattr(p, "num_frames", 2)

    @property
    def mask_shape(self):
        if hasattr(self.predictor, "mask_shape"):
            return self.predictor.mask_shape
        pt, ph, pw = self.patch_size
        h, w = self.inp_shape[-2:]
        return (self.sequence_length // pt, h // ph, w // pw)

    @property
    def inp_mask_shape(self):
        return (self.x.shape[0], int(np.prod(self.mask_shape)))

    @property
    def _is_padded(self):
        return hasattr(self.predictor, "main_stream") or hasattr(self.predictor, "max_padding_tokens")

    def set_temporal_dim(self, t_dim=1):
        if t_dim not in (1, 2):
            raise ValueError("temporal_dim must be 1 or 2")
        self.predictor.t_dim, self.predictor.c_dim = t_dim, 3 - t_dim

    t_dim = property(lambda self: self.predictor.t_dim)
    c_dim = property(lambda self: self.predictor.c_dim)

    def set_image_size(self, *args, **kwargs):
        setter = getattr(self.predictor, "set_image_size", None)
        if setter is not None:
            setter(*args, **kwargs)
        else:
            self.predictor.image_size = args[0]

    # ---- masks (prediction.py:109-129, 216-229, 357-384, 600-660) ---------------------------------------------------
    def generate_mask(self, x=None):
        assert self.mask_generator is not None
        x = self.x if x is None else x
        mask = self.mask_generator(x).view(x.size(0), -1).to(x.device)
        if self.ragged_batches:
            self._require_ragged()
            return mask
        return self.mask_rectangularizer(mask)

    def set_new_mask(self, x=None):
        self.mask = self.generate_mask(self.x if x is None else x)

    def reset_padding_masks(self):
        reset = getattr(self.predictor, "_reset_padding_mask", None)
        if self._is_padded and reset is not None:
            reset()

    def get_zeros_mask(self, x=None, frame=-1):
        """All-visible mask, with `frame` (if not None) fully masked; [B,Nt] bool (prediction.py:216-226)."""
        x = self.x if x is None else x
        if self.inp_shape is None:
            self.inp_shape = x.shape
        t, h, w = self.mask_shape
        masked_frame = torch.arange(t, device=x.device) == (frame % t if frame is not None else -1)
        return masked_frame.repeat_interleave(h * w)[None].expand(x.shape[0], -1)

    def get_fully_visible_mask(self, x=None):
        x = self.x if x is None else x
        return torch.zeros(self.mask_shape, device=x.device, dtype=torch.bool)

    def get_mask_image(self, mask, upsample=False, invert=False, shape=None):
        grid = mask.view(-1, *(self.mask_shape if shape is None else shape))
        if upsample:
            grid = upsample_masks(grid.view(grid.size(0), -1, *self.mask_shape[-2:]).float(), self.inp_shape[-2:])
        return 1 - grid if invert else grid

    @staticmethod
    def make_visible_from_patch_idx_list(mask, patch_idx_list, stride=1, b=0, t=-1):
        """Un-mask the listed patches of a [B,T,h,w] mask grid in place.  Entries are (h,w), (t,h,w) or (b,t,h,w); spatial
        indices are image coordinates divided by `stride` (prediction.py:619-638)."""
        if len(patch_idx_list) == 0:
            return mask
        idx = torch.as_tensor(np.asarray(patch_idx_list), dtype=torch.long, device=mask.device).reshape(-1, np.asarray(patch_idx_list).shape[-1])
        k = idx.shape[1]
        assert k in (2, 3, 4), k
        hh = (idx[:, -2] // stride) % mask.size(-2)
        ww = (idx[:, -1] // stride) % mask.size(-1)
        bb = idx[:, 0] if k == 4 else torch.full_like(hh, b)
        tt = idx[:, -3] if k >= 3 else torch.full_like(hh, t)
        mask[bb, tt, hh, ww] = 0
        return mask

    def generate_mask_from_patch_idx_list(self, patch_idx_list, stride=None, b=0, frame=-1):
        """Mask with `frame` hidden except the listed patches (prediction.py:640-649)."""
        assert self.x is not None
        grid = self.get_mask_image(self.get_zeros_mask(frame=frame).clone())
        if stride is None:
            stride = self.inp_shape[-1] // grid.size(-1)
        grid = self.make_visible_from_patch_idx_list(grid, patch_idx_list, stride=stride, b=b, t=frame)
        return grid.view(grid.size(0), -1)

    def get_nearby_patches(self, mask, radius=1, upsample=False, shape=None):
        """The patches of `mask` (viewed as [-1, *mask_shape], or `shape`) within `radius` of a visible one: `masking.patches_adjacent_to_visible` on the
        mask image, optionally upsampled to the input's pixels (prediction.py:345-351)."""
        nearby = masking.patches_adjacent_to_visible(self.get_mask_image(mask, shape=shape), radius=radius, size=None)
        if upsample:
            nearby = upsample_masks(nearby, size=self.inp_shape[-2:])
        return nearby

    def generate_cutout_mask(self, patch_idx_list, radius=1, stride=None, b=0, frame=-1):
        """The mask of `generate_mask_from_patch_idx_list` with frame `frame` replaced by `patches_adjacent_to_visible` of itself, the listed patches
        included (prediction.py:650-659); [B,Nt].  The reference slices `mask[:, frame:frame+1]`, which is empty for its own default frame=-1, and raises
        there; a negative frame is taken as `frame % T` here."""
        mask = self.get_mask_image(self.generate_mask_from_patch_idx_list(patch_idx_list, stride=stride, b=b, frame=frame))
        f = frame % mask.size(1)
        cutout = masking.patches_adjacent_to_visible(mask[:, f:f + 1], radius=radius)
        cutout = torch.maximum(cutout, ~mask[:, f:f + 1])
        mask[:, f] = cutout[:, 0]
        return mask.flatten(1)

    def get_masked_pred_patches(self, preds, mask, invert=False, fill_value=None):
        """`preds` [B,T',C,H,W] with everything outside the masked patches zeroed (or replaced by `fill_value`: a tensor of
        the same shape or one value per channel); prediction.py:261-283."""
        t_out, (h, w) = preds.shape[1], self.mask_shape[-2:]
        keep = upsample_masks(mask.view(-1, t_out, h, w), preds.shape[-2:]).to(preds)
        if invert:
            keep = 1.0 - keep
        keep = keep.unsqueeze(2)
        out = preds * keep
        if fill_value is None:
            return out
        if not isinstance(fill_value, torch.Tensor):
            fill_value = torch.tensor(fill_value, dtype=torch.float32).to(out).view(1, 1, -1, 1, 1)
        else:
            assert list(fill_value.shape) == list(out.shape)
        return out + (1 - keep) * fill_value

    # ---- the path itself -------------------------------------------------------------------------------------------
    def _preprocess(self, x):
        """What the predictor sees: [B,C,T,H,W] (t_dim=2), imagenet-normalised if configured (prediction.py:304-312)."""
        if self.t_dim != 1:
            x = x.transpose(self.t_dim, self.c_dim)
        return imagenet_normalize(x, temporal_dim=self.t_dim) if self.imagenet_normalize_inputs else x

    def pred_patches_to_video(self, y, x, mask):
        """Video with the input at visible patches and `y` at masked ones (prediction.py:245-259): one HIP scatter."""
        _lib.require_gpu()
        B, T, Cc, H, W = x.shape
        dev = y.device
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        y = y.to(torch.float32).contiguous()
        mask = mask.to(device=dev, dtype=torch.bool).reshape(B, -1).contiguous()
        n_vis = mask.shape[1] - int(mask[0].sum().item())
        out = torch.empty_like(x)
        with torch.cuda.device(dev):
            _lib.check(_lib.get_lib().cwm_unembed(y.data_ptr(), x.data_ptr(), mask.data_ptr(), B, T, Cc, H, W, self.patch_size[-1], n_vis,
                                                  out.data_ptr(), _lib.current_stream_handle(dev)))
        return out

    def _uses_fused_path(self, extra_args, row_kwargs) -> bool:
        return isinstance(self.predictor, PretrainVisionTransformer) and self.t_dim == 2 and not extra_args and not row_kwargs

    def _require_ragged(self, extra_args=(), row_kwargs=None, fused_call=True):
        """`ragged_batches` needs the plain predictor on its fused path; everything else says why not, at the call."""
        if self._is_padded or not isinstance(self.predictor, PretrainVisionTransformer):
            raise RuntimeError("ragged_batches=True is for the plain VMAE predictor: %s takes rows with different visible counts through its null-token "
                               "padding already" % type(self.predictor).__name__)
        if not fused_call or not self._uses_fused_path(extra_args, row_kwargs or {}):
            raise RuntimeError("ragged_batches=True runs on the fused predict path only (a two-frame movie on the GPU, no extra predictor arguments); this call "
                               "would go through the predictor's plain forward, whose rows must have equal visible counts")

    def _equalise(self, mask) -> tuple:
        """(mask, n_masked, n_vis_range) for the rows of a multi-row call: rectangularised as the reference does (prediction.py:421; in place, on torch's
        global RNG), or -- `ragged_batches` -- untouched, with the range of the rows' visible counts.  Either way the call's one host read-back."""
        if not self.ragged_batches:
            mask = self.mask_rectangularizer(mask)
            return mask, self.mask_rectangularizer.last_num_masked, None
        self._require_ragged()
        n_masked = mask.reshape(mask.shape[0], -1).sum(1)
        hi_m, lo_m = (int(v) for v in torch.stack([n_masked.max(), n_masked.min()]).tolist())
        Nt = mask[0].numel()
        return mask, None, (Nt - hi_m, Nt - lo_m)

    def _run_rect_batch(self, batch: _RectBatch, rows_per_call: Optional[int] = None, extra_args: Sequence = ()) -> torch.Tensor:
        """All rows of `batch` -> videos [R,T,C,H,W], `rows_per_call` rows per library call, every call writing its slice
        of ONE output tensor.  With `n_masked` known nothing here reads the device back, so the calls queue up behind each
        other on the stream."""
        R = batch.rows
        step = R if not rows_per_call else max(1, int(rows_per_call))
        Nt = batch.mask.shape[1]
        n_vis = None if batch.n_masked is None else Nt - batch.n_masked
        fused = self._uses_fused_path(extra_args, batch.row_kwargs)
        if batch.n_vis_range is not None:
            self._require_ragged(extra_args, batch.row_kwargs, fused_call=batch.x.is_cuda and batch.x.dim() == 5)
        out = None
        if fused:
            out = batch.out if batch.out is not None else torch.empty(batch.x.shape, device=batch.x.device, dtype=torch.float32)
        pieces = []
        for r0 in range(0, R, step):
            r1 = min(r0 + step, R)
            xs, ms = batch.x[r0:r1], batch.mask[r0:r1]
            if fused and batch.n_vis_range is not None:  # (the range was read from these very masks: nothing left to check)
                self.predictor.predict_video(xs, ms, normalize=self.imagenet_normalize_inputs, check=False, out_video=out[r0:r1],
                                             weights_synced=batch.weights_synced, ragged=True, n_vis_range=batch.n_vis_range)
                continue
            if fused:
                self.predictor.predict_video(xs, ms, normalize=self.imagenet_normalize_inputs, n_vis=n_vis, check=n_vis is None,
                                             out_video=out[r0:r1], weights_synced=batch.weights_synced)
                continue
            kw = {k: (v[r0:r1] if isinstance(v, torch.Tensor) else v) for k, v in batch.row_kwargs.items()}
            if n_vis is not None and isinstance(self.predictor, ConjoinedPaddedVisionTransformer):
                kw.update(n_vis=n_vis, check=False)  # counts known on the host: the library need not read them back
            y = self.predictor(self._preprocess(xs), ms, *extra_args, **kw)
            if self._is_padded:  # the padded predictors append max - min pad slots to the output (prediction.py:424-433)
                stream = getattr(self.predictor, "main_stream", self.predictor)
                y = y[:, : y.shape[1] - (stream.max_padding_tokens - stream.min_padding_tokens)]
            # NB the reference un-embeds with unnormalize(normalize(x)) for the conjoined model (prediction.py:436-446); the raw
            # input used here differs from that by at most one fp32 ulp at the visible pixels
            pieces.append(y if y.dim() == 5 else self.pred_patches_to_video(y, xs, mask=ms))
            if r1 < R:  # between pieces only: the state after the LAST piece is the caller's (`predict(reset_masks=False)` keeps it,
                self.reset_padding_masks()  # like the reference, prediction.py:451-452)
        return out if fused else (pieces[0] if len(pieces) == 1 else torch.cat(pieces, 0))

    def _as_rect(self, x, mask, row_kwargs=None, extra_args=(), for_video=False, alloc_video=True) -> _RectBatch:
        """Equalise the masked count over the rows the way the reference does for every multi-row call (prediction.py:421):
        in place, on torch's global RNG, and -- the one host sync -- remember the count."""
        # Host work that does not depend on the mask goes FIRST: the read-back below waits for everything queued on the stream (the previous
        # call's forward), and whatever the host still has to do after it delays this call's first kernel launch by as much (measured:
        # 230 us between the read-back and the first launch, 90 of them the walk over the parameters in sync_weights; tools/wrap_gap.py)
        synced, out = False, None
        if for_video and x.is_cuda and x.dim() == 5 and self._uses_fused_path(extra_args, row_kwargs or {}):
            self.predictor.sync_weights(x.device)
            synced = True
            if alloc_video:  # (False: the fused call wants the tokens only -- `_region_error_fused`)
                out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        n_masked, n_vis_range = None, None
        if x.size(0) > 1:
            if self.ragged_batches:
                self._require_ragged(extra_args, row_kwargs, fused_call=for_video and x.is_cuda and x.dim() == 5)
            mask, n_masked, n_vis_range = self._equalise(mask)
        return _RectBatch(x, mask, n_masked, dict(row_kwargs or {}), synced, out, n_vis_range)

    @staticmethod
    def _select_frame(video, frame):
        if frame is None:
            return video
        f = frame % video.size(1)
        return video[:, f : f + 1]

    def predict(self, x=None, mask=None, frame=-1, reset_masks=True, *args, **kwargs):
        """Predicted video [B,T,C,H,W] (or its frame `frame`) for movie x [B,T,C,H,W] in [0,1] and mask [B,Nt];
        prediction.py:406-454."""
        x = self.x if x is None else x
        mask = self.generate_mask(x) if mask is None else mask
        self.set_image_size(x.shape[-2:])
        self.inp_shape = x.shape
        video = self._run_rect_batch(self._as_rect(x, mask, kwargs, args, for_video=True), extra_args=args)
        if reset_masks:
            self.reset_padding_masks()
        return self._select_frame(video, frame)

    def predict_tokens(self, x, mask):
        """Raw predictor output [B,Nm,C*P*P] for wrapper-level input (the seam of prediction.py:419)."""
        return self.predictor(self._preprocess(x), self._as_rect(x, mask).mask)

    def predict_error(self, x=None, mask=None, target=None, frame=None, dim=-3):
        """error_func(prediction, target) summed over `dim` (prediction.py:331-343)."""
        x = self.x if x is None else x
        mask = self.generate_mask(x) if mask is None else mask
        pred = self.predict(x, mask, frame=frame)
        target = x if target is None else target
        if frame is not None:
            target = target[:, frame].unsqueeze(1)
        return self.error_func(pred, target).sum(dim, True)

    # ---- errors on a target region (prediction.py:324-329, 542-615) ----------------------------------------------------
    def _get_error(self, pred, gt, dim=-3, frame=None):
        """error_func of the last gt.shape[1] predicted frames against gt, summed over `dim` (prediction.py:324-329)."""
        return self.error_func(pred[:, -gt.shape[1]:], gt).sum(dim, True)

    def predict_with_mask(self, mask, invert_mask=False, *args, **kwargs):
        """`predict` on the generator's own input (`set_input`) with `mask` (or its complement); prediction.py:542-546."""
        assert self.x is not None
        if invert_mask:
            mask = ~mask
        return self.predict(self.x, mask.view(*self.inp_mask_shape), *args, **kwargs)

    def error_with_mask(self, mask, invert_mask=False, frame=-1, *args, **kwargs):
        """Per-pixel error [B,1,1,H,W] of `predict_with_mask` against frame `frame` of the generator's input (prediction.py:548-551)."""
        x_pred = self.predict_with_mask(mask, invert_mask, *args, **kwargs)
        return self._get_error(x_pred[:, frame].unsqueeze(1), self.x[:, frame].unsqueeze(1), dim=-3)

    def _patch3(self, patch_size=None):
        ps = tuple(self.patch_size if patch_size is None else patch_size)
        return ps if len(ps) == 3 else (1,) + ps

    def _error_takes_fused_path(self, x, target, region, aggregate_over_patches, patch_size, kwargs) -> bool:
        """The fused path of `get_error_on_target_region`: tokens -> per-patch errors in one kernel (cwm_patch_error), no predicted video."""
        if not (self._uses_fused_path((), kwargs) and x.is_cuda and x.dim() == 5 and aggregate_over_patches):
            return False
        if not (isinstance(self.error_func, nn.MSELoss) and self.error_func.reduction == "none"):
            return False
        if patch_size is not None and self._patch3(patch_size) != self._patch3():
            return False
        B, T, _, H, W = x.shape
        P = self.patch_size[-1]
        if self._patch3() != (1, P, P) or tuple(region.shape) != (B, T, H // P, W // P):
            return False
        return target is None or (tuple(target.shape) == tuple(x.shape) and target.device == x.device)

    def _region_error_fused(self, x, batch: _RectBatch, region, target, frame, want_mean):
        """(map [B,T,h,w], mean [B] or None) for the rows of a rectangular `batch` whose frames are `x` (any batch stride, 0 included): the predictor's
        tokens (normalisation fused, no video) and then ONE library call that turns tokens, frames and mask into per-patch errors.  Nothing here
        reads the device back when the batch knows its masked count."""
        pred = self.predictor
        dev = x.device
        B, T, Cc, H, W = x.shape
        P = self.patch_size[-1]
        Nt = T * (H // P) * (W // P)
        mask = batch.mask.to(device=dev, dtype=torch.bool).reshape(B, Nt).contiguous()
        n_masked = batch.n_masked if batch.n_masked is not None else int(mask[0].sum().item())  # (one row, or a caller that did not count: as `_run`)
        xs, (sb, sc, st) = pred._frame_strides(x, 2, 1)
        y = None
        if n_masked > 0:  # (nothing masked: every patch is the input's, there is no token to predict)
            y, _ = pred._run(xs, (sb, sc, st), self.imagenet_normalize_inputs, mask, Nt - n_masked, False, check=False, weights_synced=batch.weights_synced)
        tg = None if target is None else pred._frame_strides(target, 2, 1)[0]
        region = region.to(device=dev, dtype=torch.float32).contiguous()
        emap = torch.empty((B, T, H // P, W // P), device=dev, dtype=torch.float32)
        mean = torch.empty((B,), device=dev, dtype=torch.float32) if want_mean else None
        a = _lib.fill_patch_args(_lib.new_patch_error_args(), x=xs, target=tg, mask=mask, region=region, y=y, geometry=(B, T, Cc, H, W, P), n_vis=Nt - n_masked,
                                 frame=-1 if frame is None else frame % T, map=emap, mean=mean, stream=_lib.current_stream_handle(dev))
        with torch.cuda.device(dev):
            _lib.check(_lib.get_lib().cwm_patch_error(C.byref(a)))
        return emap, mean

    def get_error_on_target_region(self, x, mask, target_mask, target=None, average_error=True, frame=-1, aggregate_over_patches=True, patch_size=None,
                                   **kwargs):
        """How wrong the prediction of (x, mask) is on a region (prediction.py:553-574).  The region is `1 - target_mask`: the patches VISIBLE in a
        [B,Nt] target mask, or any [B,T,h,w] tensor of weights.  The error is `error_func` summed over the channels and averaged over each patch,
        [B,T,h,w]: with an integer `frame` the ONE predicted frame against EVERY frame of the target (`target`, default x), with frame=None frame t
        against frame t.  average_error: [B], the region-weighted mean (region sum clamped to >= 1); otherwise the region-weighted map.
        aggregate_over_patches=False: the per-pixel error [B,T,1,H,W].  Unlike the reference, which needs `set_input` or `predict` first (its
        `mask_shape` reads `inp_shape`), the image size is taken from `x`.

        The plain predictor on the GPU with the default MSE error computes this from the predicted tokens in one kernel (cwm_patch_error) and never
        builds the predicted video; everything else -- conjoined predictors, a custom error_func, aggregate_over_patches=False, another patch_size,
        extra predictor arguments, a ragged batch -- composes `predict`, `error_func` and `avg_pool3d` as the reference does."""
        ps = self._patch3()
        h, w = x.shape[-2] // ps[-2], x.shape[-1] // ps[-1]
        region = _region_of(target_mask, x, h, w)
        if self._error_takes_fused_path(x, target, region, aggregate_over_patches, patch_size, kwargs):
            self.set_image_size(x.shape[-2:])
            self.inp_shape = x.shape
            batch = self._as_rect(x, mask, for_video=True, alloc_video=False)
            if batch.n_vis_range is not None and batch.n_vis_range[0] == batch.n_vis_range[1]:  # a `ragged_batches` generator whose rows agree
                batch.n_masked, batch.n_vis_range = batch.mask[0].numel() - batch.n_vis_range[0], None
            if batch.n_vis_range is None:
                emap, mean = self._region_error_fused(x, batch, region, target, frame, want_mean=average_error)
                return mean if average_error else emap * region
            # (rows with different counts: the ragged forward's token layout is not the kernel's -- composed below; nothing was drawn or changed)
        error = self._get_error(self.predict(x, mask, frame=frame, **kwargs), x if target is None else target)
        if not aggregate_over_patches:
            return error
        ps = self._patch3(patch_size)
        error = nn.functional.avg_pool3d(error.transpose(1, 2), ps, stride=ps).squeeze(1) * region
        if not average_error:
            return error
        return error.sum((1, 2, 3)) / region.sum((1, 2, 3)).clamp(min=1)

    @staticmethod
    def unmask_one_patch(mask, idx=None, mask_shape=None, inplace=False, frame=0):
        """`mask` with one patch made visible (prediction.py:580-607).  Without `mask_shape`: mask [B,N], token `idx` of every row.  With it: the mask
        is viewed as [-1, *mask_shape] and `idx` is (h, w) -- in frame `frame` --, (t, h, w) for every row, or (b, t, h, w) for one."""
        shape = mask.shape
        if not inplace:
            mask = mask.clone()
        if mask_shape is None:
            assert len(shape) == 2, "If you don't pass a mask shape, it must be [B,N]"
            mask[:, idx] = False
            return mask
        if isinstance(idx, (list, tuple)) and len(idx) == 2:
            idx = [frame] + list(idx)
        idx = [int(i) for i in idx]
        assert len(idx) in (len(mask_shape), len(mask_shape) + 1), (idx, mask_shape)
        grid = mask.view(-1, *mask_shape)
        if len(idx) == len(mask_shape):
            grid[(slice(None),) + tuple(idx)] = False
        else:
            grid[tuple(idx)] = False
        return grid.view(*shape)

    @staticmethod
    def patch_idx_list_from_mask(mask):
        """[b, t, h, w] of every visible patch of a [B,T,h,w] mask, in row-major order (prediction.py:609-615)."""
        assert len(mask.shape) == 4, mask.shape
        return [list(p) for p in np.argwhere(~mask.bool().cpu().numpy())]

    # ---- error-guided unmasking (no counterpart in the reference: the search its keypoint net distils) -----------------
    def greedy_unmask(self, x, mask, target_mask=None, num_steps=1, candidates=None, num_candidates=None, frame=-1, target=None, sample_batch_size=None,
                      return_scores=False, radius=None):
        """Reveal, `num_steps` times, the masked patch of frame `frame` whose un-masking leaves the lowest mean error on the region
        (`get_error_on_target_region`; the default region is every patch of `frame`).  x [1,T,C,H,W], mask [1,Nt]; tokens are indices into the Nt
        tokens of the mask.  The candidates of a step are the still-masked tokens of `frame` -- of `candidates` if given; `num_candidates` of them
        drawn with `self.rng.choice(..., replace=False)` and sorted, if given.  Row c of a step's batch is the current mask with candidate c un-masked,
        so all rows have equal counts: nothing is rectangularised and torch's global RNG is not touched.  The frames go in as a stride-0 expand of
        x, never copied, and the rows are scored on the fused path in chunks of `sample_batch_size`, with one host read-back per step.  The pick is the
        lowest score; among equal scores the lowest token index.  Returns (mask_out [1,Nt], picks [num_steps], scores [num_steps]) and, with
        return_scores, a list of each step's (candidates, scores).

        An integer `radius` keeps, of each step's candidates, those on the frontier of the current mask: the masked patches of `frame` within `radius` of a
        visible one (`masking.patches_adjacent_to_visible`, computed from the host copy of the mask: no extra read-back).  A step whose candidates have
        none on the frontier searches them all.  radius=None is the search over all candidates."""
        if x.dim() != 5 or x.shape[0] != 1:
            raise ValueError("greedy_unmask searches the prompts of ONE movie: x must be [1,T,C,H,W], got %s" % (tuple(x.shape),))
        if frame is None:
            raise ValueError("greedy_unmask un-masks patches of one frame: frame must be an index")
        _, T, _, H, W = x.shape
        P = self.patch_size[-1]
        h, w = H // P, W // P
        n, Nt = h * w, T * h * w
        f = frame % T
        dev = x.device
        cur = mask.reshape(1, Nt).to(device=dev, dtype=torch.bool).clone()
        if target_mask is None:
            region = torch.zeros((1, T, h, w), device=dev, dtype=torch.float32)
            region[:, f] = 1
        elif target_mask.dim() == 2:
            region = 1 - target_mask.view(1, -1, h, w).to(x)
        else:
            region = 1 - target_mask.to(x)
        if not self._error_takes_fused_path(x, target, region, True, None, {}):
            raise RuntimeError("greedy_unmask scores its candidates on the fused error path: the plain VMAE predictor on the GPU, a two-frame movie "
                               "[1,T,C,H,W], the default MSE error_func and a [1,T,h,w] region")
        self.set_image_size(x.shape[-2:])
        self.inp_shape = x.shape
        self.predictor.sync_weights(dev)
        host = cur[0].cpu().numpy().copy()  # the search's state on the host: read once, then kept in step with `cur`
        n_masked = int(host.sum())
        allowed = None if candidates is None else np.unique(np.asarray(candidates, dtype=np.int64).reshape(-1))
        picks, best, trace = [], [], []
        for _ in range(int(num_steps)):
            cand = f * n + np.flatnonzero(host[f * n:(f + 1) * n])
            if allowed is not None:
                cand = cand[np.isin(cand, allowed)]
            if radius is not None:
                near = self._frontier_candidates(host[f * n:(f + 1) * n], h, w, radius)
                on_frontier = cand[np.isin(cand, f * n + near)]
                if len(on_frontier):
                    cand = on_frontier
            if num_candidates is not None and len(cand) > num_candidates:
                cand = np.sort(self.rng.choice(cand, size=int(num_candidates), replace=False))
            if len(cand) == 0:
                raise ValueError("greedy_unmask: no masked candidate token is left in frame %d after %d steps" % (f, len(picks)))
            R = len(cand)
            rows = cur.expand(R, Nt).clone()
            rows[torch.arange(R, device=dev), torch.from_numpy(cand).to(dev)] = False
            step = R if not sample_batch_size else max(1, int(sample_batch_size))
            scores = torch.empty((R,), device=dev, dtype=torch.float32)
            for r0 in range(0, R, step):
                r1 = min(r0 + step, R)
                k = r1 - r0
                chunk = _RectBatch(x.expand(k, -1, -1, -1, -1), rows[r0:r1], n_masked - 1, weights_synced=True)
                _, mean = self._region_error_fused(chunk.x, chunk, region.expand(k, -1, -1, -1), None if target is None else target.expand(k, -1, -1, -1, -1),
                                                   frame, want_mean=True)
                scores[r0:r1] = mean
            s = scores.cpu().numpy()  # the step's one read-back
            order = np.lexsort((cand, s))  # by score, equal scores by token index
            pick = int(cand[order[0]])
            picks.append(pick)
            best.append(float(s[order[0]]))
            trace.append((cand.copy(), s.copy()))
            host[pick] = False
            cur[0, pick] = False
            n_masked -= 1
        out = (cur, np.asarray(picks, dtype=np.int64), np.asarray(best, dtype=np.float32))
        return out + (trace,) if return_scores else out

    @staticmethod
    def _frontier_candidates(frame_mask, h, w, radius) -> np.ndarray:
        """cells of one frame's host mask [h*w] that are masked and within `radius` of a visible one (the CPU path of masking.patches_adjacent_to_visible)"""
        grid = torch.from_numpy(np.ascontiguousarray(frame_mask, dtype=np.bool_)).view(1, 1, h, w)
        near = masking.patches_adjacent_to_visible(grid, radius=radius) & grid
        return np.flatnonzero(near.view(-1).numpy())

    _select_reveal = staticmethod(masking.select_reveal)  # (the name the selection had here; tests/test_frontier_unmask_cpu.py reaches it through it)

    def frontier_unmask(self, x, mask, num_steps=1, num_reveal=1, radius=1, frame=-1, target_mask=None, target=None, sample=False, generator=None,
                        return_trace=False):
        """Unmasking that grows outward from what is visible, guided by where the prediction is still wrong: `num_steps` times, predict (x, mask) once for the
        whole batch, take the per-patch error on the region (`get_error_on_target_region`; the default region is every patch of `frame`), and reveal in
        every row the `num_reveal` masked patches of `frame` with the largest error among those within `radius` of a visible patch
        (`masking.patches_adjacent_to_visible`; radius=None: among all).  A row with fewer frontier patches than `num_reveal` fills up from its other masked
        patches; equal errors go to the lower index; a frame without a visible patch has every patch on the frontier.  sample=True draws the patches
        without replacement with probability proportional to max(error, 0) instead (an exponential race: the key is error / e with e ~ Exp(1) drawn
        from `generator` on x's device).

        x [B,T,C,H,W], mask [B,Nt] with the same masked count in every row.  Returns (mask_out [B,Nt], picks [B,num_steps,num_reveal] int64 token
        indices on x's device, errors [B,num_steps]: the region's mean error before each step's reveal) and, with return_trace, a list of each step's
        (error map [B,T,h,w], frontier [B,h,w] bool).  One read-back before the loop (the counts), none inside it: on the fused error path a step is the
        forward to tokens and one library call (cwm_unmask_step).  CPU tensors, conjoined predictors and a custom error_func compose
        `get_error_on_target_region`, the torch distance transform and the same selection rule in torch.

        This is what the reference's `EnergySampleUnmask` (perturbation.py:589-640) was meant to be; that class does not run."""
        if x.dim() != 5:
            raise ValueError("frontier_unmask: x must be [B,T,C,H,W], got %s" % (tuple(x.shape),))
        if frame is None:
            raise ValueError("frontier_unmask un-masks patches of one frame: frame must be an index")
        B, T, _, H, W = x.shape
        P = self.patch_size[-1]
        h, w = H // P, W // P
        n, Nt = h * w, T * h * w
        f = frame % T
        k, steps = int(num_reveal), int(num_steps)
        if k < 1 or steps < 1:
            raise ValueError("frontier_unmask: num_steps and num_reveal must be at least 1")
        dev = x.device
        cur = mask.reshape(B, Nt).to(device=dev, dtype=torch.bool).clone()
        thr = masking.frontier_threshold(h, w, radius)
        if target_mask is None:
            region = torch.zeros((B, T, h, w), device=dev, dtype=torch.float32)
            region[:, f] = 1
        else:
            region = _region_of(target_mask, x, h, w)
        rows = cur.sum(1)
        lo, hi, in_frame = (int(v) for v in torch.stack([rows.min(), rows.max(), cur[:, f * n:(f + 1) * n].sum(1).min()]).tolist())  # the one read-back
        if lo != hi:
            raise ValueError("frontier_unmask: every row of the mask must have the same masked count (got %d .. %d): rectangularise it first" % (lo, hi))
        if in_frame < steps * k:
            raise ValueError("frontier_unmask: %d steps of %d patches need %d masked patches in frame %d of every row, a row has %d" % (steps, k, steps * k, f, in_frame))
        self.set_image_size(x.shape[-2:])
        self.inp_shape = x.shape
        fused = self._error_takes_fused_path(x, target, region, True, None, {}) and k <= 64 and n <= 4096 and min(h, w) >= 3
        if min(h, w) < 3:
            raise ValueError("frontier_unmask: the frontier needs a grid of at least 3 x 3 patches, got %d x %d" % (h, w))
        picks = torch.empty((steps, B, k), device=dev, dtype=torch.int32 if fused else torch.int64)
        errors = torch.empty((steps, B), device=dev, dtype=torch.float32)
        trace = []
        draw = (lambda: torch.empty((B, n), device=dev, dtype=torch.float32).exponential_(generator=generator)) if sample else (lambda: None)
        if fused:
            pred = self.predictor
            pred.sync_weights(dev)
            xs, (sb, sc, st) = pred._frame_strides(x, 2, 1)
            region = region.contiguous()
            thr_dev = torch.tensor([thr], dtype=torch.float32).to(dev)
            nxt = torch.empty_like(cur)
            a = _lib.new_unmask_step_args()
            tg = None if target is None else pred._frame_strides(target, 2, 1)[0]
            a.frame, a.num_reveal, a.mode, a.threshold_dev = f, k, int(bool(sample)), thr_dev.data_ptr()
            emap = torch.empty((B, T, h, w), device=dev, dtype=torch.float32)
            front = torch.empty((B, h, w), device=dev, dtype=torch.uint8) if return_trace else None
            for s in range(steps):
                n_masked = lo - s * k
                y, _ = pred._run(xs, (sb, sc, st), self.imagenet_normalize_inputs, cur, Nt - n_masked, False, check=False, weights_synced=True)
                e = draw()
                if return_trace:
                    emap = torch.empty((B, T, h, w), device=dev, dtype=torch.float32)
                    front = torch.empty((B, h, w), device=dev, dtype=torch.uint8)
                _lib.fill_patch_args(a.base, x=xs, target=tg, mask=cur, region=region, y=y, geometry=(B, T, x.shape[2], H, W, P), n_vis=Nt - n_masked, frame=f,
                                     map=emap, mean=errors[s], stream=_lib.current_stream_handle(dev))
                a.e_dev, a.mask_out_dev, a.picks_dev, a.frontier_dev = _lib.ptr(e), nxt.data_ptr(), picks[s].data_ptr(), _lib.ptr(front)
                with torch.cuda.device(dev):
                    _lib.check(_lib.get_lib().cwm_unmask_step(C.byref(a)))
                if return_trace:
                    trace.append((emap, front.bool()))
                cur, nxt = nxt, cur
        else:
            tm = (1 - region) if target_mask is None else target_mask
            for s in range(steps):
                emap = self.get_error_on_target_region(x, cur.clone(), tm, target=target, average_error=False, frame=frame)  # [B,T,h,w], region-weighted
                errors[s] = emap.sum((1, 2, 3)) / region.sum((1, 2, 3)).clamp(min=1)
                fm = cur[:, f * n:(f + 1) * n]
                if thr < 0:
                    front = fm
                else:
                    front = fm & (masking.patch_distance_transform(fm.reshape(B, 1, h, w), self_mask=False).view(B, n) <= thr)
                cells = masking.select_reveal(emap[:, f].reshape(B, n).float(), fm, front, k, draw())
                picks[s] = f * n + cells
                cur = cur.clone()
                cur[torch.arange(B, device=dev)[:, None], f * n + cells] = False
                if return_trace:
                    trace.append((emap, front.view(B, h, w)))
        out = (cur, picks.permute(1, 0, 2).to(torch.int64).contiguous(), errors.t().contiguous())
        return out + (trace,) if return_trace else out

    # ---- marker counterfactuals: where a perturbation lands (perturbation.py:356-476 is the prompt; the read-out has no counterpart in the reference) ------
    @staticmethod
    def _marker_patches(patch_idx_list) -> np.ndarray:
        """[K,3] (t, h, w) from entries (h, w) -- frame 0 --, (t, h, w) or (0, t, h, w): the conventions of `make_visible_from_patch_idx_list`"""
        rows = []
        for p in patch_idx_list:
            p = [int(i) for i in (p.tolist() if hasattr(p, "tolist") else p)]
            if len(p) not in (2, 3, 4):
                raise ValueError("predict_marker_responses: a patch is (h, w), (t, h, w) or (0, t, h, w), got %s" % (p,))
            if len(p) == 4 and p[0] != 0:
                raise ValueError("predict_marker_responses marks ONE movie: the row of a (b, t, h, w) entry must be 0, got %s" % (p,))
            rows.append(([0] + p if len(p) == 2 else p)[-3:])
        if not rows:
            raise ValueError("predict_marker_responses: patch_idx_list is empty")
        return np.asarray(rows, dtype=np.int64)

    @staticmethod
    def _response_statistics(r):
        """(peak_index [K] int64, stats [K,4]: peak, mass, centroid_y, centroid_x) of response maps r [K,H,W] in torch: the contract of cwm_token_response"""
        K, H, W = r.shape
        flat = r.reshape(K, -1)
        idx = flat.argmax(1)
        peak = flat.gather(1, idx[:, None])[:, 0]
        mass = flat.sum(1)
        Y = torch.arange(H, device=r.device, dtype=r.dtype)[None, :, None]
        X = torch.arange(W, device=r.device, dtype=r.dtype)[None, None, :]
        empty = mass == 0
        cy = torch.where(empty, torch.div(idx, W, rounding_mode="floor").to(r.dtype), (r * Y).sum((1, 2)) / mass)
        cx = torch.where(empty, (idx % W).to(r.dtype), (r * X).sum((1, 2)) / mass)
        return idx, torch.stack([peak, mass, cy, cx], 1)

    def _responses_take_fused_path(self, x, kwargs) -> bool:
        """The fused path of `predict_marker_responses`: tokens of the marked rows and of the clean row -> one kernel (cwm_token_response), no predicted video."""
        return x.is_cuda and x.dim() == 5 and self._uses_fused_path((), kwargs)

    def predict_marker_responses(self, x, patch_idx_list, mask=None, frame=-1, marker=None, sample_batch_size=None, return_maps=False, **kwargs):
        """Where K marker counterfactuals land.  x [1,T,C,H,W] is one movie; prompt k is x with ONE marker (`marker`, an `AddMarkers`; default a 'full'
        marker of colour [1,0,0]) painted into patch k of `patch_idx_list` -- (h, w) in frame 0, (t, h, w) or (0, t, h, w) -- under `mask` (default:
        `get_zeros_mask(frame=-1)`).  The response of prompt k is r_k[Y][X] = sum_c (prediction_k - clean prediction)^2 over predicted frame `frame`.
        Returns a `MarkerResponses`: peak_yx [K,2] (the first maximum of r_k, as torch.argmax), peak [K], mass [K] = sum r_k, centroid [K,2] =
        sum r_k (Y, X) / mass (the peak position when mass == 0), on the host, and with return_maps the maps [K,H,W] on the device.

        The marked patches must be visible under `mask` and lie in another frame than `frame` (ValueError otherwise): all rows then keep the clean row's
        mask, their predicted tokens line up with the clean row's, and a visible patch of `frame` is the same input pixel in every row.  The plain predictor on the GPU predicts the clean row once and the K rows in chunks of `sample_batch_size`, all to
        TOKENS, and each chunk is one library call (cwm_token_response) on its tokens and the clean row's: no predicted video and no difference map is
        built, and the host reads the results back once, at the end (the mask once, before anything is queued).  Everything else -- a conjoined predictor, predictor keyword arguments (tensors of one
        row), CPU tensors, temporal_dim 1 -- composes `predict`, the squared difference and the same statistics in torch, chunked the same way."""
        if x.dim() != 5 or x.shape[0] != 1:
            raise ValueError("predict_marker_responses marks ONE movie: x must be [1,T,C,H,W], got %s" % (tuple(x.shape),))
        if frame is None:
            raise ValueError("predict_marker_responses reads the response in one predicted frame: frame must be an index")
        _, T, Cc, H, W = x.shape
        P = self.patch_size[-1]
        h, w = H // P, W // P
        n, Nt = h * w, T * h * w
        f = frame % T
        dev = x.device
        self.set_image_size(x.shape[-2:])
        self.inp_shape = x.shape
        marker = self.marker if marker is None else marker
        if tuple(marker.patch_size[-2:]) != (P, P):
            raise ValueError("the marker's patches are %s, the predictor's %d x %d" % (tuple(marker.patch_size[-2:]), P, P))
        patches = self._marker_patches(patch_idx_list)
        if (patches < 0).any() or (patches >= np.array([T, h, w])).any():
            raise ValueError("predict_marker_responses: a patch outside the %d x %d x %d grid" % (T, h, w))
        if (patches[:, 0] == f).any():
            raise ValueError("predict_marker_responses reads the response in predicted frame %d: a marker goes into another frame, got %s" % (
                f, patches[patches[:, 0] == f].tolist()))
        K = len(patches)
        mask = (self.get_zeros_mask(x, frame=-1) if mask is None else mask).reshape(1, Nt).to(device=dev, dtype=torch.bool)
        host = mask[0].cpu().numpy()
        tokens = patches[:, 0] * n + patches[:, 1] * w + patches[:, 2]
        if host[tokens].any():
            raise ValueError("predict_marker_responses: marked patches must be visible under the mask; masked: %s" % patches[host[tokens]].tolist())
        n_masked = int(host.sum())
        markers = marker.sample_markers(K, x, Cc)  # (the marker's numpy draws, in list order)
        where = torch.from_numpy(patches).to(dev)
        step = K if not sample_batch_size else max(1, int(sample_batch_size))
        fused = self._responses_take_fused_path(x, kwargs)
        index = torch.empty((K,), device=dev, dtype=torch.int32)
        stats = torch.empty((K, 4), device=dev, dtype=torch.float32)
        maps = torch.empty((K, H, W), device=dev, dtype=torch.float32) if return_maps else None

        def prompts(r0, r1):
            xk = x.to(torch.float32).expand(r1 - r0, -1, -1, -1, -1).clone(memory_format=torch.contiguous_format)
            sel = where[r0:r1]
            return paint_markers(xk, markers[r0:r1], torch.arange(r1 - r0, device=dev), sel[:, 0], sel[:, 1], sel[:, 2], (P, P))

        if fused:
            pred = self.predictor
            pred.sync_weights(dev)

            def tokens_of(frames, rows):
                if n_masked == 0:  # (nothing masked: nothing is predicted, every response is 0)
                    return None
                xs, strides = pred._frame_strides(frames, 2, 1)
                return pred._run(xs, strides, self.imagenet_normalize_inputs, rows, Nt - n_masked, False, check=False, weights_synced=True)[0]

            y_ref = tokens_of(x, mask)
            scratch = torch.empty((min(step, K), h, 8), device=dev, dtype=torch.float32)
            a = _lib.new_token_response_args()
            a.y_ref_dev, a.y_ref_stride_b = _lib.ptr(y_ref), 0
            for r0 in range(0, K, step):
                r1 = min(r0 + step, K)
                rows = mask.expand(r1 - r0, Nt).contiguous()
                y = tokens_of(prompts(r0, r1), rows)
                _lib.fill_patch_args(a.base, mask=rows, y=y, geometry=(r1 - r0, T, Cc, H, W, P), n_vis=Nt - n_masked, frame=f, scratch=scratch,
                                     stream=_lib.current_stream_handle(dev))
                a.peak_index_dev, a.stats_dev = index[r0:r1].data_ptr(), stats[r0:r1].data_ptr()
                a.pixel_map_dev = maps[r0:r1].data_ptr() if return_maps else None
                with torch.cuda.device(dev):
                    _lib.check(_lib.get_lib().cwm_token_response(C.byref(a)))
        else:
            clean = self.predict(x, mask.clone(), frame=f, **kwargs)
            for r0 in range(0, K, step):
                r1 = min(r0 + step, K)
                kw = {k: (v.expand(r1 - r0, *v.shape[1:]) if torch.is_tensor(v) and v.shape[0] == 1 else v) for k, v in kwargs.items()}
                video = self.predict(prompts(r0, r1), mask.expand(r1 - r0, Nt).clone(), frame=f, **kw)
                r = ((video - clean) ** 2).sum(2)[:, 0].to(torch.float32)
                index[r0:r1], stats[r0:r1] = self._response_statistics(r)
                if return_maps:
                    maps[r0:r1] = r
        packed = torch.cat([index.view(torch.float32)[:, None], stats], 1).cpu().numpy()  # the call's one read-back (the indices travel as their bits)
        flat, s = packed[:, 0].copy().view(np.int32).astype(np.int64), packed[:, 1:]
        return MarkerResponses(np.stack([flat // W, flat % W], 1), s[:, 0].copy(), s[:, 1].copy(), s[:, 2:4].copy(), maps)

    # ---- per-sample batching (prediction.py:456-540) -----------------------------------------------------------------
    def sample_tile(self, z, num_samples):
        """[B,...] -> [(B num_samples),...]: every row repeated num_samples times, '(b s)' order."""
        return z.repeat_interleave(num_samples, 0, output_size=z.shape[0] * num_samples)

    def sample_tile_all_tensors(self, num_samples, **kwargs):
        return {k: (self.sample_tile(v, num_samples) if torch.is_tensor(v) else v) for k, v in kwargs.items()}

    def predict_per_sample(self, x, masks, frame=-1, batch_size=None, split_samples=True, *args, **kwargs):
        """S masks per movie, masks [B,Nt,S]: all B*S predictions as one rectangular batch.  Returns [(B S),T',C,H,W]
        ('(b s)' rows) or, with split_samples, [B,T',C,H,W,S]."""
        assert masks.dim() == 3, masks.shape
        x = self.x if x is None else x
        B, S = x.size(0), masks.size(-1)
        rows = self.sample_tile(x, S)
        row_masks = masks.permute(0, 2, 1).reshape(B * S, -1)
        y = self.predict(rows, row_masks, frame, True, *args, **kwargs)
        return y.view(B, S, *y.shape[1:]).movedim(1, -1) if split_samples else y

    def batch_predict_per_sample(self, x, masks, frame=-1, batch_size=None, sample_dim=None, **kwargs):
        """Chunked form.  sample_dim != 0: masks [B,Nt,S], chunks of `batch_size // B` samples, result [B,T',C,H,W,S].
        sample_dim == 0: x [R,...] and masks [R,Nt] are already one row per sample, chunks of `batch_size // R`... rows as
        the reference computes it (prediction.py:504-507), result [R,T',C,H,W].  Tensor keyword arguments are per movie and
        are tiled over each chunk's samples."""
        S = masks.size(0) if sample_dim == 0 else masks.size(-1)
        per_call = S if batch_size is None else max(1, batch_size // x.size(0))
        outs = []
        for s0 in range(0, S, per_call):
            s1 = min(s0 + per_call, S)
            if sample_dim == 0:
                assert x.size(0) in (masks.size(0), masks.size(-1)), (x.shape, masks.shape)
                m = masks[s0:s1] if masks.dim() == 2 else masks[..., s0:s1].permute(0, 2, 1).reshape(-1, masks.shape[1])
                outs.append(self.predict(x[s0:s1], m, frame, True, **self.sample_tile_all_tensors(s1 - s0, **kwargs)))
            else:
                outs.append(self.predict_per_sample(x, masks[..., s0:s1], frame=frame, split_samples=True,
                                                    **self.sample_tile_all_tensors(s1 - s0, **kwargs)))
            self.reset_padding_masks()
        return torch.cat(outs, 0 if sample_dim == 0 else -1)

    # ---- inputs (prediction.py:703-739) -------------------------------------------------------------------------------
    def set_input(self, x, mask=None, make_mask=False, timestamps=None):
        if x.dim() == 4:
            x = x.unsqueeze(1)
        elif x.dim() != 5:
            raise AssertionError("Input must be a movie of shape [B,T,C,H,W] or a single frame of shape [B,C,H,W]")
        self.x, self.inp_shape = x, x.shape
        self.B, self.T, self.C = x.shape[:3]
        if mask is not None:
            self.mask = mask
        elif make_mask:
            assert self.mask_generator is not None, "You need to have a mask generator to set a new mask"
            self.set_new_mask(x)
        if timestamps is not None:
            self.timestamps = timestamps

    def get_static_input(self, x=None):
        x = self.x if x is None else x
        return x[:, :1].repeat(1, x.size(1), 1, 1, 1)

    def make_static_movie(self, x=None, T=None, frame=0):
        x = self.x if x is None else x
        T = getattr(self.predictor, "num_frames", 2) if T is None else T
        if x.dim() == 4:
            x = x.unsqueeze(1)
        assert x.dim() == 5, "x must be of shape [B,C,H,W] or [B,T,C,H,W], but is %s" % (tuple(x.shape),)
        f = frame % x.size(1)
        return x[:, f : f + 1].repeat(1, T, 1, 1, 1)

    # ---- single-prompt counterfactual (the UI's click handler, interface.py:273-299) ----------------------------------
    def reset_shifts(self):
        self.shifts = []

    def _record_shift(self, dy, dx):
        if getattr(self, "shifts", None) is None:
            self.shifts = []
        self.shift = [int(dy), int(dx)]
        self.shifts.append(np.array(self.shift))

    def _random_mask_shift(self):
        """A random shift in patch units, `ShiftPatchesAndMask.get_random_shift(is_mask_shift=True)` (perturbation.py:209-225):
        pixel shifts up to max_shift_fraction of the image, floored to whole patches, redrawn while dy + dx == 0 (sic)."""
        ph, pw = self.patch_size[-2:]
        lim = [int(self.max_shift_fraction * s) for s in self.inp_shape[-2:]]
        while True:
            dy = int(self._shift_rng.randint(-lim[0], lim[0] + 1) // ph)
            dx = int(self._shift_rng.randint(-lim[1], lim[1] + 1) // pw)
            if dy + dx != 0:
                return (dy, dx)

    def _shift_rows(self, x, passive, active, shifts, frame, fix_passive, samples_per_movie=1, frames=True, masks=True, num_frames=None):
        """Device-side prompt construction for R = B * samples_per_movie rows (library: cwm_shift_prompts; reference:
        PatchPerturbation.forward + ShiftPatchesAndMask.perturb, perturbation.py:99-113, 245-289).  x [B,T,C,H,W]; passive /
        active [R,Nt] bool (0 = patch stays visible / 0 = patch is moved); shifts int32 [R,2] (dy,dx) in patch units.
        Returns (x_shift [R,T,C,H,W], mask_shift [R,Nt]) before rectangularisation; `frames=False` / `masks=False` skips that output (None): the
        sharded loop needs the masks of all prompts on rank 0 but frames only for the rows a rank predicts (dist.py)."""
        assert frames or masks
        _lib.require_gpu()
        if not x.is_cuda:
            raise RuntimeError("counterfactual prompts are built on the GPU (no CPU fallback); got a %s tensor" % x.device)
        dev = x.device
        B, T, Cc, H, W = x.shape
        if num_frames is not None and num_frames != T:
            # a static movie given as its first frame alone (`make_static_movie`, prediction.py:731-739, is frame 0 repeated): with fix_passive=True the kernel
            # reads frame 0 for every output frame, so the T-fold copy need not exist
            if not (T == 1 and fix_passive is True):
                raise RuntimeError("num_frames=%d needs a one-frame movie and fix_passive=True" % num_frames)
            # ONE movie only: the kernel finds movie b at (b T + frame) C H W with T = num_frames, which for b > 0 lies past the end of a tensor of B frames
            if B != 1:
                raise RuntimeError("num_frames=%d is the form for one movie given as its first frame; got %d movies of one frame: pass the %d-frame movies "
                                   "themselves (make_static_movie)" % (num_frames, B, num_frames))
            T = int(num_frames)
        R, N = passive.shape
        x = x.to(torch.float32).contiguous() if frames else None  # (masks only: the frames are not read; no 1.2-MB materialisation of an expanded movie on rank 0's path)
        passive = passive.to(device=dev, dtype=torch.bool).contiguous()
        active = active.to(device=dev, dtype=torch.bool).contiguous()
        shifts = shifts.to(device=dev, dtype=torch.int32).contiguous()
        x_shift = torch.empty((R, T, Cc, H, W), device=dev, dtype=torch.float32) if frames else None
        mask_shift = torch.empty((R, N), device=dev, dtype=torch.bool) if masks else None
        with torch.cuda.device(dev):
            _lib.check(_lib.get_lib().cwm_shift_prompts(
                _lib.ptr(x), B, T, Cc, H, W, self.patch_size[-1], frame % T, samples_per_movie,
                2 if fix_passive == "make_static" else int(bool(fix_passive)),
                active.data_ptr(), passive.data_ptr(), shifts.data_ptr(), _lib.ptr(x_shift), _lib.ptr(mask_shift),
                _lib.current_stream_handle(dev)))
        return x_shift, mask_shift

    def _shift(self, x, mask, active_patches=None, shift=None, frame=1, fix_passive=False):
        """One shift applied to every movie of x (prediction.py:760-779): returns (x_shift, rectangularised mask_shift) and
        appends the shift (patch units) to `self.shifts`.  fix_passive="make_static" applies `MakeStatic` (perturbation.py:120-145)
        to the patches `mask` leaves visible first, in the same kernel."""
        if active_patches is None:
            active_patches = torch.ones_like(mask)
        self.inp_shape = x.shape
        dy, dx = self._random_mask_shift() if shift is None else (int(shift[0]), int(shift[1]))
        table = torch.tensor([[dy, dx]], dtype=torch.int32).expand(x.shape[0], 2)
        x_shift, mask_shift = self._shift_rows(x, mask.reshape(x.shape[0], -1), active_patches.reshape(x.shape[0], -1), table, frame,
                                               fix_passive=fix_passive)
        self._record_shift(dy, dx)
        if self.ragged_batches:
            self._require_ragged()
            return x_shift, mask_shift
        return x_shift, self.mask_rectangularizer(mask_shift)

    def get_counterfactual_prediction(self, x, mask=None, active_patches=None, shift=None, fix_passive=False, **kwargs):
        """Move the active patches of frame 1 by `shift` patches, keep the passive ones (`mask`), predict the whole movie
        (prediction.py:781-812).  x may be an image [C,H,W] / [B,C,H,W] (made into a static 2-frame movie) or a movie."""
        if x.dim() == 3:
            x = x[None, None]
        elif x.dim() == 4:
            x = x[:, None]
        if x.size(1) == 1:
            x = self.make_static_movie(x, T=2)
        self.inp_shape = x.shape
        mask = self.get_zeros_mask(x) if mask is None else mask
        active_patches = self.get_zeros_mask(x) if active_patches is None else active_patches
        # fix_passive: `x, _ = self.make_static(x, mask)` (prediction.py:802-803) folded into the prompt kernel
        x_p, mask_p = self._shift(x, mask, active_patches=active_patches, shift=shift, frame=1,
                                  fix_passive="make_static" if fix_passive else False)
        return self.predict(x_p, mask_p, frame=None, **kwargs)

    def make_static(self, x, mask):
        """`MakeStatic` (perturbation.py:120-145; the generator's `make_static` attribute, prediction.py:51-55): the patches `mask`
        leaves visible in frames t > 0 take the pixels of the same patch in frame 0.  Returns (x_static, mask) like the reference."""
        B = x.shape[0]
        m = mask.reshape(B, -1)
        zero = torch.zeros((B, 2), dtype=torch.int32)
        x_static, _ = self._shift_rows(x, m, torch.ones_like(m), zero, 1, fix_passive="make_static")
        return x_static, mask

    # ---- keypoints (prediction.py:816-828): any module passed as `keypoint_predictor` ---------------------------------------
    def predict_keypoints_map(self, x, *args, **kwargs):
        assert x.dim() == 5, x.shape
        if self.keypoint_predictor is None:
            return torch.ones_like(x[:, 0:1, 0:1])
        return self.keypoint_predictor(x, *args, **kwargs)

    def predict_keypoints_distribution(self, x, power=8, eps=1e-3):
        value = self.predict_keypoints_map(x).squeeze(-3)
        value = (value.sigmoid()) ** power
        value = value - value.amin((-2, -1))
        return value / value.amax((-2, -1)).clamp(min=eps)

    def predict_keypoints(self, x, num_points=8, radius=2, rel_thresh=0.1, power=8):
        """The K = num_points keypoints of every movie of x [B,T,C,H,W] (no counterpart in the reference, which only ever samples from the map): the strongest
        local maxima of `predict_keypoints_distribution(x, power)` of the first frame pair, at least rel_thresh of the row's maximum and more than `radius`
        patches (Chebyshev) apart -- `seed_select.select_seeds(peaks_only=True)`.  Returns (points [B,K,2] int32 (y, x), (-1, -1) where a row has fewer
        peaks; values [B,K], the map at the points, 0 there).  Without a keypoint predictor the map is constant and has no peaks worth the name: ValueError."""
        if self.keypoint_predictor is None:
            raise ValueError("predict_keypoints needs a generator built with a keypoint_predictor")
        from .seed_select import select_seeds
        from .segment_merge import keypoints_distribution

        sel = select_seeds(keypoints_distribution(self, x, power), num_points, self.patch_size[-1], radius=radius, peaks_only=True, rel_thresh=rel_thresh)
        return sel.seeds, sel.values

    def forward(self, x, mask=None, frame=None, *args, **kwargs):
        self.set_input(x, mask)
        if mask is None:
            self.mask = self.generate_mask(x)
        return self.predict(self.x, self.mask, frame=frame, *args, **kwargs)
