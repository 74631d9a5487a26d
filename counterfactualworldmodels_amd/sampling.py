"""Patch sampling from an energy map and the flow-sample filter (reference: cwm/models/sampling.py:11-286,
cwm/models/utils.py:91-95, :152-213): the glue of `FlowGenerator.sample_counterfactual_motion_map` between the predictor and
the flow-sample statistics.

* `EnergySamplingMaskingGenerator` / `RotatedTableEnergyMaskingGenerator` draw the visible patches of a prompt from an energy map.
  This is host logic on a few hundred elements whose whole value is that it draws what the reference draws: it pools and samples on
  the CPU, in the reference's op order, from the global torch generator (a device energy map is copied to the host first), so masks
  are bit-equal to the reference's under the same seeds; the masks are returned on the energy's device.
* `FlowSampleFilter.forward` runs on the device (`cwm_flow_filter_stats`, `cwm_flow_filter_apply`, `cwm_flow_filter_pack`:
  csrc/flowfilter.hip); there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F
from torch import nn
from torch.distributions.categorical import Categorical

from . import _lib
from .flowstats import _require_cuda, _sample_outermost, _strides5
from .masking import MaskingGenerator, upsample_masks


# ---- cwm/models/utils.py -------------------------------------------------------------------------------------------------
def boltzmann(x, beta=1, eps=1e-9):
    """exp(beta x) / max over (H, W); beta None: x unchanged (utils.py:91-95)."""
    if beta is None:
        return x
    x = torch.exp(x * beta)
    return x / x.amax((-1, -2), keepdim=True).clamp(min=eps)


def sample_image_inds_from_probs(probs, num_points, eps=1e-9, normalize=False, seed=0):
    """probs [B,H,W] -> [B,P,2] (row, column) of P categorical draws per image (utils.py:152-170)."""
    B, H, W = probs.shape
    probs = probs.reshape(B, H * W)
    if normalize:
        probs = probs - probs.amin(-1, True)
    probs = F.relu(probs + eps)
    probs = probs / probs.to(probs.dtype).sum(dim=-1, keepdim=True).clamp(min=eps)
    indices = Categorical(probs=probs).sample([num_points]).permute(1, 0).to(torch.long)  # [B,P]
    indices_h = torch.minimum(torch.maximum(torch.div(indices, W, rounding_mode="floor"), torch.tensor(0)), torch.tensor(H - 1))
    indices_w = torch.minimum(torch.maximum(torch.fmod(indices, W), torch.tensor(0)), torch.tensor(W - 1))
    return torch.stack([indices_h, indices_w], dim=-1)


def sample_from_energy(probs, num_points=1, num_samples=1, binarize=False, normalize=False, eps=1e-9):
    """probs [B,1,H,W] or [B,T,1,H,W] -> the same shape (B * num_samples rows) with the drawn points set to their energy, or to 1 with
    `binarize` (utils.py:172-213)."""
    shape = probs.shape
    if len(shape) == 5:
        B, T, _, H, W = shape
    elif len(shape) == 4:
        B, _, H, W = shape
        T = 1
        probs = probs[:, None]
    else:
        raise ValueError(probs.shape)
    assert probs.size(-3) == 1, probs.shape
    S, P = num_samples, num_points
    probs = probs.unsqueeze(1).expand(-1, S, -1, -1, -1, -1).reshape(B * S * T, H, W)
    inds = sample_image_inds_from_probs(probs, P, eps=eps, normalize=normalize)
    rows = torch.arange(B * S * T, dtype=torch.long)[:, None].expand(-1, P).to(inds.device)
    where = (rows.flatten(), inds[..., 0].flatten(), inds[..., 1].flatten())
    values = torch.ones(B * S * T * P, dtype=probs.dtype, device=probs.device) if binarize else probs[where]
    activated = torch.zeros_like(probs)
    activated[where] = values
    activated = activated.view(B * S, T, 1, H, W)
    return activated[:, 0] if len(shape) == 4 else activated


# ---- cwm/models/sampling.py:11-126 -----------------------------------------------------------------------------------------
class EnergySamplingMaskingGenerator(MaskingGenerator):
    """Sample the visible patches where an energy map is high (sampling.py:11-113).  `temperature` None: the energy is used as it is;
    otherwise exp((e - max e) * temperature).  `clumping_factor` f: f x f blocks of patches are drawn together."""

    def __init__(self, input_size, mask_ratio, seed=0, resize=True, temperature=None, clumping_factor=1, pool_mode="mean", eps=1e-9,
                 energy_power=1, **kwargs):
        if resize:
            raise NotImplementedError("resize=True resizes the energy map with torchvision.transforms.Resize, which this package does not depend on: "
                                      "pass resize=False (FlowGenerator's default) and an energy map whose sides are multiples of the patch grid")
        super().__init__(input_size=input_size, mask_ratio=mask_ratio, clumping_factor=clumping_factor, seed=seed, **kwargs)
        self.pool_mode = pool_mode
        self.cf = clumping_factor
        self.temperature = temperature
        self.eps = eps
        self.energy_power = energy_power

    def boltzmann(self, x):
        x = x - x.amax((-2, -1), keepdim=True)
        return torch.exp(x * self.temperature)

    def _get_pool_func(self, k):
        if self.pool_mode == "mean":
            return nn.AvgPool2d(k, stride=k)
        if self.pool_mode == "max":
            return nn.MaxPool2d(k, stride=k)
        if self.pool_mode == "min":
            return lambda x: -nn.MaxPool2d(k, stride=k)(-x)
        raise ValueError("pool_mode must be 'mean', 'max' or 'min', got %r" % (self.pool_mode,))

    def sample_mask_per_frame(self, video):
        energy = video.view(-1, 1, *video.shape[-2:])  # [_BT,1,H,W]
        H, W = energy.shape[-2:]
        assert (H % self.height == 0) and (W % self.width == 0)
        if (H != self.height) or (W != self.width):
            energy = self._get_pool_func(((H * self.cf) // self.height, (W * self.cf) // self.width))(energy)
        if self.temperature is not None:
            energy = self.boltzmann(energy)
        num_points = (self.num_patches_per_frame - self.num_masks_per_frame) // (self.cf ** 2)
        if self.randomize_num_visible:
            num_points = self.rng.randint(low=0, high=(num_points + 1))
        visible = sample_from_energy(torch.pow(energy, self.energy_power), binarize=True, num_points=max(num_points, 1), eps=self.eps,
                                     normalize=True) > 0.5
        if num_points == 0:
            visible = torch.zeros_like(visible)
        if self.cf > 1:
            visible = upsample_masks(visible, size=(self.height, self.width))
        return torch.logical_not(visible).flatten(1)  # [_BT,N]

    def forward(self, video, num_frames=None):
        device = video.device
        video = video.detach().cpu()  # the draws come from the global CPU generator, as in the reference on a CPU energy map
        if video.dim() == 4:
            video = video.unsqueeze(1)
        else:
            assert video.dim() == 5, video.shape
        B = video.size(0)
        masks = self.sample_mask_per_frame(video)
        masks = masks.view(B, -1, masks.shape[-1]).flatten(1)
        if B == 1 and not self.always_batch:
            masks = masks.squeeze(0)
        if self.visible_frames > 0:
            vis = torch.zeros((B, 1, self.height, self.width), dtype=torch.bool).view(masks.shape)
            masks = torch.cat(([vis] * self.visible_frames) + [masks], -1)
        return masks.to(device)


class RotatedTableEnergyMaskingGenerator(EnergySamplingMaskingGenerator):
    """The first `visible_frames` frames fully visible, the remaining one sampled from the energy (sampling.py:115-126)."""

    def __init__(self, input_size, mask_ratio, visible_frames=1, seed=0, *args, **kwargs):
        super().__init__((input_size[0] - visible_frames, *input_size[1:]), mask_ratio, seed, *args, visible_frames=visible_frames, **kwargs)
        self.visible_frames = visible_frames


# ---- cwm/models/sampling.py:128-286 ----------------------------------------------------------------------------------------
class FlowSampleFilter(nn.Module):
    """Reject flow samples in which nothing, or everything, moved (sampling.py:128-286):

    - patch_magnitude: the mean flow magnitude at the active patches is below `flow_magnitude_threshold`
    - flow_area: more than `flow_area_threshold` of the image moves faster than `flow_magnitude_threshold`
    - num_corners: at least `num_corners_threshold` corner pixels move faster than `flow_magnitude_threshold`

    `forward` runs on the device in two kernels' worth of passes (one read of the flows for the statistics, one write of the rejected
    samples); the per-method helpers are plain torch on the caller's device and are not on its path.  `last_stats` holds the [B,S]
    statistics and decisions of the last `forward`: patch_mag (fp32), area_count, corner_count (int32), reject (bool)."""

    ALL_FILTERS = ["patch_magnitude", "flow_area", "num_corners"]
    _METHOD_BITS = {"patch_magnitude": 1, "flow_area": 2, "num_corners": 4}  # CWM_FLOW_FILTER_* (include/cwm_hip.h)

    def __init__(self, filter_methods=ALL_FILTERS, flow_magnitude_threshold=5.0, flow_area_threshold=0.75, num_corners_threshold=2):
        super().__init__()
        self.filter_methods = filter_methods
        self.flow_magnitude_threshold = flow_magnitude_threshold
        self.flow_area_threshold = flow_area_threshold
        self.num_corners_threshold = num_corners_threshold
        self.last_stats = None

    def __repr__(self):
        return ("filtering by %s\nusing flow_magnitude_threshold %0.1f\n" + "using flow_area_threshold %0.2f\n" +
                "using num_corners_threshold %d") % (self.filter_methods, self.flow_magnitude_threshold, self.flow_area_threshold,
                                                     self.num_corners_threshold)

    def compute_flow_magnitude(self, flow_samples, active_patches=None):
        """flow_mag [B,H,W,S]; with active_patches [B,Np,S] also (flow_mag_down [B,S,hw], patch_flow_mag [B,S], active_second [B,S,hw])
        (sampling.py:163-205)."""
        flow_mag = flow_samples.norm(dim=1, p=2)
        if active_patches is None:
            return flow_mag
        B, _, H, W, num_samples = flow_samples.shape
        _, num_patches, _ = active_patches.shape
        assert active_patches.shape[-1] == num_samples, (active_patches.shape, num_samples)
        assert H == W, "the inference of patch size assumes H == W"
        h = w = int((num_patches / 2) ** 0.5)
        active_second = (1 - active_patches[:, (h * w):, :].float()).permute(0, 2, 1)
        flow_mag_down = F.interpolate(flow_mag.permute(0, 3, 1, 2), size=[h, w], mode="bilinear").flatten(2, 3)
        patch_flow_mag = (flow_mag_down * active_second).sum(dim=-1) / (active_second.sum(-1) + 1e-12)
        return flow_mag, flow_mag_down, patch_flow_mag, active_second

    def filter_by_patch_magnitude(self, patch_flow_mag):
        assert self.flow_magnitude_threshold is not None
        return patch_flow_mag < self.flow_magnitude_threshold

    def filter_by_flow_area(self, flow_mag):
        assert self.flow_magnitude_threshold is not None and self.flow_area_threshold is not None
        _, H, W, _ = flow_mag.shape
        flow_area = (flow_mag > self.flow_magnitude_threshold).flatten(1, 2).sum(1) / (H * W)
        return flow_area > self.flow_area_threshold

    def filter_by_num_corners(self, flow_mag):
        assert self.flow_magnitude_threshold is not None
        over = (flow_mag > self.flow_magnitude_threshold).float()
        num_corners = over[:, 0, 0] + over[:, 0, -1] + over[:, -1, 0] + over[:, -1, -1]
        return num_corners >= self.num_corners_threshold

    def _method_mask(self) -> int:
        bits = 0
        for method in self.filter_methods:
            if method not in self._METHOD_BITS:
                raise ValueError(f"Filter method must be one of {self.ALL_FILTERS}, but got {method}")
            bits |= self._METHOD_BITS[method]
        return bits

    def compute_stats(self, flow_samples, active_patches):
        """The statistics pass alone: `last_stats` of these flows (read once, not modified)."""
        methods = self._method_mask()
        _require_cuda(flow_samples, "FlowSampleFilter")
        flows, strides = _strides5(flow_samples)
        B, Cc, H, W, S = flows.shape
        if active_patches.dim() != 3 or active_patches.shape[0] != B or active_patches.shape[-1] != S:
            raise RuntimeError("expected active_patches [B=%d,Np,S=%d], got %s" % (B, S, tuple(active_patches.shape)))
        act = active_patches.to(device=flows.device)
        if act.dtype != torch.bool and act.dtype != torch.uint8:
            act = act != 0
        dev = flows.device
        stats = {"patch_mag": torch.empty((B, S), device=dev, dtype=torch.float32), "area_count": torch.empty((B, S), device=dev, dtype=torch.int32),
                 "corner_count": torch.empty((B, S), device=dev, dtype=torch.int32), "reject": torch.empty((B, S), device=dev, dtype=torch.bool)}
        with torch.cuda.device(dev):
            _lib.check(_lib.get_lib().cwm_flow_filter_stats(
                flows.data_ptr(), strides, B, Cc, H, W, S, act.data_ptr(), (C.c_int64 * 3)(*act.stride()), act.shape[1], methods,
                float(self.flow_magnitude_threshold), float(self.flow_area_threshold), float(self.num_corners_threshold), stats["patch_mag"].data_ptr(),
                stats["area_count"].data_ptr(), stats["corner_count"].data_ptr(), stats["reject"].data_ptr(), _lib.current_stream_handle(dev)))
        self.last_stats = stats
        return stats

    def forward(self, flow_samples, active_patches):
        """flow_samples [B,2,H,W,S] (any strides; zeroed IN PLACE where rejected), active_patches [B,Np,S] ->
        (the filtered samples, contiguous -- the input itself when it is contiguous --, the decisions expanded to [B,2,H,W,S] (a view of [B,1,1,1,S]))."""
        if flow_samples.is_cuda and flow_samples.dtype != torch.float32:
            raise RuntimeError("FlowSampleFilter zeroes the samples in place: expected float32 flows, got %s" % flow_samples.dtype)
        stats = self.compute_stats(flow_samples, active_patches)
        flows, strides = _strides5(flow_samples)
        B, Cc, H, W, S = flows.shape
        reject = stats["reject"]
        lib, stream = _lib.get_lib(), _lib.current_stream_handle(flows.device)
        with torch.cuda.device(flows.device):
            _lib.check(lib.cwm_flow_filter_apply(flows.data_ptr(), strides, B, Cc, H, W, S, reject.data_ptr(), stream))
            if flows.is_contiguous():
                out = flows
            elif _sample_outermost(flows):
                # the view `_batch_to_samples` hands over: one transposing pass (kept samples read once, zeros written for the others)
                out = torch.empty((B, Cc, H, W, S), device=flows.device, dtype=torch.float32)
                _lib.check(lib.cwm_flow_filter_pack(flows.data_ptr(), strides, B, Cc, H, W, S, reject.data_ptr(), out.data_ptr(), stream))
            else:
                out = flows.contiguous()
        return out, reject.view(B, 1, 1, 1, S).expand(B, Cc, H, W, S)
