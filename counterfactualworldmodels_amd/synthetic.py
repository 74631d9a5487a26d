"""Deterministic synthetic weights / frames / masks / prompts.

There are no checkpoints or datasets offline, so parity tests and `bench.py` run
on seeded synthetic data.  Everything is generated with numpy Philox streams
keyed by (seed, tensor name), so this container and the GPU box regenerate
bit-identical full-size tensors without shipping them.
"""
from __future__ import annotations

import functools
import zlib
from typing import Dict, Optional, Tuple

import numpy as np

from .config import VmaeConfig, state_dict_schema


def _rng(seed: int, name: str) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(key=[seed, zlib.crc32(name.encode())]))


def synthetic_tensor(name: str, shape: Tuple[int, ...], seed: int = 0) -> np.ndarray:
    """Xavier-uniform-like matrices (what the reference's `_init_weights` uses, vmae.py:100-107),
    but with small non-zero biases / LayerNorm affine jitter so every bias path is exercised."""
    g = _rng(seed, name)
    if name.endswith("norm.weight") or name.endswith("norm1.weight") or name.endswith("norm2.weight") or (
        "norm" in name and name.endswith(".weight")
    ):
        return (1.0 + 0.1 * (g.random(shape, dtype=np.float32) - 0.5)).astype(np.float32)
    if name.endswith("bias") or name.endswith("q_bias") or name.endswith("v_bias"):
        return (0.1 * (g.random(shape, dtype=np.float32) - 0.5)).astype(np.float32)
    if "token" in name:
        return (0.04 * (g.random(shape, dtype=np.float32) - 0.5)).astype(np.float32)
    if len(shape) >= 2:
        fan_out = shape[0]
        fan_in = int(np.prod(shape[1:]))
        a = float(np.sqrt(6.0 / (fan_in + fan_out)))
        return ((g.random(shape, dtype=np.float32) * 2.0 - 1.0) * a).astype(np.float32)
    return (0.1 * (g.random(shape, dtype=np.float32) - 0.5)).astype(np.float32)


def synthetic_state_dict(cfg: VmaeConfig, seed: int = 0, schema=None, sharp: bool = False) -> Dict[str, np.ndarray]:
    schema = schema if schema is not None else state_dict_schema(cfg)
    sd = {k: synthetic_tensor(k, shp, seed) for k, shp in schema.items()}
    return sharpen_state_dict(sd, seed) if sharp else sd


def sharpen_state_dict(sd: Dict[str, np.ndarray], seed: int = 0, qk_scale: float = 1.5, ln_range: Tuple[float, float] = (0.2, 3.0),
                       res_scale: float = 2.0) -> Dict[str, np.ndarray]:
    """Numerically hostile variant of a synthetic state dict (what trained, LayerNorm-heavy networks look like and the
    xavier-like generator does not): the q and k rows of every `attn.qkv.weight` x `qk_scale` (logits x qk_scale^2: sharp softmax),
    every LayerNorm weight ~ U(ln_range) (large dynamic range between channels), `proj` / `fc2` weights x `res_scale` (residual growth).

    The defaults are the sharpest setting at which the REFERENCE is still reproducible in fp32 (ViT-B/8: fp32 vs float64 evaluation of the
    same network 1.3e-5 max-abs; logits up to +-21, mean maximum attention weight 0.34 in the first block).  qk_scale 2 puts the reference's
    own fp32 rounding at 3.6e-4, qk_scale 4 makes the forward pass chaotic (fp32 vs float64: 6.8 max-abs on outputs of std 2): a 1e-3
    tolerance against an fp32 reference means nothing there (profiles/r3_hostile_scan.txt)."""
    out = {}
    for k, v in sd.items():
        v = v.copy()
        if k.endswith("attn.qkv.weight"):
            d = v.shape[0] // 3
            v[: 2 * d] *= qk_scale
        elif "norm" in k and k.endswith(".weight") and v.ndim == 1:
            v = (ln_range[0] + (ln_range[1] - ln_range[0]) * _rng(seed, "sharp." + k).random(v.shape, dtype=np.float32)).astype(np.float32)
        elif k.endswith("attn.proj.weight") or k.endswith("mlp.fc2.weight"):
            v *= res_scale
        out[k] = v
    return out


def synthetic_frames(batch: int, cfg: VmaeConfig, seed: int = 0) -> np.ndarray:
    """Wrapper-level input: float32 [B,T,C,H,W] in [0,1)."""
    g = np.random.Generator(np.random.PCG64(seed))
    return g.random((batch, cfg.num_frames, cfg.in_chans, cfg.img_size[0], cfg.img_size[1]), dtype=np.float32)


def synthetic_masks(batch: int, cfg: VmaeConfig, k_visible: int, seed: int = 0, clump: int = 1) -> np.ndarray:
    """bool [B,Nt]: frame 0 fully visible, frame 1 masked except `k_visible` patches per row
    (chosen as `k_visible/clump^2` clumps of clump x clump patches)."""
    g = np.random.Generator(np.random.PCG64(seed + 1))
    n = cfg.tokens_per_frame
    gh, gw = cfg.img_size[0] // cfg.patch, cfg.img_size[1] // cfg.patch
    mask = np.zeros((batch, cfg.num_frames, gh, gw), dtype=bool)
    mask[:, 1:] = True
    assert k_visible % (clump * clump) == 0
    n_clumps = k_visible // (clump * clump)
    ch, cw = gh // clump, gw // clump
    for b in range(batch):
        sel = g.permutation(ch * cw)[:n_clumps]
        for s in sel:
            i, j = divmod(int(s), cw)
            mask[b, -1, i * clump : (i + 1) * clump, j * clump : (j + 1) * clump] = False
    assert n * cfg.num_frames == mask[0].size
    return mask.reshape(batch, -1)


def synthetic_prompts(num: int, cfg: VmaeConfig, seed: int = 0, max_shift: int = 3) -> np.ndarray:
    """int32 [S,4] rows (active_h, active_w, dy, dx): one active patch and a non-zero shift in
    patch units, uniform in [-max_shift, max_shift]^2 \\ {0} (interface.py:370-377)."""
    g = np.random.Generator(np.random.PCG64(seed + 2))
    gh, gw = cfg.img_size[0] // cfg.patch, cfg.img_size[1] // cfg.patch
    out = np.zeros((num, 4), dtype=np.int32)
    for s in range(num):
        out[s, 0] = g.integers(gh)
        out[s, 1] = g.integers(gw)
        while True:
            dy, dx = g.integers(-max_shift, max_shift + 1, size=2)
            if dy != 0 or dx != 0:
                break
        out[s, 2], out[s, 3] = dy, dx
    return out


@functools.lru_cache(maxsize=None)
def _synthetic_flow_module():
    import torch

    class SyntheticFlow(torch.nn.Module):
        """Deterministic stand-in for RAFT with the multi-frame call contract of the reference
        (`raft/raft_model.py:276-300`): `flow_model(x[B,T,3,H,W] in [0,1], iters=..., backward=False)` -> [B,T-1,2,H,W] pixels.

        Every output depends on the frame content (a static movie gives a different flow from a moving one), x differs from y
        and forward differs from backward (not by a sign), and the magnitudes are several pixels, so the 2/W, 2/H flow scaling
        of the flow -> IMU input shows in the results.  It has no parameters."""

        def forward(self, x, iters=None, backward=False, **kwargs):
            a, b = x[:, :-1].float(), x[:, 1:].float()
            d = b - a
            if not backward:
                fx = 12.0 * d[:, :, 0] + 4.0 * a[:, :, 1] - 1.5
                fy = -9.0 * d[:, :, 2] + 6.0 * a[:, :, 0] * b[:, :, 1] - 2.0
            else:
                fx = -7.0 * d[:, :, 1] + 5.0 * b[:, :, 2] * b[:, :, 2] - 2.5
                fy = 10.0 * d[:, :, 0] - 3.0 * b[:, :, 0] + 1.0
            return torch.stack([fx, fy], 2)

    return SyntheticFlow


def SyntheticFlow():  # noqa: N802 -- a class factory, so that importing this module needs no torch
    return _synthetic_flow_module()()


@functools.lru_cache(maxsize=None)
def _synthetic_keypoints_module():
    import torch

    class SyntheticKeypoints(torch.nn.Module):
        """Deterministic, parameter-free stand-in for the keypoint RAFT (`load_raft_model(None, output_dim=1)`) with its multi-frame call
        contract: `keypoint_predictor(x[B,T,3,H,W] in [0,1])` -> [B,T-1,1,H,W] logits.  A function of the content of both frames of a pair,
        spread over several units so that `sigmoid(v) ** 8` is far from flat."""

        def forward(self, x, *args, **kwargs):
            if x.size(1) == 1:
                x = x.repeat(1, 2, 1, 1, 1)
            a, b = x[:, :-1].float(), x[:, 1:].float()
            v = 8.0 * (a[:, :, 0] - 0.5) + 5.0 * (b[:, :, 1] - a[:, :, 2]) + 0.5
            return v.unsqueeze(2)

    return SyntheticKeypoints


def SyntheticKeypoints():  # noqa: N802 -- a class factory, as SyntheticFlow
    return _synthetic_keypoints_module()()


RAFT_KEYPOINT_OUT_SCALE = 0.5  # on `output_block.2.weight`: see raft_state_dict


def raft_state_dict(seed: int = 0, output_dim=None) -> Dict[str, np.ndarray]:
    """Synthetic RAFT-large weights by key (`synthetic_tensor`), with batch-norm running variances 1 + 5|v|, `num_batches_tracked` 0 and the
    flow head's last convolution x 0.02: with plain xavier weights the flow grows by several pixels per iteration and after 24 iterations
    almost every correlation lookup falls outside the pyramid.  With `output_dim` the four `output_block` tensors follow (183 keys); the
    projection `output_block.2.weight` is scaled by RAFT_KEYPOINT_OUT_SCALE so that the keypoint map spans a few units either side of zero
    (measured on the reference: [-3.3, 7.6], std 2.4 at 224^2; unscaled, std 4.8 and most of `sigmoid(map) ** 8` saturated): the distribution
    made from it is neither flat nor a step."""
    from .config import raft_state_dict_schema

    out = {}
    for k, shp in raft_state_dict_schema(output_dim).items():
        if k.endswith("num_batches_tracked"):
            out[k] = np.zeros((), dtype=np.int64)
            continue
        v = synthetic_tensor(k, shp, seed)
        if k.endswith("running_var"):
            v = (1.0 + 5.0 * np.abs(v)).astype(np.float32)
        if k.startswith("update_block.flow_head.conv2."):
            v = (v * np.float32(0.02)).astype(np.float32)
        if k == "output_block.2.weight":
            v = (v * np.float32(RAFT_KEYPOINT_OUT_SCALE)).astype(np.float32)
        out[k] = v
    return out


def raft_frames(batch: int, height: int, width: int, seed: int = 0, shift: Tuple[int, int] = (3, 5), frames: int = 2) -> np.ndarray:
    """float32 [B,T,3,H,W] in [0,1): 5x5 box-filtered uniform noise; frame t is the crop of one noise field at t * shift = (dy, dx), so
    consecutive frames are related by a pure translation (RAFT finds a smooth flow of a few pixels)."""
    g = np.random.Generator(np.random.PCG64(seed))
    dy, dx = shift
    sy, sx = abs(dy) * (frames - 1), abs(dx) * (frames - 1)
    noise = g.random((batch, 3, height + 4 + sy, width + 4 + sx), dtype=np.float32).astype(np.float64)
    hh, ww = height + sy, width + sx
    box = np.zeros((batch, 3, hh, ww), dtype=np.float64)
    for i in range(5):
        for j in range(5):
            box += noise[:, :, i : i + hh, j : j + ww]
    box = (box / 25.0).astype(np.float32)
    y0, x0 = (sy if dy < 0 else 0), (sx if dx < 0 else 0)
    out = np.empty((batch, frames, 3, height, width), dtype=np.float32)
    for t in range(frames):
        y, x = y0 + t * dy, x0 + t * dx
        out[:, t] = box[:, :, y : y + height, x : x + width]
    return out


def blob_flow_samples(size: int, seed: int, blobs: np.ndarray, noise: float = 0.3, scaled_pixels=None, nan_pixels=None) -> np.ndarray:
    """float32 [B,2,H,W,S] flow samples for the flow-sample filter: uniform background noise in [-noise, noise) from PCG64(seed) plus, per
    (b, s), the blobs `blobs[b, s, k] = (cy, cx, r, ay, ax)` (r <= 0: unused): (ay, ax) / (1 + d^2 / r^2) added to (channel 1, channel 0).

    Only exactly rounded float32 operations are used (add, multiply, divide), so every host regenerates the same bits (`flow_checksum`).
    `scaled_pixels` [n,4] rows (b, s, y, x): both components multiplied by 1 + 1e-5 (a fixture's way of moving a magnitude off a threshold);
    `nan_pixels` [n,4]: both components NaN."""
    blobs = np.asarray(blobs, dtype=np.float32)
    B, S = blobs.shape[:2]
    g = np.random.Generator(np.random.PCG64(seed))
    two, one = np.float32(2.0), np.float32(1.0)
    out = (g.random((B, 2, size, size, S), dtype=np.float32) * two - one) * np.float32(noise)
    yy = np.arange(size, dtype=np.float32)[:, None]
    xx = np.arange(size, dtype=np.float32)[None, :]
    for b in range(B):
        for s in range(S):
            for cy, cx, r, ay, ax in blobs[b, s]:
                if r <= 0:
                    continue
                dy, dx = yy - cy, xx - cx
                fall = one / (one + (dy * dy + dx * dx) / (r * r))
                out[b, 0, :, :, s] += ax * fall
                out[b, 1, :, :, s] += ay * fall
    if scaled_pixels is not None:
        for b, s, y, x in np.asarray(scaled_pixels, dtype=np.int64).reshape(-1, 4):
            out[b, :, y, x, s] *= np.float32(1.0 + 1e-5)
    if nan_pixels is not None:
        for b, s, y, x in np.asarray(nan_pixels, dtype=np.int64).reshape(-1, 4):
            out[b, :, y, x, s] = np.nan
    return out


def flow_checksum(flows: np.ndarray) -> str:
    """sha256 of the float32 bytes of `flows` in C order."""
    import hashlib

    return hashlib.sha256(np.ascontiguousarray(flows, dtype=np.float32).tobytes()).hexdigest()


def sampler_energy(batch: int, side: int, seed: int, one_hot: bool = False) -> np.ndarray:
    """float32 [B,1,side,side] energy map for the patch samplers: uniform in [0,1), or all zero but one pixel per image."""
    g = np.random.Generator(np.random.PCG64(seed))
    if one_hot:
        e = np.zeros((batch, 1, side, side), dtype=np.float32)
        for b in range(batch):
            e[b, 0, g.integers(side), g.integers(side)] = 1.0
        return e
    return g.random((batch, 1, side, side), dtype=np.float32)
