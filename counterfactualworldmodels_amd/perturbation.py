"""Prompt perturbations.  `AddMarkers` (at the end of this file): the reference's marker counterfactuals, cwm/models/perturbation.py:329-476, plain torch.

`MultiShiftPatchesAndMask`: several groups of patches moved by separate pixel shifts in one prompt (reference:
cwm/models/perturbation.py:644-779, the generator's `multi_patch_shifter`, prediction.py:59-64).

Same constructor arguments and call signature as the reference class, `(x, mask_sequence, perturbation_points_sequence=None,
shift_sequence=None, frame=-1) -> (x_p, mask_ps)`, in the reference's conventions (masks: True = masked; points: True = this
patch is moved at step k).  The reference applies the K steps one after the other, each a pad / centre-crop / patchify / blend
of the whole frame; here all rows and all steps are ONE pair of HIP kernels (`cwm_multi_shift_prompts`, whose header comment
states the semantics) that find every output pixel by walking the steps backwards.  Frames and masks are bit-equal to the
reference's.  CUDA tensors only.

Two defects of the reference are not reproduced: its `_check_shapes` assigns to the read-only property `num_shifts`
(perturbation.py:668-682 against :171-175), so its `forward` raises as written; and `m_seq.expand(1, 1, num_shifts)` (:709)
fails for a [B,N] mask given with [B,N,K] points -- here that mask is the base mask of every step.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib

MAX_STEPS = 8  # kMultiShiftMaxSteps of the library


def multi_shift_rows(x, points, masks, shifts, patch, frame, fix_passive=False, samples_per_movie=1, frames=True, masks_out=True):
    """R = B * samples_per_movie prompt rows from one library call.  x [B,T,C,H,W] (CUDA); points [R,K,Nt] bool (True = moved at
    step k; step-major, the layout the kernels coalesce on); masks [R,K,Nt] / [R,1,Nt] / [R,Nt] bool base masks or None (the
    reference's call without points); shifts: integer array-like [R,K,2] of (sy, sx) pixels, on the host.  Row i reads movie
    i // samples_per_movie.  Returns (x_out [R,T,C,H,W] or None, mask_out [R,Nt] or None), masks not yet rectangularised."""
    assert frames or masks_out
    if not x.is_cuda:
        raise RuntimeError("counterfactual prompts are built on the GPU (no CPU fallback); got a %s tensor" % x.device)
    _lib.require_gpu()
    dev = x.device
    B, T, Cc, H, W = x.shape
    R, K, Nt = points.shape
    if R != B * samples_per_movie:
        raise ValueError("%d rows of points for %d movies x %d samples" % (R, B, samples_per_movie))
    table = np.ascontiguousarray(np.asarray(shifts, dtype=np.int64).reshape(R, K, 2))
    max_abs = int(np.abs(table).max()) if table.size else 0
    x = x.to(torch.float32).contiguous()
    points = points.to(device=dev, dtype=torch.bool).contiguous()
    mask_steps = 0
    if masks is not None:
        masks = masks.to(device=dev, dtype=torch.bool).reshape(R, -1, Nt).contiguous()
        mask_steps = masks.shape[1]
    shifts_dev = torch.from_numpy(table.astype(np.int32)).to(dev)
    x_out = torch.empty((R, T, Cc, H, W), device=dev, dtype=torch.float32) if frames else None
    mask_out = torch.empty((R, Nt), device=dev, dtype=torch.bool) if masks_out else None
    with torch.cuda.device(dev):
        _lib.check(_lib.get_lib().cwm_multi_shift_prompts(
            x.data_ptr(), B, T, Cc, H, W, int(patch), frame % T, samples_per_movie, K, int(bool(fix_passive)),
            points.data_ptr(), _lib.ptr(masks), mask_steps, shifts_dev.data_ptr(), min(max_abs, 2 ** 31 - 1),
            _lib.ptr(x_out), _lib.ptr(mask_out), _lib.current_stream_handle(dev)))
    return x_out, mask_out


def _stack_sequence(seq, what):
    """A list / tuple of [B,N] tensors or a [B,N] / [B,N,K] tensor -> [B,N,K]."""
    if isinstance(seq, (list, tuple)):
        assert all(m.dim() == 2 for m in seq), (what, seq[0].shape)
        return torch.stack(list(seq), -1)
    if seq.dim() == 2:
        return seq.unsqueeze(-1)
    assert seq.dim() == 3, (what, seq.shape)
    return seq


class MultiShiftPatchesAndMask(nn.Module):
    """Shift different patches by different amounts, in pixels (reference class: perturbation.py:644)."""

    def __init__(self, patch_size, max_shift_fraction=0.15, padding_mode="constant", allow_fractional_shifts=True, seed=0, **kwargs):
        super().__init__()
        if padding_mode != "constant" or not allow_fractional_shifts:
            raise NotImplementedError("MultiShiftPatchesAndMask: padding_mode='constant' with allow_fractional_shifts=True is what the "
                                      "generator builds (prediction.py:59-64) and the only mode provided")
        self.patch_size = tuple(patch_size) if isinstance(patch_size, (tuple, list)) else (1, patch_size, patch_size)
        self.max_shift_fraction = max_shift_fraction
        self.padding_mode = padding_mode
        self.allow_fractional_shifts = True
        # the reference's PatchPerturbation.__init__ (perturbation.py:26-28): a numpy stream of its own, and the GLOBAL torch generator seeded
        self.seed = seed
        self.rng = np.random.RandomState(seed=seed)
        self.torch_rng = torch.manual_seed(seed)
        self.image_size = None
        self.reset_shifts()

    # ---- the reference's bookkeeping (perturbation.py:165-175, 661-663) -----------------------------------------------------------
    def set_num_shifts(self, num_shifts=None):
        self._num_shifts = 1 if num_shifts is None else int(num_shifts)

    @property
    def num_shifts(self):
        return self._num_shifts

    def reset_shifts(self):
        self.shifts = None
        self.set_num_shifts(None)

    def get_random_shift(self):
        """A raw pixel shift of up to max_shift_fraction of the image per axis, redrawn while dy + dx == 0 (sic): the reference's
        `get_random_shift()` in fractional mode (perturbation.py:209-225)."""
        assert self.image_size is not None, "call the shifter (or set image_size) before drawing shifts"
        lim = [int(self.max_shift_fraction * s) for s in self.image_size]
        shift = (0, 0)
        while sum(shift) == 0:
            shift = (int(self.rng.randint(-lim[0], lim[0] + 1)), int(self.rng.randint(-lim[1], lim[1] + 1)))
        return shift

    def _preprocess_shifts_sequence(self, shifts_sequence) -> List[Tuple[int, int]]:
        """`num_shifts` (sy, sx) pairs from None (random), one pair, a list of pairs (one pair broadcasts) or a [2,K] / [2,1] array or
        tensor (perturbation.py:718-745)."""
        K = self.num_shifts
        if shifts_sequence is None:
            return [self.get_random_shift() for _ in range(K)]
        if hasattr(shifts_sequence, "shape"):
            arr = shifts_sequence.detach().cpu().numpy() if torch.is_tensor(shifts_sequence) else np.asarray(shifts_sequence)
            assert arr.ndim == 2, arr.shape
            assert arr.shape[0] == 2, arr.shape[0]
            assert arr.shape[1] in (K, 1), (arr.shape[1], K)
            seq = [(arr[0, s], arr[1, s]) for s in range(arr.shape[1])]
        else:
            seq = list(shifts_sequence)
            if not isinstance(seq[0], (list, tuple, np.ndarray)):
                seq = [seq]
        assert all(len(s) == 2 for s in seq), seq
        if len(seq) == 1:
            seq = seq * K
        assert len(seq) == K, (len(seq), K)
        for s in seq:
            if int(s[0]) != s[0] or int(s[1]) != s[1]:
                raise ValueError("shifts are whole pixels, got %s" % (s,))
        return [(int(s[0]), int(s[1])) for s in seq]

    def forward(self, x, mask_sequence, perturbation_points_sequence=None, shift_sequence=None, frame=-1, fix_passive=False):
        """x [B,T,C,H,W]; mask_sequence [B,Nt], [B,Nt,K] or K tensors [B,Nt] (True = masked); perturbation_points_sequence likewise
        (True = moved at step k; None: step k moves what mask k leaves visible, and there is no base mask); shift_sequence: see
        `_preprocess_shifts_sequence`.  Returns (x_p [B,T,C,H,W], mask_ps [B,Nt]).  The shifts used are left on `self.shifts`."""
        if mask_sequence is None:
            self.set_num_shifts(1)
            return (x, mask_sequence)
        if not x.is_cuda:
            raise RuntimeError("counterfactual prompts are built on the GPU (no CPU fallback); got a %s tensor" % x.device)
        assert x.dim() == 5, x.shape
        B, T, _, H, W = x.shape
        self.image_size = (H, W)
        P = self.patch_size[-1]
        if self.patch_size[-2] != P:
            raise NotImplementedError("MultiShiftPatchesAndMask: square patches only, got %s" % (self.patch_size,))
        m_seq = _stack_sequence(mask_sequence, "mask_sequence")
        if perturbation_points_sequence is None:
            points, masks = torch.logical_not(m_seq), None
        else:
            points = _stack_sequence(perturbation_points_sequence, "perturbation_points_sequence")
            assert points.dtype == torch.bool
            assert m_seq.size(-1) in (1, points.size(-1)) and m_seq.shape[:2] == points.shape[:2], (points.shape, m_seq.shape)
            masks = m_seq.permute(0, 2, 1)
        Nt = T * (H // P) * (W // P)
        if points.shape[1] != Nt:
            raise ValueError("masks of %d tokens for a movie of %d (T=%d, %dx%d, patch %d)" % (points.shape[1], Nt, T, H, W, P))
        self.set_num_shifts(points.size(-1))
        s_seq = self._preprocess_shifts_sequence(shift_sequence)
        self.shifts = list(s_seq)
        table = np.broadcast_to(np.asarray(s_seq, dtype=np.int64)[None], (B, len(s_seq), 2))
        x_p, mask_ps = multi_shift_rows(x, points.permute(0, 2, 1), masks, table, P, frame, fix_passive=fix_passive)
        return x_p, mask_ps.view(m_seq.shape[:2])


# ---- markers (reference: cwm/models/perturbation.py:329-476) ------------------------------------------------------------------------------------------------
class MarkerShape:
    """[ph, pw] float64 stencils of a marker: 'full', or 'cross' -- the rows and columns less than one pixel from the patch centre (perturbation.py:329-354)."""

    shapes = ["full", "cross"]

    def __init__(self, size):
        self.size = tuple(int(s) for s in size)

    def __call__(self, shape="full"):
        if shape not in self.shapes:
            raise NotImplementedError("%s not in set of shapes %s" % (shape, self.shapes))
        if shape == "full":
            return np.ones(self.size)
        rows, cols = (np.abs(np.arange(s) - (s - 1) / 2) < 1.0 for s in self.size)
        return (rows[:, None] | cols[None, :]).astype(np.float64)


def paint_markers(img, markers, b, t, h, w, patch_hw):
    """Marker k, [C,ph,pw], painted into patch (h[k], w[k]) of img[b[k], t[k]] IN PLACE, all K at once: where the marker's channel sum is > 0 the marker,
    elsewhere the image (perturbation.py:405-411, the same arithmetic: m * marker + (1 - m) * image).  The K patches must be different ones (markers that
    share a patch compose in order and are painted one call each).  img [R,T',C,H,W]; b, t, h, w: long tensors [K]."""
    ph, pw = patch_hw
    R, Tn, Cc, H, W = img.shape
    v = img.view(R, Tn, Cc, H // ph, ph, W // pw, pw)
    m = (markers.sum(1, True) > 0).to(img.dtype)
    v[b, t, :, h, :, w, :] = m * markers + (1 - m) * v[b, t, :, h, :, w, :]  # (the indexed dimensions come first: [K,C,ph,pw])
    return img


class AddMarkers(nn.Module):
    """Paint markers into patches of one frame and make those patches visible (reference class: perturbation.py:356-476, on `PatchPerturbation.forward`,
    :99-113): the prompt of "where does this point go".  Same constructor and call arguments, numpy draws in the same order (per marker: the shape, then
    the colour), frames and masks bit-equal to the reference's.  Plain torch on the tensors' device, CPU included.

    What the reference does, kept: a call with neither `patch_idx_list` nor `num_random_patches` marks nothing (its "everywhere visible" branch reads a
    mask it has just replaced by all-ones, :415, :424-427); a marked patch that was masked comes back visible (:455-456, :474); with `frame` an index, a
    4-entry patch index counts its frame from `frame` (0 is `frame`, :446).  What it does not do, provided: 2- and 3-entry indices, (h, w) and (b, h, w),
    which its painter accepts (:391-403) and its un-masking loop then fails on (:456) -- they mean row 0 / row b, frame 0 of the marked frames.  A mask
    whose grid is not the patch grid (its stride branch, :464-472) raises NotImplementedError."""

    def __init__(self, patch_size, marker_shapes=["full"], marker_color=[1, 0, 0], seed=0, **kwargs):
        super().__init__()
        self.patch_size = tuple(patch_size) if isinstance(patch_size, (tuple, list)) else (1, patch_size, patch_size)
        if len(self.patch_size) == 2:
            self.patch_size = (1,) + self.patch_size
        self.marker_shapes = marker_shapes
        self.marker_func = MarkerShape(size=self.patch_size[-2:])
        self.marker_color = marker_color
        # the reference's PatchPerturbation.__init__ (perturbation.py:26-28): a numpy stream of its own, and the GLOBAL torch generator seeded
        self.seed = seed
        self.rng = np.random.RandomState(seed=seed)
        self.torch_rng = torch.manual_seed(seed)

    def _get_marker_color(self, num_channels):
        if self.marker_color is None:
            return self.rng.random((3))
        if isinstance(self.marker_color[0], (list, tuple, np.ndarray)):
            return np.array((self.marker_color)[self.rng.choice(range(len(self.marker_color)))])
        assert len(self.marker_color) == num_channels
        return np.array(self.marker_color)

    def sample_marker(self, num_channels=3):
        """[C,ph,pw] float64: one draw of the shape, then the colour's (perturbation.py:384-389)"""
        shape = self.marker_func(self.rng.choice(self.marker_shapes))
        color = self._get_marker_color(num_channels)
        return shape[None] * color[:, None, None]

    def sample_markers(self, count, like, num_channels=3):
        """`count` markers in draw order as one tensor [count,C,ph,pw] of `like`'s dtype and device"""
        ph, pw = self.patch_size[-2:]
        host = np.stack([self.sample_marker(num_channels) for _ in range(count)]) if count else np.zeros((0, num_channels, ph, pw))
        return torch.tensor(host, device=like.device, dtype=like.dtype)

    def sample_random_patch(self, batch_size, frames, grid):
        """one (b, t, h, w) per row, three draws each (perturbation.py:79-91)"""
        out = []
        for b in range(batch_size):
            t = self.rng.choice(frames)
            out.append([b, int(t), int(self.rng.randint(grid[0])), int(self.rng.randint(grid[1]))])
        return out

    @staticmethod
    def _complete(idx):
        idx = [int(i) for i in (idx.tolist() if hasattr(idx, "tolist") else idx)]
        assert len(idx) in (2, 3, 4), idx
        return {2: [0, 0] + idx, 3: [idx[0], 0] + idx[1:], 4: idx}[len(idx)]

    def forward(self, x, mask=None, perturbation_points=None, patch_idx_list=None, frame=0, num_random_patches=0):
        if mask is None:
            raise ValueError("AddMarkers needs the mask the markers are added to")
        assert x.dim() == 5, x.shape
        B, T, Cc, H, W = x.shape
        pt, ph, pw = self.patch_size
        grid = (T // pt, H // ph, W // pw)
        mask = mask.clone()
        if perturbation_points is None:
            base = mask
        else:
            mask[perturbation_points] = 1
            base = torch.logical_not(perturbation_points)
        if int(np.prod(grid)) != int(np.prod(base.shape[1:])):
            raise NotImplementedError("AddMarkers: a mask of %d tokens per row for a patch grid of %s" % (int(np.prod(base.shape[1:])), grid))
        if frame is not None:
            frame = frame % T
        if patch_idx_list is None and not bool(num_random_patches):
            patches = []
        elif bool(num_random_patches):
            patches = []
            for _ in range(num_random_patches):
                patches.extend(self.sample_random_patch(B, [0] if frame is not None else list(range(T)), grid[-2:]))
        else:
            assert hasattr(patch_idx_list, "__len__")
            patches = patch_idx_list
            if not isinstance(patches[0], (list, tuple, torch.Tensor, np.ndarray)):
                patches = [patches]
        patches = [self._complete(p) for p in patches]
        x_marked = (x[:, frame].unsqueeze(1) if frame is not None else x).clone(memory_format=torch.contiguous_format)
        visible = torch.ones((B, 1 if frame is not None else grid[0]) + grid[1:], dtype=torch.bool, device=x.device)
        if patches:
            markers = self.sample_markers(len(patches), x, Cc)
            host = np.asarray(patches, dtype=np.int64)
            # rows and frames as indexing a tensor (negative counts from the end); patch rows and columns inside the grid, where the reference's painter works
            sizes = np.array([B, x_marked.shape[1], grid[1], grid[2]])
            low = np.array([-B, -x_marked.shape[1], 0, 0])
            if ((host < low) | (host >= sizes)).any():
                raise IndexError("patch index outside rows, frames and grid %s: %s" % (sizes.tolist(), host[((host < low) | (host >= sizes)).any(1)].tolist()))
            host = host % sizes
            # markers on different patches all at once; a patch marked again starts another pass, so that its markers compose in list order
            seen, passes = {}, []
            for k, key in enumerate(map(tuple, host.tolist())):
                n = seen.get(key, 0)
                seen[key] = n + 1
                if n == len(passes):
                    passes.append([])
                passes[n].append(k)
            idx = torch.from_numpy(host).to(x.device)
            for ks in passes:
                sel = idx[ks]
                paint_markers(x_marked, markers[ks], sel[:, 0], sel[:, 1], sel[:, 2], sel[:, 3], (ph, pw))
            visible[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = False
        if frame is not None:
            x_marked = torch.cat([x[:, :frame], x_marked, x[:, frame + 1:]], 1)
            full = torch.ones((B,) + grid, dtype=torch.bool, device=x.device)
            full[:, frame] = visible[:, 0]
            visible = full
        mask_marked = torch.minimum(visible.view(base.shape), base)
        if perturbation_points is not None:
            mask_marked = torch.minimum(mask, mask_marked)
        return x_marked, mask_marked
