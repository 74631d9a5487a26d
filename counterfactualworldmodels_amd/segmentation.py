"""`FlowGenerator`: batched motion counterfactuals over the HIP predictor (reference: cwm/models/segmentation.py:62-547,
760-963 -- `create_motion_counterfactuals`, `predict_counterfactual_videos_and_flows`, the IMU-conditioned override and the
flow-sample statistics).

The reference builds the B*S prompts in a per-sample Python loop and pushes them through `batch_predict_per_sample`, which
re-rectangularises and synchronises per chunk.  Here the whole prompt set is ONE batch description: every prompt's frames and
mask come out of one pair of HIP kernels (`cwm_shift_prompts`), the masks are rectangularised once (the reference's single
`mask_rectangularizer` call at segmentation.py:342: same global-RNG consumption, one host read-back), and the predictor then
runs over row ranges of that batch with the masked count already known -- no further host round trip until the result is
used.  The optical-flow model that follows in the reference is any module with the reference's `flow_model(video, backward=...)`
call signature (this package's `raft.RAFT`, or a stand-in).  `sample_counterfactual_motion_map` (segmentation.py:434-477) puts the
patch samplers and the flow-sample filter of `sampling.py` around that driver.
"""
from __future__ import annotations

import copy
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .perturbation import multi_shift_rows
from .prediction import PredictorBasedGenerator, _RectBatch
from .sampling import FlowSampleFilter, RotatedTableEnergyMaskingGenerator, boltzmann


def _shift_list(shifts, num: int) -> List[Tuple[int, int]]:
    """Normalise a shifts argument to `num` (dy, dx) pairs in patch units.  Accepted, as by the reference's
    `_preprocess_shifts_sequence` (perturbation.py:181-207): one pair, a sequence of pairs (length 1 = the same shift for
    every sample), or an array / tensor of shape [2, S] (S = 1 broadcasts)."""
    if hasattr(shifts, "shape"):
        arr = shifts.detach().cpu().numpy() if torch.is_tensor(shifts) else np.asarray(shifts)
        assert arr.ndim == 2 and arr.shape[0] == 2, arr.shape
        pairs = [(int(arr[0, s]), int(arr[1, s])) for s in range(arr.shape[1])]
    else:
        seq = list(shifts)
        if len(seq) == 2 and not isinstance(seq[0], (list, tuple, np.ndarray)):
            seq = [seq]
        assert all(len(p) == 2 for p in seq), seq
        pairs = [(int(p[0]), int(p[1])) for p in seq]
    if len(pairs) == 1:
        pairs = pairs * num
    assert len(pairs) == num, (len(pairs), num)
    return pairs


class FlowGenerator(PredictorBasedGenerator):
    """Counterfactual videos (and, with a flow model, flows) from moving patches; reference class segmentation.py:62."""

    # segmentation.py:29-41
    default_flow_filter_params = {"filter_methods": ["patch_magnitude", "flow_area", "num_corners"], "flow_magnitude_threshold": 5.0,
                                  "flow_area_threshold": 0.75, "num_corners_threshold": 2}
    default_patch_sampling_kwargs = {"energy_power": 1, "eps": 1e-16, "pool_mode": "mean", "resize": False}
    _DEFAULT_FILTER = object()  # (the reference's default argument is one filter instance shared by every generator; here each gets its own)

    def __init__(self, *args, flow_model=None, flow_model_load_path=None, raft_iters=None, flow_sample_filter=_DEFAULT_FILTER,
                 flow_sample_filter_params=None, patch_sampling_func=RotatedTableEnergyMaskingGenerator, patch_sampling_kwargs=None,
                 share_static_frame=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.flow_model = flow_model
        # the S counterfactuals of a movie begin with the same frame 0: let the flow model encode it once (`_counterfactual_flows`)
        self.share_static_frame = bool(share_static_frame)
        if flow_model is not None and flow_model_load_path is not None:
            self.load_predictor(flow_model_load_path, model=flow_model)
        self.raft_iters = raft_iters
        # the filter of the flow samples (segmentation.py:62-63)
        if flow_sample_filter is self._DEFAULT_FILTER:
            flow_sample_filter = FlowSampleFilter(**(flow_sample_filter_params or self.default_flow_filter_params))
        self.flow_sample_filter = flow_sample_filter
        # the patch sampler (segmentation.py:65-69); creating it draws `rng.randint(9999)`, as in the reference
        self._patch_sampling_func = patch_sampling_func
        self._patch_sampling_kwargs = copy.deepcopy(self.default_patch_sampling_kwargs)
        self._patch_sampling_kwargs.update(patch_sampling_kwargs or {})
        self.set_patch_sampler()

    # ---- patch sampling and the sample filter (segmentation.py:92-128) ------------------------------------------------------
    def set_flow_sample_filter(self, params=None):
        self.flow_sample_filter = None if params is None else FlowSampleFilter(**params)

    def set_patch_sampler(self, num_visible=1, mask_ratio=None, **kwargs):
        """(Re)create the sampler when there is none or keyword arguments are given -- each creation consumes one `self.rng.randint(9999)` --,
        then set its mask ratio or its number of visible (clumped) patches."""
        if (getattr(self, "patch_sampler", None) is None) or len(kwargs.keys()):
            _kwargs = copy.deepcopy(self._patch_sampling_kwargs)
            _kwargs.update(kwargs)
            try:
                mask_shape = self.mask_shape
            except Exception:
                mask_shape = self.predictor.mask_size
            self.patch_sampler = self._patch_sampling_func(input_size=mask_shape, mask_ratio=(mask_ratio or 0), seed=self.rng.randint(9999),
                                                           always_batch=True, **_kwargs)
        if mask_ratio is not None:
            self.patch_sampler.mask_ratio = mask_ratio
        elif num_visible is not None:
            self.patch_sampler.num_visible = num_visible * self.patch_sampler.clumping_factor ** 2

    def sample_patches_from_energy(self, energy=None, num_samples=10, num_visible=1, beta=None, **kwargs):
        """[B,Nt,S] bool masks (0 = visible) with `num_visible` (clumped) patches of the last frame drawn from `energy` [B,1,H,W] (None: uniform)."""
        self.set_patch_sampler(num_visible, **kwargs)
        if num_visible == 0:
            return torch.stack([self.get_zeros_mask() for _ in range(num_samples)], -1)
        if energy is None:
            assert self.x is not None
            energy = torch.ones_like(self.x[:, 0, 0:1])
        energy = boltzmann(energy, beta)
        torch.manual_seed(self.rng.randint(99999))
        return torch.stack([self.patch_sampler(energy) for _ in range(num_samples)], -1)

    def sample_counterfactual_motion_map(self, x, active_sampling_distribution=None, passive_sampling_distribution=None, active_patches=None,
                                         passive_patches=None, num_active_patches=1, num_passive_patches=0, num_samples=8, sample_batch_size=8,
                                         patch_sampling_kwargs={}, do_filter=True, **kwargs):
        """(flows [B,2,H,W,S], active_patches, passive_patches): S counterfactual flows of x, the samples in which nothing or everything
        moved zeroed by the `flow_sample_filter` (segmentation.py:434-477).  The flow model's output goes to the filter as the
        `_batch_to_samples` view; the only full-size write is the contiguous result."""
        self.set_input(x)

        def _sample_patches(dist, num_visible):
            return self.sample_patches_from_energy(energy=dist, num_samples=num_samples, num_visible=num_visible, **patch_sampling_kwargs)

        if active_patches is None:
            active_patches = _sample_patches(active_sampling_distribution, num_active_patches)
        if passive_patches is None:
            passive_patches = _sample_patches(passive_sampling_distribution, num_passive_patches)
        ys, flows = self.predict_counterfactual_videos_and_flows(x, active_patches=active_patches, passive_patches=passive_patches,
                                                                 num_samples=num_samples, sample_batch_size=sample_batch_size, fix_passive=True, **kwargs)
        flows = self._batch_to_samples(flows)
        if (self.flow_sample_filter is not None) and do_filter:
            flows, filter_mask = self.flow_sample_filter(flows, active_patches)
        return (flows, active_patches, passive_patches)

    # ---- flow model hook (segmentation.py:141-153) -------------------------------------------------------------------
    def set_raft_iters(self, iters=None):
        self.raft_iters = iters
        if hasattr(self.flow_model, "set_iters"):
            self.flow_model.set_iters(iters)

    def predict_flow(self, vid, backward=False, iters=None, **kwargs):
        """Keyword arguments go to the flow model: with the package's RAFT, `flow_init=` (a warm start for every pair) and `warm_start=True` (a movie's
        pairs as a chain, each started from the forward-interpolated flow of the pair before it; raft.RAFT._forward_multiframe)."""
        if self.flow_model is None:
            raise RuntimeError("this FlowGenerator has no flow_model (the reference plugs RAFT in here; any module called as "
                               "flow_model(video[B,T,C,H,W], backward=...) -> [B,T-1,2,H,W] works)")
        if iters is not None:
            self.set_raft_iters(iters)
        return self.flow_model(vid, backward=backward, **kwargs).to(vid)

    _FLOW_KEYS = ("iters", "raft_iters", "flow_init", "warm_start")  # the keywords of `predict_video_and_flow` that are the flow model's

    def predict_video_and_flow(self, x=None, mask=None, backward=False, propagate_error=False, **kwargs):
        """(x_pred [B,T-dt+2,C,H,W], f_pred) -- the prediction of the next frame and its flow (segmentation.py:170-197).  With dt = `sequence_length`, every
        window x[:, t:t+dt] of the movie (default: the generator's input and mask) gives frame 1 of `predict(window, mask, frame=1)`; x_pred is frame 0 followed
        by these.  propagate_error=True: the flow of x_pred as one movie; False: per window the flow of (x[t], x_pred[t+1], x[t+2:t+dt]), concatenated over
        time.  The keywords `_FLOW_KEYS` (iters or raft_iters, flow_init, warm_start) go to the flow model and every other one (x_context, mask_context,
        timestamps, ...) to `predict`: the reference hands all of them to both, so that its flow model is called with the predictor's x_context
        (reference defects not reproduced)."""
        x = self.x if x is None else x
        mask = self.mask if mask is None else mask
        flow_kw = {k: kwargs.pop(k) for k in self._FLOW_KEYS if k in kwargs}
        if "raft_iters" in flow_kw:
            flow_kw.setdefault("iters", flow_kw.pop("raft_iters"))
        T, dt = x.size(1), self.sequence_length
        x_pred = torch.cat([x[:, 0:1]] + [self.predict(x[:, t:t + dt], mask, frame=1, **kwargs).to(x) for t in range(T - dt + 1)], 1)
        if propagate_error:
            return x_pred, self.predict_flow(x_pred, backward, **flow_kw)
        f_pred = [self.predict_flow(torch.cat([x[:, t:t + 1], x_pred[:, t + 1:t + 2], x[:, t + 2:t + dt]], 1), backward, **flow_kw) for t in range(T - dt + 1)]
        return x_pred, (f_pred[0] if len(f_pred) == 1 else torch.cat(f_pred, 1))

    def _counterfactual_flows(self, y_mocos, mask, frame, backward=False, raft_iters=None):
        """The flows of the counterfactual videos y_mocos [(b s),T,C,H,W] predicted under `mask` [(b s),Nt] for the generator's input `self.x`.
        With `share_static_frame`, when the flow model has `flow_pairs` (raft.RAFT), the movie has two frames, frame 1 was predicted and no token of
        frame 0 is masked in any row -- only then is frame 0 of every video the input frame bit for bit -- the S videos of a movie go to the flow
        model as the pairs (input frame 0, frame 1 of sample s) with frame 0 expanded over the samples, so that its features are computed once per
        movie; the check of the masks is the call's one extra read-back, a single bool.  In every other case this is
        `predict_flow(y_mocos)`, as without the flag."""
        fm = self.flow_model
        x = self.x
        shared = (self.share_static_frame and fm is not None and hasattr(fm, "flow_pairs") and y_mocos.dim() == 5 and y_mocos.shape[1] == 2 and frame == 1
                  and x is not None and x.dim() == 5 and y_mocos.shape[0] % x.shape[0] == 0 and tuple(x.shape[2:]) == tuple(y_mocos.shape[2:]))
        if shared:
            R = y_mocos.shape[0]
            t = self.mask_shape[0]
            shared = t == 2 and not bool(mask.reshape(R, t, -1)[:, 0].any())
        if not shared:
            return self.predict_flow(y_mocos, backward=backward, iters=raft_iters)
        if raft_iters is not None:
            self.set_raft_iters(raft_iters)
        B, S = x.shape[0], y_mocos.shape[0] // x.shape[0]
        x0 = x[:, :1].to(device=y_mocos.device, dtype=torch.float32)  # (converted before it is expanded: an expanded view must keep its stride 0)
        second = y_mocos[:, 1].reshape(B, S, *y_mocos.shape[2:])
        flows = fm.flow_pairs(x0.expand(-1, S, -1, -1, -1), second, backward=backward, share=True)
        return flows.reshape(B * S, 1, *flows.shape[2:]).to(y_mocos)

    @staticmethod
    def batch_to_samples(flows, t=0, B=1):
        """[(b s),T,C,H,W] -> frame t as [b,C,H,W,s] (segmentation.py:129-132)."""
        assert flows.dim() == 5, flows.shape
        f = flows[:, t]
        return f.reshape(B, -1, *f.shape[1:]).movedim(1, -1)

    def _batch_to_samples(self, flows, t=0):
        assert self.x is not None
        if flows.dim() != 5:
            flows, t = flows.unsqueeze(1), 0
        return self.batch_to_samples(flows, t=t, B=self.x.size(0))

    # ---- prompt construction (segmentation.py:278-344) -----------------------------------------------------------------
    def _build_prompts(self, x, passive, active, pairs, frame, fix_passive) -> _RectBatch:
        """passive / active: [B,Nt,S] bool; pairs: S shifts (shared by all movies) or B*S shifts in '(b s)' order, None = S random
        ones.  Returns the '(b s)'-ordered rectangular batch of all B*S prompts."""
        B, N, S = passive.shape
        if x.dim() == 4:
            x = x[:, None]
        src = x[:, :1] if fix_passive else x
        T = 2 if fix_passive else x.shape[1]
        if fix_passive and T != 1:
            src = src.expand(-1, T, -1, -1, -1)  # every output frame of a static movie reads frame 0
        self.inp_shape = (B, T) + tuple(x.shape[2:])
        if pairs is None:
            pairs = [self._random_mask_shift() for _ in range(S)]
        assert len(pairs) in (S, B * S), (len(pairs), S, B)
        rows = list(pairs) * B if len(pairs) == S else list(pairs)
        table = torch.tensor(rows, dtype=torch.int32).reshape(B * S, 2)
        x_shift, mask_shift = self._shift_rows(src, passive.permute(0, 2, 1).reshape(B * S, N), active.permute(0, 2, 1).reshape(B * S, N),
                                               table, frame, fix_passive, samples_per_movie=S)
        for dy, dx in rows:
            self._record_shift(dy, dx)
        mask_shift, n_masked, n_vis_range = self._equalise(mask_shift)
        return _RectBatch(x_shift, mask_shift, n_masked, n_vis_range=n_vis_range)

    def create_motion_counterfactuals(self, x, masks, active_patches=None, shifts=None, frame=1, num_samples=None, fix_passive=True,
                                      reset_shifts=False):
        """Shift the active patches of `frame`, keep the passive ones (`masks`, 0 = visible) in place.  masks / active_patches:
        [B,Nt] (with num_samples) or [B,Nt,S]; shifts: see `_shift_list` (S pairs are used for every movie; B*S pairs address
        the '(b s)' rows one by one), None = random.  Returns (x_shift [B*S,T,C,H,W], mask_shift [B*S,Nt]), masks
        rectangularised once for all rows."""
        if getattr(self, "shifts", None) is None or reset_shifts:
            self.reset_shifts()
        if masks.dim() == 2:
            assert num_samples is not None, "Choose how many samples to shift with arg num_samples"
            masks = masks.unsqueeze(-1).expand(-1, -1, num_samples)
        S = masks.size(-1)
        if active_patches is None:
            active_patches = torch.ones_like(masks)
        elif active_patches.dim() == 2:
            active_patches = active_patches.unsqueeze(-1)
        assert active_patches.size(-1) in (1, S)
        active_patches = active_patches.expand(-1, -1, S)
        B = masks.size(0)
        if shifts is None:
            pairs = None
        elif not hasattr(shifts, "shape") and B > 1 and len(shifts) == B * S and isinstance(shifts[0], (list, tuple, np.ndarray)):
            pairs = _shift_list(shifts, B * S)
        else:
            pairs = _shift_list(shifts, S)
        batch = self._build_prompts(x, masks, active_patches, pairs, frame, fix_passive)
        return batch.x, batch.mask

    # ---- the batch driver (segmentation.py:346-432) ------------------------------------------------------------------
    def _conditioning_kwargs(self, x, kwargs):
        """Per-movie keyword tensors for the predictor (none for the plain VMAE; the IMU subclass adds its context stream)."""
        return kwargs

    @staticmethod
    def _two_frame_movie(x, fix_passive):
        if x.dim() == 3:
            return x[None, None].expand(-1, 2, -1, -1, -1), True
        if x.dim() == 4:
            return x[:, None].expand(-1, 2, -1, -1, -1), True
        assert x.dim() == 5, x.shape
        if x.size(1) == 1:
            x = x.expand(-1, 2, -1, -1, -1)
        return x[:, :2], fix_passive

    def _counterfactual_batch(self, x, active_patches, passive_patches, shifts, num_samples, fix_passive, frame, row_kwargs) -> _RectBatch:
        x, fix_passive = self._two_frame_movie(x, fix_passive)
        self.set_input(x)
        self.reset_shifts()
        passive = self.get_zeros_mask() if passive_patches is None else passive_patches
        passive = passive.unsqueeze(-1) if passive.dim() == 2 else passive
        active = active_patches.unsqueeze(-1) if active_patches.dim() == 2 else active_patches
        S = max(active.size(-1), passive.size(-1))
        if S == 1 and num_samples > 1:
            S = num_samples
        if shifts is None:
            pairs = [self._random_mask_shift() for _ in range(S)]
        else:
            n_given = shifts.shape[-1] if hasattr(shifts, "shape") else (1 if not isinstance(shifts[0], (list, tuple, np.ndarray)) else len(shifts))
            pairs = _shift_list(shifts, n_given)
        S = len(pairs)
        active = active.expand(-1, -1, S) if active.size(-1) == 1 else active
        passive = passive.expand(-1, -1, S) if passive.size(-1) == 1 else passive
        assert active.size(-1) == passive.size(-1) == S, (active.shape, passive.shape, S)
        batch = self._build_prompts(x, passive, active, pairs, frame, fix_passive)
        B = x.shape[0]
        for k, v in row_kwargs.items():  # per-movie tensors (the IMU stream) follow their movie's S prompts
            if torch.is_tensor(v) and v.shape[0] == B and B != batch.rows:
                v = self.sample_tile(v, S)
            batch.row_kwargs[k] = v
        return batch

    def predict_counterfactual_videos(self, x, active_patches, passive_patches=None, shifts=None, num_samples=8, sample_batch_size=8,
                                      fix_passive=True, frame=1, **kwargs):
        """y_mocos [B*S,T,C,H,W]: the predictor half of `predict_counterfactual_videos_and_flows`.  `sample_batch_size` rows go
        into one predictor call (None: all of them); the result does not depend on it."""
        batch = self._counterfactual_batch(x, active_patches, passive_patches, shifts, num_samples, fix_passive, frame,
                                           self._conditioning_kwargs(x, kwargs))
        y = self._run_rect_batch(batch, rows_per_call=sample_batch_size)
        self.reset_padding_masks()
        return y

    def predict_counterfactual_videos_and_flows(self, x, active_patches, passive_patches=None, shifts=None, num_samples=8,
                                                sample_batch_size=8, fix_passive=True, max_shift_fraction=None, frame=1, raft_iters=None,
                                                backward=False, **kwargs):
        """(y_mocos [B*S,T,C,H,W], flow_mocos [B*S,T-1,2,H,W]) for S motion counterfactuals per movie: active patches moved by
        the shifts, passive patches revealed in place (segmentation.py:346-432)."""
        if max_shift_fraction is not None and shifts is None:
            self.max_shift_fraction = max_shift_fraction
        batch = self._counterfactual_batch(x, active_patches, passive_patches, shifts, num_samples, fix_passive, frame,
                                           self._conditioning_kwargs(x, kwargs))
        y_mocos = self._run_rect_batch(batch, rows_per_call=sample_batch_size)
        self.reset_padding_masks()
        return y_mocos, self._counterfactual_flows(y_mocos, batch.mask, frame, backward, raft_iters)

    # ---- multi-shift counterfactuals: K patch groups per prompt, each moved by its own pixel shift (perturbation.py:644-779) ----------
    def _multi_shift_table(self, shifts, K):
        """[S',K,2] pixel shifts from K pairs (S' = 1: shared by the samples), S lists of K pairs, or a [2,K] / [2,K,S] array or tensor; each
        sample's sequence is normalised as the shifter normalises its `shift_sequence` (one pair broadcasts over the K steps)."""
        shifter = self.multi_patch_shifter
        shifter.set_num_shifts(K)
        if hasattr(shifts, "shape"):
            arr = shifts.detach().cpu().numpy() if torch.is_tensor(shifts) else np.asarray(shifts)
            assert arr.ndim in (2, 3) and arr.shape[0] == 2, arr.shape
            per_sample = [arr] if arr.ndim == 2 else [arr[..., s] for s in range(arr.shape[-1])]
        else:
            seq = list(shifts)
            nested = isinstance(seq[0], (list, tuple, np.ndarray)) and isinstance(seq[0][0], (list, tuple, np.ndarray))
            per_sample = seq if nested else [seq]
        return np.array([shifter._preprocess_shifts_sequence(s) for s in per_sample], dtype=np.int64).reshape(len(per_sample), K, 2)

    def _multi_shift_batch(self, x, active_patches, shifts, passive_patches, num_samples, fix_passive, frame, row_kwargs) -> _RectBatch:
        x, fix_passive = self._two_frame_movie(x, fix_passive)
        self.set_input(x)
        B = x.shape[0]
        assert active_patches.dim() in (3, 4), "active_patches is [B,Nt,K] or [B,Nt,K,S], got %s" % (tuple(active_patches.shape),)
        K = active_patches.size(2)
        passive = self.get_zeros_mask() if passive_patches is None else passive_patches
        # the number of samples: the patches' sample axis, else the shifts', else num_samples
        S = active_patches.size(3) if active_patches.dim() == 4 else (passive.size(-1) if passive.dim() == 3 else None)
        if shifts is None:  # K random shifts per sample from the shifter's own stream, sample by sample: what S calls of the reference's shifter draw
            S = num_samples if S is None else S
            shifter = self.multi_patch_shifter
            shifter.image_size, shifter.max_shift_fraction = tuple(x.shape[-2:]), self.max_shift_fraction
            shifter.set_num_shifts(K)
            table = np.array([shifter._preprocess_shifts_sequence(None) for _ in range(S)], dtype=np.int64).reshape(S, K, 2)
        else:
            table = self._multi_shift_table(shifts, K)
            if S is None:
                S = table.shape[0] if table.shape[0] > 1 else num_samples
            if table.shape[0] == 1:
                table = np.broadcast_to(table, (S, K, 2))
            assert table.shape[0] == S, (table.shape, S)
        Nt = active_patches.size(1)
        # '(b s)' rows, step-major tables: points [R,K,Nt] (moved = the 0s of active_patches), one base mask per row (the passive patches)
        points = torch.logical_not(active_patches.bool())
        points = points.permute(0, 3, 2, 1) if points.dim() == 4 else points.permute(0, 2, 1)[:, None].expand(-1, S, -1, -1)
        passive = passive.permute(0, 2, 1) if passive.dim() == 3 else passive[:, None].expand(-1, S, -1)
        x_shift, mask_shift = multi_shift_rows(x, points.reshape(B * S, K, Nt), passive.reshape(B * S, 1, Nt), np.broadcast_to(table[None], (B, S, K, 2)),
                                               self.patch_size[-1], frame, fix_passive=fix_passive, samples_per_movie=S)
        self.shifts = [np.array(table[s]) for _ in range(B) for s in range(S)]
        mask_shift, n_masked, n_vis_range = self._equalise(mask_shift)
        batch = _RectBatch(x_shift, mask_shift, n_masked, n_vis_range=n_vis_range)
        for k, v in row_kwargs.items():  # per-movie tensors (the IMU stream) follow their movie's S prompts
            if torch.is_tensor(v) and v.shape[0] == B and B != batch.rows:
                v = self.sample_tile(v, S)
            batch.row_kwargs[k] = v
        return batch

    def predict_multi_shift_counterfactual_videos(self, x, active_patches, shifts=None, passive_patches=None, num_samples=8, sample_batch_size=8,
                                                  fix_passive=True, frame=1, **kwargs):
        """y_mocos [B*S,T,C,H,W] for S counterfactuals per movie in each of which K groups of patches move by K separate PIXEL shifts, applied in
        order (`MultiShiftPatchesAndMask`).  active_patches [B,Nt,K] (shared by the samples) or [B,Nt,K,S], 0 = moved at step k; passive_patches
        [B,Nt] / [B,Nt,S], 0 = revealed in place (default: frame 0); shifts: see `_multi_shift_table`.  All B*S prompts come from one kernel
        call and are rectangularised once; `self.shifts` holds each row's [K,2] shifts."""
        batch = self._multi_shift_batch(x, active_patches, shifts, passive_patches, num_samples, fix_passive, frame, self._conditioning_kwargs(x, kwargs))
        y = self._run_rect_batch(batch, rows_per_call=sample_batch_size)
        self.reset_padding_masks()
        return y

    def predict_multi_shift_counterfactual_videos_and_flows(self, x, active_patches, shifts=None, passive_patches=None, num_samples=8,
                                                            sample_batch_size=8, fix_passive=True, frame=1, raft_iters=None, backward=False, **kwargs):
        """(y_mocos [B*S,T,C,H,W], flow_mocos [B*S,T-1,2,H,W]): `predict_multi_shift_counterfactual_videos`, then the flow model."""
        batch = self._multi_shift_batch(x, active_patches, shifts, passive_patches, num_samples, fix_passive, frame, self._conditioning_kwargs(x, kwargs))
        y_mocos = self._run_rect_batch(batch, rows_per_call=sample_batch_size)
        self.reset_padding_masks()
        return y_mocos, self._counterfactual_flows(y_mocos, batch.mask, frame, backward, raft_iters)

    # ---- flow from marker counterfactuals: no flow network (no counterpart in the reference; its `AddMarkers` is the prompt) ---------------------------
    @staticmethod
    def marker_displacements(patches_hw, responses, patch, use_centroid=False):
        """[K,2] float32 (dx, dy) -- RAFT's channel order -- from the centre of marked patch k, (h P + (P - 1) / 2, w P + (P - 1) / 2), to where its
        response peaks (`responses.peak_yx`) or has its centroid (`responses.centroid`)"""
        hw = np.asarray(patches_hw, dtype=np.float64).reshape(-1, 2)
        centre = hw * patch + (patch - 1) / 2.0
        to = np.asarray(responses.centroid if use_centroid else responses.peak_yx, dtype=np.float64)
        return np.stack([to[:, 1] - centre[:, 1], to[:, 0] - centre[:, 0]], 1).astype(np.float32)

    def predict_perturbation_flow(self, x, points=None, grid_stride=None, mask=None, use_centroid=False, min_mass=0., **kw):
        """Displacements read out of the predictor itself: a marker is painted into a frame-0 patch of movie x [1,T,C,H,W], and where the prediction of
        the last frame changes most is where that patch went (`predict_marker_responses`, whose keywords `kw` are passed on: marker, sample_batch_size,
        frame).  points: K patches (h, w) -> displacements [K,2] as (dx, dy) in pixels, from the patch centre to the peak of the response, or to its
        centroid.  grid_stride s instead: every s-th patch in both directions -> (flow [2, h // s, w // s], valid [h // s, w // s] = mass > min_mass):
        a response of no weight says nothing about where its patch went.  Tensors on x's device."""
        if (points is None) == (grid_stride is None):
            raise ValueError("predict_perturbation_flow: give the patches as `points` or a `grid_stride`, not both")
        P = self.patch_size[-1]
        h, w = x.shape[-2] // P, x.shape[-1] // P
        if grid_stride is not None:
            s = int(grid_stride)
            hh, ww = h // s, w // s
            if s < 1 or hh < 1 or ww < 1:
                raise ValueError("grid_stride = %s for a grid of %d x %d patches" % (grid_stride, h, w))
            hw = np.stack(np.meshgrid(np.arange(hh) * s, np.arange(ww) * s, indexing="ij"), -1).reshape(-1, 2)
        else:
            hw = np.asarray([[int(i) for i in (p.tolist() if hasattr(p, "tolist") else p)] for p in points], dtype=np.int64).reshape(-1, 2)
        res = self.predict_marker_responses(x, hw.tolist(), mask=mask, **kw)
        flow = torch.from_numpy(self.marker_displacements(hw, res, P, use_centroid)).to(x.device)
        if grid_stride is None:
            return flow
        valid = torch.from_numpy(res.mass > min_mass).to(x.device)
        return flow.view(hh, ww, 2).permute(2, 0, 1).contiguous(), valid.view(hh, ww)

    # ---- Spelke-object segmentation (the reference's README names the use and lists the algorithm as "coming soon"): segment_step.py, csrc/segment.hip ----
    _SEGMENT_KEYS = ("min_seed_mag", "abs_thresh", "rel_thresh", "vote_frac", "cos_min", "inside_frac", "ring_radius")

    def segment_step(self, flows, seeds, *, min_seed_mag, abs_thresh, rel_thresh=0.5, vote_frac=0.5, dirs=None, cos_min=0.0, k_active=0, k_passive=0,
                     inside_frac=1.0, ring_radius=1, keys=None, shape=None):
        """From S counterfactual flows [B,2,H,W,S] and a seed pixel (y, x) per row to the connected region that moves with the seed: the pixels whose flow
        magnitude reaches max(abs_thresh, rel_thresh * the seed patch's mean magnitude) (and, with `dirs` [S,2] (dy, dx), points within acos(cos_min) of the
        sample's direction) in at least vote_frac of the samples in which the seed patch itself moved by min_seed_mag, cut down to the 4-connected part that
        hangs on the seed's patch.  Returns a `SegmentStepResult` (segment, votes, cover, stats, seed_ref and, with k_active > 0, the active / passive masks
        and picks of the next round: the seed's patch and the k_active - 1 first patches covered to `inside_frac`, the k_passive first untouched patches within
        `ring_radius` of a touched one; `keys` [B,2,n] rank them, default index order).  Device tensors take one library call (cwm_segment_step; the
        `_batch_to_samples` view without a copy, nothing read back), CPU tensors the same definition in torch.  flows=None with shape=(B, H, W) is the init
        step: an empty segment, the seed's patch alone active."""
        from . import segment_step as SS

        return SS.segment_step(flows, seeds, self.patch_size[-1], min_seed_mag=min_seed_mag, abs_thresh=abs_thresh, rel_thresh=rel_thresh, vote_frac=vote_frac,
                               dirs=dirs, cos_min=cos_min, k_active=k_active, k_passive=k_passive, inside_frac=inside_frac, ring_radius=ring_radius, keys=keys,
                               shape=shape)

    def segment_spelke_object(self, x, seeds, num_iters=3, num_samples=8, shift=1, k_active=4, k_passive=4, sample=False, generator=None,
                              sample_batch_size=None, return_trace=False, **kwargs):
        """The Spelke object under a seed pixel of every movie of x [B,T,C,H,W], seeds [B,2] (y, x): move the seed's patch in S = num_samples directions, segment
        what moves with it, then `num_iters - 1` more times move k_active patches inside the segment and pin k_passive just outside it, and segment again.
        The directions are `segment_step.directions(S, shift)`: the 8 compass shifts of `shift` patches in the order E, S, W, N, SE, SW, NW, NE, cycled to S.
        Every iteration is one `predict_counterfactual_videos_and_flows` (fix_passive=True, the masks expanded over the samples) and one `segment_step` on the
        `_batch_to_samples` view with `dirs` = the shifts in pixels; iteration 0 takes its masks from the init step.  sample=True ranks the picks by keys
        drawn per iteration with torch.rand((B,2,n), generator=generator) on x's device instead of by index.  The thresholds of `segment_step` (default:
        min_seed_mag = abs_thresh = 1 pixel) are taken from the keywords, the rest goes to the counterfactual driver (raft_iters, timestamps, ...).  Seeds,
        masks and picks stay on x's device: the loop reads nothing back beyond what the counterfactual driver does.
        Returns (segment [B,H,W] bool, vote fraction [B,H,W] = votes / max(n_valid, 1)) of the last iteration and, with return_trace, a list of each
        iteration's (SegmentStepResult, active [B,Nt], passive [B,Nt]) -- the masks that iteration's counterfactuals were made with."""
        from . import segment_step as SS

        if int(k_active) < 1 or int(num_iters) < 1 or int(num_samples) < 1:
            raise ValueError("segment_spelke_object: k_active, num_iters and num_samples must be at least 1")
        step_kw = {"min_seed_mag": 1.0, "abs_thresh": 1.0}
        step_kw.update({k: kwargs.pop(k) for k in self._SEGMENT_KEYS if k in kwargs})
        movie, _ = self._two_frame_movie(x, True)
        B, (H, W) = movie.shape[0], movie.shape[-2:]
        P, S, dev = self.patch_size[-1], int(num_samples), movie.device
        n = (H // P) * (W // P)
        seeds = torch.as_tensor(seeds).to(device=dev, dtype=torch.int32).reshape(B, 2)
        shifts = SS.directions(S, shift)
        dirs = torch.tensor([(dy * P, dx * P) for dy, dx in shifts], dtype=torch.float32).to(dev)
        res = self.segment_step(None, seeds, k_active=k_active, k_passive=k_passive, shape=(B, H, W), **step_kw)
        active, passive = res.active, res.passive
        trace = []
        # the counterfactual driver rectangularises its masks on torch's global CPU generator; the caller's stream of draws is put back as it was
        with torch.random.fork_rng(devices=[]):
            for _ in range(int(num_iters)):
                _, flows = self.predict_counterfactual_videos_and_flows(x, active.unsqueeze(-1).expand(-1, -1, S), passive.unsqueeze(-1).expand(-1, -1, S),
                                                                        shifts=shifts, num_samples=S, sample_batch_size=sample_batch_size, fix_passive=True, **kwargs)
                keys = torch.rand((B, 2, n), generator=generator, device=dev) if sample else None
                res = self.segment_step(self._batch_to_samples(flows), seeds, dirs=dirs, k_active=k_active, k_passive=k_passive, keys=keys, **step_kw)
                trace.append((res, active, passive))
                active, passive = res.active, res.passive
        frac = res.votes.float() / res.stats[:, 0].clamp(min=1).float()[:, None, None]
        return (res.segment, frac, trace) if return_trace else (res.segment, frac)

    # ---- scene segmentation: many seeded segments merged into one label map (segment_merge.py, csrc/segment_merge.hip) ----
    def segment_merge(self, segments, scores=None, *, min_area=1, max_area=0, iou_thresh=0.5, contain_thresh=0.6, absorb=True, want_inter=False):
        """K candidate segments per row [B,K,H,W] (nonzero = in; a slice of a larger buffer is read in place) and their scores [B,K] (None: index order) to one
        label map: candidates outside min_area .. max_area pixels (0: no upper bound) are dropped; the others are walked from the highest score down, and one
        whose intersection with an already-kept candidate exceeds iou_thresh of their union or contain_thresh of the smaller of the two is absorbed by the first
        such one, else kept as the next label.  Pixels go to the lowest label that holds them; absorb=True paints the absorbed candidates' pixels with their
        absorber's label.  Returns a `SegmentMergeResult` (labels, owner, area, label_area, inter with want_inter, cover per patch, stats).  Device tensors take
        one library call (cwm_segment_merge, nothing read back), CPU tensors the same definition in torch."""
        from . import segment_merge as SM

        return SM.segment_merge(segments, scores, self.patch_size[-1], min_area=min_area, max_area=max_area, iou_thresh=iou_thresh, contain_thresh=contain_thresh,
                                absorb=absorb, want_inter=want_inter)

    def select_seeds(self, map, k=8, **kw):
        """At most k well-spaced seed pixels [B,k,2] per row of a score map -- [B,H,W] pixels or [B,gh,gw] cells of this generator's patch grid: the strongest
        first, or with `e` an exponential race, under non-maximum suppression of `radius` cells (`seed_select.select_seeds` has the keywords).  Returns a
        `SeedSelection`.  Device tensors take one library call (cwm_seed_select, nothing read back), CPU tensors the same definition in torch."""
        from . import seed_select as SS

        return SS.select_seeds(map, k, self.patch_size[-1], **kw)

    def segment_scene(self, x, seeds=None, num_seeds=8, num_rounds=1, seed_distribution=None, generator=None, score="votes", seed_batch_size=None, free_below=None,
                      min_area=None, max_area_frac=0.5, iou_thresh=0.5, contain_thresh=0.6, absorb=True, seed_mode="sample", seed_radius=0, seed_rel_thresh=0.,
                      **kwargs):
        """The Spelke objects of every movie of x [B,T,C,H,W] as one label map: `num_rounds` rounds of `num_seeds` seeds, each seed run through
        `segment_spelke_object` (x repeated over the round's seeds, in chunks of `seed_batch_size` rows; **kwargs pass through: num_iters, num_samples, the
        thresholds, raft_iters, ...), every round written into one [B, num_rounds num_seeds, H, W] buffer (at most 64 candidates) and one `segment_merge` over all
        candidates so far after every round, the strided slice read in place.  score="votes" ranks a candidate by the mean vote fraction inside its segment,
        (frac * segment).sum / area.clamp(min=1); score="area" by its area.  min_area defaults to one patch, max_area is max_area_frac of the image (a segment
        larger than that is what camera motion gives).
        Seeds: round 0 takes `seeds` [B,num_seeds,2] (y, x) when given.  Every other round draws cells of the patch grid -- round 0 among all cells, round r > 0
        among those the merge leaves uncovered (cover == 0, or cover < free_below) -- without replacement and in proportion to `seed_distribution` ([B,H,W],
        averaged to patches, or [B,gh,gw]; None: uniform) by the exponential race of `frontier_unmask(sample=True)`: key = p / e, e from `generator`, in the order
        of `masking.select_reveal`.  A seed is the centre pixel of its cell; a slot that finds no cell is a dead row: seed (-1, -1), an all-zero candidate, never
        valid.  seed_distribution may also be "keypoints" (`predict_keypoints_distribution` of the movie; needs a keypoint_predictor) or a callable
        f(movie [B,T,C,H,W]) -> [B,H,W]; a movability map is passed as a tensor, `M(x)[:, 0]` of a `MovabilityPredictor` M.
        seed_mode="sample" with seed_radius=0 is the draw just described.  With seed_radius > 0 the same exponential draw runs through `select_seeds`: picks of
        a round keep more than seed_radius cells (Chebyshev) from each other and from every seed of the earlier rounds.  seed_mode="peaks" draws nothing: the
        seeds are the strongest local maxima of the map among the free cells (`select_seeds(peaks_only=True)`, in round 0 too unless `seeds` is given), at
        least seed_rel_thresh of the row's maximum, spaced and kept off earlier seeds in the same way; on a [B,H,W] map a seed is the pixel where its cell
        peaks, not the cell's centre.
        Everything stays on x's device and the loop reads nothing back beyond what the counterfactual driver does; it runs inside
        torch.random.fork_rng(devices=[]), so the caller's global CPU stream of draws is left as it was.  Returns a `SceneSegmentation` (labels [B,H,W] uint8,
        num_labels [B], seeds, segments [B,K,H,W] bool, scores, owner, label_area, cover, stats)."""
        from . import segment_merge as SM

        return SM.segment_scene(self, x, seeds=seeds, num_seeds=num_seeds, num_rounds=num_rounds, seed_distribution=seed_distribution, generator=generator, score=score,
                                seed_batch_size=seed_batch_size, free_below=free_below, min_area=min_area, max_area_frac=max_area_frac, iou_thresh=iou_thresh,
                                contain_thresh=contain_thresh, absorb=absorb, seed_mode=seed_mode, seed_radius=seed_radius, seed_rel_thresh=seed_rel_thresh, **kwargs)

    # ---- scene segments through a movie: label maps linked frame to frame by the backward flow (segment_track.py, csrc/segment_track.hip) ----
    def track_step(self, state, cur_labels, flow=None, **kw):
        """One frame of tracking: `state` (a `segment_track.TrackState`, or None for the first frame: no previous frame, every label is born), this frame's label
        map [B,H,W] uint8 as `segment_scene` returns it (None: the frame is carried by the flow alone) and the flow [B,2,H,W] from this frame to the previous
        one (`predict_flow(backward=True)` of the pair; None: zero motion).  The previous track map is warped onto this frame, overlaps are counted, tracks and
        labels are linked one to one (intersection above iou_thresh of the union, the larger overlap first), unlinked tracks coast on the flow for up to
        max_age frames (carry=True) or end, unlinked labels of at least min_area pixels are born into free slots under new ids.  Keywords: iou_thresh=0.3,
        min_inter=1, min_area=1, max_age=2, carry=True, want_table, want_warped.  Returns a `TrackStepResult` (state, area, bbox, moments, slot_of_cur,
        linked_cur, stats).  Device tensors take one library call (cwm_segment_track, nothing read back), CPU tensors the same definition in torch."""
        from . import segment_track as ST

        return ST.track_step(state, cur_labels, flow, **kw)

    def track_scene(self, x, segment_every=1, flow_kwargs=None, iou_thresh=0.3, min_inter=1, min_area=1, max_age=2, carry=True, return_segmentations=False,
                    occlusion=False, occ_alpha=0.01, occ_beta=0.5, motion=False, motion_kwargs=None, points=None, point_kwargs=None, **segment_scene_kwargs):
        """The Spelke objects of a movie x [B,T,C,H,W] with identities that persist over time.  The movie's backward flows come from ONE call,
        `predict_flow(x, backward=True, **flow_kwargs)` (so `warm_start=True` and the shared encoders of the package's RAFT apply).  Frames t <= T-2 with
        t % segment_every == 0 are segmented by `segment_scene(x[:, t:t+2], **segment_scene_kwargs)`, in ascending t on the caller's generator; every other
        frame, the last one included, has no segmentation and is carried by the flow.  Frame by frame `track_step` links the label maps: frame 0 has no
        previous frame, so every label is born.  ValueError when max_age < segment_every, or carry is off with segment_every > 1: tracks would die between
        segmentations.  occlusion=True makes one more call, `predict_flow(x, **flow_kwargs)`, for the forward flows, and every step warps along the backward
        flow masked by the forward-backward check (`flow_consistency.check`, occ_alpha and occ_beta): the strip an object uncovers warps nothing in and is 0
        in a carried frame.  motion=True (needs occlusion=True; no further flow call) also fills `motion`, `motion_counts` and `occluders` of the result with ONE
        `object_motion.measure` call over the T-1 pairs (keywords: motion_kwargs): how every slot moves to the next frame and who hides whom.  points [B,K,2] (x, y)
        (needs occlusion=True; no further flow call) also fills `points` of the result with ONE `point_track.track` call on the flows, slot maps and -- with
        motion=True -- models the call already has (keywords: point_kwargs: start, alpha, beta, max_coast): where each point is in every frame and when it
        is hidden.  Nothing is read
        back beyond what `segment_scene` does.  Returns a `TrackedScene` (labels [B,T,H,W] uint8 slots 1 .. 64; track_id, age,
        area [B,T,64]; bbox, moments, stats; with return_segmentations the per-frame `SceneSegmentation` objects, None for a carried frame)."""
        from . import segment_track as ST

        return ST.track_scene(self, x, segment_every=segment_every, flow_kwargs=flow_kwargs, iou_thresh=iou_thresh, min_inter=min_inter, min_area=min_area,
                              max_age=max_age, carry=carry, return_segmentations=return_segmentations, occlusion=occlusion, occ_alpha=occ_alpha,
                              occ_beta=occ_beta, motion=motion, motion_kwargs=motion_kwargs, points=points, point_kwargs=point_kwargs, **segment_scene_kwargs)

    # ---- where points go through a movie, and when they are hidden (point_track.py, csrc/point_track.hip) ----
    def track_points(self, x, points, start=None, scene=None, flows=None, alpha=0.01, beta=0.5, max_coast=8, **flow_kwargs):
        """`point_track.track` on a movie x [B,T,C,H,W]: points [B,K,2] (x, y) in pixels, each followed from frame `start` ([B,K] int; default 0) to the last
        frame along the forward flows, believed only where the forward-backward test (alpha, beta) holds.  flows: a given (fwd, bwd) pair, both [B,T-1,2,H,W] in
        pair order as `predict_flow_and_occlusion` returns them; None makes one `predict_flow(x, **flow_kwargs)` call per direction, as that method does.
        scene: a `TrackedScene` of the same movie (`track_scene`): its `labels` tell when a point stands on another object than the one it started on -- it is
        then hidden (state 1) and coasts on its object's motion model `scene.motion` (from `track_scene(motion=True)`; None: on its last believed flow
        vector) for up to max_coast frames, and is picked up again when it re-emerges.  Returns `PointTracks` (xy [B,T,K,2], state and under [B,T,K], owner
        [B,K]; state 0 visible, 1 hidden, 2 left the frame, 3 lost, 255 not started).  Device tensors take one library call (cwm_point_track: one kernel
        launch for the whole movie, nothing read back), CPU tensors the same definition in torch."""
        from . import point_track as PT

        if flows is None:
            if x.dim() != 5 or x.shape[1] < 2:
                raise ValueError("track_points: x must be a movie [B,T,C,H,W] of at least two frames, got %s" % (tuple(x.shape),))
            fwd = self.predict_flow(x, **flow_kwargs)
            bwd = self.predict_flow(x, backward=True, **flow_kwargs).flip(1)
        else:
            fwd, bwd = flows
        labels, model = (None, None) if scene is None else (scene.labels, scene.motion)
        return PT.track(fwd, points.to(fwd.device), bwd=bwd, labels=labels, model=model, start=start, alpha=alpha, beta=beta, max_coast=max_coast)

    # ---- how every slot moves and who hides whom (object_motion.py, csrc/object_motion.hip) ----
    def object_motion(self, labels, flow, code=None, other=None, **kw):
        """`object_motion.measure`: per slot of `labels` ([B,H,W] or [B,T,H,W] uint8, as `segment_scene` and `track_scene` return them) the pixel counts by
        class, the sums and the model of a least-squares affine fit to `flow` (from that frame to the other one, on its own grid) -- translation, rotation,
        looming; slot 0 is the camera's own motion --, and with `code` (the codes of `flow_consistency.check` for this flow) and `other` (the slot map of the
        other frame) the table of who was hidden behind whom, which `object_motion.occlusion_order` turns into a depth order.  Keywords: min_pixels=1,
        min_affine=16, min_det=1.0.  Returns an `ObjectMotion` (sums, counts, model, occluders).  Device tensors take one library call (cwm_object_motion,
        nothing read back), CPU tensors the same definition in torch."""
        from . import object_motion as OM

        return OM.measure(labels, flow, code=code, other=other, **kw)

    # ---- which objects move when one is pushed (object_response.py, csrc/object_response.hip) ----
    def object_interactions(self, x, labels, slots=None, num_slots=8, num_samples=8, shift=1, k_active=4, k_passive=4, ring_radius=1, sample=False, generator=None,
                            slot_batch_size=None, sample_batch_size=None, min_mag=1.0, self_frac=0.5, move_frac=0.5, **kwargs):
        """Push every slot of a slot map and see which other slots move: x [B,T,C,H,W], labels [B,H,W] uint8 as `segment_scene` / `track_scene` give them,
        slots [K] or [B,K] (default 1 .. num_slots: a fixed count, so nothing is read back to learn how many labels exist).  Per (scene, slot) the k_active
        cells of the patch grid with the most pixels of the slot are moved (sample=True: picked on torch.rand keys from `generator` among the cells the slot
        touches) and the first k_passive cells that hold no pixel of any slot within `ring_radius` of it are pinned -- a neighbouring object is never pinned, it
        must stay free to respond; a slot without a pixel is a dead row.  The rows go through `predict_counterfactual_videos_and_flows` (S = num_samples shifts
        `segment_step.directions(S, shift)`, fix_passive=True, **kwargs pass through: raft_iters, ...), the movie repeated over `slot_batch_size` slots per call
        (None: all K), and the `_batch_to_samples` view of each call goes into ONE `object_response.measure` with dirs = the shifts in pixels (thresholds:
        min_mag, self_frac, move_frac).  Returns an `ObjectInteractions`: tab, valid, agg, coupling, stats [B,K,..], slots, the masks active / passive
        [B,K,2n], and moves, mutual, carries, tested of `object_response.relations` at its defaults -- `object_response.groups(mutual)` and `merge_labels`
        repair a map that split one body into several slots.  Everything stays on x's device, nothing is read back beyond what the counterfactual driver does,
        and the loop runs inside torch.random.fork_rng(devices=[]): the caller's global CPU stream of draws is left as it was."""
        from . import object_response as OR

        return OR.object_interactions(self, x, labels, slots=slots, num_slots=num_slots, num_samples=num_samples, shift=shift, k_active=k_active, k_passive=k_passive,
                                      ring_radius=ring_radius, sample=sample, generator=generator, slot_batch_size=slot_batch_size,
                                      sample_batch_size=sample_batch_size, min_mag=min_mag, self_frac=self_frac, move_frac=move_frac, **kwargs)

    # ---- what the scene shows when the viewer moves: ego-motion counterfactuals and their parallax (parallax.py, csrc/parallax.hip) ----
    def ego_motion_flows(self, x, head_motions=None, shifts=None, num_samples=8, anchors=None, num_anchors=9, shift=2, mask=None, sample_batch_size=None, **kwargs):
        """S flow samples of every movie of x [B,T,C,H,W] under S motions of the VIEWER: (flows [B,2,H,W,S], dirs int32 [S,2] (dy, dx) in pixels, or None).
        With `head_motions` ([S,C,L], shared by the movies, or [B,S,C,L], in the predictor's layout; IMU-conditioned generators only) sample s is one row of
        `predict_imu_video_and_flow` with head motion s, `sample_batch_size` rows per call (None: all B S), every movie under one mask (`mask` [B,Nt], default
        one `generate_mask` draw); dirs is None, because the image motion a head motion causes is not known in advance -- `parallax.measure` then measures every
        sample against its own mean flow.  Otherwise the anchored pan: `anchors` ([B,n] patch indices of frame 1; default `num_anchors` cells on an evenly
        spaced lattice of the patch grid, `parallax.lattice_anchors`) are moved together by shift s of `shifts` (S pairs (dy, dx) in patches; default
        `segment_step.directions(num_samples, shift)`) in ONE `predict_counterfactual_videos_and_flows` (fix_passive=True; `mask`: its passive patches, default
        none; **kwargs pass through: raft_iters, head_motion, ...), and dirs is the shifts in pixels.  The flows are the `_batch_to_samples` view of the flow
        model's output.  Runs inside torch.random.fork_rng(devices=[]): the caller's global CPU stream of draws is left as it was; x is not modified.  Given
        anchors are checked against the grid (one read-back when they are a device tensor)."""
        from . import parallax as PX

        return PX.ego_motion_flows(self, x, head_motions=head_motions, shifts=shifts, num_samples=num_samples, anchors=anchors, num_anchors=num_anchors, shift=shift,
                                   mask=mask, sample_batch_size=sample_batch_size, **kwargs)

    def parallax(self, x, labels=None, min_pixels=1, min_ref=0.25, min_samples=None, want_spread=True, want_off=True, order_min_pixels=16, **kwargs):
        """Relative depth from motion parallax: `ego_motion_flows(x, **kwargs)` followed by ONE `parallax.measure` on its view (thresholds: min_pixels, min_ref,
        min_samples).  labels [B,H,W] uint8 as `segment_scene` / `track_scene` give them: the reference motion of a head-motion sample is then the mean flow of
        slot 0, the background (ref_slot=0), and the per-slot histogram and table are filled.  Returns a `parallax.Parallax` (par, spread, off, cnt, ref, hist,
        slot_tab, dirs) with nearer [B,65,65] and rank [B,65] of `parallax.depth_order(slot_tab, order_min_pixels)` attached (None without labels).  A pure
        rotation of the viewer gives a flat map.  Nothing is read back beyond what the counterfactual driver does."""
        from . import parallax as PX

        return PX.parallax(self, x, labels=labels, min_pixels=min_pixels, min_ref=min_ref, min_samples=min_samples, want_spread=want_spread, want_off=want_off,
                           order_min_pixels=order_min_pixels, **kwargs)

    # ---- whether a flow vector can be believed: the forward-backward check (flow_consistency.py, csrc/flow_consistency.hip) ----
    def predict_flow_and_occlusion(self, x, alpha=0.01, beta=0.5, **flow_kwargs):
        """The forward and backward flows of a movie x [B,T,C,H,W] -- one `predict_flow` call each -- and where they cannot be believed.  Returns
        (fwd [B,T-1,2,H,W]: pair t from frame t to frame t+1 on frame t's grid; bwd [B,T-1,2,H,W] in PAIR order: pair t from frame t+1 to frame t on frame
        t+1's grid (a flipped copy of what `predict_flow(backward=True)` stores); occ_fwd, occ_bwd bool [B,T-1,H,W]: the round trip fails or leaves the frame;
        the `FlowConsistency` of ONE `flow_consistency.check(fwd, bwd, both=True, want_res=True, want_masked=True)` call: index 0 forward, 1 backward)."""
        from . import flow_consistency as FC

        if x.dim() != 5 or x.shape[1] < 2:
            raise ValueError("predict_flow_and_occlusion: x must be a movie [B,T,C,H,W] of at least two frames, got %s" % (tuple(x.shape),))
        fwd = self.predict_flow(x, **flow_kwargs)
        bwd = self.predict_flow(x, backward=True, **flow_kwargs).flip(1)
        fc = FC.check(fwd, bwd, alpha=alpha, beta=beta, both=True, want_res=True, want_masked=True)
        return fwd, bwd, fc.code[0] != 0, fc.code[1] != 0, fc

    # ---- statistics over the flow samples (segmentation.py:250-276, 479-547): device kernels, see flowstats.py ----------
    def compute_flow_samples_magnitude(self, flows, normalize=True, dim=-4, eps=1e-2):
        from . import flowstats

        return flowstats.compute_flow_samples_magnitude(flows, normalize=normalize, dim=dim, eps=eps)

    def compute_mean_motion_map(self, flows, normalize_per_sample=False, normalize=True, dim=-4, eps=1e-2):
        from . import flowstats

        return flowstats.compute_mean_motion_map(flows, normalize_per_sample=normalize_per_sample, normalize=normalize, dim=dim, eps=eps)

    @staticmethod
    def compute_flow_corrs(flow_samples, *args, **kwargs):
        from . import flowstats

        return flowstats.compute_flow_corrs(flow_samples, *args, **kwargs)


class ImuGenerator(FlowGenerator):
    """The part of the reference's `ImuGenerator` (segmentation.py:549-754) that the IMU-conditioned driver and the UI use, around
    a conjoined predictor with an IMU context stream (the flow -> IMU head-motion predictor): an all-visible default mask
    generator over the predictor's `mask_size`, `_preprocess`, `num_head_tokens`, `reshape_input` / `reshape_output` and
    `_is_padded`.  Prediction from dataset dicts (`predict_imu`, and the `forward` that is it) is not provided; the forward of the IMU-CONDITIONED model,
    `predict_imu_video_and_flow`, is `ImuConditionedFlowGenerator`'s."""

    def __init__(self, *args, head_mask_generator=None, head_mask_ratio=0, always_use_predicted=False, require_none_missing=False, **kwargs):
        super().__init__(*args, **kwargs)
        assert hasattr(self.predictor, "context_stream")
        self.num_head_tokens = self.predictor.context_stream.encoder.num_tokens
        if self.mask_generator is None:
            from .masking import MaskingGenerator

            self.mask_generator = MaskingGenerator(input_size=self.predictor.mask_size, mask_ratio=0, always_batch=True, create_on_cpu=False)
        self.head_mask_generator = head_mask_generator
        self.head_mask_ratio = head_mask_ratio
        self._always_use_predicted = always_use_predicted
        self._require_none_missing = require_none_missing
        self.missing_imu = None

    @property
    def _is_padded(self):
        return hasattr(self.predictor.context_stream, "padding_mask")

    def reshape_input(self, x, tubelet_size=None):
        """[B,C,(T pt)] -> [B,T,(pt C)] (segmentation.py:640-643)."""
        pt = tubelet_size or self.predictor.context_stream.patch_size[0]
        B, Cc, L = x.shape
        return x.reshape(B, Cc, L // pt, pt).permute(0, 2, 3, 1).reshape(B, L // pt, pt * Cc)

    def reshape_output(self, y, tubelet_size=None):
        """[B,T,(pt C)] -> [B,C,(T pt)] (segmentation.py:645-649)."""
        pt = tubelet_size or self.predictor.context_stream.patch_size[0]
        B, T, F = y.shape
        Cc = F // pt
        return y.reshape(B, T, pt, Cc).permute(0, 3, 1, 2).reshape(B, Cc, T * pt)


class ImuConditionedFlowGenerator(FlowGenerator):
    """The IMU-conditioned variant (segmentation.py:760-963) for a conjoined RGB+IMU predictor.  The head motion is either an
    input (`head_motion` [B,6,400] in the predictor's layout) or, with a `head_motion_predictor` (the flow -> IMU model
    `imu400_8x8patch_2frames_1tube_flowbackrgb01`, which needs a flow model: the generator's `flow_model` is handed to it), estimated
    from the video: `static_head_motion=True` (the default) -> `get_static_imu`, False -> `predict_imu_from_video` (:834-880).  It is
    forwarded exactly as the reference forwards it: as `x_context`, with an all-visible (or, with mask_head_motion, all-masked)
    `mask_context`, tiled over every movie's prompts.  `predict_imu_video_and_flow` (:885-929, and `forward`, :966) asks the plain question -- the next frame
    and its flow under a given head motion --, and `ego_motion_flows` / `parallax` ask it for S head motions, one per row, and read the answers out as motion
    parallax (parallax.py)."""

    def __init__(self, *args, head_motion_predictor=None, head_motion_load_path=None, head_motion_generator=ImuGenerator,
                 head_motion_kwargs=None, head_motion_mask_generator=None, **kwargs):
        super().__init__(*args, **kwargs)
        if head_motion_predictor is None:
            return  # no `head_motion_generator` attribute: head_motion must be passed (interface.py's hasattr guard)
        hk = dict(head_motion_kwargs) if head_motion_kwargs is not None else {"head_mask_ratio": 1}
        hk.setdefault("imagenet_normalize_inputs", self.imagenet_normalize_inputs)
        hk.setdefault("temporal_dim", self.predictor.t_dim)
        hk["predictor_load_path"] = head_motion_load_path
        if not isinstance(head_motion_predictor, torch.nn.Module):
            head_motion_predictor = head_motion_predictor()
        if getattr(head_motion_predictor, "flow_model", "absent") is None and self.flow_model is not None:
            head_motion_predictor.set_flow_model(self.flow_model)
        self.head_motion_generator = head_motion_generator(predictor=head_motion_predictor, mask_generator=head_motion_mask_generator,
                                                           flow_model=self.flow_model, **hk)

    def get_fake_head_motion(self, x):
        """An all-zero, entirely masked IMU: what the flow -> IMU model is given to predict the head motion (segmentation.py:818-832)."""
        B = x.size(0)
        h = torch.zeros((B, self.head_tubelet_size * self.num_head_tokens, self.head_motion_channels), device=x.device, dtype=x.dtype)
        h_mask = torch.ones((B, self.num_head_tokens), device=x.device, dtype=torch.bool)
        if self.head_motion_generator.t_dim == 2:
            h = h.transpose(1, 2)
        return h, h_mask

    def predict_imu_from_video(self, x, timestamps=None):
        """[B,25,96]: the head motion the flow -> IMU model predicts from frames 0 and 1 of x [B,T,C,H,W] (segmentation.py:834-870)."""
        if not hasattr(self, "head_motion_generator"):
            raise RuntimeError("this generator has no head_motion_predictor: pass head_motion= to the counterfactual calls")
        G = self.head_motion_generator
        fake_imu, imu_mask = self.get_fake_head_motion(x)
        mask = G.mask_generator(x).to(x.device)
        return G.predictor(G._preprocess(x), mask=mask, timestamps=timestamps, x_context=fake_imu, mask_context=imu_mask, output_main=False,
                           output_context=True)

    def get_static_imu(self, x=None, timestamps=None):
        """The head motion of a static movie: frame 0 repeated (segmentation.py:873-877)."""
        x = self.x if x is None else x
        return self.predict_imu_from_video(x[:, 0:1].expand(-1, x.size(1), -1, -1, -1).contiguous(), timestamps=timestamps)

    def _head_model(self):
        """The model that defines the head-motion layout: the head-motion predictor when there is one (segmentation.py:799-809), else the
        conditioned predictor."""
        G = getattr(self, "head_motion_generator", None)
        return G.predictor if G is not None else self.predictor

    @property
    def num_head_tokens(self):
        return self._head_model().context_stream.encoder.num_tokens

    @property
    def head_tubelet_size(self):
        return self._head_model().context_stream.patch_size[0]

    @property
    def head_motion_channels(self):
        return getattr(self._head_model().get_context_input, "num_channels", 6)

    def get_zeros_imu(self, x=None):
        x = self.x if x is None else x
        return torch.zeros((x.shape[0], self.head_motion_channels, self.head_tubelet_size * self.num_head_tokens), device=x.device, dtype=x.dtype)

    def predict_imu_video_and_flow(self, x, mask=None, timestamps=None, head_motion=None, mask_head_motion=False, static_head_motion=False, return_flow=True,
                                   return_head_motion=False, **kwargs):
        """The next frame and its flow under a GIVEN head motion (segmentation.py:885-929): (y, flow) of `predict_video_and_flow(x, mask, x_context=the head
        motion, mask_context=all visible, or with mask_head_motion all masked)`.  mask None: one `generate_mask` draw.  The head motion is, in the reference's
        order of precedence, `head_motion` ([B,C,L] in the predictor's layout, forwarded as it is, as the counterfactual calls take it), else with
        static_head_motion `get_static_imu()`, else `predict_imu_from_video(x)`; the two estimates are the head-motion predictor's output and go through its
        generator's `reshape_output`, as in `_conditioning_kwargs`.  return_head_motion=True returns that head motion -- as given, or as estimated ([B,T,F], before
        the reshape) -- and predicts nothing.  return_flow=False (unused in the reference) skips the flow model: (y, None).  **kwargs: see
        `predict_video_and_flow`."""
        self.set_input(x)
        self.mask = self.generate_mask(x) if mask is None else mask
        given = head_motion is not None
        if given:
            h = head_motion
        elif static_head_motion:
            h = self.get_static_imu()
        else:
            h = self.predict_imu_from_video(x, timestamps=timestamps)
        if return_head_motion:
            return h
        h_mask = torch.zeros(h.size(0), self.num_head_tokens, dtype=torch.bool, device=h.device)
        if mask_head_motion:
            h_mask = ~h_mask
        kw = dict(kwargs, x_context=h if given else self.head_motion_generator.reshape_output(h), mask_context=h_mask)
        if timestamps is not None:
            kw["timestamps"] = timestamps
        if return_flow:
            y, flow = self.predict_video_and_flow(x, mask=self.mask, **kw)
        else:
            for k in self._FLOW_KEYS:
                kw.pop(k, None)
            T, dt = x.size(1), self.sequence_length
            y, flow = torch.cat([x[:, 0:1]] + [self.predict(x[:, t:t + dt], self.mask, frame=1, **kw).to(x) for t in range(T - dt + 1)], 1), None
        self.reset_padding_masks()
        return y, flow

    def forward(self, *args, **kwargs):
        """segmentation.py:966"""
        return self.predict_imu_video_and_flow(*args, **kwargs)

    def _conditioning_kwargs(self, x, kwargs):
        """segmentation.py:931-963: `head_motion` -> x_context, an all-visible (mask_head_motion: all-masked) mask_context."""
        kw = dict(kwargs)
        head_motion = kw.pop("head_motion", None)
        mask_head_motion = kw.pop("mask_head_motion", False)
        static_head_motion = kw.pop("static_head_motion", True)
        kw.pop("timestamps", None)
        if head_motion is None and hasattr(self, "head_motion_generator"):  # predict_imu_video_and_flow, segmentation.py:884-910, 931-963
            movie, _ = self._two_frame_movie(x, True)
            self.set_input(movie)
            if self.mask_generator is not None:
                self.generate_mask(movie)  # unused, as in the reference: drawn for its place in the global RNG sequence (:895-898)
            h = self.get_static_imu(movie) if static_head_motion else self.predict_imu_from_video(movie)
            head_motion = self.head_motion_generator.reshape_output(h)
        if head_motion is None:
            raise RuntimeError("pass head_motion [B,%d,%d], or build the generator with head_motion_predictor= (the flow->IMU model "
                               "conjoined_vmae.imu400_8x8patch_2frames_1tube_flowbackrgb01) to estimate it from the video"
                               % (self.head_motion_channels, self.head_tubelet_size * self.num_head_tokens))
        h_mask = torch.zeros(head_motion.shape[0], self.num_head_tokens, dtype=torch.bool, device=head_motion.device)
        if mask_head_motion:
            h_mask = ~h_mask
        kw.update(x_context=head_motion, mask_context=h_mask, n_vis_context=0 if mask_head_motion else self.num_head_tokens)
        return kw
