"""A plain-torch restatement of the reference's `FlowSampleFilter.forward` (cwm/models/sampling.py:163-286), statement for statement, on
whatever device and dtype the flows have.  It is the yardstick of `tools/flow_filter_step.py` and the comparison of the GPU smoke test;
`tests/test_motion_sampling_cpu.py` pins it to the goldens recorded from the reference itself."""
import torch
import torch.nn.functional as F

ALL_FILTERS = ("patch_magnitude", "flow_area", "num_corners")


def flow_filter_stats(flow_samples, active_patches, flow_magnitude_threshold=5.0):
    """patch_mag [B,S] (the flows' dtype), area_count [B,S] int64, corner_count [B,S] int64, flow_mag [B,H,W,S]."""
    B, _, H, W, num_samples = flow_samples.shape
    flow_mag = flow_samples.norm(dim=1, p=2)
    assert H == W
    h = w = int((active_patches.shape[1] / 2) ** 0.5)
    active_second = 1 - active_patches[:, (h * w):, :].to(flow_samples.dtype)
    active_second = active_second.permute(0, 2, 1)
    flow_mag_down = F.interpolate(flow_mag.permute(0, 3, 1, 2), size=[h, w], mode="bilinear")
    flow_mag_down = flow_mag_down.flatten(2, 3)
    patch_mag = (flow_mag_down * active_second).sum(dim=-1) / (active_second.sum(-1) + 1e-12)
    over = flow_mag > flow_magnitude_threshold
    area_count = over.flatten(1, 2).sum(1)
    corner_count = over[:, 0, 0].long() + over[:, 0, -1].long() + over[:, -1, 0].long() + over[:, -1, -1].long()
    return patch_mag, area_count, corner_count, flow_mag


def flow_filter_forward(flow_samples, active_patches, filter_methods=ALL_FILTERS, flow_magnitude_threshold=5.0, flow_area_threshold=0.75,
                        num_corners_threshold=2):
    """(flow_samples zeroed in place and made contiguous, the expanded mask [B,2,H,W,S], the [B,S] decisions)."""
    B, _, H, W, num_samples = flow_samples.shape
    patch_mag, area_count, corner_count, _ = flow_filter_stats(flow_samples, active_patches, flow_magnitude_threshold)
    filter_mask = torch.zeros(B, num_samples).to(flow_samples.device).bool()
    for method in filter_methods:
        if method == "patch_magnitude":
            _filter_mask = patch_mag < flow_magnitude_threshold
        elif method == "flow_area":
            _filter_mask = (area_count / (H * W)) > flow_area_threshold
        elif method == "num_corners":
            _filter_mask = corner_count.float() >= num_corners_threshold
        else:
            raise ValueError(f"Filter method must be one of {ALL_FILTERS}, but got {method}")
        filter_mask = filter_mask | _filter_mask
    decisions = filter_mask
    filter_mask = filter_mask.view(B, 1, 1, 1, num_samples).contiguous().expand_as(flow_samples)
    flow_samples[filter_mask] = 0.0
    return flow_samples.contiguous(), filter_mask, decisions
