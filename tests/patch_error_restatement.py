"""float64 torch restatement of the patch-error map and mean (`cwm_patch_error`; the reference's `get_error_on_target_region`, prediction.py:553-574, on
`_get_error`, :324-329, of `pred_patches_to_video`, :245-259), from the predicted tokens, the frames, the target, the mask, the region and the frame.

    map[b][t][i][j] = (1 / P^2) sum_{pixels of patch (i,j)} sum_c (pred_f - target_t)^2       f = frame, or t when frame is None
    mean[b]         = sum(map * region) / max(sum(region), 1)

Everything is computed in float64 from the float32 inputs, so the results are exact up to 2^-53: what an fp32 implementation may differ by is its own rounding,
`map_bound` and `mean_bound` below.
"""
import torch

EPS = 2.0 ** -24  # half an fp32 ulp, relative: the error of one fp32 operation


def unembed(y, x, mask, P):
    """`pred_patches_to_video` in float64: y [B,Nm,P*P*C] (feature order ph, pw, c) at the masked patches in ascending token order, x [B,T,C,H,W] elsewhere"""
    B, T, C, H, W = x.shape
    gh, gw = H // P, W // P
    patches = x.double().reshape(B, T, C, gh, P, gw, P).permute(0, 1, 3, 5, 4, 6, 2).reshape(B, T * gh * gw, P * P * C).clone()
    mask = mask.reshape(B, -1).bool()
    if y is not None and bool(mask.any()):
        patches[mask] = y.double().reshape(-1, P * P * C)
    return patches.reshape(B, T, gh, gw, P, P, C).permute(0, 1, 6, 2, 4, 3, 5).reshape(B, T, C, H, W)


def error_map(y, x, mask, P, target=None, frame=-1):
    """[B,T,h,w] float64"""
    B, T, C, H, W = x.shape
    pred = unembed(y, x, mask, P)
    if frame is not None:
        f = frame % T
        pred = pred[:, f:f + 1]
    tgt = (x if target is None else target).double()
    sq = ((pred - tgt) ** 2).sum(2)  # [B,T,H,W] (an integer frame broadcasts against every target frame)
    return sq.reshape(B, T, H // P, P, W // P, P).sum((3, 5)) / (P * P)


def error_mean(emap, region=None):
    """[B] float64; region [B,T,h,w] weights (None: ones)"""
    region = torch.ones_like(emap) if region is None else region.double()
    return (emap * region).sum((1, 2, 3)) / region.sum((1, 2, 3)).clamp(min=1)


def map_bound(C, P):
    """Relative error of a patch value computed in fp32, ANY summation order: the C P^2 terms are non-negative, so a sum of n of them is off by at most
    (n - 1) eps of its value; each term carries the rounding of its subtraction (twice, through the square) and of the square itself."""
    return (C * P * P + 2) * EPS


def mean_bound(C, P, n_el):
    """The same for the mean over n_el = T h w map values with non-negative weights: the product with the weight, the sum, the division"""
    return map_bound(C, P) + (n_el + 2) * EPS
