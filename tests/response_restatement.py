"""float64 torch restatement of the response of a perturbation (`cwm_token_response`): the squared difference of two predictions of frame f, from their
predicted tokens and the mask they share.

    r[b][Y][X] = sum_c (y[b][row][k] - y_ref[b][row][k])^2     at the masked patches of frame f; 0 at its visible ones (both predictions copy the input there)
    map        = mean of r over each patch
    peak_index = torch.argmax over the H W pixels of the frame (the first maximum; a NaN is the maximum)
    peak       = r at that pixel;  mass = sum r;  centroid = sum r (Y, X) / mass, the peak position when mass == 0

Everything is computed in float64 from the float32 inputs, so the results are exact up to 2^-53 per operation.  What an fp32 implementation may differ by is
its own rounding.  Every sum here is a sum of NON-NEGATIVE terms, so the bounds below follow from operation counts alone, for any summation order and with or
without fused multiply-adds: a result that went through n roundings, each relative and at most EPS, is within gamma(n) = n EPS / (1 - n EPS) of its value
(Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1); a sum of k non-negative terms adds k - 1 roundings to the worst of its terms.
"""
import torch

EPS = 2.0 ** -24  # half an fp32 ulp, relative: the error of one fp32 operation


def gamma(n):
    return n * EPS / (1 - n * EPS)


def response(y, y_ref, mask, T, C, H, W, P, frame):
    """[B,H,W] float64.  y [B,Nm,P*P*C] (feature order ph, pw, c) at the masked tokens in ascending order; y_ref the same or [1,Nm,P*P*C]; mask [B,Nt]"""
    B = y.shape[0]
    gh, gw = H // P, W // P
    n = gh * gw
    mask = mask.reshape(B, T * n).bool()
    tok = torch.zeros((B, T * n, P * P * C), dtype=torch.float64)
    d = y.double() - y_ref.double().expand(B, -1, -1)
    tok[mask] = (d * d).reshape(-1, P * P * C)  # (NaN stays NaN)
    tok = tok[:, frame * n:(frame + 1) * n].reshape(B, gh, gw, P, P, C).sum(-1)  # a visible token keeps its 0
    return tok.permute(0, 1, 3, 2, 4).reshape(B, H, W)


def patch_map(r, P):
    B, H, W = r.shape
    return r.reshape(B, H // P, P, W // P, P).sum((2, 4)) / (P * P)


def statistics(r):
    """(peak_index [B] int64, stats [B,4] float64: peak, mass, centroid_y, centroid_x)"""
    B, H, W = r.shape
    flat = r.reshape(B, -1)
    idx = torch.argmax(flat, 1)
    peak = flat.gather(1, idx[:, None])[:, 0]
    mass = flat.sum(1)
    Y = torch.arange(H, dtype=torch.float64)[None, :, None]
    X = torch.arange(W, dtype=torch.float64)[None, None, :]
    py, px = (idx // W).double(), (idx % W).double()
    empty = mass == 0
    safe = torch.where(empty, torch.ones_like(mass), mass)
    cy = torch.where(empty, py, (r * Y).sum((1, 2)) / safe)
    cx = torch.where(empty, px, (r * X).sum((1, 2)) / safe)
    return idx, torch.stack([peak, mass, cy, cx], 1)


# ---- what fp32 may differ by, relative to the exact value ----------------------------------------------------------------------------------------------------
def pixel_bound(C):
    """r at one pixel: each of the C terms carries the rounding of its subtraction (twice, through the square) and of the square; C - 1 additions"""
    return gamma(C + 2)


def map_bound(C, P):
    """a patch value: C P^2 terms; the division by P^2 is exact"""
    return gamma(C * P * P + 2)


def mass_bound(C, H, W):
    return gamma(C + 2 + H * W - 1)


def centroid_bound(C, H, W):
    """sum r Y / sum r: the numerator has one more rounding per term (the product); a quotient of two quantities within gamma(a) and gamma(b) is within
    gamma(a + 2 b) of the exact quotient (Higham, Lemma 3.3), and the division rounds once"""
    a, b = C + 3 + H * W - 1, C + 2 + H * W - 1
    return gamma(a + 2 * b + 1)


def index_gap(r):
    """per row: the largest response minus the second largest.  An implementation whose pixel values are within `pixel_bound` of these must return THIS argmax
    whenever gap > 2 pixel_bound max(r): no other pixel can overtake the first."""
    top = torch.topk(r.reshape(r.shape[0], -1), 2, dim=1).values
    return top[:, 0] - top[:, 1], top[:, 0]
