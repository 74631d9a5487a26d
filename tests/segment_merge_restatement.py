"""A NumPy restatement of `cwm_segment_merge` (the definition: include/cwm_hip.h, csrc/segment_merge.hip) in plain loops, the two threshold tests in np.float32
operations taken one at a time, and the builders of the inputs the merge tests share.  Test infrastructure only.

Every output is an integer or an integer divided by P P, and each threshold test is one correctly rounded float32 multiply and one compare on both sides, so the
device, the torch composition and this restatement have to be EQUAL.

The hand-worked case (`hand_worked()`): image 8 x 12, P = 4, K = 5, min_area = 2, max_area = 0, iou_thresh = 0.5, contain_thresh = 0.6.
  k0 = rows 0-3 x cols 0-5 (value 1), k1 = rows 0-3 x cols 1-6 (value 7), k2 = rows 4-7 x cols 6-11 (value 1), k3 = rows 2-5 x cols 4-7 (value 255),
  k4 = the single pixel (0, 11); scores (.9, .8, .7, .95, 1.0).
  area  (24, 24, 24, 16, 1); k4 is below min_area: not valid.
  inter (24, 20, 0, 4, 0) / (20, 24, 0, 6, 0) / (0, 0, 24, 4, 0) / (4, 6, 4, 16, 0) / (0, 0, 0, 0, 1)
  order k3 (.95), k0 (.9), k1 (.8), k2 (.7).  k3 is kept: label 1.  k0 against k3: 4 > .5 * 36 no, 4 > .6 * 16 no: kept, label 2.  k1 against k3: 6 > .5 * 34 no,
  6 > 9.6 no; against k0: 20 > .5 * 28 = 14 yes: absorbed by label 2.  k2 against k3: 4 > 18 no, 4 > 9.6 no; against k0: 0: kept, label 3.
  owner (2, 2, 3, 1, 0).
  absorb = 1: label 1 paints k3's 16 pixels; label 2 paints k0 and k1 (rows 0-3 x cols 0-6 = 28) less the 6 of k3: 22; label 3 paints k2's 24 less 4: 20.
              label_area (16, 22, 20, 0, 0), stats (4, 3, 58, 1), cover ((1, .875, 0), (0, .75, 1))
  absorb = 0: label 2 paints k0 alone, 24 less 4: 20.  label_area (16, 20, 20, 0, 0), stats (4, 3, 56, 1), cover ((1, .75, 0), (0, .75, 1))"""
import numpy as np

F32 = np.float32


def order(valid, score):
    """the valid candidates in the selection order: the higher score first, a NaN above every number, -0 equal to +0, the lower index first"""
    def rank(k):
        s = float(score[k])
        return (0, 0.0, k) if s != s else (1, -s + 0.0, k)
    return sorted((int(k) for k in np.flatnonzero(valid)), key=rank)


def merge(segs, scores, P, *, min_area=1, max_area=0, iou_thresh=0.5, contain_thresh=0.6, absorb=1):
    """segs [B,K,H,W] (nonzero = in), scores [B,K] float32 or None.  Returns a dict of arrays named as the outputs of the call."""
    segs = np.asarray(segs) != 0
    B, K, H, W = segs.shape
    gh, gw = H // P, W // P
    scores = np.zeros((B, K), F32) if scores is None else np.asarray(scores, F32)
    iou_t, con_t = F32(iou_thresh), F32(contain_thresh)
    hi = max_area if max_area > 0 else H * W
    out = {"labels": np.zeros((B, H, W), np.uint8), "owner": np.zeros((B, K), np.int32), "area": np.zeros((B, K), np.int32), "label_area": np.zeros((B, K), np.int32),
           "inter": np.zeros((B, K, K), np.int32), "cover": np.zeros((B, gh, gw), F32), "stats": np.zeros((B, 4), np.int32)}
    for b in range(B):
        area, inter = out["area"][b], out["inter"][b]
        for k in range(K):
            area[k] = np.count_nonzero(segs[b, k])
        for j in range(K):
            for k in range(j, K):
                inter[j, k] = inter[k, j] = np.count_nonzero(segs[b, j] & segs[b, k])
        valid = [area[k] >= max(1, min_area) and area[k] <= hi for k in range(K)]
        kept, sets, owner = [], [], out["owner"][b]
        with np.errstate(invalid="ignore"):
            for k in order(valid, scores[b]):
                for m, j in enumerate(kept):
                    I = int(inter[j, k])
                    if F32(I) > iou_t * F32(int(area[j]) + int(area[k]) - I) or F32(I) > con_t * F32(min(int(area[j]), int(area[k]))):
                        owner[k] = m + 1
                        if absorb:
                            sets[m].append(k)
                        break
                else:
                    kept.append(k)
                    sets.append([k])
                    owner[k] = len(kept)
        lab = out["labels"][b]
        for m in range(len(kept), 0, -1):  # the lowest label is painted last, over the others
            for k in sets[m - 1]:
                lab[segs[b, k]] = m
        for m in range(1, K + 1):
            out["label_area"][b, m - 1] = np.count_nonzero(lab == m)
        for i in range(gh):
            for j in range(gw):
                out["cover"][b, i, j] = F32(np.count_nonzero(lab[i * P:(i + 1) * P, j * P:(j + 1) * P])) / F32(P * P)
        out["stats"][b] = (sum(valid), len(kept), np.count_nonzero(lab), sum(valid) - len(kept))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------------
def rect(H, W, y0, y1, x0, x1, value=1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = value
    return m


def hand_worked():
    """(segs [1,5,8,12] uint8, scores [1,5], P, keywords)"""
    segs = np.stack([rect(8, 12, 0, 4, 0, 6, 1), rect(8, 12, 0, 4, 1, 7, 7), rect(8, 12, 4, 8, 6, 12, 1), rect(8, 12, 2, 6, 4, 8, 255), rect(8, 12, 0, 1, 11, 12, 1)])[None]
    scores = np.array([[.9, .8, .7, .95, 1.0]], F32)
    return segs, scores, 4, dict(min_area=2, max_area=0, iou_thresh=0.5, contain_thresh=0.6)


HAND = {"area": [[24, 24, 24, 16, 1]], "owner": [[2, 2, 3, 1, 0]],
        "inter": [[[24, 20, 0, 4, 0], [20, 24, 0, 6, 0], [0, 0, 24, 4, 0], [4, 6, 4, 16, 0], [0, 0, 0, 0, 1]]],
        1: {"label_area": [[16, 22, 20, 0, 0]], "stats": [[4, 3, 58, 1]], "cover": [[[1, .875, 0], [0, .75, 1]]]},
        0: {"label_area": [[16, 20, 20, 0, 0]], "stats": [[4, 3, 56, 1]], "cover": [[[1, .75, 0], [0, .75, 1]]]}}


def random_rects(seed, B, K, H, W, values=(1, 7, 255)):
    """random rectangles; every odd candidate is a near-duplicate of the one before it (shifted by at most one pixel); content differs per row"""
    g = np.random.default_rng(seed)
    segs = np.zeros((B, K, H, W), np.uint8)
    for b in range(B):
        for k in range(K):
            if k % 2 and g.random() < 0.7:
                dy, dx = g.integers(-1, 2, 2)
                segs[b, k] = np.roll(segs[b, k - 1], (dy, dx), (0, 1))
                segs[b, k][segs[b, k] != 0] = values[k % len(values)]
            else:
                y0, x0 = g.integers(0, H - 1), g.integers(0, W - 1)
                y1, x1 = g.integers(y0 + 1, H + 1), g.integers(x0 + 1, W + 1)
                segs[b, k] = rect(H, W, y0, y1, x0, x1, values[k % len(values)])
    return segs, g.random((B, K), dtype=F32)


def identical(B, K, H, W):
    segs = np.zeros((B, K, H, W), np.uint8)
    segs[:, :, 1:H - 1, 2:W - 1] = 255
    return segs


def special_scores(B, K):
    """NaN, +-inf, +-0 and ties, cycled over the candidates, shifted per row"""
    vals = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 0.5, 0.5, np.nan, -1.0, 0.0], F32)
    return np.stack([vals[(np.arange(K) + b) % len(vals)] for b in range(B)])


def chain(H=16, W=16):
    """a contains b contains c: 12 x 12, 8 x 8 and 4 x 4 squares from the same corner"""
    return np.stack([rect(H, W, 0, 12, 0, 12), rect(H, W, 0, 8, 0, 8), rect(H, W, 0, 4, 0, 4)])[None]


def half_overlap(H=8, W=16):
    """two 4 x 6 rectangles that share 4 x 4 pixels: areas 24 and 24, intersection 16, union 32 -- I / U is exactly 0.5, I / min is 2 / 3"""
    return np.stack([rect(H, W, 0, 4, 0, 6), rect(H, W, 0, 4, 2, 8)])[None]


def shifted_pairs(H=512, W=512, n=32):
    """the largest case: n rectangles of 160 x 200 shifted by (9, 7) pixels each, each one twice (candidates 2 i and 2 i + 1 are equal); scores fall with the index"""
    segs = np.zeros((1, 2 * n, H, W), np.uint8)
    for i in range(n):
        segs[0, 2 * i] = segs[0, 2 * i + 1] = rect(H, W, 9 * i, 9 * i + 160, 7 * i, 7 * i + 200, 1 + i)
    return segs, np.linspace(1.0, 0.0, 2 * n, dtype=F32)[None]
