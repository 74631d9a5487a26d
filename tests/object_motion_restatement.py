"""A NumPy restatement of `cwm_object_motion` (the definition: include/cwm_hip.h, csrc/object_motion.hip): steps 1 to 6 as written there -- int64 sums, and the
model as np.float64 operations, one per line, in the stated order (NumPy has no fused multiply-add) --, and the cases the object-motion tests share.  Test
infrastructure only.

The device, the torch composition and this restatement have to be EQUAL: the integer tables by value, the model as int64 bit patterns (`bits`)."""
import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
SIDE = 65
NAMES = ("sums", "counts", "model", "occ")


def bits(a):
    """the bit patterns of a float64 array (other dtypes are returned as they are)"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def model_of(sums, min_pixels=1, min_affine=16, min_det=1.0):
    """step 6: sums [..,65,16] int64 -> model [..,65,12] float64"""
    S = [sums[..., i].astype(F64) for i in range(14)]  # (round to nearest)
    N = sums[..., 0]
    some = N >= min_pixels
    n = np.where(N > 0, S[0], F64(1))  # (an empty slot divides by 1; it is zeroed below)
    with np.errstate(all="ignore"):
        mx = S[1] / n
        my = S[2] / n
        mu = S[6] / n
        mv = S[7] / n

        def cov(s, a, b):
            q = s / n
            p = a * b
            return q - p

        cxx, cxy, cyy = cov(S[3], mx, mx), cov(S[4], mx, my), cov(S[5], my, my)
        cxu, cyu, cxv, cyv = cov(S[8], mx, mu), cov(S[9], my, mu), cov(S[10], mx, mv), cov(S[11], my, mv)
        d0 = cxx * cyy
        d1 = cxy * cxy
        det = d0 - d1
        affine = some & (N >= min_affine) & (det >= min_det)
        scale, scale2 = F64(2.0 ** -8), F64(2.0 ** -16)

        def coef(p, q, r, s):
            e0 = p * q
            e1 = r * s
            e = e0 - e1
            e = e / det
            return e * scale

        a11, a12 = coef(cxu, cyy, cyu, cxy), coef(cyu, cxx, cxu, cxy)
        a21, a22 = coef(cxv, cyy, cyv, cxy), coef(cyv, cxx, cxv, cxy)
        tu = mu * scale
        tv = mv * scale
        var_u = cov(S[12], mu, mu) * scale2
        var_v = cov(S[13], mv, mv) * scale2
    zero = np.zeros_like(det)
    valid = np.where(affine, F64(2), np.where(some, F64(1), F64(0)))
    cols = [valid, tu, tv] + [np.where(affine, a, zero) for a in (a11, a12, a21, a22)] + [mx, my, var_u, var_v, zero]
    out = np.stack([np.where(some, c, zero) for c in cols], -1)
    assert out.dtype == F64
    return out


def motion(labels, flow, code=None, other=None, min_pixels=1, min_affine=16, min_det=1.0):
    """labels [R,H,W] uint8, flow [R,2,H,W] float32, code / other [R,H,W] uint8 or None -> dict of sums int64 [R,65,16], counts int32 [R,65,4], model float64
    [R,65,12], occ int32 [R,65,65] (None without other)"""
    labels, flow = np.asarray(labels, np.uint8), np.asarray(flow, F32)
    R, H, W = labels.shape
    # 1 slot
    l = labels.astype(I64)
    l = np.where(l > 64, 0, l)
    # 2 target
    u, v = flow[:, 0], flow[:, 1]
    xi = np.broadcast_to(np.arange(W, dtype=I64)[None, None, :], (R, H, W))
    yi = np.broadcast_to(np.arange(H, dtype=I64)[None, :, None], (R, H, W))
    with np.errstate(invalid="ignore", over="ignore"):
        usable = np.isfinite(u) & np.isfinite(v) & (np.abs(u) <= F32(4096)) & (np.abs(v) <= F32(4096))
        fx, fy = xi.astype(F32) + u, yi.astype(F32) + v
        assert fx.dtype == F32
        inside = (fx >= F32(0)) & (fx <= F32(W - 1)) & (fy >= F32(0)) & (fy <= F32(H - 1))
    # 3 class
    k = np.where(usable & inside, 0 if code is None else (np.asarray(code) != 0).astype(I64), 2)
    rows = np.broadcast_to(np.arange(R)[:, None, None], (R, H, W))
    counts = np.zeros((R, SIDE, 4), I64)
    np.add.at(counts, (rows, l, k), 1)
    # 4 sums
    k0 = k == 0
    qu = np.rint(np.where(k0, u, F32(0)) * F32(256)).astype(I64)
    qv = np.rint(np.where(k0, v, F32(0)) * F32(256)).astype(I64)
    assert np.abs(qu).max(initial=0) <= 1 << 20 and np.abs(qv).max(initial=0) <= 1 << 20
    terms = [np.ones_like(xi), xi, yi, xi * xi, xi * yi, yi * yi, qu, qv, xi * qu, yi * qu, xi * qv, yi * qv, qu * qu, qv * qv]
    sums = np.zeros((R, SIDE, 16), I64)
    for i, t in enumerate(terms):
        np.add.at(sums[:, :, i], (rows[k0], l[k0]), t[k0])
    # 5 occluder
    occ = None
    if other is not None:
        k1 = k == 1
        sx, sy = np.rint(fx[k1]).astype(I64), np.rint(fy[k1]).astype(I64)
        m = np.asarray(other, np.uint8)[rows[k1], sy, sx].astype(I64)
        m = np.where(m > 64, 0, m)
        occ = np.zeros((R, SIDE, SIDE), I64)
        np.add.at(occ, (rows[k1], l[k1], m), 1)
        occ = occ.astype(np.int32)
    # 6 model
    return {"sums": sums, "counts": counts.astype(np.int32), "model": model_of(sums, min_pixels, min_affine, min_det), "occ": occ}


# ---- the shared cases --------------------------------------------------------------------------------------------------------------------------------------
HOSTILE = np.array([np.nan, np.inf, -np.inf, 5000.0, -4096.5], F32)


def case_random(R, H, W, seed=3, top=80, reach=6.0):
    """labels in blocks of 4 x 8 pixels drawn from 0 .. top (values above 64 occur and read as 0), with single pixels redrawn; fractional flows of up to +-reach
    px; NaN, +-inf, 5000 and -4096.5 sprinkled over one channel; row 0 of every plane targets the last column exactly and column 0 the last row exactly (on the
    edge: inside); random code bytes 0, 1, 2 and 7; an independent other map.  Returns labels, flow, code, other"""
    g = np.random.default_rng(seed)
    blocks = g.integers(0, top + 1, (R, (H + 3) // 4, (W + 7) // 8))
    labels = np.repeat(np.repeat(blocks, 4, 1), 8, 2)[:, :H, :W].copy()
    pick = g.random(labels.shape) < 0.05
    labels[pick] = g.integers(0, top + 1, int(pick.sum()))
    flow = g.uniform(-reach, reach, (R, 2, H, W)).astype(F32)
    flow[:, :, ::3, ::5] = np.round(flow[:, :, ::3, ::5] * 256) / 256  # (some exact multiples of 1/256; the others round)
    bad = g.random((R, H, W)) < 0.04
    ch = g.integers(0, 2, int(bad.sum()))
    b, y, x = np.nonzero(bad)
    flow[b, ch, y, x] = HOSTILE[g.integers(0, len(HOSTILE), int(bad.sum()))]
    flow[:, 0, 0, :], flow[:, 1, 0, :] = F32(W - 1) - np.arange(W, dtype=F32), 0
    flow[:, 0, 1:, 0], flow[:, 1, 1:, 0] = 0, (F32(H - 1) - np.arange(H, dtype=F32))[1:]
    code = g.choice(np.array([0, 0, 0, 1, 1, 2, 7], np.uint8), (R, H, W))
    other = g.integers(0, top + 1, (R, H, W)).astype(np.uint8)
    return labels.astype(np.uint8), flow, code, other


def case_rows(R, H, W, seed=5):
    """every wave sees one label: whole image rows of one slot (the slot changes every two rows), a smooth flow"""
    g = np.random.default_rng(seed)
    labels = np.broadcast_to(((np.arange(H) // 2) % 65)[None, :, None], (R, H, W)).astype(np.uint8)
    flow = (g.integers(-512, 513, (R, 2, H, W)) / 256).astype(F32)
    code = (g.random((R, H, W)) < 0.2).astype(np.uint8)
    other = np.roll(labels, 3, 1)
    return labels, flow, code, other


def case_checker(R, H, W, seed=6):
    """labels change every pixel and all 64 slots (and 0) are live: no wave and no lane holds one slot"""
    g = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    labels = np.broadcast_to(((ys * 7 + xs) % 65)[None], (R, H, W)).astype(np.uint8)
    flow = (g.integers(-768, 769, (R, 2, H, W)) / 256).astype(F32)
    code = (g.random((R, H, W)) < 0.3).astype(np.uint8)
    other = np.broadcast_to(((ys + xs * 3) % 65)[None], (R, H, W)).astype(np.uint8)
    return labels, flow, code, other


# the translation scene of the issue: 32 x 48, slot 1 moves 8 px to the right and slides behind slot 2, uncovering background
TH, TW = 32, 48


def translation_scene():
    """labels A and B [1,H,W] uint8, forward flow (A to B, on A's grid) and backward flow (B to A, on B's grid) [1,2,H,W] float32"""
    A, B = np.zeros((1, TH, TW), np.uint8), np.zeros((1, TH, TW), np.uint8)
    A[:, 8:24, 8:24], A[:, 8:24, 28:40] = 1, 2
    B[:, 8:24, 16:28], B[:, 8:24, 28:40] = 1, 2
    fwd, back = np.zeros((1, 2, TH, TW), F32), np.zeros((1, 2, TH, TW), F32)
    fwd[:, 0][A == 1] = 8
    back[:, 0][B == 1] = -8
    return A, B, fwd, back


def rotation_scene():
    """one slot on the 16 x 16 block rows 8..23 x cols 16..31 of a 32 x 48 frame: u = -(y - 15.5) / 64, v = (x - 23.5) / 64 (every 256 u is an integer)"""
    labels = np.zeros((1, TH, TW), np.uint8)
    labels[:, 8:24, 16:32] = 1
    ys, xs = np.meshgrid(np.arange(TH, dtype=F64), np.arange(TW, dtype=F64), indexing="ij")
    flow = np.zeros((1, 2, TH, TW), F32)
    flow[0, 0], flow[0, 1] = -(ys - 15.5) / 64, (xs - 23.5) / 64
    assert np.array_equal(flow * 256, np.rint(flow * 256))
    flow[:, :, labels[0] == 0] = 0
    return labels, flow
