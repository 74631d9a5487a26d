"""`cwm_parallax` restated in NumPy from the text of its definition in include/cwm_hip.h (steps 1 - 7), plainly: loops over rows, samples and slots, arrays over
the pixels, ONE np.float64 operation per line, a stable argsort for the order statistics.  The tests hold the torch composition (CPU) and the library (GPU) to it
by EQUALITY of bit patterns.  Also the shared cases: every one generates flows that are exactly representable (multiples of 1/512 px: half of them fall on a
rounding tie of step 2)."""
import numpy as np

NAMES = ("par", "spread", "off", "cnt", "ref", "hist", "slot_tab")
COMPASS = ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, -1), (-1, 1))  # (dy, dx): E, S, W, N, SE, SW, NW, NE


def bits(a):
    """float arrays as their bit patterns, so that NaNs and signed zeros compare"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


def dirs_of(S, px=8):
    return np.array([(COMPASS[s % 8][0] * px, COMPASS[s % 8][1] * px) for s in range(S)], np.int32)


def min_ref_q_of(min_ref):
    return int(round(float(min_ref) * 256.0))


def parallax(flows, dirs=None, labels=None, ref_slot=-1, min_pixels=1, min_ref=0.25, min_samples=None):
    flows = np.asarray(flows, np.float32)
    R, _, H, W, S = flows.shape
    min_samples = (S + 1) // 2 if min_samples is None else min_samples
    f64, q = np.float64, min_ref_q_of(min_ref)
    u, v = flows[:, 0], flows[:, 1]  # [R,H,W,S]
    with np.errstate(invalid="ignore"):
        usable = (np.abs(u) <= np.float32(4096)) & (np.abs(v) <= np.float32(4096))  # 1
        qu = np.rint(np.where(usable, u, np.float32(0)) * np.float32(256)).astype(np.int64)  # 2 (np.rint rounds half to even)
        qv = np.rint(np.where(usable, v, np.float32(0)) * np.float32(256)).astype(np.int64)
    lab = None
    if labels is not None:
        lab = np.asarray(labels).astype(np.int64)
        lab = np.where(lab > 64, 0, lab)
    out = dict(par=np.empty((R, H, W), np.float32), spread=np.empty((R, H, W), np.float32), off=np.empty((R, H, W), np.float32), cnt=np.empty((R, H, W), np.uint8),
               ref=np.empty((R, S, 4), f64), hist=None, slot_tab=None)
    if lab is not None:
        out["hist"], out["slot_tab"] = np.zeros((R, 65, 256), np.int32), np.zeros((R, 65, 8), np.int32)
    nan32 = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
    for r in range(R):
        p = np.full((H, W, S), np.inf, f64)
        c = np.full((H, W, S), np.inf, f64)
        ok = np.zeros((H, W, S), bool)
        for s in range(S):
            if dirs is not None:  # 3
                mu, mv, N = f64(256 * int(dirs[s][1])), f64(256 * int(dirs[s][0])), H * W
            else:
                m = usable[r, :, :, s] if ref_slot < 0 else usable[r, :, :, s] & (lab[r] == ref_slot)
                SU, SV, N = int(qu[r, :, :, s][m].sum()), int(qv[r, :, :, s][m].sum()), int(m.sum())
                mu = f64(SU) / f64(N) if N else f64(0)
                mv = f64(SV) / f64(N) if N else f64(0)
            uu = mu * mu
            vv = mv * mv
            den = uu + vv
            thr = f64(q) * f64(q)
            live = N >= min_pixels and den >= thr
            out["ref"][r, s] = (mu, mv, den, 1.0 if live else 0.0)
            if not live:
                continue
            ok[:, :, s] = usable[r, :, :, s]
            du, dv = qu[r, :, :, s].astype(f64), qv[r, :, :, s].astype(f64)  # 4 (exact)
            a = du * mu
            b = dv * mv
            t = a + b
            p[:, :, s] = t / den
            a = du * mv
            b = dv * mu
            t = a - b
            t = np.abs(t)
            c[:, :, s] = t / den
        n = ok.sum(-1)  # 5
        good = n >= min_samples
        P = np.take_along_axis(np.where(ok, p, np.inf), np.argsort(np.where(ok, p, np.inf), axis=-1, kind="stable"), -1)
        Cc = np.take_along_axis(np.where(ok, c, np.inf), np.argsort(np.where(ok, c, np.inf), axis=-1, kind="stable"), -1)
        m1 = np.maximum(n - 1, 0)
        pick = lambda arr, k: np.take_along_axis(arr, k[..., None], -1)[..., 0]  # noqa: E731
        q1, med, q3, cmed = pick(P, m1 // 4), pick(P, m1 // 2), pick(P, (3 * m1) // 4), pick(Cc, m1 // 2)
        with np.errstate(invalid="ignore"):
            d = np.where(good, q3, 0.0) - np.where(good, q1, 0.0)
        out["par"][r] = np.where(good, np.where(good, med, 0.0).astype(np.float32), nan32)
        out["spread"][r] = np.where(good, d.astype(np.float32), nan32)
        out["off"][r] = np.where(good, np.where(good, cmed, 0.0).astype(np.float32), nan32)
        out["cnt"][r] = n.astype(np.uint8)
        if lab is None:
            continue
        for y in range(H):  # 6
            for x in range(W):
                l = lab[r, y, x]
                if good[y, x]:
                    b = np.floor(med[y, x] * f64(32.0)) + f64(128.0)
                    b = min(max(b, f64(0.0)), f64(255.0))
                    out["hist"][r, l, int(b)] += 1
                else:
                    out["slot_tab"][r, l, 1] += 1
        for l in range(65):  # 7
            cum = np.cumsum(out["hist"][r, l].astype(np.int64))
            ns = int(cum[-1])
            row = out["slot_tab"][r, l]
            row[0] = ns
            if ns == 0:
                row[2:7] = -1
                continue
            for i, k in enumerate(((ns - 1) // 2, (ns - 1) // 4, (3 * (ns - 1)) // 4)):
                row[2 + i] = min(b for b in range(256) if cum[b] > k)
            some = np.nonzero(out["hist"][r, l])[0]
            row[5], row[6] = some[0], some[-1]
    return out


# ---- cases: (flows [R,2,H,W,S] float32, labels [R,H,W] uint8) -------------------------------------------------------------------------------------------------
def block_labels(rng, R, H, W, top=5):
    """labels in blocks of 4 x 8 pixels, slots 0 .. top"""
    g = rng.integers(0, top + 1, (R, (H + 3) // 4, (W + 7) // 8))
    return np.repeat(np.repeat(g, 4, 1), 8, 2)[:, :H, :W].astype(np.uint8)


def case_random(R, H, W, S, seed=0):
    """flows in 1/512 px up to +- 24 px; the background drifts with the sample so that the reference motion lives"""
    rng = np.random.default_rng(seed)
    k = rng.integers(-24 * 512, 24 * 512 + 1, (R, 2, H, W, S))
    drift = rng.integers(2 * 512, 12 * 512, (1, 2, 1, 1, S)) * rng.choice([-1, 1], (1, 2, 1, 1, S))
    flows = ((k // 8 + drift) / 512.0).astype(np.float32)
    return flows, block_labels(rng, R, H, W)


def case_ties(R, H, W, S, seed=1):
    """few distinct values, so that the order statistics fall on ties, and many zero vectors: with a reference motion of either sign their projections are
    -0.0 and +0.0 in different sample positions"""
    rng = np.random.default_rng(seed)
    vals = np.array([0.0, 0.0, 0.0, 1.0, -1.0, 0.5, 8.0, -8.0], np.float32)
    flows = vals[rng.integers(0, len(vals), (R, 2, H, W, S))]
    flows[:, :, : H // 2, : W // 2] = 0.0
    flows[:, :, H // 2:, : W // 2] = np.float32(-0.0)
    return flows, block_labels(rng, R, H, W, top=3)


def case_hostile(R, H, W, S, seed=2):
    """NaN, +-inf, exactly 4096 and the float above it, pixels without a usable sample, row 0 without a usable vector at all, a sample (the last) in which
    nothing moves, no pixel of slot 3 in the last row, labels above 64"""
    rng = np.random.default_rng(seed)
    flows, labels = case_random(R, H, W, S, seed)
    bad = np.array([np.nan, np.inf, -np.inf, 4096.0, -4096.0, np.nextafter(np.float32(4096), np.float32(np.inf)), -np.nextafter(np.float32(4096), np.float32(np.inf))],
                   np.float32)
    hit = rng.random(flows.shape) < 0.08
    flows[hit] = bad[rng.integers(0, len(bad), int(hit.sum()))]
    flows[:, :, 1, :, :] = np.nan  # an image row of pixels without a usable sample
    flows[:, 0, 2, 0:4, :] = np.inf
    flows[..., S - 1] = 0.0
    flows[0] = np.nan
    labels = labels.copy()
    labels[:, 0, :4] = (65, 200, 255, 64)
    labels[-1][labels[-1] == 3] = 2
    return flows, labels


def plane_labels(R, H, W):
    """the background 0, a rectangle of slot 1 and a rectangle of slot 2"""
    labels = np.zeros((R, H, W), np.uint8)
    labels[:, H // 8: H // 2, W // 8: W // 2] = 1
    labels[:, H // 2 + 1: H - 2, W // 2 + 2: W - 3] = 2
    return labels


def case_planes(R, H, W, S, px=8):
    """three depth planes under the pans dirs_of(S): the background moves by exactly 1 d_s, slot 1 by 2 d_s, slot 2 by 3 d_s.  Returns (flows, labels, dirs)"""
    labels, dirs = plane_labels(R, H, W), dirs_of(S, px)
    gain = (labels.astype(np.float32) + 1.0)[:, None, :, :, None]  # [R,1,H,W,1]
    d = np.stack([dirs[:, 1], dirs[:, 0]], 0).astype(np.float32)[None, :, None, None, :]  # (dx, dy): channel 0 is horizontal
    return (gain * d).astype(np.float32), labels, dirs
