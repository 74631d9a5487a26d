"""The definition of `cwm_seed_select` (the header comment of csrc/seed_select.hip) restated in NumPy with plain loops: every comparison is on float32 values, the
relative threshold is one `np.float32` multiply and the race's key one `np.float32` division.  Also the case generators the CPU and GPU tests share.

select(...) -> dict(seeds [B,K,2] int32, cells [B,K] int32, values [B,K] float32, pooled [B,n] float32, peaks [B,n] uint8, stats [B,4] int32)"""
import numpy as np


def before(ka, ia, kb, ib):
    """the order of csrc/select_order.h: the higher key first, a NaN above every number, -0 equal to +0, the lower index first"""
    na, nb = np.isnan(ka), np.isnan(kb)
    if na or nb:
        return (na and not nb) or (na and nb and ia < ib)
    if ka != kb:
        return ka > kb
    return ia < ib


def select(map, P, K, radius=1, peaks_only=False, abs_thresh=-np.inf, rel_thresh=0.0, free=None, e=None, prior=None, cells=False):
    map = np.asarray(map, np.float32)
    B = map.shape[0]
    if cells:
        gh, gw = map.shape[1:]
    else:
        gh, gw = map.shape[1] // P, map.shape[2] // P
    n, r = gh * gw, int(radius)
    out = dict(seeds=np.full((B, K, 2), -1, np.int32), cells=np.full((B, K), -1, np.int32), values=np.zeros((B, K), np.float32),
               pooled=np.zeros((B, n), np.float32), peaks=np.zeros((B, n), np.uint8), stats=np.zeros((B, 4), np.int32))
    for b in range(B):
        v, sy, sx = np.zeros(n, np.float32), np.zeros(n, np.int64), np.zeros(n, np.int64)
        for c in range(n):  # 1 pool
            i, j = divmod(c, gw)
            if cells:
                v[c], sy[c], sx[c] = map[b, i, j], i * P + P // 2, j * P + P // 2
                continue
            best = None
            for py in range(P):
                for px in range(P):
                    x = map[b, i * P + py, j * P + px]
                    if not np.isnan(x) and (best is None or x > best[0]):  # (strictly greater: the first pixel that attains the maximum; -0 == +0)
                        best = (x, py, px)
            if best is None:
                v[c] = np.nan
            else:
                v[c], sy[c], sx[c] = best[0], i * P + best[1], j * P + best[2]
        out["pooled"][b] = v
        number = ~np.isnan(v)
        near = lambda c, d: abs(c // gw - d // gw) <= r and abs(c % gw - d % gw) <= r  # noqa: E731
        for c in range(n):  # 4 peaks
            if number[c]:
                i, j = divmod(c, gw)
                window = [y * gw + x for y in range(max(i - r, 0), min(i + r, gh - 1) + 1) for x in range(max(j - r, 0), min(j + r, gw - 1) + 1)]
                out["peaks"][b, c] = all(not before(v[d], d, v[c], c) for d in window if d != c and number[d])
        is_free = np.ones(n, bool) if free is None else np.asarray(free).reshape(B, n)[b] != 0
        out["stats"][b, 0] = int((number & is_free).sum())
        if not number.any():  # 2 no row maximum: no candidates
            continue
        m = np.float32(v[number].max())
        t = np.float32(abs_thresh)  # 3
        if rel_thresh > 0:
            t = max(t, np.float32(rel_thresh) * m)
        pri = [] if prior is None else [int(q) for q in np.asarray(prior).reshape(B, -1)[b] if 0 <= q < n]
        cand = {}
        for c in range(n):  # 5, 6
            if not (is_free[c] and number[c] and v[c] >= t) or (peaks_only and not out["peaks"][b, c]) or any(near(c, q) for q in pri):
                continue
            with np.errstate(all="ignore"):
                cand[c] = v[c] if e is None else np.float32(max(v[c], np.float32(0))) / np.float32(np.asarray(e, np.float32).reshape(B, n)[b, c])
        out["stats"][b, 1] = len(cand)
        for k in range(K):  # 7
            pick = None
            for c in sorted(cand):
                if pick is None or before(cand[c], c, cand[pick], pick):
                    pick = c
            if pick is None:
                break
            out["cells"][b, k], out["values"][b, k], out["seeds"][b, k] = pick, v[pick], (sy[pick], sx[pick])
            cand = {c: key for c, key in cand.items() if not near(c, pick)}
            out["stats"][b, 2] += 1
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------------------
GRIDS = [(3, 3, 4), (5, 7, 4), (28, 28, 8), (14, 14, 16), (64, 64, 4)]  # (gh, gw, P)


def bumps(seed, B, gh, gw, P, n_bumps=6):
    """a smooth pixel map [B,H,W] with a few bumps of different heights per row (different content per row), plus a little noise"""
    rng = np.random.RandomState(seed)
    H, W = gh * P, gw * P
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = rng.rand(B, H, W).astype(np.float32) * 0.05
    for b in range(B):
        for _ in range(n_bumps):
            cy, cx, s, h = rng.rand() * H, rng.rand() * W, 1.0 + rng.rand() * P, 0.3 + rng.rand()
            out[b] += (h * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))).astype(np.float32)
    return out


def quantised(seed, B, gh, gw, P, levels=5):
    """few distinct values: plateaus and ties everywhere"""
    return (np.random.RandomState(seed).randint(0, levels, (B, gh * P, gw * P)) / np.float32(levels)).astype(np.float32)


def signed_zeros(seed, B, gh, gw, P):
    """-0, +0 and a few negative numbers: the maximum of most cells is a zero of either sign"""
    rng = np.random.RandomState(seed)
    m = np.where(rng.rand(B, gh * P, gw * P) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    return np.where(rng.rand(*m.shape) < 0.3, np.float32(-1.0), m).astype(np.float32)


def with_nans(m, seed):
    """NaN pixels sprinkled inside cells, cell (0, 0) of row 0 all NaN, the last row all NaN"""
    rng = np.random.RandomState(seed)
    m = m.copy()
    m[rng.rand(*m.shape) < 0.2] = np.nan
    P = 4
    m[0, :P, :P] = np.nan
    m[-1] = np.nan
    return m


def draws(seed, B, n):
    return np.random.RandomState(seed).exponential(size=(B, n)).astype(np.float32)


def free_cells(seed, B, n, frac=0.7):
    return (np.random.RandomState(seed).rand(B, n) < frac).astype(np.uint8)


def same(a, b):
    """bit equality of two float32 arrays, every NaN taken as one value"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.where(np.isnan(a), np.float32(np.nan), a).view(np.int32), np.where(np.isnan(b), np.float32(np.nan), b).view(np.int32))


def assert_equal(got, want, what=""):
    """every output by equality; the floats bit for bit"""
    for k in ("seeds", "cells", "peaks", "stats"):
        assert np.array_equal(np.asarray(got[k]).reshape(want[k].shape).astype(want[k].dtype), want[k]), (what, k, np.asarray(got[k]).reshape(want[k].shape), want[k])
    for k in ("values", "pooled"):
        assert same(np.asarray(got[k]).reshape(want[k].shape), want[k]), (what, k)


def cases():
    """[(name, keyword arguments of select())]: the cases of the issue, every one small enough for the loops above"""
    out = []

    def add(name, map, P, K=8, **kw):
        out.append((name, dict(map=map, P=P, K=K, **kw)))

    for gh, gw, P in GRIDS:  # grids, three rows of different content (two at the 4096-cell limit)
        big = gh * gw == 4096
        add("grid_%dx%d_P%d" % (gh, gw, P), bumps(gh + P, 2 if big else 3, gh, gw, P), P, radius=3 if big else 1, peaks_only=True, rel_thresh=0.1)
    m28 = bumps(5, 3, 28, 28, 8)
    for r in (0, 1, 3):
        add("radius_%d" % r, m28, 8, radius=r)
    add("radius_64_5x7", bumps(6, 3, 5, 7, 4), 4, radius=64)
    add("radius_64_14x14_peaks", bumps(7, 3, 14, 14, 16), 16, radius=64, peaks_only=True)
    add("dead_slots", m28, 8, K=64, radius=3)
    add("dead_slots_peaks", m28, 8, K=64, radius=2, peaks_only=True, rel_thresh=0.2)
    add("constant", np.full((3, 40, 56), 0.25, np.float32), 8, K=64, radius=2)
    add("constant_peaks", np.full((2, 40, 56), 0.25, np.float32), 8, K=16, radius=1, peaks_only=True)
    add("plateaus", quantised(8, 3, 5, 7, 4), 4, K=12, radius=1, peaks_only=True)
    add("signed_zeros", signed_zeros(9, 3, 5, 7, 4), 4, K=12, radius=1)
    add("signed_zeros_peaks", signed_zeros(10, 3, 5, 7, 4), 4, K=12, radius=1, peaks_only=True, rel_thresh=0.5)
    nan = with_nans(bumps(11, 3, 5, 7, 4), 12)
    add("nan", nan, 4, K=12, radius=1)
    add("nan_peaks_race", nan, 4, K=12, radius=1, peaks_only=True, e=draws(13, 3, 35))
    m57 = bumps(14, 3, 5, 7, 4)
    add("free_none", m57, 4, radius=1, free=np.zeros((3, 35), np.uint8))
    free = free_cells(15, 3, 35)
    free[np.arange(3), select(m57, 4, 1, radius=0)["cells"][:, 0]] = 0
    add("free_without_top", m57, 4, radius=1, peaks_only=True, free=free)
    add("prior", m57, 4, radius=1, prior=np.array([[-1, 0, 17], [34, -1, -1], [-1, -1, -1]], np.int32))
    add("prior_radius_0", m57, 4, radius=0, prior=np.array([[-1, 0], [34, 6], [28, 99]], np.int32), free=free_cells(16, 3, 35))
    add("rel_negative_maximum", -1 - m57, 4, radius=1, rel_thresh=0.5)
    add("rel_negative_maximum_2", -1 - m57, 4, radius=1, rel_thresh=2.0, abs_thresh=-3.0)
    add("abs_alone", m57, 4, radius=0, abs_thresh=0.5)
    add("rel_and_abs", m57, 4, radius=1, abs_thresh=0.2, rel_thresh=0.6, peaks_only=True)
    add("race", m28, 8, radius=2, e=draws(17, 3, 784), free=free_cells(18, 3, 784))
    add("race_peaks", m28, 8, radius=2, peaks_only=True, e=draws(19, 3, 784))
    add("race_nan_draws", m57, 4, radius=1, e=np.where(np.arange(35)[None] % 5 == 0, np.float32(np.nan), draws(20, 3, 35)))
    cells = quantised(21, 3, 7, 5, 1, levels=7)
    add("cells", cells, 16, radius=1, cells=True, peaks_only=True)
    add("cells_race", bumps(22, 3, 9, 6, 1, 3), 8, radius=1, cells=True, e=draws(23, 3, 54), free=free_cells(24, 3, 54), prior=np.array([[3, -1], [-1, -1], [53, 20]], np.int32))
    add("cells_nan", with_nans(bumps(25, 3, 8, 8, 1, 3), 26), 4, radius=2, cells=True)
    return out


_WANT = {}


def want(name, kw):
    """the restatement of a case, computed once per process"""
    if name not in _WANT:
        _WANT[name] = select(**kw)
    return _WANT[name]
