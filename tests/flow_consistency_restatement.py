"""A NumPy restatement of `cwm_flow_consistency` (the definition: include/cwm_hip.h, csrc/flow_consistency.hip): the seven steps as written there, np.float32
arrays throughout and every arithmetic step one NumPy operation, so that each is rounded to float32 on its own -- NumPy has no fused multiply-add; and the cases
the consistency tests share.  Test infrastructure only.

The device, the torch composition and this restatement have to be EQUAL: floats are compared as bit patterns (`bits`), so that NaN and the sign of zero count.
The magnitudes are ordinary (flows up to a few tens of pixels, thresholds >= 1e-6 where they are not exactly 0): no intermediate is subnormal, the tests pin
the definition and not a denormal mode."""
import numpy as np

F32 = np.float32
QNAN = np.array([0x7fc00000], np.uint32).view(F32)[0]
NAMES = ("code", "res", "masked", "cell", "stats")


def bits(a):
    """the bit patterns of a float32 array (other dtypes are returned as they are)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def one_direction(a, o, alpha, beta, P=0, contract=False):
    """a, o [B,2,H,W] float32 -> dict of code [B,H,W] uint8, res [B,H,W], masked [B,2,H,W], cell [B,H/P,W/P] (None without P), stats [B,4] int32.
    contract=True is NOT the definition: it fuses ru ru + rv rv into one rounding (the product exact in float64), as a contracting compiler would, so that a test
    can show how many pixels of a case tell the two apart"""
    a, o = np.asarray(a, F32), np.asarray(o, F32)
    B, _, H, W = a.shape
    alpha, beta = F32(alpha), F32(beta)
    u, v = a[:, 0], a[:, 1]
    xs = np.broadcast_to(np.arange(W, dtype=F32)[None, None, :], (B, H, W))
    ys = np.broadcast_to(np.arange(H, dtype=F32)[None, :, None], (B, H, W))
    with np.errstate(invalid="ignore", over="ignore"):
        # 1 target
        fx, fy = xs + u, ys + v
        inside = (fx >= F32(0)) & (fx <= F32(W - 1)) & (fy >= F32(0)) & (fy <= F32(H - 1))
        # 2 sample (an outside pixel samples at its own place; what it reads is discarded below)
        fx, fy = np.where(inside, fx, xs), np.where(inside, fy, ys)
        x0f, y0f = np.floor(fx), np.floor(fy)
        wx, wy = fx - x0f, fy - y0f
        ix0, iy0 = x0f.astype(np.int64), y0f.astype(np.int64)
        ix1, iy1 = np.minimum(ix0 + 1, W - 1), np.minimum(iy0 + 1, H - 1)
        rows = np.arange(B)[:, None, None]
        s = []
        for c in range(2):
            o00, o01, o10, o11 = o[rows, c, iy0, ix0], o[rows, c, iy0, ix1], o[rows, c, iy1, ix0], o[rows, c, iy1, ix1]
            d = o01 - o00
            d = wx * d
            top = o00 + d
            d = o11 - o10
            d = wx * d
            bot = o10 + d
            d = bot - top
            d = wy * d
            s.append(top + d)
        # 3 residual
        ru, rv = u + s[0], v + s[1]
        ru2, rv2 = ru * ru, rv * rv
        res = (ru.astype(np.float64) * ru.astype(np.float64) + rv2.astype(np.float64)).astype(F32) if contract else ru2 + rv2
        uu, vv, s00, s11 = u * u, v * v, s[0] * s[0], s[1] * s[1]
        m_a, m_s = uu + vv, s00 + s11
        mag = m_a + m_s
        thr = alpha * mag
        thr = thr + beta
        assert all(t.dtype == F32 for t in (fx, wx, top, s[0], res, mag, thr))
        # 4 decision
        code = np.where(inside, np.where(res <= thr, 0, 1), 2).astype(np.uint8)
        res = np.where(inside & (res == res), res, F32(np.inf)).astype(F32)
    # 5 masked
    masked = np.where((code == 0)[:, None], a, QNAN).astype(F32)
    # 6 cells
    cell = None
    if P:
        count = (code != 0).reshape(B, H // P, P, W // P, P).sum((2, 4))
        cell = count.astype(F32) / F32(P * P)
    # 7 stats
    stats = np.stack([(code == k).sum((1, 2)) for k in range(3)] + [np.zeros(B, np.int64)], 1).astype(np.int32)
    return {"code": code, "res": res, "masked": masked, "cell": cell, "stats": stats}


def consistency(a, o, alpha, beta, P=0, both=False):
    """the call: every output with a leading direction dimension D = 1 + both; direction 1 exchanges the roles of a and o"""
    dirs = [one_direction(a, o, alpha, beta, P)] + ([one_direction(o, a, alpha, beta, P)] if both else [])
    return {k: None if dirs[0][k] is None else np.stack([d[k] for d in dirs]) for k in NAMES}


# ---- the shared cases: name -> (a [B,2,H,W], o [B,2,H,W], alpha, beta) ------------------------------------------------------------------------------------
def grid(B, H, W):
    ys, xs = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
    return np.broadcast_to(xs, (B, H, W)), np.broadcast_to(ys, (B, H, W))


def const_flow(B, H, W, dx, dy):
    f = np.empty((B, 2, H, W), F32)
    f[:, 0], f[:, 1] = dx, dy
    return f


def case_consistent(B, H, W):
    """an exactly consistent integer pair (the frame moves by (+2, -1)) with alpha = beta = 0: every inside pixel has code 0 and res 0"""
    return const_flow(B, H, W, 2, -1), const_flow(B, H, W, -2, 1), 0.0, 0.0


def case_half(B, H, W, seed=1):
    """half-pixel flows: both weights 0.5, against a varied other flow"""
    g = np.random.default_rng(seed)
    a = g.integers(-2, 3, (B, 2, H, W)).astype(F32) + F32(0.5)
    o = (g.integers(-8, 9, (B, 2, H, W)) * 0.25).astype(F32)
    return a, o, 0.01, 0.5


def case_threshold(B, H, W, beta=0.25):
    """u = 0.5 against a zero other flow, alpha = 0: res = 0.25.  beta = 0.25: res == thr, consistent.  The next smaller beta: inconsistent"""
    return const_flow(B, H, W, 0.5, 0), np.zeros((B, 2, H, W), F32), 0.0, beta


BETA_BELOW = float(np.nextafter(F32(0.25), F32(0)))


def case_border(B, H, W, ulp=False):
    """every pixel of row 0 targets column W-1 exactly, of row 1 row H-1 exactly, of row 2 column 0 and of row 3 row 0: all inside, and the first two read their
    taps through the clamp.  With ulp the first four pixels of row 0 target one ulp OUTSIDE instead: (0, 0) the float after W-1, (0, 1) the float after H-1
    in y, (0, 2) the float before 0 in x (2 + the float before -2: the sum is exact), (0, 3) -1e-6 in y.  The other rows move by fractions"""
    g = np.random.default_rng(H * W + B)
    xs, ys = grid(B, H, W)
    a = g.uniform(-1.0, 1.0, (B, 2, H, W)).astype(F32)
    a[:, 0, 0], a[:, 1, 0] = F32(W - 1) - xs[:, 0], 0
    a[:, 0, 1], a[:, 1, 1] = 0, F32(H - 1) - ys[:, 1]
    a[:, 0, 2], a[:, 1, 2] = -xs[:, 2], 0
    a[:, 0, 3], a[:, 1, 3] = 0, -ys[:, 3]
    if ulp:
        a[:, :, 0, :4] = 0
        a[:, 0, 0, 0] = np.nextafter(F32(W - 1), F32(np.inf))
        a[:, 1, 0, 1] = np.nextafter(F32(H - 1), F32(np.inf))
        a[:, 0, 0, 2] = np.nextafter(F32(-2), F32(-np.inf))
        a[:, 1, 0, 3] = F32(-1e-6)
    o = g.uniform(-1.0, 1.0, (B, 2, H, W)).astype(F32)
    return a, o, 0.01, 0.5


HOSTILE = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 31, -(2.0 ** 31), 3e9], F32)


def case_hostile_a(B, H, W):
    """NaN, +-inf, 1e30 and 2^31 in one channel of EVERY pixel of a: code 2 everywhere.  o is poison (NaN): it is not read"""
    g = np.random.default_rng(7)
    a = g.uniform(-3, 3, (B, 2, H, W)).astype(F32)
    pick = g.integers(0, 2, (B, H, W))
    vals = HOSTILE[g.integers(0, len(HOSTILE), (B, H, W))]
    a[:, 0] = np.where(pick == 0, vals, a[:, 0])
    a[:, 1] = np.where(pick == 1, vals, a[:, 1])
    return a, np.full((B, 2, H, W), np.nan, F32), 0.01, 0.5


def case_hostile_o(B, H, W):
    """NaN and +-inf sprinkled over o under the taps of a fractional flow: code 1, res +inf, masked NaN there"""
    g = np.random.default_rng(9)
    a = g.uniform(-2.5, 2.5, (B, 2, H, W)).astype(F32)
    o = g.uniform(-2.5, 2.5, (B, 2, H, W)).astype(F32)
    pick = g.random(o.shape) < 0.15
    o[pick] = HOSTILE[:3][g.integers(0, 3, int(pick.sum()))]
    return a, o, 0.01, 0.5


def case_random(B, H, W, seed=3, reach=6.0):
    """random fractional flows of up to +-reach px, the other flow near the negative of the first: all three codes occur, and thousands of pixels whose res bits
    would differ under a fused multiply-add"""
    g = np.random.default_rng(seed)
    a = g.uniform(-reach, reach, (B, 2, H, W)).astype(F32)
    o = (-a + g.normal(0, 0.6, a.shape)).astype(F32)
    return a, o, 0.01, 0.5


CASES = {"consistent": case_consistent, "half": case_half, "threshold": case_threshold, "border": case_border, "hostile_a": case_hostile_a,
         "hostile_o": case_hostile_o, "random": case_random}
SHAPES = ((4, 4), (8, 12), (20, 12), (24, 40), (16, 80), (64, 64))
