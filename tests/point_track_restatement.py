"""A NumPy restatement of `cwm_point_track` (the definition: include/cwm_hip.h, csrc/point_track.hip): steps 1 to 5 as written there, in scalar loops over rows,
points and frames with np.float32 / np.float64 scalars, so that every step is one rounded operation (NumPy has no fused multiply-add), and the cases the
point-track tests share.  Test infrastructure only.

The device, the torch composition and this restatement have to be EQUAL: state, under and owner by value, xy as int32 bit patterns (`bits`), NaN included."""
import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
SIDE = 65
NAMES = ("xy", "state", "under", "owner")
QNAN = np.array([0x7fc00000], np.int32).view(F32)[0]


def bits(a):
    """the bit patterns of a float32 array (other dtypes are returned as they are)"""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _inside(x, y, W, H):
    return bool(x >= F32(0) and x <= F32(W - 1) and y >= F32(0) and y <= F32(H - 1))


def _sample(flow, px, py, W, H):
    """both channels of flow [2,H,W] at an inside point: step 2 of cwm_flow_consistency"""
    x0f, y0f = np.floor(px), np.floor(py)
    wx, wy = px - x0f, py - y0f
    ix0, iy0 = int(x0f), int(y0f)
    ix1, iy1 = min(ix0 + 1, W - 1), min(iy0 + 1, H - 1)
    out = []
    for c in range(2):
        o00, o01, o10, o11 = flow[c, iy0, ix0], flow[c, iy0, ix1], flow[c, iy1, ix0], flow[c, iy1, ix1]
        d = o01 - o00
        d = wx * d
        top = o00 + d
        d = o11 - o10
        d = wx * d
        bot = o10 + d
        d = bot - top
        d = wy * d
        s = top + d
        assert type(s) is F32 and type(wx) is F32
        out.append(s)
    return out


def track(fwd, points, bwd=None, labels=None, model=None, start=None, alpha=0.01, beta=0.5, max_coast=8):
    """fwd / bwd [B,T-1,2,H,W] float32, labels [B,T,H,W] uint8, model [B,T,65,12] float64, points [B,K,2] float32, start [B,K] int -> dict of xy float32
    [B,T,K,2], state, under uint8 [B,T,K], owner uint8 [B,K]"""
    fwd, points = np.asarray(fwd, F32), np.asarray(points, F32)
    bwd = None if bwd is None else np.asarray(bwd, F32)
    model = None if model is None else np.asarray(model, F64)
    assert model is None or labels is not None
    B, T, H, W = fwd.shape[0], fwd.shape[1] + 1, fwd.shape[3], fwd.shape[4]
    K = points.shape[1]
    alpha, beta = F32(alpha), F32(beta)
    xy = np.full((B, T, K, 2), QNAN, F32)
    state = np.full((B, T, K), 255, np.uint8)
    under = np.zeros((B, T, K), np.uint8)
    owner = np.zeros((B, K), np.uint8)
    with np.errstate(all="ignore"):
        for b in range(B):
            for k in range(K):
                s = 0 if start is None else int(start[b, k])
                if s < 0 or s >= T:
                    continue  # never started
                px, py = points[b, k, 0], points[b, k, 1]
                last = (F32(0), F32(0))
                run, own, coasted = 0, 0, False
                for t in range(s, T):
                    # 1 inside
                    if not _inside(px, py, W, H):
                        state[b, t:, k] = 2
                        break
                    # 2 under
                    un = 0
                    if labels is not None:
                        un = int(labels[b, t, int(np.rint(py)), int(np.rint(px))])
                        un = un if un <= 64 else 0
                    if t == s:
                        own = un
                        owner[b, k] = own
                    # 3 hidden
                    hidden = (un != own) if labels is not None else (t > s and coasted)
                    run = run + 1 if hidden else 0
                    if run > max_coast:
                        state[b, t:, k] = 3
                        break
                    state[b, t, k], under[b, t, k] = (1 if hidden else 0), un
                    xy[b, t, k, 0], xy[b, t, k, 1] = px, py
                    if t == T - 1:
                        break
                    # 4 flow
                    moved = False
                    if un == own:
                        a0, a1 = _sample(fwd[b, t], px, py, W, H)
                        usable = bool(np.abs(a0) <= F32(4096) and np.abs(a1) <= F32(4096))
                        qx, qy = px + a0, py + a1
                        if usable and not _inside(qx, qy, W, H):
                            px, py, moved, coasted = qx, qy, True, False  # leaves
                        elif usable:
                            ok = True
                            if bwd is not None:
                                o0, o1 = _sample(bwd[b, t], qx, qy, W, H)
                                ru, rv = a0 + o0, a1 + o1
                                ru2, rv2 = ru * ru, rv * rv
                                res = ru2 + rv2
                                aa0, aa1, oo0, oo1 = a0 * a0, a1 * a1, o0 * o0, o1 * o1
                                m_a, m_o = aa0 + aa1, oo0 + oo1
                                mag = m_a + m_o
                                thr = alpha * mag
                                thr = thr + beta
                                assert type(thr) is F32 and type(res) is F32
                                ok = bool(res <= thr)
                            if ok:
                                px, py, last, moved, coasted = qx, qy, (a0, a1), True, False
                    # 5 coast
                    if not moved:
                        c0, c1 = last
                        if model is not None:
                            m = model[b, t, own]
                            if bool(m[0] >= F64(1)):
                                dx, dy = F64(px) - m[7], F64(py) - m[8]
                                e0, e1 = m[3] * dx, m[4] * dy
                                cu = e0 + e1
                                cu = m[1] + cu
                                e0, e1 = m[5] * dx, m[6] * dy
                                cv = e0 + e1
                                cv = m[2] + cv
                                assert type(cu) is F64 and type(cv) is F64
                                f0, f1 = F32(cu), F32(cv)
                                if np.isfinite(f0) and np.isfinite(f1):
                                    c0, c1 = f0, f1
                        px, py, coasted = px + c0, py + c1, True
                    assert type(px) is F32 and type(py) is F32
    return {"xy": xy, "state": state, "under": under, "owner": owner}


# ---- the shared cases --------------------------------------------------------------------------------------------------------------------------------------
SUBSETS = [dict(bwd=bw, labels=lb, model=md, start=st) for bw in (False, True) for lb, md in ((False, False), (True, False), (True, True)) for st in (False, True)]


def pick(case, bwd=True, labels=True, model=True, start=True):
    """the keyword arguments of a subset of a case's optional inputs"""
    return {k: (case[k] if on else None) for k, on in (("bwd", bwd), ("labels", labels), ("model", model), ("start", start))}


def case_passing(T=8, W=64):
    """64 x 64, T = 8: slot 0 a static background, slot 1 a 16 x 16 square at x in [4 + 4t, 20 + 4t), y in [24, 40), moving +4 px per frame, slot 2 a static pillar
    at x in [32, 40), y in [16, 48) painted over slot 1.  fwd[t] = (4, 0) on frame t's slot-1 pixels, bwd[t] = (-4, 0) on frame t+1's slot-1 pixels, 0 elsewhere.
    The models come from `object_motion.measure_torch` on the forward pairs with the codes of `flow_consistency.check_torch` (entry T-1 zeros, as
    `TrackedScene.motion` has it).  T and W are parameters for the one property the 8 frames of 64 px cannot show: a point that leaves the frame"""
    import torch

    from counterfactualworldmodels_amd import flow_consistency as FC, object_motion as OM

    H = 64
    labels = np.zeros((1, T, H, W), np.uint8)
    for t in range(T):
        labels[0, t, 24:40, min(4 + 4 * t, W):min(20 + 4 * t, W)] = 1
        labels[0, t, 16:48, 32:40] = 2
    fwd, bwd = np.zeros((1, T - 1, 2, H, W), F32), np.zeros((1, T - 1, 2, H, W), F32)
    for t in range(T - 1):
        fwd[0, t, 0][labels[0, t] == 1] = 4
        bwd[0, t, 0][labels[0, t + 1] == 1] = -4
    lt, ft, bt = torch.from_numpy(labels), torch.from_numpy(fwd), torch.from_numpy(bwd)
    code = FC.check_torch(ft, bt).code
    m = OM.measure_torch(lt[:, :-1], ft, code=code, other=lt[:, 1:]).model
    model = torch.cat([m, torch.zeros_like(m[:, :1])], 1).numpy()
    points = np.array([[[12, 32], [19, 32], [50, 8], [35, 20]]], F32)  # on the square, on its rightmost column, on the background, on the pillar
    return dict(fwd=fwd, bwd=bwd, labels=labels, model=model, points=points, start=None)


def case_random(B, T, H, W, K, seed):
    """smooth random flows of a few pixels with planted NaN, inf and 1e9 vectors; random slot maps in blocks with values above 64; random models with valid 0, 1
    and 2 (and 1.5, -1) and planted NaN entries; points that are NaN, inf and outside the frame, points with integer and half-integer coordinates (the rintf
    ties), points exactly on column W-1 and row H-1; starts throughout 0 .. T-1"""
    g = np.random.default_rng(seed)

    def smooth():
        coarse = g.uniform(-3, 3, (B, T - 1, 2, (H + 7) // 8 + 1, (W + 7) // 8 + 1))
        f = np.repeat(np.repeat(coarse, 8, 3), 8, 4)[..., :H, :W] + g.uniform(-0.25, 0.25, (B, T - 1, 2, H, W))
        f = f.astype(F32)
        bad = g.random((B, T - 1, H, W)) < 0.03
        b, t, y, x = np.nonzero(bad)
        f[b, t, g.integers(0, 2, len(b)), y, x] = np.array([np.nan, np.inf, -np.inf, 1e9, -1e9, 4096.5], F32)[g.integers(0, 6, len(b))]
        return f

    fwd, bwd = smooth(), smooth()
    bwd[:, :, :, ::2] = -fwd[:, :, :, ::2]  # (half of the image rows nearly consistent, so that both outcomes of the test occur)
    blocks = g.integers(0, 6, (B, T, (H + 3) // 4, (W + 7) // 8))
    labels = np.repeat(np.repeat(blocks, 4, 2), 8, 3)[..., :H, :W].copy()
    stray = g.random(labels.shape) < 0.05
    labels[stray] = g.integers(0, 256, int(stray.sum()))
    labels = labels.astype(np.uint8)
    model = np.zeros((B, T, SIDE, 12), F64)
    model[..., 0] = g.choice(np.array([0.0, 1.0, 2.0, 2.0, 1.5, -1.0]), (B, T, SIDE))
    model[..., 1:3] = g.uniform(-3, 3, (B, T, SIDE, 2))
    model[..., 3:7] = g.uniform(-0.05, 0.05, (B, T, SIDE, 4)) * (model[..., :1] >= 2)
    model[..., 7], model[..., 8] = g.uniform(0, W, (B, T, SIDE)), g.uniform(0, H, (B, T, SIDE))
    hurt = g.random((B, T, SIDE)) < 0.15
    b, t, l = np.nonzero(hurt)
    model[b, t, l, g.integers(0, 9, len(b))] = np.array([np.nan, np.inf, 1e300, -1e300])[g.integers(0, 4, len(b))]
    points = np.stack([g.uniform(0, W - 1, (B, K)), g.uniform(0, H - 1, (B, K))], -1).astype(F32)
    kind = g.integers(0, 10, (B, K))
    points[kind == 0] = np.rint(points[kind == 0])  # integers
    points[kind == 1] = np.minimum(np.floor(points[kind == 1]) + F32(0.5), F32(min(H, W) - 1))  # half-integers: the ties of rintf
    points[kind == 2, 0] = W - 1  # exactly on the last column
    points[kind == 3, 1] = H - 1  # exactly on the last row
    special = np.array([[np.nan, 1], [1, np.nan], [np.inf, 0], [-1, 2], [2, -0.5], [W - 0.5, 1], [1, H], [-0.0, 0.0], [1e9, 1e9]], F32)
    if K >= 63:
        for i, sp in enumerate(special):
            points[i % B, (3 + 7 * i) % K] = sp
    start = g.integers(0, T, (B, K)).astype(np.int32)
    start[:, ::3] = 0
    return dict(fwd=fwd, bwd=bwd, labels=labels, model=model, points=points, start=start)
