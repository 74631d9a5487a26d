"""A NumPy restatement of `cwm_segment_step` (the definition: include/cwm_hip.h, csrc/segment.hip), in loops and float32 operations taken one at a time, and
the builders of the exact-arithmetic inputs the segment tests share.  Test infrastructure only.

Exact arithmetic: every synthetic flow is (0.75 k, 1.0 k) or (3, 4)-proportional with a small integer k, so the magnitudes (1.25 k, 5 k) and the sums of P P
of them are exact in float32 whatever a compiler contracts, and every threshold lies strictly between two attainable values.  Device, CPU composition and this
restatement therefore have to be EQUAL."""
import numpy as np

try:
    from scipy import ndimage as _ndi
except Exception:  # pragma: no cover
    _ndi = None

F32 = np.float32


def components(cand):
    """4-connected labels of a bool image, 0 = background"""
    if _ndi is not None:
        return _ndi.label(cand)[0]
    H, W = cand.shape
    lab = np.zeros((H, W), dtype=np.int64)
    nxt = 0
    for y in range(H):
        for x in range(W):
            if cand[y, x] and not lab[y, x]:
                nxt += 1
                lab[y, x] = nxt
                todo = [(y, x)]
                while todo:
                    cy, cx = todo.pop()
                    for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                        if 0 <= ny < H and 0 <= nx < W and cand[ny, nx] and not lab[ny, nx]:
                            lab[ny, nx] = nxt
                            todo.append((ny, nx))
    return lab


def order(cells, key):
    """`cells` in the selection order: the higher key first, a NaN above every number, -0 equal to +0, the lower index first"""
    def rank(c):
        k = float(key[c])
        return (0, 0.0, c) if k != k else (1, -k + 0.0, c)
    return sorted((int(c) for c in cells), key=rank)


def step(flows, seeds, P, *, min_seed_mag=0.0, abs_thresh=0.0, rel_thresh=0.5, vote_frac=0.5, dirs=None, cos_min=0.0, k_active=0, k_passive=0, inside_frac=1.0,
         ring_radius=1, keys=None, shape=None):
    """flows [B,2,H,W,S] float32 (None: the init step on shape = (B, H, W)); seeds [B,2] (y, x); dirs [S,2] (dy, dx); keys [B,2,n].  Returns a dict of arrays named
    as the outputs of the call (seed_ref: NaN where the sample is not valid)."""
    if flows is None:
        B, H, W = shape
        S = 0
    else:
        flows = np.asarray(flows, dtype=F32)
        B, _, H, W, S = flows.shape
    gh, gw = H // P, W // P
    n = gh * gw
    K = k_active + k_passive
    out = {"seed_ref": np.zeros((B, S), F32), "votes": np.zeros((B, H, W), np.uint8), "segment": np.zeros((B, H, W), np.uint8), "cover": np.zeros((B, gh, gw), F32),
           "stats": np.zeros((B, 4), np.int32), "picks": np.full((B, K), -1, np.int32), "active": np.ones((B, 2 * n), np.uint8), "passive": np.ones((B, 2 * n), np.uint8)}
    out["active"][:, :n] = 0
    out["passive"][:, :n] = 0
    with np.errstate(all="ignore"):
        for b in range(B):
            sy, sx = min(max(int(seeds[b][0]), 0), H - 1), min(max(int(seeds[b][1]), 0), W - 1)
            cy0, cx0 = sy // P, sx // P
            c0 = cy0 * gw + cx0
            n_valid = 0
            votes = np.zeros((H, W), np.int64)
            for s in range(S):
                u, v = flows[b, 0, :, :, s], flows[b, 1, :, :, s]
                m = np.sqrt(u * u + v * v).astype(F32)
                acc = F32(0)
                for r in range(P):
                    for c in range(P):
                        acc = F32(acc + m[cy0 * P + r, cx0 * P + c])
                ref = F32(acc / F32(P * P))
                valid = bool(ref >= F32(min_seed_mag))
                out["seed_ref"][b, s] = ref if valid else np.nan
                if not valid:
                    continue
                n_valid += 1
                ok = m >= np.fmax(F32(abs_thresh), F32(F32(rel_thresh) * ref))
                if dirs is not None:
                    dy, dx = F32(dirs[s][0]), F32(dirs[s][1])
                    dn = np.sqrt(F32(dx * dx + dy * dy)).astype(F32)
                    ok &= (u * dx + v * dy).astype(F32) >= ((F32(cos_min) * m).astype(F32) * dn).astype(F32)
                votes += ok
            out["votes"][b] = votes
            nf = np.ceil(F32(F32(vote_frac) * F32(n_valid)))
            need = max(1, int(nf)) if np.isfinite(nf) else (1 if nf != nf or nf < 0 else 256)
            cand = (votes >= need) & (n_valid > 0)
            lab = components(cand)
            cell = lab[cy0 * P:(cy0 + 1) * P, cx0 * P:(cx0 + 1) * P]
            hit = sorted(set(cell[cell > 0].tolist()))
            seg = np.isin(lab, hit) & cand if hit else np.zeros_like(cand)
            out["segment"][b] = seg
            count = seg.reshape(gh, P, gw, P).sum((1, 3))
            out["cover"][b] = (count.astype(F32) / F32(P * P)).astype(F32)
            out["stats"][b] = (n_valid, int(seg.sum()), int(cand.sum()), int(bool(hit)))
            if k_active <= 0:
                out["active"][b, n:] = 1
                continue
            cover = out["cover"][b].reshape(n)
            inside = cover >= F32(inside_frac)
            touched = count.reshape(n) > 0
            ring = np.zeros(n, bool)
            for c in range(n):
                cy, cx = divmod(c, gw)
                if touched[c]:
                    continue
                for t in np.flatnonzero(touched):
                    ty, tx = divmod(int(t), gw)
                    if max(abs(ty - cy), abs(tx - cx)) <= ring_radius:
                        ring[c] = True
                        break
            ka = np.zeros(n, F32) if keys is None else np.asarray(keys[b][0], F32)
            kp = np.zeros(n, F32) if keys is None else np.asarray(keys[b][1], F32)
            act = [c0] + order([c for c in range(n) if inside[c] and c != c0], ka)[:k_active - 1]
            pas = order(np.flatnonzero(ring), kp)[:k_passive]
            for i, c in enumerate(act):
                out["picks"][b, i] = n + c
                out["active"][b, n + c] = 0
            for i, c in enumerate(pas):
                out["picks"][b, k_active + i] = n + c
                out["passive"][b, n + c] = 0
    return out


# ---- exact inputs -----------------------------------------------------------------------------------------------------------------------------------------
def flows_of(masks, scales, base=(0.75, 1.0)):
    """[1,2,H,W,S] float32: sample s is scales[s] * base on masks[s] (or on the one mask given) and 0 elsewhere"""
    masks = np.asarray(masks, bool)
    if masks.ndim == 2:
        masks = np.broadcast_to(masks, (len(scales),) + masks.shape)
    S, H, W = masks.shape
    f = np.zeros((1, 2, H, W, S), F32)
    for s, k in enumerate(scales):
        f[0, 0, :, :, s] = masks[s] * F32(base[0] * k)
        f[0, 1, :, :, s] = masks[s] * F32(base[1] * k)
    return f


def hand_worked():
    """the 24 x 24 example of the issue: a 16 x 12 block at rows 4-19, cols 2-13 and a block at rows 2-9, cols 18-22 that touches nothing"""
    m = np.zeros((24, 24), bool)
    m[4:20, 2:14] = True
    m[2:10, 18:23] = True
    return flows_of(m, (1, 2, 0, 1, 3)), np.array([[10, 5]], np.int32), dict(min_seed_mag=0.5, abs_thresh=1.0, rel_thresh=0.5, vote_frac=0.6)


def serpentine(H, W):
    """alternate full rows joined at alternating ends: one component that a row-by-row sweep crosses slowly"""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    for i, y in enumerate(range(1, H, 2)):  # (24 x 24: 12 rows of 24 and 12 joints, the last a loose end = 300 pixels)
        m[y, W - 1 if i % 2 == 0 else 0] = True
    return m


def spiral(H, W):
    """a one-pixel path that winds inwards from the top-left corner, a free ring between its turns"""
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    for _ in range(H * W):
        ny, nx = y + dy, x + dx
        ahead2 = (ny + dy, nx + dx)
        blocked = not (0 <= ny < H and 0 <= nx < W) or m[ny, nx] or (0 <= ahead2[0] < H and 0 <= ahead2[1] < W and m[ahead2])
        if blocked:
            dy, dx = dx, -dy
            ny, nx = y + dy, x + dx
            ahead2 = (ny + dy, nx + dx)
            if not (0 <= ny < H and 0 <= nx < W) or m[ny, nx] or (0 <= ahead2[0] < H and 0 <= ahead2[1] < W and m[ahead2]):
                break
        y, x = ny, nx
        m[y, x] = True
    return m


def diagonal_pair(H, W):
    """two blocks that touch only at a corner"""
    m = np.zeros((H, W), bool)
    m[2:8, 2:8] = True
    m[8:14, 8:14] = True
    return m
