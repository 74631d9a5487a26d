"""A NumPy restatement of `cwm_object_response` (the definition: include/cwm_hip.h, csrc/object_response.hip) -- steps 1 to 8 as written there, int64 sums and the
coupling as np.float64 operations, one per line --, of `object_response.relations` / `groups`, and the cases the object-response tests share.  Written from the
definition and independent of the torch composition.  Test infrastructure only.

The device, the torch composition and this restatement have to be EQUAL: the integer tables by value, the coupling as int64 bit patterns (`bits`)."""
import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
SIDE = 65
NAMES = ("tab", "valid", "agg", "coupling", "stats")
COMPASS = ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, -1), (-1, 1))  # (dy, dx): E, S, W, N, SE, SW, NW, NE


def bits(a):
    """the bit patterns of a float64 array (other dtypes are returned as they are)"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def dirs_of(S, step=8):
    """[S,2] int32 (dy, dx): the compass cycled, in pixels"""
    return np.array([(COMPASS[s % 8][0] * step, COMPASS[s % 8][1] * step) for s in range(S)], np.int32)


def min_q2_of(min_mag):
    return int(round(float(min_mag) * 256.0)) ** 2


def response(flows, labels, pushed, dirs=None, min_mag=1.0, min_pixels=1, self_frac=0.5, move_frac=0.5):
    """flows [R,2,H,W,S] float32, labels [R,H,W] uint8 (one map per ROW), pushed [R] int, dirs [S,2] int (dy, dx) or None -> dict of tab int64 [R,S,65,8],
    valid uint8 [R,S], agg int64 [R,65,4], coupling float64 [R,65,4], stats int32 [R,4]"""
    flows, labels, pushed = np.asarray(flows, F32), np.asarray(labels, np.uint8), np.asarray(pushed, I64).reshape(-1)
    R, _, H, W, S = flows.shape
    assert labels.shape == (R, H, W) and pushed.shape == (R,)
    min_q2 = min_q2_of(min_mag)
    tab = np.zeros((R, S, SIDE, 8), I64)
    # 1 slot
    l = labels.astype(I64)
    l = np.where(l > 64, 0, l)
    rows = np.broadcast_to(np.arange(R)[:, None, None], (R, H, W))
    for s in range(S):
        # 2 usable
        u, v = flows[:, 0, :, :, s], flows[:, 1, :, :, s]
        with np.errstate(invalid="ignore"):
            usable = (np.abs(u) <= F32(4096)) & (np.abs(v) <= F32(4096))
        np.add.at(tab[:, s, :, 7], (rows[~usable], l[~usable]), 1)
        # 3 quantise
        pu, pv = (u[usable] * F32(256)), (v[usable] * F32(256))
        assert pu.dtype == F32
        qu, qv = np.rint(pu).astype(I64), np.rint(pv).astype(I64)
        q2 = qu * qu + qv * qv
        moved = q2 >= min_q2
        # 4 table
        at = (rows[usable], l[usable])
        for i, t in enumerate((np.ones_like(qu), moved.astype(I64), qu, qv, np.where(moved, qu, 0), np.where(moved, qv, 0), q2)):
            np.add.at(tab[:, s, :, i], at, t)
    valid = np.zeros((R, S), np.uint8)
    agg = np.zeros((R, SIDE, 4), I64)
    coupling = np.zeros((R, SIDE, 4), F64)
    stats = np.zeros((R, 4), np.int32)
    for r in range(R):
        a = int(pushed[r])
        alive = 1 <= a <= 64
        # 5 valid samples
        for s in range(S):
            if not alive:
                continue
            na, ma = tab[r, s, a, 0], tab[r, s, a, 1]
            if na >= min_pixels and F64(ma) / F64(na) >= F64(self_frac):
                valid[r, s] = 1
        n_valid = int(valid[r].sum())
        # 6 aggregate
        for s in range(S):
            if not valid[r, s]:
                continue
            n, m, su, sv = (tab[r, s, :, i] for i in range(4))
            agg[r, :, 0] += n
            agg[r, :, 1] += m
            if dirs is not None:
                agg[r, :, 2] += su * int(dirs[s][1]) + sv * int(dirs[s][0])
            some = n > 0
            frac = m[some].astype(F64) / n[some].astype(F64)
            agg[r, np.nonzero(some)[0][frac >= F64(move_frac)], 3] += 1
        # 7 coupling
        N, M, A, V = (agg[r, :, i] for i in range(4))
        for l_ in range(SIDE):
            if n_valid > 0:
                coupling[r, l_, 0] = F64(V[l_]) / F64(n_valid)
            if N[l_] != 0:
                mean = F64(A[l_]) / F64(N[l_])
                coupling[r, l_, 1] = F64(M[l_]) / F64(N[l_])
                coupling[r, l_, 2] = mean * F64(2.0 ** -8)
                if alive and N[a] != 0 and A[a] != 0:
                    den = F64(A[a]) / F64(N[a])
                    coupling[r, l_, 3] = mean / den
        # 8 stats
        stats[r] = (n_valid, a if alive else 0, tab[r, 0, a, 0] + tab[r, 0, a, 7] if alive else 0, 0)
    return {"tab": tab, "valid": valid, "agg": agg, "coupling": coupling, "stats": stats}


def relations(coupling, stats, slots, has_dirs=True, min_vote=0.5, min_gain=0.25):
    """coupling [B,K,65,4], stats [B,K,4], slots [B,K] -> (moves [B,65,65], mutual, carries, tested [B,65]) bool"""
    B, K = coupling.shape[:2]
    moves, tested = np.zeros((B, SIDE, SIDE), bool), np.zeros((B, SIDE), bool)
    for b in range(B):
        for k in range(K):
            a = int(slots[b][k])
            if not 1 <= a <= 64 or stats[b, k, 0] <= 0:
                continue
            tested[b, a] = True
            for l in range(1, SIDE):
                if l != a and coupling[b, k, l, 0] >= min_vote and (not has_dirs or coupling[b, k, l, 3] >= min_gain):
                    moves[b, a, l] = True
    back = moves.transpose(0, 2, 1)
    return moves, moves & back, moves & ~back & tested[:, None, :], tested


def groups(mutual):
    """[B,65] int32: the lowest slot reachable over mutual links (a flood fill per slot)"""
    B = mutual.shape[0]
    out = np.zeros((B, SIDE), np.int32)
    for b in range(B):
        link = mutual[b] | mutual[b].T
        for a in range(SIDE):
            seen, todo = {a}, [a]
            while todo:
                c = todo.pop()
                for d in np.nonzero(link[c])[0]:
                    if int(d) not in seen:
                        seen.add(int(d))
                        todo.append(int(d))
            out[b, a] = min(seen)
    return out


# ---- the shared cases: each returns (flows [R,2,H,W,S], labels [B,H,W], pushed [R]) with R = B K -------------------------------------------------------------
HOSTILE = np.array([np.nan, np.inf, -np.inf, 5000.0, -4096.5, 4096.0, -4096.0], F32)


def per_row(labels, K):
    """[B,H,W] -> [B K,H,W]: the map of scene b for each of its K pushes"""
    return np.repeat(labels, K, 0)


def case_random(B, K, H, W, S, seed=3, top=80, min_mag=1.0):
    """labels in blocks of 4 x 8 pixels drawn from 0 .. top (values above 64 occur and read as 0) with single pixels redrawn; flows of up to +-3 px, some exact
    multiples of 1/256; NaN, +-inf, 5000, -4096.5 and +-4096 exactly sprinkled over one channel; one image row of every plane holds magnitudes that straddle
    the threshold: q2 = min_q2 exactly, one step below and one above.  pushed: random slots, with 0, 65 and -3 among them when there are enough rows"""
    g = np.random.default_rng(seed)
    R = B * K
    blocks = g.integers(0, top + 1, (B, (H + 3) // 4, (W + 7) // 8))
    labels = np.repeat(np.repeat(blocks, 4, 1), 8, 2)[:, :H, :W].copy()
    pick = g.random(labels.shape) < 0.05
    labels[pick] = g.integers(0, top + 1, int(pick.sum()))
    flows = g.uniform(-3, 3, (R, 2, H, W, S)).astype(F32)
    flows[:, :, ::3, ::5] = np.round(flows[:, :, ::3, ::5] * 256) / 256
    bad = g.random((R, H, W, S)) < 0.04
    r, y, x, s = np.nonzero(bad)
    flows[r, g.integers(0, 2, len(r)), y, x, s] = HOSTILE[g.integers(0, len(HOSTILE), len(r))]
    q = int(round(min_mag * 256))
    flows[:, 0, 1, :, :] = (np.array([q, q - 1, q + 1, -q], F32) / 256)[np.arange(W) % 4][None, :, None]
    flows[:, 1, 1, :, :] = 0
    pushed = g.integers(1, 65, R)
    if R >= 4:
        pushed[1], pushed[2], pushed[3] = 0, 65, -3
    return flows, labels.astype(np.uint8), pushed.astype(np.int32)


def case_rows(B, K, H, W, S, seed=5):
    """whole image rows of one slot (the slot changes every two rows): every wave of 256 pixels holds few slots"""
    g = np.random.default_rng(seed)
    labels = np.broadcast_to(((np.arange(H) // 2) % 65)[None, :, None], (B, H, W)).astype(np.uint8)
    flows = (g.integers(-512, 513, (B * K, 2, H, W, S)) / 256).astype(F32)
    return flows, labels.copy(), ((np.arange(B * K) * 7) % (min(65, H // 2) - 1) + 1).astype(np.int32)


def case_checker(B, K, H, W, S, seed=6):
    """a label change at every pixel and all 64 slots (and 0) live: no wave and no lane holds one slot"""
    g = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    labels = np.broadcast_to(((ys * 7 + xs) % 65)[None], (B, H, W)).astype(np.uint8)
    flows = (g.integers(-768, 769, (B * K, 2, H, W, S)) / 256).astype(F32)
    return flows, labels.copy(), ((np.arange(B * K) * 11) % 64 + 1).astype(np.int32)


def scene_labels(B, H, W):
    """three objects: slot 1 and slot 2 side by side, slot 3 apart from them"""
    labels = np.zeros((B, H, W), np.uint8)
    labels[:, H // 8:H // 2, W // 8:3 * W // 8] = 1
    labels[:, H // 8:H // 2, 3 * W // 8:5 * W // 8] = 2
    labels[:, 5 * H // 8:7 * H // 8, W // 4:W // 2] = 3
    return labels


def case_scene(B, H, W, S, step=8):
    """K = 3 pushes per scene, row b 3 + k pushes slot k + 1; every flow is an exact multiple of 1/256 px.  In sample s the pushed slot moves by 2.5 px along
    COMPASS[s % 8] (the direction of dirs_of(S, step)); slots 1 and 2 move together whichever of the two is pushed (the other at gain 3/4); slot 3 moves only
    when it is pushed, and then slot 2 moves at half gain.  In sample r % S of row r nothing moves: n_valid = S - 1.  Returns flows, labels, pushed, dirs"""
    K = 3
    labels = scene_labels(B, H, W)
    flows = np.zeros((B * K, 2, H, W, S), F32)
    for r in range(B * K):
        b, a = r // K, r % K + 1
        gain = {1: {1: 1.0, 2: 0.75}, 2: {1: 0.75, 2: 1.0}, 3: {3: 1.0, 2: 0.5}}[a]
        for s in range(S):
            if s == r % S:
                continue
            dy, dx = COMPASS[s % 8]
            for l, gn in gain.items():
                flows[r, 0, :, :, s][labels[b] == l] = F32(2.5 * gn * dx)
                flows[r, 1, :, :, s][labels[b] == l] = F32(2.5 * gn * dy)
    assert np.array_equal(flows * 256, np.rint(flows * 256))
    return flows, labels, np.tile(np.arange(1, K + 1, dtype=np.int32), B), dirs_of(S, step)


def push_masks(labels, slots, P, k_active=4, k_passive=4, ring_radius=1, keys=None):
    """`object_response.push_masks` cell by cell: labels [B,H,W], slots [B,K], keys [B,K,n] or None -> active, passive bool [B,K,2n] (0 = picked), pushed [B,K]"""
    B, H, W = labels.shape
    K, gh, gw = slots.shape[1], H // P, W // P
    n = gh * gw
    active, passive = np.ones((B, K, 2 * n), bool), np.ones((B, K, 2 * n), bool)
    active[..., :n], passive[..., :n] = False, False
    pushed = np.zeros((B, K), np.int32)
    for b in range(B):
        lab = np.where(labels[b] > 64, 0, labels[b])
        cell = lambda m: m.reshape(gh, P, gw, P).sum((1, 3)).reshape(-1)  # noqa: E731
        occupied = cell(lab > 0) > 0
        for k in range(K):
            a = int(slots[b][k])
            count = cell(lab == a) if 1 <= a <= 64 else np.zeros(n, np.int64)
            touched = [i for i in range(n) if count[i] > 0]
            if not touched:
                continue
            pushed[b, k] = a
            rank = (lambda i: (-float(np.float32(count[i])), i)) if keys is None else (lambda i: (-float(keys[b, k, i]), i))
            for i in sorted(touched, key=rank)[:k_active]:
                active[b, k, n + i] = False
            ring = [i for i in range(n) if not occupied[i] and any(max(abs(i // gw - j // gw), abs(i % gw - j % gw)) <= ring_radius for j in touched)]
            for i in ring[:k_passive]:
                passive[b, k, n + i] = False
    return active, passive, pushed
