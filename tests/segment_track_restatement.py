"""A NumPy restatement of `cwm_segment_track` (the definition: include/cwm_hip.h, csrc/segment_track.hip): a plain loop over the nine steps, written from the
contract, the warp in np.float32 adds and np.rint, the link test in np.float32 operations taken one at a time; and the builders of the inputs the tracking tests
share.  Test infrastructure only.

Every output is an integer, so the device, the torch composition and this restatement have to be EQUAL.

The hand-worked case (`hand_worked()`): image 8 x 12, two calls.  iou_thresh = 0.3, min_inter = 1, min_area = 2, max_age = 1, carry = 1.
  prev    slot 1 = rows 0-3 x cols 1-4, slot 3 = rows 4-7 x cols 8-11.  State: track_id (7, 0, 9, 0 ...), every age 0, next_id 10: two tracks.
  flow    u = +1, v = 0 everywhere: pixel (y, x) looks at (y, x + 1).  w: slot 1 at rows 0-3 x cols 0-3 (16), slot 3 at rows 4-7 x cols 7-10 (16); column 11 looks
          outside.
  cur     label 1 = rows 0-3 x cols 0-4 (20), label 2 = rows 5-7 x cols 0-2 (9), label 3 = the pixel (0, 11) (1): three labels.
  call 1  n[1][1] = 16, n[1][0] = 4, n[2][0] = 9, n[3][0] = 1, n[0][3] = 16, n[0][0] = 50.  (1, 1): 16 > .3 * (20 + 16 - 16) = 6: LINKED.  Slot 3 is not linked,
          area_w = 16, age 0 + 1 <= 1: it COASTS with age 1.  Label 2 (9 >= 2) is BORN into slot 2, the lowest free one, with id 10; label 3 is below min_area:
          dropped.  out: 1 on label 1's 20 pixels, 2 on label 2's 9, 3 on rows 4-7 x cols 7-10.  track_id (7, 10, 9), age (0, 0, 1), next_id 11.
          stats (1 linked, 1 born, 1 coasting, 0 ended, 1 dropped, 3 live, 45 pixels, 0)
  call 2  prev = out of call 1, no flow, the same cur, the state call 1 wrote.  n[1][1] = 20, n[2][2] = 9, n[0][3] = 16, n[3][0] = 1: (1, 1) and (2, 2) are linked;
          slot 3 has age 1 + 1 > 1: it ENDS.  track_id (7, 10, 0), age (0, 0, 0), next_id 11.  stats (2, 0, 0, 1, 1, 2, 29, 0)"""
import numpy as np

F32 = np.float32
S = 64  # slots, and labels


def wrap32(v):
    """two's-complement 32-bit wrap-around of a Python integer"""
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def empty_state(B):
    return {"track_id": np.zeros((B, S), np.int32), "age": np.zeros((B, S), np.int32), "next_id": np.ones((B,), np.int32)}


def track(prev, cur, flow, state, shape, *, iou_thresh=0.3, min_inter=1, min_area=1, max_age=2, carry=1):
    """prev, cur [B,H,W] uint8 or None; flow [B,2,H,W] float32 or None; state: a dict (track_id [B,64], age [B,64], next_id [B]) or None; shape = (B, H, W).
    Returns a dict of arrays named as the outputs of the call (the new state under track_id, age, next_id)."""
    B, H, W = shape
    thr = F32(iou_thresh)
    st = empty_state(B) if state is None else state
    o = {"out": np.zeros((B, H, W), np.uint8), "track_id": np.zeros((B, S), np.int32), "age": np.zeros((B, S), np.int32), "next_id": np.zeros((B,), np.int32),
         "area": np.zeros((B, S), np.int32), "bbox": np.zeros((B, S, 4), np.int32), "moments": np.zeros((B, S, 2), np.int64),
         "slot_of_cur": np.zeros((B, S), np.int32), "linked_cur": np.zeros((B, S), np.int32), "table": np.zeros((B, S + 1, S + 1), np.int32),
         "warped": np.zeros((B, H, W), np.uint8), "stats": np.zeros((B, 8), np.int32)}
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for b in range(B):
        tid_in, age_in, next_in = [int(v) for v in st["track_id"][b]], [int(v) for v in st["age"][b]], int(st["next_id"][b])
        live = [False] + [v != 0 for v in tid_in]  # by slot 1 .. 64
        # 0 inputs
        c = np.zeros((H, W), np.int64) if cur is None else np.asarray(cur[b]).astype(np.int64)
        c[c > S] = 0
        # 1 warp
        w = np.zeros((H, W), np.int64)
        if prev is not None:
            u = np.zeros((H, W), F32) if flow is None else np.asarray(flow[b, 0], F32)
            v = np.zeros((H, W), F32) if flow is None else np.asarray(flow[b, 1], F32)
            with np.errstate(invalid="ignore", over="ignore"):
                rx, ry = np.rint(xs.astype(F32) + u), np.rint(ys.astype(F32) + v)
                inside = (rx >= F32(0)) & (rx <= F32(W - 1)) & (ry >= F32(0)) & (ry <= F32(H - 1))
            sy, sx = np.where(inside, ry, 0).astype(np.int64), np.where(inside, rx, 0).astype(np.int64)
            w = np.where(inside, np.asarray(prev[b]).astype(np.int64)[sy, sx], 0)
            w[w > S] = 0
            w = np.where(np.array(live)[w], w, 0)
        # 2 table
        n = np.zeros((S + 1, S + 1), np.int64)
        np.add.at(n, (c.ravel(), w.ravel()), 1)
        area_cur, area_w = n.sum(1), n.sum(0)
        # 3 link
        cands = []
        with np.errstate(invalid="ignore"):
            for ci in range(1, S + 1):
                for pi in range(1, S + 1):
                    k = int(n[ci, pi])
                    if k >= max(1, min_inter) and F32(k) > thr * F32(int(area_cur[ci]) + int(area_w[pi]) - k):
                        cands.append((-k, (ci - 1) * S + (pi - 1), ci, pi))
        slot_of, linked = [0] * (S + 1), [0] * (S + 1)
        for _ in range(S):
            if not cands:
                break
            _, _, ci, pi = min(cands)  # the higher count first, the lower index first
            slot_of[ci], linked[pi] = pi, ci
            cands = [t for t in cands if t[2] != ci and t[3] != pi]
        # 4 coast or end
        tid_out, age_out, coast, ended = [0] * (S + 1), [0] * (S + 1), [False] * (S + 1), [False] * (S + 1)
        for p in range(1, S + 1):
            if not live[p]:
                continue
            if linked[p]:
                tid_out[p] = tid_in[p - 1]
            elif carry and area_w[p] > 0 and age_in[p - 1] + 1 <= max_age:
                coast[p], tid_out[p], age_out[p] = True, tid_in[p - 1], age_in[p - 1] + 1
            else:
                ended[p] = True
        # 5 births
        free = [p for p in range(1, S + 1) if not live[p] or ended[p]]
        next_id, born = next_in, 0
        for ci in range(1, S + 1):
            if slot_of[ci] or area_cur[ci] < max(1, min_area) or not free:
                continue
            p = free.pop(0)
            slot_of[ci], tid_out[p], age_out[p] = p, wrap32(next_id), 0
            next_id, born = next_id + 1, born + 1
        # 6 paint
        by_label = np.array(slot_of)[c]
        out = np.where(by_label > 0, by_label, np.where(np.array(coast)[w], w, 0))
        # 7 read-outs
        for s in range(1, S + 1):
            yy, xx = np.nonzero(out == s)
            o["area"][b, s - 1] = len(yy)
            o["bbox"][b, s - 1] = (yy.min(), xx.min(), yy.max(), xx.max()) if len(yy) else (0, 0, -1, -1)
            o["moments"][b, s - 1] = (yy.sum(), xx.sum())
        # 8 tables, 9 stats
        o["out"][b], o["warped"][b], o["table"][b] = out, w, n
        o["track_id"][b], o["age"][b], o["next_id"][b] = tid_out[1:], age_out[1:], wrap32(next_id)
        o["slot_of_cur"][b], o["linked_cur"][b] = slot_of[1:], linked[1:]
        dropped = sum(1 for ci in range(1, S + 1) if area_cur[ci] >= 1 and not slot_of[ci])
        o["stats"][b] = (sum(1 for p in linked[1:] if p), born, sum(coast), sum(ended), dropped, sum(1 for t in tid_out[1:] if t != 0), np.count_nonzero(out), 0)
    return o


def new_state(o):
    return {"track_id": o["track_id"], "age": o["age"], "next_id": o["next_id"]}


def sequence(label_maps, back_flows, shape, **kw):
    """label_maps: T entries [B,H,W] or None; back_flows [B,T,2,H,W] or None.  Frame 0 has no previous frame and no flow.  Returns the list of per-frame results."""
    res, state, prev = [], None, None
    for t, cur in enumerate(label_maps):
        r = track(prev, cur, None if t == 0 or back_flows is None else back_flows[:, t], state, shape, **kw)
        res.append(r)
        state, prev = new_state(r), r["out"]
    return res


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------------
def rect(H, W, y0, y1, x0, x1, value=1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = value
    return m


HAND_KW = dict(iou_thresh=0.3, min_inter=1, min_area=2, max_age=1, carry=1)


def hand_worked():
    """(prev [1,8,12], cur [1,8,12], flow [1,2,8,12], state)"""
    prev = (rect(8, 12, 0, 4, 1, 5, 1) + rect(8, 12, 4, 8, 8, 12, 3))[None]
    cur = (rect(8, 12, 0, 4, 0, 5, 1) + rect(8, 12, 5, 8, 0, 3, 2) + rect(8, 12, 0, 1, 11, 12, 3))[None]
    flow = np.zeros((1, 2, 8, 12), F32)
    flow[:, 0] = 1
    state = empty_state(1)
    state["track_id"][0, 0], state["track_id"][0, 2], state["next_id"][0] = 7, 9, 10
    return prev, cur, flow, state


HAND = [{"track_id": [7, 10, 9], "age": [0, 0, 1], "next_id": [11], "stats": [[1, 1, 1, 0, 1, 3, 45, 0]], "area": [20, 9, 16],
         "bbox": [[0, 0, 3, 4], [5, 0, 7, 2], [4, 7, 7, 10]], "moments": [[30, 40], [54, 9], [88, 136]], "slot_of_cur": [1, 2, 0], "linked_cur": [1, 0, 0]},
        {"track_id": [7, 10, 0], "age": [0, 0, 0], "next_id": [11], "stats": [[2, 0, 0, 1, 1, 2, 29, 0]], "area": [20, 9, 0],
         "bbox": [[0, 0, 3, 4], [5, 0, 7, 2], [0, 0, -1, -1]], "moments": [[30, 40], [54, 9], [0, 0]], "slot_of_cur": [1, 2, 0], "linked_cur": [1, 2, 0]}]


def random_maps(seed, B, H, W, n_prev=5, n_cur=5, big_bytes=True):
    """(prev, cur, state): random rectangles painted over each other; slots and labels drawn from 1 .. 64, a few bytes above 64 in both maps; most slots that
    appear in prev are live with random ids and ages 0 .. 3, one of them is free (its pixels count as 0); content differs per row"""
    g = np.random.default_rng(seed)
    prev, cur, state = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.uint8), empty_state(B)

    def paint(m, value):
        y0, x0 = g.integers(0, H - 1), g.integers(0, W - 1)
        y1, x1 = g.integers(y0 + 1, min(H, y0 + max(2, H // 2)) + 1), g.integers(x0 + 1, min(W, x0 + max(2, W // 2)) + 1)
        m[y0:y1, x0:x1] = value

    for b in range(B):
        slots = g.choice(np.arange(1, S + 1), size=min(n_prev, S), replace=False)
        for i, s in enumerate(slots):
            paint(prev[b], s)
            if i != 1:  # (the second slot stays free: a slot byte without a track)
                state["track_id"][b, s - 1], state["age"][b, s - 1] = 100 + int(s), g.integers(0, 4)
        labels = np.arange(1, min(n_cur, S) + 1)
        for c in labels:
            if g.random() < 0.6 and len(slots):  # near where a track is: a shifted copy of a slot's pixels, where it still shows
                src = np.roll(prev[b] == slots[int(c) % len(slots)], tuple(g.integers(-1, 2, 2)), (0, 1))
                cur[b][src] = c
            else:
                paint(cur[b], c)
        if big_bytes:
            paint(prev[b], 65 + int(g.integers(0, 190)))
            cur[b, g.integers(0, H), g.integers(0, W)] = 200
        state["next_id"][b] = 1000 + b
    return prev, cur, state


def flows(kind, seed, B, H, W):
    """[B,2,H,W] float32: "int" piecewise integer motion, "half" integers plus one half (the tie rule of rintf), "special" NaN, +-inf and +-1e30 sprinkled over
    integer motion, "frac" arbitrary fractions"""
    g = np.random.default_rng(seed)
    f = np.zeros((B, 2, H, W), F32)
    for b in range(B):
        for ch in range(2):
            f[b, ch] = g.integers(-2, 3)
            f[b, ch, :H // 2, W // 3:] = g.integers(-3, 4)
    if kind == "half":
        f += F32(0.5)
        f[:, :, ::2] -= F32(1.0)  # -0.5 and +0.5 offsets: half to even rounds both ways
    elif kind == "frac":
        f += g.uniform(-1.5, 1.5, f.shape).astype(F32)
    elif kind == "special":
        vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9, 2.0 ** 31, -(2.0 ** 31)], F32)
        pick = g.random(f.shape) < 0.3
        f[pick] = vals[g.integers(0, len(vals), int(pick.sum()))]
    elif kind != "int":
        raise ValueError(kind)
    return f


def full_table(B, H, W):
    """every slot live and present in prev (so none is free), cur with labels nowhere near them: every label wants a birth and every one is dropped"""
    prev, cur, state = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.uint8), empty_state(B)
    prev[:, 0, :] = (np.arange(W) % S) + 1  # one row of slot bytes
    state["track_id"][:] = np.arange(1, S + 1) + 500
    state["next_id"][:] = 900
    cur[:, H // 2:, :W // 2], cur[:, H // 2:, W // 2:] = 1, 2
    return prev, cur, state


def garbage_state(seed, B):
    g = np.random.default_rng(seed)
    big = lambda *s: g.integers(-2 ** 31, 2 ** 31, s, dtype=np.int64).astype(np.int32)  # noqa: E731
    return {"track_id": big(B, S), "age": big(B, S), "next_id": np.array([2 ** 31 - 1, -5, 0][:B] + [7] * max(0, B - 3), np.int32)}


def largest():
    """512 x 512: 64 slots and 64 labels, an 8 x 8 grid of 48 x 48 squares in cells of 64; the labels are the slots' squares moved by (3, 2) and renumbered in
    reverse; the flow is (2, 3) so that each label meets its own slot's warped square by 48 x 48 less an L of 1 pixel"""
    H = W = 512
    prev, cur, state = np.zeros((1, H, W), np.uint8), np.zeros((1, H, W), np.uint8), empty_state(1)
    for i in range(8):
        for j in range(8):
            s = i * 8 + j + 1
            prev[0, 64 * i + 8:64 * i + 56, 64 * j + 8:64 * j + 56] = s
            cur[0, 64 * i + 5:64 * i + 53, 64 * j + 6:64 * j + 54] = S + 1 - s
    state["track_id"][0] = np.arange(1, S + 1) * 3
    state["next_id"][0] = 1000
    flow = np.zeros((1, 2, H, W), F32)
    flow[0, 0], flow[0, 1] = 3, 2  # w's squares sit at (64 i + 6, 64 j + 5): one pixel off the labels' both ways
    return prev, cur, flow, state
