"""The prompt kernels of csrc/elementwise.hip restated as plain loops over numpy arrays (no GPU, no vectorisation): what include/cwm_hip.h says
`cwm_multi_shift_prompts` and `cwm_prompt_table_expand` compute, one pixel / one cell at a time.

tests/test_prompt_kernels_cpu.py pins this file to the reference's recorded outputs (every case of tests/golden/multi_shift.npz, bit for bit) and to
`oracle.vmae_oracle.create_motion_counterfactuals`; tests/test_prompt_kernels_gpu.py then holds the kernels against it at geometries the recordings
do not have (per-row tables, T = 3, C = 1 / 5, several prompts per movie).

Tables are the C entry point's: R = B S rows in '(b s)' order (row i reads movie i // S), Nt = T gh gw cells, n = gh gw,
    points [R,K,Nt] bool   non-zero = step k moves this patch (only those of frame `frame` move)
    masks  [R,Km,Nt] bool  base masks, Km = K or 1 (one mask for every step), or None
    shifts [R,K,2] int     (sy, sx) in pixels
"""
import numpy as np


def patch_shift(s, P):
    """Whole patches a pixel shift moves the mask by: truncated toward zero (-3 px at P = 8 is 0 patches, not -1)."""
    s = int(s)
    return (abs(s) // P) if s >= 0 else -(abs(s) // P)


def multi_shift_sources(points, shifts, P, frame, T, H, W):
    """Per row and pixel of frame `frame`, the position the output pixel is read from: int array [R,H,W,2] of (cy, cx), (-1, -1) where the walk left the
    image (the pixel is 0).  For every pixel keep (cy, cx) = (y, x) and walk the steps backwards, k = K - 1 .. 0: if the cell (cy // P - my_k, cx // P - mx_k)
    is inside the grid and step k moves it, (cy, cx) -= (sy_k, sx_k); a position outside the image ends the walk."""
    R, K, Nt = points.shape
    gh, gw = H // P, W // P
    n = gh * gw
    assert Nt == T * n and shifts.shape == (R, K, 2) and 0 <= frame < T
    src = np.empty((R, H, W, 2), dtype=np.int64)
    for i in range(R):
        for y in range(H):
            for x in range(W):
                cy, cx = y, x
                for k in range(K - 1, -1, -1):
                    sy, sx = int(shifts[i, k, 0]), int(shifts[i, k, 1])
                    pi, pj = cy // P - patch_shift(sy, P), cx // P - patch_shift(sx, P)
                    if 0 <= pi < gh and 0 <= pj < gw and points[i, k, frame * n + pi * gw + pj]:
                        cy, cx = cy - sy, cx - sx
                        if not (0 <= cy < H and 0 <= cx < W):
                            cy = cx = -1
                            break
                src[i, y, x] = (cy, cx)
    return src


def multi_shift_frames(x, points, shifts, P, frame, S=1, fix_passive=0, sources=None):
    """x [B,T,C,H,W] float32 -> x_out [R,T,C,H,W]: frames other than `frame` are copies (of frame 0 when fix_passive), frame `frame` is read through
    `multi_shift_sources`; a later step wins where destinations overlap because the walk meets it first."""
    B, T, Cc, H, W = x.shape
    R = points.shape[0]
    assert R == B * S and fix_passive in (0, 1)
    src = multi_shift_sources(points, shifts, P, frame, T, H, W) if sources is None else sources
    out = np.empty((R, T, Cc, H, W), dtype=x.dtype)
    for i in range(R):
        b = i // S
        for t in range(T):
            ft = 0 if fix_passive else t
            if t != frame:
                out[i, t] = x[b, ft]
                continue
            for y in range(H):
                for xx in range(W):
                    cy, cx = src[i, y, xx]
                    for c in range(Cc):
                        out[i, t, c, y, xx] = x[b, ft, c, cy, cx] if cy >= 0 else 0.0
    return out


def multi_shift_mask(points, masks, shifts, P, frame, T, H, W):
    """mask_out [R,Nt] = AND_k step_k; step_k = (M_k | A_k) & shifted_k with base masks, shifted_k without; shifted_k = !A_k moved by (my_k, mx_k)
    patches in frame `frame` (a cell whose source is outside the grid is masked), !A_k in the other frames."""
    R, K, Nt = points.shape
    gh, gw = H // P, W // P
    n = gh * gw
    assert Nt == T * n and (masks is None or masks.shape in ((R, K, Nt), (R, 1, Nt)))
    out = np.empty((R, Nt), dtype=bool)
    for i in range(R):
        for tau in range(Nt):
            t, hw = tau // n, tau % n
            keep = True
            for k in range(K):
                a = bool(points[i, k, tau])
                shifted = not a
                if t == frame:
                    pi, pj = hw // gw - patch_shift(shifts[i, k, 0], P), hw % gw - patch_shift(shifts[i, k, 1], P)
                    shifted = (not points[i, k, frame * n + pi * gw + pj]) if (0 <= pi < gh and 0 <= pj < gw) else True
                step = shifted
                if masks is not None:
                    m = bool(masks[i, 0 if masks.shape[1] == 1 else k, tau])
                    step = (m or a) and shifted
                keep = keep and step
            out[i, tau] = keep
    return out


def prompt_table_expand(table, T, gh, gw, frame):
    """table [S,4] rows (h, w, dy, dx) -> (active [S,Nt], passive [S,Nt], shifts [S,2]).  passive: frame 0 visible (0), later frames masked (1).
    active: passive with cell (h, w) of frame `frame` cleared when 0 <= h < gh and 0 <= w < gw; a cell outside the grid clears nothing.  The shifts are
    copied whatever the cell is."""
    S = table.shape[0]
    n = gh * gw
    passive = np.empty((S, T * n), dtype=bool)
    for i in range(S):
        for tau in range(T * n):
            passive[i, tau] = tau >= n
    active = passive.copy()
    shifts = np.empty((S, 2), dtype=np.int32)
    for i in range(S):
        h, w = int(table[i, 0]), int(table[i, 1])
        if 0 <= h < gh and 0 <= w < gw:
            active[i, frame * n + h * gw + w] = False
        shifts[i, 0], shifts[i, 1] = table[i, 2], table[i, 3]
    return active, passive, shifts


def tables_of_golden_case(g, c, tag):
    """A `case_*` record of multi_shift.npz (the reference's [B,Nt,K] layout) -> (points [B,K,Nt], masks [B,Km,Nt] | None, shifts [B,K,2]) as the C entry
    point takes them: without points the reference moves the visible patches of each step's mask and has no base mask."""
    masks = g["case_%s_masks" % tag]
    m3 = masks if masks.ndim == 3 else masks[..., None]
    shifts = g["case_%s_shifts" % tag]
    if c["has_points"]:
        points, base = g["case_%s_points" % tag].transpose(0, 2, 1), m3.transpose(0, 2, 1)
    else:
        points, base = ~m3.transpose(0, 2, 1), None
    return np.ascontiguousarray(points), None if base is None else np.ascontiguousarray(base), np.broadcast_to(shifts[None], (masks.shape[0],) + shifts.shape).copy()
