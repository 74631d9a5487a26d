"""Goldens of the multi-shift prompts, recorded from the REFERENCE on the CPU (through ref_import.py) -> multi_shift.npz.

The reference's `MultiShiftPatchesAndMask.forward` (cwm/models/perturbation.py:644-779) cannot run as written: `_check_shapes` assigns to
`num_shifts`, a property without a setter (:171-175).  `RunnableMultiShift` below gives the property a setter and changes nothing else.

Kernel cases (`case_*`): B = 2, T = 2, C = 3, every input pixel a distinct positive integer (x[b,t,c,y,x] = 1 + its linear index: any wrong
source pixel shows, a padded pixel is the only 0, and the fixture compresses).  Per case the reference's x_p and mask_ps, the tables it was
given, and three non-vacuity counts: moved pixels, zero-padded pixels, and cells that are the destination of more than one step.
End-to-end record (`e2e_*`): tiny predictor + `synthetic.SyntheticFlow`, two movies at B = 1, S = 4 prompts of K = 3 steps each: the
reference's shifter per sample on the static movie with shift_sequence=None (the drawn shifts are recorded), ONE rectangulariser call over the
stacked rows, the reference's `predict`, the stand-in flow.  Run: python tests/golden/make_golden_multi_shift.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import ref_import  # noqa: E402
from counterfactualworldmodels_amd import synthetic as S  # noqa: E402
from make_golden_motion_sampling import TINY, ref_generator  # noqa: E402

MAX_STEPS = 8      # the library's stated maximum K
E2E_SEED = 4321    # torch's global generator is seeded with E2E_SEED + movie right before the one rectangulariser call
E2E_MAX_SHIFT_FRACTION = 0.5  # 16 px at 32^2: shifts of up to two patches (the default 0.15 gives |s| <= 4 < P: the mask would never move)


def runnable_class(ns):
    class RunnableMultiShift(ns.perturbation.MultiShiftPatchesAndMask):
        num_shifts = property(lambda self: ns.perturbation.ShiftPatchesAndMask.num_shifts.fget(self), lambda self, v: self.set_num_shifts(v))

    return RunnableMultiShift


def frames(B, H, W, T=2, Cc=3):
    return (np.arange(B * T * Cc * H * W, dtype=np.float32) + 1).reshape(B, T, Cc, H, W)


def tables(rng, B, H, W, P, K, n_points, frame, T=2, n_visible=3):
    """Random base masks [B,Nt,K] (n_visible visible cells of frame 0 ... per step) and points [B,Nt,K] (n_points cells of frame `frame`, one of
    the other frame)."""
    gh, gw = H // P, W // P
    n = gh * gw
    masks = np.ones((B, T * n, K), dtype=bool)
    points = np.zeros((B, T * n, K), dtype=bool)
    f = frame % T
    for b in range(B):
        for k in range(K):
            masks[b, rng.choice(T * n, n_visible, replace=False), k] = False
            points[b, f * n + rng.choice(n, n_points, replace=False), k] = True
            points[b, ((f + 1) % T) * n + rng.integers(n), k] = True
    return masks, points


def cell(P, H, W, frame, pi, pj, T=2):
    gw = W // P
    return (frame % T) * (H // P) * gw + pi * gw + pj


def kernel_cases():
    """tag -> dict(H, W, P, frame, masks [B,Nt,K] or [B,Nt], points [B,Nt,K] or None, shifts [K][2], expand_mask)."""
    rng = np.random.Generator(np.random.PCG64(20240611))
    out = {}

    def rand_shifts(K, P):
        return [[int(v) for v in rng.integers(-(2 * P + 1), 2 * P + 2, size=2)] for _ in range(K)]

    def add(tag, H, W, P, frame, masks, points, shifts, expand_mask=False):
        out[tag] = dict(H=H, W=W, P=P, frame=frame, masks=masks, points=points, shifts=[list(map(int, s)) for s in shifts], expand_mask=expand_mask)

    def single(H, W, P, cells, K=None, frame=1):
        """All-masked base masks and, per step, the listed (pi, pj) cells of frame `frame` as points (both movies; movie 1 one cell further right)."""
        K = len(cells) if K is None else K
        n2 = 2 * (H // P) * (W // P)
        masks, points = np.ones((2, n2, K), dtype=bool), np.zeros((2, n2, K), dtype=bool)
        for k, step in enumerate(cells):
            for pi, pj in step:
                points[0, cell(P, H, W, frame, pi, pj), k] = True
                points[1, cell(P, H, W, frame, pi, min(pj + 1, W // P - 1)), k] = True
        return masks, points

    m, p = tables(rng, 2, 32, 32, 8, 3, 4, 1); add("p8_random", 32, 32, 8, 1, m, p, rand_shifts(3, 8))
    m, p = tables(rng, 2, 32, 32, 4, 3, 9, 0); add("p4_random_frame0", 32, 32, 4, 0, m, p, rand_shifts(3, 4))
    m, p = tables(rng, 2, 32, 48, 8, 4, 5, 1); add("wide_k4", 32, 48, 8, 1, m, p, rand_shifts(4, 8))
    # |s| < P at border patches: zeros come in from outside, the mask does not move
    m, p = single(32, 32, 8, [[(0, 0), (3, 2)], [(3, 3), (1, 0)]]); add("border_subpatch", 32, 32, 8, 1, m, p, [[3, 5], [-6, -2]])
    # a negative sub-patch shift: truncation toward zero keeps the mask in place, floor would move it by -1 patch
    m, p = single(32, 32, 8, [[(1, 1)], [(2, 2)]]); add("negative_subpatch", 32, 32, 8, 1, m, p, [[-3, -2], [-7, 1]])
    m, p = single(32, 32, 8, [[(1, 1)], [(2, 0)], [(0, 2)]]); add("axis_and_zero_steps", 32, 32, 8, 1, m, p, [[0, 11], [-9, 0], [0, 0]])
    m, p = tables(rng, 2, 32, 32, 8, 2, 4, 1); add("odd_sx", 32, 32, 8, 1, m, p, [[8, 5], [-4, -7]])
    m, p = tables(rng, 2, 32, 32, 8, 3, 4, 1); add("sx_multiples_of_4", 32, 32, 8, 1, m, p, [[3, 8], [-5, -4], [9, 12]])
    # step 2 picks up what step 1 put down: (0,0) -> (1,1) by (8,8) [movie 1: (0,1) -> (1,2)], then (1,1) [(1,2)] -> one patch and 3 px further right
    m, p = single(32, 32, 8, [[(0, 0)], [(1, 1)]]); add("chain", 32, 32, 8, 1, m, p, [[8, 8], [0, 11]])
    # two steps, two sources, one destination (2,1) [movie 1: (2,2)]: the later step wins
    m, p = single(32, 32, 8, [[(1, 1)], [(2, 0)]]); add("overlap", 32, 32, 8, 1, m, p, [[8, 0], [0, 8]])
    # the destination of (0,0) by (-8,0) is outside the frame: the token vanishes from the mask; the second patch stays inside
    m, p = single(32, 32, 8, [[(0, 0), (2, 2)]]); add("leaves_frame", 32, 32, 8, 1, m, p, [[-8, 0]])
    m, p = tables(rng, 2, 32, 32, 8, 2, 4, -1); add("frame_minus1", 32, 32, 8, -1, m, p, rand_shifts(2, 8))
    m, _ = tables(rng, 2, 32, 32, 8, 3, 4, 1, n_visible=5); add("no_points", 32, 32, 8, 1, m, None, rand_shifts(3, 8))
    m, p = tables(rng, 2, 32, 32, 8, 3, 4, 1); add("base_mask_2d", 32, 32, 8, 1, m[..., 0], p, rand_shifts(3, 8), expand_mask=True)
    m, p = tables(rng, 2, 32, 32, 8, 1, 5, 1); add("k1", 32, 32, 8, 1, m, p, [[-8, 16]])
    m, p = tables(rng, 2, 32, 32, 8, MAX_STEPS, 3, 1); add("k_max", 32, 32, 8, 1, m, p, rand_shifts(MAX_STEPS, 8))
    # Patch sizes that are no multiple of 4 (a group of four pixels can lie across two patches) on non-square frames, a 2 x 4, a 4 x 2 and a 2 x 2 grid.  Their
    # tables come from a generator of their own, drawn after everything above: the sixteen cases above do not change.  Each has an sx that is a multiple of 4
    # and one that is not, a point whose destination leaves the grid, and a cell that two steps write to (asserted in run_kernel_cases).
    rng2 = np.random.Generator(np.random.PCG64(20250117))
    m, p = tables(rng2, 2, 12, 24, 6, 3, 3, 1); add("p6_12x24", 12, 24, 6, 1, m, p, [[6, 8], [-7, 7], [3, -4]])
    m, p = tables(rng2, 2, 24, 12, 6, 2, 3, 0); add("p6_24x12", 24, 12, 6, 0, m, p, [[-6, 4], [-11, -7]])
    m, p = tables(rng2, 2, 24, 24, 12, 4, 2, 1); add("p12_24x24", 24, 24, 12, 1, m, p, [[12, 0], [0, -12], [-5, 16], [13, 7]])
    return out


NON_MULTIPLE_OF_4_CASES = ("p6_12x24", "p6_24x12", "p12_24x24")


def leaving_destinations(case):
    """Number of (movie, step, point) triples of frame `frame` whose destination cell is outside the grid."""
    H, W, P, f = case["H"], case["W"], case["P"], case["frame"] % 2
    gh, gw = H // P, W // P
    n = gh * gw
    count = 0
    for k, (sy, sx) in enumerate(case["shifts"]):
        my, mx = int(np.sign(sy)) * (abs(sy) // P), int(np.sign(sx)) * (abs(sx) // P)
        for b in range(case["points"].shape[0]):
            for c in np.flatnonzero(case["points"][b, f * n:(f + 1) * n, k]):
                count += not (0 <= c // gw + my < gh and 0 <= c % gw + mx < gw)
    return count


def overlapping_destinations(case):
    """Number of (movie, cell) pairs that more than one step writes to (destination = point cell + truncated patch shift, inside the grid)."""
    H, W, P, f = case["H"], case["W"], case["P"], case["frame"] % 2
    gh, gw = H // P, W // P
    n = gh * gw
    pts = case["points"] if case["points"] is not None else ~(case["masks"] if case["masks"].ndim == 3 else case["masks"][..., None])
    hits = np.zeros((pts.shape[0], gh, gw), dtype=np.int64)
    for k, (sy, sx) in enumerate(case["shifts"]):
        my, mx = int(np.sign(sy)) * (abs(sy) // P), int(np.sign(sx)) * (abs(sx) // P)
        for b in range(pts.shape[0]):
            for c in np.flatnonzero(pts[b, f * n:(f + 1) * n, k]):
                pi, pj = c // gw + my, c % gw + mx
                if 0 <= pi < gh and 0 <= pj < gw:
                    hits[b, pi, pj] += 1
    return int((hits > 1).sum())


def run_kernel_cases(ns, out):
    Shifter = runnable_class(ns)
    cases = kernel_cases()
    meta = {}
    total_zero = total_overlap = 0
    for tag, c in cases.items():
        x = frames(2, c["H"], c["W"])
        masks = torch.from_numpy(c["masks"])
        if c["expand_mask"]:  # the reference's own expand (perturbation.py:709) fails for B > 1: it gets the mask of every step
            masks = masks.unsqueeze(-1).expand(-1, -1, len(c["shifts"])).clone()
        points = None if c["points"] is None else torch.from_numpy(c["points"])
        shifter = Shifter(patch_size=(1, c["P"], c["P"]), max_shift_fraction=0.15, padding_mode="constant", allow_fractional_shifts=True)
        with torch.no_grad():
            x_p, mask_ps = shifter(torch.from_numpy(x), masks, points, [tuple(s) for s in c["shifts"]], frame=c["frame"])
        x_p, mask_ps = x_p.numpy(), mask_ps.numpy()
        f = c["frame"] % 2
        moved = int((x_p[:, f] != x[:, f]).sum())
        zeros = int((x_p == 0).sum())
        overlap = overlapping_destinations(c)
        assert np.array_equal(x_p[:, 1 - f], x[:, 1 - f]) and moved > 0, tag
        assert np.isin(x_p, np.concatenate([[0], x.ravel()])).all()
        total_zero += zeros
        total_overlap += overlap
        meta[tag] = dict(H=c["H"], W=c["W"], P=c["P"], frame=c["frame"], K=len(c["shifts"]), has_points=c["points"] is not None, moved=moved, zeros=zeros,
                         overlap=overlap)
        out["case_%s_masks" % tag] = c["masks"]
        if c["points"] is not None:
            out["case_%s_points" % tag] = c["points"]
        out["case_%s_shifts" % tag] = np.array(c["shifts"], dtype=np.int64)
        out["case_%s_x_p" % tag] = x_p
        out["case_%s_mask_ps" % tag] = mask_ps
        print("[golden] multi_shift %-20s K=%d moved %5d px, zero-padded %4d px, overlapping destinations %d, visible tokens %s"
              % (tag, len(c["shifts"]), moved, zeros, overlap, (~mask_ps).sum(1).tolist()))
    assert total_zero > 0 and total_overlap > 0, (total_zero, total_overlap)
    assert meta["border_subpatch"]["zeros"] > 0 and meta["overlap"]["overlap"] > 0 and meta["k_max"]["K"] == MAX_STEPS
    for tag in NON_MULTIPLE_OF_4_CASES:
        sx = [s[1] for s in cases[tag]["shifts"]]
        assert cases[tag]["P"] % 4 != 0 or tag == "p12_24x24"
        assert meta[tag]["K"] >= 2 and any(v % 4 == 0 for v in sx) and any(v % 4 != 0 for v in sx), tag
        assert meta[tag]["zeros"] > 0 and meta[tag]["overlap"] > 0 and leaving_destinations(cases[tag]) > 0, (tag, meta[tag], leaving_destinations(cases[tag]))
    out["cases"] = np.array(json.dumps(meta))
    out["max_steps"] = np.array(MAX_STEPS)


def run_shift_forms(ns, out):
    """`_preprocess_shifts_sequence` of the reference on each accepted form, and the draws of a fresh shifter (seed 0) at 32 x 48 and 224 x 224."""
    Shifter = runnable_class(ns)
    sh = Shifter(patch_size=(1, 8, 8))
    forms = {}
    for name, K, arg in [("pair", 3, (5, -2)), ("pair_in_list", 3, [(5, -2)]), ("list", 3, [(1, 2), (-3, 4), (0, 7)]),
                         ("tensor_2xK", 3, torch.tensor([[1, -3, 0], [2, 4, 7]])), ("tensor_2x1", 4, torch.tensor([[6], [-9]])),
                         ("array_2xK", 2, np.array([[1, -3], [2, 4]]))]:
        sh.set_num_shifts(K)
        kind = "tensor" if torch.is_tensor(arg) else ("array" if isinstance(arg, np.ndarray) else "list")
        if kind == "list":
            got, from_reference = sh._preprocess_shifts_sequence(arg), True
        else:
            # the reference splits a [2,S] array into S columns (perturbation.py:722-731) and then fails its own list checks on them (:733-736: the
            # columns are arrays, not lists, so they are wrapped once more): recorded is what the split intends, column s = step s, one column broadcast
            try:
                bad = sh._preprocess_shifts_sequence(arg)
                assert any(np.ndim(s[0]) > 0 for s in bad), "the reference handled an array form: record its answer instead"
            except AssertionError as e:
                assert "record its answer" not in str(e)
            cols = np.asarray(arg)
            got, from_reference = [(cols[0, s], cols[1, s]) for s in range(cols.shape[1])] * (K if cols.shape[1] == 1 else 1), False
        forms[name] = dict(K=K, arg=np.asarray(arg).tolist(), kind=kind, from_reference=from_reference, want=[[int(s[0]), int(s[1])] for s in got])
    out["shift_forms"] = np.array(json.dumps(forms))
    for tag, size in [("32x48", (32, 48)), ("224", (224, 224))]:
        sh = Shifter(patch_size=(1, 8, 8), max_shift_fraction=0.15)
        sh.image_size = size
        sh.set_num_shifts(6)
        out["draws_" + tag] = np.array(sh._preprocess_shifts_sequence(None) + sh._preprocess_shifts_sequence(None), dtype=np.int64)
        assert (np.abs(out["draws_" + tag]).max(0) <= [int(0.15 * size[0]), int(0.15 * size[1])]).all()


def run_e2e(ns, out):
    Shifter = runnable_class(ns)
    S_, K = 4, 3
    x = torch.from_numpy(S.synthetic_frames(2, TINY, 47))
    out["e2e_x"] = x.numpy()
    n = 16

    def prompts(movie, seed):
        rng = np.random.Generator(np.random.PCG64(seed))
        G = ref_generator(ns, seed=movie, max_shift_fraction=E2E_MAX_SHIFT_FRACTION)
        G.multi_patch_shifter = Shifter(patch_size=G.predictor.patch_size, max_shift_fraction=E2E_MAX_SHIFT_FRACTION, padding_mode="constant",
                                        allow_fractional_shifts=True)
        xs = G.make_static_movie(x[movie:movie + 1, 0:1], T=2)
        G.set_input(xs)
        passive = G.get_zeros_mask()  # [1,Nt]: frame 0 visible, frame 1 masked
        active = np.ones((1, 2 * n, K, S_), dtype=bool)  # this package's convention: 0 = moved
        for s in range(S_):
            for k, c in enumerate(rng.choice(n, K, replace=False)):
                active[0, n + c, k, s] = False
        rows, masks, shifts = [], [], []
        with torch.no_grad():
            for s in range(S_):
                points = torch.from_numpy(~active[..., s])
                m = passive.unsqueeze(-1).expand(-1, -1, K).clone()
                G.multi_patch_shifter.set_shapes(xs, m)
                drawn = G.multi_patch_shifter._preprocess_shifts_sequence(None)  # what forward(shift_sequence=None) draws, here so that it can be recorded
                x_p, mask_p = G.multi_patch_shifter(xs, m, points, drawn, frame=1)
                rows.append(x_p); masks.append(mask_p); shifts.append([[int(d[0]), int(d[1])] for d in drawn])
        return G, active, torch.cat(rows, 0), torch.cat(masks, 0), shifts

    for movie in (0, 1):
        # the active cells come from the first seed at which the rows do NOT all mask equally many tokens (a token whose destination leaves the frame or is
        # overwritten vanishes): otherwise the one rectangulariser call of the record would have nothing to do
        for seed in range(99, 140):
            G, active, rows, masks, shifts = prompts(movie, seed)
            if len(set(masks.sum(1).tolist())) > 1:
                break
        else:
            raise AssertionError("no seed gives rows with different masked counts")
        with torch.no_grad():
            torch.manual_seed(E2E_SEED + movie)
            rect = G.mask_rectangularizer(masks.clone())
            y = G.predict(rows, rect, frame=None)
            flow = G.predict_flow(y, backward=False)
        assert not torch.equal(rect, masks)
        assert (np.abs(np.array(shifts)) >= 8).any(), "no shift of a whole patch drawn"
        t = "e2e_m%d_" % movie
        out[t + "active"], out[t + "shifts"], out[t + "mask"] = active, np.array(shifts, dtype=np.int64), rect.numpy()
        out[t + "x_p"], out[t + "videos"], out[t + "flows"] = rows.numpy(), y.numpy(), flow.numpy()
        print("[golden] multi_shift e2e movie %d: shifts %s, masked per row %s (before the rectangulariser %s), |flow| max %.2f"
              % (movie, shifts, rect.sum(1).tolist(), masks.sum(1).tolist(), float(flow.abs().max())))
    out["e2e_seed"] = np.array(E2E_SEED)
    out["e2e_max_shift_fraction"] = np.array(E2E_MAX_SHIFT_FRACTION)


def main():
    ns = ref_import.import_reference()
    assert ns.segmentation is not None, getattr(ns, "segmentation_error", None)
    torch.set_num_threads(8)
    out = {}
    run_kernel_cases(ns, out)
    run_shift_forms(ns, out)
    run_e2e(ns, out)
    path = os.path.join(HERE, "multi_shift.npz")
    if os.path.exists(path):
        # what the fixture held before this run comes out byte for byte: every array but the JSON index of the cases, and that index entry by entry
        old = np.load(path)
        for k in old.files:
            if k != "cases":
                assert k in out and np.asarray(out[k]).dtype == old[k].dtype and np.asarray(out[k]).shape == old[k].shape \
                    and np.asarray(out[k]).tobytes() == old[k].tobytes(), "array %s of the existing multi_shift.npz changed" % k
        old_meta, new_meta = json.loads(str(old["cases"])), json.loads(str(out["cases"]))
        assert list(new_meta)[:len(old_meta)] == list(old_meta) and all(new_meta[t] == old_meta[t] for t in old_meta), "a recorded case changed"
        print("[golden] multi_shift.npz: all %d existing arrays byte-identical, %d new" % (len(old.files), len(out) - len(old.files)))
    np.savez_compressed(path, **out)
    print("[golden] multi_shift.npz %.0f kB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
