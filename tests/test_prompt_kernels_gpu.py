"""The index-arithmetic kernels of csrc/elementwise.hip at geometries the other suites do not reach: un-embed (both kernels, strided and misaligned frames),
the single-shift prompt pair, the prompt table, the multi-shift pair and the pick table of the rectangulariser.

Every comparison is exact (bit patterns of the floats, equality of the masks).  Every output buffer is followed by 64 guard elements that must keep their
fill value.  Every case asserts, on the reference alone, that it exercises what it is there for; the seeds below were chosen on the CPU so that these
conditions hold.  References: `oracle.vmae_oracle` (pred_patches_to_video, create_motion_counterfactuals, make_static) and the per-pixel loops of
tests/prompt_kernels_restatement.py, which tests/test_prompt_kernels_cpu.py pins to the reference's recordings.  Non-square frames throughout: on a square
grid gh == gw, and an exchange of the two passes unnoticed."""
import functools

import numpy as np
import pytest
import torch

import prompt_kernels_restatement as PR
from counterfactualworldmodels_amd import _lib
from oracle import vmae_oracle as O

pytestmark = pytest.mark.gpu
GUARD = 64


def stream():
    return _lib.current_stream_handle(torch.device("cuda:0"))


def guarded(shape, dtype, fill, offset=0):
    """(buffer, view of `shape` starting `offset` elements into it); buffer = offset + numel + GUARD elements, all `fill`."""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[offset:offset + n].view(shape)


def guards_intact(buf, view, fill, offset=0):
    n = view.numel()
    return buf.numel() == offset + n + GUARD and bool((buf[offset + n:] == fill).all()) and bool((buf[:offset] == fill).all())


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def distinct_frames(B, T, Cc, H, W):
    """Every pixel a distinct positive integer (exact in fp32): a wrong source pixel shows, and 0 is a padded pixel only."""
    return (np.arange(B * T * Cc * H * W, dtype=np.float32) + 1).reshape(B, T, Cc, H, W)


# ---- un-embed ------------------------------------------------------------------------------------------------------------------------------------------
UNEMBED_CASES = [(2, 2, 3, 24, 40, 8, 11), (2, 3, 3, 16, 24, 4, 30), (1, 2, 3, 32, 48, 16, 5), (2, 2, 2, 16, 24, 8, 5), (2, 2, 1, 8, 12, 4, 3), (2, 1, 4, 16, 8, 8, 1)]


@functools.lru_cache(maxsize=None)
def unembed_case(case):
    """(x [B,T,C,H,W] in [1, 2), y [B,Nm,P P C] in [-2, -1], mask [B,Nt], reference video) on the CPU.  Every row has masked and visible patches in every
    frame, and the rows' masks differ."""
    B, T, Cc, H, W, P, n_vis = case
    gen = torch.Generator().manual_seed(100 + UNEMBED_CASES.index(case))
    n = (H // P) * (W // P)
    Nt = T * n
    x = torch.rand(B, T, Cc, H, W, generator=gen) + 1.0
    y = -(torch.rand(B, Nt - n_vis, P * P * Cc, generator=gen) + 1.0)
    while True:
        mask = torch.ones(B, Nt, dtype=torch.bool)
        for b in range(B):
            mask[b, torch.randperm(Nt, generator=gen)[:n_vis]] = False
        per_frame = (~mask).view(B, T, n).sum(-1)
        if bool(((per_frame > 0) & (per_frame < n)).all()) and all(not torch.equal(mask[b], mask[0]) for b in range(1, B)):
            break
    want = O.pred_patches_to_video(y, x, mask, P)
    assert float(x.min()) >= 1.0 and float(y.max()) <= -1.0 and bool((want > 0).any()) and bool((want < 0).any())
    return x, y, mask, want


def three_channel_kernel(Cc, H, x_view, y, out):
    """`launch_unembed`'s rule: unembed3_kernel needs C == 3, an even H, 16-byte aligned y / out / x and batch, time and channel strides that are multiples of
    4 floats; everything else runs the generic unembed_kernel."""
    sb, st, sc = x_view.stride()[:3]
    return Cc == 3 and H % 2 == 0 and all(t.data_ptr() % 16 == 0 for t in (x_view, y, out)) and all(s % 4 == 0 for s in (sb, st, sc))


def run_unembed(y, x_view, mask, P, n_vis, out, hook):
    """`cwm_unembed` (contiguous frames) or the development hook `cwm_dev_unembed` with the frames' own strides."""
    B, T, Cc, H, W = x_view.shape
    sb, st, sc, sh, sw = x_view.stride()
    assert sw == 1 and sh == W and out.is_contiguous() and y.is_contiguous() and mask.is_contiguous()
    if hook:
        d = _lib.get_dev_lib()
        _lib.check(d.cwm_dev_unembed(y.data_ptr(), x_view.data_ptr(), sb, sc, st, mask.data_ptr(), B, T, Cc, H, W, P, n_vis, out.data_ptr(), stream()), d)
    else:
        assert x_view.is_contiguous()
        _lib.check(_lib.get_lib().cwm_unembed(y.data_ptr(), x_view.data_ptr(), mask.data_ptr(), B, T, Cc, H, W, P, n_vis, out.data_ptr(), stream()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", UNEMBED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_unembed_equals_pred_patches_to_video(case):
    B, T, Cc, H, W, P, n_vis = case
    x, y, mask, want = unembed_case(case)
    xd, yd, md, wd = x.cuda(), y.cuda(), mask.cuda(), want.cuda()
    results = {}
    for hook in (False, True):
        buf, out = guarded(x.shape, torch.float32, -7.0)
        run_unembed(yd, xd, md, P, n_vis, out, hook)
        assert three_channel_kernel(Cc, H, xd, yd, out) == (Cc == 3)
        assert same_bits(out, wd) and guards_intact(buf, out, -7.0), (case, hook)
        results[hook] = out.clone()
    if Cc != 3:
        return
    # the three-channel cases once more through the GENERIC kernel: x 4 bytes off the 16-byte grid, out likewise, and frames inside a padded buffer whose
    # channel and time strides are no multiple of 4 floats (rows and pixels stay contiguous)
    xbuf, x_off = guarded(x.shape, torch.float32, 777.0, offset=1)
    x_off.copy_(xd)
    buf, out = guarded(x.shape, torch.float32, -7.0)
    assert x_off.data_ptr() % 16 == 4 and not three_channel_kernel(Cc, H, x_off, yd, out)
    for hook in (False, True):
        out.fill_(-7.0)
        run_unembed(yd, x_off, md, P, n_vis, out, hook)
        assert same_bits(out, results[False]) and guards_intact(buf, out, -7.0) and guards_intact(xbuf, x_off, 777.0, offset=1), (case, "x off", hook)
    buf, out = guarded(x.shape, torch.float32, -7.0, offset=1)
    assert out.data_ptr() % 16 == 4 and not three_channel_kernel(Cc, H, xd, yd, out)
    for hook in (False, True):
        out.fill_(-7.0)
        run_unembed(yd, xd, md, P, n_vis, out, hook)
        assert same_bits(out, results[False]) and guards_intact(buf, out, -7.0, offset=1), (case, "out off", hook)
    L = H * W + 3
    xpad = torch.full((B, T, Cc, L), 777.0, device="cuda")
    x_str = torch.as_strided(xpad, (B, T, Cc, H, W), (T * Cc * L, Cc * L, L, W, 1))
    x_str.copy_(xd)
    buf, out = guarded(x.shape, torch.float32, -7.0)
    assert x_str.stride(1) % 4 != 0 and x_str.stride(2) % 4 != 0 and not three_channel_kernel(Cc, H, x_str, yd, out)
    run_unembed(yd, x_str, md, P, n_vis, out, True)
    assert same_bits(out, results[False]) and guards_intact(buf, out, -7.0), (case, "strided")
    assert bool((xpad[..., H * W:] == 777.0).all()) and torch.equal(x_str, xd) and not bool((out == 777.0).any())


def test_unembed_with_nothing_masked_returns_the_frames():
    B, T, Cc, H, W, P = 2, 2, 3, 24, 40, 8
    x = (torch.rand(B, T, Cc, H, W, generator=torch.Generator().manual_seed(7)) + 1.0).cuda()
    Nt = T * (H // P) * (W // P)
    mask = torch.zeros(B, Nt, dtype=torch.bool, device="cuda")
    dummy = torch.full((4,), -1.0, device="cuda")
    for hook in (False, True):
        buf, out = guarded(x.shape, torch.float32, -7.0)
        run_unembed(dummy, x, mask, P, Nt, out, hook)
        assert same_bits(out, x) and guards_intact(buf, out, -7.0)


# ---- single shift ----------------------------------------------------------------------------------------------------------------------------------------
SHIFT_CASES = [(2, 3, 2, 3, 16, 24, 8, 1), (1, 4, 3, 3, 24, 16, 4, 2), (2, 2, 2, 1, 32, 48, 16, 0), (1, 5, 2, 2, 16, 40, 8, 1)]
SHIFT_SEED = 0   # the tables of every case below meet `shift_non_vacuity` with this seed


def shift_tables(case, seed=SHIFT_SEED):
    """x [B,T,C,H,W], passive / active [R,Nt] (0 = visible / 0 = moved) and patch shifts [R,2] for R = B S prompts: two or three active patches of frame
    `frame` per prompt (and, on odd rows, one of another frame, which is re-masked and never moved), shifts of every kind the kernel distinguishes."""
    B, S_, T, Cc, H, W, P, frame = case
    gen = torch.Generator().manual_seed(seed)
    gh, gw = H // P, W // P
    n = gh * gw
    R = B * S_
    x = torch.rand(B, T, Cc, H, W, generator=gen)
    passive = torch.rand(R, T * n, generator=gen) < 0.5
    active = torch.ones(R, T * n, dtype=torch.bool)
    shifts = torch.zeros(R, 2, dtype=torch.int32)
    for i in range(R):
        cells = torch.randperm(n, generator=gen)[:2 + i % 2]
        active[i, frame * n + cells] = False
        if i % 2 and T > 1:
            active[i, ((frame + 1) % T) * n + int(torch.randint(n, (1,), generator=gen))] = False
        pi, pj = cells // gw, cells % gw
        kind = i % 4   # 0: no shift, 1: some destination inside the grid, 2: one leaves on the row axis, 3: one leaves on the column axis
        if kind == 1:
            dy = 1 if int(pi.min()) < gh - 1 else -1
            dx = 1 if int(pj[pi.argmin() if dy == 1 else pi.argmax()]) < gw - 1 else -1
            shifts[i] = torch.tensor([dy, dx])
        elif kind == 2:
            shifts[i] = torch.tensor([gh - int(pi.max()), 0])
        elif kind == 3:
            shifts[i] = torch.tensor([0, -(int(pj.min()) + 1)])
    return x, passive, active, shifts


def shift_non_vacuity(case, passive, active, shifts):
    B, S_, T, Cc, H, W, P, frame = case
    gh, gw = H // P, W // P
    n = gh * gw
    inside = row_out = col_out = zero = False
    for i in range(active.shape[0]):
        dy, dx = int(shifts[i, 0]), int(shifts[i, 1])
        zero |= (dy, dx) == (0, 0)
        for c in torch.nonzero(~active[i, frame * n:(frame + 1) * n]).flatten().tolist():
            r_in, c_in = 0 <= c // gw + dy < gh, 0 <= c % gw + dx < gw
            inside |= r_in and c_in and (dy, dx) != (0, 0)
            row_out |= (not r_in) and c_in
            col_out |= r_in and (not c_in)
    assert inside and row_out and col_out and zero, (case, inside, row_out, col_out, zero)
    assert all(2 <= int((~active[i, frame * n:(frame + 1) * n]).sum()) <= 3 for i in range(active.shape[0]))
    if B > 1:
        assert not torch.equal(active[S_:], active[:S_]) and not torch.equal(passive[S_:], passive[:S_])
    # MakeStatic: patches the passive mask leaves visible and patches it masks, among the moved ones and in every frame
    src = passive[:, frame * n:(frame + 1) * n][~active[:, frame * n:(frame + 1) * n]]
    assert bool(src.any()) and bool((~src).any()) and all(0 < int(passive[:, t * n:(t + 1) * n].sum()) < passive.shape[0] * n for t in range(T))


@functools.lru_cache(maxsize=None)
def shift_reference(case, fix_passive):
    """The oracle's frames and masks for `fix_passive` 0 (the movie as given), 1 (make_static_movie) and 2 (MakeStatic on each prompt's visible patches)."""
    B, S_, T, Cc, H, W, P, frame = case
    x, passive, active, shifts = shift_tables(case, SHIFT_SEED)
    R, Nt = passive.shape
    table = [(int(r[0]), int(r[1])) for r in shifts]
    if fix_passive < 2:
        bns = lambda a: a.view(B, S_, Nt).permute(0, 2, 1)  # noqa: E731
        return O.create_motion_counterfactuals(x, bns(passive), bns(active), table, P, frame=frame, fix_passive=bool(fix_passive))
    xs, ms = [], []
    for i in range(R):
        b = i // S_
        static = O.make_static(x[b:b + 1], passive[i:i + 1], P)
        xo, mo = O.shift_patches_and_mask(static, passive[i:i + 1], active[i:i + 1], table[i], P, frame)
        xs.append(xo)
        ms.append(mo)
    return torch.cat(xs, 0), torch.cat(ms, 0)


@pytest.mark.parametrize("fix_passive", [0, 1, 2])
@pytest.mark.parametrize("case", SHIFT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_shift_prompts_equal_the_oracle(case, fix_passive):
    B, S_, T, Cc, H, W, P, frame = case
    x, passive, active, shifts = shift_tables(case, SHIFT_SEED)
    shift_non_vacuity(case, passive, active, shifts)
    want_x, want_m = shift_reference(case, fix_passive)
    R, Nt = passive.shape
    assert not torch.equal(want_x[:, frame], x[:, 0 if fix_passive == 1 else frame].repeat_interleave(S_, 0))   # something moved
    if fix_passive:
        assert not torch.equal(want_x, shift_reference(case, 0)[0])   # the frames of the movie differ: the static forms are visible
    xd, pd, ad, sd = x.cuda(), passive.cuda(), active.cuda(), shifts.cuda()
    lib = _lib.get_lib()
    for frames, masks in ((True, True), (True, False), (False, True)):
        xbuf, xo = guarded((R, T, Cc, H, W), torch.float32, -7.0) if frames else (None, None)
        mbuf, mo = guarded((R, Nt), torch.uint8, 3) if masks else (None, None)
        _lib.check(lib.cwm_shift_prompts(xd.data_ptr(), B, T, Cc, H, W, P, frame, S_, fix_passive, ad.data_ptr(), pd.data_ptr(), sd.data_ptr(), _lib.ptr(xo),
                                         _lib.ptr(mo), stream()))
        torch.cuda.synchronize()
        if frames:
            assert same_bits(xo.cpu(), want_x) and guards_intact(xbuf, xo, -7.0), (case, fix_passive, frames, masks)
        if masks:
            assert torch.equal(mo.cpu().bool(), want_m) and int(mo.max()) <= 1 and guards_intact(mbuf, mo, 3), (case, fix_passive, frames, masks)


# ---- prompt table ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", [1, 2])
def test_prompt_table_cells_outside_the_grid_clear_nothing(frame):
    """(S, T, gh, gw) = (9, 3, 2, 5).  Rows 2, 4, 6 and 8 name cells outside the grid whose linear index h gw + w names another cell: w == gw is (h + 1, 0),
    w == -1 is (h - 1, gw - 1), h == gh is a cell of the next frame, h == -1 one of the frame before.  They clear nothing, their shifts are copied, and the
    rows between them are expanded as ever."""
    S_, T, gh, gw = 9, 3, 2, 5
    n = gh * gw
    table = np.array([[0, 0, 1, -1], [1, 4, 0, 2], [0, gw, 3, 3], [0, 3, -2, 0], [1, -1, 5, 6], [1, 0, 0, -4], [gh, 1, 7, 8], [1, 2, 2, 2], [-1, 3, -9, 9]],
                     dtype=np.int32)
    want_a, want_p, want_s = PR.prompt_table_expand(table, T, gh, gw, frame)
    in_grid = [0, 1, 3, 5, 7]
    assert (~want_a).sum(1).tolist() == [n + (i in in_grid) for i in range(S_)]   # frame 0 and, for in-grid rows, one more cell
    # what the linear index alone would have cleared is a masked cell of the reference in at least three of the four rows (so clearing it would show)
    alias = [frame * n + int(table[i, 0]) * gw + int(table[i, 1]) for i in (2, 4, 6, 8)]
    assert sum(0 <= a < T * n and bool(want_a[i, a]) for i, a in zip((2, 4, 6, 8), alias)) >= 3
    td = torch.from_numpy(table).cuda()
    abuf, a = guarded((S_, T * n), torch.uint8, 3)
    pbuf, p = guarded((S_, T * n), torch.uint8, 3)
    sbuf, s = guarded((S_, 2), torch.int32, -77)
    _lib.check(_lib.get_lib().cwm_prompt_table_expand(td.data_ptr(), S_, T, gh, gw, frame, a.data_ptr(), p.data_ptr(), s.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert torch.equal(p.cpu().bool(), torch.from_numpy(want_p)) and int(p.max()) <= 1
    assert torch.equal(s.cpu(), torch.from_numpy(want_s)) and torch.equal(s.cpu(), torch.from_numpy(table[:, 2:]))
    assert torch.equal(a.cpu().bool()[in_grid], torch.from_numpy(want_a)[in_grid]), "in-grid rows"
    assert torch.equal(a.cpu().bool(), torch.from_numpy(want_a)), "a cell outside the grid cleared a cell"
    assert guards_intact(abuf, a, 3) and guards_intact(pbuf, p, 3) and guards_intact(sbuf, s, -77)


# ---- multi-shift -----------------------------------------------------------------------------------------------------------------------------------------
#               B, S, T, C,  H,  W,  P, frame, K, seed
MULTI_CASES = {"p6_rows": (2, 2, 3, 5, 12, 24, 6, 2, 3, 0), "p12_one_channel": (1, 2, 2, 1, 24, 24, 12, 1, 2, 0), "p8_wide_k8": (2, 1, 2, 3, 16, 40, 8, 1, 8, 0)}


@functools.lru_cache(maxsize=None)
def multi_tables(name):
    """Per-row tables: points [R,K,Nt] (about a third of the cells of frame `frame` per step, one cell of another frame), base masks [R,K,Nt], pixel shifts
    [R,K,2] with |s| < min(H, W); row 0's sx are all multiples of 4.  Returns them with the restatement's source map of frame `frame`."""
    B, S_, T, Cc, H, W, P, frame, K, seed = MULTI_CASES[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    gh, gw = H // P, W // P
    n = gh * gw
    R = B * S_
    points = np.zeros((R, K, T * n), dtype=bool)
    masks = rng.random((R, K, T * n)) < 0.6
    lim = min(H, W) - 1
    shifts = rng.integers(-lim, lim + 1, size=(R, K, 2))
    shifts[0, :, 1] = 4 * rng.integers(-(lim // 4), lim // 4 + 1, size=K)
    for i in range(R):
        for k in range(K):
            points[i, k, frame * n + rng.choice(n, max(1, n // 3), replace=False)] = True
            points[i, k, ((frame + 1) % T) * n + rng.integers(n)] = True
    return points, masks, shifts, PR.multi_shift_sources(points, shifts, P, frame, T, H, W)


def raw_multi_shift(x, points, masks, shifts, case, fix_passive, frames=True, masks_out=True):
    B, S_, T, Cc, H, W, P, frame, K, _ = case
    R, _, Nt = points.shape
    xbuf, xo = guarded((R, T, Cc, H, W), torch.float32, -7.0) if frames else (None, None)
    mbuf, mo = guarded((R, Nt), torch.uint8, 3) if masks_out else (None, None)
    _lib.check(_lib.get_lib().cwm_multi_shift_prompts(
        x.data_ptr(), B, T, Cc, H, W, P, frame, S_, K, fix_passive, points.data_ptr(), _lib.ptr(masks), 0 if masks is None else masks.shape[1], shifts.data_ptr(),
        int(shifts.abs().max()), _lib.ptr(xo), _lib.ptr(mo), stream()))
    torch.cuda.synchronize()
    assert (xbuf is None or guards_intact(xbuf, xo, -7.0)) and (mbuf is None or guards_intact(mbuf, mo, 3))
    return xo, mo


def multi_non_vacuity(name):
    """What a multi-shift case is there for, asserted on the restatement alone; returns the number of zero-padded pixels of frame `frame`."""
    B, S_, T, Cc, H, W, P, frame, K, _ = MULTI_CASES[name]
    points, masks, shifts, src = multi_tables(name)
    R = B * S_
    ys, xs = np.mgrid[0:H, 0:W]
    moved = int(((src[..., 0] != ys) | (src[..., 1] != xs)).sum())
    padded = int((src[..., 0] < 0).sum())
    assert moved > 0 and padded > 0 and padded < moved, (name, moved, padded)
    assert (shifts[0, :, 1] % 4 == 0).all() and (shifts[1:, :, 1] % 4 != 0).any() and np.abs(shifts).max() < min(H, W)
    assert (np.abs(shifts) >= P).any() and (np.abs(shifts) % P != 0).any()
    if S_ > 1:
        assert not np.array_equal(points[0], points[1]) and not np.array_equal(shifts[0], shifts[1])   # rows of one movie have tables of their own
    if P % 4:
        # four-pixel groups that lie across two patches AND whose pixels were read from places that are not four neighbours: the kernel's split branch
        g4 = src.reshape(R, H, W // 4, 4, 2)
        across = (np.arange(0, W, 4) % P + 3 >= P)[None, None, :]
        together = ((g4[..., 0] == g4[..., :1, 0]).all(-1)) & ((g4[..., 1] - g4[..., :1, 1] == np.arange(4)).all(-1))
        assert int((across & ~together & (g4[..., 0] >= 0).any(-1)).sum()) > 0, name
    return padded


@pytest.mark.parametrize("name", list(MULTI_CASES))
def test_multi_shift_raw_abi_equals_the_restatement(name):
    case = MULTI_CASES[name]
    B, S_, T, Cc, H, W, P, frame, K, _ = case
    points, masks, shifts, src = multi_tables(name)
    R = B * S_
    x = distinct_frames(B, T, Cc, H, W)
    padded = multi_non_vacuity(name)
    xd, pd, sd = torch.from_numpy(x).cuda(), torch.from_numpy(points).cuda(), torch.from_numpy(shifts.astype(np.int32)).cuda()
    base = {"none": None, "shared": np.ascontiguousarray(masks[:, :1]), "per_step": masks}
    want_m = {k: PR.multi_shift_mask(points, m, shifts, P, frame, T, H, W) for k, m in base.items()}
    assert not np.array_equal(want_m["none"], want_m["shared"]) and not np.array_equal(want_m["shared"], want_m["per_step"])
    for fix_passive in (0, 1):
        want_x = PR.multi_shift_frames(x, points, shifts, P, frame, S=S_, fix_passive=fix_passive, sources=src)
        assert int((want_x == 0).sum()) == padded * Cc
        for kind, m in base.items():
            md = None if m is None else torch.from_numpy(m).cuda()
            xo, mo = raw_multi_shift(xd, pd, md, sd, case, fix_passive)
            assert same_bits(xo.cpu(), torch.from_numpy(want_x)), (name, fix_passive, kind)
            assert torch.equal(mo.cpu().bool(), torch.from_numpy(want_m[kind])) and int(mo.max()) <= 1, (name, fix_passive, kind)
        only_x, none_m = raw_multi_shift(xd, pd, None, sd, case, fix_passive, masks_out=False)
        none_x, only_m = raw_multi_shift(xd, pd, None, sd, case, fix_passive, frames=False)
        assert none_m is None and none_x is None and same_bits(only_x.cpu(), torch.from_numpy(want_x)) and torch.equal(only_m.cpu().bool(), torch.from_numpy(want_m["none"]))
    assert not np.array_equal(PR.multi_shift_frames(x, points, shifts, P, frame, S=S_, fix_passive=0, sources=src), want_x)   # fix_passive 1 is visible


# ---- pick table rows -------------------------------------------------------------------------------------------------------------------------------------
def test_flip_picks_skips_table_rows_outside_the_mask():
    """The mask is rows [2, 2 + B) of a larger tensor.  The table names row 1, row -1 (the tensor's row 1), row B (the first row behind the mask) and row 3:
    rows 1 and 3 get their picks, every other byte of the tensor stays."""
    B, Nt = 5, 40
    big = (torch.rand(2 + B + 2, Nt, generator=torch.Generator().manual_seed(3)) < 0.5).to(torch.uint8)
    rows, to_value, picks = [1, -1, B, 3], [0, 0, 1, 1], [[0, 2], [0, 1], [0, 3], [1, 4, 5]]
    want = big.clone()
    for r, to, pk in zip(rows, to_value, picks):
        cand = torch.nonzero(big[2 + r] != to).flatten()
        assert cand.numel() > max(pk)   # every pick names a token: applied to its row, it would change it
        if 0 <= r < B:
            want[2 + r, cand[pk]] = to
    assert not torch.equal(want[3], big[3]) and not torch.equal(want[5], big[5]) and 2 * Nt >= GUARD
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in picks])]).tolist()
    table = torch.tensor([len(rows)] + rows + offsets + to_value + sum(picks, []), dtype=torch.int32).cuda()
    bd = big.cuda()
    _lib.check(_lib.get_lib().cwm_mask_flip_picks(bd[2:2 + B].data_ptr(), B, Nt, table.data_ptr(), len(rows), stream()))
    torch.cuda.synchronize()
    got = bd.cpu()
    assert torch.equal(got[3], want[3]) and torch.equal(got[5], want[5]), "the valid rows hold their picks"
    assert torch.equal(got[:2], big[:2]), "a row index below 0 wrote in front of the mask"
    assert torch.equal(got[2 + B:], big[2 + B:]), "a row index >= B wrote behind the mask"
    assert torch.equal(got, want)


# ---- one-frame movies ------------------------------------------------------------------------------------------------------------------------------------
def test_num_frames_is_refused_for_more_than_one_movie():
    """`_shift_rows(num_frames=T)` is the form for ONE static movie given as its first frame.  With B > 1 the kernel would look for movie b at frame b T of a
    tensor of B frames: refused before anything is allocated or launched.  B == 1 equals the materialised movie."""
    from counterfactualworldmodels_amd import config as C, segmentation, vmae

    cfg = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
    G = segmentation.FlowGenerator(predictor=vmae.PretrainVisionTransformer(cfg).cuda().eval(), imagenet_normalize_inputs=True, temporal_dim=2)
    gen = torch.Generator().manual_seed(2)
    n, S_ = 16, 3
    x = torch.rand(2, 1, 3, 32, 32, generator=gen).cuda()
    passive = (torch.arange(2 * n) >= n)[None].expand(2 * S_, -1).cuda()
    active = passive.clone()
    active[torch.arange(2 * S_), n + torch.arange(2 * S_)] = False
    shifts = torch.tensor([[1, 0], [0, -1], [0, 0], [-1, 1], [2, 0], [0, 3]], dtype=torch.int32)
    before = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match="one movie"):
        G._shift_rows(x, passive, active, shifts, 1, True, samples_per_movie=S_, num_frames=2)
    assert torch.cuda.memory_allocated() == before
    for b in range(2):
        rows = slice(b * S_, (b + 1) * S_)
        want_x, want_m = G._shift_rows(x[b:b + 1].expand(-1, 2, -1, -1, -1), passive[rows], active[rows], shifts[rows], 1, True, samples_per_movie=S_)
        got_x, got_m = G._shift_rows(x[b:b + 1], passive[rows], active[rows], shifts[rows], 1, True, samples_per_movie=S_, num_frames=2)
        assert same_bits(got_x, want_x) and torch.equal(got_m, want_m) and not torch.equal(want_x[:, 1], want_x[:, 0])
