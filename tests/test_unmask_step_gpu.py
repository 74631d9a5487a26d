"""`cwm_unmask_step` on a real MI355X through the C ABI, with synthetic tokens and no model: the distance, the frontier, the picks and the new mask against
the torch restatement (tests/unmask_restatement.py), and the error map and mean against `cwm_patch_error` on the same arguments -- all bit for bit: the
distance is one correctly rounded division of exact integers, the selection is a total order, and the map is the same kernel's.

Shapes: a 3 x 5 grid (the minimum side, not square, one partly filled pass of the 256 lanes), 28 x 28 (four passes, the last partly filled), 56 x 56 (3136
cells: the largest square grid under the 4096-cell LDS limit), and B = 3 rows sharing one movie at batch stride 0."""
import ctypes

import pytest
import torch

import unmask_restatement as UR
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
P, Cc, T, F = 4, 3, 2, 1
GEOMETRIES = {"g3x5": (3, 12, 20, False), "g28": (2, 112, 112, False), "g56": (1, 224, 224, False), "stride0": (3, 12, 20, True)}
_CACHE = {}


def stream():
    return _lib.current_stream_handle(torch.device("cuda:0"))


def frames(name):
    """(x [B,T,C,H,W] on the device, h, w), made once per geometry and never written"""
    if name not in _CACHE:
        B, H, W, shared = GEOMETRIES[name]
        g = torch.Generator().manual_seed(11 + len(name))
        x = torch.rand((1 if shared else B, T, Cc, H, W), generator=g).cuda()
        _CACHE[name] = (x.expand(B, -1, -1, -1, -1) if shared else x, H // P, W // P)
    return _CACHE[name]


def tokens_of(x, mask):
    """the frames' own patches as tokens, feature order (ph pw c), one row per masked token: a prediction without error"""
    B, _, _, H, W = x.shape
    h, w = H // P, W // P
    pt = x.reshape(B, T, Cc, h, P, w, P).permute(0, 1, 3, 5, 4, 6, 2).reshape(B, T * h * w, P * P * Cc)
    return torch.stack([pt[b][mask[b]] for b in range(B)], 0).contiguous()


def frame_mask(B, h, w, masked_cells_per_row):
    """[B, Nt] bool on the CPU: frame 0 visible, frame 1 masked at the listed cells"""
    n = h * w
    m = torch.zeros((B, T * n), dtype=torch.bool)
    for b, cells in enumerate(masked_cells_per_row):
        m[b, n + torch.as_tensor(cells, dtype=torch.long)] = True
    return m


def fill(a, x, mask_dev, y, n_vis, region=None, **outputs):
    B, _, _, H, W = x.shape
    _lib.fill_patch_args(a.base, x=x, mask=mask_dev, region=region, y=y, geometry=(B, T, Cc, H, W, P), n_vis=n_vis, frame=F, stream=stream(), **outputs)


def patch_error(x, mask_dev, y, n_vis, region=None):
    B, _, _, H, W = x.shape
    a = _lib.new_unmask_step_args()
    emap = torch.full((B, T, H // P, W // P), -7.0, device="cuda")
    mean = torch.full((B,), -7.0, device="cuda")
    fill(a, x, mask_dev, y, n_vis, region, map=emap, mean=mean)
    _lib.check(_lib.get_lib().cwm_patch_error(ctypes.byref(a.base)))
    return emap, mean


def run_on_device(x, md, y, k, thr, e=None, region=None, use_scratch=False):
    """one call on the current stream, device tensors in and out and no synchronisation: (map, mean, picks, mask_out, dist, frontier).  Outputs start from a
    sentinel so that what the call does not write shows."""
    B, _, _, H, W = x.shape
    h, w = H // P, W // P
    n = h * w
    a = _lib.new_unmask_step_args()
    emap = torch.full((B, T, h, w), -7.0, device="cuda")
    mean = torch.full((B,), -7.0, device="cuda")
    fill(a, x, md, y, T * n - (0 if y is None else y.shape[1]), region, **(dict(scratch=emap) if use_scratch else dict(map=emap, mean=mean)))
    thr_dev = torch.full((1,), thr, dtype=torch.float32, device="cuda")
    mask_out, picks = torch.full_like(md, True), torch.full((B, k), -9, dtype=torch.int32, device="cuda")
    dist, front = torch.full((B, n), -7.0, device="cuda"), torch.full((B, n), 9, dtype=torch.uint8, device="cuda")
    a.frame, a.num_reveal, a.mode, a.threshold_dev, a.e_dev = F, k, int(e is not None), thr_dev.data_ptr(), _lib.ptr(e)
    a.mask_out_dev, a.picks_dev, a.dist_dev, a.frontier_dev = mask_out.data_ptr(), picks.data_ptr(), dist.data_ptr(), front.data_ptr()
    _lib.check(_lib.get_lib().cwm_unmask_step(ctypes.byref(a)))
    return emap, mean, picks, mask_out, dist, front


def run(x, mask, y, k, thr, e=None, region=None, use_scratch=False):
    """one call on CPU masks / draws; returns a dict of CPU tensors"""
    md = mask.cuda()
    out = run_on_device(x, md, y, k, thr, None if e is None else e.cuda(), region, use_scratch)
    torch.cuda.synchronize()
    assert torch.equal(md.cpu(), mask)  # the input mask is not written
    return dict(zip(("map", "mean", "picks", "mask_out", "dist", "frontier"), (t.cpu() for t in out)))


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def check(name, mask, y, k, radius, e=None, region=None):
    x, h, w = frames(name)
    thr = UR.threshold(h, w, radius)
    got = run(x, mask, y, k, thr, e, region)
    emap, mean = patch_error(x, mask.cuda(), y, T * h * w - int(mask[0].sum()), region)
    assert torch.equal(bits(got["map"]), bits(emap.cpu())) and torch.equal(bits(got["mean"]), bits(mean.cpu())), "map / mean differ from cwm_patch_error"
    want = UR.step(mask, emap.cpu(), T, h, w, F, k, thr, e, None if region is None else region.cpu())
    for key in ("dist", "frontier", "picks", "mask_out"):
        assert torch.equal(bits(got[key]), bits(want[key])), (name, key, k, radius)
    return got, want


def random_tokens(mask, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((mask.shape[0], int(mask[0].sum()), P * P * Cc), generator=g).cuda()


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_fully_masked_frame(name):
    """no visible cell: d = 0, every cell is frontier under any radius, the k largest errors go"""
    x, h, w = frames(name)
    B, n = x.shape[0], h * w
    mask = frame_mask(B, h, w, [range(n)] * B)
    y = random_tokens(mask, 1)
    for k, radius in ((1, 1), (5, None), (min(64, n), 2)):
        got, _ = check(name, mask, y, k, radius)
        assert (got["dist"] == 0).all() and (got["frontier"] == 1).all() and (got["picks"] >= n).all()
        assert got["mask_out"].sum(1).tolist() == [n - k] * B


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_one_visible_corner_and_a_frontier_smaller_than_k(name):
    x, h, w = frames(name)
    B, n = x.shape[0], h * w
    mask = frame_mask(B, h, w, [[c for c in range(n) if c != (w - 1 if b % 2 else n - w)] for b in range(B)])  # bottom-left, top-right, ...
    y = random_tokens(mask, 2)
    for k, radius in ((1, 1), (5, 1), (5, 2), (min(64, n - 1), 1), (5, None)):
        got, want = check(name, mask, y, k, radius)
        nf = want["frontier"].sum(1)
        if radius is not None and int(nf.max()) < k:  # the row fills up from the other masked cells: the frontier first, all of it
            for b in range(B):
                first = set((got["picks"][b, : int(nf[b])] - n).tolist())
                assert first == set(torch.nonzero(want["frontier"][b]).view(-1).tolist())
    if name == "g28":
        assert int(UR.frontier(mask[:, n:], h, w, UR.threshold(h, w, 1)).sum(1).max()) == 3 < 5


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_all_but_k_visible_and_a_row_short_of_masked_cells(name):
    x, h, w = frames(name)
    B, n = x.shape[0], h * w
    g = torch.Generator().manual_seed(3)
    k = 5
    mask = frame_mask(B, h, w, [torch.randperm(n, generator=g)[:k].tolist() for _ in range(B)])
    y = random_tokens(mask, 3)
    got, _ = check(name, mask, y, k, 1)
    assert not got["mask_out"].any()  # exactly the k masked cells went
    got, _ = check(name, mask, y, 8, 2)  # three picks too many: -1, and nothing cleared for them
    assert (got["picks"][:, 5:] == -1).all() and (got["picks"][:, :5] >= n).all() and not got["mask_out"].any()
    if B > 1:  # rows of equal count, one of them with most of its masked tokens in the other frame
        mask[1] = False
        mask[1, :3] = True
        mask[1, n + 1], mask[1, n + n - 1] = True, True
        got, _ = check(name, mask, y, 4, None)
        assert (got["picks"][1, 2:] == -1).all() and sorted(got["picks"][1, :2].tolist()) == [n + 1, 2 * n - 1]
        assert got["mask_out"][1].nonzero().view(-1).tolist() == [0, 1, 2]  # the other frame's mask bytes are copied


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_zero_errors_leave_the_choice_to_the_index_and_a_nan_goes_first(name):
    x, h, w = frames(name)
    B, n = x.shape[0], h * w
    g = torch.Generator().manual_seed(4)
    mask = frame_mask(B, h, w, [torch.randperm(n, generator=g)[: (2 * n) // 3].tolist() for _ in range(B)])
    y = tokens_of(x, mask.cuda())
    got, want = check(name, mask, y, 5, 1)
    assert (got["map"][:, F] == 0).all()
    for b in range(B):  # all keys equal: the five lowest frontier cells, or the frontier and then the lowest others
        fr = torch.nonzero(want["frontier"][b]).view(-1).tolist()
        rest = [c for c in torch.nonzero(mask[b, n:]).view(-1).tolist() if c not in fr]
        assert (got["picks"][b] - n).tolist() == (fr + rest)[:5]
    y = y.clone()
    y[0, y.shape[1] - 1, 7] = float("nan")  # the last masked token of row 0: the highest masked cell of frame 1
    got, want = check(name, mask, y, 5, None)
    last = int(torch.nonzero(mask[0, n:]).view(-1)[-1])
    assert torch.isnan(got["map"][0, F].view(-1)[last]) and int(got["picks"][0, 0]) == n + last


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_race_mode_region_weights_and_scratch(name):
    x, h, w = frames(name)
    B, n = x.shape[0], h * w
    g = torch.Generator().manual_seed(5)
    mask = frame_mask(B, h, w, [torch.randperm(n, generator=g)[: n // 2 + 1].tolist() for _ in range(B)])
    y = random_tokens(mask, 5)
    e = torch.empty((B, n)).exponential_(generator=g)
    top, _ = check(name, mask, y, 5, 2)
    race, _ = check(name, mask, y, 5, 2, e=e)
    assert not torch.equal(top["picks"], race["picks"])
    region = (torch.randint(0, 5, (B, T, h, w), generator=g).float() / 2).cuda()
    check(name, mask, y, 5, 1, region=region)
    check(name, mask, y, min(64, n // 2), None, e=e, region=region)
    # the map in scratch_dev alone, no mean: same picks; and the same call twice gives the same bits
    thr = UR.threshold(h, w, 2)
    a = run(x, mask, y, 5, thr, e, use_scratch=True)
    b = run(x, mask, y, 5, thr, e)
    assert torch.equal(a["picks"], race["picks"]) and torch.equal(bits(a["map"]), bits(race["map"])) and (a["mean"] == -7).all()
    for key in a:
        if key != "mean":
            assert torch.equal(bits(a[key]), bits(b[key])), key


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_nothing_to_reveal_reads_only_the_mask(name):
    """num_reveal = 0 with NULL frames, tokens, region and map: dist (both self_mask values) and frontier alone are written"""
    x, h, w = frames(name)
    B, n = x.shape[0], h * w
    g = torch.Generator().manual_seed(6)
    mask = frame_mask(B, h, w, [torch.randperm(n, generator=g)[: (3 * n) // 4].tolist() for _ in range(B)])
    md = mask.cuda()
    for self_mask in (0, 1):
        a = _lib.new_unmask_step_args()
        _lib.fill_patch_args(a.base, mask=md, geometry=(B, T, 0, h * P, w * P, P), stream=stream())
        a.frame, a.self_mask = F, self_mask
        thr = torch.tensor([UR.threshold(h, w, 1)]).cuda()
        dist = torch.full((B, n), -7.0, device="cuda")
        front = torch.full((B, n), 9, dtype=torch.uint8, device="cuda")
        a.threshold_dev, a.dist_dev, a.frontier_dev = thr.data_ptr(), dist.data_ptr(), front.data_ptr()
        _lib.check(_lib.get_lib().cwm_unmask_step(ctypes.byref(a)))
        assert torch.equal(bits(dist.cpu()), bits(UR.distance(mask[:, n:], h, w, self_mask=bool(self_mask))))
        assert torch.equal(front.cpu().bool(), UR.frontier(mask[:, n:], h, w, UR.threshold(h, w, 1)))


def test_argument_errors_launch_nothing():
    x, h, w = frames("g3x5")
    B, n = x.shape[0], h * w
    mask = frame_mask(B, h, w, [range(n)] * B).cuda()
    y = random_tokens(mask.cpu(), 7)
    lib = _lib.get_lib()

    def args():
        a = _lib.new_unmask_step_args()
        emap = torch.empty((B, T, h, w), device="cuda")
        fill(a, x, mask, y, n, map=emap)
        out = torch.full_like(mask, True)
        picks = torch.full((B, 64), -9, dtype=torch.int32, device="cuda")
        a.frame, a.num_reveal, a.mask_out_dev, a.picks_dev = F, 2, out.data_ptr(), picks.data_ptr()
        return a, (emap, out, picks)

    def refused(a, keep, text):
        assert lib.cwm_unmask_step(ctypes.byref(a)) != 0
        assert text in lib.cwm_last_error(), lib.cwm_last_error()
        torch.cuda.synchronize()
        assert keep[1].all() and (keep[2] == -9).all()  # nothing ran

    a, keep = args()
    a.mask_out_dev = mask.data_ptr()
    refused(a, keep, b"alias")
    a, keep = args()
    a.mask_out_dev = mask.data_ptr() + n  # a partial overlap is aliasing too
    refused(a, keep, b"alias")
    a, keep = args()
    a.num_reveal = 65
    refused(a, keep, b"num_reveal")
    a, keep = args()
    a.struct_size += 8
    refused(a, keep, b"struct_size")
    a, keep = args()
    a.base.H = 8  # a 2 x 5 grid
    refused(a, keep, b"at least 3 x 3")
    a, keep = args()
    a.frame = T
    refused(a, keep, b"frame")
    a, keep = args()
    a.base.map_dev = None
    refused(a, keep, b"scratch_dev")
    a, keep = args()
    a.mode = 1  # race without e_dev
    refused(a, keep, b"e_dev")
    a, keep = args()
    a.base.H, a.base.W = 4 * 65, 4 * 64  # 4160 cells
    refused(a, keep, b"4096")
    a, keep = args()
    a.base.n_vis = 2 * n + 1  # cwm_patch_error's own check, still before the first launch
    refused(a, keep, b"n_vis")
    a, keep = args()
    assert lib.cwm_unmask_step(ctypes.byref(a)) == 0
    torch.cuda.synchronize()
    flat = keep[2].view(-1)  # picks_dev is [B, k] with k = 2: the first 2 B slots of the buffer
    assert (flat[: 2 * B] >= n).all() and (flat[2 * B:] == -9).all()
