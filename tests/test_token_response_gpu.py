"""The response kernel (`cwm_token_response`) on a real MI355X against the float64 restatement (tests/response_restatement.py), on hand-built tokens: no model.

Bounds (derived in the restatement from operation counts; every sum is of non-negative terms): a pixel of the map within gamma(C + 2) of its value, a patch
value within gamma(C P^2 + 2), the peak as a pixel, the mass within gamma(C + 1 + H W), the centroid within gamma(3 (C + 1 + H W) + 2); gamma(n) = n 2^-24 /
(1 - n 2^-24).  The peak index is EQUAL to the restatement's: in every row used the two largest responses are further apart than twice the pixel bound of the
largest (asserted on the inputs themselves, here and without a GPU in tests/test_markers_cpu.py), so no rounding within the bound can change the argmax.

Measured on an MI355X (run with -s), relative to the value: pixels and peak at most 1.5e-7 (bound 3.0e-7), patch values 3.4e-7 (4.6e-5 at P = 8),
mass 1.4e-7 (1.6e-5), centroid 2.0e-7 (4.7e-5); protocol A: the call returned with a 29 ms delay still running."""
import ctypes

import pytest
import torch

import response_restatement as RR
import stream_order as SO
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu

# name -> (T, C, H, W, P, floats the token pointer is off the 16-byte grid): the three patch sizes, a grid that is not square, the generic kernel (C != 3, and
# C = 3 with unaligned tokens)
GEOMETRIES = {
    "p4": (2, 3, 16, 16, 4, 0),
    "p8_wide": (2, 3, 16, 32, 8, 0),
    "p16": (2, 3, 32, 32, 16, 0),
    "one_channel": (2, 1, 16, 16, 4, 0),
    "four_channels": (2, 4, 16, 16, 4, 0),
    "unaligned": (2, 3, 16, 16, 4, 1),
}
ROWS = (1, 5)


def cases(name):
    """(B, shared reference, frame, seed) of a geometry"""
    k = sorted(GEOMETRIES).index(name)
    return [(B, shared, frame, 1000 * k + 100 * B + 10 * shared + frame) for B in ROWS for shared in (True, False) for frame in (0, 1)]


def inputs(name, B, shared, frame, seed):
    """CPU tensors: y [B,Nm,P P C] and y_ref [1 or B,Nm,P P C] seeded normal, mask [B,Nt] with half of each frame's patches masked, at other places in every row:
    frame `frame` has visible patches inside it"""
    T, Cc, H, W, P, _ = GEOMETRIES[name]
    n = (H // P) * (W // P)
    g = torch.Generator().manual_seed(seed)
    mask = torch.zeros((B, T, n), dtype=torch.bool)
    for b in range(B):
        for t in range(T):
            mask[b, t, torch.randperm(n, generator=g)[:n // 2]] = True
    Nm = T * (n // 2)
    y = torch.randn((B, Nm, P * P * Cc), generator=g)
    y_ref = torch.randn((1 if shared else B, Nm, P * P * Cc), generator=g)
    assert mask[:, frame].any(1).all() and (~mask[:, frame]).any(1).all()
    return y, y_ref, mask.view(B, T * n)


def decided(r, Cc):
    """the condition for index equality, on the float64 responses: every row's largest response leads the second by more than twice the pixel bound"""
    gap, top = RR.index_gap(r)
    return bool((gap > 2 * RR.pixel_bound(Cc) * top).all()), float((gap / top).min())


def stream():
    return _lib.current_stream_handle(torch.device("cuda:0"))


def on_device(t, offset=0):
    """a device copy of t whose pointer is `offset` floats off the allocation's (16-byte aligned) start"""
    if not offset:
        return t.cuda()
    buf = torch.empty((t.numel() + offset,), device="cuda", dtype=t.dtype)
    view = buf[offset:].view(t.shape)
    view.copy_(t)
    return view


def run_kernel(y, y_ref, mask, geom, frame, want=("map", "pixels", "index", "stats"), n_vis=None, scratch=True):
    """`cwm_token_response` on device tensors.  Returns (map, pixels, index, stats), None where not asked for; outputs start as NaN / -1"""
    T, Cc, H, W, P = geom[:5]
    B = mask.shape[0]
    h, w = H // P, W // P
    a = _lib.new_token_response_args()
    a.y_ref_dev = _lib.ptr(y_ref)
    a.y_ref_stride_b = 0 if y_ref is None or y_ref.shape[0] == 1 else y_ref.stride(0)
    emap = torch.full((B, h, w), float("nan"), device="cuda") if "map" in want else None
    pixels = torch.full((B, H, W), float("nan"), device="cuda") if "pixels" in want else None
    index = torch.full((B,), -1, device="cuda", dtype=torch.int32) if "index" in want else None
    stats = torch.full((B, 4), float("nan"), device="cuda") if "stats" in want else None
    work = torch.full((B, h, 8), float("nan"), device="cuda") if scratch and (index is not None or stats is not None) else None
    _lib.fill_patch_args(a.base, mask=mask, y=y, geometry=(B, T, Cc, H, W, P), n_vis=(T * h * w - (0 if y is None else y.shape[1])) if n_vis is None else n_vis,
                         frame=frame, map=emap, scratch=work, stream=stream())
    a.pixel_map_dev, a.peak_index_dev, a.stats_dev = _lib.ptr(pixels), _lib.ptr(index), _lib.ptr(stats)
    _lib.check(_lib.get_lib().cwm_token_response(ctypes.byref(a)))
    return emap, pixels, index, stats


def within(name, got, want, rel):
    got, want = got.double().cpu(), want.double().cpu()
    err = (got - want).abs()
    print("%-44s max error %.3e of values up to %.3e (relative bound %.3e)" % (name, err.max().item(), want.abs().max().item(), rel))
    assert bool((err <= rel * want.abs()).all()), (name, (err - rel * want.abs()).max().item())


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_kernel_equals_the_restatement(name):
    T, Cc, H, W, P, off = GEOMETRIES[name]
    for B, shared, frame, seed in cases(name):
        y, y_ref, mask = inputs(name, B, shared, frame, seed)
        r = RR.response(y, y_ref, mask, T, Cc, H, W, P, frame)
        ok, lead = decided(r, Cc)
        assert ok, (name, B, shared, frame, lead)  # no row is left out
        want_index, want_stats = RR.statistics(r)
        emap, pixels, index, stats = run_kernel(on_device(y, off), y_ref.cuda(), mask.cuda(), GEOMETRIES[name], frame)
        tag = "%s B %d %s frame %d" % (name, B, "shared" if shared else "per row", frame)
        within(tag + " pixels", pixels, r, RR.pixel_bound(Cc))
        within(tag + " map", emap, RR.patch_map(r, P), RR.map_bound(Cc, P))
        assert torch.equal(index.cpu().long(), want_index), (tag, index.tolist(), want_index.tolist())
        within(tag + " peak", stats[:, 0], want_stats[:, 0], RR.pixel_bound(Cc))
        within(tag + " mass", stats[:, 1], want_stats[:, 1], RR.mass_bound(Cc, H, W))
        within(tag + " centroid", stats[:, 2:], want_stats[:, 2:], RR.centroid_bound(Cc, H, W))
        vis = ~mask.view(B, T, H // P, W // P)[:, frame]
        assert bool((emap.cpu()[vis] == 0).all()) and bool((emap.cpu()[~vis] > 0).all())  # a visible patch of the frame: exactly 0
        assert bool((stats[:, 0].cpu() == pixels.cpu().view(B, -1).gather(1, want_index[:, None])[:, 0]).all())  # the peak IS the map's value there


def full_frame_case(values, T=2, Cc=3, H=16, W=16, P=4, B=1):
    """frame 0 visible, frame 1 masked; y_ref = 0 and y = 0 but for `values`: {(b, Y, X, c): v}.  Returns device (y, y_ref, mask) and the geometry"""
    gh, gw = H // P, W // P
    n = gh * gw
    y = torch.zeros((B, gh, gw, P, P, Cc))
    for (b, Y, X, c), v in values.items():
        y[b, Y // P, X // P, Y % P, X % P, c] = v
    mask = torch.zeros((B, T, n), dtype=torch.bool)
    mask[:, 1] = True
    return y.view(B, n, P * P * Cc).cuda(), torch.zeros((1, n, P * P * Cc)).cuda(), mask.view(B, T * n).cuda(), (T, Cc, H, W, P)


def test_equal_responses_the_lower_index_wins():
    """2^2 = 4 and 1^2 + 1^2 + 1^2 + 1^2 ... are exact: three pixels of response 4 in different patch rows, lanes and items -- the first in linear order"""
    values = {(0, 9, 3, 0): 2.0, (0, 5, 14, 1): -2.0, (0, 5, 15, 2): 2.0, (0, 12, 0, 0): 1.0,
              (1, 6, 6, 0): 2.0, (1, 6, 5, 2): 2.0, (1, 2, 11, 1): 1.0}
    y, y_ref, mask, geom = full_frame_case(values, B=2)
    emap, pixels, index, stats = run_kernel(y, y_ref, mask, geom, 1)
    assert index.tolist() == [5 * 16 + 14, 6 * 16 + 5]
    assert stats[:, 0].tolist() == [4.0, 4.0] and stats[:, 1].tolist() == [13.0, 9.0]
    # sums of small integers are exact; the one rounding is the division
    want = torch.tensor([[88.0 / 13, 128.0 / 13], [(4 * 6 + 4 * 6 + 2) / 9.0, (4 * 6 + 4 * 5 + 11) / 9.0]], dtype=torch.float64)
    assert bool(((stats[:, 2:].cpu().double() - want).abs() <= RR.EPS * want).all())
    assert pixels[0, 9, 3].item() == 4.0 and pixels[0, 12, 0].item() == 1.0 and pixels.sum().item() == 22.0
    assert emap[0, 2, 0].item() == 4.0 / 16 and emap[0, 1, 3].item() == 8.0 / 16


def test_a_fully_visible_frame_has_no_response():
    y, y_ref, mask, geom = full_frame_case({(0, 3, 3, 0): 5.0})
    emap, pixels, index, stats = run_kernel(y, y_ref, mask, geom, 0)  # frame 0: visible
    assert index.tolist() == [0] and stats.tolist() == [[0.0, 0.0, 0.0, 0.0]]
    assert bool((pixels == 0).all()) and bool((emap == 0).all())
    # nothing masked at all: there are no tokens, and none is asked for
    T, Cc, H, W, P = geom
    nothing = torch.zeros_like(mask)
    emap, pixels, index, stats = run_kernel(None, None, nothing, geom, 1)
    assert index.tolist() == [0] and stats.tolist() == [[0.0, 0.0, 0.0, 0.0]] and bool((pixels == 0).all())
    # a response of one pixel: the centroid is that pixel
    emap, pixels, index, stats = run_kernel(y, y_ref, mask, geom, 1)
    assert index.tolist() == [3 * 16 + 3] and stats.tolist() == [[25.0, 25.0, 3.0, 3.0]]


def test_a_nan_is_the_peak():
    values = {(0, 9, 3, 0): 2.0, (0, 10, 7, 1): float("nan"), (0, 2, 2, 0): 3.0}
    y, y_ref, mask, geom = full_frame_case(values)
    emap, pixels, index, stats = run_kernel(y, y_ref, mask, geom, 1)
    assert index.tolist() == [10 * 16 + 7]
    assert bool(stats.isnan().all())  # the peak, the mass and both centroid coordinates
    assert bool(pixels[0, 10, 7].isnan()) and int(pixels.isnan().sum()) == 1 and int(emap.isnan().sum()) == 1 and bool(emap[0, 2, 1].isnan())
    want = torch.argmax(pixels.cpu().view(1, -1), 1)
    assert want.tolist() == index.tolist()


def test_each_output_alone_and_two_calls_are_bit_equal():
    name = "p8_wide"
    y, y_ref, mask = (t.cuda() for t in inputs(name, 5, False, 1, 77))
    geom = GEOMETRIES[name]
    both = run_kernel(y, y_ref, mask, geom, 1)
    again = run_kernel(y, y_ref, mask, geom, 1)
    assert all(torch.equal(u, v) for u, v in zip(both, again)) and not any(o.isnan().any() for o in both)
    for k, which in enumerate(("map", "pixels", "index", "stats")):
        alone = run_kernel(y, y_ref, mask, geom, 1, want=(which,))
        assert [o is None for o in alone] == [j != k for j in range(4)]
        assert torch.equal(alone[k], both[k]), which
    # arguments that cannot be run are refused, naming what is wrong, and nothing is written
    lib = _lib.get_lib()
    with pytest.raises(RuntimeError, match="no output requested"):
        run_kernel(y, y_ref, mask, geom, 1, want=())
    with pytest.raises(RuntimeError, match="scratch"):
        run_kernel(y, y_ref, mask, geom, 1, want=("index",), scratch=False)
    with pytest.raises(RuntimeError, match="frame = 2 of 2"):
        run_kernel(y, y_ref, mask, geom, 2)
    with pytest.raises(RuntimeError, match="y_ref_dev"):
        run_kernel(y, None, mask, geom, 1)
    assert lib.cwm_last_error() is not None


def test_the_row_of_a_token_is_clamped_into_the_tokens():
    """A mask with more masked tokens than there are token rows: y and y_ref are interior views of larger buffers whose guard rows hold NaN, wide enough that a
    rank that was NOT clamped would still read allocated memory -- and would read a NaN"""
    T, Cc, H, W, P = 2, 3, 16, 16, 4
    n, B = 16, 3
    Nt, Nm = T * n, 10
    guard = Nt
    g = torch.Generator().manual_seed(5)
    bufs = []
    for _ in range(2):
        big = torch.full((guard + B * Nm + guard, P * P * Cc), float("nan"))
        big[guard:guard + B * Nm] = torch.randn((B * Nm, P * P * Cc), generator=g)
        bufs.append(big.cuda())
    y, y_ref = (b[guard:guard + B * Nm].view(B, Nm, P * P * Cc) for b in bufs)
    mask = torch.ones((B, Nt), dtype=torch.bool).cuda()  # 32 masked tokens claimed to be 10
    emap, pixels, index, stats = run_kernel(y, y_ref, mask, (T, Cc, H, W, P), 1, n_vis=Nt - Nm)
    assert not any(o.isnan().any() for o in (emap, pixels, stats)) and bool((index >= 0).all()) and bool((index < H * W).all())
    # every token of frame 1 has rank >= 16 > Nm - 1: all patches show the last token row
    d = (y[:, -1] - y_ref[:, -1]).double().cpu().view(B, P, P, Cc)
    want = (d * d).sum(-1).repeat(1, 4, 4)
    within("clamped rows", pixels, want, RR.pixel_bound(Cc))


def test_late_inputs_and_early_consumers():
    """Protocol A of tests/stream_order.py: the inputs arrive behind a delay on a side stream, the call returns while the delay runs, and its outputs are
    consumed and its inputs overwritten on the stream right after it"""
    name = "p8_wide"
    geom = GEOMETRIES[name]
    y, y_ref, mask = (t.cuda() for t in inputs(name, 5, True, 1, 300))
    mask_p = inputs(name, 5, True, 1, 301)[2].cuda()  # another mask with the same count per row
    call = lambda yy, rr, mm: run_kernel(yy, rr, mm, geom, 1)  # noqa: E731
    truth, poison = [y, y_ref, mask], [SO.poison_like(y), SO.poison_like(y_ref), mask_p]
    first, _ = SO.plain(call, [t.clone() for t in truth])
    want, ms = SO.plain(call, [t.clone() for t in truth])
    assert SO.same(first, want)
    SO.check_poison("token_response", truth, poison, want, call)
    SO.protocol_a("token_response", call, truth, poison, want, ms, True)
