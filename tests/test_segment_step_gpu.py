"""`cwm_segment_step` on a real MI355X through the C ABI against the NumPy restatement (tests/segment_restatement.py), for EQUALITY: every input is exact in
float32 (the restatement's docstring says why), so votes, segments, stats and picks agree integer for integer and seed_ref / cover bit for bit.

Shapes: 24 x 24 P = 8 (3 x 3 grid), 32 x 32 P = 4 (8 x 8 grid: ring and selection), 24 x 40 P = 8 (bit rows that are no whole word, H != W), 64 x 64 P = 16
(two words per bit row); S in {1, 5, 70} (70: past one wave of samples).  Layouts: the sample-outermost view, packed contiguous, a strided slice [..., ::2], a
base pointer one float off.  Every output sits between guard bytes that must survive the call."""
import ctypes

import numpy as np
import pytest
import torch

import segment_restatement as SR
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
GUARD = 0xA5
LAYOUTS = ("view", "packed", "strided", "offset")
OUT = ("seed_ref", "votes", "segment", "cover", "stats", "picks", "active", "passive")


def stream():
    return _lib.current_stream_handle(torch.device("cuda:0"))


def lay_out(flows, layout):
    """a device tensor [B,2,H,W,S] equal to `flows` in the given layout"""
    f = torch.from_numpy(np.ascontiguousarray(flows))
    B, C, H, W, S = f.shape
    if layout == "view":     # the `_batch_to_samples` view of a [(b s), 1, C, H, W] batch
        return f.permute(0, 4, 1, 2, 3).contiguous().cuda().permute(0, 2, 3, 4, 1)
    if layout == "packed":
        return f.cuda()
    if layout == "strided":  # every second sample of a packed tensor of 2 S samples
        wide = torch.full((B, C, H, W, 2 * S), float("nan"))
        wide[..., ::2] = f
        return wide.cuda()[..., ::2]
    buf = torch.zeros(f.numel() + 1, device="cuda")  # "offset": packed, the base pointer one float past an aligned address
    buf[1:] = f.reshape(-1).cuda()
    return buf[1:].view(B, C, H, W, S)


def guarded(shape, dtype):
    """(the buffer, its interior view): 64 guard bytes on either side of the output"""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((nbytes + 128,), GUARD, dtype=torch.uint8, device="cuda")
    return buf, buf[64:64 + nbytes].view(dtype).view(*shape)


def run(flows, seeds, P, layout="view", shape=None, skip=(), dirs=None, keys=None, k_active=0, k_passive=0, min_seed_mag=0.0, abs_thresh=0.0, rel_thresh=0.5,
        vote_frac=0.5, cos_min=0.0, inside_frac=1.0, ring_radius=1, expect=0, mutate=None):
    """one call; returns (rc, dict of CPU arrays, the device flows); every output not in `skip` is allocated between guards that are checked"""
    init = flows is None
    if init:
        B, H, W = shape
        S, fd = 0, None
    else:
        fd = lay_out(flows, layout) if not torch.is_tensor(flows) else flows
        B, _, H, W, S = fd.shape
    n, K = (H // P) * (W // P), k_active + k_passive
    shapes = {"seed_ref": ((B, S), torch.float32), "votes": ((B, H, W), torch.uint8), "segment": ((B, H, W), torch.uint8), "cover": ((B, n), torch.float32),
              "stats": ((B, 4), torch.int32), "picks": ((B, K), torch.int32), "active": ((B, 2 * n), torch.uint8), "passive": ((B, 2 * n), torch.uint8)}
    bufs = {k: guarded(*shapes[k]) for k in OUT if k not in skip}
    a = _lib.new_segment_step_args()
    _lib.fill_patch_args(a.base, geometry=(B, 2, 0, H, W, P), stream=stream())
    if not init:
        a.flows_dev, a.C, a.S = fd.data_ptr(), 2, S
        for i, st in enumerate(fd.stride()):
            a.flow_strides[i] = st
    sd = torch.as_tensor(np.asarray(seeds, np.int32)).cuda()
    dd = None if dirs is None else torch.as_tensor(np.asarray(dirs, np.float32)).cuda()
    kd = None if keys is None else torch.as_tensor(np.asarray(keys, np.float32)).cuda()
    a.seeds_dev, a.dirs_dev, a.keys_dev = sd.data_ptr(), _lib.ptr(dd), _lib.ptr(kd)
    a.min_seed_mag, a.abs_thresh, a.rel_thresh, a.vote_frac, a.cos_min, a.inside_frac = min_seed_mag, abs_thresh, rel_thresh, vote_frac, cos_min, inside_frac
    a.k_active, a.k_passive, a.ring_radius = k_active, k_passive, ring_radius
    for k, field in zip(OUT, ("seed_ref_dev", "votes_dev", "segment_dev", "cover_dev", "stats_dev", "picks_dev", "active_out_dev", "passive_out_dev")):
        setattr(a, field, bufs[k][1].data_ptr() if k in bufs else None)
    if mutate:
        mutate(a)
    rc = _lib.get_lib().cwm_segment_step(ctypes.byref(a))
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.get_lib().cwm_last_error())
    out = {}
    for k, (buf, view) in bufs.items():
        nb = buf.numel() - 128
        assert bool((buf[:64] == GUARD).all()) and bool((buf[64 + nb:] == GUARD).all()), "guard bytes around %s" % k
        out[k] = view.cpu().numpy()
    return rc, out, fd


def check(flows, seeds, P, layout="view", shape=None, **kw):
    want = SR.step(flows, seeds, P, shape=shape, **{k: v for k, v in kw.items() if k != "skip"})
    _, got, _ = run(flows, seeds, P, layout, shape=shape, **kw)
    B = want["votes"].shape[0]
    sel = kw.get("k_active", 0) > 0
    for k, v in got.items():
        if k in ("picks", "active", "passive") and not sel:
            assert (v.view(np.uint8) == GUARD).all(), "%s written without a selection" % k
            continue
        w = want[k].reshape(v.shape)
        if v.dtype == np.float32:
            assert np.array_equal(np.isnan(v), np.isnan(w)) and np.array_equal(np.nan_to_num(v).view(np.int32), np.nan_to_num(w).view(np.int32)), (k, layout)
        else:
            assert np.array_equal(v, w), (k, layout)
    return want


_CASES = {}


def case(name):
    """(flows, seeds, P, kwargs) of a named case, built once and not written"""
    if name not in _CASES:
        kw = dict(min_seed_mag=0.5, abs_thresh=1.0)
        if name == "hand":
            f, seeds, kw = SR.hand_worked()
            _CASES[name] = (f, seeds, 8, kw)
        elif name == "ring32":  # 8 x 8 grid, selection and ring, two rows with different seeds
            m = np.zeros((32, 32), bool)
            m[8:20, 8:22] = True
            f = np.concatenate([SR.flows_of(m, (1, 2, 3, 0, 1)), SR.flows_of(m, (2, 0, 0, 3, 1))], 0)
            _CASES[name] = (f, [[9, 9], [0, 31]], 4, dict(kw, k_active=5, k_passive=6, vote_frac=0.6))
        elif name == "wide40":  # 24 x 40: a bit row of 40 bits = one word and a quarter
            m = np.zeros((24, 40), bool)
            m[3:21, 5:38] = True
            m[10:12, 30:34] = False
            _CASES[name] = (SR.flows_of(m, (1, 1, 2, 3, 1)), [[12, 33]], 8, dict(kw, k_active=3, k_passive=3))
        elif name == "p16":     # 64 x 64, P = 16: a cell's row is half a word
            m = np.zeros((64, 64), bool)
            m[10:50, 20:60] = True
            _CASES[name] = (SR.flows_of(m, (1, 2, 1, 3, 2), base=(3.0, 4.0)), [[17, 40]], 16, dict(kw, k_active=2, k_passive=4, inside_frac=0.5))
        elif name == "s70":     # 70 samples whose scale cycles through 0 .. 4: past one wave of samples, some not valid
            m = np.zeros((24, 24), bool)
            m[2:22, 3:20] = True
            masks = np.broadcast_to(m, (70, 24, 24)).copy()
            masks[1::3, 12:22] = False  # a third of the samples move the upper half only
            _CASES[name] = (SR.flows_of(masks, [s % 5 for s in range(70)]), [[5, 5]], 8, dict(kw, vote_frac=0.7, k_active=2, k_passive=2))
        elif name == "s1":
            m = np.zeros((24, 24), bool)
            m[0:9, 0:24] = True
            _CASES[name] = (SR.flows_of(m, (2,)), [[0, 23]], 8, dict(kw, k_active=1, k_passive=1))
    return _CASES[name]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["hand", "ring32", "wide40", "p16", "s70", "s1"])
def test_cases_in_every_layout(name, layout):
    f, seeds, P, kw = case(name)
    want = check(f, seeds, P, layout, **kw)
    if name == "hand":
        assert want["stats"].tolist() == [[4, 192, 232, 1]]


@pytest.mark.parametrize("shape", [(24, 24), (24, 40), (64, 64)])
def test_serpentine_spiral_and_full_image(shape):
    H, W = shape
    P = 16 if H == 64 else 8
    kw = dict(min_seed_mag=0.1, abs_thresh=1.0, vote_frac=1.0)
    m = SR.serpentine(H, W)
    want = check(SR.flows_of(m, (1, 2)), [[0, 0]], P, **kw)
    assert want["stats"][0, 1] == m.sum() == want["stats"][0, 2] and (shape != (24, 24) or m.sum() == 300)
    sp = SR.spiral(H, W)
    want = check(SR.flows_of(sp, (4,)), [[0, 3]], P, "packed", **kw)
    assert want["stats"][0, 1] == sp.sum() and SR.components(sp).max() == 1
    want = check(SR.flows_of(np.ones((H, W), bool), (1, 3)), [[H - 1, W - 1]], P, k_active=3, k_passive=2, **kw)
    assert want["stats"][0, 1] == H * W and (want["cover"] == 1).all() and (want["picks"][0, 3:] == -1).all()


def test_diagonal_touch_empty_seed_cell_and_seeds_outside():
    m = SR.diagonal_pair(24, 24)
    f = SR.flows_of(m, (1, 1, 3))
    kw = dict(min_seed_mag=0.1, abs_thresh=1.0)
    want = check(f, [[3, 3]], 8, **kw)
    assert want["stats"].tolist() == [[3, 36, 72, 1]]
    # the seed cell (2, 2) holds no moving pixel (min_seed_mag 0 keeps the samples valid): no candidate in it, the segment is empty, active = c0 alone
    want = check(f, [[20, 20]], 8, k_active=3, k_passive=2, **dict(kw, min_seed_mag=0.0))
    assert want["stats"].tolist() == [[3, 0, 72, 0]] and want["picks"].tolist() == [[9 + 8, -1, -1, -1, -1]]
    want = check(np.concatenate([f, f], 0), [[-100, 2 ** 31 - 1], [-2 ** 31, -1]], 8, k_active=2, k_passive=1, **kw)  # clamped to (0, 23) and (0, 0)
    assert want["stats"][:, 3].tolist() == [0, 1] and want["picks"][:, 0].tolist() == [9 + 2, 9 + 0]


def test_nan_and_inf():
    m = np.zeros((24, 24), bool)
    m[0:12, 0:12] = True
    f = SR.flows_of(m, (1, 2, 1, 4))
    f[0, 0, 2, 3, 1] = np.nan
    f[0, 1, 9, 9, 0] = np.nan
    f[0, 0, 10, 10, 2] = np.inf
    keys = np.zeros((1, 2, 9), np.float32)
    keys[0, 0, 3], keys[0, 0, 1], keys[0, 1, 5], keys[0, 1, 2] = np.nan, np.inf, np.nan, -np.inf
    for layout in LAYOUTS:
        want = check(f, [[0, 0]], 8, layout, min_seed_mag=0.5, abs_thresh=1.0, vote_frac=1.0, k_active=3, k_passive=3, inside_frac=0.25, keys=keys)
        assert want["stats"][0, 0] == 3 and np.isnan(want["seed_ref"][0, 1]) and want["votes"][0, 9, 9] == 2
        assert want["picks"][0].tolist() == [9 + 0, 9 + 3, 9 + 1, 9 + 5, 9 + 6, 9 + 7]  # NaN keys first, -inf last; cell 4 is covered to 15/64 only
    f[0, 0, 0, 0, :] = np.inf
    check(f, [[0, 0]], 8, min_seed_mag=0.5, abs_thresh=1.0, vote_frac=1.0)
    f[...] = np.nan
    want = check(f, [[0, 0]], 8, min_seed_mag=0.5, abs_thresh=1.0, k_active=2, k_passive=2)
    assert want["stats"].tolist() == [[0, 0, 0, 0]]


def test_directions():
    m = np.zeros((24, 24), bool)
    m[4:20, 4:20] = True
    f = SR.flows_of(m, (1, 1, 1))
    f[0, :, 12:20, 4:20, 1] *= -1
    dirs = [(8, 6)] * 3
    for layout in LAYOUTS:
        want = check(f, [[5, 5]], 8, layout, dirs=dirs, cos_min=1.0, vote_frac=1.0, min_seed_mag=0.1, abs_thresh=1.0)
        assert want["stats"].tolist() == [[3, 128, 128, 1]]
    check(f, [[5, 5]], 8, dirs=dirs, cos_min=-1.0, vote_frac=1.0, min_seed_mag=0.1, abs_thresh=1.0)


@pytest.mark.parametrize("skip", ["segment", "cover", "stats", "picks", "active", "passive"])
def test_every_optional_output_null_in_turn(skip):
    f, seeds, P, kw = case("ring32")
    check(f, seeds, P, skip=(skip,), **kw)


def test_init_step_and_determinism():
    want = check(None, [[10, 5], [40, -1]], 8, shape=(2, 24, 24), k_active=3, k_passive=2)
    assert want["picks"][:, 0].tolist() == [9 + 3, 9 + 6] and not want["votes"].any()
    check(None, [[10, 5]], 8, shape=(1, 24, 24), k_active=1, skip=("votes", "seed_ref"))
    f, seeds, P, kw = case("s70")
    for layout in ("view", "packed"):
        _, a, fd = run(f, seeds, P, layout, **kw)
        _, b, _ = run(fd, seeds, P, layout, **kw)
        assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def test_limits_name_their_field_and_launch_nothing():
    """every output keeps its guard pattern: nothing was launched"""
    f, seeds, P, kw = case("hand")
    lib = _lib.get_lib()

    def refused(word, flows=f, P=P, mutate=None, shape=None, skip=(), **over):
        _, got, _ = run(flows, seeds if shape is None else [[0, 0]] * shape[0], P, shape=shape, expect=-1, mutate=mutate, skip=skip, **dict(kw, **over))
        msg = lib.cwm_last_error().decode()
        assert word in msg and "cwm_segment_step" in msg, msg
        assert all((v.view(np.uint8) == GUARD).all() for v in got.values()), msg

    refused("C = 3", mutate=lambda a: setattr(a, "C", 3))
    refused("base.P", mutate=lambda a: setattr(a.base, "P", 5))
    refused("base.H", mutate=lambda a: setattr(a.base, "H", 20))
    refused("base.W", mutate=lambda a: setattr(a.base, "W", 28))
    refused("base.T", mutate=lambda a: setattr(a.base, "T", 3))
    refused("S = 256", mutate=lambda a: setattr(a, "S", 256))
    refused("S = 0", mutate=lambda a: setattr(a, "S", 0))
    refused("S = 5 without flows_dev", mutate=lambda a: setattr(a, "flows_dev", None))
    refused("k_active", k_active=65)
    refused("k_passive", k_active=1, k_passive=65)
    refused("ring_radius", ring_radius=0)
    refused("votes_dev", skip=("votes",))
    refused("seed_ref_dev", skip=("seed_ref",))
    refused("struct_size", mutate=lambda a: setattr(a, "struct_size", a.struct_size - 8))
    refused("pixels", flows=None, P=16, shape=(1, 1024, 512))       # 2^19 pixels
    refused("n = 8192", flows=None, P=4, shape=(1, 256, 512))       # 2^17 pixels, 8192 patches
    refused("words", flows=None, P=16, shape=(1, 16384, 16))        # 2^18 pixels, 1024 patches, but 16384 one-word bit rows


def test_largest_image():
    """512 x 512, P = 16: 2^18 pixels, 8192 words per bitmap (all 64 KiB of dynamic LDS), 1024 cells = four per thread of the selection.  The serpentine is the
    slowest component there is for the sweeps (256 rows of 16 words joined at alternating ends); the loop's cap is 2^18 + 1 and is not what ends it."""
    H = W = 512
    m = SR.serpentine(H, W)
    want = check(SR.flows_of(m, (2,)), [[0, 0]], 16, "packed", min_seed_mag=0.1, abs_thresh=1.0)
    assert want["stats"][0, 1] == m.sum() == 256 * 512 + 256
    m = np.zeros((H, W), bool)
    m[100:300, 150:420] = True
    m[300:310, 200:210] = True
    keys = np.random.default_rng(5).integers(0, 4, (1, 2, 1024)).astype(np.float32)  # many ties
    want = check(SR.flows_of(m, (1, 3), base=(3.0, 4.0)), [[305, 205]], 16, "view", min_seed_mag=0.1, abs_thresh=1.0, k_active=40, k_passive=64, keys=keys)
    assert want["stats"].tolist() == [[2, 200 * 270 + 100, 200 * 270 + 100, 1]] and (want["picks"] >= 0).all()
