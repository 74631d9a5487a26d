"""`cwm_flow_consistency` on a real MI355X through the C ABI against the NumPy restatement (tests/flow_consistency_restatement.py), for EQUALITY: floats are
compared as bit patterns, so NaN, the sign of zero and every last bit of `res` count -- a fused multiply-add anywhere in the kernel's arithmetic shows here.

Shapes: 4 x 4 (every pixel is a border pixel, one thread owns a row), 8 x 12, 20 x 12 (partial tiles, no cells), 24 x 40 with P = 8, 16 x 80 with P = 4 and 16
(crosses a 64-column tile edge), 64 x 64 (several tiles per row of the batch), 512 x 512 once (the limit).  Flow layouts, for a and o alike: packed, a pair
[:, t] of a [B,T,2,H,W] tensor, a channel-strided view, a base pointer four bytes off a 16-byte address; whatever surrounds a plane is NaN (or 1e9), so a tap
beyond the plane would show.  Every output sits between 64 guard bytes of 0xA5, and can be placed four bytes off a 16-byte address."""
import ctypes

import numpy as np
import pytest
import torch

import flow_consistency_restatement as R
from counterfactualworldmodels_amd import _lib

pytestmark = pytest.mark.gpu
GUARD = 0xA5
OUT = R.NAMES
FIELD = dict(code="code_dev", res="res_dev", masked="masked_dev", cell="cell_dev", stats="stats_dev")
LAYOUTS = ("packed", "pair", "channel", "offset")
P_OF = {(4, 4): (4,), (8, 12): (4,), (20, 12): (0,), (24, 40): (8,), (16, 80): (4, 16), (64, 64): (8,)}
assert tuple(P_OF) == R.SHAPES


def lay_out(f, layout, fill=float("nan")):
    """a device view [B,2,H,W] float32 equal to `f` in the given layout; everything around its planes holds `fill`"""
    t = torch.from_numpy(np.ascontiguousarray(f, np.float32))
    B, _, H, W = t.shape
    if layout == "packed":
        return t.cuda()
    if layout == "pair":  # pair 1 of a [B,3,2,H,W] tensor
        wide = torch.full((B, 3, 2, H, W), fill)
        wide[:, 1] = t
        return wide.cuda()[:, 1]
    if layout == "channel":  # channels 1 and 3 of a [B,5,H,W] tensor
        wide = torch.full((B, 5, H, W), fill)
        wide[:, 1::2] = t
        v = wide.cuda()[:, 1::2]
        assert v.stride(1) == 2 * H * W
        return v
    buf = torch.full((t.numel() + 8,), fill, dtype=torch.float32, device="cuda")  # "offset": packed, four bytes past an aligned address, guard elements around
    buf[5:5 + t.numel()] = t.reshape(-1).cuda()
    v = buf[5:5 + t.numel()].view(B, 2, H, W)
    assert v.data_ptr() % 16 == 4
    return v


def guarded(shape, dtype, shift=0):
    """(the buffer, its interior view): 64 guard bytes on either side (64 + shift in front)"""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((nbytes + 128 + shift,), GUARD, dtype=torch.uint8, device="cuda")
    return buf, buf[64 + shift:64 + shift + nbytes].view(dtype).view(*shape)


def out_shapes(D, B, H, W, P):
    f32 = torch.float32
    return {"code": ((D, B, H, W), torch.uint8), "res": ((D, B, H, W), f32), "masked": ((D, B, 2, H, W), f32),
            "cell": ((D, B, H // P, W // P) if P else None, f32), "stats": ((D, B, 4), torch.int32)}


def run(a, o, alpha, beta, P=0, both=1, la="packed", lo="packed", skip=(), expect=0, mutate=None, shift=0, fill=float("nan")):
    """one call; a and o are NumPy arrays (laid out here) or device views.  Returns (dict of CPU arrays of the outputs not in `skip`, the message of a refusal);
    checks the guard bytes around every output"""
    ad = a if torch.is_tensor(a) else lay_out(a, la, fill)
    od = o if torch.is_tensor(o) else lay_out(o, lo, fill)
    B, _, H, W = ad.shape
    shapes = out_shapes(2 if both else 1, B, H, W, P if P in (4, 8, 16) and H % P == 0 and W % P == 0 else 0)
    bufs = {k: guarded(*shapes[k], shift=shift) for k in OUT if k not in skip and shapes[k][0] is not None}
    if "cell" not in bufs and "cell" not in skip and P:  # (a P the call must refuse: any buffer will do)
        bufs["cell"] = guarded((64,), torch.float32)
    lib = _lib.get_lib()
    args = _lib.new_flow_consistency_args()
    _lib.fill_patch_args(args.base, geometry=(B, 1, 0, H, W, P), stream=_lib.current_stream_handle(torch.device("cuda:0")))
    args.a_dev, args.o_dev = ad.data_ptr(), od.data_ptr()
    args.a_strides[0], args.a_strides[1], args.o_strides[0], args.o_strides[1] = ad.stride(0), ad.stride(1), od.stride(0), od.stride(1)
    args.alpha, args.beta, args.both = alpha, beta, both
    for k in OUT:
        setattr(args, FIELD[k], bufs[k][1].data_ptr() if k in bufs else None)
    if mutate:
        mutate(args)
    rc = lib.cwm_flow_consistency(ctypes.byref(args))
    torch.cuda.synchronize()
    msg = lib.cwm_last_error().decode()
    assert rc == expect, (rc, msg)
    out = {}
    for k, (buf, view) in bufs.items():
        n = view.numel() * view.element_size()
        assert bool((buf[:64 + shift] == GUARD).all()) and bool((buf[64 + shift + n:] == GUARD).all()), "guard bytes around %s" % k
        if expect:
            assert bool((buf == GUARD).all()), "%s written by a refused call" % k
        out[k] = view.cpu().numpy()
    return out, msg


def equal(got, want, what=""):
    assert got, what
    for k, v in got.items():
        assert v.dtype == want[k].dtype and v.shape == want[k].shape, (k, what)
        assert np.array_equal(R.bits(v), R.bits(want[k])), (k, what, int((R.bits(v) != R.bits(want[k])).sum()))


_WANT = {}


def check(key, a, o, alpha, beta, P=0, both=1, **kw):
    """against the restatement, computed once per key and left unchanged"""
    key = (key, alpha, beta, P, both)
    if key not in _WANT:
        _WANT[key] = R.consistency(a, o, alpha, beta, P, bool(both))
    got, _ = run(a, o, alpha, beta, P, both, **kw)
    equal(got, _WANT[key], (key, kw))
    return _WANT[key]


@pytest.mark.parametrize("name", sorted(R.CASES))
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_every_shared_case(H, W, name):
    for i, B in enumerate((1, 3)):
        a, o, alpha, beta = R.CASES[name](B, H, W)
        for j, P in enumerate(P_OF[(H, W)]):
            n = H + len(name) + i + j
            check((name, H, W, B), a, o, alpha, beta, P, la=LAYOUTS[n % 4], lo=LAYOUTS[(n // 4 + i) % 4], skip=() if P else ("cell",))
        check((name, H, W, B), a, o, alpha, beta, 0, both=0, skip=("cell",))


def test_threshold_equality_is_consistent_and_the_next_beta_is_not():
    H, W = 8, 12
    w = check("thr", *R.case_threshold(1, H, W), both=0, skip=("cell",))
    assert not w["code"][0, :, :, :W - 1].any() and (w["res"][0, :, :, :W - 1] == 0.25).all() and w["stats"][0].tolist() == [[H * (W - 1), 0, H, 0]]
    w = check("thr", *R.case_threshold(1, H, W, beta=R.BETA_BELOW), both=0, skip=("cell",))
    assert (w["code"][0, :, :, :W - 1] == 1).all() and w["stats"][0].tolist() == [[0, H * (W - 1), H, 0]]
    w = check("consistent", *R.case_consistent(3, 64, 64), skip=("cell",))
    assert not w["code"][w["code"] != 2].any() and not w["res"][w["code"] != 2].any()


@pytest.mark.parametrize("H,W", [(4, 4), (24, 40), (16, 80)])
def test_targets_on_the_border_are_inside_and_one_ulp_further_is_outside(H, W):
    """o lies between guard elements (its neighbours in the layouts below): NaN, then 1e9 -- nothing beyond the plane may influence the result"""
    for ulp in (False, True):
        a, o, alpha, beta = R.case_border(2, H, W, ulp=ulp)
        for lo, fill in (("pair", float("nan")), ("offset", 1e9), ("channel", 1e9), ("offset", float("nan"))):
            w = check(("one ulp outside" if ulp else "on the border", H, W), a, o, alpha, beta, both=0, lo=lo, fill=fill, skip=("cell",))
        if ulp:
            assert (w["code"][0, :, 0, :4] == 2).all()
        else:
            assert (w["code"][0, :, :4] != 2).all()


def test_hostile_values():
    B, H, W = 3, 24, 40
    a, o, alpha, beta = R.case_hostile_a(B, H, W)
    w = check("hostile_a", a, o, alpha, beta, P=8, both=0, lo="pair")
    assert (w["code"] == 2).all() and np.isposinf(w["res"]).all() and (R.bits(w["masked"]) == 0x7fc00000).all() and (w["cell"] == 1).all()
    a, o, alpha, beta = R.case_hostile_o(B, H, W)
    w = check("hostile_o", a, o, alpha, beta, P=8, both=0, la="channel")
    hit = (w["code"] == 1) & np.isposinf(w["res"])
    assert hit.sum() > 100 and (R.bits(w["masked"][0, :, 0])[hit[0]] == 0x7fc00000).all()


def test_every_layout_of_a_and_of_o_and_outputs_off_alignment():
    a, o, alpha, beta = R.case_random(3, 24, 40, reach=4.0)
    for la in LAYOUTS:
        for lo in LAYOUTS:
            check("layouts", a, o, alpha, beta, P=8, la=la, lo=lo)
    check("layouts", a, o, alpha, beta, P=8, shift=4)  # every output four bytes past an aligned address
    check("layouts", a, o, alpha, beta, P=8, shift=1, skip=("res", "masked", "cell", "stats"))  # the codes one byte past


def test_every_output_null_in_turn():
    a, o, alpha, beta = R.case_random(2, 16, 80, reach=4.0)
    for k in OUT:
        check("optional", a, o, alpha, beta, P=16, skip=(k,))
    for k in OUT:
        check("optional", a, o, alpha, beta, P=16, skip=tuple(n for n in OUT if n != k))


def test_both_is_two_calls_with_the_roles_exchanged_and_two_calls_give_the_same_bits():
    a, o, alpha, beta = R.case_random(3, 64, 64)
    ad, od = lay_out(a, "pair"), lay_out(o, "channel")
    two, _ = run(ad, od, alpha, beta, 8, 1)
    again, _ = run(ad, od, alpha, beta, 8, 1)
    fwd, _ = run(ad, od, alpha, beta, 8, 0)
    bwd, _ = run(od, ad, alpha, beta, 8, 0)
    for k in OUT:
        assert np.array_equal(R.bits(two[k]), R.bits(again[k])), k
        assert np.array_equal(R.bits(two[k][0]), R.bits(fwd[k][0])) and np.array_equal(R.bits(two[k][1]), R.bits(bwd[k][0])), k
    equal(two, R.consistency(a, o, alpha, beta, 8, True))


def test_limits_are_refused_with_the_field_named():
    z = np.zeros((1, 2, 8, 12), np.float32)

    def refused(field, a=z, P=0, **kw):
        _, msg = run(a, a, kw.pop("alpha", 0.01), kw.pop("beta", 0.5), P, kw.pop("both", 1), expect=-1, **kw)
        assert msg.startswith("cwm_flow_consistency") and field in msg, (field, msg)

    dev = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")  # noqa: E731
    refused("base.batch = 0", mutate=lambda g: setattr(g.base, "batch", 0))
    refused("base.batch = 65536", mutate=lambda g: setattr(g.base, "batch", 65536))
    refused("base.H = 10", dev(1, 2, 10, 12))
    refused("base.W = 10", dev(1, 2, 12, 10))
    refused("base.H = 0", mutate=lambda g: setattr(g.base, "H", 0))
    refused("base.W = -4", mutate=lambda g: setattr(g.base, "W", -4))
    refused("base.H base.W", dev(1, 2, 512, 516))
    refused("a_dev", mutate=lambda g: setattr(g, "a_dev", None))
    refused("o_dev", mutate=lambda g: setattr(g, "o_dev", None))
    refused("a_strides", mutate=lambda g: g.a_strides.__setitem__(0, -192))
    refused("a_strides", mutate=lambda g: g.a_strides.__setitem__(1, -96))
    refused("o_strides", mutate=lambda g: g.o_strides.__setitem__(0, -192))
    refused("o_strides", mutate=lambda g: g.o_strides.__setitem__(1, -96))
    for bad in (-1.0, float("nan"), float("inf")):
        refused("alpha", alpha=bad)
        refused("beta", beta=bad)
    refused("both = 2", both=2)
    refused("both = -1", both=-1)
    refused("no output", skip=OUT)
    refused("base.P = 0", mutate=lambda g: setattr(g, "cell_dev", g.code_dev))
    refused("base.P = 5", P=5)
    refused("base.P = 12", P=12)
    refused("multiples of base.P", P=8)  # 8 x 12
    refused("multiples of base.P", dev(1, 2, 24, 40), P=16)
    refused("struct_size", mutate=lambda g: setattr(g, "struct_size", g.struct_size - 8))


def test_largest_case():
    """512 x 512 (2^18 pixels), both directions, P = 16: 256 tiles per direction"""
    a, o, alpha, beta = R.case_random(1, 512, 512, seed=5)
    w = check("largest", a, o, alpha, beta, P=16)
    assert all((w["code"] == k).sum() > 1000 for k in range(3)) and w["stats"].sum() == 2 * 512 * 512
