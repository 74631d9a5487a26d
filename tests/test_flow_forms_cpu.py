"""Which kernel form the five flow-sample entry points launch (csrc/flow_view.h), read out through the development library's `cwm_dev_flow_forms`, against
the forms written out here.  The expected values come from the predicates as `cwm_flow_features`, `cwm_flow_motion_sum`, `cwm_flow_filter_stats`,
`cwm_flow_filter_apply` and `cwm_flow_filter_pack` stated them before there was one classification: `entry_point_rules` restates those, statement for statement,
and the named cases below are worked out by hand from them.  The GPU tests compare values per layout and cannot see a launch that took a slower form.
No GPU needed: a form is host arithmetic."""
import ctypes

import pytest

from counterfactualworldmodels_amd import _lib as L

BASE, AUX = 0x7F0000000000, 0x7F4000000000  # 16-byte aligned "device addresses"
REF = L.DEV_FLOW_REFUSED
SCALAR, VEC4 = L.DEV_FLOW_FEATURES_SCALAR, L.DEV_FLOW_FEATURES_VEC4
STRIDED, TILE, ROWS16, ROWS32, ROWS64 = (L.DEV_FLOW_MOTION_STRIDED, L.DEV_FLOW_MOTION_TILE, L.DEV_FLOW_MOTION_ROWS16, L.DEV_FLOW_MOTION_ROWS32,
                                         L.DEV_FLOW_MOTION_ROWS64)
PLANES, PLANES_VEC, PACKED, PACKED_VEC = L.DEV_FLOW_COUNT_PLANES, L.DEV_FLOW_COUNT_PLANES_VEC, L.DEV_FLOW_COUNT_PACKED, L.DEV_FLOW_COUNT_PACKED_VEC
V1, V4 = L.DEV_FLOW_FINISH_V1, L.DEV_FLOW_FINISH_V4
Z_PLANES, Z_PLANES_VEC, Z_SCATTER = L.DEV_FLOW_ZERO_PLANES, L.DEV_FLOW_ZERO_PLANES_VEC, L.DEV_FLOW_ZERO_SCATTER
PACK = L.DEV_FLOW_PACK_TRANSPOSE
HP = 4  # patches per frame of the masks below (a 2 x 2 grid)


def flows(layout, S, H=16, W=16, B=2, C=2, base=BASE, sb_pad=0, sc_pad=0):
    """(strides, B, C, H, W, S, address) of [B, C, H, W, S] flow samples: "packed" (`.contiguous()`), "view" (the sample-outermost view of a [(b s), 1, C, H, W]
    batch), "strided" (a W + 6 wide sample-outermost buffer cut to W columns from column 3, as tests/test_motion_sampling_gpu.py layouts)"""
    if layout == "packed":
        sc = H * W * S + sc_pad
        st = (C * sc + sb_pad, sc, W * S, S, 1)
    else:
        Wb = W + 6 if layout == "strided" else W
        sc = H * Wb + sc_pad
        st = (S * C * sc + sb_pad, sc, Wb, 1, C * sc)
        base += 12 if layout == "strided" else 0
    return st, B, C, H, W, S, base


def entry_point_rules(st, B, C, H, W, S, f, aux, nps, mst, mask):
    """the five entry points' own predicates, as they stood"""
    sb, sc, sh, sw, ss = st
    a16 = lambda p: p & 15 == 0
    if not (f and B > 0 and C > 0 and H > 0 and W > 0 and S > 0):
        return (REF,) * 6
    # cwm_flow_features
    features = VEC4 if (ss == 1 and S % 4 == 0 and a16(f) and a16(aux) and sb % 4 == 0 and sc % 4 == 0 and sh % 4 == 0 and sw % 4 == 0) else SCALAR
    # cwm_flow_motion_sum
    tile_mm, tile_sum = (256 if S <= 32 else 128 if S <= 64 else 64), 64
    smem_mm, smem_sum = tile_mm * (S + 1) * 4, (tile_sum * (S + 1) + 2 * S) * 4
    packed = ss == 1 and sw == S and sh == W * S
    q = 16 if S == 64 else 32 if S == 128 else (64 if S % 256 == 0 else 0)
    rows_form = packed and q and sb % 4 == 0 and sc % 4 == 0 and a16(f) and (not nps or a16(aux))
    tile_form = not rows_form and packed and smem_mm <= 150 * 1024 and smem_sum <= 150 * 1024
    motion = REF if nps and not aux else {16: ROWS16, 32: ROWS32, 64: ROWS64}[q] if rows_form else TILE if tile_form else STRIDED
    # check_flows (the filter's three entry points)
    if not (C == 2 and H == W and H * W <= 1 << 30 and S <= 65535 and B <= 65535):
        return features, motion, REF, REF, REF, REF
    # cwm_flow_filter_stats
    HW = H * W
    base4 = a16(f) and sb % 4 == 0 and sc % 4 == 0
    packed = ss == 1 and sw == S and sh == W * S and S <= 8192
    if packed:
        count = PACKED_VEC if base4 and S % 4 == 0 else PACKED
    else:
        count = PLANES_VEC if sw == 1 and sh == W and HW % 4 == 0 and base4 and ss % 4 == 0 else PLANES
    ab, ap, as_ = mst
    finish = V4 if as_ == 1 and S % 4 == 0 and ab % 4 == 0 and ap % 4 == 0 and (mask + HP * ap) & 3 == 0 else V1  # active_dev + h h ap
    # cwm_flow_filter_apply
    if sw == 1 and sh == W:
        zero = Z_PLANES_VEC if HW % 4 == 0 and a16(f) and sb % 4 == 0 and sc % 4 == 0 and ss % 4 == 0 else Z_PLANES
    else:
        zero = Z_SCATTER if S <= 8192 else REF
    # cwm_flow_filter_pack
    pack = PACK if sw == 1 and sh == W and sc == H * W else REF
    return features, motion, count, finish, zero, pack


def library_forms(st, B, C, H, W, S, f, aux=AUX, nps=0, mst=None):
    d = L.get_dev_lib()
    out = L.CwmDevFlowFormsOut()
    mst = mst or (2 * HP * S, S, 1)  # a contiguous [B, Np = 2 HP, S] mask ...
    mask = aux - HP * mst[1]         # ... placed so that its frame-2 half begins at `aux`: one address decides the alignment of all three
    L.check(d.cwm_dev_flow_forms((ctypes.c_int64 * 5)(*st), B, C, H, W, S, f, aux, nps, (ctypes.c_int64 * 3)(*mst), mask, HP, ctypes.byref(out)), d)
    got = (out.features, out.motion, out.count, out.finish, out.zero, out.pack)
    assert got == entry_point_rules(st, B, C, H, W, S, f, aux, nps, mst, mask), "the restated entry points disagree"
    return got


# name -> (arguments of library_forms, (features, motion, count, finish, zero, pack)), by hand from the entry points' predicates
CASES = {
    # the counterfactual batch: every 16-byte form
    "packed S=256": ((flows("packed", 256),), (VEC4, ROWS64, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=512": ((flows("packed", 512),), (VEC4, ROWS64, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=64": ((flows("packed", 64),), (VEC4, ROWS16, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=128": ((flows("packed", 128),), (VEC4, ROWS32, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=24": ((flows("packed", 24),), (VEC4, TILE, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=100": ((flows("packed", 100),), (VEC4, TILE, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=37": ((flows("packed", 37),), (SCALAR, TILE, PACKED, V1, Z_SCATTER, REF)),
    # (64 x 701 + 1400) x 4 = 185 056 bytes of LDS > 150 KB
    "packed S=700": ((flows("packed", 700),), (VEC4, STRIDED, PACKED_VEC, V4, Z_SCATTER, REF)),
    # one sample: the packed tensor is also the sample-outermost view (sw = S = 1, sh = W, sc = H W); the motion map's tile (S is no rows size), the filter's packed form first
    # (the sample stride 1 is no multiple of 4: the planes are zeroed with 4-byte stores)
    "packed S=1": ((flows("packed", 1),), (SCALAR, TILE, PACKED, V1, Z_PLANES, PACK)),
    "packed S=1 9x9": ((flows("packed", 1, 9, 9),), (SCALAR, TILE, PACKED, V1, Z_PLANES, PACK)),
    # the motion map's LDS boundary: (64 (S + 1) + 2 S) x 4 <= 153 600  <=>  66 S <= 38 336  <=>  S <= 580
    "packed S=580": ((flows("packed", 580),), (VEC4, TILE, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=581": ((flows("packed", 581),), (SCALAR, STRIDED, PACKED, V1, Z_SCATTER, REF)),
    # the filter's sample limit (2 S counters / S list entries in LDS); 8192 = 32 x 256 is a rows size
    "packed S=8192": ((flows("packed", 8192, 4, 4),), (VEC4, ROWS64, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=8193": ((flows("packed", 8193, 4, 4),), (SCALAR, STRIDED, PLANES, V1, REF, REF)),
    # pixel counts: 81 is no multiple of 4 -- nothing of the packed forms depends on it (S is the vector axis)
    "packed S=24 9x9": ((flows("packed", 24, 9, 9),), (VEC4, TILE, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=256 9x9": ((flows("packed", 256, 9, 9),), (VEC4, ROWS64, PACKED_VEC, V4, Z_SCATTER, REF)),
    # the sample-outermost view: vectors along the pixels, where H W is a multiple of 4
    "view S=24": ((flows("view", 24),), (SCALAR, STRIDED, PLANES_VEC, V4, Z_PLANES_VEC, PACK)),
    "view S=256": ((flows("view", 256),), (SCALAR, STRIDED, PLANES_VEC, V4, Z_PLANES_VEC, PACK)),
    "view S=37": ((flows("view", 37),), (SCALAR, STRIDED, PLANES_VEC, V1, Z_PLANES_VEC, PACK)),
    "view S=24 9x9": ((flows("view", 24, 9, 9),), (SCALAR, STRIDED, PLANES, V4, Z_PLANES, PACK)),
    "view S=8193": ((flows("view", 8193, 4, 4),), (SCALAR, STRIDED, PLANES_VEC, V1, Z_PLANES_VEC, PACK)),
    # a cut of a wider buffer: rows are not adjacent (sh = W + 6), the base is 12 bytes past an aligned address
    "strided S=24": ((flows("strided", 24),), (SCALAR, STRIDED, PLANES, V4, Z_SCATTER, REF)),
    "strided S=256 9x9": ((flows("strided", 256, 9, 9),), (SCALAR, STRIDED, PLANES, V4, Z_SCATTER, REF)),
    # misalignment: a base address 4 bytes off
    "packed S=256 base+4": ((flows("packed", 256, base=BASE + 4),), (SCALAR, TILE, PACKED, V4, Z_SCATTER, REF)),
    "packed S=24 base+4": ((flows("packed", 24, base=BASE + 4),), (SCALAR, TILE, PACKED, V4, Z_SCATTER, REF)),
    "view S=24 base+4": ((flows("view", 24, base=BASE + 4),), (SCALAR, STRIDED, PLANES, V4, Z_PLANES, PACK)),
    # ... a batch or channel stride that is no multiple of 4 (a padded allocation; H, W, S strides still packed / planes)
    "packed S=256 sb+2": ((flows("packed", 256, sb_pad=2),), (SCALAR, TILE, PACKED, V4, Z_SCATTER, REF)),
    "packed S=256 sc+2": ((flows("packed", 256, sc_pad=2),), (SCALAR, TILE, PACKED, V4, Z_SCATTER, REF)),
    "view S=24 sb+2": ((flows("view", 24, sb_pad=2),), (SCALAR, STRIDED, PLANES, V4, Z_PLANES, PACK)),
    # (the sample stride of the view is C sc: sc + 2 keeps it a multiple of 4 only by C = 2 -> 2 sc + 4 ... sc = 258: ss = 516; sc itself is not)
    "view S=24 sc+2": ((flows("view", 24, sc_pad=2),), (SCALAR, STRIDED, PLANES, V4, Z_PLANES, REF)),
    # ... the other address: the features' output, the motion map's work buffer (read only with per-sample normalisation), the mask (4-byte loads)
    "packed S=256 aux+4": ((flows("packed", 256), AUX + 4), (SCALAR, ROWS64, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=256 aux+4 nps": ((flows("packed", 256), AUX + 4, 1), (SCALAR, TILE, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=256 nps": ((flows("packed", 256), AUX, 1), (VEC4, ROWS64, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=64 aux+4 nps": ((flows("packed", 64), AUX + 4, 1), (SCALAR, TILE, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=24 aux+4 nps": ((flows("packed", 24), AUX + 4, 1), (SCALAR, TILE, PACKED_VEC, V4, Z_SCATTER, REF)),
    "packed S=256 aux+1": ((flows("packed", 256), AUX + 1), (SCALAR, ROWS64, PACKED_VEC, V1, Z_SCATTER, REF)),
    "packed S=256 no work buffer nps": ((flows("packed", 256), 0, 1), (VEC4, REF, PACKED_VEC, V4, Z_SCATTER, REF)),
    "view S=24 no work buffer nps": ((flows("view", 24), 0, 1), (SCALAR, REF, PLANES_VEC, V4, Z_PLANES_VEC, PACK)),
    # ... the mask's strides: a [B, S, Np] mask seen as [B, Np, S]; rows of 6 bytes
    "packed S=256 mask transposed": ((flows("packed", 256), AUX, 0, (8 * 256, 1, 8)), (VEC4, ROWS64, PACKED_VEC, V1, Z_SCATTER, REF)),
    "packed S=24 mask rows of 26": ((flows("packed", 24), AUX, 0, (8 * 26, 26, 1)), (VEC4, TILE, PACKED_VEC, V1, Z_SCATTER, REF)),
    # three channels: the statistics take them, the filter does not; nor a frame that is not square
    "packed S=256 C=3": ((flows("packed", 256, C=3),), (VEC4, ROWS64, REF, REF, REF, REF)),
    "packed S=24 16x24": ((flows("packed", 24, 16, 24),), (VEC4, TILE, REF, REF, REF, REF)),
    "no flows": ((flows("packed", 24, base=0),), (REF,) * 6),
    "S=0": ((flows("packed", 0),), (REF,) * 6),
}


@pytest.mark.parametrize("name", list(CASES))
def test_entry_points_choose_the_forms_they_chose(name):
    (fl, *rest), want = CASES[name]
    assert library_forms(*fl, *rest) == want


def test_sweep_of_layouts_and_sample_counts():
    """every layout x sample count x pixel count x alignment of the issue's table, against the restated entry points (library_forms asserts it), and the
    sweep reaches every form"""
    seen = [set() for _ in range(6)]
    n = 0
    for layout in ("packed", "view", "strided"):
        for S in (1, 24, 37, 64, 100, 128, 256, 512, 580, 581, 700, 8192, 8193):
            for hw in (9, 16) if S < 8192 else (4,):
                for kw in ({}, {"base": BASE + 4}, {"sb_pad": 2}, {"sc_pad": 2}, {"C": 3}):
                    for aux, nps in ((AUX, 0), (AUX, 1), (AUX + 4, 0), (AUX + 4, 1), (AUX + 1, 0), (0, 1)):
                        got = library_forms(*flows(layout, S, hw, hw, **kw), aux, nps)
                        n += 1
                        for k, v in enumerate(got):
                            seen[k].add(v)
    assert n == 3 * (11 * 2 + 2) * 5 * 6
    assert seen == [{SCALAR, VEC4}, {REF, STRIDED, TILE, ROWS16, ROWS32, ROWS64}, {REF, PLANES, PLANES_VEC, PACKED, PACKED_VEC}, {REF, V1, V4},
                    {REF, Z_PLANES, Z_PLANES_VEC, Z_SCATTER}, {REF, PACK}]


def test_argument_refusals_name_the_entry_point():
    """CWM_ERR_INVALID from the shared argument checks, with the entry point's name.  No device: every call here is invalid TWICE -- the check under test and, behind
    it, a null pointer the entry point refuses next --, so that a regression of the first shows as a wrong message and never as a launch on these invented addresses.
    (The refusals that come from the layout need real buffers behind them: tests/test_flowstats_gpu.py.)"""
    lib = L.get_lib()
    st, B, C, H, W, S, f = flows("packed", 24, 4, 4)
    strides = (ctypes.c_int64 * 5)(*st)
    assert lib.cwm_flow_features(None, strides, B, C, H, W, S, 1, None, None) == -1 and b"cwm_flow_features: null pointer" in lib.cwm_last_error()
    assert lib.cwm_flow_features(f, strides, B, C, H, W, 0, 1, None, None) == -1 and b"cwm_flow_features: B=2, C=2, H=4, W=4, S=0 must be" in lib.cwm_last_error()
    assert lib.cwm_flow_motion_sum(f, strides, 0, C, H, W, S, 0, 0.01, None, None, None) == -1 and b"cwm_flow_motion_sum: B=0" in lib.cwm_last_error()
    assert lib.cwm_flow_filter_apply(f, strides, B, 3, H, W, S, None, None) == -1 and b"cwm_flow_filter_apply: flow samples have C=2" in lib.cwm_last_error()
    assert lib.cwm_flow_filter_pack(f, strides, B, C, H, 5, S, None, None, None) == -1 and b"cwm_flow_filter_pack: H=4 != W=5" in lib.cwm_last_error()
    assert (lib.cwm_flow_filter_stats(f, strides, 70000, C, H, W, S, None, None, 8, 0, 1.0, 1.0, 1.0, None, None, None, None, None) == -1
            and b"cwm_flow_filter_stats: H W=16, S=24 or B=70000 beyond the launch grid" in lib.cwm_last_error())
