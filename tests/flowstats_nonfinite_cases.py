"""The non-finite and flat flow-sample cases of tests/test_flowstats_nonfinite_cpu.py (which holds this table against the oracle) and
tests/test_flowstats_nonfinite_gpu.py (which holds the kernels against the oracle on it): shapes, one per kernel form of csrc/flow_view.h, the poison placements,
the flat inputs, and what torch's arithmetic (oracle/flowstats_oracle.py; segmentation.py:250-276, :479-547) makes of them.

The rules, with `amin` / `amax` returning NaN for a range that holds one and `clamp(min=eps)` keeping it:
  * a NaN magnitude stays one pixel's NaN while nothing is normalised; under either normalisation its range is NaN and every pixel of the batch row is NaN;
  * an infinite magnitude (a flow of +-inf, or 3e19, whose square overflows) is an Inf pixel while nothing is normalised; under exactly one normalisation the
    range is infinite: (x - lo) / inf = 0 elsewhere and inf / inf = NaN at the pixel itself; under both, the first leaves that NaN and the second spreads it;
  * batch row 1 is never poisoned and is never touched by row 0.
Everything is poisoned in batch row 0 only.  No GPU needed to import this module."""
import ctypes

import torch

NAN, INF = float("nan"), float("inf")
BATCH = 2
CHANNELS = (2, 3)
EPS = 1e-2
OPTION_PAIRS = ((False, False), (False, True), (True, False), (True, True))  # (normalize_per_sample, normalize)

# ---- motion maps: name -> (form, layout, S, H, W).  360 pixels = 5 workgroups of 64 and one of 40 in the rows forms and the tile form's sum pass, one range tile of 256
# and one of 104 (range replica 1) at S = 24, two of 128 and one of 104 at S = 37, one and a half turns of the strided range kernel's 256 threads; 60 pixels leave most of those idle.
MOTION_SHAPES = {
    "strided 12x30": ("STRIDED", "view", 5, 12, 30),
    "strided 6x10": ("STRIDED", "view", 5, 6, 10),
    "tile256 S=24": ("TILE", "packed", 24, 12, 30),
    "tile128 S=37": ("TILE", "packed", 37, 12, 30),
    "rows16 S=64": ("ROWS16", "packed", 64, 12, 30),
    "rows32 S=128": ("ROWS32", "packed", 128, 12, 30),
    "rows64 S=256": ("ROWS64", "packed", 256, 12, 30),
    "rows64 S=512": ("ROWS64", "packed", 512, 12, 30),
}


def clean_flows(C, H, W, S, seed):
    """[BATCH, C, H, W, S] finite samples, as the other motion-map tests draw them"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(BATCH, C, H, W, S, generator=g) * 1.5


def as_layout(flows, layout):
    """the same samples in the reference's packed layout or as the sample-major view of a [(b s), C, H, W] batch (strided: the sample stride is C H W)"""
    if layout == "packed":
        return flows.contiguous()
    return flows.permute(0, 4, 1, 2, 3).contiguous().permute(0, 2, 3, 4, 1)


def partial_pixel(HW):
    """a pixel of the last, partial workgroup of every form (64-pixel workgroups; 256 / 128-pixel range tiles; the strided kernels' 256 threads)"""
    return HW - 23


def motion_poisons(C, HW, S):
    """name -> [(pixel or None = all, sample or None = all, channel, value)]: one placement per run, written into batch row 0.  Sample indices in the upper half of
    the samples where there is a choice: at S = 512 that is the second 256-sample piece of the whole-wave form."""
    last, part, mid = HW - 1, partial_pixel(HW), HW // 3
    out = {}
    for name, v in (("nan", NAN), ("+inf", INF), ("-inf", -INF)):
        out["%s first" % name] = [(0, 0, 0, v)]
        out["%s last" % name] = [(last, S - 1, C - 1, v)]
        out["%s partial workgroup" % name] = [(part, S // 2 + 1, C - 1, v)]
    out["nan whole sample"] = [(None, S - 2, 0, NAN)]
    out["nan whole pixel"] = [(mid, None, C - 1, NAN)]
    out["nan and +inf in two samples"] = [(mid, 1, 0, NAN), (part, S - 1, C - 1, INF)]
    out["+inf and -inf in one sample"] = [(mid, S // 2, 0, INF), (part, S // 2, C - 1, -INF)]
    out["3e19"] = [(7, S // 2 + 2, 0, 3e19)]
    return out


def poisoned(flows, placement):
    """a copy of `flows` [B, C, H, W, S] with `placement` written into batch row 0"""
    B, C, H, W, S = flows.shape
    out = flows.clone()
    flat = out.view(B, C, H * W, S)
    for pix, s, c, v in placement:
        flat[0, c, slice(None) if pix is None else pix, slice(None) if s is None else s] = v
    return out


def poisoned_pixels(placement, HW):
    """(pixels whose magnitude is NaN in some sample, pixels whose magnitude is infinite in some sample) as bool [HW]"""
    nan, inf = torch.zeros(HW, dtype=torch.bool), torch.zeros(HW, dtype=torch.bool)
    for pix, s, c, v in placement:
        (nan if v != v else inf)[slice(None) if pix is None else pix] = True   # (3e19: its square is inf in fp32)
    return nan, inf


def expected_pattern(placement, HW, nps, nm):
    """(isnan, isinf) of batch row 0 of the motion map, bool [HW], by the rules in the module docstring"""
    nan, inf = poisoned_pixels(placement, HW)
    none, every = torch.zeros(HW, dtype=torch.bool), torch.ones(HW, dtype=torch.bool)
    if not (nps or nm):
        return nan, inf & ~nan
    if nan.any() or (nps and nm):
        return every, none
    return inf, none


def finite_pairs(placement):
    """the option pairs for which the reference leaves every pixel but the poisoned ones finite"""
    has_nan = any(v != v for _, _, _, v in placement)
    return ((False, False),) if has_nan else ((False, True), (True, False))


# ---- flat samples (finite): the `eps` clamp, the branch that divides by eps and not by the range
def flat_flows(kind, C, H, W, S, seed):
    """"flat samples": sample 0 is all zeros (range 0) and sample S - 1 has magnitudes in [1, 1.00125] (range 0.00125 < eps: it normalises to [0, 0.125], not to
    [0, 1]); the other samples are as usual.  "all flat": every sample's magnitude is (64 + s % 16 + j) / 1024 with j in 0 .. 9 per pixel -- every per-sample range and the
    mean map's own range (<= 9 / 1024) are below eps = 0.01.  Those magnitudes are small multiples of 2^-10, so a sum of up to 512 of them is exact in fp32 in ANY order and
    what is left is the rounding of sum / S at values below 0.09 (an ulp of 7.5e-9; divided by eps: 1e-6): the 1e-5 bound judges the clamp, not a summation order."""
    g = torch.Generator().manual_seed(seed)
    HW = H * W
    if kind == "flat samples":
        fl = clean_flows(C, H, W, S, seed)
        v = fl.view(BATCH, C, HW, S)
        v[:, :, :, 0] = 0.0
        narrow = 1.0 + 0.00125 * torch.rand(BATCH, HW, generator=g)
        narrow[:, 0], narrow[:, HW - 1] = 1.0, 1.00125
        v[:, :, :, S - 1] = 0.0
        v[:, C - 1, :, S - 1] = narrow
        return fl
    assert kind == "all flat"
    j = torch.randint(0, 10, (BATCH, HW, S), generator=g)
    j[:, 0], j[:, HW - 1] = 0, 9
    mag = (64 + (torch.arange(S) % 16)[None, None, :] + j).float() / 1024.0
    fl = torch.zeros(BATCH, C, HW, S)
    fl[:, 0] = -mag   # (a magnitude is |x| exactly where one channel holds it)
    return fl.view(BATCH, C, H, W, S)


FLAT_KINDS = ("flat samples", "all flat")

# ---- the finish kernel on 4-D input: H, W -> which path of flow_map_finish_kernel
FINISH_SHAPES = {
    "registers 360": (12, 30),        # a multiple of 4, <= 65536 pixels
    "loop 63": (9, 7),                # no multiple of 4
    "loop 66048": (258, 256),         # above the 65536 pixels the registers hold
}


def finish_maps(H, W, seed):
    """name -> [BATCH, 1, H, W] maps (either sign: a 4-D input is any map); map 1 is the same clean map in every case"""
    g = torch.Generator().manual_seed(seed)
    clean = torch.randn(BATCH, 1, H, W, generator=g) * 2.0
    HW = H * W
    out = {"clean": clean}
    for name, idx, v in (("nan first", 0, NAN), ("nan last", HW - 1, NAN), ("nan between", HW // 2 + 3, NAN), ("+inf between", HW // 2 + 3, INF),
                         ("-inf between", HW // 3, -INF), ("+inf first and -inf last", None, None)):
        m = clean.clone()
        if idx is None:
            m.view(BATCH, HW)[0, 0], m.view(BATCH, HW)[0, HW - 1] = INF, -INF
        else:
            m.view(BATCH, HW)[0, idx] = v
        out[name] = m
    flat = clean.clone()
    flat.view(BATCH, HW)[0] = 0.05 + torch.randint(0, 33, (HW,), generator=g).float() / 4096.0   # range <= 32 / 4096 < eps
    out["flat"] = flat
    return out


# ---- features and covariance: name -> (H, W, downsample, S, MODE of flow_cov_kernel)
COV_SHAPES = {
    "P=264 S=5": (12, 22, 1, 5, 0),       # S no multiple of 4: scalar loads
    "P=264 S=36": (12, 22, 1, 36, 1),     # 16-byte loads with bounds: three tile rows, the last one 8 rows; a second step of 4 samples
    "P=256 S=32": (16, 16, 1, 32, 2),     # whole tiles and whole steps: no bounds path
    "P=264 S=36 ds=2": (24, 44, 2, 36, 1),
}


def cov_mode(P, S, row0=0):
    """csrc/flowstats.hip cwm_flow_cov, for the 16-byte aligned work buffer every torch allocation is"""
    return 0 if S % 4 else 2 if (P % 128 == 0 and S % 32 == 0 and row0 % 128 == 0) else 1


def cov_slabs(P):
    return ((0, 7), (P // 3, P - P // 3), (P - 1, 1))


def cov_poisons(H, W, ds, S, C=2):
    """name -> (placement as [(y, x, sample, channel, value)], poisoned positions): position 0 at the last sample, position P - 1 at sample 0 (the row and the sample
    that MODE 1's clamped loads read a second time), a position of the middle tile; at ds = 2 also +inf and -inf in ONE pooling cell, which pools to NaN"""
    Wd = W // ds
    P = (H // ds) * Wd
    mid = P // 2 + 5
    cell = lambda p: ((p // Wd) * ds, (p % Wd) * ds)
    out = {}
    for name, v in (("nan", NAN), ("+inf", INF), ("-inf", -INF)):
        out["%s position 0" % name] = ([cell(0) + (S - 1, 0, v)], [0])
        out["%s position P-1" % name] = ([cell(P - 1) + (0, C - 1, v)], [P - 1])
        out["%s middle tile" % name] = ([cell(mid) + (S // 2, 0, v)], [mid])
    if ds > 1:
        y, x = cell(mid)
        out["+inf and -inf in one cell"] = ([(y, x, 3, 0, INF), (y + 1, x + 1, 3, 0, -INF)], [mid])
    return out


def cov_poisoned(flows, placement):
    out = flows.clone()
    for y, x, s, c, v in placement:
        out[0, c, y, x, s] = v
    return out


# ---- which form an entry point takes (development library; tests/test_flow_forms_cpu.py has the whole table)
def motion_form(strides, B, C, H, W, S, address, nps=True):
    """cwm_flow_motion_sum's kernel form for flows at `address` with these strides, as a name of MOTION_SHAPES (the work buffer: a 16-byte aligned allocation)"""
    from counterfactualworldmodels_amd import _lib as L

    d = L.get_dev_lib()
    out = L.CwmDevFlowFormsOut()
    aux, hp = 0x7F4000000000, 4
    mst = (2 * hp * S, S, 1)
    L.check(d.cwm_dev_flow_forms((ctypes.c_int64 * 5)(*strides), B, C, H, W, S, address, aux, int(nps), (ctypes.c_int64 * 3)(*mst), aux - hp * mst[1], hp,
                                 ctypes.byref(out)), d)
    return {L.DEV_FLOW_REFUSED: "REFUSED", L.DEV_FLOW_MOTION_STRIDED: "STRIDED", L.DEV_FLOW_MOTION_TILE: "TILE", L.DEV_FLOW_MOTION_ROWS16: "ROWS16",
            L.DEV_FLOW_MOTION_ROWS32: "ROWS32", L.DEV_FLOW_MOTION_ROWS64: "ROWS64"}[out.motion]


def features_form(strides, B, C, H, W, S, address):
    from counterfactualworldmodels_amd import _lib as L

    d = L.get_dev_lib()
    out = L.CwmDevFlowFormsOut()
    aux, hp = 0x7F4000000000, 4
    mst = (2 * hp * S, S, 1)
    L.check(d.cwm_dev_flow_forms((ctypes.c_int64 * 5)(*strides), B, C, H, W, S, address, aux, 0, (ctypes.c_int64 * 3)(*mst), aux - hp * mst[1], hp, ctypes.byref(out)), d)
    return {L.DEV_FLOW_FEATURES_SCALAR: "SCALAR", L.DEV_FLOW_FEATURES_VEC4: "VEC4"}[out.features]


def motion_bound(S, ref):
    """the bound of test_motion_map_kernel_forms_match_oracle: an fp32 sum over S samples in whichever order the form adds them"""
    fin = ref[torch.isfinite(ref)]
    return max(1e-5, 4e-8 * S) * max(1.0, fin.abs().max().item() if fin.numel() else 0.0)
