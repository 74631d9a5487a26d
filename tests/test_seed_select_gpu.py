"""`cwm_seed_select` on a real MI355X through the C ABI against the NumPy restatement of its definition (tests/seed_select_restatement.py), every output by
equality (the floats bit for bit): the restatement's list of cases -- grids from 3 x 3 cells to the 4096-cell limit, three rows of different content, radius
0 / 1 / 3 / 64, dead slots, constant maps and signed zeros, NaN pixels / cells / rows, free and prior cells, both thresholds, race mode, the cells form --
maps read in place from a channel slice and from padded buffers (16-byte aligned and not), outputs pre-filled with sentinels, NULL outputs, repeats, the
refusals, and the package's own wrapper.  Every call of this file shares one workspace pre-filled with 0xA5, which the call has to initialise itself."""
import ctypes

import numpy as np
import pytest
import torch

import seed_select_restatement as R
from counterfactualworldmodels_amd import _lib, seed_select as SS

pytestmark = pytest.mark.gpu
CASES = R.cases()
OUT = ("seeds", "cells", "values", "pooled", "peaks", "stats")
_WORK = []


def workspace():
    """one workspace for the largest geometry of the file, refilled with 0xA5 before every call"""
    if not _WORK:
        _WORK.append(torch.empty((int(_lib.get_lib().cwm_seed_select_work_bytes(3, 256, 256, 4)),), dtype=torch.uint8, device="cuda"))  # 3 rows of 4096 cells
    _WORK[0].fill_(0xA5)
    return _WORK[0]


def placed(m, layout):
    """the map [B,H,W] on the device as a view of the layout's storage"""
    m = torch.from_numpy(m).cuda()
    B, H, W = m.shape
    if layout == "plain":
        return m
    if layout == "channel":
        buf = torch.rand((B, 3, H, W), device="cuda")
        buf[:, 1] = m
        return buf[:, 1]
    pad, shift = {"padded": (8, 0), "unaligned": (6, 1)}[layout]  # a row stride of W + 8; one of W + 6 from an address that is no multiple of 16 bytes
    buf = torch.rand((B * H * (W + pad) + shift,), device="cuda")
    view = buf[shift:].reshape(B, H, W + pad)[:, :, :W]
    view.copy_(m)
    return view


def run(kw, layout="plain", skip=(), expect=0, mutate=None):
    """one call; every output pre-filled with a sentinel.  Returns ({name: numpy array}, message)"""
    kw = dict(kw)
    m, P, K, cells = kw.pop("map"), kw.pop("P"), kw.pop("K"), kw.pop("cells", False)
    view = m if torch.is_tensor(m) else placed(np.ascontiguousarray(m), "plain" if cells else layout)
    B = view.shape[0]
    H, W = (view.shape[1] * P, view.shape[2] * P) if cells else view.shape[1:]
    n = (H // P) * (W // P) if P else 0
    dev = lambda name, dtype: None if kw.get(name) is None else torch.from_numpy(np.ascontiguousarray(kw[name], dtype)).cuda()  # noqa: E731
    free, e, prior = dev("free", np.uint8), dev("e", np.float32), dev("prior", np.int32)
    full = lambda shape, v, dtype: torch.full(shape, v, dtype=dtype, device="cuda")  # noqa: E731
    out = dict(seeds=full((B, K, 2), -9, torch.int32), cells=full((B, K), -9, torch.int32), values=full((B, K), -7.0, torch.float32),
               pooled=full((B, n), -7.0, torch.float32), peaks=full((B, n), 99, torch.uint8), stats=full((B, 4), -9, torch.int32))
    sentinel = {k: v.clone() for k, v in out.items()}
    work = workspace()
    a = _lib.new_seed_select_args()
    _lib.fill_patch_args(a.base, geometry=(B, 1, 0, H, W, P), stream=_lib.current_stream_handle(view.device))
    a.map_dev, a.cells = view.data_ptr(), int(cells)
    if not cells:
        a.map_strides[0], a.map_strides[1] = view.stride(0), view.stride(1)
    a.free_dev, a.e_dev, a.prior_dev, a.n_prior = _lib.ptr(free), _lib.ptr(e), _lib.ptr(prior), 0 if prior is None else prior.shape[1]
    a.K, a.radius, a.peaks_only = K, kw.get("radius", 1), int(kw.get("peaks_only", False))
    a.abs_thresh, a.rel_thresh = kw.get("abs_thresh", -np.inf), kw.get("rel_thresh", 0.0)
    a.work_dev, a.work_bytes = work.data_ptr(), work.numel()
    for k in OUT:
        setattr(a, k + "_dev", None if k in skip else out[k].data_ptr())
    if mutate:
        mutate(a)
    rc = _lib.get_lib().cwm_seed_select(ctypes.byref(a))
    torch.cuda.synchronize()
    msg = _lib.get_lib().cwm_last_error().decode()
    assert rc == expect, (rc, msg)
    for k in skip if rc == 0 else OUT:
        assert torch.equal(out[k], sentinel[k]), "output %s was not asked for and has been written" % k
    return {k: v.cpu().numpy() for k, v in out.items()}, msg


def check(name, kw, layout="plain", skip=()):
    got, _ = run(kw, layout, skip)
    want = R.want(name, kw)
    R.assert_equal({k: (want[k] if k in skip else got[k]) for k in OUT}, want, (name, layout))  # (every element equal: no sentinel is left in an output asked for)
    return got


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_case_equals_the_restatement(name, kw):
    check(name, kw)


@pytest.mark.parametrize("layout", ["channel", "padded", "unaligned"])
def test_maps_are_read_in_place(layout):
    for name in ("grid_5x7_P4", "grid_28x28_P8", "grid_14x14_P16", "nan"):
        check(name, dict(CASES)[name], layout)


def test_every_optional_output_null_in_turn_and_alone():
    name = "race_peaks"
    kw = dict(CASES)[name]
    for k in OUT:
        check(name, kw, skip=(k,))
        check(name, kw, skip=tuple(o for o in OUT if o != k))


def test_two_calls_give_the_same_bits():
    for name in ("grid_64x64_P4", "race", "nan_peaks_race"):
        a, _ = run(dict(CASES)[name])
        b, _ = run(dict(CASES)[name])
        assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in OUT), name


def test_the_wrapper_and_the_torch_composition_on_the_device():
    for name in ("grid_28x28_P8", "prior", "cells_race", "dead_slots_peaks"):
        kw = dict(dict(CASES)[name])
        m, P, K = torch.from_numpy(kw.pop("map")).cuda(), kw.pop("P"), kw.pop("K")
        rest = {k: (torch.from_numpy(np.asarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        want = R.want(name, dict(CASES)[name])
        for fn in (SS.select_seeds, SS.select_seeds_torch):
            sel = fn(m, K, P, **rest)
            assert sel.seeds.is_cuda and sel.peaks.dtype == torch.bool
            R.assert_equal({k: getattr(sel, k).cpu().numpy() for k in OUT}, want, (name, fn.__name__))
    chan = torch.rand((2, 3, 32, 48), device="cuda")
    assert torch.equal(SS.select_seeds(chan[:, 1], 5, 8).seeds, SS.select_seeds(chan[:, 1].contiguous(), 5, 8).seeds)


def test_limits_are_refused_with_the_field_named():
    lib = _lib.get_lib()
    ok = dict(map=np.zeros((1, 8, 12), np.float32), P=4, K=2)

    def refused(field, kw=ok, **more):
        _, msg = run(kw, expect=-1, **more)
        assert msg.startswith("cwm_seed_select") and field in msg, (field, msg)

    refused("K = 0", mutate=lambda a: setattr(a, "K", 0))
    refused("K = 65", mutate=lambda a: setattr(a, "K", 65))
    refused("radius = -1", mutate=lambda a: setattr(a, "radius", -1))
    refused("radius = 65", mutate=lambda a: setattr(a, "radius", 65))
    refused("n_prior = 65", mutate=lambda a: setattr(a, "n_prior", 65))
    refused("prior_dev", mutate=lambda a: setattr(a, "n_prior", 3))
    refused("peaks_only = 2", mutate=lambda a: setattr(a, "peaks_only", 2))
    refused("cells = 2", mutate=lambda a: setattr(a, "cells", 2))
    refused("abs_thresh", mutate=lambda a: setattr(a, "abs_thresh", float("nan")))
    refused("rel_thresh", mutate=lambda a: setattr(a, "rel_thresh", float("inf")))
    refused("base.P = 5", dict(map=torch.zeros((1, 10, 10), device="cuda"), P=5, K=2))
    refused("base.H = 10", dict(map=torch.zeros((1, 10, 12), device="cuda"), P=4, K=2))
    refused("base.H base.W", dict(map=torch.zeros((1, 512, 516), device="cuda"), P=4, K=2))
    refused("patches", dict(map=torch.zeros((1, 512, 512), device="cuda"), P=4, K=2))
    refused("map_dev", mutate=lambda a: setattr(a, "map_dev", None))
    refused("map_strides", mutate=lambda a: a.map_strides.__setitem__(1, 8))
    refused("map_strides", mutate=lambda a: a.map_strides.__setitem__(0, -96))
    refused("work_dev", mutate=lambda a: setattr(a, "work_dev", None))
    refused("work_dev", mutate=lambda a: setattr(a, "work_dev", a.work_dev + 8))
    refused("work_bytes", mutate=lambda a: setattr(a, "work_bytes", 16))
    refused("struct_size", mutate=lambda a: setattr(a, "struct_size", a.struct_size - 8))
    refused("no output", skip=OUT)
    assert lib.cwm_seed_select_work_bytes(1, 8, 12, 4) == 32 + 16  # 6 cells: floats and offset bytes, each rounded up to 16
    for B, H, W, P in ((0, 8, 12, 4), (1, 0, 12, 4), (1, 8, -4, 4), (1, 10, 12, 4), (1, 8, 12, 5), (1, 512, 516, 4), (1, 512, 512, 4), (70000, 8, 12, 4)):
        assert lib.cwm_seed_select_work_bytes(B, H, W, P) == 0, (B, H, W, P)
