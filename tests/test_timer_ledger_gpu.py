"""What the kernel timers book (cwm_timing_enable / cwm_timing_collect and the cwm_conj_* pair: the roofline block of the benchmark's --full run) against the
ledger of tests/timer_ledger.py: FLOPs from the CPU oracle's own count plus named terms, bytes and launch counts from the schedule -- all exact --, the
invariance of the books under tilings and lanes, and the semantics of the two hooks.  Tiny models only."""
import math
import os
import time

import numpy as np
import pytest
import torch

import timer_ledger as L
from counterfactualworldmodels_amd import _lib, config as C, conjoined_vmae as CV, synthetic as S, vmae
from oracle import vmae_oracle as O
from test_conj_oracle import TINY_CONJ, TINY_MAIN, conj_weights

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = C.VmaeConfig(name="tiny_8x8", img_size=(32, 32), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)  # tests/test_model_gpu.py
TINY16 = C.VmaeConfig(name="tiny_16x16", img_size=(64, 64), patch=16, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
CASES = {"tiny8": (TINY, 3, 4), "tiny4": (TINY_MAIN, 2, 5), "tiny16": (TINY16, 2, 3)}  # configuration, batch, visible frame-1 patches
VMAE_CLASSES = {"GEMM": _lib.KCLASS_GEMM, "ATTENTION": _lib.KCLASS_ATTENTION, "GEMM_WIDE": _lib.KCLASS_GEMM_WIDE, "GEMM_NARROW": _lib.KCLASS_GEMM_NARROW,
                "LAYERNORM": _lib.KCLASS_LAYERNORM, "PATCH_GATHER": _lib.KCLASS_PATCH_GATHER, "FILL_MASK": _lib.KCLASS_FILL_MASK, "UNEMBED": _lib.KCLASS_UNEMBED}
CONJ_CLASSES = dict(VMAE_CLASSES, CROSS_ATTN=_lib.KCLASS_CROSS_ATTN, SMALL_ATTN=_lib.KCLASS_SMALL_ATTN)
ENABLED = ("GEMM", "ATTENTION", "LAYERNORM", "PATCH_GATHER", "FILL_MASK", "UNEMBED", "CROSS_ATTN", "SMALL_ATTN")  # (wide / narrow come with the GEMM class)
DEFAULTS = {"prune_last_block": 1, "mask_token_tables": 1, "index_fused": 1, "gemm_tile": 1, "gemm_debug": 0, "min_lane_rows": 0}
ZERO = {"launches": 0, "total_ms": 0.0, "total_flops": 0.0}

_models, _oracle = {}, {}


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count & ~7  # csrc/gemm.hip gemm_cu_count


def model(name, mode):
    """one handle per (case, mode) for the whole module, back at the ledger's settings: one lane, one launch per GEMM, nothing enabled, books empty"""
    cfg = CASES[name][0]
    if (name, mode) not in _models:
        m = vmae.PretrainVisionTransformer(cfg, mode=mode)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 5).items()})
        m = m.to("cuda:0").eval()
        m.sync_weights(torch.device("cuda:0"))
        _models[(name, mode)] = m
    m = _models[(name, mode)]
    for k, v in DEFAULTS.items():
        m.set_option(k, v)
    m.set_lanes(1)
    enable(m, VMAE_CLASSES, False)
    collect(m, VMAE_CLASSES)
    return m


def inputs(name, seed=0):
    cfg, B, k_vis = CASES[name]
    x = torch.from_numpy(S.synthetic_frames(B, cfg, seed))
    mask = torch.from_numpy(S.synthetic_masks(B, cfg, k_vis, seed, 1))
    return x.cuda(), O.preprocess(x).cuda(), mask.cuda(), cfg.tokens_per_frame + k_vis


def oracle(name, n_vis):
    """the oracle's FLOP count at a rectangular mask of n_vis visible tokens per row (it depends on the shapes only): computed once per module"""
    if (name, n_vis) not in _oracle:
        cfg, B, _ = CASES[name]
        mask = torch.ones(B, cfg.num_tokens, dtype=torch.bool)
        mask[:, :n_vis] = False
        _oracle[(name, n_vis)] = L.vmae_oracle_flops(cfg, mask)
    return _oracle[(name, n_vis)]


def enable(m, classes, on=True):
    for name, k in classes.items():
        if name in ENABLED:
            m.timing_enable(k, on)


def collect(m, classes):
    """every class's books; the GEMM class first (collecting it books the wide / narrow split)"""
    return {name: m.timing_collect(k) for name, k in classes.items()}


def planes_of(mode):
    return 2 if mode == "parity" else 1


def check_books(tag, got, want):
    """launches and FLOPs / bytes of every class, exactly; prints both sides first"""
    lines = ["[books] %s" % tag] + ["    %-13s booked %5d launches %16d   expected %5d launches %16d%s" % (
        k, got[k]["launches"], int(got[k]["total_flops"]), want[k][0], want[k][1],
        "" if (got[k]["launches"], got[k]["total_flops"]) == want[k] else "   <-- differs by %+d launches, %+d" % (
            got[k]["launches"] - want[k][0], int(got[k]["total_flops"]) - want[k][1])) for k in want]
    print("\n".join(lines))
    bad = [k for k in want if (got[k]["launches"], got[k]["total_flops"]) != want[k]]
    assert not bad, "%s: the books of %s differ from the ledger\n%s" % (tag, bad, "\n".join(lines))


SETTINGS = ("defaults", "prune_last_block=0", "mask_token_tables=0", "index_fused=0", "nothing_masked", "video", "ragged")


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("mode", ["parity", "fast"])
@pytest.mark.parametrize("name", list(CASES))
def test_ledger(name, mode, setting):
    """One forward with every class enabled: FLOPs == the oracle's count + the named terms (printed), bytes and launches == the schedule."""
    cfg, B, _ = CASES[name]
    m = model(name, mode)
    x, xp, mask, n_vis = inputs(name)
    Nt = cfg.num_tokens
    opts = dict(prune_last_block=1, mask_token_tables=1, index_fused=1)
    if "=" in setting:
        key, val = setting.split("=")
        opts[key] = int(val)
        m.set_option(key, int(val))
    cap, n_min, video, run = n_vis, 0, False, None
    if setting == "nothing_masked":
        cap, mask = Nt, torch.zeros_like(mask)
    elif setting == "video":
        video = True
    elif setting == "ragged":  # row b sees 3 b more tokens than row 0 (5 with three rows: 0, 3, 5 -- unequal steps)
        for b in range(1, B):
            extra = torch.nonzero(mask[b])[: 3 * b - (b > 1), 0]
            mask[b, extra] = False
        counts = (~mask).sum(1).tolist()
        n_min, cap = min(counts), max(counts)
        assert n_min == n_vis and len(set(counts)) == B
    c = L.VmaeCall(cfg, B, cap, n_vis_min=n_min, planes=planes_of(mode), video=video, **opts)
    enable(m, VMAE_CLASSES)
    if video:
        m.predict_video(x, mask)
    elif n_min:
        m(xp, mask, ragged=True, n_vis_range=(n_min, cap))
    else:
        m(xp, mask)
    got = collect(m, VMAE_CLASSES)
    enable(m, VMAE_CLASSES, False)
    tag = "%s %s %s" % (name, mode, setting)
    rows = L.vmae_flop_ledger(c, oracle(name, cap))
    print(L.format_ledger(tag + " (GEMM | attention FLOPs)", rows, (got["GEMM"]["total_flops"], got["ATTENTION"]["total_flops"])))
    want = L.vmae_books(c, cus=cus())
    assert (rows[-1][1], rows[-1][2]) == (want["GEMM"][1], want["ATTENTION"][1])  # the ledger agrees with itself (tests/test_timer_ledger_cpu.py)
    check_books(tag, got, want)


@pytest.mark.parametrize("mode", ["parity", "fast"])
def test_two_lanes_book_the_work_of_one(mode):
    """B = 3 forced onto two lanes (2 + 1 samples): FLOPs and bytes per class are those of the one-lane call, launches those of the two half batches"""
    cfg, B, _ = CASES["tiny8"]
    m = model("tiny8", mode)
    x, xp, mask, n_vis = inputs("tiny8")
    c = L.VmaeCall(cfg, B, n_vis, planes=planes_of(mode), video=True)
    m.set_option("min_lane_rows", 1)
    m.set_lanes(2)
    enable(m, VMAE_CLASSES)
    m.predict_video(x, mask)
    got = collect(m, VMAE_CLASSES)
    enable(m, VMAE_CLASSES, False)
    one, two = L.vmae_books(c, cus=cus()), L.vmae_books(c, lanes=2, cus=cus())
    rows = L.vmae_flop_ledger(c, oracle("tiny8", n_vis))
    print(L.format_ledger("tiny8 %s two lanes (GEMM | attention FLOPs)" % mode, rows, (got["GEMM"]["total_flops"], got["ATTENTION"]["total_flops"])))
    assert all(two[k] == (2 * one[k][0], one[k][1]) for k in one)
    check_books("tiny8 %s two lanes" % mode, got, two)


@pytest.mark.parametrize("mode", ["parity", "fast"])
def test_gemm_books_do_not_depend_on_the_tiling(mode):
    """Tiling and split-K change the launches, not the work: the GEMM class's FLOPs are identical under "gemm_tile" 0, 1, 4, 6 and "gemm_debug" 32, 4, the
    launches are those of the plan (tests/gemm_plan_restatement.py), wide + narrow is the whole class (launches and FLOPs bit for bit, milliseconds up to the
    rounding of three sums of n doubles), and the split classes are empty until the GEMM class has been collected."""
    cfg, B, _ = CASES["tiny8"]
    m = model("tiny8", mode)
    x, xp, mask, n_vis = inputs("tiny8")
    c = L.VmaeCall(cfg, B, n_vis, planes=planes_of(mode))
    gemm_classes = {k: VMAE_CLASSES[k] for k in ("GEMM", "GEMM_WIDE", "GEMM_NARROW")}
    flops = L.vmae_books(c, cus=cus())["GEMM"][1]
    for tile, debug in ((0, 0), (1, 0), (4, 0), (6, 0), (0, 32), (0, 4)):
        m.set_option("gemm_tile", tile)
        m.set_option("gemm_debug", debug)
        m.timing_enable(_lib.KCLASS_GEMM, True)
        m(xp, mask)
        assert m.timing_collect(_lib.KCLASS_GEMM_WIDE) == ZERO and m.timing_collect(_lib.KCLASS_GEMM_NARROW) == ZERO
        got = collect(m, gemm_classes)
        m.timing_enable(_lib.KCLASS_GEMM, False)
        want = L.vmae_books(c, cus=cus(), gemm_tile=tile, gemm_debug=debug)
        assert want["GEMM"][1] == flops
        check_books("tiny8 %s gemm_tile=%d gemm_debug=%d" % (mode, tile, debug), got, {k: want[k] for k in gemm_classes})
        g, w, n = got["GEMM"], got["GEMM_WIDE"], got["GEMM_NARROW"]
        assert w["launches"] + n["launches"] == g["launches"] and w["total_flops"] + n["total_flops"] == g["total_flops"]
        assert abs(w["total_ms"] + n["total_ms"] - g["total_ms"]) <= 3 * g["launches"] * 2.0 ** -53 * g["total_ms"]
        if tile == 4:
            assert n["launches"] == 0 and w["launches"] == g["launches"] > 0


def test_collect_resets_disabled_classes_stay_empty_and_forwards_add_up():
    cfg, B, _ = CASES["tiny8"]
    m = model("tiny8", "parity")
    x, xp, mask, n_vis = inputs("tiny8")
    one = L.vmae_books(L.VmaeCall(cfg, B, n_vis, video=True), cus=cus())
    enable(m, VMAE_CLASSES)
    m.timing_enable(_lib.KCLASS_LAYERNORM, False)  # one class off, the others go on
    n = 3
    for _ in range(n):
        m.predict_video(x, mask)
    got = collect(m, VMAE_CLASSES)
    want = {k: ((0, 0) if k == "LAYERNORM" else (n * v[0], n * v[1])) for k, v in one.items()}
    check_books("tiny8 parity, %d forwards, LAYERNORM disabled" % n, got, want)
    assert got["LAYERNORM"] == ZERO
    again = collect(m, VMAE_CLASSES)  # collect returns AND resets
    assert all(v == ZERO for v in again.values()), again
    enable(m, VMAE_CLASSES, False)
    m.predict_video(x, mask)          # nothing enabled: nothing booked
    assert all(v == ZERO for v in collect(m, VMAE_CLASSES).values())


def test_event_pool_grows_past_its_first_512_pairs():
    """timing_enable pre-creates 512 event pairs per class; timer_begin creates more when a class launches more often between two collects: 35 tiny forwards
    are 525 GEMM launches.  Launches and FLOPs stay exact, and the next collect starts from zero."""
    cfg, B, _ = CASES["tiny8"]
    m = model("tiny8", "fast")
    x, xp, mask, n_vis = inputs("tiny8")
    one = L.vmae_books(L.VmaeCall(cfg, B, n_vis, planes=1), cus=cus())
    n = 35
    assert n * one["GEMM"][0] > 512 >= (n - 1) * one["GEMM"][0]
    enable(m, VMAE_CLASSES)
    for _ in range(n):
        m(xp, mask, check=False)
    torch.cuda.synchronize()
    got = collect(m, VMAE_CLASSES)
    check_books("tiny8 fast, %d forwards between two collects" % n, got, {k: (n * v[0], n * v[1]) for k, v in one.items()})
    assert all(math.isfinite(v["total_ms"]) and (v["total_ms"] > 0) == (v["launches"] > 0) for v in got.values())
    m(xp, mask)
    check_books("tiny8 fast, one forward after the pool grew", collect(m, VMAE_CLASSES), one)
    enable(m, VMAE_CLASSES, False)


def test_outputs_do_not_depend_on_the_timers():
    """every class enabled or none: the same tokens and video, bit for bit"""
    for mode in ("parity", "fast"):
        m = model("tiny8", mode)
        m.set_option("gemm_tile", 0)
        x, xp, mask, _ = inputs("tiny8")
        tok0, vid0 = (t.clone() for t in m.predict_video(x, mask))
        enable(m, VMAE_CLASSES)
        tok1, vid1 = (t.clone() for t in m.predict_video(x, mask))
        enable(m, VMAE_CLASSES, False)
        collect(m, VMAE_CLASSES)
        assert torch.equal(tok0, tok1) and torch.equal(vid0, vid1), mode


def timed_span(run, m, classes):
    """(sum of the classes' milliseconds, host wall milliseconds around the call and the device's synchronisation, the books)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    got = collect(m, classes)
    return sum(got[k]["total_ms"] for k in ENABLED if k in got), wall, got


def check_times(tag, run, m, classes):
    """One lane, one in-order stream: every launch is an interval of its own inside the host's span around the call, so the classes' milliseconds are finite,
    positive where something was launched, and together no more than the wall time.  (Measured before asserting: the excess is printed.)"""
    for rep in range(3):
        total, wall, got = timed_span(run, m, classes)
        print("[time] %s run %d: classes 0, 1, 4-9 together %.4f ms, host wall %.4f ms, excess %.4f ms; %s" % (
            tag, rep, total, wall, total - wall, {k: round(v["total_ms"], 4) for k, v in got.items() if v["launches"]}))
        for k, v in got.items():
            assert math.isfinite(v["total_ms"]) and (v["total_ms"] > 0) == (v["launches"] > 0), (k, v)
        assert got["GEMM"]["launches"] > 0 and total <= wall, (tag, total, wall)


def test_time_sanity_one_lane():
    m = model("tiny8", "parity")
    x, xp, mask, _ = inputs("tiny8")
    enable(m, VMAE_CLASSES)
    check_times("tiny8 parity", lambda: m.predict_video(x, mask), m, VMAE_CLASSES)
    enable(m, VMAE_CLASSES, False)


# ---- the IMU-conditioned (conjoined) handle ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def conj():
    g = np.load(os.path.join(GOLDEN, "conj_tiny.npz"))
    m = CV.ConjoinedPaddedVisionTransformer(TINY_CONJ, mode="parity")
    m.load_state_dict(conj_weights(TINY_CONJ, int(g["seed"])))
    m = m.cuda().eval()
    x, mask, imu, mc = (torch.from_numpy(g[k]) for k in ("x", "mask", "imu", "mask_context"))
    m.sync_weights(torch.device("cuda:0"))
    counts = {out: L.conj_oracle_flops(TINY_CONJ, (x.shape[0], 3, 2, 32, 32), mask, tuple(imu.shape), mc, output_context=out) for out in (False, True)}
    return m, O.preprocess(x).cuda(), mask.cuda(), imu.cuda(), mc.cuda(), counts


@pytest.mark.parametrize("ctx_out", [False, True])
@pytest.mark.parametrize("mode", ["parity", "fast"])
def test_conjoined_ledger(conj, mode, ctx_out):
    """The tiny padded model on the inputs of conj_tiny.npz (ragged visible counts, masked IMU tokens): the GEMM class against the oracle's matrix products
    + terms; attention, cross attention and context self-attention together against its batched products, and the two conjoined classes each in closed
    form; one launch per cross block, per context block and per main-stream block."""
    m, xp, mask, imu, mc, counts = conj
    m.mode = mode
    m.set_option("gemm_tile", 1)
    cfg = TINY_CONJ
    c = L.ConjCall(cfg, mask.shape[0], int((~mask).sum(1).max()), int((~mc).sum(1).max()), planes=planes_of(mode), ctx_out=ctx_out)
    enable(m, CONJ_CLASSES)
    m(xp, mask, x_context=imu, mask_context=mc, output_main=True, output_context=ctx_out)
    got = collect(m, CONJ_CLASSES)
    enable(m, CONJ_CLASSES, False)
    rows = L.conj_flop_ledger(c, counts[ctx_out])
    attn = sum(got[k]["total_flops"] for k in ("ATTENTION", "CROSS_ATTN", "SMALL_ATTN"))
    tag = "tiny conjoined %s ctx_out=%d" % (mode, ctx_out)
    print(L.format_ledger(tag + " (GEMM | attention + cross + context attention FLOPs)", rows, (got["GEMM"]["total_flops"], attn)))
    gemms = L.conj_gemms(c)
    n_blocks = cfg.main.enc_depth + cfg.main.dec_depth
    want = {"GEMM": (len(gemms), rows[-1][1]), "GEMM_WIDE": (0, 0), "GEMM_NARROW": (len(gemms), rows[-1][1]),
            "ATTENTION": (n_blocks, L.conj_main_attn_flops(c)), "CROSS_ATTN": (len(cfg.enc_cross) + len(cfg.dec_cross), L.conj_cross_attn_flops(c)),
            "SMALL_ATTN": (n_blocks, L.conj_small_attn_flops(c))}
    assert rows[-1][1] == sum(g.flops for g in gemms) and rows[-1][2] == sum(want[k][1] for k in ("ATTENTION", "CROSS_ATTN", "SMALL_ATTN"))
    check_books(tag, got, want)
    assert attn == rows[-1][2]
    assert got["PATCH_GATHER"]["launches"] == 1 and got["PATCH_GATHER"]["total_flops"] == c.B * c.vm * c.k_main * (4 + 2 * c.planes)


def test_conjoined_outputs_and_times_with_the_timers_on(conj):
    """An enabled timer moves the context stream's blocks from their side stream onto the lane's stream: same outputs, bit for bit; and on that one stream
    the classes' times are positive and together inside the host's span."""
    m, xp, mask, imu, mc, _ = conj
    m.mode = "parity"
    m.set_option("gemm_tile", 0)
    run = lambda: m(xp, mask, x_context=imu, mask_context=mc, output_main=True, output_context=True)
    y0, yc0 = (t.clone() for t in run())
    enable(m, CONJ_CLASSES)
    y1, yc1 = (t.clone() for t in run())
    collect(m, CONJ_CLASSES)
    assert torch.equal(y0, y1) and torch.equal(yc0, yc1)
    check_times("tiny conjoined parity", run, m, CONJ_CLASSES)
    enable(m, CONJ_CLASSES, False)
    y2, yc2 = run()
    assert torch.equal(y0, y2) and torch.equal(yc0, yc2)


def test_flow_input_gather_books_seven_channels():
    """the flow -> IMU head-motion model (tests/test_head_motion_gpu.py: every frame-1 token visible, only the dummy IMU token): its flow + RGB gather books
    B * visible tokens * 7 * P * P elements, read as fp32 and written as one or two bf16 planes, in one launch"""
    m = CV.imu400_8x8patch_2frames_1tube_flowbackrgb01(flow_model=S.SyntheticFlow(), mode="parity")
    cfg = m.cfg
    m.load_state_dict({k: torch.from_numpy(S.synthetic_tensor(k, shp, 0)) for k, shp in C.conj_state_dict_schema(cfg).items()}, strict=False)
    m = m.cuda().eval()
    frames = C.VmaeConfig(name="frames_224", patch=8)
    x = torch.from_numpy(S.synthetic_frames(1, frames, 0)).transpose(1, 2)
    x = ((x - torch.tensor(C.IMAGENET_MEAN).view(1, 3, 1, 1, 1)) / torch.tensor(C.IMAGENET_STD).view(1, 3, 1, 1, 1)).cuda()
    N = cfg.main.num_tokens
    assert N == 784 and cfg.main.in_chans == 7
    args = dict(x_context=torch.zeros(1, 6, 400, device="cuda"), mask_context=torch.ones(1, 25, dtype=torch.bool, device="cuda"), output_main=False, output_context=True)
    mask = torch.zeros(1, 2 * N, dtype=torch.bool, device="cuda")
    flows = m.compute_flows(x)
    m(x, mask, flows=flows, **args)  # (creates the handle)
    for mode in ("parity", "fast"):
        m.mode = mode
        m.timing_enable(_lib.KCLASS_PATCH_GATHER, True)
        m(x, mask, flows=flows, **args)
        got = m.timing_collect(_lib.KCLASS_PATCH_GATHER)
        m.timing_enable(_lib.KCLASS_PATCH_GATHER, False)
        want = 1 * N * 7 * 8 * 8 * (4 + 2 * planes_of(mode))
        print("[books] flow-input gather %s: booked %d launches %d bytes, expected 1 launch %d bytes" % (mode, got["launches"], int(got["total_flops"]), want))
        assert (got["launches"], got["total_flops"]) == (1, want)
