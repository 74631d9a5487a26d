"""bench.py -- predicted frames/s of the VMAE predictor path on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps 20 --warmup 3           # the headline alone: set up, warm up, time the steps, print the line
    python bench.py --gpus 1 --steps 20 --warmup 3 --full    # + every check and side measurement (roofline, secondary mode, prompts256, CPU baseline)
    python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR   # + the last timed step's outputs as DIR/<name>.npy
    python bench.py --workload prompts256 --gpus N          # BASELINE configs[3] alone: 256 prompts on one frame pair, sharded over N ranks
    python bench.py --workload flowstats | prompt_build      # the kernels after / before the predictor path (one GPU)
                                                            # (prompts256: strong scaling; with --full, per_rank_ms = every rank's {build, broadcast, own_prompts, predict, gather})
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A step = one call of the wrapper's `predict` (reference: prediction.py:406-454) on one batch of synthetic frame pairs
already resident in HBM: raw [B,2,3,224,224] frames + masks -> mask rectangulariser (host read-back of the row counts, as
the reference does for every B > 1), normalise, tubelet patch embed + mask gather, ViT encoder over visible tokens, ViT
decoder over the full token set, pixel head, patch un-embed -> predicted frames.
N=1 workload = BASELINE.json configs[1]: ViT-B/8, batch 32.  With N>1 every rank runs the same
per-GPU batch on its own shard of frame pairs (independent units, no data-path collective): weak
scaling, value = all ranks' frame pairs / max-over-ranks time.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from counterfactualworldmodels_amd import _lib, config as C, synthetic as S, vmae  # noqa: E402  (loading the library makes no HIP call)

PEAK_BF16_TFLOPS = 2500.0  # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0      # HBM3E (same guide)
# (index_gather_kernel: round 5 -- mask -> permutation, its inverse, the row check AND the patch gather in one launch; rounds 1-4 booked the gather alone here)
EDGE_CLASSES = (("layernorm_kernel", _lib.KCLASS_LAYERNORM), ("index_gather_kernel", _lib.KCLASS_PATCH_GATHER),
                ("fill_mask_tokens_kernel", _lib.KCLASS_FILL_MASK), ("unembed_kernel", _lib.KCLASS_UNEMBED))

# BASELINE configs[3]: 256 motion-counterfactual prompts over ONE frame pair, sharded over the ranks
# (rank 0 broadcasts frame + prompt table, every rank builds + predicts its slice, all-gather).
PROMPTS = dict(cfg="base_8x8patch_2frames_1tube", total=256, chunk=32,
               name="ViT-base VMAE 8x8, 256 motion-counterfactual prompts on one frame pair (BASELINE configs[3])")

WORKLOADS = {
    "base8": dict(cfg="base_8x8patch_2frames_1tube", batch=32, k_vis=8, clump=1,
                  name="ViT-base VMAE 8x8, batch=32 synthetic frame pairs (BASELINE configs[1])"),
    "large4": dict(cfg="large_4x4patch_2frames_1tube", batch=8, k_vis=32, clump=2,
                   name="ViT-large VMAE 4x4, batch=8 (BASELINE configs[2])"),
}


def build_info():
    """Which library this line was measured with: version, source hash, the hipcc that compiled it, and whether that compiler is the one the
    ISA lint of the hand-counted waits last passed on (csrc/LINT_PASSED.json; tools/asm_lds_lint.py --record)."""
    from counterfactualworldmodels_amd import build

    lib = _lib.get_lib()
    comp = lib.cwm_compiler_version().decode()
    return {"library": lib.cwm_version().decode(), "source_hash": lib.cwm_source_hash().decode(), "compiler": comp,
            "lint_passed_on_this_compiler": build.lint_record().get("hipcc") == comp}


def timed_steps(G, x, mask, n_vis, steps, distributed):
    """K steps of the reference's `predict` (prediction.py:406-454) on the wrapper `G`: mask rectangulariser (its one host
    read-back per call included), normalise, forward, un-embed; all frames returned.  Returns (seconds, the last step's frames)."""
    if distributed:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = None
    for _ in range(steps):
        y = None  # (the previous step's frames are released first: every step reuses one allocation, as when nothing is kept)
        y = G.predict(x, mask, frame=None)
    torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    dt = time.perf_counter() - t0
    if distributed:
        t = torch.tensor([dt], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt, y


DUMP_BUDGET_BYTES = 60 * 10**6  # --dump-outputs: the arrays written (their .npy headers aside) stay under 64 MB in all


def dump_outputs(out_dir, arrays):
    """`--dump-outputs DIR`: what the timed path returned in its last step, one DIR/<name>.npy per array (float32; float64 stays float64; masks as
    0.0 / 1.0).  When they exceed DUMP_BUDGET_BYTES together, the arrays above an equal share of it are viewed as rows of their last axis and keep a
    fixed, seeded subset of those rows in ascending order (the same subset in every run and every build of the same command); the others are whole."""
    import numpy as np

    if out_dir is None or not arrays:
        return
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: (v.detach() if v.dtype == torch.float64 else v.detach().float()) for k, v in arrays.items()}
    nbytes = {k: v.numel() * v.element_size() for k, v in arrays.items()}
    share = DUMP_BUDGET_BYTES / len(arrays)
    small = sum(b for b in nbytes.values() if b <= share)
    large = sum(b for b in nbytes.values() if b > share)
    frac = (DUMP_BUDGET_BYTES - small) / large if sum(nbytes.values()) > DUMP_BUDGET_BYTES else 1.0
    written, sampled = 0, []
    for name, v in arrays.items():
        if frac < 1.0 and nbytes[name] > share:
            v = v.reshape(-1, v.shape[-1])
            rows = torch.randperm(v.shape[0], generator=torch.Generator().manual_seed(0))[:max(1, int(v.shape[0] * frac))].sort().values
            v = v.index_select(0, rows.to(v.device))
            sampled.append(name)
        a = v.cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written += a.nbytes
    sys.stderr.write("bench.py: wrote %d output array(s), %.1f MB, to %s%s\n"
                     % (len(arrays), written / 1e6, out_dir, " (a seeded sample of the rows of %s)" % ", ".join(sampled) if sampled else ""))


def pmc_profile(workload, mode, kernel):
    """(HBM bytes per launch, MFMA-busy fraction, tag) of `kernel` from the committed rocprofv3 PMC passes of this same command on one
    lane (separate FETCH_SIZE / WRITE_SIZE / SQ_VALU_MFMA_BUSY_CYCLES runs, gfx950 corrections applied: tools/summarize_profiles.py ->
    profiles/pmc_summary_latest.json, one entry per workload / mode); Nones if there is no entry.  (The counters cannot be read from
    inside this process.)"""
    path = os.path.join(ROOT, "profiles", "pmc_summary_latest.json")
    try:
        with open(path) as f:
            entry = json.load(f)["entries"]["%s/%s" % (workload, mode)]
        return entry["hbm_bytes_per_launch"].get(kernel), entry.get("mfma_busy", {}).get(kernel), entry.get("tag")
    except (OSError, KeyError, ValueError, TypeError):
        return None, None, None


def profile_fields(workload, mode, kernel, frac):
    """The roofline fields that come from the committed profile of this command, and the executed-work fraction."""
    traffic, busy, tag = pmc_profile(workload, mode, kernel)
    return {
        "traffic": traffic, "mfma_busy": busy,
        "executed_frac": (3.0 if mode == "parity" else 1.0) * frac,
        "from_profile": {"tag": tag, "note": "traffic (HBM bytes per launch: 2 x FETCH_SIZE + WRITE_SIZE, the guide's gfx950 correction) and mfma_busy "
                                             "(SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 x 1024 SIMDs)) are the committed rocprofv3 PMC passes of this "
                                             "command on one lane (profiles/<tag>_pmc_summary.json); the counters cannot be read inside this process, so "
                                             "they are the profile's numbers, not measurements of this run.  executed_frac = frac x the MFMA products per "
                                             "algorithmic product (3 in parity mode)"},
    }


def edge_kernels(collect):
    """the HBM-bound edge kernels, achieved GB/s = algorithmic bytes of the launches (cwm_hip.h CWM_KCLASS_*: every input
    element read once, every output element written once) / their summed HIP-event durations, against the 8 TB/s HBM peak."""
    out = {}
    for name, kc in EDGE_CLASSES:
        st = collect(kc)
        if st["launches"]:
            gbs = st["total_flops"] / (st["total_ms"] * 1e-3) / 1e9   # (`total_flops` carries bytes for these classes)
            out[name] = {"bound": "hbm", "achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS, "launches": st["launches"],
                         "avg_launch_us": 1e3 * st["total_ms"] / st["launches"], "bytes_per_launch": st["total_flops"] / st["launches"]}
    return out


def cpu_baseline(cfg, k_vis, clump, seed, budget_s=20.0):
    """The oracle (CPU restatement of the reference, torch fp32 eager) on this box's host cores."""
    from oracle import vmae_oracle as O

    # thread count: best of a scan on the MI355X host (2x EPYC 9575F, 256 hw threads): 16 threads
    # 0.78 s/forward vs 0.90 (8), 0.93 (32), 1.6 (64), 3.2 (128), 45 (256, oversubscribed)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    W = {k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, seed).items()}
    B = 8 if cfg.num_tokens <= 2048 else 2  # (ViT-B/8: batch 8 -- ~3 s per pass on 16 threads; the 6272-token models take ~10x longer per sample: batch 2)
    x = torch.from_numpy(S.synthetic_frames(B, cfg, seed))
    mask = torch.from_numpy(S.synthetic_masks(B, cfg, k_vis, seed, clump))
    spec = O.SPECS[cfg.name]
    with torch.no_grad():
        O.predict(W, spec, x, mask, frame=None)  # warm-up
        n, t0 = 0, time.perf_counter()
        while True:
            O.predict(W, spec, x, mask, frame=None)
            n += 1
            if time.perf_counter() - t0 > budget_s or n >= 6:
                break
        dt = time.perf_counter() - t0
    return {
        "value": B * n / dt, "unit": "frames/s", "cores": torch.get_num_threads(), "host_threads_available": os.cpu_count(), "kind": "port",
        "sample": "%d forward passes of batch %d (%s, k_vis=%d) through oracle/vmae_oracle.py, torch CPU fp32 eager on %d threads (the best of an 8 ... 256 "
                  "scan on this host type; the GPU line runs batch 32)" % (n, B, cfg.name, k_vis, torch.get_num_threads()),
    }


def n_gpus_expected(world, distributed):
    return world if distributed else 1


def prompts_measure(args, rank, local_rank, world, distributed, model=None, steps=None, warmup=None):
    """BASELINE configs[3], strong scaling: 256 prompts on ONE frame pair, sharded over the ranks (dist.py: one packed RCCL
    broadcast, per-rank prompt construction + 32-row predictor calls with no host sync in between, one all-gather).
    value = prompts / max-over-ranks time.  Returns (the last timed step's predictions, the result dict: rank 0 prints it or embeds it)."""
    from counterfactualworldmodels_amd import dist as cdist, segmentation

    cfg = C.CONFIGS[PROMPTS["cfg"]]
    dev = torch.device("cuda", local_rank)
    steps = steps or args.steps
    warmup = max(warmup if warmup is not None else args.warmup, 1)
    if model is None:
        model = vmae.PretrainVisionTransformer(cfg, mode=args.mode)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 0).items()})
        model = model.to(dev).eval()
    G = segmentation.FlowGenerator(predictor=model, imagenet_normalize_inputs=True, temporal_dim=2)
    # (inputs resident in HBM when the timed region starts, like the frame pairs of the headline workload: rank 0 holds the image and the prompt table)
    x0 = torch.from_numpy(S.synthetic_frames(1, cfg, 0))[:, 0:1].to(dev) if rank == 0 else None  # one image; frame 2 := frame 1
    table = torch.from_numpy(S.synthetic_prompts(PROMPTS["total"], cfg, 0)).to(dev) if rank == 0 else None
    hooks = cdist.prompt_hooks(G, frame=-1)
    comm = cdist.get_comm(dev)   # N > 1: RCCL through the C ABI (cwm_comm_init); the torch group only hands the id around
    shapes = ((1, 1, cfg.in_chans) + tuple(cfg.img_size), (PROMPTS["total"], 4), cfg.num_tokens)

    def step():
        return cdist.sharded_counterfactual_predictions(x0, table, *hooks, dev, chunk=PROMPTS["chunk"], gather=True, comm=comm, shapes=shapes)

    for _ in range(warmup):
        y = step()
    assert y.shape[0] == PROMPTS["total"]
    assert comm.world == n_gpus_expected(world, distributed), (comm.world, world)
    if distributed:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        y = None
        y = step()
    torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    dt = time.perf_counter() - t0
    if distributed:
        t = torch.tensor([dt], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    # --full: one more (untimed) step with HIP-event spans around its phases, from every rank: a bad curve on the multi-GPU node can then be read from
    # ONE run -- which rank, which phase (rank 0 alone builds all prompts and rectangularises; the gather runs on a side stream)
    per_rank = None
    if args.full:
        ph = cdist.PhaseTimes(dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        cdist.sharded_counterfactual_predictions(x0, table, *hooks, dev, chunk=PROMPTS["chunk"], gather=True, comm=comm, shapes=shapes, times=ph)
        torch.cuda.synchronize()
        mine = {k: round(v, 3) for k, v in ph.result().items()}
        mine["wall"] = round(1e3 * (time.perf_counter() - t1), 3)
        per_rank = [mine]
        if distributed:
            per_rank = [None] * world
            dist.all_gather_object(per_rank, mine)
    n_gpus = world if distributed else 1
    # --full, N > 1: the gathered result must be the same on every rank and equal, bit for bit, to the single-process result of the same prompts under the
    # same torch seed (the rectangulariser's draws happen on rank 0 either way; every predictor call covers the same 32 consecutive prompts in both runs)
    check = None
    if distributed and args.full:
        torch.manual_seed(4321)
        y_sh = step()
        mine = [float(y_sh.double().sum()), float(y_sh[::37].double().abs().sum())]
        sums = [None] * world
        dist.all_gather_object(sums, mine)
        check = {"same_on_all_ranks": bool(all(v == sums[0] for v in sums))}
        if rank == 0:
            torch.manual_seed(4321)
            y_ref = cdist.sharded_counterfactual_predictions(x0, table, *hooks, dev, chunk=PROMPTS["chunk"], gather=True, comm=cdist.LocalComm())
            check["equals_single_process"] = bool(torch.equal(y_sh, y_ref))
            check["max_abs_diff"] = float((y_sh - y_ref).abs().max())
            del y_ref
        del y_sh
        dist.barrier()
    return y, {
        "sharded_result_check": check,
        "per_rank_ms": per_rank,
        "metric": "predicted frames/sec (2x224x224, ViT-B/8)", "value": PROMPTS["total"] * steps / dt, "unit": "frames/s",
        "n_gpus": n_gpus, "steps": steps, "warmup": warmup, "ms_per_step": 1e3 * dt / steps,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": PROMPTS["name"], "predictor": cfg.name, "prompts": PROMPTS["total"], "chunk": PROMPTS["chunk"],
                   "mode": args.mode, "lanes": args.lanes, "collectives": type(comm).__name__, "comm_world": comm.world,
                   "gather": comm.last_collective,
                   "parallelism": "prompts sharded over %d rank(s): one packed broadcast(frame, prompt table, masks) + one all_gather(predicted frames)" % n_gpus},
    }


def run_prompts(args, rank, local_rank, world, distributed):
    from counterfactualworldmodels_amd import dist as cdist

    y, out = prompts_measure(args, rank, local_rank, world, distributed)
    if rank == 0:
        dump_outputs(args.dump_outputs, {"video": y})
    del y
    if distributed:
        torch.cuda.synchronize()
        dist.barrier()
        cdist.reset_comm()
        dist.destroy_process_group()
    if rank == 0:
        out["build"] = build_info()
        print(json.dumps(out))


def run_imu(args, rank, local_rank, world, distributed):
    """BASELINE configs[4]: IMU-conditioned conjoined base-4x4 predictor, batch 16 (weak scaling over ranks)."""
    from counterfactualworldmodels_amd import conjoined_vmae as CV

    cfg = C.CONJ_CONFIGS["imu400_base_4x4patch_2frames_1tube"]
    dev = torch.device("cuda", local_rank)
    B = args.batch or 16
    model = CV.ConjoinedPaddedVisionTransformer(cfg, mode=args.mode)
    model.load_state_dict({k: torch.from_numpy(S.synthetic_tensor(k, shp, 0)) for k, shp in C.conj_state_dict_schema(cfg).items()})
    model = model.to(dev).eval()
    x = torch.from_numpy(S.synthetic_frames(B, cfg.main, rank)).to(dev).transpose(1, 2)  # [B,C,T,H,W] view, raw frames
    mask = torch.from_numpy(S.synthetic_masks(B, cfg.main, 4, rank)).to(dev)
    g = torch.Generator().manual_seed(rank)
    imu = (torch.randn(B, 6, 400, generator=g) * 0.1).to(dev)
    mc = torch.zeros(B, 25, dtype=torch.bool, device=dev)

    def step():
        return model(x, mask, x_context=imu, mask_context=mc, normalize=True, check=False)

    def region():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = None
        for _ in range(args.steps):
            y = None
            y = step()
        torch.cuda.synchronize()
        if distributed:
            dist.barrier()
        dt = time.perf_counter() - t0
        if distributed:
            t = torch.tensor([dt], device="cuda", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt, y

    step()
    model.set_lanes(args.lanes)
    if os.environ.get("CWM_CONJ_CTX_STREAM") == "0":  # profiling runs: the context stream's launches on the lane's own stream, so that no two
        model.set_option("conj_ctx_stream", 0)          # kernels overlap and per-kernel durations mean what they say
    for _ in range(max(args.warmup, 1)):
        step()
    dt, y = region()
    if rank == 0:  # (the model returns its main stream's tokens, or the tuple (main, context) when it is set to output both)
        dump_outputs(args.dump_outputs, dict(zip(("tokens", "context_tokens"), y)) if isinstance(y, tuple) else {"tokens": y})
    del y
    n_gpus = world if distributed else 1
    flops_pair = 1.422e12  # SURVEY.md §8(d), cfg 5 (k=4)
    value = B * n_gpus * args.steps / dt
    out = {
        "metric": "predicted frames/sec (2x224x224, IMU-conditioned ViT-B/4)", "value": value, "unit": "frames/s", "n_gpus": n_gpus,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": "IMU-conditioned ViT-base 4x4 (conjoined RGB+IMU streams), batch=16 (BASELINE configs[4])", "predictor": cfg.name,
                   "per_gpu_batch": B, "mode": args.mode, "lanes": args.lanes, "tokens_decoder": cfg.main.num_tokens + cfg.main_max_pad},
        "model_tflops": flops_pair * value / 1e12, "model_frac_of_bf16_peak": flops_pair * value / 1e12 / (PEAK_BF16_TFLOPS * n_gpus),
    }
    if args.full:
        imu_kernel_region(args, model, step, region, out, B, n_gpus)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        out["build"] = build_info()
        print(json.dumps(out))


def imu_kernel_region(args, model, step, region, out, B, n_gpus):
    """--full: the kernel region of the IMU workload (as in the headline workload): the same steps on ONE lane with HIP events around every launch of a
    class -> out["roofline"]."""
    classes = {"gemm_wide": _lib.KCLASS_GEMM_WIDE, "gemm_narrow": _lib.KCLASS_GEMM_NARROW, "attention": _lib.KCLASS_ATTENTION,
               "cross_attention": _lib.KCLASS_CROSS_ATTN, "context_self_attention": _lib.KCLASS_SMALL_ATTN}
    model.set_lanes(1)
    for _ in range(2):
        step()
    for kc in [_lib.KCLASS_GEMM, _lib.KCLASS_ATTENTION, _lib.KCLASS_CROSS_ATTN, _lib.KCLASS_SMALL_ATTN] + [kc for _, kc in EDGE_CLASSES]:
        model.timing_enable(kc, True)
    dt_one, _ = region()
    model.timing_collect(_lib.KCLASS_GEMM)  # books the wide / narrow split
    stats = {name: model.timing_collect(kc) for name, kc in classes.items()}
    edge = edge_kernels(model.timing_collect)
    for kc in [_lib.KCLASS_GEMM, _lib.KCLASS_ATTENTION, _lib.KCLASS_CROSS_ATTN, _lib.KCLASS_SMALL_ATTN] + [kc for _, kc in EDGE_CLASSES]:
        model.timing_enable(kc, False)
    model.set_lanes(args.lanes)

    def entry(st):
        tf = st["total_flops"] / (st["total_ms"] * 1e-3) / 1e12 if st["total_ms"] > 0 else 0.0
        return {"achieved": tf, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": tf / PEAK_BF16_TFLOPS, "launches": st["launches"],
                "avg_launch_us": 1e3 * st["total_ms"] / max(st["launches"], 1), "share_of_step": st["total_ms"] / (1e3 * dt_one) if dt_one > 0 else None}

    dom = max(("gemm_wide", "gemm_narrow", "attention"), key=lambda k: stats[k]["total_ms"])
    planes = 2 if args.mode == "parity" else 1
    names = {"gemm_wide": "cwm::gemm8p_kernel<%d>" % planes, "gemm_narrow": "cwm::gemm_bf16_kernel<%d, 128, 128, 2, 4, 2>" % planes,
             "attention": "cwm::attention_pipe_kernel<%d, 4>" % planes,
             "cross_attention": "cwm::cross_attn_mfma_kernel (+ combine)", "context_self_attention": "cwm::small_attn_mfma_kernel"}
    dom_entry = entry(stats[dom])
    out["roofline"] = dict(dom_entry, bound="mfma", kernel=names[dom], edge_kernels=edge, **profile_fields("imu4", args.mode, names[dom], dom_entry["frac"]),
                           region={"lanes": 1, "steps": args.steps, "ms_per_step": 1e3 * dt_one / args.steps, "value": B * n_gpus * args.steps / dt_one},
                           note="algorithmic FLOPs of the class's launches / their summed HIP-event durations in a one-lane kernel region (rank 0)",
                           other_kernel={names[k]: entry(v) for k, v in stats.items() if k != dom})


# ---- the kernels on either side of the predictor path (prompt construction before it, flow-sample statistics after it) -------
PEAK_F32_MFMA_TFLOPS = 157.3  # v_mfma_f32_16x16x4_f32, MI355X_MICROARCH.md (exact fp32 products: what torch.cov computes)


_HOST_ISSUE_MS = {}


def _stage_ms(fn, steps, key=None):
    """Mean device time of `fn` over `steps` calls between two HIP events on torch's current stream -- the stream every C-ABI call of these workloads
    launches on (`_lib.current_stream_handle`).  The host's time to ISSUE the calls is kept beside it (`key`): a stage of a few small kernels is bound by the
    Python / ctypes call overhead, and then the event span measures the host, not the kernels (rocprofv3's per-kernel durations under profiles/ are the kernel rates)."""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    issue = time.perf_counter() - t0
    b.record()
    torch.cuda.synchronize()
    if key is not None:
        _HOST_ISSUE_MS[key] = 1e3 * issue / steps
    return a.elapsed_time(b) / steps


def _hbm_entry(bytes_per_call, ms, kernels, key=None):
    gbs = bytes_per_call / (ms * 1e-3) / 1e9
    e = {"bound": "hbm", "achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS, "avg_us": 1e3 * ms, "bytes_per_call": bytes_per_call,
         "kernels": kernels}
    if key in _HOST_ISSUE_MS:
        e["host_issue_us"] = 1e3 * _HOST_ISSUE_MS[key]
        e["issue_bound"] = bool(_HOST_ISSUE_MS[key] > 0.8 * ms)  # the host needs as long to issue the stage's calls as the events saw: the span is not kernel time
    return e


def aux_profile(workload, prefix):
    """(HBM bytes per launch, MFMA-busy share) of the kernel whose name starts with `prefix` (template arguments follow it in rocprofv3's names) from the committed
    PMC passes of this command (profiles/pmc_summary_latest.json: the largest dispatches of the kernel -- these workloads launch it at two sizes), or Nones."""
    path = os.path.join(ROOT, "profiles", "pmc_summary_latest.json")
    try:
        with open(path) as f:
            entry = json.load(f)["entries"]["%s/f32" % workload]
    except (OSError, KeyError, ValueError, TypeError):
        return None, None
    pick = lambda d: next((v for k, v in sorted(d.items()) if k.startswith(prefix)), None)
    return pick(entry.get("hbm_bytes_per_launch", {})), pick(entry.get("mfma_busy", {}))


def aux_traffic(workload, prefix):
    return aux_profile(workload, prefix)[0]


def flowstats_measure(S_samples, steps, dev, cpu=False, full=True):
    """One frame pair's S counterfactual flow samples [1, 2, 224, 224, S] (the reference's layout: sample axis innermost) through the reductions of
    segmentation.py:250-276, 479-547 at downsample 2 (P = 112 x 112 = 12544 positions): pooled magnitudes -> z-score prologue -> covariance [P, P] ->
    mean motion map.  `value` is samples reduced per second over the default chain (features + covariance + motion map); with `full` every stage is also
    timed on its own (`stages`).  res["outputs"] = the last timed chain's results."""
    from counterfactualworldmodels_amd import flowstats as FS

    H = W = 224
    ds = 2
    P = (H // ds) * (W // ds)
    g = torch.Generator().manual_seed(0)
    flows = (torch.randn(1, 2, H, W, S_samples, generator=g) * 2).to(dev)
    stages = flowstats_stages(flows, ds, P, S_samples, steps) if full else None

    def chain():
        return (FS.compute_flow_corrs(flows, downsample=ds, use_covariance=True),
                FS.compute_mean_motion_map(flows, normalize_per_sample=True))

    for _ in range(2):
        chain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = None
    for _ in range(steps):
        y = None
        y = chain()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"value": S_samples * steps / dt, "ms_per_step": 1e3 * dt / steps, "stages": stages, "samples": S_samples, "positions": P,
           "outputs": {"corrs": y[0], "motion_map": y[1]}}
    if cpu:
        from oracle import flowstats_oracle as FO

        torch.set_num_threads(min(16, os.cpu_count() or 1))
        fc = flows.cpu()
        t0 = time.perf_counter()
        n = 0
        while n < 4 and time.perf_counter() - t0 < 20.0:
            FO.compute_flow_corrs(fc, ds, True)
            FO.compute_mean_motion_map(fc, normalize_per_sample=True, normalize=True)
            n += 1
        dtc = time.perf_counter() - t0
        res["cpu_baseline"] = {"value": S_samples * n / dtc, "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port",
                               "sample": "%d passes of the same chain (S = %d, 224x224, downsample 2) through oracle/flowstats_oracle.py, torch CPU fp32 on %d threads"
                                         % (n, S_samples, torch.get_num_threads())}
    return res


def flowstats_stages(flows, ds, P, S_samples, steps):
    """--full: every stage of the flow-statistics chain timed on its own (HIP events on the launching stream)."""
    from counterfactualworldmodels_amd import flowstats as FS

    H, W = flows.shape[2:4]
    x = FS.flow_features(flows, ds)
    stages = {}
    f_bytes = flows.numel() * 4
    x_bytes = x.numel() * 4
    ms = _stage_ms(lambda: FS.flow_features(flows, ds), steps, "features")
    stages["features"] = _hbm_entry(f_bytes + x_bytes, ms, ["flow_features_kernel"], "features")
    xz = x.clone()
    ms = _stage_ms(lambda: FS.transform_features(xz, zscore=True), steps, "zscore")  # (in place, again and again on the same buffer: the values do not matter here)
    stages["zscore_prologue"] = _hbm_entry(3 * x_bytes, ms, ["flow_colpartial_kernel (one pass over x)", "flow_colfinish_kernel", "flow_apply_kernel (read + write)"], "zscore")
    ms_cov = _stage_ms(lambda: FS.feature_cov_rows(x, 0, P, True), steps, "cov")
    out_bytes = P * P * 4
    flops = 2.0 * P * P * S_samples
    cov = _hbm_entry(out_bytes + 3 * x_bytes, ms_cov, ["flow_center_kernel", "flow_cov_kernel"], "cov")
    tf = flops / (ms_cov * 1e-3) / 1e12
    tiles = (P + 127) // 128
    executed = (tiles + 1) / (2.0 * tiles)  # the kernel computes the 128 x 128 tiles on and above the diagonal only and mirrors them
    cov["as_mfma"] = {"bound": "mfma", "achieved": tf, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": tf / PEAK_F32_MFMA_TFLOPS, "flops_per_call": flops,
                      "executed_frac": executed * tf / PEAK_F32_MFMA_TFLOPS,
                      "note": "fp32-input MFMA (exact fp32 products); the algorithmic count is the full [P, P] product 2 P^2 S that torch.cov performs -- the kernel executes "
                              "%.3f of it (symmetry: tiles on and above the diagonal), so `frac` can exceed 1 while `executed_frac` is the matrix pipe's own share" % executed}
    stages["covariance"] = cov
    ms = _stage_ms(lambda: FS.compute_mean_motion_map(flows, normalize_per_sample=True), steps, "motion")
    stages["motion_map"] = _hbm_entry(2 * f_bytes + H * W * 4 * 3, ms, ["flow_mag_minmax_*_kernel", "flow_motion_sum_*_kernel", "flow_map_finish_kernel"], "motion")
    return stages


def run_flowstats(args):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    main_S, other_S = 256, 24
    r = flowstats_measure(main_S, args.steps, dev, cpu=args.full and not args.no_cpu_baseline, full=args.full)
    dump_outputs(args.dump_outputs, r.pop("outputs"))
    out = {
        "metric": "counterfactual flow samples reduced/sec (224x224, downsample 2: features -> covariance [12544^2] -> motion map)", "value": r["value"], "unit": "samples/s",
        "n_gpus": 1, "steps": args.steps, "warmup": 2, "ms_per_step": r["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic", "config": {"workload": "flow-sample statistics of one frame pair (SURVEY.md 8 f-4; segmentation.py:250-276, 479-547), S = 256 samples",
                                        "samples": main_S, "positions": r["positions"], "downsample": 2},
        "build": build_info(),
    }
    if not args.full:
        print(json.dumps(out))
        return
    r2 = flowstats_measure(other_S, args.steps, dev)
    r2.pop("outputs")
    cov = r["stages"]["covariance"]
    roof = dict(cov["as_mfma"], kernel="cwm::flow_cov_kernel (+ flow_center_kernel)", avg_launch_us=cov["avg_us"], traffic=aux_traffic("flowstats", "cwm::flow_cov_kernel<true, 2>"), mfma_busy=aux_profile("flowstats", "cwm::flow_cov_kernel<true, 2>")[1],
                as_hbm={k: cov[k] for k in ("achieved", "peak", "unit", "frac", "bytes_per_call")},
                stages={k: v for k, v in r["stages"].items() if k != "covariance"},
                note="S = 256: 2 P^2 S = 80.6 GFLOP of exact-fp32 MFMA against a 629-MB result: the fp32 matrix pipe bounds it (0.51 ms at peak vs 0.08 ms of HBM write); "
                     "at S = 24 (secondary) the same kernel is bound by the 629-MB write.  HIP events around the stage's calls on the launching stream")
    out["roofline"] = roof
    out["secondary"] = {"samples": other_S, "value": r2["value"], "unit": "samples/s", "ms_per_step": r2["ms_per_step"], "stages": r2["stages"],
                        "note": "S = 24 (the demo notebooks' sample count): the covariance stage is bound by the HBM write of the [P, P] result"}
    if "cpu_baseline" in r:
        out["cpu_baseline"] = r["cpu_baseline"]
    print(json.dumps(out))


def run_prompt_build(args):
    """device-side construction of the 256 motion-counterfactual prompts of BASELINE configs[3] from one image (frames [256, 2, 3, 224, 224]
    = 308 MB + masks [256, 1568]); reference: the per-sample loop of segmentation.py:324-338 over perturbation.py:245-289."""
    from counterfactualworldmodels_amd import dist as cdist, segmentation

    cfg = C.CONFIGS[PROMPTS["cfg"]]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model = vmae.PretrainVisionTransformer(cfg, mode=args.mode)
    G = segmentation.FlowGenerator(predictor=model, imagenet_normalize_inputs=True, temporal_dim=2)
    x0 = torch.from_numpy(S.synthetic_frames(1, cfg, 0))[:, 0:1].to(dev)
    table_h = torch.from_numpy(S.synthetic_prompts(PROMPTS["total"], cfg, 0))
    table = table_h.to(dev)
    build, rect, _ = cdist.prompt_hooks(G, frame=-1)
    n = PROMPTS["total"]
    frame_bytes = n * 2 * 3 * cfg.img_size[0] * cfg.img_size[1] * 4
    mask_bytes = n * cfg.num_tokens
    in_bytes = 3 * cfg.img_size[0] * cfg.img_size[1] * 4
    xs, ms_ = build(x0, table)
    assert xs.shape == (n, 2, 3) + tuple(cfg.img_size) and ms_.shape == (n, cfg.num_tokens)
    del xs, ms_
    if args.full:  # every call and kernel timed on its own -> `roofline`
        t_all = _stage_ms(lambda: build(x0, table), args.steps)
        t_masks = _stage_ms(lambda: build(x0, table, frames=False), args.steps)
        t_32 = _stage_ms(lambda: build(x0, table[:32]), args.steps)
        # the frames kernel alone through the C ABI (no torch index ops around it)
        passive = (torch.arange(cfg.num_tokens, device=dev) >= cfg.tokens_per_frame)[None].expand(n, -1).contiguous()
        active = passive.clone()
        gw = cfg.img_size[1] // cfg.patch
        active[torch.arange(n, device=dev), cfg.tokens_per_frame + table[:, 0].long() * gw + table[:, 1].long()] = False
        shifts = table[:, 2:4].contiguous()
        xb = x0.expand(-1, 2, -1, -1, -1)
        t_kernel = _stage_ms(lambda: G._shift_rows(xb, passive, active, shifts, 1, True, samples_per_movie=n, masks=False), args.steps)
        t_mask_kernel = _stage_ms(lambda: G._shift_rows(xb, passive, active, shifts, 1, True, samples_per_movie=n, frames=False), args.steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = None
    for _ in range(args.steps):
        y = None
        y = build(x0, table)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dump_outputs(args.dump_outputs, {"frames": y[0], "masks": y[1]})
    del y
    out = {
        "metric": "motion-counterfactual prompts built/sec (2x224x224 frames + 1568-token masks, ViT-B/8 grid)", "value": n * args.steps / dt, "unit": "prompts/s", "n_gpus": 1,
        "steps": args.steps, "warmup": 1, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32 copies, u8 masks",
        "data": "synthetic", "config": {"workload": "device-side construction of the 256 prompts of BASELINE configs[3] (SURVEY.md 8 f-1; segmentation.py:324-338, "
                                                    "perturbation.py:245-289)", "prompts": n, "predictor_grid": cfg.name},
        "build": build_info(),
    }
    if args.full:
        out["roofline"] = dict(_hbm_entry(frame_bytes + in_bytes, t_kernel, ["shift_prompts_x_kernel"]), kernel="cwm::shift_prompts_x_kernel", avg_launch_us=1e3 * t_kernel,
                               traffic=aux_traffic("prompt_build", "cwm::shift_prompts_x_kernel"),
                               other_kernel={"cwm::shift_prompts_mask_kernel": _hbm_entry(3 * mask_bytes, t_mask_kernel, ["shift_prompts_mask_kernel"])},
                               host_call_ms={"frames + masks, 256 prompts (torch index ops + both kernels)": t_all, "masks only, 256 prompts (rank 0 of a sharded call)": t_masks,
                                             "frames + masks, 32 prompts (one rank's shard at 8 ranks)": t_32},
                               note="algorithmic bytes = 256 x 1.2 MB of frames written + the 602-KB image read once; HIP events around the C-ABI call on the launching stream")
    if args.full and not args.no_cpu_baseline:
        from oracle import vmae_oracle as O

        torch.set_num_threads(min(16, os.cpu_count() or 1))
        xc = x0.cpu().expand(-1, 2, -1, -1, -1).contiguous()
        pas, act = passive.cpu().t()[None].contiguous(), active.cpu().t()[None].contiguous()  # [1, Nt, S]
        sh = [tuple(int(v) for v in r) for r in table_h[:, 2:4].tolist()]
        t0 = time.perf_counter()
        k = 0
        while k < 3 and time.perf_counter() - t0 < 20.0:
            O.create_motion_counterfactuals(xc, pas, act, sh, cfg.patch, frame=1, fix_passive=True)
            k += 1
        dtc = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": n * k / dtc, "unit": "prompts/s", "cores": torch.get_num_threads(), "kind": "port",
                               "sample": "%d passes over the same 256 prompts through oracle/vmae_oracle.py create_motion_counterfactuals (the reference's per-sample loop)" % k}
    print(json.dumps(out))


def count_gpus_without_hip():
    """GPUs of this box from the KFD topology in sysfs (nodes with SIMDs), without a HIP call: torch.cuda.device_count() falls through to
    hipGetDeviceCount on ROCm builds without amdsmi, which initialises the runtime in the caller.  *_VISIBLE_DEVICES lists cap the count.
    None if sysfs has no topology (then the caller may still ask torch)."""
    import glob

    n = 0
    nodes = glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")
    if not nodes:
        return None
    for path in nodes:
        try:
            with open(path) as f:
                props = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
            if int(props.get("simd_count", "0")) > 0:
                n += 1
        except (OSError, ValueError):
            pass
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([t for t in v.split(",") if t.strip() != ""]))
    return n


def self_launch(args):
    """`python bench.py --gpus N` without a launcher (WORLD_SIZE unset): start the N ranks with torch.distributed.run as a CHILD
    process -- the parent only counts the GPUs (from sysfs, no HIP call), relays the child's output and exit code; the ranks are always
    fresh processes.  Fails loudly when the box has fewer than N GPUs: a line must never claim more GPUs than it ran on."""
    import socket
    import subprocess

    have = count_gpus_without_hip()
    if have is None:
        have = torch.cuda.device_count()
    if have < args.gpus and os.environ.get("CWM_BENCH_ONE_DEVICE") != "1":
        sys.stderr.write("bench.py: --gpus %d requested but this box has %d GPU(s); refusing to measure fewer GPUs than asked for\n" % (args.gpus, have))
        return 2
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.run(cmd, env=env).returncode


def full_extras(args, out, model, G, x, mask, n_vis, cfg, wl, B, checksum_before, rank, local_rank, world, distributed):
    """--full, after the timed region of the base8 / large4 workloads: the output-stability check, the one-lane kernel region (`roofline`), the other
    arithmetic mode (`secondary`), BASELINE configs[3] beside the headline (`prompts256`) and the CPU baseline -- each into `out`."""
    n_gpus = world if distributed else 1
    checksum_after = float(G.predict(x, mask, frame=None).double().sum())
    # one more (untimed) step before and after the timed region: same input, same bits expected (a timing-dependent fault would show here)
    out["output_stable"] = bool(checksum_before == checksum_after and checksum_after == checksum_after)

    # ---- kernel region: the same K steps on ONE lane with a HIP event pair around every GEMM launch -> `roofline`.  With two lanes a
    # launch shares the chip with whatever the other lane runs, so its duration says nothing about the kernel; here launches are alone.
    # With --lanes 1 the two regions are the same thing (and that is the command the rocprofv3 summaries under profiles/ are taken from).
    model.set_lanes(1)
    if args.lanes != 1:
        for _ in range(2):
            G.predict(x, mask, frame=None)
    model.timing_enable(_lib.KCLASS_GEMM, True)
    model.timing_enable(_lib.KCLASS_ATTENTION, True)
    for _, kc in EDGE_CLASSES:
        model.timing_enable(kc, True)
    dt_one, _ = timed_steps(G, x, mask, n_vis, args.steps, distributed)
    gemm = model.timing_collect(_lib.KCLASS_GEMM)                 # every GEMM launch ...
    gemm_wide = model.timing_collect(_lib.KCLASS_GEMM_WIDE)       # ... split by the kernel that ran it
    gemm_narrow = model.timing_collect(_lib.KCLASS_GEMM_NARROW)
    attn = model.timing_collect(_lib.KCLASS_ATTENTION)            # softmax(q k^T) v: 4 N^2 64 FLOP per (batch, head)
    edge = edge_kernels(model.timing_collect)
    model.timing_enable(_lib.KCLASS_GEMM, False)
    model.timing_enable(_lib.KCLASS_ATTENTION, False)
    for _, kc in EDGE_CLASSES:
        model.timing_enable(kc, False)
    model.set_lanes(args.lanes)

    planes = 2 if args.mode == "parity" else 1
    kernels = {  # (names as rocprofv3 prints them)
        "cwm::gemm8p_kernel<%d>" % planes: gemm_wide,                          # 256x256 8-phase: qkv, fc1, whole rounds of fc2
        "cwm::gemm_bf16_kernel<%d, 128, 128, 2, 4, 2>" % planes: gemm_narrow,  # 128x128, 8 waves: proj, narrow outputs, remainders
        "cwm::attention_pipe_kernel<%d, 4>" % planes: attn,   # softmax(q k^T) v
    }

    def tflops(st):
        return st["total_flops"] / (st["total_ms"] * 1e-3) / 1e12 if st["total_ms"] > 0 else 0.0

    def kentry(k, v):
        tf = tflops(v)
        return dict({"achieved": tf, "frac": tf / PEAK_BF16_TFLOPS, "launches": v["launches"], "avg_launch_us": 1e3 * v["total_ms"] / max(v["launches"], 1),
                     "share_of_step": v["total_ms"] / (1e3 * dt_one) if dt_one > 0 else None}, **profile_fields(args.workload, args.mode, k, tf / PEAK_BF16_TFLOPS))

    dom = max(kernels, key=lambda k: kernels[k]["total_ms"])  # dominant kernel = most device time in the kernel region (attention included)
    st = kernels[dom]
    ach = tflops(st)
    out["roofline"] = {
        "bound": "mfma", "kernel": dom, "achieved": ach, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_BF16_TFLOPS,
        **profile_fields(args.workload, args.mode, dom, ach / PEAK_BF16_TFLOPS),
        "edge_kernels": edge,
        "launches": st["launches"], "avg_launch_us": 1e3 * st["total_ms"] / max(st["launches"], 1),
        "share_of_step": st["total_ms"] / (1e3 * dt_one) if dt_one > 0 else None,
        "region": {"lanes": 1, "steps": args.steps, "ms_per_step": 1e3 * dt_one / args.steps, "value": B * n_gpus * args.steps / dt_one,
                   "note": "kernel region: the same steps as the timed region, one lane, HIP events around every GEMM / attention launch"},
        "note": "algorithmic FLOPs (2*M*N*K per GEMM launch, 4*N^2*64 per (batch, head) of an attention launch) of this kernel's launches in the "
                "kernel region / their summed HIP-event durations (rank 0)"
                + ("; parity mode executes 3x these FLOPs on the MFMA pipe (executed_frac)" if args.mode == "parity" else ""),
        "all_gemm": {"achieved": tflops(gemm), "launches": gemm["launches"], "avg_launch_us": 1e3 * gemm["total_ms"] / max(gemm["launches"], 1),
                     "share_of_step": gemm["total_ms"] / (1e3 * dt_one) if dt_one > 0 else None},
        "other_kernel": {k: kentry(k, v) for k, v in kernels.items() if k != dom},
    }

    if not args.no_secondary:
        other = "fast" if args.mode == "parity" else "parity"
        model.mode = other
        for _ in range(2):
            G.predict(x, mask, frame=None)
        dt2, _ = timed_steps(G, x, mask, n_vis, args.steps, distributed)
        out["secondary"] = {"mode": other, "value": B * n_gpus * args.steps / dt2, "unit": "frames/s",
                            "ms_per_step": 1e3 * dt2 / args.steps,
                            "note": "plain-bf16 fast mode does NOT meet the 1e-3 parity tolerance (see tests/test_model_gpu.py)"
                            if other == "fast" else "split-bf16 parity mode"}
        model.mode = args.mode

    # ---- BASELINE configs[3] beside the headline, at every N: the >= 6x target of the north star is quoted on this STRONG-scaling
    # batch (256 prompts in total), while `value` above is the weak-scaling frame-pair throughput.  Measurement plumbing only: a
    # failure here is reported in the line, it does not take the headline down.
    if args.workload == "base8" and not args.no_prompts:
        try:
            _, pm = prompts_measure(args, rank, local_rank, world, distributed, model=model, steps=max(3, args.steps // 4), warmup=2)
            out["prompts256"] = {k: pm[k] for k in ("value", "unit", "n_gpus", "ms_per_step", "scaling", "steps", "per_rank_ms", "sharded_result_check")}
            out["prompts256"]["config"] = pm["config"]
            out["rccl_ranks"], out["collectives"] = pm["config"]["comm_world"], pm["config"]["collectives"]
        except Exception as e:  # noqa: BLE001
            out["prompts256"] = {"error": "%s: %s" % (type(e).__name__, e)}
            if distributed:
                # the multi-rank path IS what N > 1 is run for: a broken broadcast / gather must not exit 0.  The headline measured above is
                # still printed (with the error in it), then every rank that saw the failure leaves with a non-zero code -- without the
                # teardown collectives, which ranks that are out of step with each other could not complete
                import traceback

                traceback.print_exc()
                if rank == 0:
                    print(json.dumps(out), flush=True)
                os._exit(3)

    if rank == 0 and n_gpus == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(cfg, wl["k_vis"], wl["clump"], 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="base8", choices=sorted(WORKLOADS) + ["prompts256", "imu4", "flowstats", "prompt_build"])
    ap.add_argument("--mode", default="parity", choices=["parity", "fast"])
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--full", action="store_true",
                    help="also run every check and side measurement beside the headline (output stability, roofline kernel region, the other "
                         "arithmetic mode, prompts256, per-rank phases, per-stage timings, CPU baseline); a plain run only times the steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32, at most 64 MB in all: a seeded sample of larger outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the extra fast-mode measurement")
    ap.add_argument("--no-prompts", action="store_true", help="with --full: skip the 256-prompt strong-scaling measurement beside the headline")
    ap.add_argument("--lanes", type=int, default=2, choices=[1, 2, 3, 4],
                    help="2 (library default): the batch runs as two half batches on two HIP streams; 1: one stream")
    args = ap.parse_args()

    if args.workload in ("flowstats", "prompt_build"):  # one-GPU edge workloads: no launcher, no process group
        if args.gpus != 1:
            sys.stderr.write("bench.py: --workload %s measures one GPU\n" % args.workload)
            sys.exit(2)
        return run_flowstats(args) if args.workload == "flowstats" else run_prompt_build(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    distributed = world > 1
    if world != args.gpus:  # the line reports n_gpus = the launcher's world size: it must be what was asked for
        sys.stderr.write("bench.py: --gpus %d but the launcher started %d rank(s) (WORLD_SIZE)\n" % (args.gpus, world))
        sys.exit(2)
    # Test hooks (tools/run_bench_2ranks_1gpu.sh): CWM_BENCH_ONE_DEVICE=1 puts every rank on cuda:0 and CWM_BENCH_BACKEND=gloo replaces the
    # launcher's RCCL group, so that the multi-rank control flow (sharding, packed broadcast, gather, max-over-ranks clock) can be run
    # on a one-GPU box; RCCL itself refuses two ranks on one device.  Never set for measurements.
    if os.environ.get("CWM_BENCH_ONE_DEVICE") == "1":
        local_rank = 0
    backend = os.environ.get("CWM_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    n_gpus = world if distributed else 1
    if args.workload == "prompts256":
        return run_prompts(args, rank, local_rank, world, distributed)
    if args.workload == "imu4":
        return run_imu(args, rank, local_rank, world, distributed)

    wl = WORKLOADS[args.workload]
    cfg = C.CONFIGS[wl["cfg"]]
    B = args.batch or wl["batch"]
    n_vis = cfg.tokens_per_frame + wl["k_vis"]
    dev = torch.device("cuda", local_rank)

    model = vmae.PretrainVisionTransformer(cfg, mode=args.mode)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 0).items()})
    model = model.to(dev).eval()
    # every rank owns a different shard of synthetic frame pairs (seed = rank)
    x = torch.from_numpy(S.synthetic_frames(B, cfg, rank)).to(dev)
    mask = torch.from_numpy(S.synthetic_masks(B, cfg, wl["k_vis"], rank, wl["clump"])).to(dev)

    from counterfactualworldmodels_amd import segmentation

    G = segmentation.FlowGenerator(predictor=model, imagenet_normalize_inputs=True, temporal_dim=2)
    model.sync_weights()
    model.set_lanes(args.lanes)
    if args.full:
        model.predict_video(x, mask, normalize=True, n_vis=n_vis, check=True)  # validates the synthetic masks once (device-side row check)
    for _ in range(max(args.warmup, 1)):
        G.predict(x, mask, frame=None)
    if args.full:
        checksum_before = float(G.predict(x, mask, frame=None).double().sum())  # (untimed) the same step again after the timed region must give the same bits
    torch.cuda.synchronize()

    # ---- timed region: `value` -------------------------------------------------------------------------------------------------
    dt, y = timed_steps(G, x, mask, n_vis, args.steps, distributed)
    if rank == 0:
        dump_outputs(args.dump_outputs, {"video": y})
    del y

    value = B * n_gpus * args.steps / dt
    flops_pair = C.algorithmic_flops(cfg, n_vis)
    out = {
        "metric": "predicted frames/sec (2x224x224, ViT-B/8)" if args.workload == "base8" else "predicted frames/sec (2x224x224, ViT-L/4)",
        "value": value, "unit": "frames/s", "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16", "data": "synthetic",
        "config": {
            "workload": wl["name"], "predictor": cfg.name, "per_gpu_batch": B, "global_batch": B * n_gpus, "n_vis": n_vis,
            "tokens_decoder": cfg.num_tokens, "mode": args.mode,
            "lanes": "%d (%s)" % (args.lanes, "the batch runs as two half batches on two HIP streams inside the library" if args.lanes == 2
                                  else "every kernel on one stream"),
            "arithmetic": "split-bf16 (hi+lo) MFMA operands, 3 MFMAs/product, fp32 accumulate" if args.mode == "parity"
            else "bf16 MFMA operands, fp32 accumulate",
            "parallelism": "dp%d (independent frame pairs per rank, no collective)" % n_gpus,
            "weights": "random-init (deterministic synthetic generator)",
        },
        "model_tflops": flops_pair * value / 1e12,
        "model_frac_of_bf16_peak": flops_pair * value / 1e12 / (PEAK_BF16_TFLOPS * n_gpus),
        "build": build_info(),
    }
    if args.full:
        full_extras(args, out, model, G, x, mask, n_vis, cfg, wl, B, checksum_before, rank, local_rank, world, distributed)
    if distributed:
        from counterfactualworldmodels_amd import dist as cdist

        torch.cuda.synchronize()
        dist.barrier()
        cdist.reset_comm()  # destroys the RCCL communicator of the data path (every rank, after the last collective)
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
