"""Per-launch numbers of this tree's library (development build), parity mode:
  * the M = 12672 encoder shapes (one lane's 16 x 792 rows) on the 8-phase kernel, the half-height row tile on ("gemm_debug" 0) and off (2048);
  * the decoder Q/K/V shape at M = 50176 (all rows) and M = 25344 (visible rows), and at one lane's 25088 / 12672;
  * the model's own event timers over one-lane steps with the mask-token table on and off: LayerNorm, GEMM and mask-fill (+ gather) class totals per step."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from counterfactualworldmodels_amd import _lib, config as CF, synthetic as S, vmae

torch.cuda.init()
lib = _lib.get_dev_lib()
us = C.c_double()
def gemm(M, N, K, epi, **sw):
    for k, v in sw.items(): _lib.check(lib.cwm_debug_set(k.encode(), v), lib)
    best = 1e30
    for _ in range(5):
        _lib.check(lib.cwm_bench_gemm(M, N, K, _lib.mode_id("parity"), epi, 20, C.byref(us)), lib)
        best = min(best, us.value)
    for k in sw: lib.cwm_debug_set(k.encode(), 0)
    return best
print("== encoder shapes at M = 12672, 8-phase kernel forced (as inside a two-lane call): half-height tile off / on")
for name, N, K, epi in [("enc.qkv", 2304, 768, 3), ("enc.proj", 768, 768, 0), ("enc.fc1", 3072, 768, 1), ("enc.fc2", 768, 3072, 0)]:
    off, on = gemm(12672, N, K, epi, gemm_tile=4, gemm_debug=2048), gemm(12672, N, K, epi, gemm_tile=4, gemm_debug=0)
    print("%-9s M 12672 N %4d K %4d  full tile %7.1f us  half-height %7.1f us  %+.2f %%" % (name, N, K, off, on, 100 * (off - on) / off), flush=True)
print("== decoder Q/K/V (N 1152, K 384), default tile rule")
for M in (50176, 25344, 25088, 12672):
    print("dec.qkv  M %5d  %7.1f us" % (M, gemm(M, 1152, 384, 3)), flush=True)

cfg = CF.CONFIGS["base_8x8patch_2frames_1tube"]
m = vmae.PretrainVisionTransformer(cfg, mode="parity")
m.load_state_dict({k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 0).items()})
m = m.cuda().eval()
x = torch.from_numpy(S.synthetic_frames(32, cfg, 0)).cuda()
mask = torch.from_numpy(S.synthetic_masks(32, cfg, 8, 0, 1)).cuda()
m.predict_video(x, mask, n_vis=792)
m.set_lanes(1)
print("== one-lane batch-32 step, event timers per kernel class (ms per step), mask-token table off / on")
classes = [("layernorm", _lib.KCLASS_LAYERNORM), ("gemm", _lib.KCLASS_GEMM), ("mask fill (+ gather)", _lib.KCLASS_FILL_MASK)]
res = {}
for tables in (0, 1, 0, 1):
    m.set_option("mask_token_tables", tables)
    for _ in range(3): m.predict_video(x, mask, n_vis=792, check=False)
    for _, k in classes: m.timing_enable(k, True)
    torch.cuda.synchronize()
    steps = 10
    for _ in range(steps): m.predict_video(x, mask, n_vis=792, check=False)
    torch.cuda.synchronize()
    for name, k in classes:
        st = m.timing_collect(k)
        res.setdefault((name, tables), []).append((st["launches"] / steps, 1e3 * st["total_ms"] / steps))
        m.timing_enable(k, False)
for name, _ in classes:
    for tables in (0, 1):
        print("%-22s tables %d: %s" % (name, tables, "  ".join("%.0f launches %.1f us" % r for r in res[(name, tables)])), flush=True)
