"""Same-process A/B of the default two-lane ViT-B/8 batch-32 parity step between ANOTHER build of the library (the parent commit's: CWM_HIP_LIB_OUT=... python -m
counterfactualworldmodels_amd.build in a checkout of it) and this tree's, for the round-7 work-removal parts:  python tools/ab_parts.py PARENT_LIB [PAIRS]
Two model handles in one process, one per library (`use_library`), measured alternately -- A B, then B A, so that what the second measurement of a pair gains or
loses by its place cancels over two pairs; a measurement = the average of 20 steps after 5 warm-up steps.  Cases: parent against parent (two handles of the
parent library: the spread of the method), each part alone through its switch, both switches off, both parts, parent against parent again.  Every case also
compares the outputs of its two handles bit for bit.  CASES=substring,... selects cases."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from counterfactualworldmodels_amd import _lib, config as C, synthetic as S, vmae

pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 10
cfg = C.CONFIGS["base_8x8patch_2frames_1tube"]
sd = {k: torch.from_numpy(v) for k, v in S.synthetic_state_dict(cfg, 0).items()}
x = torch.from_numpy(S.synthetic_frames(32, cfg, 0)).cuda()
mask = torch.from_numpy(S.synthetic_masks(32, cfg, 8, 0, 1)).cuda()
nv = cfg.tokens_per_frame + 8
parent_lib = _lib._bind(os.path.abspath(sys.argv[1]))
print("parent library: %s   this tree: %s" % (parent_lib.cwm_source_hash().decode(), _lib.get_lib().cwm_source_hash().decode()), flush=True)


def model(lib, **opts):
    m = vmae.PretrainVisionTransformer(cfg, mode="parity")
    m.load_state_dict(sd)
    if lib is not None:
        m.use_library(lib)
    for k, v in opts.items():
        m.set_option(k, v)
    m = m.cuda().eval()
    m.predict_video(x, mask, n_vis=nv)
    return m


def run(m):
    for _ in range(5):
        m.predict_video(x, mask, n_vis=nv, check=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        y = m.predict_video(x, mask, n_vis=nv, check=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / 20, y


cases = [("parent vs parent", dict(lib=parent_lib), dict(lib=parent_lib)),
         ("C half-height tile alone", dict(lib=parent_lib), dict(lib=None, mask_token_tables=0)),
         ("A mask-token tables alone", dict(lib=parent_lib), dict(lib=None, gemm_debug=2048)),
         ("none: new library, both switches off", dict(lib=parent_lib), dict(lib=None, gemm_debug=2048, mask_token_tables=0)),
         ("all parts", dict(lib=parent_lib), dict(lib=None)),
         ("parent vs parent again", dict(lib=parent_lib), dict(lib=parent_lib))]
only = os.environ.get("CASES")
for name, ka, kb in cases:
    if only and not any(o in name for o in only.split(",")):
        continue
    a, b = model(**ka), model(**kb)
    gains, eq = [], True
    for p in range(pairs):
        if p % 2 == 0:
            ta, ya = run(a)
            tb, yb = run(b)
        else:
            tb, yb = run(b)
            ta, ya = run(a)
        eq = eq and all(torch.equal(u, v) for u, v in zip(ya, yb))
        gains.append(100.0 * (ta - tb) / ta)
        print("  %-46s pair %2d  A %.3f ms  B %.3f ms  gain %+.2f %%" % (name, p, 1e3 * ta, 1e3 * tb, gains[-1]), flush=True)
    print("%-48s median gain %+.3f %%  mean %+.3f  (A-first pairs %+.3f, B-first pairs %+.3f)  min %+.2f  max %+.2f  stdev %.2f  outputs bit-equal %s" % (
        name, statistics.median(gains), statistics.mean(gains), statistics.median(gains[0::2]), statistics.median(gains[1::2]), min(gains), max(gains),
        statistics.pstdev(gains), eq), flush=True)
    del a, b
    torch.cuda.empty_cache()
