"""A plain-Python restatement of how a GEMM launch was laid out BEFORE `gemm_plan` (csrc/gemm.hip) became the one place that decides it: the
functions the launcher and the engine shared then -- `gemm_choose_tile`, `gemm_mixed_split`, `deep_tile_rows`, `gemm_splitk_parts` -- and the
launcher's own conditions (`launch_gemm_checked`, `launch_gemm_cfg`), statement for statement and in the launcher's order.  Written from that code,
not from `gemm_plan`: `tests/test_gemm_plan_cpu.py` holds the library's read-out (`cwm_dev_gemm_plan`) against it, so a change of the rule shows up as
a difference from what the library did before."""

EPI_F32, EPI_BF16_GELU, EPI_BF16, EPI_QKV = range(4)
KERNEL_128, KERNEL_DEEP128, KERNEL_DEEP64, KERNEL_8PHASE = range(4)


def choose_tile(M, N, K, epi, overlapped, cus, gemm_tile=0, gemm_debug=0):
    """gemm_choose_tile: Tuning.gemm_tile if set, else the measured rule (no per-shape hook here)"""
    cfg = gemm_tile
    if cfg == 0:
        cfg = 1
        bf16_out = epi != EPI_F32
        half_ok = not (gemm_debug & 1024) and N >= 384 and N % 256 == 128
        if K >= (256 if (bf16_out and not (gemm_debug & 512)) else 512) and M >= 512 and (N >= 1024 or (N >= 512 and N % 256 == 0) or half_ok):
            tiles_m, tiles_n = (M + 255) // 256, (N + 255) // 256
            tiles = tiles_m * (tiles_n - 1) + (tiles_m * 3 + 4) // 5 if (half_ok and N % 256 == 128) else tiles_m * tiles_n
            if tiles < cus:
                long_or_direct = bf16_out or K >= 1024
                cfg = 4 if (tiles * 2 >= cus or (overlapped and long_or_direct and tiles * 5 >= cus * 2)) else 1
            elif overlapped and not (gemm_debug & 128):
                cfg = 4
            else:
                last = tiles % cus
                full_enough = last * 2 >= cus if (bf16_out or K >= 1024) else last * 5 >= cus * 4
                if last == 0 or full_enough:
                    cfg = 4
                elif half_ok and N < 512:
                    cfg = 1 if tiles < 2 * cus else 4
                elif K >= 1024 or N >= 1024:
                    cfg = 6
    return cfg


def mixed_split(M, N, cus, m_offset=0):
    """gemm_mixed_split: ((m_offset, M) of the 8-phase rows, (m_offset, M) of the rest), or None if the shape has no whole round"""
    tiles_n, tiles_m = (N + 255) // 256, (M + 255) // 256
    rounds = (tiles_m * tiles_n) // cus
    big_rows = min(tiles_m - 1, rounds * cus // tiles_n)
    if rounds < 1 or big_rows < 1:
        return None
    return (m_offset, big_rows * 256), (m_offset + big_rows * 256, M - big_rows * 256)


def deep_tile_rows(M, N, cus, gemm_debug=0):
    tiles128 = ((M + 127) // 128) * ((N + 127) // 128)
    return 64 if (tiles128 * 2 <= cus and M > 64 and not (gemm_debug & 256)) else 128


def splitk_parts(M, N, K, planes, cus, gemm_debug=0):
    if gemm_debug & (4 | 32):
        return 1
    tiles128 = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles128 > cus:
        return 1
    bm = deep_tile_rows(M, N, cus, gemm_debug)
    tiles = ((M + bm - 1) // bm) * ((N + 127) // 128)
    nk_all = K // (64 // planes)
    sk = min(cus // tiles, nk_all // 12, 8)
    return sk if sk >= 3 else 1


def launch_cfg(m_offset, M, N, K, planes, cfg, cus, gemm_debug):
    """launch_gemm_cfg: (m_offset, M, kernel, split-K parts) of one launch on tile configuration 1 or 4"""
    assert cfg in (1, 4)
    if cfg == 4:
        return (m_offset, M, KERNEL_8PHASE, 1)
    tiles128 = ((M + 127) // 128) * ((N + 127) // 128)
    deep = not (gemm_debug & 4) and tiles128 <= cus
    splitk = 1
    if deep and not (gemm_debug & 32):
        sk = splitk_parts(M, N, K, planes, cus, gemm_debug)
        if sk >= 3:
            splitk = sk
    if deep:
        return (m_offset, M, KERNEL_DEEP64 if deep_tile_rows(M, N, cus, gemm_debug) == 64 else KERNEL_DEEP128, splitk)
    return (m_offset, M, KERNEL_128, splitk)


def plan(M, N, K, epi, planes, overlapped, cus, gemm_tile=0, gemm_debug=0, forced_cfg=0):
    """launch_gemm_checked after its argument checks: (cfg, [(m_offset, M, kernel, split-K parts) per launch])"""
    cfg = forced_cfg if forced_cfg > 0 else choose_tile(M, N, K, epi, overlapped, cus, gemm_tile, gemm_debug)
    if cfg == 6:
        split = mixed_split(M, N, cus)
        if split:
            (o0, m0), (o1, m1) = split
            return 6, [launch_cfg(o0, m0, N, K, planes, 4, cus, gemm_debug), launch_cfg(o1, m1, N, K, planes, 1, cus, gemm_debug)]
        cfg = 1
    return cfg, [launch_cfg(0, M, N, K, planes, cfg, cus, gemm_debug)]
