"""The consumers of RAFT's feature maps addressed by frame slot (include/cwm_hip_dev.h cwm_dev_raft_*_slots; csrc/raft_kernels.hip corr_kernel,
fmap_pool_kernel, corr_lookup_on_the_fly_kernel, cnet_split_kernel) against the existing launches on inputs replicated per pair: only the addressing
differs, so the results are bit for bit equal.  Compact inputs carry one frame more than any slot reaches, filled with NaN; every buffer a kernel
writes lies between guard regions that must stay as they were.  2 rows x 3 pairs on 1/8 grids of 16 x 16, 16 x 20 and the odd 17 x 19."""
import ctypes as C

import pytest
import torch

from counterfactualworldmodels_amd import _lib

from gpu_utils import stream

pytestmark = pytest.mark.gpu
B, PPG = 2, 3
P = B * PPG
GRIDS = ((16, 16), (16, 20), (17, 19))
GUARD, SENTINEL = 4096, 12345.0
# name -> (frames of buffer 1, (s1b, s1t), offset of fmap1, frames of buffer 2 (0: image2 lives in buffer 1), (s2b, s2t), offset of fmap2), in frames
PATTERNS = {
    "P1_first": (2, (1, 0), 0, 6, (3, 1), 0),
    "P1_second": (6, (3, 1), 0, 2, (1, 0), 0),
    "P2_first": (3, (0, 1), 0, 6, (3, 1), 0),
    "P2_second_P1_first": (2, (1, 0), 0, 3, (0, 1), 0),
    "P3_forward": (8, (4, 1), 0, 0, (4, 1), 1),
    "P3_backward": (8, (4, 1), 1, 0, (4, 1), 0),
    "P3_repeated": (6, (3, 1), 0, 0, (3, 1), 0),
}


def dev_lib():
    return _lib.get_dev_lib()


def slots(sb, st, off=0):
    return [off + (p // PPG) * sb + (p % PPG) * st for p in range(P)]


def guarded(*shape):
    """(whole buffer, the view between the guards), everything set to the sentinel"""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(*shape)


def guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all() and (whole[-GUARD:] == SENTINEL).all())


def compact(n_frames, rows, width, seed):
    """[n_frames + 1, rows, width]: random frames and one more, never addressed, of NaN"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_frames + 1, rows, width, generator=g)
    x[n_frames] = float("nan")
    return x.cuda()


def operands(name, h8, w8, seed):
    """(fmap1 pointer tensor, fmap2 pointer tensor, replicated fmap1, replicated fmap2) for a pattern: the pointer tensors are views into the compact buffers"""
    n1, s1, o1, n2, s2, o2 = PATTERNS[name]
    buf1 = compact(n1, h8 * w8, 256, seed)
    buf2 = compact(n2, h8 * w8, 256, seed + 1) if n2 else buf1
    assert max(slots(*s1, o1)) < n1 and max(slots(*s2, o2)) < (n2 or n1)  # every slot lies inside its buffer, before the NaN frame
    rep1 = buf1[slots(*s1, o1)].contiguous()
    rep2 = buf2[slots(*s2, o2)].contiguous()
    assert torch.isfinite(rep1).all() and torch.isfinite(rep2).all()
    return buf1[o1:], buf2[o2:], rep1, rep2


def coordinates(h8, w8, seed):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h8, dtype=torch.float32), torch.arange(w8, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys], -1)[None].expand(P, -1, -1, -1)
    return (grid + 12.0 * torch.rand(P, h8, w8, 2, generator=g) - 6.0).contiguous().cuda()  # some samples leave the map: the zero padding is exercised


@pytest.mark.parametrize("h8,w8", GRIDS)
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_all_pairs_correlation_and_lookup_by_slot(name, h8, w8):
    d = dev_lib()
    f1, f2, rep1, rep2 = operands(name, h8, w8, 100)
    (s1b, s1t), (s2b, s2t) = PATTERNS[name][1], PATTERNS[name][4]
    coords = coordinates(h8, w8, 7)
    want_whole, want = guarded(P, h8, w8, 324)
    _lib.check(d.cwm_raft_corr_lookup(rep1.data_ptr(), rep2.data_ptr(), coords.data_ptr(), P, h8, w8, want.data_ptr(), stream()), d)
    got_whole, got = guarded(P, h8, w8, 324)
    _lib.check(d.cwm_dev_raft_corr_lookup_slots(f1.data_ptr(), f2.data_ptr(), coords.data_ptr(), P, PPG, h8, w8, s1b, s1t, s2b, s2t, got.data_ptr(), stream()), d)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, want) and got.abs().max() > 0
    assert guards_intact(got_whole) and guards_intact(want_whole)


@pytest.mark.parametrize("h8,w8", GRIDS)
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_pooled_levels_and_on_the_fly_lookup_by_slot(name, h8, w8):
    d = dev_lib()
    f1, f2, rep1, rep2 = operands(name, h8, w8, 200)
    (s1b, s1t), (s2b, s2t) = PATTERNS[name][1], PATTERNS[name][4]
    coords = coordinates(h8, w8, 8)
    want_whole, want = guarded(P, h8, w8, 324)
    _lib.check(d.cwm_raft_corr_lookup_on_the_fly(rep1.data_ptr(), rep2.data_ptr(), coords.data_ptr(), P, h8, w8, want.data_ptr(), stream()), d)
    # every distinct second image is pooled once: image2's own frames (rows that share it: one; pairs that share it: one per row)
    nb2, nt2 = (B if s2b else 1), (PPG if s2t else 1)
    n2 = nb2 * nt2
    s2pb, s2pt = (nt2 if nb2 > 1 else 0), (1 if nt2 > 1 else 0)
    levels, wholes = [f2], []
    for l in range(1, 4):
        h, w = h8 >> (l - 1), w8 >> (l - 1)
        whole, lvl = guarded(n2, (h // 2) * (w // 2), 256)
        first = l == 1  # level 1 reads the encoder's frame order, the later ones the compact level before them
        _lib.check(d.cwm_dev_raft_fmap_pool_slots(levels[-1].data_ptr(), n2, nt2 if first else 1, s2b if first else 1, s2t if first else 0, h, w, 256,
                                                  lvl.data_ptr(), stream()), d)
        levels.append(lvl)
        wholes.append(whole)
    got_whole, got = guarded(P, h8, w8, 324)
    ptrs = (C.c_void_p * 4)(*[t.data_ptr() for t in levels])
    _lib.check(d.cwm_dev_raft_corr_lookup_on_the_fly_slots(f1.data_ptr(), ptrs, coords.data_ptr(), P, PPG, h8, w8, s1b, s1t, s2b, s2t, s2pb, s2pt, got.data_ptr(),
                                                           stream()), d)
    torch.cuda.synchronize()
    assert all(torch.isfinite(lvl).all() for lvl in levels[1:]) and all(guards_intact(w_) for w_ in wholes)
    # the pooled maps are those of the replicated input's distinct frames
    pair_of_frame = {s: p for p, s in reversed(list(enumerate(slots(s2pb, s2pt))))}
    level1 = torch.nn.functional.avg_pool2d(rep2.view(P, h8, w8, 256).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    for j in range(n2):
        assert torch.allclose(levels[1][j].view(h8 // 2, w8 // 2, 256), level1[pair_of_frame[j]], rtol=0, atol=1e-6), j
    assert torch.isfinite(got).all() and torch.equal(got, want) and got.abs().max() > 0
    assert guards_intact(got_whole) and guards_intact(want_whole)


@pytest.mark.parametrize("h8,w8", GRIDS)
@pytest.mark.parametrize("name,sb,st,n", [("P1", 1, 0, 2), ("P2", 0, 1, 3), ("P1_and_P2", 0, 0, 1), ("P3", 3, 1, 6)])
def test_context_split_by_slot(name, sb, st, n, h8, w8):
    d = dev_lib()
    hw8 = h8 * w8
    M = P * hw8
    cn = compact(n, hw8, 256, 300)
    rep = cn[slots(sb, st)].contiguous()
    outs = {}
    for kind in ("want", "got"):
        h_whole, h = guarded(M, 128)
        x_whole, x = guarded(M, 256)
        if kind == "want":
            _lib.check(d.cwm_dev_raft_cnet_split(rep.data_ptr(), M, h.data_ptr(), x.data_ptr(), stream()), d)
        else:
            _lib.check(d.cwm_dev_raft_cnet_split_slots(cn.data_ptr(), M, hw8, PPG, sb, st, h.data_ptr(), x.data_ptr(), stream()), d)
        torch.cuda.synchronize()
        assert guards_intact(h_whole) and guards_intact(x_whole)
        assert bool((x[:, 128:] == SENTINEL).all())  # the motion features' half of x is not this kernel's
        outs[kind] = (h, x)
    (h0, x0), (h1, x1) = outs["want"], outs["got"]
    assert torch.isfinite(h1).all() and torch.isfinite(x1).all() and torch.equal(h1, h0) and torch.equal(x1, x0)
    assert torch.equal(h1, torch.tanh(rep.view(M, 256)[:, :128])) or torch.allclose(h1, torch.tanh(rep.view(M, 256)[:, :128]), atol=1e-6)
    assert torch.equal(x1[:, :128], torch.relu(rep.view(M, 256)[:, 128:]))


def test_slot_entry_points_refuse_bad_arguments():
    d = dev_lib()
    t = torch.zeros(16, device="cuda")
    p = t.data_ptr()
    assert d.cwm_dev_raft_corr_lookup_slots(p, p, p, 6, 4, 16, 16, 1, 0, 3, 1, p, stream()) != 0   # 6 pairs are not rows of 4
    assert d.cwm_dev_raft_corr_lookup_slots(p, p, p, 6, 3, 16, 16, -1, 0, 3, 1, p, stream()) != 0  # a negative stride
    assert d.cwm_dev_raft_fmap_pool_slots(p, 0, 1, 1, 0, 16, 16, 256, p, stream()) != 0
    assert d.cwm_dev_raft_cnet_split_slots(p, 7, 2, 1, 1, 0, p, p, stream()) != 0                   # 7 rows are not whole maps of 2
    ptrs = (C.c_void_p * 4)(p, p, p, None)
    assert d.cwm_dev_raft_corr_lookup_on_the_fly_slots(p, ptrs, p, 6, 3, 16, 16, 1, 0, 3, 1, 3, 1, p, stream()) != 0 and b"level 3" in d.cwm_last_error()
