"""RAFT's shared frames, the host side (no GPU): the frame plan of a forward (`cwm_dev_raft_frame_slots`: which images of a call are one frame, read
off the two image sources' strides) over a table of calls, the two new entry points in the header, the map and the bindings, and the generator's
routing of counterfactual videos through `RAFT.flow_pairs` with a stub flow model that records its call."""
import ctypes as C
import os
import re

import pytest
import torch

from counterfactualworldmodels_amd import _lib, raft

from test_motion_sampling_cpu import tiny_generator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 128, 160
IMG = 3 * H * W            # floats of one contiguous frame
BASE1, BASE2 = 1 << 30, 1 << 34  # two buffers far apart (addresses only: the plan reads nothing through them)
F = 4                      # bytes per float


def call(batch, pairs, src1, src2):
    """src: (address, stride_b, stride_t, stride_c) in floats"""
    a = _lib.new_raft_forward_args()
    a.image1_dev, a.image1_stride_b, a.image1_stride_t, a.image1_stride_c = src1
    a.image2_dev, a.image2_stride_b, a.image2_stride_t, a.image2_stride_c = src2
    a.batch, a.pairs, a.height, a.width = batch, pairs, H, W
    return a


def plan(a, share):
    P = a.batch * max(a.pairs, 1)
    s1, s2, cs = (C.c_int * P)(), (C.c_int * P)(), (C.c_int * P)()
    nf, nc = C.c_int(-1), C.c_int(-1)
    d = _lib.get_dev_lib()
    _lib.check(d.cwm_dev_raft_frame_slots(C.byref(a), int(share), s1, s2, cs, C.byref(nf), C.byref(nc)), d)
    return list(s1), list(s2), list(cs), nf.value, nc.value


def images(a):
    """(address, channel stride) of image1 and image2 of every pair, from the strides"""
    ppg = max(a.pairs, 1)
    one, two = [], []
    for b in range(a.batch):
        for t in range(ppg):
            one.append((a.image1_dev + F * (b * a.image1_stride_b + t * a.image1_stride_t), a.image1_stride_c))
            two.append((a.image2_dev + F * (b * a.image2_stride_b + t * a.image2_stride_t), a.image2_stride_c))
    return one, two


def movie(T, batch=2, base=BASE1):
    """x[B,T]: (first, second) = (x[:, :-1], x[:, 1:])"""
    sb, st = T * IMG, IMG
    return (base, sb, st, H * W), (base + F * st, sb, st, H * W)


PLAIN = ((BASE1, 3 * IMG, IMG, H * W), (BASE2, 3 * IMG, IMG, H * W))
# name -> (batch, pairs, image1, image2, a pattern is recognised)
CALLS = {
    "plain": (2, 3, *PLAIN, False),
    "p1_image1": (2, 3, (BASE1, IMG, 0, H * W), PLAIN[1], True),
    "p1_image2": (2, 3, PLAIN[0], (BASE2, IMG, 0, H * W), True),
    "p2_image1": (2, 3, (BASE1, 0, IMG, H * W), PLAIN[1], True),
    "p2_image2": (3, 1, PLAIN[0], (BASE2, 0, IMG, H * W), True),
    "p1_and_p2": (2, 3, (BASE1, 0, 0, H * W), PLAIN[1], True),
    "p1_both": (2, 3, (BASE1, IMG, 0, H * W), (BASE2, IMG, 0, H * W), True),
    "pairs_0": (3, 0, (BASE1, IMG, 0, H * W), (BASE2, IMG, 0, H * W), False),
    "pairs_0_repeated": (3, 0, (BASE1, IMG, IMG, H * W), (BASE1, IMG, IMG, H * W), True),
    "partial_overlap": (2, 3, (BASE1, 4 * IMG, IMG, H * W), (BASE1 + F * W, 4 * IMG, IMG, H * W), False),
    "channel_strides_differ": (2, 3, (BASE1, 4 * IMG, IMG, H * W), (BASE1 + F * IMG, 4 * IMG, IMG, 2 * H * W), False),
    "negative_stride_t": (2, 3, (BASE1 + F * 3 * IMG, 4 * IMG, -IMG, H * W), (BASE1 + F * 2 * IMG, 4 * IMG, -IMG, H * W), False),
    "negative_stride_b_p1": (2, 3, (BASE1 + F * IMG, -IMG, 0, H * W), PLAIN[1], False),
    "one_pair_per_row_movie": (3, 1, *movie(2, 3), False),
}
for T in (2, 3, 4, 5):
    first, second = movie(T)
    if T > 2:
        CALLS["p3_forward_T%d" % T] = (2, T - 1, first, second, True)
        CALLS["p3_backward_T%d" % T] = (2, T - 1, second, first, True)
    CALLS["p3_repeated_T%d" % T] = (2, T - 1, first, first, True)
CALLS["p3_forward_p2_T4"] = (2, 3, (BASE1, 0, IMG, H * W), (BASE1 + F * IMG, 0, IMG, H * W), True)


def check_slots(slots, n):
    assert sorted(set(slots)) == list(range(n)), (slots, n)  # the slots fill [0, n)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_frame_slots_merge_exactly_the_equal_images_of_a_recognised_pattern(name):
    batch, pairs, src1, src2, recognised = CALLS[name]
    a = call(batch, pairs, src1, src2)
    P = batch * max(pairs, 1)
    one, two = images(a)
    for share in (0, 1):
        s1, s2, cs, nf, nc = plan(a, share)
        check_slots(s1 + s2, nf)
        check_slots(cs, nc)
        if share and recognised:
            frames, slots = one + two, s1 + s2
            for i in range(2 * P):
                for j in range(2 * P):
                    assert (slots[i] == slots[j]) == (frames[i] == frames[j]), (name, i, j, slots, frames[i], frames[j])
            assert nf == len(set(frames)) < 2 * P and nc == len(set(one))
        else:
            assert len(set(s1 + s2)) == 2 * P and nf == 2 * P and nc == P, (name, share, s1, s2)
        # the context follows image1: equal context slots <=> equal first images (never merged beyond them)
        for i in range(P):
            for j in range(P):
                assert (cs[i] == cs[j]) == (s1[i] == s1[j]), (name, share, cs, s1)
                assert cs[i] != cs[j] or one[i] == one[j]


def test_the_counts_of_the_patterns():
    want = {"p1_image1": (2 + 6, 2), "p1_image2": (6 + 2, 6), "p2_image1": (3 + 6, 3), "p1_and_p2": (1 + 6, 1), "p1_both": (4, 2), "pairs_0_repeated": (3, 3),
            "p3_forward_T3": (6, 4), "p3_backward_T3": (6, 4), "p3_forward_T5": (10, 8), "p3_repeated_T4": (6, 6), "p3_forward_p2_T4": (4, 3), "p2_image2": (3 + 1, 3)}
    for name, counts in want.items():
        batch, pairs, src1, src2, _ = CALLS[name]
        assert plan(call(batch, pairs, src1, src2), 1)[3:] == counts, name


def test_share_off_is_the_pair_order_of_every_call():
    for name, (batch, pairs, src1, src2, _) in CALLS.items():
        P = batch * max(pairs, 1)
        s1, s2, cs, nf, nc = plan(call(batch, pairs, src1, src2), 0)
        assert s1 == list(range(P)) and s2 == list(range(P, 2 * P)) and cs == list(range(P)) and (nf, nc) == (2 * P, P), name


def test_frame_slots_refuses_bad_arguments():
    d = _lib.get_dev_lib()
    a = call(2, 3, *PLAIN)
    buf, n = (C.c_int * 6)(), C.c_int()
    assert d.cwm_dev_raft_frame_slots(C.byref(a), 2, buf, buf, buf, C.byref(n), C.byref(n)) != 0 and b"share" in d.cwm_last_error()
    assert d.cwm_dev_raft_frame_slots(C.byref(a), 1, None, buf, buf, C.byref(n), C.byref(n)) != 0
    a.batch = 0
    assert d.cwm_dev_raft_frame_slots(C.byref(a), 1, buf, buf, buf, C.byref(n), C.byref(n)) != 0


def test_surface_header_map_and_bindings():
    header = open(os.path.join(ROOT, "include", "cwm_hip.h")).read()
    dev_header = open(os.path.join(ROOT, "include", "cwm_hip_dev.h")).read()
    for name in ("cwm_raft_set_share_frames", "cwm_raft_encoder_images"):
        assert re.search(r"CWM_API int %s\(" % name, header) and name in _lib.SIGNATURES and hasattr(_lib.get_lib(), name), name
        assert "void* stream" not in re.search(r"CWM_API int %s\([^;]*;" % name, header).group(0)  # neither takes a stream
    assert "raft_model.py:276-300" in header and "segmentation.py:431" in header and header.count("added after 0.10.4; the version string is unchanged") >= 2
    assert _lib.get_lib().cwm_version().decode().startswith("cwm_hip 0.10.4")
    exports = open(os.path.join(ROOT, "counterfactualworldmodels_amd", "csrc", "exports.map")).read()
    assert "cwm_*" in exports  # the map exports the prefix: the two names are in it
    for name in ("cwm_dev_raft_frame_slots", "cwm_dev_raft_corr_lookup_slots", "cwm_dev_raft_fmap_pool_slots", "cwm_dev_raft_corr_lookup_on_the_fly_slots",
                 "cwm_dev_raft_cnet_split_slots"):
        assert name in dev_header and name in _lib.DEV_SIGNATURES and name not in _lib.SIGNATURES, name
        assert not hasattr(C.CDLL(_lib.library_path()), name)
    # a null handle is refused, not dereferenced (a handle needs a device: the refusal of on = 2 and the (0, 0) before a forward are in the GPU file)
    lib = _lib.get_lib()
    n = C.c_int()
    assert lib.cwm_raft_set_share_frames(None, 1) != 0 and lib.cwm_raft_encoder_images(None, C.byref(n), C.byref(n)) != 0


def test_raft_module_surface():
    m = raft.RAFT()
    assert m.share_frames is False and m.last_encoder_images == (0, 0)
    assert m.set_share_frames(True) is m and m.share_frames is True and m.set_share_frames(False).share_frames is False
    assert raft.RAFT(raft._args(share_frames=True)).share_frames is True
    assert {"set_share_frames", "encoder_images"} <= set(m._ABI) and m._ABI["encoder_images"] == "cwm_raft_encoder_images"
    with pytest.raises(RuntimeError, match="one shape"):
        m.flow_pairs(torch.zeros(1, 2, 3, 128, 128), torch.zeros(1, 3, 3, 128, 128))
    with pytest.raises(RuntimeError):  # no CPU fallback
        m.flow_pairs(torch.zeros(1, 2, 3, 128, 128), torch.zeros(1, 2, 3, 128, 128))


# ---- the generator's routing --------------------------------------------------------------------------------------------------------------------
class StubFlow:
    """Records its calls; returns flows that name the route"""

    def __init__(self, pairs=True):
        self.calls = []
        if pairs:
            self.flow_pairs = self._flow_pairs

    def __call__(self, video, backward=False, **kw):
        self.calls.append(("forward", video, backward, kw))
        return torch.zeros(video.shape[0], video.shape[1] - 1, 2, *video.shape[-2:])

    def _flow_pairs(self, first, second, iters=24, flow_init=None, backward=False, share=None):
        self.calls.append(("flow_pairs", first, second, backward, share))
        return torch.ones(first.shape[0], first.shape[1], 2, *first.shape[-2:])


def routed(share=True, pairs=True, frame=1, T=2, mask_frame0=False, backward=False, B=2, S=3):
    flow = StubFlow(pairs)
    G = tiny_generator(flow_model=flow, share_static_frame=share) if share is not None else tiny_generator(flow_model=flow)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 2, 3, 32, 32, generator=g)
    G.set_input(x)
    G.inp_shape = x.shape
    y = torch.rand(B * S, T, 3, 32, 32, generator=g)
    Nt = 2 * 4 * 4
    mask = torch.zeros(B * S, Nt, dtype=torch.bool)
    mask[:, Nt // 2:] = True  # frame 1 is predicted
    if mask_frame0:
        mask[B * S - 1, 3] = True  # one token of frame 0, in the last row only
    flows = G._counterfactual_flows(y, mask, frame, backward=backward)
    return G, flow, x, y, flows


@pytest.mark.parametrize("backward", [False, True])
def test_generator_hands_the_shared_frame_to_flow_pairs(backward):
    G, flow, x, y, flows = routed(backward=backward)
    assert G.share_static_frame is True and len(flow.calls) == 1
    kind, first, second, bw, share = flow.calls[0]
    assert kind == "flow_pairs" and bw is backward and share is True
    assert tuple(first.shape) == tuple(second.shape) == (2, 3, 3, 32, 32)
    assert first.stride(1) == 0 and first.data_ptr() == x.data_ptr() and first.stride(0) == x.stride(0)  # frame 0 of the input, expanded over S: no copy
    assert torch.equal(first[:, 1], x[:, 0]) and torch.equal(second.reshape(6, 3, 32, 32), y[:, 1])
    assert tuple(flows.shape) == (6, 1, 2, 32, 32) and bool((flows == 1).all())


@pytest.mark.parametrize("why,kw", [("a frame-0 token is masked", dict(mask_frame0=True)), ("frame != 1", dict(frame=0)), ("three frames", dict(T=3)),
                                    ("the model lacks flow_pairs", dict(pairs=False)), ("the flag is off", dict(share=False)),
                                    ("the default is off", dict(share=None))])
def test_generator_falls_back_to_the_video_call(why, kw):
    G, flow, x, y, flows = routed(**kw)
    assert [c[0] for c in flow.calls] == ["forward"], why
    assert flow.calls[0][1] is y and flow.calls[0][2] is False
    assert tuple(flows.shape) == (6, y.shape[1] - 1, 2, 32, 32) and bool((flows == 0).all())
    assert G.share_static_frame is bool(kw.get("share", True))
