"""`FlowGenerator.track_scene` on a real MI355X against the loop composed by hand from `G.segment_scene`, the stub's flows and the NumPy restatement of the link
step (tests/segment_track_restatement.py): the tiny predictor of tests/test_spelke_segment_gpu.py and the two-object table of tests/test_segment_merge_cpu.py.
The stub flow model here answers `backward=True` with a given integer frame motion per pair (stored as the package's RAFT stores backward pairs: pair t at index
T-2-t); otherwise it answers from the table of the frame being segmented -- the two objects moved by the motion so far, the part that leaves the image cut
off -- and it can blank object B for chosen frames."""
import numpy as np
import pytest
import torch

import segment_track_restatement as TR
from counterfactualworldmodels_amd import segmentation, synthetic as S
from test_segment_cpu import TINY
from test_segment_merge_cpu import S_ as NS, two_object_table
from test_spelke_segment_gpu import predictor

pytestmark = pytest.mark.gpu
KW = dict(num_iters=2, num_samples=NS, k_active=2, k_passive=2, min_seed_mag=1.0, abs_thresh=1.0)
B, T, H, W = 2, 5, 32, 32
MOTION = ((0, 1), (1, 1), (0, 1), (1, 0))  # (dy, dx) of the content from frame t to frame t + 1
SEEDS = [[[4, 4], [20, 28], [12, 12], [28, 4]], [[28, 28], [28, 4], [4, 12], [4, 8]]]  # row 0: A, B, A, nothing; row 1: B, nothing, A, A


def moved(m, dy, dx):
    """m [..., H, W] moved down by dy and right by dx (both >= 0); what leaves the image is cut off"""
    out = np.zeros_like(m)
    out[..., dy:, dx:] = m[..., :m.shape[-2] - dy, :m.shape[-1] - dx]
    return out


class MovieFlow(torch.nn.Module):
    """the stub flow model; `frame` is the frame whose pair the counterfactual flows are asked for"""

    def __init__(self, blank=()):
        super().__init__()
        a, b, table = two_object_table()
        self.a, self.b, self.frame, self.back_calls, self.blank = a, b, 0, 0, set(blank)
        self.tables, self.where = [], []
        dy = dx = 0
        for t in range(T):
            tab = table[0] * (~b if t in self.blank else np.ones_like(b))[None, :, :, None]  # [2,H,W,S]
            self.tables.append(torch.from_numpy(moved(tab.transpose(3, 0, 1, 2), dy, dx)).contiguous().cuda())  # [S,2,H,W]
            self.where.append((moved(a, dy, dx), moved(b, dy, dx)))
            if t < T - 1:
                dy, dx = dy + MOTION[t][0], dx + MOTION[t][1]

    def forward(self, video, backward=False, **kw):
        R = video.shape[0]
        if not backward:
            table = self.tables[self.frame]
            return table.repeat(R // table.shape[0], 1, 1, 1)[:, None]
        self.back_calls += 1
        assert video.shape[1] == T
        f = torch.zeros((R, T - 1, 2, H, W), device=video.device)
        for t, (dy, dx) in enumerate(MOTION):  # the pair (x[t+1], x[t]) on frame t+1's grid looks back by the motion
            f[:, T - 2 - t, 0], f[:, T - 2 - t, 1] = -dx, -dy
        return f


def back_flows():
    f = np.zeros((B, T, 2, H, W), np.float32)
    for t, (dy, dx) in enumerate(MOTION):
        f[:, t + 1, 0], f[:, t + 1, 1] = -dx, -dy
    return f


def generator(blank=()):
    flow = MovieFlow(blank)
    G = segmentation.FlowGenerator(predictor=predictor(TINY), flow_model=flow, imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
    pair = torch.from_numpy(S.synthetic_frames(B, TINY, 3))
    return G, flow, torch.cat([pair, pair, pair[:, :1]], 1).cuda()  # [B,5,C,H,W]; the stub does not look at the pixels


def tracked(G, flow, x, segment_every, **kw):
    """G.track_scene with the stub told which frame every `segment_scene` call is for (the calls come in ascending t)"""
    calls = []
    inner = G.segment_scene

    def segment_scene(xx, **skw):
        flow.frame = len(calls) * segment_every
        calls.append(flow.frame)
        return inner(xx, **skw)

    G.segment_scene = segment_scene
    try:
        out = G.track_scene(x, segment_every=segment_every, seeds=torch.tensor(SEEDS, device="cuda"), num_seeds=4, **kw, **KW)
    finally:
        del G.segment_scene
    assert calls == [t for t in range(T - 1) if t % segment_every == 0]
    return out


def by_hand(G, flow, x, segment_every, **kw):
    """the loop: `segment_scene` of every segmented frame's pair, then the restatement's link step frame by frame on the stub's backward flows"""
    maps = []
    for t in range(T):
        flow.frame = t
        seg = t <= T - 2 and t % segment_every == 0
        maps.append(G.segment_scene(x[:, t:t + 2], seeds=torch.tensor(SEEDS, device="cuda"), num_seeds=4, **KW).labels.cpu().numpy() if seg else None)
    return TR.sequence(maps, back_flows(), (B, H, W), **kw), maps


def compare(out, want):
    assert out.labels.is_cuda and out.labels.dtype == torch.uint8 and tuple(out.labels.shape) == (B, T, H, W)
    for t in range(T):
        for k, name in (("out", "labels"), ("track_id", "track_id"), ("age", "age"), ("stats", "stats"), ("area", "area"), ("bbox", "bbox"), ("moments", "moments")):
            assert np.array_equal(getattr(out, name)[:, t].cpu().numpy(), want[t][k]), (t, name)


def slot_at(labels, t, mask):
    """the one slot that covers `mask` in frame t of every row"""
    slots = [np.unique(labels[r, t][mask]) for r in range(B)]
    assert all(len(s) == 1 and s[0] > 0 for s in slots), slots
    return [int(s[0]) for s in slots]


def test_ids_persist_and_a_blanked_object_coasts_ends_and_returns():
    G, flow, x = generator(blank=(1, 2))
    torch.manual_seed(13)
    state = torch.get_rng_state()
    out = tracked(G, flow, x, 1, max_age=1)
    assert torch.equal(torch.get_rng_state(), state), "the caller's global CPU RNG state"
    assert flow.back_calls == 1, "one backward flow call per movie"
    want, _ = by_hand(G, flow, x, 1, max_age=1)
    assert flow.back_calls == 1
    compare(out, want)
    labels, ids, age = out.labels.cpu().numpy(), out.track_id.cpu().numpy(), out.age.cpu().numpy()
    a0, b0 = slot_at(labels, 0, flow.where[0][0]), slot_at(labels, 0, flow.where[0][1])
    for r in range(B):
        ida, idb = ids[r, 0, a0[r] - 1], ids[r, 0, b0[r] - 1]
        assert sorted((ida, idb)) == [1, 2]
        for t in range(T):  # A is found in every segmented frame and carried into the last one: one slot, one id, where the object has moved to
            assert slot_at(labels, t, flow.where[t][0])[r] == a0[r] and ids[r, t, a0[r] - 1] == ida and age[r, t, a0[r] - 1] == (1 if t == T - 1 else 0)
        # B is blanked in frames 1 and 2: it coasts for max_age = 1 frame, ends, and comes back in frame 3 under a NEW id
        assert slot_at(labels, 1, flow.where[1][1])[r] == b0[r] and ids[r, 1, b0[r] - 1] == idb and age[r, 1, b0[r] - 1] == 1
        assert not labels[r, 2][flow.where[2][1]].any() and idb not in ids[r, 2]
        b3 = slot_at(labels, 3, flow.where[3][1])[r]
        assert ids[r, 3, b3 - 1] == 3 and out.stats[r, 3].tolist()[:4] == [1, 1, 0, 0] and out.stats[r, 2].tolist()[:4] == [1, 0, 0, 1]
    torch.set_rng_state(state)


def test_segment_every_two_carries_frames_by_the_flow_alone():
    G, flow, x = generator()
    out = tracked(G, flow, x, 2, max_age=2, return_segmentations=True)
    assert flow.back_calls == 1 and [s is not None for s in out.segmentations] == [True, False, True, False, False]
    want, maps = by_hand(G, flow, x, 2, max_age=2)
    compare(out, want)
    labels, ids = out.labels.cpu().numpy(), out.track_id.cpu().numpy()
    assert np.array_equal(out.segmentations[2].labels.cpu().numpy(), maps[2])
    for t in (1, 3, 4):  # a carried frame is the frame before it moved by the motion: pure propagation, no births, no links
        assert np.array_equal(labels[:, t], moved(labels[:, t - 1], *MOTION[t - 1])) and labels[:, t].any()
        assert out.stats[:, t, :2].tolist() == [[0, 0]] * B and np.array_equal(ids[:, t], ids[:, t - 1])
    assert np.array_equal(ids[:, 2], ids[:, 0]) and out.stats[:, 2, 0].tolist() == [2, 2]  # frame 2 is segmented again and linked to the carried tracks


def test_track_scene_refuses_what_would_let_tracks_die():
    G, flow, x = generator()
    with pytest.raises(ValueError, match="max_age"):
        G.track_scene(x, segment_every=3, max_age=2)
    with pytest.raises(ValueError, match="carry"):
        G.track_scene(x, segment_every=2, carry=False)
    assert flow.back_calls == 0
