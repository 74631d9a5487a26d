"""`FlowGenerator.track_scene(occlusion=True)` on a real MI355X against the loop composed by hand from the NumPy restatements of the consistency check
(tests/flow_consistency_restatement.py) and of the link step (tests/segment_track_restatement.py), with a stub flow model and given segmentations, as
tests/test_track_scene_gpu.py stubs them.

The scene, 64 x 64 and four frames: a rectangle moves 3 px per frame over a static background (to the right in row 0 of the batch, downwards in row 1).
`segment_every = 2`: frames 0 and 2 are segmented (the rectangle is label 1), frames 1 and 3 are carried by the flow alone.  The strip the rectangle uncovers
has no true backward flow.  The stub answers 0 there, as for the background around it, so the warp finds the OBJECT's slot at the same place in the previous
frame: without the check a carried frame paints the strip as object (the smear).  (Extending the object's own backward motion, -3, over the strip instead would
make the strip look at the background 3 px behind the object's old position, which carries no slot: nothing would be painted and there would be nothing to
repair.)  The stub's forward flow moves the object's pixels by +3 and the background by 0, so the strip's round trip ends 3 px off and fails the check."""
import numpy as np
import pytest
import torch

import flow_consistency_restatement as R
import segment_track_restatement as TR
from counterfactualworldmodels_amd import config as C, segment_merge, segmentation, synthetic as S
from test_spelke_segment_gpu import predictor

pytestmark = pytest.mark.gpu
CFG = C.VmaeConfig(name="tiny64_8x8", img_size=(64, 64), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
B, T, H, W, STEP = 2, 4, 64, 64, 3
FIELDS = (("out", "labels"), ("track_id", "track_id"), ("age", "age"), ("stats", "stats"), ("area", "area"), ("bbox", "bbox"), ("moments", "moments"))


def where(t):
    """bool [B,H,W]: the rectangle in frame t"""
    m = np.zeros((B, H, W), bool)
    m[0, 20:40, 10 + STEP * t:30 + STEP * t] = True
    m[1, 8 + STEP * t:28 + STEP * t, 30:50] = True
    return m


def pair_flows():
    """back, fwd [B,T,2,H,W]: back[:, t] from frame t to frame t-1 on frame t's grid, fwd[:, t] from frame t-1 to frame t on frame t-1's grid; entry 0 zeros"""
    back, fwd = np.zeros((B, T, 2, H, W), np.float32), np.zeros((B, T, 2, H, W), np.float32)
    for t in range(1, T):
        for b, ch in ((0, 0), (1, 1)):
            back[b, t, ch] = np.where(where(t)[b], -STEP, 0)
            fwd[b, t, ch] = np.where(where(t - 1)[b], STEP, 0)
    return back, fwd


class MovieFlow(torch.nn.Module):
    """the stub flow model: [B,T-1,2,H,W], a backward call stored as the package's RAFT stores it (pair t at index T-2-t)"""

    def __init__(self):
        super().__init__()
        self.calls = []
        back, fwd = pair_flows()
        self.back, self.fwd = torch.from_numpy(back[:, 1:]).cuda().flip(1), torch.from_numpy(fwd[:, 1:]).cuda()

    def forward(self, video, backward=False, **kw):
        assert tuple(video.shape[:2]) == (B, T)
        self.calls.append("backward" if backward else "forward")
        return (self.back if backward else self.fwd).clone()


def generator():
    flow = MovieFlow()
    G = segmentation.FlowGenerator(predictor=predictor(CFG), flow_model=flow, imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
    pair = torch.from_numpy(S.synthetic_frames(B, CFG, 3))
    return G, flow, torch.cat([pair, pair], 1).cuda()  # [B,4,C,H,W]; the stub does not look at the pixels


def tracked(G, x, **kw):
    """G.track_scene with the segmentations given: the rectangle of the frame as label 1 (the calls come in ascending t: frames 0 and 2)"""
    frames = []

    def segment_scene(xx, **skw):
        t = 2 * len(frames)
        frames.append(t)
        return segment_merge.SceneSegmentation(labels=torch.from_numpy(where(t).astype(np.uint8)).cuda())

    G.segment_scene = segment_scene
    try:
        out = G.track_scene(x, segment_every=2, max_age=2, **kw)
    finally:
        del G.segment_scene
    assert frames == [0, 2]
    return out


def by_hand(occlusion):
    back, fwd = pair_flows()
    res, state, prev = [], None, None
    for t in range(T):
        cur = where(t).astype(np.uint8) if t in (0, 2) else None
        flow = None if t == 0 else R.one_direction(back[:, t], fwd[:, t], 0.01, 0.5)["masked"] if occlusion else back[:, t]
        res.append(TR.track(prev, cur, flow, state, (B, H, W), max_age=2))
        state, prev = TR.new_state(res[-1]), res[-1]["out"]
    return res


def compare(out, want):
    assert out.labels.is_cuda and out.labels.dtype == torch.uint8 and tuple(out.labels.shape) == (B, T, H, W)
    for t in range(T):
        for k, name in FIELDS:
            assert np.array_equal(getattr(out, name)[:, t].cpu().numpy(), want[t][k]), (t, name)


def test_occlusion_keeps_the_uncovered_strip_out_of_carried_frames():
    G, flow, x = generator()
    torch.manual_seed(13)
    state = torch.get_rng_state()
    out = tracked(G, x, occlusion=True)
    assert torch.equal(torch.get_rng_state(), state), "the caller's global CPU RNG state"
    assert sorted(flow.calls) == ["backward", "forward"], "the flow model is called exactly twice"
    compare(out, by_hand(True))
    labels = out.labels.cpu().numpy()
    for t in (1, 3):
        strip = where(t - 1) & ~where(t)
        assert strip.reshape(B, -1).sum(1).tolist() == [20 * STEP] * B and not labels[:, t][strip].any(), "the carried frame's strip is 0"
        assert (labels[:, t][where(t)] == labels[:, 0][where(0)][0]).all(), "the object itself is carried"
    assert out.track_id[:, :, 0].tolist() == [[1] * T] * B and out.stats[:, 2, 0].tolist() == [1] * B  # one track, linked again in frame 2


def test_predict_flow_and_occlusion_checks_both_directions_in_pair_order():
    G, flow, x = generator()
    fwd, bwd, occ_fwd, occ_bwd, fc = G.predict_flow_and_occlusion(x)
    assert flow.calls == ["forward", "backward"], "one flow call per direction"
    back, forw = pair_flows()
    assert np.array_equal(fwd.cpu().numpy(), forw[:, 1:]) and np.array_equal(bwd.cpu().numpy(), back[:, 1:]), "pair t of both at index t"
    a, o = forw[:, 1:].reshape(B * (T - 1), 2, H, W), back[:, 1:].reshape(B * (T - 1), 2, H, W)
    want = R.consistency(a, o, 0.01, 0.5, 0, True)
    for k, name in (("code", "code"), ("res", "res"), ("masked", "masked"), ("stats", "stats")):
        got = getattr(fc, name).cpu().numpy()
        assert got.shape[:3] == (2, B, T - 1) and np.array_equal(R.bits(got.reshape(want[k].shape)), R.bits(want[k])), name
    assert occ_fwd.dtype == torch.bool and torch.equal(occ_fwd, fc.code[0] != 0) and torch.equal(occ_bwd, fc.code[1] != 0)
    for t in range(1, T):  # backward: the uncovered strip is occluded and nothing else; forward: the pixels the object is about to cover
        assert np.array_equal(occ_bwd[:, t - 1].cpu().numpy(), where(t - 1) & ~where(t))
        assert np.array_equal(occ_fwd[:, t - 1].cpu().numpy(), where(t) & ~where(t - 1))


def test_without_occlusion_nothing_changes_and_the_strip_is_painted():
    G, flow, x = generator()
    torch.manual_seed(13)
    state = torch.get_rng_state()
    off = tracked(G, x, occlusion=False)
    assert flow.calls == ["backward"], "the flow model is called once"
    plain = tracked(G, x)
    assert flow.calls == ["backward"] * 2 and torch.equal(torch.get_rng_state(), state)
    for _, name in FIELDS:
        assert torch.equal(getattr(off, name), getattr(plain, name)), name
    compare(plain, by_hand(False))
    labels = plain.labels.cpu().numpy()
    for t in (1, 3):
        strip = where(t - 1) & ~where(t)
        assert labels[:, t][strip].all(), "the carried frame paints the strip as object"
