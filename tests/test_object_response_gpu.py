"""`cwm_object_response` on a real MI355X through the C ABI against the NumPy restatement (tests/object_response_restatement.py), for EQUALITY: the integer tables
by value, the coupling as int64 bit patterns.

Shapes: 8 x 12 with S = 1 and S = 3 (the smallest legal plane, one wave, most lanes past the plane), 24 x 40 with S = 2 (the last workgroup is partial), 64 x 64
with B = 2, K = 3, S = 5 (four workgroups per plane) on random blocks (mixed waves), whole image rows of one slot (one-slot waves), a label change at every pixel
(64-slot waves) and the three-object scene, 512 x 512 once (the limit: sums beyond 2^32).  Flows as the sample-outer view of a [(r s),1,2,H,W] tensor (wide
loads), packed [R,2,H,W,S] and four bytes off their alignment (the scalar form); labels with push stride 0 and as a [:, 1:] slice of a larger buffer.  Then the
Python layers on the device: `measure` against its CPU copy, the driver `FlowGenerator.object_interactions` under a stub flow model against the loop composed by
hand, and one run with the package's RAFT at random weights."""
import ctypes

import numpy as np
import pytest
import torch

import object_response_restatement as R
from counterfactualworldmodels_amd import _lib, object_response as OR

pytestmark = pytest.mark.gpu
FIELD = dict(tab="tab_dev", valid="valid_dev", agg="agg_dev", coupling="coupling_dev", stats="stats_dev")
DTYPE = dict(tab=torch.int64, valid=torch.uint8, agg=torch.int64, coupling=torch.float64, stats=torch.int32)


def dev(a):
    return None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).cuda())


def new_outs(Rr, S, prefill=True):
    shape = dict(tab=(Rr, S, 65, 8), valid=(Rr, S), agg=(Rr, 65, 4), coupling=(Rr, 65, 4), stats=(Rr, 4))
    fill = lambda k: (float("nan") if k == "coupling" else (247 if k == "valid" else -9)) if prefill else 0  # noqa: E731
    return {k: torch.full(shape[k], fill(k), dtype=DTYPE[k], device="cuda") for k in FIELD}


def as_bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def run(flows, labels, pushed, dirs=None, min_mag=1.0, min_pixels=1, self_frac=0.5, move_frac=0.5, expect=0, mutate=None, prefill=True, outs=None):
    """one call: flows [R,2,H,W,S] in whatever strides they have, labels [B,H,W] (push stride 0) or a [B,K,H,W] view.  Returns (dict of CPU arrays, the message)"""
    fl, lab, pu, di = dev(flows), dev(labels), dev(np.asarray(pushed, np.int32) if not torch.is_tensor(pushed) else pushed), dev(dirs)
    Rr, _, H, W, S = fl.shape
    B = lab.shape[0]
    K = Rr // B
    ls = (lab.stride(0), 0) if lab.dim() == 3 else (lab.stride(0), lab.stride(1))
    if outs is None:
        outs = new_outs(Rr, S, prefill)
    before = {k: v.clone() for k, v in outs.items()}
    lib = _lib.get_lib()
    a = _lib.new_object_response_args()
    _lib.fill_patch_args(a.base, geometry=(B, K, 0, H, W, 0), stream=_lib.current_stream_handle(torch.device("cuda:0")))
    a.flows_dev, a.S = fl.data_ptr(), S
    for i in range(5):
        a.flow_strides[i] = fl.stride(i)
    a.labels_dev, a.labels_strides[0], a.labels_strides[1] = lab.data_ptr(), ls[0], ls[1]
    a.pushed_dev, a.dirs_dev = pu.data_ptr(), _lib.ptr(di)
    a.min_q2, a.min_pixels, a.self_frac, a.move_frac = R.min_q2_of(min_mag), min_pixels, self_frac, move_frac
    for k, f in FIELD.items():
        setattr(a, f, outs[k].data_ptr())
    if mutate:
        mutate(a)
    rc = lib.cwm_object_response(ctypes.byref(a))
    torch.cuda.synchronize()
    msg = lib.cwm_last_error().decode()
    assert rc == expect, (rc, msg)
    if expect:
        for k, v in outs.items():
            assert torch.equal(as_bits(v), as_bits(before[k])), "%s written by a refused call" % k
    return {k: v.cpu().numpy() for k, v in outs.items()}, msg


def equal(got, want, what=""):
    for k in R.NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, what, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(R.bits(got[k]), R.bits(want[k])), (k, what, int((R.bits(got[k]) != R.bits(want[k])).sum()))


def sample_outer(flows):
    """the `_batch_to_samples` view of a [(r s),1,2,H,W] device tensor holding flows [R,2,H,W,S]"""
    f = dev(flows)
    Rr, _, H, W, S = f.shape
    out = f.permute(0, 4, 1, 2, 3).contiguous().reshape(Rr * S, 1, 2, H, W)
    v = out[:, 0].reshape(Rr, S, 2, H, W).movedim(1, -1)
    assert v.data_ptr() == out.data_ptr() and v.stride() == (S * 2 * H * W, H * W, W, 1, 2 * H * W)
    return v


def shifted(t, n=1):
    """the same values and strides, the base n elements off"""
    buf = torch.zeros((t.untyped_storage().nbytes() // t.element_size() + n + 4,), dtype=t.dtype, device="cuda")
    flat = torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)
    buf[n:n + flat.numel()] = flat
    return torch.as_strided(buf, t.shape, t.stride(), n + t.storage_offset())


def check(flows, labels, pushed, dirs=None, what="", **kw):
    """the restatement once, then the three flow layouts against it"""
    K = len(pushed) // len(labels)
    want = R.response(flows, R.per_row(labels, K), pushed, dirs, **kw)
    outer = sample_outer(flows)
    off = shifted(outer)
    assert outer.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    for name, f in (("sample-outer", outer), ("packed", dev(flows)), ("off alignment", off)):
        got, _ = run(f, labels, pushed, dirs, **kw)
        equal(got, want, (what, name))
    return want


def test_smallest_plane():
    for S in (1, 3):
        flows, labels, pushed = R.case_random(1, 2, 8, 12, S, seed=11)
        w = check(flows, labels, pushed, R.dirs_of(S), what="8x12 S=%d" % S)
        assert (w["tab"][..., 0] + w["tab"][..., 7]).sum() == 2 * S * 96
        check(flows, labels, pushed, None, what="8x12 no dirs")


def test_partial_last_workgroup():
    flows, labels, pushed = R.case_random(2, 2, 24, 40, 2, seed=12)
    w = check(flows, labels, pushed, R.dirs_of(2), what="24x40")
    assert w["stats"][:, 0].max() > 0
    check(flows, labels, pushed, R.dirs_of(2), min_mag=2.0, min_pixels=6, self_frac=0.2, move_frac=0.9, what="24x40 thresholds")


@pytest.mark.parametrize("case", ["random", "rows", "checker", "scene"])
def test_64_x_64(case):
    B, K, H, W, S = 2, 3, 64, 64, 5
    dirs = R.dirs_of(S)
    if case == "scene":
        flows, labels, pushed, dirs = R.case_scene(B, H, W, S)
    else:
        flows, labels, pushed = getattr(R, "case_" + case)(B, K, H, W, S)
    w = check(flows, labels, pushed, dirs, what=case)
    if case == "random":
        assert (labels > 64).any() and np.isnan(flows).any() and np.isinf(flows).any() and (flows == 4096).any() and w["tab"][..., 7].sum() > 1000
        assert w["stats"][1:4, 0].tolist() == [0, 0, 0] and w["valid"].any() and 0 < w["tab"][..., 1].sum() < w["tab"][..., 0].sum()
    elif case == "checker":
        assert (w["tab"][..., 0] > 0).all()
    elif case == "scene":
        assert w["stats"][:, 0].tolist() == [S - 1] * 6
        c = w["coupling"].reshape(B, K, 65, 4)
        assert c[0, :, :4, 3].tolist() == [[0.0, 1.0, 0.75, 0.0], [0.0, 0.75, 1.0, 0.0], [0.0, 0.0, 0.5, 1.0]]


def test_the_limit_512_x_512():
    H = W = 512
    labels = np.ones((1, H, W), np.uint8)
    labels[0, :, 256:] = 2
    flows = np.empty((1, 2, H, W, 2), np.float32)
    flows[0, 0, :, :, 0], flows[0, 1, :, :, 0] = 4096, -4096
    flows[0, 0, :, :, 1], flows[0, 1, :, :, 1] = 300.5, -0.00390625
    pushed, dirs = np.array([1], np.int32), np.array([[0, 4096], [0, 8]], np.int32)
    want = R.response(flows, labels, pushed, dirs)
    assert want["tab"][0, 0, 1, 6] == 1 << 58 and want["tab"][0, 1, 1, 2] > 1 << 32 and want["agg"][0, 1, 2] == (1 << 49) + 131072 * 76928 * 8
    assert want["stats"][0].tolist() == [2, 1, 131072, 0] and want["coupling"][0, 2, 3] == 1.0
    got, _ = run(sample_outer(flows), labels, pushed, dirs)
    equal(got, want, "512x512")


def test_label_layouts():
    B, K, H, W, S = 2, 3, 24, 40, 2
    flows, labels, pushed = R.case_random(B, K, H, W, S, seed=14)
    want = R.response(flows, R.per_row(labels, K), pushed, R.dirs_of(S))
    per_push = dev(labels)[:, None].expand(B, K, H, W).contiguous()
    big = torch.zeros((B, K + 1, H, W), dtype=torch.uint8, device="cuda")
    big[:, 1:] = per_push
    for name, lab in (("stride 0", dev(labels)), ("[B,K,H,W]", per_push), ("[:, 1:] slice", big[:, 1:]), ("one byte off", shifted(per_push))):
        got, _ = run(sample_outer(flows), lab, pushed, R.dirs_of(S))
        equal(got, want, name)
    other = per_push.clone()
    other[:, 1] = 0
    got, _ = run(sample_outer(flows), other, pushed, R.dirs_of(S))
    equal(got, R.response(flows, other.reshape(B * K, H, W).cpu().numpy(), pushed, R.dirs_of(S)), "a map per push")


def test_the_call_zeroes_its_own_tables_and_two_calls_give_equal_bits():
    flows, labels, pushed = R.case_random(2, 3, 64, 64, 5, seed=9)
    f, dirs = sample_outer(flows), R.dirs_of(5)
    fresh, _ = run(f, labels, pushed, dirs, prefill=False)
    outs = new_outs(6, 5, prefill=True)
    one, _ = run(f, labels, pushed, dirs, outs=outs)
    two, _ = run(f, labels, pushed, dirs, outs=outs)  # (into what the first call left)
    for k in R.NAMES:
        assert np.array_equal(R.bits(one[k]), R.bits(two[k])) and np.array_equal(R.bits(one[k]), R.bits(fresh[k])), k
    equal(one, R.response(flows, R.per_row(labels, 3), pushed, dirs))


def test_limits_are_refused_with_the_field_named():
    flows, labels, pushed = R.case_random(1, 2, 8, 12, 2, seed=1)

    def refused(field, flows=flows, labels=labels, pushed=pushed, **kw):
        _, msg = run(flows, labels, pushed, R.dirs_of(flows.shape[-1]), expect=-1, **kw)
        assert msg.startswith("cwm_object_response") and field in msg, (field, msg)

    refused("struct_size", mutate=lambda a: setattr(a, "struct_size", a.struct_size - 8))
    refused("base.batch = 0", mutate=lambda a: setattr(a.base, "batch", 0))
    refused("base.T = 0", mutate=lambda a: setattr(a.base, "T", 0))
    refused("base.T = 65536", mutate=lambda a: setattr(a.base, "T", 65536))
    refused("base.H = 10", mutate=lambda a: setattr(a.base, "H", 10))
    refused("base.W = 10", mutate=lambda a: setattr(a.base, "W", 10))
    refused("base.H = 0", mutate=lambda a: setattr(a.base, "H", 0))
    refused("base.H base.W", mutate=lambda a: (setattr(a.base, "H", 512), setattr(a.base, "W", 516)))
    refused("S = 0", mutate=lambda a: setattr(a, "S", 0))
    refused("S = 256", mutate=lambda a: setattr(a, "S", 256))
    for i in range(5):
        refused("flow_strides[%d]" % i, mutate=lambda a, i=i: a.flow_strides.__setitem__(i, -4))
    for i in range(2):
        refused("labels_strides", mutate=lambda a, i=i: a.labels_strides.__setitem__(i, -96))
    for f in ("flows_dev", "labels_dev", "pushed_dev", "tab_dev", "valid_dev", "agg_dev", "coupling_dev", "stats_dev"):
        refused(f, mutate=lambda a, f=f: setattr(a, f, None))
    refused("min_q2", mutate=lambda a: setattr(a, "min_q2", -1))
    refused("min_pixels = 0", min_pixels=0)
    for name in ("self_frac", "move_frac"):
        for bad in (-0.25, 1.5, float("nan"), float("inf")):
            refused(name, **{name: bad})
    got, _ = run(flows, labels, pushed, None, self_frac=0.0, move_frac=1.0)  # (the ends of the range, and no dirs, are accepted)
    equal(got, R.response(flows, R.per_row(labels, 2), pushed, None, self_frac=0.0, move_frac=1.0))


def same_fields(d, c):
    for k in OR.ObjectResponse.__slots__[:5]:
        u, v = getattr(d, k).cpu(), getattr(c, k)
        assert u.dtype == v.dtype and u.shape == v.shape, k
        assert torch.equal(as_bits(u), as_bits(v)), k


def test_measure_on_the_device_equals_measure_on_the_cpu():
    B, K, H, W, S = 2, 3, 64, 64, 5
    flows, labels, pushed = (torch.from_numpy(a) for a in R.case_random(B, K, H, W, S, seed=13))
    dirs = torch.from_numpy(R.dirs_of(S))
    c = OR.measure(flows, labels, pushed, dirs=dirs)
    d = OR.measure(sample_outer(flows.cuda()), labels.cuda(), pushed.cuda(), dirs=dirs.cuda())
    assert d.tab.is_cuda and tuple(d.tab.shape) == (B, K, S, 65, 8) and d.valid.dtype == torch.bool and tuple(d.coupling.shape) == (B, K, 65, 4)
    same_fields(d, c)
    same_fields(OR.measure(flows.cuda().reshape(B, K, 2, H, W, S), labels.cuda(), pushed.cuda().reshape(B, K), min_mag=2.0, move_frac=0.8),
                OR.measure(flows, labels, pushed, min_mag=2.0, move_frac=0.8))
    per_push = labels[:, None].expand(B, K, H, W).clone()
    per_push[:, 2] = 0
    same_fields(OR.measure(flows.cuda(), per_push.cuda(), pushed.cuda(), dirs=dirs.cuda()), OR.measure(flows, per_push, pushed, dirs=dirs))
    for got, want in zip(OR.relations(d, pushed.cuda().reshape(B, K)), OR.relations(c, pushed.reshape(B, K))):
        assert got.is_cuda and torch.equal(got.cpu(), want)
    g = OR.groups(OR.relations(d, pushed.cuda().reshape(B, K))[1])
    assert g.is_cuda and torch.equal(OR.merge_labels(labels.cuda(), g).cpu(), OR.merge_labels(labels, g.cpu()))


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------------------------
NS = 5


class TableFlow(torch.nn.Module):
    """flow_model(video [(r s),T,C,H,W]) -> [(r s),1,2,H,W]: call i gets the rows `order[i]` of the table [R,2,H,W,S] (default: the first rows), whatever the
    video shows"""

    def __init__(self, table, order=None):
        super().__init__()
        self.table = torch.from_numpy(table).permute(0, 4, 1, 2, 3).contiguous().cuda()  # [R,S,2,H,W]
        self.order, self.calls, self.last = order, 0, None

    def forward(self, video, backward=False, **kw):
        S = self.table.shape[1]
        rows = list(range(video.shape[0] // S)) if self.order is None else self.order[self.calls]
        self.calls += 1
        assert len(rows) * S == video.shape[0]
        self.last = self.table[rows].reshape(len(rows) * S, 1, *self.table.shape[2:])
        return self.last


def tiny_generator(flow_model):
    from counterfactualworldmodels_amd import segmentation
    from test_segment_cpu import TINY
    from test_spelke_segment_gpu import predictor

    return segmentation.FlowGenerator(predictor=predictor(TINY), flow_model=flow_model, imagenet_normalize_inputs=True, temporal_dim=2, seed=0), TINY


@pytest.fixture(scope="module")
def tiny():
    from counterfactualworldmodels_amd import synthetic as S

    flows, labels, pushed, dirs = R.case_scene(2, 32, 32, NS)
    fm = TableFlow(flows)
    G, cfg = tiny_generator(fm)
    x = torch.from_numpy(S.synthetic_frames(2, cfg, 3)).cuda()
    return G, fm, x, flows, labels, pushed, dirs


@pytest.mark.parametrize("sample", [False, True])
def test_driver_equals_the_loop_composed_by_hand(tiny, sample):
    from counterfactualworldmodels_amd import segment_step as SS

    G, fm, x, flows, labels, pushed, dirs = tiny
    lab = torch.from_numpy(labels).cuda()
    slots = torch.tensor([1, 2, 3, 9], device="cuda")  # (slot 9 has no pixel: a dead row; its flows are a repeat of row 0's)
    table = fm.table
    fm.table = torch.cat([table[:3], table[:1], table[3:], table[3:4]])
    x0, lab0, slots0 = x.clone(), lab.clone(), slots.clone()
    torch.manual_seed(11)
    state = torch.get_rng_state()
    gen = torch.Generator(device="cuda").manual_seed(7)
    fm.order, fm.calls = None, 0
    res = G.object_interactions(x, lab, slots=slots, num_samples=NS, k_active=2, k_passive=3, sample=sample, generator=gen)
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(x, x0) and torch.equal(lab, lab0) and torch.equal(slots, slots0) and fm.calls == 1
    assert res.tab.is_cuda and tuple(res.tab.shape) == (2, 4, NS, 65, 8) and tuple(res.active.shape) == (2, 4, 32) and res.slots.tolist() == [[1, 2, 3, 9]] * 2
    # by hand: the masks from the restatement, the public counterfactual driver, the restatement on the same flows
    gen = torch.Generator(device="cuda").manual_seed(7)
    keys = torch.rand((2, 4, 16), generator=gen, device="cuda").cpu().numpy() if sample else None
    act, pas, pu = R.push_masks(labels, slots.cpu().numpy()[None].repeat(2, 0), 8, k_active=2, k_passive=3, keys=keys)
    assert np.array_equal(res.active.cpu().numpy(), act) and np.array_equal(res.passive.cpu().numpy(), pas) and pu.tolist() == [[1, 2, 3, 0]] * 2
    assert act[:, 3, 16:].all() and pas[:, 3, 16:].all() and not act[:, :3, 16:].all(-1).any()
    a, p = (torch.from_numpy(m.reshape(8, 32)).cuda().unsqueeze(-1).expand(-1, -1, NS) for m in (act, pas))
    fm.calls = 0
    with torch.random.fork_rng(devices=[]):
        _, f = G.predict_counterfactual_videos_and_flows(x.repeat_interleave(4, 0), a, p, shifts=SS.directions(NS), num_samples=NS, sample_batch_size=None, fix_passive=True)
    hand = G._batch_to_samples(f).cpu().numpy()
    assert np.array_equal(hand[:3], flows[:3]) and np.array_equal(hand[4:7], flows[3:])
    want = R.response(hand, R.per_row(labels, 4), pu.reshape(-1), dirs)
    got = {k: getattr(res, k).reshape((8,) + tuple(getattr(res, k).shape[2:])).cpu().numpy() for k in R.NAMES}
    got["valid"] = got["valid"].astype(np.uint8)
    equal(got, want, "driver")
    rel = R.relations(want["coupling"].reshape(2, 4, 65, 4), want["stats"].reshape(2, 4, 4), pu)
    for k, w in zip(("moves", "mutual", "carries", "tested"), rel):
        assert np.array_equal(getattr(res, k).cpu().numpy(), w), k
    # the pinned relations: 1 and 2 are one body, 3 moves 2 and is not moved by it, slot 9 was never tested
    for b in range(2):
        assert np.argwhere(rel[0][b]).tolist() == [[1, 2], [2, 1], [3, 2]] and np.argwhere(rel[1][b]).tolist() == [[1, 2], [2, 1]]
        assert np.argwhere(rel[2][b]).tolist() == [[3, 2]] and np.nonzero(rel[3][b])[0].tolist() == [1, 2, 3]
    assert OR.groups(res.mutual)[0, :5].tolist() == [0, 1, 1, 3, 4] and res.stats[:, 3].tolist() == [[0, 0, 0, 0]] * 2
    # in chunks of slots: the same result
    fm.order, fm.calls = [[0, 1, 2, 4, 5, 6], [3, 7]], 0
    gen = torch.Generator(device="cuda").manual_seed(7)
    chunked = G.object_interactions(x, lab, slots=slots, num_samples=NS, k_active=2, k_passive=3, sample=sample, generator=gen, slot_batch_size=3)
    assert fm.calls == 2
    for k in OR.ObjectInteractions.__slots__:
        assert torch.equal(as_bits(getattr(chunked, k)), as_bits(getattr(res, k))), k
    fm.table, fm.order = table, None


def test_with_raft_at_random_weights():
    """128 x 128, patch 8, S = 4, two RAFT iterations, three slots.  Equality with the restatement on the flows read back is exact: every decision is an integer
    or a single binary64 division"""
    from counterfactualworldmodels_amd import config as C, segmentation, synthetic as S
    from test_raft_fast_gpu import build
    from test_spelke_segment_gpu import Recorder, predictor

    cfg = C.VmaeConfig(name="tiny_128", img_size=(128, 128), patch=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=128, dec_depth=1, dec_heads=2)
    G = segmentation.FlowGenerator(predictor=predictor(cfg), flow_model=Recorder(build(0)), imagenet_normalize_inputs=True, temporal_dim=2, seed=0)
    x = torch.from_numpy(S.synthetic_frames(1, cfg, 5)).cuda()
    labels = R.scene_labels(1, 128, 128)
    res = G.object_interactions(x, torch.from_numpy(labels).cuda(), num_slots=3, num_samples=4, k_active=3, k_passive=3, raft_iters=2, min_mag=0.05)
    shapes = dict(tab=(1, 3, 4, 65, 8), valid=(1, 3, 4), agg=(1, 3, 65, 4), coupling=(1, 3, 65, 4), stats=(1, 3, 4), slots=(1, 3), active=(1, 3, 512), passive=(1, 3, 512),
                  moves=(1, 65, 65), mutual=(1, 65, 65), carries=(1, 65, 65), tested=(1, 65), dirs=(4, 2))
    dtypes = dict(tab=torch.int64, agg=torch.int64, coupling=torch.float64, stats=torch.int32, slots=torch.int32, dirs=torch.int32)
    for k, s in shapes.items():
        t = getattr(res, k)
        assert tuple(t.shape) == s and t.is_cuda and t.dtype == dtypes.get(k, torch.bool), (k, t.shape, t.dtype)
    tab = res.tab.cpu().numpy()
    area = np.array([(np.where(labels[0] > 64, 0, labels[0]) == l).sum() for l in range(65)])
    assert ((tab[..., 0] + tab[..., 7]) == area).all()  # for every row, sample and slot
    print("[raft] n_valid %s, moved pixels of the pushed slots %s" % (res.stats[0, :, 0].tolist(), [int(tab[0, k, :, k + 1, 1].sum()) for k in range(3)]))
    flows = G._batch_to_samples(G.flow_model.last).cpu().numpy()  # the very same flows, read back
    want = R.response(flows, R.per_row(labels, 3), [1, 2, 3], res.dirs.cpu().numpy(), min_mag=0.05)
    got = {k: getattr(res, k)[0].cpu().numpy() for k in R.NAMES}
    got["valid"] = got["valid"].astype(np.uint8)
    equal(got, want, "raft")
