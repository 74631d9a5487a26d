"""Stream-ordering protocols for the entry points of include/cwm_hip.h that take a stream, stated once, and the table of cases that
tests/test_stream_order_gpu.py runs.  The table is plain data and this module loads neither torch nor the native library at import, so that
tests/test_stream_order_cpu.py can hold it against the header without a GPU.

Every comparison is `torch.equal` against a PLAIN run of the same case: default stream, `torch.cuda.synchronize()` before and after.  The paths are bit-stable
run to run, so there is no tolerance.

  Delay       a chain of dependent matmuls on one stream, with events around it; `Delay.check()` fails the test when the measured delay stayed below its target
              (a test whose delay did not happen proves nothing).
  Poison      float inputs NaN, index-like inputs ANOTHER VALID value of the same kind (never an out-of-range index): a missed ordering is a wrong number.
  A  late inputs, early consumers   on a side stream: poisoned inputs, device sync, delay, truth copied in, the call, clones of the outputs, poison written
                                    back over the inputs (write after read), stream sync, compare
  B  busy null stream               delay on the default (null) stream, then at once a call on a fresh non-blocking stream that allocates and zero-fills
  C  back to back                   behind a delay, two calls with different inputs on one handle without a host sync between them
  D  two caller streams             call 1 on s1, s2.wait_stream(s1), call 2 on s2, clones on s2
"""
from __future__ import annotations

import re
from typing import Callable, Dict, List, Sequence, Tuple

# ---- the case table ----------------------------------------------------------------------------------------------------------------------------------------
# case name (the GPU file registers one runner per name) -> (entry points of include/cwm_hip.h the case calls: functions, and the args structs whose `stream`
# field it sets; protocols; True when the header documents the call as not synchronising the host, so that it must return while the delay is still running)
CASES: Dict[str, Tuple[Tuple[str, ...], str, bool]] = {
    "vit": (("cwm_forward", "cwm_forward_args"), "ABCD", True),  # check=False is asynchronous; check=True is run as well
    "conj": (("cwm_conj_forward", "cwm_conj_forward_args"), "ABCD", True),
    "raft": (("cwm_raft_forward", "cwm_raft_forward_args", "cwm_raft_forward_ex"), "ABC", True),
    "raft_forward_interpolate": (("cwm_raft_forward_interpolate",), "A", True),
    "raft_convex_upsample": (("cwm_raft_convex_upsample", "cwm_raft_convex_upsample1"), "A", True),
    "raft_head_project": (("cwm_raft_head_project",), "A", True),
    "raft_corr_lookup": (("cwm_raft_corr_lookup", "cwm_raft_corr_lookup_on_the_fly"), "A", False),  # both synchronise (they free their pyramid)
    "flow_corrs": (("cwm_flow_features", "cwm_flow_transform", "cwm_flow_cov"), "AC", True),
    "flow_motion_map": (("cwm_flow_motion_sum", "cwm_flow_map_finish"), "AC", True),
    "flow_features": (("cwm_flow_features",), "AC", True),
    "flow_filter": (("cwm_flow_filter_stats", "cwm_flow_filter_apply", "cwm_flow_filter_pack"), "AC", True),
    "shift_prompts": (("cwm_shift_prompts",), "A", True),
    "prompt_table_expand": (("cwm_prompt_table_expand",), "A", True),
    "multi_shift_prompts": (("cwm_multi_shift_prompts",), "A", True),
    "patch_error": (("cwm_patch_error", "cwm_patch_error_args"), "A", True),
    "unembed": (("cwm_unembed",), "AB", False),  # reads its error word back
    "rectangularize": (("cwm_mask_row_counts", "cwm_mask_flip_picks"), "AC", False),  # the wrapper reads the row counts back
    "linear": (("cwm_linear",), "AB", False),  # the stand-alone entry points synchronise their stream before they free their scratch
    "attention": (("cwm_attention",), "A", False),
    "attention_ragged": (("cwm_attention_ragged",), "AB", False),
    "layernorm": (("cwm_layernorm",), "A", False),
    "mask_to_perm": (("cwm_mask_to_perm",), "AB", False),
    "split_bf16": (("cwm_split_bf16",), "A", True),
}

# stream-taking entry points without a case, each with the reason
EXEMPT: Dict[str, str] = {
    "cwm_broadcast": "RCCL collective: needs several ranks; collectives are not exercised this way on a shared machine (tests/test_dist_cpu.py covers the host logic)",
    "cwm_allgather": "RCCL collective: needs several ranks",
    "cwm_allgatherv": "RCCL collective: needs several ranks",
    "cwm_allreduce_sum_f32": "RCCL collective: needs several ranks",
}
# not in the table either: capture into a hipGraph (INTEGRATION.md "Streams") is a separate piece of work


def stream_entry_points(header_text: str) -> List[str]:
    """Every `CWM_API` function of the header with a `void* stream` parameter, and every `typedef struct NAME { ... }` with a `void* stream;` field."""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    names = []
    for m in re.finditer(r"CWM_API\s+[\w\s\*]+?\b(\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        if re.search(r"void\s*\*\s*stream\b", m.group(2)):
            names.append(m.group(1))
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\w+\s*;", text, flags=re.S):
        if re.search(r"void\s*\*\s*stream\s*;", m.group(2)):
            names.append(m.group(1))
    return names


def covered() -> Dict[str, List[str]]:
    out: Dict[str, List[str]] = {}
    for case, (entries, _, _) in CASES.items():
        for e in entries:
            out.setdefault(e, []).append(case)
    return out


# ---- what follows needs torch and a GPU (imported by the GPU test file only) -------------------------------------------------------------------------------
MIN_DELAY_MS = 20.0


class Delay:
    """A chain of dependent matmuls whose length was calibrated once (`Delay.calibrate()`): `Delay(stream, target_ms)` enqueues it with an event on either side;
    `check()`, after the final synchronisation, asserts that the measured delay reached the target."""

    N = 2048
    _ms_per_matmul = None
    _bufs = None

    @classmethod
    def calibrate(cls):
        import torch

        if cls._ms_per_matmul is not None:
            return
        g = torch.Generator().manual_seed(0)
        q, _ = torch.linalg.qr(torch.randn(cls.N, cls.N, generator=g))  # orthogonal: the chain neither grows nor decays
        cls._bufs = (q.cuda(), torch.randn(cls.N, cls.N, generator=g).cuda(), torch.empty(cls.N, cls.N, device="cuda"))
        for _ in range(2):  # (the first pass also pays the BLAS library's start-up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            cls._chain(64)
            e1.record()
            torch.cuda.synchronize()
        cls._ms_per_matmul = max(e0.elapsed_time(e1) / 64, 1e-3)

    @classmethod
    def _chain(cls, n):
        import torch

        q, a, b = cls._bufs
        for _ in range(n):
            torch.mm(a, q, out=b)
            a, b = b, a

    @classmethod
    def warm(cls, stream):
        """one matmul on `stream` (the BLAS handle and workspace torch keeps per stream), to be followed by a device synchronisation"""
        import torch

        cls.calibrate()
        with torch.cuda.stream(stream):
            cls._chain(2)

    def __init__(self, stream, target_ms):
        import torch

        self.calibrate()
        self.target_ms = max(float(target_ms), MIN_DELAY_MS)
        self.begin, self.end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = int(1.5 * self.target_ms / self._ms_per_matmul) + 2  # half as long again: the calibration ran on a warm device
        with torch.cuda.stream(stream):
            self.begin.record(stream)
            self._chain(n + (n & 1))  # (even: the chain ends in the buffer it began in)
            self.end.record(stream)

    def running(self) -> bool:
        return not self.end.query()

    def check(self):
        """after the final synchronisation"""
        got = self.begin.elapsed_time(self.end)
        assert got >= self.target_ms, "the delay ran %.1f ms, short of its target %.1f ms: the test proves nothing" % (got, self.target_ms)
        return got


_STREAMS: Dict[int, object] = {}


def side_stream(i: int):
    """Side stream i of the module, a `torch.cuda.Stream()` (non-blocking) made once.  Protocols A, C and D run on the same few streams in every case, as a
    caller's loop does: a handle keeps per-stream scratch (the split-K slabs of the small-launch GEMMs: csrc/engine.hip attach_splitk_workspace) for the last 8
    streams it saw, and evicts the oldest with a hipFree -- a device-wide wait -- when a ninth arrives.  A fresh stream per run made every later call of a
    long-lived handle wait for the delay in front of it, so that nothing was queued behind unfinished work any more."""
    import torch

    if i not in _STREAMS:
        _STREAMS[i] = torch.cuda.Stream()
    return _STREAMS[i]


LOG: List[str] = []  # one line per protocol run (pytest -s / -rP)


def note(line: str):
    LOG.append(line)
    print(line)


def plain(call: Callable, inputs: Sequence) -> Tuple:
    """(outputs, synchronised wall time in ms) of `call(*inputs)` on the default stream with a device synchronisation on either side.  The outputs are clones
    that stay alive: the streamed run cannot be handed their memory with the right answer still in it."""
    import time

    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call(*inputs)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return tuple(o.clone() for o in _tuple(out)), ms


def _tuple(out):
    import torch

    return (out,) if torch.is_tensor(out) else tuple(out)


def same(a, b) -> bool:
    import torch

    return len(a) == len(b) and all(u.shape == v.shape and torch.equal(u, v) for u, v in zip(a, b))


def poison_like(t):
    """NaN for floats; index-like inputs get their poison from the case (another valid value), never from here"""
    import torch

    assert t.is_floating_point()
    return torch.full_like(t, float("nan"))


def check_poison(name, truth, poison, want, call=None, poison_runs=True):
    """the conditions of a case: every poisoned input differs from its truth (on the CPU), and the plain run on the poison -- where it runs at all -- differs from
    the plain run on the truth; otherwise the case could not fail"""
    import torch

    for i, (t, p) in enumerate(zip(truth, poison)):
        assert t.shape == p.shape and t.dtype == p.dtype, (name, i)
        assert not torch.equal(t.cpu(), p.cpu()), "%s: poison of input %d equals its truth" % (name, i)
    if call is not None and poison_runs:
        got, _ = plain(call, [p.clone() for p in poison])
        assert not same(got, want), "%s: the plain run on the poison equals the plain run on the truth" % name


def protocol_a(name, call, truth, poison, want, plain_ms, asynchronous, extra=""):
    """late inputs and early consumers.  `truth` / `poison`: device tensors (made and synchronised before); `call(*buffers)` -> output tensor(s)"""
    import torch

    s = side_stream(0)
    Delay.warm(s)
    with torch.cuda.stream(s):
        bufs = [p.clone() for p in poison]
        torch.cuda.synchronize()
        d = Delay(s, 3 * plain_ms)
        for b, t in zip(bufs, truth):
            b.copy_(t, non_blocking=True)
        out = _tuple(call(*bufs))
        running = d.running()
        got = tuple(o.clone() for o in out)
        for b, p in zip(bufs, poison):
            b.copy_(p, non_blocking=True)
        s.synchronize()
    ms = d.check()
    note("[A %s%s] delay %.1f ms (target %.1f), call returned with the delay %s" % (name, extra, ms, d.target_ms, "running" if running else "FINISHED"))
    if asynchronous:
        assert running, "%s%s: documented as asynchronous, but the call returned after the work queued before it had finished" % (name, extra)
    assert same(got, want), "%s%s: protocol A (late inputs / early consumers) differs from the plain run" % (name, extra)
    torch.cuda.synchronize()


def protocol_b(name, call, inputs, want, plain_ms, extra=""):
    """busy null stream, fresh buffers: the delay on the default stream, then at once `call(*inputs)` on a fresh non-blocking stream"""
    import torch

    assert torch.cuda.default_stream().cuda_stream == 0
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    d = Delay(torch.cuda.default_stream(), 3 * plain_ms)
    with torch.cuda.stream(s):
        out = _tuple(call(*inputs))
        waited = not d.running()
        got = tuple(o.clone() for o in out)
    torch.cuda.synchronize()
    ms = d.check()
    note("[B %s%s] null-stream delay %.1f ms; at the return of the call the delay had %s" % (
        name, extra, ms, "FINISHED (the library waited for the device itself)" if waited else "not finished (nothing waited for the null stream)"))
    assert same(got, want), "%s%s: protocol B (busy null stream, fresh buffers) differs from the plain run" % (name, extra)
    return waited


def protocol_c(name, call, truth1, truth2, start1, start2, want1, want2, plain_ms, asynchronous, extra=""):
    """back to back: behind a delay on a side stream, two calls with different inputs and no host synchronisation between them.  start1 / start2: what the
    input buffers hold until the truths are copied in behind the delay (the poison of protocol A)"""
    import torch

    s = side_stream(0)
    Delay.warm(s)
    with torch.cuda.stream(s):
        b1 = [p.clone() for p in start1]
        b2 = [p.clone() for p in start2]
        torch.cuda.synchronize()
        d = Delay(s, 6 * plain_ms)
        for b, t in zip(b1 + b2, list(truth1) + list(truth2)):
            b.copy_(t, non_blocking=True)
        o1 = _tuple(call(*b1))
        o2 = _tuple(call(*b2))
        running = d.running()
        g1, g2 = tuple(o.clone() for o in o1), tuple(o.clone() for o in o2)
        s.synchronize()
    ms = d.check()
    note("[C %s%s] delay %.1f ms, both calls returned with the delay %s" % (name, extra, ms, "running" if running else "FINISHED"))
    if asynchronous:
        assert running, "%s%s: documented as asynchronous, but two calls returned after the work queued before them had finished" % (name, extra)
    assert same(g1, want1), "%s%s: protocol C, first of two back-to-back calls differs from its plain run" % (name, extra)
    assert same(g2, want2), "%s%s: protocol C, second of two back-to-back calls differs from its plain run" % (name, extra)
    torch.cuda.synchronize()


def protocol_d(name, call, truth1, truth2, start1, start2, want1, want2, plain_ms, extra=""):
    """one handle, two caller streams chained by the caller"""
    import torch

    s1, s2 = side_stream(1), side_stream(2)
    Delay.warm(s1)
    Delay.warm(s2)
    with torch.cuda.stream(s1):
        b1 = [p.clone() for p in start1]
        b2 = [p.clone() for p in start2]
        torch.cuda.synchronize()
        d = Delay(s1, 6 * plain_ms)
        for b, t in zip(b1 + b2, list(truth1) + list(truth2)):
            b.copy_(t, non_blocking=True)
        o1 = _tuple(call(*b1))
    s2.wait_stream(s1)
    with torch.cuda.stream(s2):
        o2 = _tuple(call(*b2))
        running = d.running()
        g1, g2 = tuple(o.clone() for o in o1), tuple(o.clone() for o in o2)
        s2.synchronize()
    s1.synchronize()
    ms = d.check()
    note("[D %s%s] delay %.1f ms, both calls returned with the delay %s" % (name, extra, ms, "running" if running else "FINISHED"))
    assert same(g1, want1), "%s%s: protocol D, the call on the first stream differs from its plain run" % (name, extra)
    assert same(g2, want2), "%s%s: protocol D, the call on the second stream differs from its plain run" % (name, extra)
    torch.cuda.synchronize()
