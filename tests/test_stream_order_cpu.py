"""The table of stream-ordering cases (tests/stream_order.py CASES / EXEMPT, run by tests/test_stream_order_gpu.py) stays complete: every entry point of
include/cwm_hip.h that takes a stream has a case or a written reason.  Runs without a GPU and without the native library."""
import os
import re

import stream_order as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "cwm_hip.h")) as fh:
        return fh.read()


def uncovered(header_text):
    have = set(SO.covered()) | set(SO.EXEMPT)
    return [n for n in SO.stream_entry_points(header_text) if n not in have]


def test_the_parser_finds_the_stream_parameters_and_fields():
    names = SO.stream_entry_points(header())
    assert len(names) == len(set(names)) and len(names) >= 34  # (30 functions and 4 args structs when this test was written)
    # one function with the stream last, one with it in the middle of a long list, the four args structs, and nothing without a stream
    for n in ("cwm_split_bf16", "cwm_flow_filter_stats", "cwm_forward_args", "cwm_conj_forward_args", "cwm_patch_error_args", "cwm_raft_forward_args", "cwm_allgatherv"):
        assert n in names, n
    for n in ("cwm_forward", "cwm_model_create", "cwm_raft_set_corr", "cwm_config", "cwm_kernel_stats", "cwm_flow_transform_work_bytes"):
        assert n not in names, n


def test_every_stream_taking_entry_point_has_a_case_or_a_reason():
    assert uncovered(header()) == []


def test_no_case_and_no_exemption_names_something_that_does_not_exist():
    text = header()
    declared = set(re.findall(r"\b(cwm_\w+)\b", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))
    streamed = set(SO.stream_entry_points(text))
    for name, reason in SO.EXEMPT.items():
        assert name in streamed, "exemption for %s, which is no stream-taking entry point of the header" % name
        assert reason.strip()
        assert name not in SO.covered(), name
    for name, cases in SO.covered().items():
        # (a function that takes its stream inside an args struct is named next to the struct: it must exist, the struct must carry the stream)
        assert name in declared, "%s (cases %s) is not in the header" % (name, cases)
    for case, (entries, protocols, asynchronous) in SO.CASES.items():
        assert entries and protocols and set(protocols) <= set("ABCD") and "A" in protocols and isinstance(asynchronous, bool), case
        assert any(e in streamed for e in entries), case


def test_a_new_stream_taking_function_without_a_case_is_noticed():
    text = header().replace("CWM_API const char* cwm_last_error(void);",
                            "CWM_API int cwm_new_kernel(const float* x_dev, int n,\n                           void* stream);\n"
                            "typedef struct cwm_new_args { int n; void* stream; } cwm_new_args;\nCWM_API const char* cwm_last_error(void);")
    assert uncovered(text) == ["cwm_new_kernel", "cwm_new_args"]


def test_every_case_has_a_runner_in_the_gpu_file():
    """read as text: importing the GPU file would load the native library"""
    with open(os.path.join(ROOT, "tests", "test_stream_order_gpu.py")) as fh:
        src = fh.read()
    registered = set(re.findall(r'^@case\("(\w+)"\)', src, flags=re.M))
    assert registered == set(SO.CASES), (sorted(set(SO.CASES) - registered), sorted(registered - set(SO.CASES)))
