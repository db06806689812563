"""No GPU: the table of tests/test_gpu_streams.py (tests/_stream_table.py) against the header and against INTEGRATION.md.
Every prototype of include/tomo_mi355x.h that takes a `void *stream` is run by a case of that file on a side stream behind a
delay; the table names nothing the header does not have; its asynchronous / synchronising split is the one the document
states; every case the table names is registered in the test file.  There is no exclusion list."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import _stream_table as ST  # noqa: E402


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def header_prototypes():
    """{name: parameter list} of every function prototype of the header, comments removed"""
    text = re.sub(r"/\*.*?\*/", " ", _read("include", "tomo_mi355x.h"), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(tomo_\w+)\s*\(([^;{}()]*)\)\s*;", text)}


def stream_prototypes():
    return sorted(name for name, params in header_prototypes().items() if re.search(r"\bvoid\s*\*\s*stream\b", params))


def test_the_parser_sees_the_header():
    protos = header_prototypes()
    assert "void *stream" in protos["tomo_fp3d"] and "void *stream" in protos["tomo_halo_pull2"]      # a one- and a three-line one
    assert "stream" not in protos["tomo_ctx_create"] and "stream" not in protos["tomo_release_scratch"]
    assert len(protos) > 120


def test_every_prototype_with_a_stream_has_a_case():
    want = stream_prototypes()
    assert len(want) == 85, len(want)      # a new entry point raises the figure together with its case
    missing = [n for n in want if n not in ST.TABLE]
    assert not missing, ("no case of tests/test_gpu_streams.py runs", missing)


def test_the_table_names_nothing_the_header_does_not_have():
    extra = sorted(set(ST.TABLE) - set(stream_prototypes()))
    assert not extra, extra


def test_the_split_is_the_one_integration_md_states():
    """the bullet "Every entry point is asynchronous on the stream passed in, except three kinds" names the exceptions: the
    entries that wait for their stream, and those that wait with a tolerance > 0 only"""
    text = " ".join(_read("INTEGRATION.md").split())
    m = re.search(r"Every entry point is asynchronous on the stream passed in, except three kinds:(.*?)With a tolerance of 0 they "
                  r"are asynchronous\.", text)
    assert m, "the bullet of INTEGRATION.md was reworded: this test reads it"
    waits, marker, with_tolerance = m.group(1).partition("with a tolerance > 0, and only then,")
    assert marker
    assert not re.search(r"`tomo_\w*\*", m.group(1)), "a wildcard names no entry point"
    sync = {n for n, (_, kind) in ST.TABLE.items() if kind == ST.SYNC}
    tol = {n for n, (_, kind) in ST.TABLE.items() if kind == ST.TOL}
    named_async = {"tomo_pwls_weights_scaled"}          # named in the bullet as the asynchronous twin
    assert set(re.findall(r"`(tomo_\w+)`", waits)) - named_async == sync, sorted(sync)
    assert ST.TABLE["tomo_pwls_weights_scaled"][1] == ST.ASYNC
    assert set(re.findall(r"`(tomo_\w+)`", with_tolerance)) - {"tomo_rel_change"} == tol == set(ST.TOL_ENTRIES), sorted(tol)
    assert all(kind in (ST.ASYNC, ST.SYNC, ST.TOL) for _, kind in ST.TABLE.values())


def test_every_entry_point_with_a_tolerance_argument_is_of_the_third_kind():
    """the header's own parameter lists: `double tol` / `double tolerance` marks the entries that may wait at a check"""
    protos = header_prototypes()
    takes = {n for n in stream_prototypes() if re.search(r"\bdouble\s+tol(erance)?\b", protos[n])}
    assert takes == set(ST.TOL_ENTRIES), (sorted(takes - set(ST.TOL_ENTRIES)), sorted(set(ST.TOL_ENTRIES) - takes))


def test_every_case_of_the_table_is_registered_in_the_test_file():
    text = _read("tests", "test_gpu_streams.py")
    registered = re.findall(r'^@case\("(\w+)"\)', text, flags=re.M)
    assert sorted(registered) == sorted(ST.CASES), (sorted(set(ST.CASES) - set(registered)), sorted(set(registered) - set(ST.CASES)))
    assert len(registered) == len(set(registered))
