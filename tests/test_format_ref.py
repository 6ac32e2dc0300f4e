"""tests/fmtref.py checked on the host (no GPU): format_ref (numpy) against format_ref_loop (b"%d" and b"".join) on
every named case, the precondition every case is named for, format_ref against the system grep, the checker's own
teeth, and the new entry point's presence in the header, the bindings and the library."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fmtref
from fmtref import LOG_PATTERNS as PATTERNS
from fmtref import (BIG_PERIODS, LADDER_BASE, NL, Fmt, all_format_cases, assert_format, big_case, chain_cuts, format_ref,
                    format_ref_loop, grep_fmt, label_crossing, label_spans, make_log, python_grep)
from gatherref import BLOCK, TILE, WIN, gather_ref

CASES = all_format_cases() + [big_case()]
HERE = os.path.dirname(os.path.abspath(__file__))


def test_case_names_are_unique():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_the_two_references_agree(case):
    out, off = case.want()
    out2, off2 = format_ref_loop(case.data, case.offsets, case.ids, case.fmt, case.doc_first)
    np.testing.assert_array_equal(off, off2)
    assert bytes(out) == bytes(out2)
    assert_format(case, int(off2[-1]), off2, out2)
    if case.fmt.plain():
        plain, plain_off = gather_ref(case.data, case.offsets, case.ids)
        assert bytes(out) == bytes(plain) and np.array_equal(off, plain_off)


def seps_of(case):
    """The segments that start with the group separator, from the output alone."""
    out, off = case.want()
    a, _ = label_spans(case)
    return np.flatnonzero(a > off[:-1].astype(np.int64)).tolist()


@pytest.mark.parametrize("case", [c for c in CASES if c.need is not None], ids=repr)
def test_preconditions(case):
    need, f = case.need, case.fmt
    out, off = case.want()
    kind = need if isinstance(need, str) else need[0]
    if kind == "prints":
        for k, v in ((0, need[1]), (case.n_ids - 1, need[2])):
            seg = bytes(out[int(off[k]):int(off[k + 1])])
            assert seg.startswith(b"%d:%d:" % (v, v)), (seg, v)
        # a digit count's edge lies between them, or they are the first or the last value there is
        assert len(str(need[1])) != len(str(need[2])) or need[1] == 0 or need[2] == fmtref.LIMIT - 1
    elif kind == "ladder":
        a, b = label_spans(case)
        assert a[1] % 16 == need[1] and b[1] - a[1] == 19 and int(case.offsets[1]) % 16 == need[2]
    elif kind == "label_crosses":
        j = label_crossing(case, need[1])
        a, b = label_spans(case)
        assert j is not None and a[j] < need[1] < b[j] and b[j] - a[j] == 38
    elif kind == "block_edge":
        a, b = label_spans(case)
        assert case.n_ids > 2 * BLOCK and (b - a == 38).all() and case.ids[BLOCK] == case.ids[BLOCK - 1] + 1
    elif kind == "out_bytes":
        assert out.size == need[1]
    elif kind == "out_empty":
        assert out.size == 0 and case.n_ids > 64 * BLOCK // 2 and not f.plain()
    elif kind == "empty_blocks":
        assert (np.diff(off.astype(np.int64))[:-1] == 0).all() and out.size == 37 and case.n_ids > 40 * BLOCK
    elif kind == "long_doc":
        assert np.diff(case.offsets.astype(np.int64)).max() > 130 * TILE
    elif kind == "steps":
        ids = case.ids.astype(np.int64)
        for k in (BLOCK, 1024):
            assert (ids[k] == ids[k - 1] + 1) == (need[1] == "adjacent"), k
        want = ([0] if f.sep_first else []) + ([BLOCK, 1024] if need[1] == "apart" else [])
        assert seps_of(case) == want
        assert len(f.group_sep) in (1, 3, 8)
    elif kind == "seps":
        assert seps_of(case) == need[1]
    else:
        assert kind == "terminate"
        lens = np.diff(case.offsets.astype(np.int64))
        ends = case.data[np.maximum(case.offsets[1:].astype(np.int64) - 1, 0)]
        assert (lens == 0).any() and ((lens > 0) & (ends == NL)).any() and ((lens > 0) & (ends != NL)).any()
        assert case.n % 16 != 0 and lens[-1] > 0 and case.data[-1] != NL and case.ids.max() == case.n_docs - 1
        t = f.terminate
        for k in range(case.n_ids):                             # every segment ends in the terminator, once more at most
            seg = out[int(off[k]):int(off[k + 1])]
            assert seg[-1] == t
        added = out.size - format_ref(case.data, case.offsets, case.ids, Fmt(**{**f.kwargs(), "terminate": None}))[0].size
        assert 0 < added < case.n_ids or case.n_ids == 1


def test_the_cases_cover_what_the_kernels_branch_on():
    names = {c.name for c in CASES}
    for n in fmtref.N_IDS:
        for k in fmtref.FLAG_SETS:
            assert f"ids{n}_{k}" in names
    assert {c.need[1] for c in CASES if c.need and c.need[0] == "ladder"} == set(range(16))
    assert {c.need[2] for c in CASES if c.need and c.need[0] == "ladder"} == set(range(16))
    assert LADDER_BASE + 3 < 10 ** 18 and len(str(LADDER_BASE)) == 18
    big = big_case()
    assert big.want()[0].size % 2 == 1 and big.want()[0].size * BIG_PERIODS > 64 << 20
    assert big.fmt.sep_first and big.fmt.group_sep           # so that every period prints the same bytes
    assert label_crossing(next(c for c in CASES if c.name == "label_crosses_window"), WIN) is not None


def test_chain_cuts_are_document_boundaries():
    case = next(c for c in CASES if c.name == "terminate_all_labels")
    cuts = chain_cuts(case.offsets)
    assert len(cuts) == 3 and cuts == sorted(set(cuts)) and all(c in set(case.offsets.tolist()) for c in cuts)
    assert 0 < cuts[0] and cuts[-1] < case.n


# ---------------------------------------------------------------------------
# the checker's teeth

def _defects(case):
    out, off = case.want()
    one = out.copy()
    one[out.size // 2] ^= 1
    yield "a flipped byte", out.size, off, one
    yield "one byte short", out.size - 1, off, out
    bad = off.copy()
    bad[off.size // 2] += np.uint64(1)
    yield "a moved offset", out.size, bad, out
    yield "an offset too few", out.size, off[:-1], out


def test_assert_format_catches():
    case = next(c for c in CASES if c.name == "ids65_all")
    out, off = case.want()
    assert_format(case, out.size, off, np.concatenate([out, np.full(32, 0xA5, np.uint8)]), fill=0xA5)
    for name, n, o, b in _defects(case):
        with pytest.raises(AssertionError):
            assert_format(case, n, o, b)
        del name
    with pytest.raises(AssertionError):
        assert_format(case, out.size, off, np.concatenate([out, np.array([0xA5, 0, 0xA5], np.uint8)]), fill=0xA5)


# ---------------------------------------------------------------------------
# against grep

GREP_RUNS = [(["-n"], dict(number=True), 0, 0), (["-b"], dict(byte_offset=True), 0, 0), (["-nb"], dict(number=True, byte_offset=True), 0, 0),
             (["-C", "1"], {}, 1, 1), (["-A", "2", "-n"], dict(number=True), 0, 2), ([], {}, 0, 0)]


@pytest.mark.skipif(shutil.which("grep") is None, reason="no grep installed")
@pytest.mark.parametrize("run", GREP_RUNS, ids=lambda r: " ".join(r[0]) or "plain")
def test_format_ref_equals_grep(tmp_path, run):
    args, kw, before, after = run
    data = make_log()
    assert not data.endswith(b"\n")
    (tmp_path / "log").write_bytes(data)
    (tmp_path / "pat").write_bytes(b"".join(p + b"\n" for p in PATTERNS))
    want = subprocess.run(["grep", "-F", "-f", str(tmp_path / "pat")] + args + [str(tmp_path / "log")], stdout=subprocess.PIPE,
                          env={**os.environ, "LC_ALL": "C"}).stdout
    off, ids, first = python_grep(data, PATTERNS, before, after)[:3]
    assert 0 < ids.size < off.size - 1 and ids[-1] == off.size - 2
    out, _ = format_ref(np.frombuffer(data, np.uint8), off, ids, grep_fmt(kw, before, after), first)
    assert bytes(out) == want
    if before or after:
        assert b"\n--\n" in want and re.search(rb"^\d+-", want, re.M) if kw.get("number") else b"\n--\n" in want


# ---------------------------------------------------------------------------
# the entry point exists

def test_the_symbol_is_declared_bound_and_exported():
    import inspect

    from phfpfac_amd import GpuMatcher, _ffi
    header = open(os.path.join(HERE, "..", "include", "pfac.h")).read()
    assert re.search(r"\bint\s+pfac_documents_gather_format\s*\(", header)
    for name in ("PFAC_LINE_NUMBER", "PFAC_LINE_OFFSET", "PFAC_LINE_TERMINATE", "PFAC_LINE_CONTEXT_SEP", "PFAC_LINE_SEP_FIRST",
                 "PFAC_LINE_MAX_GROUP_SEP"):
        m = re.search(rf"#define\s+{name}\s+(\d+)u", header)
        assert m and int(m.group(1)) == getattr(_ffi, name), name
    assert "pfac_documents_gather_format" in _ffi.HIP_SYMBOLS
    assert hasattr(_ffi.hip_lib(), "pfac_documents_gather_format")
    import ctypes as C
    assert C.sizeof(_ffi.CLineFormat) == 32
    for name in ("gather_documents_formatted", "grep_text"):
        assert callable(getattr(GpuMatcher, name, None)), name
    p = inspect.signature(GpuMatcher.grep_text).parameters
    assert p["number_base"].default == 1 and p["offset_base"].default == 0 and p["sep_first"].default is False
