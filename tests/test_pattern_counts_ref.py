"""Counts per pattern, the host half (no GPU): PfacTable.counts_by_pattern turns the per-state counts the device
delivers (pfac_records_count_states) into counts by 1-based pattern id.  The state counts here come from the table's own
lookup walked on the host; the expected pattern counts from a brute-force count over the pattern lines (literal tables)
and from oracle/charclass_oracle.py (class tables)."""
import importlib.util
import os

import numpy as np
import pytest

import countref
import phfpfac_amd
from phfpfac_amd import GpuMatcher, PfacTable, _ffi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("charclass_oracle", os.path.join(REPO, "oracle", "charclass_oracle.py"))
cco = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cco)


def test_literal_table_with_a_duplicate_line():
    """`ab` is lines 1 and 2: line 2 wins (the reference's rule), line 1 counts 0."""
    lines = [b"ab", b"ab", b"abc"]
    table = PfacTable.from_bytes(b"".join(p + b"\n" for p in lines), 256)
    data = np.frombuffer(b"abcab abab cabc xabx ab", dtype=np.uint8)
    sc = countref.walk_state_counts(table, data)
    got = table.counts_by_pattern(sc)
    want = countref.brute_counts(lines, data)
    assert got.dtype == np.uint64 and got.size == 4
    np.testing.assert_array_equal(got, want)
    assert got[1] == 0 and got[2] == 7 and got[3] == 2 and got[0] == 0
    assert int(got.sum()) == int(sc.sum())
    with pytest.raises(ValueError):
        table.counts_by_pattern(sc[:-1])
    np.testing.assert_array_equal(table.counts_by_pattern(np.zeros(3, dtype=np.uint64)), np.zeros(4, dtype=np.uint64))


def test_class_table_states_and_patterns_many_to_many():
    """`[ab]x` ends in two final states (`ax`, `bx`), and the state of `ax` stands for patterns 1, 2 and 4."""
    img = b"[ab]x\nax\nb\n[ab]x\nxa[0-9]\n"
    table = PfacTable.from_charclass(img, 256)
    multi = [list(table.out_ids[table.out_first[s]:table.out_first[s + 1]]) for s in range(table.num_final)]
    assert [1, 2, 4] in multi and [1, 4] in multi               # one state, several patterns; pattern 1 in two states
    rng = np.random.default_rng(12)
    data = np.frombuffer(b"abx0123 ", dtype=np.uint8)[rng.integers(0, 8, 5000)]
    sc = countref.walk_state_counts(table, data)
    got = table.counts_by_pattern(sc)
    _, want_ids = cco.match(img, data)
    want = countref.pattern_counts(want_ids, 5)
    assert got.size == 6 and (want[1:] > 20).all()
    np.testing.assert_array_equal(got, want)
    assert int(got.sum()) > int(sc.sum())                       # a record of a shared state counts once per pattern


def test_reference_output_lines_parse_into_counts():
    text = open(os.path.join(REPO, "tests", "golden", "out", "exp_x_expinput_s1_w256.txt"), "rb").read()
    counts, lines = countref.parse_counts(text, 4)
    assert lines == 47 and int(counts.sum()) == 47 and counts[0] == 0
    with pytest.raises(AssertionError):
        countref.parse_counts(text + b"junk\n", 4)


def test_new_symbols_are_bound_and_exported():
    for name in ("pfac_records_count_states", "pfac_selection_count_states", "pfac_state_counts_d2h"):
        assert name in _ffi.HIP_SYMBOLS
        assert hasattr(_ffi.hip_lib(), name)
    assert _ffi.PFAC_COUNT_ACCUMULATE == 1 and phfpfac_amd.PFAC_COUNT_ACCUMULATE == 1
    assert "PFAC_COUNT_ACCUMULATE" in phfpfac_amd.__all__
    for name in ("count_states", "count_selection_states", "state_counts_to_host", "count_patterns"):
        assert callable(getattr(GpuMatcher, name))
    assert callable(PfacTable.counts_by_pattern)
