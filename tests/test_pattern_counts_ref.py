"""Counts per pattern, the host half (no GPU): PfacTable.counts_by_pattern turns the per-state counts the device
delivers (pfac_records_count_states) into counts by 1-based pattern id.  The state counts here come from the table's own
lookup walked on the host; the expected pattern counts from a brute-force count over the pattern lines (literal tables)
and from oracle/charclass_oracle.py (class tables).

The second half is the CPU twin of the chained-counts test of tests/test_gpu_pattern_counts.py: the text cut into owned
ranges (each scanned with the halo behind it), the CPU oracle over every part, composed with tests/wordref.py and with
tests/llref.py chained through exit -> entry, sums to the histograms of one scan of the whole -- so what the GPU test
expects is the reference's own property, for the very cut lists it uses."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import countref
import phfpfac_amd
import wordref
from llref import greedy, line_lengths
from orc import Oracle
from phfpfac_amd import GpuMatcher, PfacTable, _ffi
from phfpfac_amd.matcher import tiled_bytes

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


# ---------------------------------------------------------------------------
# chained ranges: the counts accumulated over the ranges are the counts of one scan of the whole

TILE = 4096
CHAIN_N = 65536 + 123                   # 17 tiles, the last one ragged
CHAIN_FORMS = (("experimentpattern", {}, 2), ("xaa", {}, 4), ("xaa+xab+xac+xad", {"PFAC_WIDE": "1"}, 8))     # 2-, 4- and 8-byte records
CUT_LISTS = ("fixed", "k2", "k5", "k17")


@functools.lru_cache(maxsize=None)
def _chain_whole(path, para_path):
    """(buf, pos, ids, lens, M) of the whole text: the tiled paragraph and the CPU oracle's records of it."""
    buf = tiled_bytes(CHAIN_N, open(para_path, "rb").read())
    o = Oracle(path, 1, 1)
    pos, ids = o.scan_spec(np.ascontiguousarray(buf))
    o.close()
    ll = line_lengths(path)
    for a in (buf, pos, ids):
        a.setflags(write=False)
    return buf, pos.astype(np.int64), ids.astype(np.int64), ll[ids], int(ll.max())


def chain_cuts(name, form, buf, pos, lens, M):
    """The cut list `name` of record form number `form`: ascending, from 0 to CHAIN_N.  "kK": K ranges at seeded random
    cuts; "fixed": the shapes where chaining goes wrong."""
    n = buf.size
    if name != "fixed":
        k = int(name[1:])
        rng = np.random.default_rng([form, k, 0x43555453])
        return [0] + sorted(int(c) for c in rng.integers(0, n + 1, k - 1)) + [n]
    assert M >= 4
    long = np.flatnonzero((lens > 2) & (pos > 7 * TILE))
    # two bytes into a match, which then ends in the halo (experimentpattern's text holds single a's only, matches of one
    # byte: there the cut falls right behind one)
    in_match = int(pos[long[0]]) + 2 if long.size else int(pos[np.flatnonzero(pos > 7 * TILE)[0]]) + 1
    in_word = 12 * TILE + 1 + int(np.flatnonzero(wordref.cuts(buf)[12 * TILE + 1:])[0])      # inside a word
    cuts = [0, 2 * TILE,                # a cut on a multiple of 4096
            2 * TILE + 1,               # a one-byte range
            2 * TILE + 3,               # a range shorter than max_pat_len - 1
            2 * TILE + 3,               # an empty range
            in_match, in_word, n]       # ... and the last range ends at N
    assert cuts == sorted(cuts) and 2 < M - 1 and in_match % TILE and wordref.cuts(buf)[in_word]
    assert ((pos < in_match) & (pos + lens > in_match)).any() or not long.size
    return cuts


def chain_parts(buf, cuts, M):
    """(a, b, part, prev_byte, next_byte) per owned range [a, b): the part is buf[a : min(b + M, N)]."""
    n = buf.size
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        avail = min(b + M, n)
        out.append((a, b, np.ascontiguousarray(buf[a:avail]), int(buf[a - 1]) if a else -1, int(buf[avail]) if avail < n else -1))
    return out


@functools.lru_cache(maxsize=None)
def chain_reference(path, para_path, name, form):
    """What the CPU says about every range of cut list `name`, each scanned on its own: the pattern ids of its records
    ("plain"), of those the whole-word filter keeps ("kept"), of the leftmost-longest picks chained through exit -> entry
    over the unfiltered ("sel") and the filtered records ("fsel"), with the entry each selection starts from; and the same
    four for one scan of the whole ("whole")."""
    buf, pos, ids, lens, M = _chain_whole(path, para_path)
    ll = line_lengths(path)
    keep = wordref.filter_words(buf, pos, lens)
    whole = dict(plain=ids, kept=ids[keep], sel=ids[greedy(pos, lens, 0, buf.size)[0]],
                 fsel=ids[keep][greedy(pos[keep], lens[keep], 0, buf.size)[0]])
    o = Oracle(path, 1, 1)
    ranges, entry, fentry = [], 0, 0
    for a, b, part, prev, nxt in chain_parts(buf, chain_cuts(name, form, buf, pos, lens, M), M):
        ppos, pids = o.scan_spec(part)
        own = ppos < b - a
        ppos, pids = ppos[own].astype(np.int64), pids[own].astype(np.int64)
        plen = ll[pids]
        k = wordref.filter_words(part, ppos, plen, None, wordref.BOTH, prev, nxt)
        idx, ex = greedy(ppos, plen, entry, b - a)
        fidx, fex = greedy(ppos[k], plen[k], fentry, b - a)
        ranges.append(dict(plain=pids, kept=pids[k], sel=pids[idx], fsel=pids[k][fidx], entry=entry, fentry=fentry))
        entry, fentry = int(ex), int(fex)
    o.close()
    return dict(ranges=ranges, whole=whole, M=M)


@pytest.mark.parametrize("name", CUT_LISTS)
@pytest.mark.parametrize("form", range(len(CHAIN_FORMS)), ids=[f[0] for f in CHAIN_FORMS])
def test_chained_ranges_sum_to_the_whole_in_the_reference(form, name, resolve):
    pat = CHAIN_FORMS[form][0]
    path, para = resolve(pat), resolve("paragraph402")
    table = PfacTable.from_file(path, 256)
    ref = chain_reference(path, para, name, form)
    assert ref["M"] == table.max_pat_len
    whole = ref["whole"]
    assert 0 < whole["fsel"].size <= whole["kept"].size < whole["plain"].size and whole["fsel"].size != whole["sel"].size
    assert form == 0 or whole["sel"].size < whole["plain"].size      # (one-byte matches never overlap: every one is picked)
    for what in ("plain", "kept", "sel", "fsel"):
        total = sum(countref.state_counts(table, r[what]) for r in ref["ranges"])
        np.testing.assert_array_equal(total, countref.state_counts(table, whole[what]), err_msg=f"{pat} {name}: {what}")
        np.testing.assert_array_equal(sum(countref.pattern_counts(r[what], table.n_patterns) for r in ref["ranges"]),
                                      countref.pattern_counts(whole[what], table.n_patterns))
    if name == "fixed":
        sizes = [int(r["plain"].size) for r in ref["ranges"]]
        assert sizes[3] == 0 and len(sizes) == 7                # (the empty range)
