"""Term counts per document without a GPU: the two references of tests/termref.py held against one another on every
case of tests/test_gpu_terms.py, the preconditions that make those cases test what they are named for, the reference
held against the CPU oracle's own scan of a small log, the four kinds of wrong result that `termref.check` must
refuse, and PfacTable.states_to_patterns."""
import numpy as np
import pytest

import docref
import passguard
import scoreref
import termref
from phfpfac_amd import PfacTable
from termref import BLOCK, EDGES, GROUP, SORT_BLOCK, cases, check, names, sort_passes, sort_shape, term_counts, term_counts_by_counter

ALL = [(W, name) for W in (2, 4) for name in names(W)]


def test_the_names_are_the_cases():
    for W in (2, 4):
        assert list(cases(W)) == names(W)


def test_the_tables_give_four_and_thirteen_state_bits():
    assert termref.num_final(2) == len(passguard.LINES16) == int(passguard.cpu().table(2).num_final)
    assert termref.state_bits(termref.num_final(2)) == 4
    assert termref.state_bits(termref.num_final(4)) == 13


@pytest.mark.parametrize("W,name", ALL, ids=[f"{W}-{n}" for W, n in ALL])
def test_the_two_references_agree(W, name):
    c = cases(W)[name]
    a, b = c.want(), term_counts_by_counter(c.states, c.first, c.num_final)
    for x, y, what in zip(a, b, ("row_ptr", "states", "counts")):
        assert x.dtype == y.dtype and np.array_equal(x, y), what
    check(a, *b)
    # the column sums are the histogram of the states, the row sums the documents' sizes
    np.testing.assert_array_equal(np.bincount(a[1], weights=a[2], minlength=c.num_final).astype(np.int64),
                                  np.bincount(c.states, minlength=c.num_final))
    rows = np.repeat(np.arange(c.n_docs), np.diff(a[0].astype(np.int64)))
    np.testing.assert_array_equal(np.bincount(rows, weights=a[2], minlength=c.n_docs).astype(np.int64), np.diff(c.first.astype(np.int64)))


def test_the_sizes_and_the_big_case():
    by = cases(2)
    assert [by[f"n{n}"].n for n in termref.SIZES] == list(termref.SIZES)
    assert by["n0"].n_docs > 0 and by["nodocs"].n_docs == 0 and by["nodocs"].n == 0
    big = by["big"]
    assert big.n == 1025 * 4096 + 1 and -(-big.n // GROUP) > 1024          # the group prefix works with two groups per thread
    chunks, n_blocks, trips = sort_shape(big.n)
    assert n_blocks > 4 and trips > 1                 # ... and the prefix over a digit's row with several trips and a carry
    assert sort_shape(1024) == (0, 0, 0) and sort_shape(1025) == (1, 2, 1) and sort_shape(4097)[1] == 5
    R = termref.SORT_ROWS
    assert sort_shape(1024 * R) == (1, R, R // 256) and sort_shape(1024 * R + 1) == (2, R // 2 + 1, -(-(R // 2 + 1) // 256))
    # several chunks per workgroup: the GPU test limits the workgroups to three (the PFAC_TERMS_ROWS knob)
    for name in termref.CHUNKED:
        chunks, n_blocks, _ = sort_shape(by[name].n, termref.CHUNKED_ROWS)
        assert chunks > 1 and 1 < n_blocks <= termref.CHUNKED_ROWS and chunks * n_blocks * SORT_BLOCK >= by[name].n
    assert sort_shape(by["big"].n, termref.CHUNKED_ROWS)[0] > 1000
    assert big.n * 8 < 35_000_000


def test_pass_counts_land_on_both_sides_of_every_step():
    seen = set()
    for W in (2, 4):
        got = tuple(cases(W)[f"passes-d{d}"].passes for d in termref.PASS_DOCS)
        assert got == termref.WANT_PASSES[W]
        for d, p in zip(termref.PASS_DOCS, got):
            c = cases(W)[f"passes-d{d}"]
            assert c.n > SORT_BLOCK and c.n_docs == d and p == sort_passes(d, c.num_final)
            assert int(np.diff(c.first.astype(np.int64))[-1]) > 0 and int(c.states.max()) == c.num_final - 1   # the key's top bits are used
            seen.add(p)
        for d in (17, 524289):
            assert cases(W)[f"passes-one-d{d}"].n <= SORT_BLOCK
    assert seen == {1, 2, 3, 4, 5}
    nf = termref.num_final(4)
    for lo, hi in ((16, 17), (2048, 2049), (524288, 524289)):                # one document more adds a pass
        assert any(sort_passes(hi, f) == sort_passes(lo, f) + 1 for f in (16, nf)), (lo, hi)


def test_runs_lie_across_every_kind_of_edge():
    c = cases(2)["run3000"]
    w = c.want()
    assert 3000 in w[2].tolist() and int(w[2].max()) == 3000
    for edge in EDGES:
        assert c.runs_across(edge) >= 1, edge
    assert cases(2)["equal"].want()[2].tolist() == [5000] and cases(2)["equal"].runs_across(GROUP) == 1
    d = cases(2)["distinct"]
    assert d.want()[1].size == d.n and (d.want()[2] == 1).all()
    assert cases(2)["big"].runs_across(BLOCK) > 100 and cases(2)["big"].runs_across(SORT_BLOCK) >= 1


@pytest.mark.parametrize("run", termref.EMPTY_RUNS)
def test_empty_documents_at_the_front_the_middle_a_block_edge_and_the_end(run):
    c = cases(2)[f"empty{run}"]
    runs = [r for r in c.empty_runs() if r[1] == run]
    assert len(runs) == 4
    (d0, _, i0), (_, _, i1), (_, _, i2), (d3, _, i3) = runs
    assert d0 == 0 and i0 == 0
    assert 0 < i1 < c.n and i1 % BLOCK != 0
    assert 0 < i2 < c.n and i2 % BLOCK == 0
    assert d3 + run == c.n_docs and i3 == c.n
    row = c.want()[0].astype(np.int64)
    assert (np.diff(row)[d0:d0 + run] == 0).all() and row[-1] == row[d3]


def test_input_orders():
    c = cases(2)["descending"]
    f = c.first.astype(np.int64)
    assert all((np.diff(c.states[a:b].astype(np.int64)) <= 0).all() for a, b in zip(f[:-1], f[1:]))
    assert any((np.diff(c.states[a:b].astype(np.int64)) < 0).any() for a, b in zip(f[:-1], f[1:]))
    s = cases(2)["same"]
    row, st, cnt = s.want()
    assert st.reshape(-1, 3).tolist() == [[2, 7, 11]] * s.n_docs and cnt.reshape(-1, 3).tolist() == [[1, 2, 1]] * s.n_docs


def test_row_sums_of_an_oracle_scan_are_the_score_counts():
    """A small log scanned document by document by the CPU oracle (docref): the matrix's row sums are scoreref's counts
    of the whole-buffer records cut by the header's rule, and its column sums the histogram of the kept ids."""
    x = passguard.cpu()
    key = x.size_key("t3")
    off = x.offsets(2, key, "rand")
    first, _, ids = docref.oracle_per_doc(x.tinfo(2)["matcher"], x.input(key[0])[:key[1]], off)
    n_ids = len(passguard.LINES16) + 1
    row, st, cnt = term_counts(ids, first, n_ids)
    pos, wids, lens = x.scan(2, key)
    sc = scoreref.scores_cut(pos, wids, lens, off, np.ones(n_ids, dtype=np.int64))
    np.testing.assert_array_equal(np.bincount(np.repeat(np.arange(off.size - 1), np.diff(row.astype(np.int64))), weights=cnt,
                                              minlength=off.size - 1).astype(np.uint64), sc["count"])
    np.testing.assert_array_equal(np.bincount(st, weights=cnt, minlength=n_ids).astype(np.int64), np.bincount(ids, minlength=n_ids))
    assert int(sc["count"].sum()) == ids.size > 1000


# ---------------------------------------------------------------------------
# wrong results of the kinds a kernel of this shape can give

def _heads(keys, also):
    h = np.concatenate([[True], keys[1:] != keys[:-1]]) if keys.size else np.zeros(0, dtype=bool)
    return h | also


def _from_heads(c, keys, heads):
    at = np.flatnonzero(heads)
    sb = termref.state_bits(c.num_final)
    cnt = np.diff(np.concatenate([at, [keys.size]]))
    row = np.searchsorted(at, c.first.astype(np.int64), side="left")
    return row.astype(np.uint64), (keys[at] & ((1 << sb) - 1)).astype(np.uint32), cnt.astype(np.uint32)


def test_the_reference_refuses_wrong_results():
    c = cases(2)["run3000"]
    keys = c.sorted_keys()
    none = np.zeros(keys.size, dtype=bool)
    good = _from_heads(c, keys, _heads(keys, none))
    check(c.want(), *good)
    # runs not merged across a block of 64
    with pytest.raises(AssertionError):
        check(c.want(), *_from_heads(c, keys, _heads(keys, np.arange(keys.size) % BLOCK == 0)))
    # row_ptr short by one group's sum
    row = good[0].copy()
    late = c.first.astype(np.int64) >= GROUP
    assert late.any() and not late.all()
    row[late] -= np.uint64(_heads(keys, none)[:GROUP].sum())
    with pytest.raises(AssertionError, match="row_ptr"):
        check(c.want(), row, good[1], good[2])
    # states unsorted inside a document (the pairs themselves are right)
    st, cnt = good[1].copy(), good[2].copy()
    assert int(good[0][1]) >= 2
    st[[0, 1]], cnt[[0, 1]] = st[[1, 0]], cnt[[1, 0]]
    with pytest.raises(AssertionError, match="ascend"):
        check(c.want(), good[0], st, cnt)
    # a count off by one on a run that lies across a sort block
    at = np.flatnonzero(_heads(keys, none))
    ends = np.concatenate([at[1:], [keys.size]])
    j = int(np.flatnonzero((at // SORT_BLOCK) != ((ends - 1) // SORT_BLOCK))[0])
    cnt = good[2].copy()
    cnt[j] -= 1
    with pytest.raises(AssertionError, match="counts"):
        check(c.want(), good[0], good[1], cnt)


# ---------------------------------------------------------------------------
# PfacTable.states_to_patterns

def test_states_to_patterns():
    t = PfacTable.from_bytes(b"abc\nxy\nq\n", 256)
    ids = t.states_to_patterns(np.arange(t.num_final, dtype=np.uint32))
    assert sorted(ids.tolist()) == [1, 2, 3] and np.array_equal(ids, np.asarray(t.idmap)[: t.num_final])
    assert t.states_to_patterns(np.empty(0, dtype=np.uint32)).size == 0
    with pytest.raises(ValueError):
        t.states_to_patterns([t.num_final])
    multi = PfacTable.from_charclass(b"[a-c]x\nax\nq\n", 256)
    with pytest.raises(ValueError, match="outputs"):
        multi.states_to_patterns([0])
    single = PfacTable.from_charclass(b"[a-c]x\nq\n", 256)
    assert sorted(single.states_to_patterns(np.arange(single.num_final)).tolist()) == [1, 2]
