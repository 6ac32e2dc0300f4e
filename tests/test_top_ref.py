"""The rank reference against itself, without a GPU: tests/topref.py's two references agree on every case that
tests/test_gpu_top.py runs, and every case has the properties it is named for -- so a pass on the GPU cannot be vacuous."""
import numpy as np
import pytest

from phfpfac_amd import _ffi
from scoreref import U64_MAX, predicate, predicate_loop
from topref import (BLOCK, BY_COUNT, CASE_IDS, GROUP, LOWEST, RANKED, SORT_BLOCK, SORT_SIZES, WORKGROUP, case, key_word, ks_of,
                    ranking, ranking_py, sort_case, tie_class, top, top_heap)


def test_the_constants_are_the_products():
    assert (BY_COUNT, LOWEST, RANKED) == (_ffi.PFAC_TOP_BY_COUNT, _ffi.PFAC_TOP_LOWEST, _ffi.PFAC_TOP_RANKED)
    assert SORT_BLOCK == _ffi.PFAC_TOP_SORT_BLOCK
    assert {"pfac_documents_top_scores", "pfac_documents_top_scores_d2h"} <= set(_ffi.HIP_SYMBOLS)
    from phfpfac_amd import GpuMatcher
    for name in ("top_documents", "top_scores_to_host", "top_lines", "top_scored_documents"):
        assert callable(getattr(GpuMatcher, name))


@pytest.mark.parametrize("n,keys,rule", CASE_IDS, ids=[f"{n}-{k}-{r}" for n, k, r in CASE_IDS])
def test_references_agree(n, keys, rule):
    c = case(n, keys, rule)
    if n <= 4097:
        np.testing.assert_array_equal(c.cand, predicate_loop(c.sc, c.off, **c.kw))
    for flags in (0, BY_COUNT, LOWEST, BY_COUNT | LOWEST):
        rank = c.rank(flags)
        np.testing.assert_array_equal(rank, ranking_py(c.sc, c.cand, flags), err_msg=f"{c} flags {flags}")
        ks = ks_of(c.sc, rank, flags)
        assert {0, 1, U64_MAX, rank.size + 1} <= set(ks)
        k = ks[len(ks) // 2]
        np.testing.assert_array_equal(top(rank, k, flags | RANKED)[0], top_heap(c.sc, c.cand, flags, k))
        ids, n_top = top(rank, k, flags)
        assert n_top == min(k, c.cand.size) and (np.diff(ids.astype(np.int64)) > 0).all()
        assert set(ids.tolist()) == set(top(rank, k, flags | RANKED)[0].tolist())


def straddles(ids, edge):
    """The ids lie in more than one unit of `edge` documents."""
    u = np.unique(ids.astype(np.int64) // edge)
    return u.size > 1


def test_tie_classes_lie_where_the_kernels_change_path():
    """The tie-heavy case past a workgroup: k cuts inside a class, that class has members in several 64-document
    blocks, in several groups (a wave's range and its prefix) and in two workgroups, and more members than `need` --
    under all four key orders."""
    c = case(WORKGROUP + 70, "ties", "all")
    for flags in (0, BY_COUNT, LOWEST, BY_COUNT | LOWEST):
        rank = c.rank(flags)
        b, e = tie_class(c.sc, rank, flags)
        k = (b + e) // 2
        assert b < k < e and k in ks_of(c.sc, rank, flags)
        need = k - b
        members = rank[b:e]
        assert 0 < need < members.size
        assert (np.diff(members.astype(np.int64)) > 0).all()                    # ties in id order
        taken, left = members[:need], members[need:]
        for edge in (BLOCK, GROUP):
            assert straddles(members, edge) and straddles(taken, edge) and straddles(left, edge), (flags, edge)
        assert straddles(members, WORKGROUP)                        # (the members not taken reach into the second workgroup)
        # the cut does not fall on a block's or a group's edge
        assert int(taken[-1]) // BLOCK == int(left[0]) // BLOCK or int(left[0]) % BLOCK != 0


@pytest.mark.parametrize("n", [4097, WORKGROUP + 70])
def test_digit_sets_differ_in_one_digit_only(n):
    """byte<p>: all keys agree outside byte p of the key word, under both keys; p = 7 is the select's first digit and the
    sort's last, p = 0 the other way round."""
    for p in range(8):
        c = case(n, f"byte{p}", "all")
        for flags in (0, BY_COUNT):
            w = key_word(c.sc, flags)
            diff = np.bitwise_or.reduce(w ^ w[0])
            assert diff != 0 and (int(diff) & ~(0xFF << (8 * p))) == 0, (p, flags)
            values, sizes = np.unique(w, return_counts=True)
            assert values.size > 100 and sizes.max() > n // 4       # many keys, and one large class among them
    c = case(n, "extremes", "all")
    assert (c.sc["count"] >= np.uint64(2 ** 63)).any() and (c.sc["count"] < np.uint64(2 ** 63)).any()
    assert {int(x) for x in np.unique(c.sc["score"])} == {-(2 ** 63), -1, 0, 1, 2 ** 63 - 1}


def test_rules_leave_fewer_candidates_than_documents():
    c = case(4097, "sparse", "matched")
    assert 0 < c.cand.size < 4097 // 10 and int((c.sc["count"] == 0).sum()) > 4000
    assert predicate(c.sc, min_count=1).size == c.cand.size
    c = case(WORKGROUP + 70, "extremes", "dense")
    lens = np.diff(c.off).astype(object)
    prod = np.abs(c.sc["score"].astype(object) * (2 ** 63 + 5))
    assert (prod >= 2 ** 63).any() and (lens * 2 ** 40 >= 2 ** 63).any() and 0 < c.cand.size < c.n
    c = case(4097, "sparse", "inverted")
    assert c.cand.size == int((c.sc["count"] == 0).sum())
    c = case(65, "ties", "dense-inverted")
    assert 0 < c.cand.size <= 65


@pytest.mark.parametrize("n_top", SORT_SIZES)
def test_sort_cases_have_classes_across_blocks(n_top):
    sc = sort_case(n_top)
    cand = np.arange(sc.size, dtype=np.uint64)
    for flags in (0, BY_COUNT | LOWEST):
        rank = ranking(sc, cand, flags)
        np.testing.assert_array_equal(rank, ranking_py(sc, cand, flags))
        ids, got = top(rank, n_top, flags | RANKED)
        assert got == n_top
        w = key_word(sc, flags)[ids.astype(np.int64)]
        assert (np.diff(w.astype(object)) >= 0).all() and np.unique(w).size >= 2
        b, e = tie_class(sc, rank, flags, at=n_top - 1)
        assert b < n_top < e                                        # k cuts the last class
        if n_top > SORT_BLOCK:
            w_in = key_word(sc, flags)[np.sort(ids).astype(np.int64)]  # the entries as the compaction delivers them
            at = np.flatnonzero(w_in == w_in[-1])
            assert at[0] // SORT_BLOCK != at[-1] // SORT_BLOCK      # a class enters the sort in more than one block
