"""The rank over document scores on the GPU (run with -m gpu on an MI355X): pfac_documents_top_scores and
pfac_documents_top_scores_d2h against tests/topref.py, whose cases tests/test_top_ref.py holds against a second
reference and checks for their preconditions without a GPU.  Most cases feed host-made scores through d_scores, as the
predicate's tests do: no scan, small shapes.  Integer work: bit-exact.  No expectation comes from the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import topref
from fmtref import Fmt, format_ref
from heapguard import FILLS, GuardedBuffer
from phfpfac_amd import SCORE_DTYPE, GpuMatcher, PfacError, PfacTable
from phfpfac_amd import _ffi
from scoreref import I64_MAX, I64_MIN, U64_MAX, make
from splitref import split_offsets
from topref import (ALL_FLAGS, BY_COUNT, CASE_IDS, LOWEST, RANKED, SORT_SIZES, case, ks_of, ranking, sort_case, tie_class, top)

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_OVERFLOW = _ffi.PFAC_E_ARG, _ffi.PFAC_E_STATE, _ffi.PFAC_E_OVERFLOW


def status_of(fn):
    with pytest.raises(PfacError) as e:
        fn()
    return e.value.status


def upload(arr, slack=0):
    raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
    t = torch.zeros(max(raw.size + slack, 16), dtype=torch.uint8, device="cuda:0")
    if raw.size:
        t[:raw.size].copy_(torch.from_numpy(raw.copy()))
    torch.cuda.synchronize()
    return t


def flag_kw(flags):
    return dict(by="count" if flags & BY_COUNT else "score", lowest=bool(flags & LOWEST), ranked=bool(flags & RANKED))


def same_pairs(got, want, what=""):
    assert got.dtype == SCORE_DTYPE and got.size == want.size, what
    for f in ("score", "count"):
        ne = np.flatnonzero(got[f] != want[f])
        assert ne.size == 0, f"{what}: {ne.size} of {want.size} {f}s differ, first at entry {int(ne[0])}: {int(got[f][ne[0]])}, want {int(want[f][ne[0]])}"


@pytest.fixture(scope="module")
def g():
    with GpuMatcher(0, 1) as m:
        yield m


def run(g, sc, d_sc, k, flags, want_ids, what, **kw):
    """One call into the slot's buffers, checked against the reference's ids: the count, the ids, the pairs."""
    n = g.top_documents(sc.size, k, d_scores=d_sc, **flag_kw(flags), **kw)
    assert n == want_ids.size, f"{what}: n_top {n}, want {want_ids.size}"
    ids = g.matching_documents_to_host(n)
    ne = np.flatnonzero(ids != want_ids)
    assert ne.size == 0, f"{what}: {ne.size} of {n} ids differ, first at rank {int(ne[0])}: {int(ids[ne[0]])}, want {int(want_ids[ne[0]])}"
    pairs = g.top_scores_to_host(n)
    same_pairs(pairs, sc[want_ids.astype(np.int64)], what)
    return ids, pairs


# ---------------------------------------------------------------------------
# sizes x key sets x rules x flags x k

@pytest.mark.parametrize("n,keys,rule", CASE_IDS, ids=[f"{n}-{k}-{r}" for n, k, r in CASE_IDS])
def test_top_equals_reference(g, n, keys, rule):
    """Every k of topref.ks_of under all eight flag combinations; one k of each combination twice, byte for byte."""
    c = case(n, keys, rule)
    d_sc = upload(c.sc)
    d_off = None if c.off is None else upload(c.off)
    seen = set()
    for flags in ALL_FLAGS:
        rank = c.rank(flags)
        ks = ks_of(c.sc, rank, flags)
        for k in ks:
            want, n_top = top(rank, k, flags)
            run(g, c.sc, d_sc, k, flags, want, f"{c} flags {flags} k {k}", d_doc_offsets=d_off, **c.kw)
            seen.add(n_top)
        b, e = tie_class(c.sc, rank, flags)
        k = (b + e) // 2 if e - b > 1 else max(rank.size - 1, 1)
        want, _ = top(rank, k, flags)
        first = run(g, c.sc, d_sc, k, flags, want, f"{c} flags {flags} k {k}, first run", d_doc_offsets=d_off, **c.kw)
        again = run(g, c.sc, d_sc, k, flags, want, f"{c} flags {flags} k {k}, second run", d_doc_offsets=d_off, **c.kw)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    assert 0 in seen and c.cand.size in seen


def test_all_equal_keys_give_the_first_ids(g):
    sc = topref.keyset("equal", 4097)
    d_sc = upload(sc)
    for flags in ALL_FLAGS:
        for k in (1, 64, 65, 4096, 4097, 5000):
            run(g, sc, d_sc, k, flags, np.arange(min(k, 4097), dtype=np.uint64), f"flags {flags} k {k}")


def test_candidates_fewer_than_k(g):
    """min_count = 1 on scores that are mostly {0, 0}: the call reports the candidates and no {0, 0}."""
    c = case(4097, "sparse", "matched")
    d_sc = upload(c.sc)
    for flags in ALL_FLAGS:
        want, n_top = top(c.rank(flags), 1000, flags)
        assert n_top == c.cand.size < 1000
        _, pairs = run(g, c.sc, d_sc, 1000, flags, want, f"flags {flags}", min_count=1)
        assert (pairs["count"] >= 1).all()
    # without the rule the same k fills up with them
    rank = ranking(c.sc, np.arange(c.n, dtype=np.uint64), BY_COUNT)
    _, pairs = run(g, c.sc, d_sc, 1000, BY_COUNT | RANKED, top(rank, 1000, RANKED)[0], "no rule")
    assert int((pairs["count"] == 0).sum()) == 1000 - c.cand.size


@pytest.mark.parametrize("n_top", SORT_SIZES)
def test_sort_block_edges(g, n_top):
    """n_top one below, at and one above the sort's block size, and the same for two blocks; three key values, so every
    class spans the blocks and must keep ascending ids."""
    sc = sort_case(n_top)
    d_sc = upload(sc)
    cand = np.arange(sc.size, dtype=np.uint64)
    for flags in (RANKED, RANKED | BY_COUNT | LOWEST, RANKED | LOWEST, 0):
        want, n = top(ranking(sc, cand, flags), n_top, flags)
        assert n == n_top
        a = run(g, sc, d_sc, n_top, flags, want, f"n_top {n_top} flags {flags}")
        b = run(g, sc, d_sc, n_top, flags, want, f"n_top {n_top} flags {flags} again")
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---------------------------------------------------------------------------
# buffers and errors

@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("flags", [0, RANKED, RANKED | BY_COUNT, LOWEST])
def test_callers_buffers_at_exact_capacity(g, fill, flags):
    c = case(4097, "ties", "window")
    d_sc = upload(c.sc)
    rank = c.rank(flags)
    b, e = tie_class(c.sc, rank, flags)
    for k in ((b + e) // 2, 1, rank.size + 5):
        want, n_top = top(rank, k, flags)
        ids, prs = GuardedBuffer(n_top * 8, fill=fill), GuardedBuffer(n_top * 16, fill=fill)
        # one too small: the exact count, nothing written
        with pytest.raises(PfacError) as err:
            g.top_documents(c.n, k, d_scores=d_sc, d_out=ids.ptr, d_top_scores=prs.ptr, out_cap=n_top - 1, **flag_kw(flags), **c.kw)
        assert err.value.status == E_OVERFLOW and err.value.n_top == n_top
        g.sync()
        ids.check(payload_untouched=True, what="d_ids_out after an overflow")
        prs.check(payload_untouched=True, what="d_top_scores_out after an overflow")
        # (a failed call discards the slot-owned results)
        assert status_of(lambda: g.matching_documents_to_host(1)) == E_STATE
        assert status_of(lambda: g.top_scores_to_host(0)) == E_STATE
        assert g.top_documents(c.n, k, d_scores=d_sc, d_out=ids.ptr, d_top_scores=prs.ptr, out_cap=n_top, **flag_kw(flags), **c.kw) == n_top
        g.sync()
        ids.check(what="d_ids_out")
        prs.check(what="d_top_scores_out")
        np.testing.assert_array_equal(ids.host().view(np.uint64), want)
        same_pairs(prs.host().view(SCORE_DTYPE), c.sc[want.astype(np.int64)], f"flags {flags} k {k}")
        # they went to the caller's buffers
        assert status_of(lambda: g.matching_documents_to_host(n_top)) == E_STATE
        assert status_of(lambda: g.top_scores_to_host(n_top)) == E_STATE
        # one caller's buffer and one of the slot's
        assert g.top_documents(c.n, k, d_scores=d_sc, d_top_scores=prs.ptr, out_cap=n_top, **flag_kw(flags), **c.kw) == n_top
        np.testing.assert_array_equal(g.matching_documents_to_host(n_top), want)
        assert status_of(lambda: g.top_scores_to_host(n_top)) == E_STATE
        prs.check(what="d_top_scores_out alone")
        with pytest.raises(PfacError) as err:
            g.top_documents(c.n, k, d_scores=d_sc, d_top_scores=prs.ptr, out_cap=n_top - 1, **flag_kw(flags), **c.kw)
        assert err.value.status == E_OVERFLOW and err.value.n_top == n_top


def test_arguments_and_state():
    sc = make(np.array([5, -2, 5, 0], dtype=np.int64), np.array([1, 2, 3, 0], dtype=np.uint64))
    with GpuMatcher(0, 1) as g:
        L, ctx = g._L, g._ctx
        d_sc = upload(sc)
        p = int(d_sc.data_ptr())
        n = C.c_uint64(7)
        rule = _ffi.CScoreRule(I64_MIN, I64_MAX, 1, U64_MAX, 0, 0)
        dens = _ffi.CScoreRule(I64_MIN, I64_MAX, 0, U64_MAX, 1, 1000)

        def call(scores=p, off=None, n_docs=4, r=None, rflags=0, k=2, flags=0, ids=None, cap=0, prs=None):
            return L.pfac_documents_top_scores(ctx, 0, scores, off, n_docs, None if r is None else C.byref(r), rflags, k, flags, ids, cap,
                                               prs, C.byref(n))
        # no scores in the slot
        assert call(scores=None) == E_STATE and n.value == 0
        assert status_of(lambda: g.top_documents(4, 2)) == E_STATE
        assert status_of(lambda: g.top_scores_to_host(0)) == E_STATE
        # a density without offsets: the state comes before the arguments
        assert call(r=dens, flags=8) == E_STATE
        # arguments
        assert call(flags=8) == E_ARG and call(flags=1 << 31) == E_ARG
        assert call(r=rule, rflags=2) == E_ARG
        assert call(scores=p + 8) == E_ARG
        assert call(n_docs=1 << 32) == E_ARG
        assert call(ids=p + 4, cap=4) == E_ARG
        assert call(prs=p + 8, cap=4) == E_ARG
        assert call(r=dens, off=p + 4) == E_ARG
        assert L.pfac_documents_top_scores(ctx, 0, p, None, 4, None, 0, 2, 0, None, 0, None, None) == E_ARG
        assert L.pfac_documents_top_scores(ctx, 1, p, None, 4, None, 0, 2, 0, None, 0, None, C.byref(n)) == E_ARG
        # k == 0 and n_docs == 0 give 0 and a fetchable, empty result
        assert call(k=0) == 0 and n.value == 0
        assert g.matching_documents_to_host(0).size == 0 and g.top_scores_to_host(0).size == 0
        assert call(n_docs=0) == 0 and n.value == 0
        # with rule == NULL the rule's flags are not read as a rule, yet they must be legal
        assert call(rflags=1, k=U64_MAX, flags=RANKED) == 0 and n.value == 4
        assert g.matching_documents_to_host(4).tolist() == [0, 2, 3, 1]
        same_pairs(g.top_scores_to_host(4), sc[[0, 2, 3, 1]])
        same_pairs(g.top_scores_to_host(2, first=1), sc[[2, 3]])
        assert g.top_scores_to_host(0, first=4).size == 0
        assert status_of(lambda: g.top_scores_to_host(2, first=3)) == E_ARG
        assert status_of(lambda: g.top_scores_to_host(5)) == E_ARG
        # a failed call discards both slot-owned results
        assert call(flags=8) == E_ARG
        assert status_of(lambda: g.matching_documents_to_host(4)) == E_STATE
        assert status_of(lambda: g.top_scores_to_host(4)) == E_STATE
        # the Python layer's own checks
        with pytest.raises(ValueError):
            g.top_documents(4, 2, by="density", d_scores=d_sc)
        with pytest.raises(ValueError):
            g.top_documents(4, -1, d_scores=d_sc)
        with pytest.raises(ValueError):
            g.top_documents(4, 1, density=(1, 0), d_scores=d_sc)


# ---------------------------------------------------------------------------
# end to end: the small log of the score tests

LINES = [b"GET /index.html 200 alice",          # 0: GET, alice
         b"POST /login 403 bob",                # 1: 403, bob
         b"",                                   # 2
         b"GET /admin 500 root error",          # 3: GET, root, error
         b"error: disk full",                   # 4: error
         b"alice and bob",                      # 5: alice, bob
         b"nothing here",                       # 6
         b"error error alice root",             # 7: error x 2, alice, root
         b"assassin bob",                       # 8: ass x 2, assassin, bob
         b"root root root",                     # 9: root x 3
         b"GET 403 GET",                        # 10: GET x 2, 403
         b"errors and assassins"]               # 11: error, ass x 2, assassin
#            id:   1      2    3      4     5    6    7    8
PATS = b"alice\nbob\nerror\nroot\nGET\n403\nass\nassassin\n"
WEIGHTS = [0, 1, 1, -2, 5, 0, -5, 2, 10]
LOG = np.frombuffer(b"\n".join(LINES) + b"\n" + b"bob error", dtype=np.uint8)          # 12: bob, error (no newline)
SCORE = [1, -4, 0, 3, -2, 2, 0, 2, 15, 15, -5, 12, -1]
COUNT = [2, 2, 0, 3, 1, 2, 0, 4, 4, 3, 3, 4, 2]
SCORE_NO = [1, -4, 0, 3, -2, 2, 0, 2, 11, 15, -5, 8, -1]       # non-overlapping: "assassin" is one pick
COUNT_NO = [2, 2, 0, 3, 1, 2, 0, 4, 2, 3, 3, 2, 2]
SCORE_WW = [1, -4, 0, 3, -2, 2, 0, 2, 11, 15, -5, 0, -1]       # whole words: "errors", "assassins" and the "ass" inside go
COUNT_WW = [2, 2, 0, 3, 1, 2, 0, 4, 2, 3, 3, 0, 2]


def test_the_best_lines_of_a_small_log():
    off = split_offsets(LOG, 0x0A)[0]
    want = make(SCORE, COUNT)
    nd = off.size - 1
    assert nd == 13
    t = PfacTable.from_bytes(PATS, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(t)
        g.set_pattern_weights(WEIGHTS)
        got_off, got = g.score_lines(LOG)
        np.testing.assert_array_equal(got_off, off)
        same_pairs(got, want, "score_lines")
        # the three best scores, in rank order: the tie of lines 8 and 9 goes to the smaller id
        assert g.top_documents(nd, 3) == 3
        assert g.matching_documents_to_host(3).tolist() == [8, 9, 11]
        same_pairs(g.top_scores_to_host(3), want[[8, 9, 11]])
        out_bytes = g.gather_documents(nd, 3, LOG.size)
        assert bytes(g.gathered_to_host(out_bytes)) == b"assassin bob\nroot root root\nerrors and assassins\n"
        out_bytes = g.gather_documents_formatted(nd, 3, LOG.size, number=True)
        assert bytes(g.gathered_to_host(out_bytes)) == b"9:assassin bob\n10:root root root\n12:errors and assassins\n"
        # the four largest counts: 4 at lines 7, 8 and 11, then the first of the lines with 3
        assert g.top_documents(nd, 4, by="count") == 4
        assert g.matching_documents_to_host(4).tolist() == [7, 8, 11, 3]
        out_bytes = g.gather_documents(nd, 4, LOG.size)
        assert bytes(g.gathered_to_host(out_bytes)) == (b"error error alice root\nassassin bob\nerrors and assassins\n"
                                                        b"GET /admin 500 root error\n")
        np.testing.assert_array_equal(g.gathered_offsets_to_host(4), [0, 23, 36, 57, 83])
        # the same set in document order, as grep prints, with its separators
        assert g.top_documents(nd, 4, by="count", ranked=False) == 4
        ids = g.matching_documents_to_host(4)
        assert ids.tolist() == [3, 7, 8, 11]
        same_pairs(g.top_scores_to_host(4), want[[3, 7, 8, 11]])
        fmt = Fmt(number=True, terminate=0x0A, group_sep=b"--\n")
        out_bytes = g.gather_documents_formatted(nd, 4, LOG.size, **fmt.kwargs())
        ref_out, ref_off = format_ref(LOG, off, ids, fmt)
        np.testing.assert_array_equal(g.gathered_to_host(out_bytes), ref_out)
        np.testing.assert_array_equal(g.gathered_offsets_to_host(4), ref_off)
        assert bytes(ref_out) == b"4:GET /admin 500 root error\n--\n8:error error alice root\n9:assassin bob\n--\n12:errors and assassins\n"
        # the two worst scores among the matched lines
        assert g.top_documents(nd, 2, lowest=True, min_count=1) == 2
        assert g.matching_documents_to_host(2).tolist() == [10, 1]
        # a density: at least one point per two bytes -- lines 8, 9 and 11 -- and the best of them by count
        assert g.top_documents(nd, 2, by="count", density=(1, 2), min_count=1) == 2
        assert g.matching_documents_to_host(2).tolist() == [8, 11]
        # more asked for than there is
        assert g.top_documents(nd, 100, min_score=12) == 3
        # one pass with the matching calls: a matching call replaces the ids, the pairs stay
        assert g.top_documents(nd, 3) == 3
        n = g.matching_documents_scored(nd, min_count=4)
        assert g.matching_documents_to_host(n).tolist() == [7, 8, 11]
        same_pairs(g.top_scores_to_host(3), want[[8, 9, 11]])
        small = upload(np.zeros(2))
        assert status_of(lambda: g.matching_documents_scored(nd, min_count=1, out_cap=0, d_out=small)) == E_OVERFLOW
        assert status_of(lambda: g.matching_documents_to_host(0)) == E_STATE
        same_pairs(g.top_scores_to_host(3), want[[8, 9, 11]])

        # the conveniences
        out, out_off, ids, pairs = g.top_lines(LOG, 3)
        assert ids.tolist() == [8, 9, 11] and bytes(out) == b"assassin bob\nroot root root\nerrors and assassins\n"
        np.testing.assert_array_equal(out_off, [0, 13, 28, 49])
        same_pairs(pairs, want[[8, 9, 11]])
        out, out_off, ids, pairs = g.top_lines(LOG, 3, non_overlapping=True)
        assert ids.tolist() == [9, 8, 11] and bytes(out) == b"root root root\nassassin bob\nerrors and assassins\n"
        same_pairs(pairs, make(SCORE_NO, COUNT_NO)[[9, 8, 11]])
        out, out_off, ids, pairs = g.top_lines(LOG, 3, whole_words=True)
        assert ids.tolist() == [9, 8, 3] and bytes(out) == b"root root root\nassassin bob\nGET /admin 500 root error\n"
        same_pairs(pairs, make(SCORE_WW, COUNT_WW)[[9, 8, 3]])
        out, out_off, ids, pairs = g.top_lines(LOG, 2, by="count", ranked=False, min_score=3)
        assert ids.tolist() == [8, 11] and bytes(out) == b"assassin bob\nerrors and assassins\n"
        docs = [bytes(LOG[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])]
        ids, pairs = g.top_scored_documents(docs, 4, by="count")
        assert ids.tolist() == [7, 8, 11, 3]
        same_pairs(pairs, want[[7, 8, 11, 3]])
        ids, pairs = g.top_scored_documents(docs, 2, non_overlapping=True, lowest=True, min_count=1)
        assert ids.tolist() == [10, 1]


def test_on_a_folded_scan():
    lines = [b"ERROR Error", b"error", b"none", b"eRRor x error ERROR", b"Error"]
    data = np.frombuffer(b"\n".join(lines) + b"\n", dtype=np.uint8)
    t = PfacTable.from_bytes(b"error\n", 256, ignore_case=True)
    with GpuMatcher(0, 1) as g:
        g.load_table(t)
        assert g.case_fold
        g.set_pattern_weights([0, 2])
        out, out_off, ids, pairs = g.top_lines(data, 3, by="count")
        assert ids.tolist() == [3, 0, 1] and pairs["count"].tolist() == [3, 2, 1] and pairs["score"].tolist() == [6, 4, 2]
        assert bytes(out) == b"eRRor x error ERROR\nERROR Error\nerror\n"
