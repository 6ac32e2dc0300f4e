"""The checker of the gather and of the context lines, checked on the host (no GPU): each numpy reference of
tests/gatherref.py against its second form on every named case and on 300 seeded ones, the preconditions the named
cases are there for, the shared checks against numpy stand-ins with seeded defects (each must be caught), and the new
entry points' presence in the built library and on GpuMatcher."""
import numpy as np
import pytest

import gatherref
from gatherref import (BLOCK, U64_MAX, WIN, all_gather_cases, assert_context, assert_gather, context_cases, context_ids,
                       context_ids_loop, context_windows, gather_ref, gather_ref_loop, sparse_first)
from splitref import doc_first_case, matching_ids

CASES = all_gather_cases()
LOOP_BUDGET = 300_000                   # documents x window the two-loop definition is run for (it is quadratic)


# ---------------------------------------------------------------------------
# the references against their second forms

@pytest.mark.parametrize("case", CASES, ids=repr)
def test_gather_reference_equals_the_slices(case):
    out, off = gather_ref(case.data, case.offsets, case.ids)
    lout, loff = gather_ref_loop(case.data, case.offsets, case.ids)
    np.testing.assert_array_equal(off, loff)
    assert bytes(out) == bytes(lout)
    assert_gather(case, int(lout.size), loff, lout, what="(the second reference)")


def test_gather_reference_on_seeded_cases():
    for seed in range(300):
        rng = np.random.default_rng([seed, 0x4741])
        n_docs = int(rng.integers(0, 60))
        lens = rng.integers(0, int(rng.choice([2, 18, 70])), n_docs)
        lead = int(rng.integers(0, 20))
        off = lead + np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)])
        data = rng.integers(0, 256, int(off[-1]) + int(rng.integers(0, 9))).astype(np.uint8)
        ids = rng.integers(0, n_docs, int(rng.integers(0, 90))) if n_docs else np.zeros(0, np.int64)
        out, ooff = gather_ref(data, off, ids)
        lout, loff = gather_ref_loop(data, off, ids)
        assert np.array_equal(ooff, loff) and bytes(out) == bytes(lout), seed


def test_context_reference_equals_the_definition():
    ran = 0
    for kind, n_docs, before, after in context_cases():
        if n_docs * (min(before, n_docs) + min(after, n_docs) + 1) > LOOP_BUDGET:
            continue                                               # (the seeded cases below cover wide windows at small n_docs)
        first = doc_first_case(kind, n_docs)
        assert np.array_equal(context_ids(first, before, after), context_ids_loop(first, before, after)), (kind, n_docs, before, after)
        ran += 1
    assert ran >= 150
    for seed in range(300):
        rng = np.random.default_rng([seed, 0x4358])
        n_docs = int(rng.integers(0, 200))
        first = sparse_first(n_docs, np.flatnonzero(rng.random(n_docs) < rng.choice([0.02, 0.2, 0.7])))
        before, after = (int(rng.choice([0, 1, 2, 5, 64, n_docs, n_docs + 7, U64_MAX])) for _ in range(2))
        assert np.array_equal(context_ids(first, before, after), context_ids_loop(first, before, after)), seed


def test_context_of_zero_is_the_plain_call():
    for kind, n_docs, _, _ in context_cases():
        first = doc_first_case(kind, n_docs)
        assert np.array_equal(context_ids(first, 0, 0), matching_ids(first))


# ---------------------------------------------------------------------------
# what the named cases are there for

def test_named_cases_meet_their_preconditions():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert sorted(c.n_ids for c in CASES if c.name.startswith("ids") and c.name[3:].isdigit()) == sorted(gatherref.N_IDS)
    seen_src, seen_cut, needs = set(), set(), set()
    for c in CASES:
        off = c.offsets.astype(np.int64)
        out, out_off = gather_ref(c.data, c.offsets, c.ids)
        out_off = out_off.astype(np.int64)
        need = c.need[0] if isinstance(c.need, tuple) else c.need
        needs.add(need)
        if need == "out_empty":
            assert out.size == 0 and c.n_ids > 0
        elif need == "segments_per_window":
            assert np.bincount(out_off[:-1] // WIN).max() >= WIN          # more than 1024 segments fall in one window ...
            assert np.bincount(out_off[:-1] // 16).max() >= 16            # ... and 16 documents start in one 16-byte chunk
        elif need in ("res0", "res5"):
            assert set((off[c.ids.astype(np.int64)] % 16).tolist()) == {int(need[3:])}
        elif need == "partial_tail":
            assert out.size % 16 != 0 and set(np.diff(off).tolist()) == {15, 16, 17}
        elif need == "long_doc":
            k = int(np.argmax(np.diff(out_off)))
            assert out_off[k + 1] // WIN - out_off[k] // WIN >= 4 and 0 < k < c.n_ids - 1      # it spans at least 5 windows
            assert out_off[k] % 16 != 0
        elif need == "whole_input":
            assert c.n_ids == 1 and out.size == c.n == 130 * 4096 + 5 and out.size // WIN >= 5
        elif need == "empty_blocks":
            assert (np.diff(out_off)[:40 * BLOCK] == 0).all() and out.size > 0      # whole blocks and groups of empty documents in front
        elif need == "ladder":
            _, src, cut = c.need
            assert off[int(c.ids[0])] % 16 == src and out_off[1] % 16 == cut
            seen_src.add((c.name.startswith("ladder"), src))
            seen_cut.add(cut)
        elif need == "id_list":
            assert c.n % 16 != 0 and off[-1] == c.n
            kind = c.need[1]
            ids = c.ids.astype(np.int64)
            if kind == "last_only":
                assert ids.tolist() == [c.n_docs - 1] and off[-1] // 16 * 16 < off[-1]       # it ends in the last partial input chunk
            elif kind == "reversed":
                assert (np.diff(ids) < 0).all()
            elif kind == "repeats":
                assert np.unique(ids).size < ids.size
            elif kind == "every_other":
                assert (np.diff(ids) == 2).all()
            else:
                assert ids.tolist() == list(range(c.n_docs))
    assert {s for _, s in seen_src} == set(range(16)) and seen_cut == set(range(16))
    assert needs >= {"out_empty", "segments_per_window", "res0", "res5", "partial_tail", "long_doc", "whole_input", "empty_blocks",
                     "ladder", "id_list", None}


def test_context_cases_drop_some_documents_and_keep_some():
    first = doc_first_case("runs", 4097)
    sparse = sparse_first(4097, [0, 500, 2000, 2003, 4096])
    for before, after in context_windows(4097)[1:7]:
        for f in (first, sparse) if before + after < 6 else (sparse,):     # (a wide window around the dense mix is everything)
            k = context_ids(f, before, after).size
            assert matching_ids(f).size < k < 4097, (before, after)
    assert context_ids(first, 4097, 4097).size == 4097 and context_ids(first, U64_MAX, U64_MAX).size == 4097
    assert context_ids(doc_first_case("all_empty", 4097), U64_MAX, U64_MAX).size == 0


# ---------------------------------------------------------------------------
# the checks catch seeded defects

def _lens(case):
    off = case.offsets.astype(np.int64)
    ids = case.ids.astype(np.int64)
    return off, ids, off[ids + 1] - off[ids]


def _right(case):
    out, out_off = gather_ref(case.data, case.offsets, case.ids)
    return int(out.size), out_off, np.concatenate([out, np.full(32, 0xA5, np.uint8)])


def defect_last_partial_chunk_not_written(case):
    n, off, buf = _right(case)
    buf[n // 16 * 16:n] = 0xA5
    return n, off, buf


def defect_byte_past_the_end(case):
    n, off, buf = _right(case)
    buf[n:(n + 15) // 16 * 16] = 0                                 # the last store rounded up to 16 bytes
    return n, off, buf


def defect_empty_document_shifts_its_successor(case):
    off, ids, lens = _lens(case)
    out_off = np.concatenate([[0], np.cumsum(np.maximum(lens, 1))])
    buf = np.full(int(out_off[-1]) + 32, 0xA5, np.uint8)
    for k, i in enumerate(ids):
        buf[out_off[k]:out_off[k] + lens[k]] = case.data[off[i]:off[i + 1]]
    return int(out_off[-1]), out_off, buf


def defect_source_read_from_the_aligned_address_below(case):
    off, ids, lens = _lens(case)
    n, out_off, buf = _right(case)
    for k, i in enumerate(ids):
        a = off[i] // 16 * 16
        buf[int(out_off[k]):int(out_off[k]) + lens[k]] = case.data[a:a + lens[k]]
    return n, out_off, buf


def defect_inclusive_offsets(case):
    n, out_off, buf = _right(case)
    return n, np.append(out_off[1:], out_off[-1]), buf


GATHER_DEFECTS = {
    defect_last_partial_chunk_not_written: "len_15_16_17",
    defect_byte_past_the_end: "len_15_16_17",
    defect_empty_document_shifts_its_successor: "ids1025",
    defect_source_read_from_the_aligned_address_below: "all_16_res5",
    defect_inclusive_offsets: "ids65",
}


@pytest.mark.parametrize("defect", list(GATHER_DEFECTS), ids=lambda f: f.__name__)
def test_assert_gather_catches(defect):
    case = next(c for c in CASES if c.name == GATHER_DEFECTS[defect])
    n, off, buf = _right(case)
    assert_gather(case, n, off, buf, fill=0xA5)                    # the stand-in without the defect passes
    with pytest.raises(AssertionError):
        assert_gather(case, *defect(case), fill=0xA5)


def _windows(first, before, after, clamp=True):
    n = len(first) - 1
    out = []
    for e in matching_ids(first).astype(np.int64).tolist():       # grep's own direction: `before` lines in front of a match
        lo, hi = e - before, e + after
        if not clamp and (lo < 0 or hi > n - 1):
            continue                                               # a window that leaves the input is dropped whole
        out.extend(range(max(lo, 0), min(hi, n - 1) + 1))
    return out


def defect_window_not_clamped(first, before, after):
    return np.unique(np.array(_windows(first, before, after, clamp=False), dtype=np.uint64))


def defect_before_and_after_swapped(first, before, after):
    return context_ids(first, after, before)


def defect_duplicates_where_windows_overlap(first, before, after):
    return np.array(sorted(_windows(first, before, after)), dtype=np.uint64)


CONTEXT_DEFECTS = {
    defect_window_not_clamped: (sparse_first(100, [0, 50, 99]), 2, 3),
    defect_before_and_after_swapped: (sparse_first(100, [10, 50]), 1, 4),
    defect_duplicates_where_windows_overlap: (sparse_first(100, [10, 12, 50]), 2, 3),
}


@pytest.mark.parametrize("defect", list(CONTEXT_DEFECTS), ids=lambda f: f.__name__)
def test_assert_context_catches(defect):
    first, before, after = CONTEXT_DEFECTS[defect]
    right = np.unique(np.array(_windows(first, before, after), dtype=np.uint64))    # a third form, from the matches outwards
    assert_context(right, right.size, first, before, after)
    got = defect(first, before, after)
    with pytest.raises(AssertionError):
        assert_context(got, got.size, first, before, after)


# ---------------------------------------------------------------------------
# the entry points exist

NEW_SYMBOLS = ("pfac_documents_matching_context", "pfac_documents_gather", "pfac_documents_gather_d2h",
               "pfac_documents_gather_offsets_d2h")
NEW_METHODS = ("gather_documents", "gathered_to_host", "gathered_offsets_to_host", "grep_lines")


def test_the_library_exports_the_calls_and_the_matcher_has_the_methods():
    import inspect

    from phfpfac_amd import GpuMatcher, _ffi
    lib = _ffi.hip_lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _ffi.HIP_SYMBOLS, name
    for name in NEW_METHODS:
        assert callable(getattr(GpuMatcher, name, None)), name
    params = inspect.signature(GpuMatcher.matching_documents).parameters
    assert params["before"].default == 0 and params["after"].default == 0
