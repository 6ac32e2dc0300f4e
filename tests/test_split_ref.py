"""The references and the protocol of the delimiter-split and matching-documents tests, checked without a GPU: the numpy
reference of the split against the bytes.split one, the matching reference against a plain loop, the named cases'
preconditions, and the GPU tests' own checks (splitref.assert_split / assert_matching) run against a numpy stand-in of
the device code with seeded defects -- each defect must be caught by at least one case."""
import numpy as np
import pytest

import splitref
from splitref import (TILE, all_split_cases, assert_matching, assert_split, doc_first_case, matching_ids, matching_ids_loop,
                      split_offsets, split_offsets_pieces)

CASES = all_split_cases()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_numpy_reference_equals_pieces_reference(case):
    off, n_docs, tail = split_offsets(case.data, case.delim)
    off2, n_docs2, tail2 = split_offsets_pieces(case.data.tobytes(), case.delim)
    assert n_docs == n_docs2 and tail == tail2
    np.testing.assert_array_equal(off, off2)
    # the rules of pfac_records_segment hold by construction
    assert off[0] == 0 and off[-1] == case.n and bool((off[1:] >= off[:-1]).all())
    assert 0 <= tail <= case.n and (tail == case.n or case.data[-1] != case.delim)


def test_references_agree_on_seeded_random_inputs():
    rng = np.random.default_rng(20261018)
    for k in range(400):
        n = int(rng.integers(0, 300))
        delim = int(rng.integers(0, 256))
        alphabet = np.array([delim, delim ^ 1, (delim + 1) & 0xFF, int(rng.integers(0, 256))], dtype=np.uint8)
        data = alphabet[rng.integers(0, 4, n)] if k % 2 else rng.integers(0, 256, n).astype(np.uint8)
        off, n_docs, tail = split_offsets(data, delim)
        off2, n_docs2, tail2 = split_offsets_pieces(data.tobytes(), delim)
        assert (n_docs, tail) == (n_docs2, tail2), (k, n, delim)
        np.testing.assert_array_equal(off, off2)


def test_worked_examples():
    ex = lambda s: (split_offsets(np.frombuffer(s, np.uint8), 10)[0].tolist(),) + split_offsets(np.frombuffer(s, np.uint8), 10)[1:]   # noqa: E731
    assert ex(b"") == ([0], 0, 0)
    assert ex(b"\n") == ([0, 1], 1, 1)
    assert ex(b"a") == ([0, 1], 1, 0)
    assert ex(b"ab\n\n\ncd") == ([0, 3, 4, 5, 7], 4, 5)
    assert ex(b"ab\ncd\n") == ([0, 3, 6], 2, 6)


def test_case_preconditions():
    by = {c.name: c for c in CASES}
    assert len(by) == len(CASES)
    for n in splitref.LENGTHS:
        for d in splitref.DELIMS:
            c = by[f"len{n}_d{d:02x}"]
            assert c.n == n and (n < 4095 or int((c.data == d).sum()) > 10)
    assert not (by["no_delimiter"].data == 10).any()
    c = by["first_and_last_byte"]
    assert c.data[0] == 10 and c.data[-1] == 10 and split_offsets(c.data, 10)[2] == c.n
    c = by["tile_last_and_next_first"]
    assert c.data[TILE - 1] == 10 and c.data[TILE] == 10
    c = by["tile_of_delimiters"]                                   # more than 63 document starts in one tile: 4096
    off = split_offsets(c.data, 10)[0]
    assert int(((off >= TILE) & (off < 2 * TILE)).sum()) == TILE > 63
    for name, k in (("run_of_2", 2), ("run_of_64", 64), ("run_of_65", 65)):
        off, n_docs, _ = split_offsets(by[name].data, 10)
        assert n_docs == k + 1 and int((np.diff(off.astype(np.int64)) == 1).sum()) == k - 1
    c = by["delimiter_in_last_partial_chunk"]
    assert c.n % 16 and c.data[c.n - 2] == 10 and c.n - 2 >= c.n // 16 * 16
    assert by["only_delimiters_short"].n == 33 and (by["only_delimiters_short"].data == 10).all()
    for c in CASES:
        if c.need == "adversarial":
            d = c.delim
            assert set(np.unique(c.data).tolist()) <= {d, d ^ 1, d ^ 0x80, (d + 1) & 0xFF, (d - 1) & 0xFF}
            assert c.data[64] == d and c.data[65] == d ^ 1 and 100 < int((c.data == d).sum()) < c.n - 100
        assert c.storage(c.delim).size % TILE == 0 and c.storage(c.delim).size >= c.n + 16
    assert {c.delim for c in CASES if c.need == "adversarial"} >= {0x00, 0x01}


# ---------------------------------------------------------------------------
# the protocol against a stand-in with seeded defects

def haszero_mask(storage, delim):
    """The classic (x - 0x01..) & ~x & 0x80.. test per 32-bit word: flags a 0x01 byte above a zero byte as zero too."""
    w = np.ascontiguousarray(storage).view("<u4").astype(np.uint64)
    x = w ^ np.uint64(delim * 0x01010101)
    t = ((x - np.uint64(0x01010101)) & ~x & np.uint64(0x80808080)) & np.uint64(0xFFFFFFFF)
    return ((t[:, None] >> (np.arange(4, dtype=np.uint64) * np.uint64(8) + np.uint64(7))) & np.uint64(1)).astype(bool).ravel()


def stand_in(storage, n, delim, defect=None):
    """What the device code computes, in numpy, from the padded storage -- with one defect switched on."""
    read = n
    if defect == "last_partial_ignored":
        read = n // 16 * 16
    elif defect == "past_end_counted":
        read = (n + 15) // 16 * 16
    eq = haszero_mask(storage, delim) if defect == "haszero_swar" else (storage == delim)
    ends = (np.flatnonzero(eq[:read]) + 1).astype(np.uint64)
    open_tail = n > 0 and storage[n - 1] != delim
    closing = [n] if open_tail and defect != "closing_missing" else []
    off = np.concatenate([np.zeros(1, np.uint64), ends, np.array(closing, dtype=np.uint64)])
    n_docs = int(ends.size) + (1 if open_tail else 0)
    tail = (int(ends[-1]) if ends.size else 0) if open_tail else n
    if defect == "closing_missing" and open_tail:
        off = np.concatenate([off, np.zeros(1, np.uint64)])       # (the slot the missing store leaves as it was)
    return n_docs, tail, (lambda first, k: off[first:first + k])


def run_protocol(defect):
    """-> names of the cases whose check fails."""
    caught = []
    for case in CASES:
        for pad in (case.delim, case.delim ^ 0xFF):
            s = case.storage(pad)
            try:
                assert_split(case, pad, *stand_in(s, case.n, case.delim, defect))
            except AssertionError:
                caught.append(case.name)
                break
    return caught


def test_protocol_passes_a_correct_stand_in():
    assert run_protocol(None) == []


@pytest.mark.parametrize("defect, must_catch", [
    ("last_partial_ignored", "delimiter_in_last_partial_chunk"),
    ("past_end_counted", "len17_d0a"),
    ("haszero_swar", "adversarial_d00"),
    ("closing_missing", "no_delimiter"),
])
def test_protocol_catches_seeded_defects(defect, must_catch):
    caught = run_protocol(defect)
    assert must_catch in caught, (defect, caught)


def test_haszero_stand_in_really_miscounts():
    s = np.array([0, 1, 1, 0x80] + [7] * 12, dtype=np.uint8)
    assert haszero_mask(s, 0)[:4].tolist() == [True, True, True, False] and (s == 0)[:4].tolist() == [True, False, False, False]


# ---------------------------------------------------------------------------
# matching documents

@pytest.mark.parametrize("kind", splitref.MATCH_KINDS)
@pytest.mark.parametrize("n_docs", splitref.MATCH_DOCS)
def test_matching_reference_equals_loop(kind, n_docs):
    first = doc_first_case(kind, n_docs)
    assert first.size == n_docs + 1 and first[0] == 0 and bool((first[1:] >= first[:-1]).all())
    for invert in (False, True):
        ids = matching_ids(first, invert)
        np.testing.assert_array_equal(ids, matching_ids_loop(first, invert))
        assert_matching(ids, ids.size, first, invert)
    both = np.sort(np.concatenate([matching_ids(first, False), matching_ids(first, True)]))
    np.testing.assert_array_equal(both, np.arange(n_docs, dtype=np.uint64))
    n_match = matching_ids(first).size
    if kind == "all_empty":
        assert n_match == 0
    elif kind == "none_empty":
        assert n_match == n_docs
    elif n_docs > 1:
        assert 0 < n_match < n_docs                              # some documents, not all
    if kind == "runs" and n_docs > 4300:
        cnt = np.diff(first.astype(np.int64))
        assert not cnt[40:100].any() and cnt[100:140].all() and cnt[4000:4200].all() and not cnt[4200:4300].any()
        assert 40 < 64 < 100 and 4000 < 4096 < 4200              # the runs cross a block-of-64 edge and a group edge


def test_matching_check_catches_ids_out_of_order():
    first = doc_first_case("alternating", 200)
    ids = matching_ids(first)
    swapped = ids.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    with pytest.raises(AssertionError, match="ascend"):
        assert_matching(swapped, ids.size, first, False, "swapped")
    with pytest.raises(AssertionError):
        assert_matching(ids[::-1], ids.size, first, False, "reversed")
    with pytest.raises(AssertionError):
        assert_matching(ids, ids.size, first, True, "wrong polarity")
