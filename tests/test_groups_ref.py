"""Pattern groups without a GPU: PfacTable.state_group_masks, the references of tests/groupref.py held against one
another (the per-document oracle, bytes.find, the cut by hand; oracle/charclass_oracle.py for a class table), the
preconditions of every case of tests/test_gpu_groups.py, and the predicate's truth table."""
import importlib.util
import itertools
import os

import numpy as np
import pytest

from groupref import ALL, SHAPES, TILES, cases, groups_for, masks_by_find, masks_by_id, masks_cut, masks_per_doc, predicate, predicate_loop
from passguard import cut_by_hand
from phfpfac_amd import PfacTable
from splitref import matching_ids

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("charclass_oracle", os.path.join(REPO, "oracle", "charclass_oracle.py"))
cco = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cco)

CLASS_PATTERNS = b"[a-c]x\nax\n[^a-z0-9 ]\nq[0-9][0-9]\n[a-c]\nax[xy]\n[a-c]x\n"     # "ax" ends patterns 1, 2 and 7 in one state


# ---------------------------------------------------------------------------
# state_group_masks

def test_literal_table_takes_the_groups_of_idmap():
    t = PfacTable.from_bytes(b"he\nshe\nhis\nhers\nxyz\n", 256)
    groups = [None, 0, 63, (1, 2), None, [5]]                   # group 0, group 63, two groups, ungrouped, an iterable
    m = t.state_group_masks(groups)
    assert m.dtype == np.uint64 and m.size == t.num_final
    by_id = masks_by_id(groups)
    assert by_id.tolist() == [0, 1, 1 << 63, 6, 0, 32]
    np.testing.assert_array_equal(m, by_id[np.asarray(t.idmap, dtype=np.int64)])
    assert sorted(m.tolist()) == sorted(by_id[1:].tolist())
    # ready masks, as a uint64 array
    np.testing.assert_array_equal(t.state_group_masks(by_id), m)
    np.testing.assert_array_equal(t.state_group_masks(np.array(groups_for(5), dtype=object)), t.state_group_masks(groups_for(5)))


def test_duplicate_lines_take_the_winning_lines_groups():
    t = PfacTable.from_bytes(b"abc\nxy\nabc\n", 256)
    groups = [None, 3, 4, 9]
    m = t.state_group_masks(groups)
    reach = t.final_lengths() >= 1
    ids = np.asarray(t.idmap, dtype=np.int64)
    win = int(ids[reach][[int(x) in (1, 3) for x in ids[reach]]][0])    # the line of "abc" that the scan reports
    assert sorted(m[reach].tolist()) == sorted([1 << 4, 1 << groups[win]])
    np.testing.assert_array_equal(m, masks_by_id(groups)[ids])


def test_class_table_ors_every_id_of_a_state():
    t = PfacTable.from_charclass(CLASS_PATTERNS, 256)
    groups = [None, 0, 63, 7, None, (1, 2), 9, 20]
    by_id = masks_by_id(groups)
    m = t.state_group_masks(groups)
    multi = 0
    for s in range(t.num_final):
        ids = t.out_ids[t.out_first[s]:t.out_first[s + 1]]
        want = 0
        for i in ids:
            want |= int(by_id[int(i)])
        assert int(m[s]) == want, s
        multi += len(ids) > 1
        if sorted(int(i) for i in ids) == [1, 2, 7]:
            assert want == 1 | 1 << 63 | 1 << 20
    assert multi >= 1


def test_wrong_arguments_raise():
    t = PfacTable.from_bytes(b"he\nshe\n", 256)
    for bad in ([None, 1], [None, 1, 2, 3], np.zeros(2, dtype=np.uint64), []):
        with pytest.raises(ValueError):
            t.state_group_masks(bad)
    for bad in ([None, 64, 0], [None, -1, 0], [None, (1, 70), 0]):
        with pytest.raises(ValueError):
            t.state_group_masks(bad)


# ---------------------------------------------------------------------------
# the references agree

def test_three_forms_of_the_reference_agree():
    """lines16 over three tiles, every offset shape: the per-document oracle (THE reference), bytes.find per document
    and pattern, and the cut by hand of the whole-buffer records."""
    c = cases()
    info = c.x.tinfo(2)
    by_id = c.by_id(2)
    no = c.n_owned(3)
    buf = c.text[:no]
    pos, ids, lens = c.scan(2, 3)
    seen = 0
    for shape in SHAPES:
        off = c.offsets(2, 3, shape)
        want = masks_per_doc(info["matcher"], buf, off, by_id)
        np.testing.assert_array_equal(masks_by_find(buf, off, info["lines"], by_id), want, err_msg=shape)
        np.testing.assert_array_equal(masks_cut(pos, ids, lens, off, by_id), want, err_msg=shape)
        np.testing.assert_array_equal(c.want(2, 3, shape), want, err_msg=shape)
        seen |= int(np.bitwise_or.reduce(want))
    assert seen == 1 | 1 << 63 | 1 << 7 | 6                     # every group of the grouping occurs


def test_dictionary_cut_agrees_with_the_per_document_oracle():
    c = cases()
    info = c.x.tinfo(4)
    off = c.offsets(4, 3, "mid")
    pos, ids, lens = c.scan(4, 3)
    want = masks_per_doc(info["matcher"], c.text[:c.n_owned(3)], off, c.by_id(4))
    np.testing.assert_array_equal(masks_cut(pos, ids, lens, off, c.by_id(4)), want)


def test_class_table_reference_agrees_with_bytes_of_each_document():
    """A class table's rows (pos, id) come from oracle/charclass_oracle.py; cut by hand over the whole buffer they give
    what matching every document's own bytes gives."""
    rng = np.random.default_rng(77)
    alphabet = np.frombuffer(b"abcxyzq0123456789 AB-!", dtype=np.uint8)
    data = alphabet[rng.integers(0, alphabet.size, 5000)]
    parsed = cco.parse(CLASS_PATTERNS)
    plen = np.array([0] + [len(p) for p in parsed], dtype=np.int64)
    by_id = masks_by_id([None, 0, 63, 7, None, (1, 2), 9, 20])
    off = np.unique(np.concatenate([[0, 5000], rng.integers(0, 5000, 300)])).astype(np.uint64)
    pos, ids = cco.match(CLASS_PATTERNS, data, parsed)
    got = masks_cut(pos, ids.astype(np.int64), plen[ids], off, by_id)
    want = np.zeros(off.size - 1, dtype=np.uint64)
    for d in range(off.size - 1):
        _, di = cco.match(CLASS_PATTERNS, data[int(off[d]):int(off[d + 1])], parsed)
        for i in di:
            want[d] |= by_id[int(i)]
    np.testing.assert_array_equal(got, want)
    assert (want == 0).any() and (want != 0).any()


# ---------------------------------------------------------------------------
# the case list

@pytest.mark.parametrize("tiles", TILES)
@pytest.mark.parametrize("W", [2, 4])
def test_every_case_is_the_case_it_is_named_for(W, tiles):
    c = cases()
    for shape in SHAPES:
        facts = c.check_preconditions(W, tiles, shape)
        assert facts["n_docs"] >= 1
        want = c.want(W, tiles, shape)
        assert want.size == facts["n_docs"]
        if shape != "one":
            assert (want != 0).any()


# ---------------------------------------------------------------------------
# the predicate

def test_predicate_truth_table():
    vals = [0, 1, 2, 3, 1 << 63, (1 << 63) | 1, 6, 7, ALL]
    m = np.array(vals, dtype=np.uint64)
    sets = [0, 1, 2, 3, 1 << 63, (1 << 63) | 1, 4, ALL]
    n = 0
    for a, y, x, inv in itertools.product(sets, sets, sets, (False, True)):
        got = predicate(m, a, y, x, inv)
        np.testing.assert_array_equal(got, predicate_loop(m, a, y, x, inv))
        n += 1
    assert n == 8 * 8 * 8 * 2
    assert predicate(m).tolist() == list(range(len(vals)))                       # no demand at all: every document
    assert predicate(m, invert=True).size == 0
    assert predicate(m, any_of=0, all_of=3).tolist() == [3, 7, 8]                # any_of == 0 asks for nothing
    assert predicate(m, any_of=ALL).tolist() == list(range(1, len(vals)))
    assert predicate(m, all_of=1, none_of=2).tolist() == [1, 5]
    assert predicate(m, all_of=1, none_of=2, invert=True).tolist() == [0, 2, 3, 4, 6, 7, 8]


def test_predicate_reduces_to_documents_matching():
    """Every pattern in one group: mask != 0 is "the document has a kept record", pfac_documents_matching's flag."""
    c = cases()
    pos, ids, lens = c.scan(2, 3)
    one_group = np.full(c.by_id(2).size, 1 << 5, dtype=np.uint64)
    for shape in SHAPES:
        off = c.offsets(2, 3, shape)
        first = cut_by_hand(pos, ids, lens, off)[0]
        m = masks_cut(pos, ids, lens, off, one_group)
        for inv in (False, True):
            np.testing.assert_array_equal(predicate(m, any_of=ALL, invert=inv), matching_ids(first, inv), err_msg=shape)
            np.testing.assert_array_equal(predicate(m, all_of=1 << 5, invert=inv), matching_ids(first, inv), err_msg=shape)
