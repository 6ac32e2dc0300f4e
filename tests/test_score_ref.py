"""Document scores without a GPU: PfacTable.state_weights, the references of tests/scoreref.py held against one another
(the cut by hand against overlapping bytes.find; the numpy predicate against Python integers), and the preconditions of
the cases of tests/test_gpu_scores.py."""
import itertools

import numpy as np
import pytest

import scoreref
from groupref import SHAPES, TILES, cases
from phfpfac_amd import SCORE_DTYPE, PfacTable
from scoreref import CYCLE, I64_MAX, I64_MIN, U64_MAX, predicate, predicate_loop, scores_by_find, scores_cut, weights_for

CLASS_PATTERNS = b"[a-c]x\nax\n[^a-z0-9 ]\nq[0-9][0-9]\n[a-c]\nax[xy]\n[a-c]x\n"     # "ax" ends patterns 1, 2 and 7 in one state


def test_the_dtype_is_the_struct():
    assert SCORE_DTYPE == scoreref.SCORE and SCORE_DTYPE.itemsize == 16


def test_weights_for_holds_what_the_cases_need():
    w = weights_for(16)
    assert w[0] == 0 and len(w) == 17 and tuple(w[1:8]) == CYCLE and w[8] == CYCLE[0]
    assert 0 in CYCLE and 3 in CYCLE and -3 in CYCLE and -(2 ** 31) in CYCLE and 2 ** 31 - 1 in CYCLE


# ---------------------------------------------------------------------------
# state_weights

def test_literal_table_takes_the_weight_of_idmap_and_of_the_winning_duplicate():
    t = PfacTable.from_bytes(b"abc\nxy\nabc\nq\n", 256)
    weights = [0, 5, -7, 11, 0]
    w = t.state_weights(weights)
    assert w.dtype == np.int32 and w.size == t.num_final
    ids = np.asarray(t.idmap, dtype=np.int64)
    np.testing.assert_array_equal(w, np.array(weights)[ids][: t.num_final])
    reach = t.final_lengths() >= 1
    win = int(ids[reach][[int(x) in (1, 3) for x in ids[reach]]][0])      # the line of "abc" that the scan reports
    assert sorted(w[reach].tolist()) == sorted([-7, 0, weights[win]])
    ext = t.state_weights([0, -(2 ** 31), 2 ** 31 - 1, 0, 1])
    assert int(ext.min()) == -(2 ** 31) and int(ext.max()) == 2 ** 31 - 1


def test_class_table_sums_every_id_of_a_state():
    t = PfacTable.from_charclass(CLASS_PATTERNS, 256)
    weights = [0, 3, 0, -3, 1, -(2 ** 31), 2 ** 31 - 1, -1]
    assert weights == weights_for(7)
    w = t.state_weights(weights)
    multi = 0
    for s in range(t.num_final):
        ids = [int(i) for i in t.out_ids[t.out_first[s]:t.out_first[s + 1]]]
        assert int(w[s]) == sum(weights[i] for i in ids), s
        multi += len(ids) > 1
        if sorted(ids) == [1, 2, 7]:
            assert int(w[s]) == 3 + 0 - 1
    assert multi >= 1
    # a sum that leaves int32: patterns 1, 2 and 7 end in one state
    with pytest.raises(ValueError, match="int32"):
        t.state_weights([0, 2 ** 31 - 1, 1, 0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="int32"):
        t.state_weights([0, -(2 ** 31), 0, 0, 0, 0, 0, -1])
    assert int(t.state_weights([0, 2 ** 31 - 1, 1, 0, 0, 0, 0, -1]).max()) == 2 ** 31 - 1       # ... and one that just fits


def test_wrong_arguments_raise():
    t = PfacTable.from_bytes(b"he\nshe\n", 256)
    for bad in ([0, 1], [0, 1, 2, 3], []):
        with pytest.raises(ValueError):
            t.state_weights(bad)
    for bad in ([0, 2 ** 31, 0], [0, 0, -(2 ** 31) - 1]):
        with pytest.raises(ValueError, match="int32"):
            t.state_weights(bad)


# ---------------------------------------------------------------------------
# the references agree

@pytest.mark.parametrize("W", [2, 8])
def test_the_cut_agrees_with_overlapping_find(W):
    """lines16 over three tiles of the planted text, every offset shape: the cut by hand of the whole-buffer records
    against bytes.find of every pattern in every document's own bytes."""
    c = cases()
    info = c.x.tinfo(W)
    by_id = scoreref.by_id_of(W)
    no = c.n_owned(3)
    pos, ids, lens = c.scan(W, 3)
    for shape in SHAPES:
        off = c.offsets(W, 3, shape)
        got = scores_cut(pos, ids, lens, off, by_id)
        np.testing.assert_array_equal(got, scores_by_find(c.text[:no], off, info["lines"], by_id), err_msg=shape)
        np.testing.assert_array_equal(scoreref.want(W, 3, shape), got, err_msg=shape)
        assert got["count"].sum() > 0


def test_dictionary_cut_agrees_with_overlapping_find():
    """The dictionary's table (width 4) over the first tile, cut into mid-sized documents: only the lines that occur
    at all are searched per document."""
    c = cases()
    info = c.x.tinfo(4)
    by_id = scoreref.by_id_of(4)
    pos, ids, lens = c.scan(4, 3)
    n = 4096
    head = pos + lens <= n
    off = np.unique(np.concatenate([[0, n], np.arange(173, n, 257)])).astype(np.uint64)
    text = bytes(c.text[:n])
    same = {}                                                   # the ids of every distinct line that occurs in the text
    for i, ln in enumerate(info["lines"], 1):
        if ln and ln in text:
            same.setdefault(ln, []).append(i)
    reported = set(int(i) for i in ids[head])
    lines, w = [], [0]
    for ln, cand in same.items():                               # of duplicate lines the scan reports one id
        hit = [i for i in cand if i in reported]
        assert len(hit) == 1, (ln, cand, hit)
        lines.append(ln)
        w.append(int(by_id[hit[0]]))
    assert reported == set(i for cand in same.values() for i in cand if i in reported)
    want = scores_by_find(np.frombuffer(text, dtype=np.uint8), off, lines, np.array(w, dtype=np.int64))
    np.testing.assert_array_equal(scores_cut(pos[head], ids[head], lens[head], off, by_id), want)
    assert want["count"].sum() > 0


def test_totals_wrap_like_int64():
    sc = scoreref.make(np.array([I64_MAX, 1, 5], dtype=np.int64), np.array([1, 2, 3], dtype=np.uint64))
    assert scoreref.totals(sc) == (I64_MIN + 5, 6)


# ---------------------------------------------------------------------------
# the predicate

def test_predicate_agrees_with_python_integers():
    rng = np.random.default_rng(0x5C0)
    special = [I64_MIN, I64_MIN + 1, -(2 ** 62), -3, -1, 0, 1, 3, 2 ** 62, I64_MAX - 1, I64_MAX]
    score = np.array(special + rng.integers(-50, 50, 40).tolist(), dtype=np.int64)
    count = np.array([0, 1, 2, U64_MAX, U64_MAX - 1, 2 ** 63] * 8 + [7, 9, 11], dtype=np.uint64)
    sc = scoreref.make(score, count)
    lens = [0, 1, 2, 3, 1000, 2 ** 40, 64, 7] * 6 + [2 ** 62, 2 ** 63, 5]
    off = np.array([sum(lens[:k]) for k in range(len(lens) + 1)], dtype=np.uint64)
    assert int(off[-1]) < 2 ** 64
    windows = [(None, None), (0, None), (None, 0), (-3, 3), (I64_MIN, I64_MAX), (1, 0), (I64_MAX, None), (None, I64_MIN)]
    counts = [(None, None), (1, None), (None, 2), (2, U64_MAX - 1), (U64_MAX, None), (0, 0)]
    densities = [None, (1, 1000), (-1, 3), (0, 1), (I64_MAX, U64_MAX), (I64_MIN, U64_MAX), (-(2 ** 40), 2 ** 63 + 5), (3, 1)]
    n = 0
    for (lo, hi), (cl, ch), dens, inv in itertools.product(windows, counts, densities, (False, True)):
        kw = dict(min_score=lo, max_score=hi, min_count=cl, max_count=ch, density=dens, invert=inv)
        np.testing.assert_array_equal(predicate(sc, off, **kw), predicate_loop(sc, off, **kw), err_msg=str(kw))
        n += 1
    assert n == 8 * 6 * 8 * 2
    # products past 2^63 decide: equal in the low 64 bits, different as integers
    two = scoreref.make(np.array([2 ** 62, 2 ** 62], dtype=np.int64), np.array([1, 1], dtype=np.uint64))
    off2 = np.array([0, 2 ** 62, 2 ** 63], dtype=np.uint64)
    assert (2 ** 62 * 8) % 2 ** 64 == (4 * 2 ** 62) % 2 ** 64 == 0
    assert predicate(two, off2, density=(4, 8)).tolist() == [0, 1]
    assert predicate(two, off2, density=(8, 4)).tolist() == []
    assert predicate(two, off2, density=(8, 8)).tolist() == [0, 1]
    assert predicate(two, off2, density=(9, 8)).tolist() == []
    assert predicate(sc).size == sc.size and predicate(sc, invert=True).size == 0


# ---------------------------------------------------------------------------
# the case list

@pytest.mark.parametrize("tiles", TILES)
@pytest.mark.parametrize("W", [2, 4])
def test_every_scan_holds_the_documents_the_gpu_tests_rely_on(W, tiles):
    """(Width 8 scans with the table of width 2.)"""
    scoreref.check_preconditions(W, tiles)
    c = cases()
    for shape in SHAPES:
        c.check_preconditions(W, tiles, shape)
        sc = scoreref.want(W, tiles, shape)
        assert sc.size == c.offsets(W, tiles, shape).size - 1
        assert int(sc["count"].sum()) <= c.scan(W, tiles)[0].size
