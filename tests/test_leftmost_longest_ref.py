"""The host references of leftmost-longest selection (tests/llref.py) checked against each other and against the worked
example that pins the rule.  CPU only."""
import numpy as np
import pytest

from llref import check_greedy, greedy

PATTERNS = [b"a", b"ab", b"bc", b"abcd"]


def brute_records(patterns, text):
    """(pos, len, id) of every occurrence, in (pos, len) order."""
    rec = []
    for p in range(len(text)):
        for pid, pat in enumerate(patterns, start=1):
            if text.startswith(pat, p):
                rec.append((p, len(pat), pid))
    rec.sort()
    a = np.array(rec, dtype=np.int64).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2]


def picks(patterns, text, entry, n_owned):
    pos, lens, ids = brute_records(patterns, text[:n_owned + max(len(x) for x in patterns) - 1])
    keep = pos < n_owned
    pos, lens, ids = pos[keep], lens[keep], ids[keep]
    sel, ex = greedy(pos, lens, entry, n_owned)
    assert check_greedy(pos, lens, (pos[sel], lens[sel]), entry, n_owned) == ex
    return [(int(pos[i]), patterns[ids[i] - 1].decode()) for i in sel], ex


def test_worked_example():
    text = b"xabcabcd"
    assert picks(PATTERNS, text, 0, 8) == ([(1, "ab"), (4, "abcd")], 0)
    assert picks(PATTERNS, text, 2, 8) == ([(2, "bc"), (4, "abcd")], 0)
    # the same input as two owned ranges [0, 2) and [2, 8), the second scan's positions relative to byte 2
    first, ex = picks(PATTERNS, text, 0, 2)
    assert (first, ex) == ([(1, "ab")], 1)
    assert picks(PATTERNS, text[2:], ex, 6) == ([(2, "abcd")], 0)
    # entry 0 instead of the returned 1 picks `bc` at 0: what chaining must not do
    assert picks(PATTERNS, text[2:], 0, 6)[0][0] == (0, "bc")


def test_empty_and_past_the_end():
    e = np.empty(0, dtype=np.int64)
    assert greedy(e, e, 3, 0)[1] == 3
    assert check_greedy(e, e, (e, e), 3, 0) == 3
    pos, lens = np.array([0, 1]), np.array([2, 1])
    sel, ex = greedy(pos, lens, 5, 2)
    assert sel.size == 0 and ex == 3


def test_check_greedy_rejects_wrong_selections():
    pos = np.array([0, 0, 1, 3, 4, 6], dtype=np.int64)
    lens = np.array([1, 3, 2, 2, 1, 2], dtype=np.int64)
    sel, ex = greedy(pos, lens, 0, 7)
    assert pos[sel].tolist() == [0, 3, 6] and ex == 1
    assert check_greedy(pos, lens, (pos[sel], lens[sel]), 0, 7) == 1
    for sp, sl in (([0, 3], [3, 2]),                       # stops early
                   ([0, 4, 6], [3, 1, 2]),                 # skips the first candidate after an end
                   ([0, 3, 6], [1, 2, 2]),                 # not the longest at 0
                   ([1, 3, 6], [2, 2, 2])):                # not the first candidate
        with pytest.raises(AssertionError):
            check_greedy(pos, lens, (np.array(sp), np.array(sl)), 0, 7)


def random_records(rng, n, max_len, density, runs=False):
    """(pos, len) in (pos, len) order: either random positions and lengths, or (runs) the records of `a`-runs for
    the patterns of lengths 2 and 3 (every chain from an even entry avoids every chain from an odd one)."""
    if runs:
        text = np.where(rng.random(n) < 0.01, 1, 0)
        pos, lens = [], []
        for p in range(n):
            for L in (2, 3):
                if p + L <= n and not text[p:p + L].any():
                    pos.append(p)
                    lens.append(L)
        return np.array(pos, dtype=np.int64), np.array(lens, dtype=np.int64)
    at = np.flatnonzero(rng.random(n) < density)
    k = rng.integers(1, 4, at.size)
    pos = np.repeat(at, k)
    lens = rng.integers(1, max_len + 1, pos.size)
    order = np.lexsort((lens, pos))
    return pos[order].astype(np.int64), lens[order].astype(np.int64)


@pytest.mark.parametrize("seed", range(12))
def test_references_agree_on_random_records(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 20000))
    max_len = int(rng.choice([1, 2, 4, 30, 1000]))
    pos, lens = random_records(rng, n, max_len, float(rng.choice([0.01, 0.3, 1.0])), runs=seed % 3 == 0)
    for entry in (0, 1, 2, min(max_len, 7)):
        n_owned = n if seed % 2 else max(1, n - int(rng.integers(0, 50)))
        keep = pos < n_owned
        sel, ex = greedy(pos[keep], lens[keep], entry, n_owned)
        got = check_greedy(pos[keep], lens[keep], (pos[keep][sel], lens[keep][sel]), entry, n_owned)
        assert got == ex
        assert 0 <= ex <= max(max_len, entry)
        if sel.size:
            assert (np.diff(pos[keep][sel]) >= lens[keep][sel][:-1]).all()       # non-overlapping


def test_chaining_equals_one_pass():
    """Owned ranges with the exit of one as the entry of the next select what one pass over everything selects."""
    rng = np.random.default_rng(7)
    pos, lens = random_records(rng, 5000, 0, 0, runs=True)
    want, _ = greedy(pos, lens, 1, 5000)
    cuts = [0, 1234, 1235, 3001, 5000]
    got, entry = [], 1
    for a, b in zip(cuts[:-1], cuts[1:]):
        keep = (pos >= a) & (pos < b)
        sel, entry = greedy(pos[keep] - a, lens[keep], entry, b - a)
        got.append(pos[keep][sel])
    np.testing.assert_array_equal(np.concatenate(got), pos[want])
