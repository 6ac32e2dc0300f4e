"""Host reference for the rank over document scores, pfac_documents_top_scores (the checker, never the product), and the
score sets that make the cases of tests/test_gpu_top.py test what they are named for.  Nothing comes from the device.

Two references that share no code beyond the candidates (scoreref.predicate, itself held against predicate_loop in
tests/test_score_ref.py):
  `ranking`     np.lexsort over (id, key word): the key mapped to the 64-bit word whose unsigned ascending order is the
                rank order -- the header's words: sign bit flipped for scores, all bits inverted for "largest first";
  `ranking_py`  Python's sorted (and, for one k, heapq) over tuples (key, id) of Python ints, the key negated for
                "largest first": no key word, no numpy.
The reported documents are the first min(k, candidates) of the ranking; without PFAC_TOP_RANKED the same ids ascending.

The cases (`CASES`): a size, a key set, a rule.  `KEYSETS` names the generators; `ks_of` gives every k a case runs with:
0, 1, the four ends of the tie class that the middle of the ranking falls into (so k cuts inside it, before it and
behind it), n_cand - 1, n_cand, n_cand + 1 and 2^64 - 1."""
import heapq

import numpy as np

from scoreref import I64_MAX, I64_MIN, SCORE, U64_MAX, make, predicate

BY_COUNT, LOWEST, RANKED = 1, 2, 4          # PFAC_TOP_*, written apart from the product's
ALL_FLAGS = tuple(range(8))
BLOCK = 64                                  # documents per ballot of the compaction
GROUP = 64 * BLOCK                          # documents per wave of the compaction: one group and its prefix
WORKGROUP = 4 * GROUP                       # documents per workgroup of the compaction
SORT_BLOCK = 1024                           # PFAC_TOP_SORT_BLOCK
SIZES = (1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5, WORKGROUP + 70)


def key_word(sc, flags):
    """The order-preserving unsigned 64-bit word of every document's key."""
    if flags & BY_COUNT:
        w = sc["count"].astype(np.uint64)
    else:
        w = sc["score"].view(np.uint64) ^ np.uint64(1 << 63)
    return w if flags & LOWEST else ~w


def ranking(sc, cand, flags):
    """The candidates `cand` (ascending ids) in rank order."""
    cand = np.asarray(cand, dtype=np.uint64)
    w = key_word(sc, flags)[cand.astype(np.int64)]
    return cand[np.lexsort((cand, w))]


def _key_py(sc, d, flags):
    key = int(sc["count"][d]) if flags & BY_COUNT else int(sc["score"][d])
    return key if flags & LOWEST else -key


def ranking_py(sc, cand, flags):
    return np.array([d for _, d in sorted((_key_py(sc, int(d), flags), int(d)) for d in cand)], dtype=np.uint64)


def top_heap(sc, cand, flags, k):
    """The first k of the ranking from a heap, for one k."""
    return np.array([d for _, d in heapq.nsmallest(min(k, len(cand)), ((_key_py(sc, int(d), flags), int(d)) for d in cand))],
                    dtype=np.uint64)


def top(rank, k, flags):
    """What the call reports for k: (ids, n_top)."""
    ids = rank[:min(int(k), rank.size)]
    return (ids if flags & RANKED else np.sort(ids)), ids.size


def tie_class(sc, rank, flags, at=None):
    """[b, e): the ranks of the class of equal keys that rank `at` (default: the middle) falls into."""
    if rank.size == 0:
        return 0, 0
    w = key_word(sc, flags)[rank.astype(np.int64)]
    at = rank.size // 2 if at is None else at
    same = np.flatnonzero(w == w[at])
    return int(same[0]), int(same[-1]) + 1


def ks_of(sc, rank, flags):
    b, e = tie_class(sc, rank, flags)
    n = rank.size
    ks = {0, 1, n - 1, n, n + 1, U64_MAX, b, b + 1, (b + e) // 2, e - 1, e, e + 1}
    return sorted(k for k in ks if k >= 0)


# ---------------------------------------------------------------------------
# the key sets (host-made scores; `n` documents)

BASE = 0x4123456789ABCDEF                   # keys "equal in 7 of 8 bytes" differ from it in one byte


def _byte_keys(n, rng, pos):
    v = rng.integers(0, 256, n).astype(np.uint64)
    v[rng.integers(0, n, max(n // 3, 1))] = np.uint64(0x80)      # a tie class inside
    w = (np.uint64(BASE) & ~np.uint64(0xFF << (8 * pos))) | (v << np.uint64(8 * pos))
    return w.view(np.int64).copy(), w.copy()


def keyset(name, n, seed=0):
    """scores (SCORE[n]) of a named key set."""
    rng = np.random.default_rng(0x70B + 131 * seed + n)
    if name == "equal":
        return make(np.full(n, -7, dtype=np.int64), np.full(n, 3, dtype=np.uint64))
    if name == "perm":
        p = rng.permutation(n)
        return make((p - n // 2).astype(np.int64), rng.permutation(n).astype(np.uint64))
    if name == "extremes":
        s = np.array([I64_MIN, -1, 0, 1, I64_MAX], dtype=np.int64)[rng.integers(0, 5, n)]
        c = np.array([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, U64_MAX], dtype=np.uint64)[rng.integers(0, 6, n)]
        return make(s, c)
    if name == "ties":                                           # five values: every class is large and lies everywhere
        s = np.array([-3, 0, 5, 5 + 2 ** 40, I64_MIN + 9], dtype=np.int64)[rng.integers(0, 5, n)]
        c = np.array([0, 1, 2, 2 ** 63, 2 ** 63 + 2 ** 31], dtype=np.uint64)[rng.integers(0, 5, n)]
        return make(s, c)
    if name == "sparse":                                         # mostly {0, 0}
        s, c = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint64)
        hit = rng.choice(n, max(n // 50, 1), replace=False)
        c[hit] = rng.integers(1, 6, hit.size).astype(np.uint64)
        s[hit] = rng.integers(-4, 9, hit.size)
        return make(s, c)
    if name.startswith("byte"):
        return make(*_byte_keys(n, rng, int(name[4:])))
    raise KeyError(name)


KEYSETS = ("equal", "perm", "extremes", "ties", "sparse") + tuple(f"byte{p}" for p in range(8))


def lengths(n, seed=0):
    """Document offsets (uint64[n + 1]) whose lengths make the density's products pass 2^63: a few huge, a few empty."""
    rng = np.random.default_rng(0xDE5 + seed + n)
    lens = [int(x) for x in rng.integers(0, 5000, n)]
    for i, v in zip(range(0, n, max(n // 7, 1)), (2 ** 62, 0, 2 ** 61, 1, 2 ** 60, 0, 3)):
        lens[i] = v
    return np.array(np.cumsum([0] + lens, dtype=object) % 2 ** 64, dtype=np.uint64)


# the rules a case may run under: name -> kwargs of scoreref.predicate (and of GpuMatcher.top_documents)
RULES = {
    "all": dict(),
    "matched": dict(min_count=1),
    "window": dict(min_score=-3, max_score=2 ** 41, max_count=2 ** 63),
    "inverted": dict(min_count=1, invert=True),
    "dense": dict(density=(-(2 ** 40), 2 ** 63 + 5)),
    "dense-inverted": dict(density=(3, 1000), min_count=0, invert=True),
}


class Case:
    """One (size, key set, rule): the scores, the offsets where the rule has a density, the candidates."""

    def __init__(self, n, keys, rule="all"):
        self.n, self.keys, self.rule = n, keys, rule
        self.sc = keyset(keys, n)
        self.kw = RULES[rule]
        self.off = lengths(n) if "density" in self.kw else None
        self.cand = predicate(self.sc, self.off, **self.kw)
        self._rank = {}

    def __repr__(self):
        return f"{self.n}-{self.keys}-{self.rule}"

    def rank(self, flags):
        key = flags & (BY_COUNT | LOWEST)
        if key not in self._rank:
            self._rank[key] = ranking(self.sc, self.cand, key)
        return self._rank[key]


def case_list():
    """Every size with the tie-heavy key set and no rule; the other key sets and the rules at the sizes where the code
    takes another path: one block, one group and a bit, more than one workgroup."""
    out = [(n, "ties", "all") for n in SIZES]
    for n in (65, 4097, WORKGROUP + 70):
        out += [(n, k, "all") for k in KEYSETS if k != "ties"]
        out += [(n, k, r) for k, r in (("sparse", "matched"), ("ties", "window"), ("sparse", "inverted"), ("extremes", "dense"),
                                       ("ties", "dense-inverted"), ("perm", "matched"))]
    return out


CASE_IDS = case_list()
_CASES = {}


def case(n, keys, rule):
    if (n, keys, rule) not in _CASES:
        _CASES[(n, keys, rule)] = Case(n, keys, rule)
    return _CASES[(n, keys, rule)]


def sort_case(n_top, seed=0):
    """Scores of n_top + 300 documents for the sort's sizes: three key values only, so that every tie class spans the
    sort's blocks, and k = n_top cuts the last class."""
    n = n_top + 300
    rng = np.random.default_rng(0x50B7 + n_top + seed)
    return make(np.array([-9, 4, 2 ** 50], dtype=np.int64)[rng.integers(0, 3, n)], rng.integers(0, 3, n).astype(np.uint64))


SORT_SIZES = tuple(m * SORT_BLOCK + d for m in (1, 2) for d in (-1, 0, 1))
