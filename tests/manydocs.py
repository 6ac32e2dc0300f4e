"""Cases, references and checks for the document passes at millions of documents and ids (the checker, never the
product): the sizes at which the compaction, the rank, the gather and the split leave the paths the other tests reach,
flag, score, mask and id patterns that put the truth where a wrong prefix shows, one scanned input of more than six
million documents for the heap-driven passes (`heap_input`), array-at-a-time references, and one check function per
pass.  Imports without a GPU and without torch; nothing comes from the device.

The sizes come from the constants of phfpfac_amd/csrc/pfac_hip.hip:
  GROUP_DOCS  = DM_BLOCKS * WAVE = 64 * 64: the documents whose count is ONE group sum of the compaction (dm_run and
                pfac_top_compact_kernel);
  SCAN_THREADS = 1024: pfac_scan_groups_kernel is one block of 1024 threads, thread t owns the `per` = ceil(n_groups /
                1024) sums from t * per on, and the thread that owns the last sum writes the total;
  HIST_TRIP   = 2048 * TOP_BINS = 2048 * 256: the documents one trip of pfac_top_hist_kernel's grid-stride loop covers
                (its grid is capped at 2048 workgroups of TOP_BINS threads);
  ID_GROUP    = RP_BLOCK * RP_GROUP = 64 * 16: the ids whose bytes are ONE group sum of the gather (ga_run);
  SORT_BLOCK  = PFAC_TOP_SORT_BLOCK: the ranked sort's block, whose 256 counts per block go through the same scan;
  SPLIT_GROUP = 64 tiles of 4096 bytes: the bytes whose delimiters are ONE group sum of the split.

References.  Where an existing reference already works on whole arrays it is used as it is: splitref.matching_ids and
split_offsets, gatherref.context_ids and gather_ref, fmtref.format_ref, groupref.predicate, topref.key_word, tie_class
and top.  Twins are written here for the two that do not at these sizes: `ranking` (a stable sort of the key words of
candidates that ascend, for topref.ranking's lexsort over two keys) and `score_ids` (the density in int64, for
scoreref.predicate's Python integers in object arrays); tests/test_manydocs_cases.py holds each to the existing one on
that module's own cases, which is their only claim to truth."""
import numpy as np

import topref
from fmtref import NL, Fmt, format_ref, lines_data
from gatherref import context_ids, gather_ref
from groupref import predicate as group_ids
from scoreref import make
from splitref import matching_ids
from topref import BY_COUNT, LOWEST, RANKED, key_word, tie_class, top

TILE = 4096
GROUP_DOCS = 64 * 64
SCAN_THREADS = 1024
HIST_TRIP = 2048 * 256
ID_GROUP = 64 * 16
SORT_BLOCK = topref.SORT_BLOCK
SPLIT_GROUP = 64 * TILE

# 1024 groups (per = 1: the last thread owns the total), 1025 (per = 2: half the threads idle), 2049 (per = 3)
DOCS = (GROUP_DOCS * 1024, GROUP_DOCS * 1024 + 1, GROUP_DOCS * 2048 + 1)
# one trip of the histogram exactly, one document into the second trip, a third trip of one wave and a lane
HIST_DOCS = (HIST_TRIP, HIST_TRIP + 1, 2 * HIST_TRIP + 65) + DOCS
IDS = (ID_GROUP * 1024, ID_GROUP * 1024 + 1, ID_GROUP * 2048 + 1)
EDGE = 1024                              # the first group whose prefix a thread other than its own number computes


def groups_of(n, group):
    return (n + group - 1) // group


def per_of(n_groups):
    """`per` of pfac_scan_groups_kernel."""
    return (n_groups + SCAN_THREADS - 1) // SCAN_THREADS


def total_owner(n_groups):
    """The thread of pfac_scan_groups_kernel that writes the total."""
    return (n_groups - 1) // per_of(n_groups)


# ---------------------------------------------------------------------------
# flag patterns: which documents are the truth (a function of the name and n alone)

FLAGS = ("all", "none", "alternating", "runs", "last", "group_firsts", "late")


def flags(name, n):
    d = np.arange(n, dtype=np.int64)
    if name == "all":
        return np.ones(n, dtype=bool)
    if name == "none":
        return np.zeros(n, dtype=bool)
    if name == "alternating":
        return d % 2 == 0                # (so that document n - 1 of an odd n is one)
    if name == "runs":                   # seeded runs of 1..9000 documents (longer than two groups), on and off in turn
        rng = np.random.default_rng([0x52554E, n])
        lens = rng.integers(1, 9001, n // 3000 + 64)
        assert int(lens.sum()) >= n
        f = np.repeat(np.arange(lens.size), lens)[:n] % 2 == 1
        f[EDGE * GROUP_DOCS - 600:EDGE * GROUP_DOCS - 100] = True       # (group 1023 is not left to chance, nor is 1024)
        f[EDGE * GROUP_DOCS:EDGE * GROUP_DOCS + 50] = True
        return f
    if name == "last":
        return d == n - 1
    if name == "group_firsts":
        return d % GROUP_DOCS == 0
    if name == "late":                   # only the documents of groups >= 1024
        return d >= EDGE * GROUP_DOCS
    raise KeyError(name)


def doc_first_of(f):
    """A doc_first in which exactly the documents of `f` hold records (1..3 of them)."""
    cnt = f.astype(np.uint64) * (np.uint64(1) + np.arange(f.size, dtype=np.uint64) % np.uint64(3))
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(cnt, dtype=np.uint64)])


WHERE = dict(all_of=0x21, any_of=1 << 63, none_of=0x40)


def masks_of(f):
    """Group masks that satisfy WHERE exactly in the documents of `f`: the others miss a group of all_of, miss any_of,
    or hold none_of, in turn."""
    d = np.arange(f.size, dtype=np.uint64) % np.uint64(3)
    other = np.array([(1 << 63) | 0x01, 0x21, (1 << 63) | 0x61], dtype=np.uint64)[d]
    return np.where(f, np.uint64((1 << 63) | 0x21 | 0x100), other)


RULE = dict(min_score=-4, max_score=90, min_count=2)
DENSITY = (2, 1)                         # at least two points per byte


def doc_lengths(n):
    return (np.arange(n, dtype=np.int64) * 7 + 3) % 5


def offsets_of(lens):
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])


def scores_of(f, dense=False):
    """Scores that satisfy RULE -- with `dense`: RULE and DENSITY over doc_lengths -- exactly in the documents of `f`.
    The truth holds {2 * length, 2}.  The others are, in turn, one below min_score, one above max_score and one count
    short; with `dense` the first of the three is inside both windows and one point short of the density."""
    n = f.size
    ln = doc_lengths(n)
    d = np.arange(n, dtype=np.int64) % 3
    first = 2 * ln - 1 if dense else np.full(n, RULE["min_score"] - 1, dtype=np.int64)
    score = np.where(f, 2 * ln, np.where(d == 0, first, np.where(d == 1, RULE["max_score"] + 1, 2 * ln)))
    count = np.where(f, 2, np.array([2, 3, 1], dtype=np.int64)[d])
    return make(score, count.astype(np.uint64))


def score_ids(sc, off=None, min_score=None, max_score=None, min_count=None, max_count=None, density=None, invert=False):
    """scoreref.predicate with the density's products in int64: exact while they fit, which is asserted."""
    s, c = sc["score"], sc["count"]
    ok = np.ones(s.size, dtype=bool)
    if min_score is not None:
        ok &= s >= np.int64(min_score)
    if max_score is not None:
        ok &= s <= np.int64(max_score)
    if min_count is not None:
        ok &= c >= np.uint64(min_count)
    if max_count is not None:
        ok &= c <= np.uint64(max_count)
    if density is not None:
        num, den = int(density[0]), int(density[1])
        length = np.diff(np.asarray(off, dtype=np.uint64)).astype(np.int64)
        bound = 2 ** 62
        assert s.size == 0 or (int(np.abs(s).max()) * den < bound and abs(num) * int(length.max()) < bound and int(length.min()) >= 0)
        ok &= s * np.int64(den) >= np.int64(num) * length
    return np.flatnonzero(ok != bool(invert)).astype(np.uint64)


# ---------------------------------------------------------------------------
# the rank

RANK_KEYS = (("ties", "all"), ("perm", "all"), ("perm", "dense"))
RANK_DENSITY = (1, 3)                    # a third of a point per byte: about half of "perm"'s documents


def ranking(sc, cand, order):
    """topref.ranking for candidates that ascend: a stable sort of their key words keeps the ids ascending in a tie."""
    cand = np.asarray(cand, dtype=np.uint64)
    w = key_word(sc, order)[cand.astype(np.int64)]
    return cand[np.argsort(w, kind="stable")]


class RankCase:
    """One (size, key set, rule) of the rank: topref's key set, the candidates, and the ranking per order, each once."""

    def __init__(self, n, keys, rule):
        self.n, self.keys, self.rule = n, keys, rule
        self.sc = topref.keyset(keys, n)
        self.kw = dict(density=RANK_DENSITY) if rule == "dense" else {}
        self.off = offsets_of(np.arange(n, dtype=np.int64) % 41) if rule == "dense" else None
        self.cand = score_ids(self.sc, self.off, **self.kw)
        self._rank = {}

    def __repr__(self):
        return f"{self.n}-{self.keys}-{self.rule}"

    def rank(self, order):
        order &= BY_COUNT | LOWEST
        if order not in self._rank:
            self._rank[order] = ranking(self.sc, self.cand, order)
        return self._rank[order]

    def ks(self, order):
        """1, the sort's block and one more, one more than 1024 groups of documents, the candidates and one more, and
        the middle of the tie class that the middle of the ranking falls into (topref.ks_of's)."""
        b, e = tie_class(self.sc, self.rank(order), order)
        n = self.cand.size
        return sorted({1, SORT_BLOCK, SORT_BLOCK + 1, GROUP_DOCS * 1024 + 1, n, n + 1, (b + e) // 2})


_RANK = {}


def rank_case(n, keys, rule):
    """The case, kept while its size is the one in use (a case of 8 M documents holds a few hundred MiB)."""
    if (n, keys, rule) not in _RANK:
        for k in [k for k in _RANK if k[0] != n]:
            del _RANK[k]
        _RANK[(n, keys, rule)] = RankCase(n, keys, rule)
    return _RANK[(n, keys, rule)]


# ---------------------------------------------------------------------------
# the gather

ID_LISTS = ("ascending", "repeats", "reversed", "same")
EMPTY_RUN = 64 * 1024 + 700              # more than 64 groups of ids without a byte
EMPTY_AT = (300 * ID_GROUP, 100_000 + 37)        # one run starts on a group edge, one off it


def gather_lengths(n_docs):
    """Seeded lengths 0..40 with the two runs of EMPTY_RUN empty documents."""
    lens = np.random.default_rng([0x6741, n_docs]).integers(0, 41, n_docs)
    for at in EMPTY_AT:
        lens[at:at + EMPTY_RUN] = 0
    lens[:4], lens[-4:] = (17, 3, 29, 1), (5, 40, 2, 23)        # whichever end an id list's last group reads has bytes
    return lens


def id_list(name, n_ids, n_docs):
    if name == "ascending":
        assert n_ids == n_docs
        return np.arange(n_ids, dtype=np.uint64)
    if name == "reversed":
        return np.arange(n_docs - 1, n_docs - 1 - n_ids, -1).astype(np.uint64)
    if name == "repeats":                # ascending, every id three times or so
        return np.sort(np.random.default_rng([0x1D5, n_ids]).integers(0, n_docs, n_ids)).astype(np.uint64) // np.uint64(3) * np.uint64(3)
    if name == "same":                   # one document of 40 bytes, n_ids times
        return np.full(n_ids, SAME_ID, dtype=np.uint64)
    raise KeyError(name)


SAME_ID = 12345

FORMATS = {"number": dict(number=True), "offset": dict(byte_offset=True), "both": dict(number=True, byte_offset=True, terminate=NL),
           "context": dict(number=True, terminate=NL, context_sep=True, group_sep=b"--\n")}
FORMAT_IDS = {"number": "ascending", "offset": "reversed", "both": "ascending", "context": "repeats"}


class GatherData:
    """n_docs = n_ids documents (fmtref.lines_data: seeded bytes, two documents in three end in a newline) and a
    doc_first of seeded runs for the context separators."""

    def __init__(self, n_ids):
        self.n_ids = self.n_docs = n_ids
        lens = gather_lengths(n_ids)
        lens[SAME_ID] = 40
        self.data, off = lines_data(lens, 0x6742 + n_ids)
        self.offsets = off.astype(np.uint64)
        self.n = int(self.data.size)
        self.doc_first = doc_first_of(flags("runs", n_ids))
        self._want = {}

    def ids(self, name):
        return id_list(name, self.n_ids, self.n_docs)

    def want(self, name, fmt=None):
        """(out, out_off) of the id list `name`, plain or under FORMATS[fmt]; the last one asked for is kept."""
        if (name, fmt) not in self._want:
            self._want.clear()
            ids = self.ids(name)
            self._want[(name, fmt)] = gather_ref(self.data, self.offsets, ids) if fmt is None else \
                format_ref(self.data, self.offsets, ids, Fmt(**FORMATS[fmt]), self.doc_first)
        return self._want[(name, fmt)]

    def storage(self):
        """The input followed by zeros up to the next tile boundary (at least 16 of them)."""
        s = np.zeros((self.n + 16 + TILE - 1) // TILE * TILE, dtype=np.uint8)
        s[:self.n] = self.data
        return s


_GATHER = {}


def gather_data(n_ids):
    if n_ids not in _GATHER:
        _GATHER.clear()
        _GATHER[n_ids] = GatherData(n_ids)
    return _GATHER[n_ids]


# the offsets' rule at depth: more than five million documents of 0..4 bytes, every fourth one selected
RULE_DOCS = DOCS[2]
RULE_BREAK = 5_000_000


def rule_case():
    """(n_bytes, offsets, ids): the ids select document RULE_BREAK and the last document."""
    off = offsets_of(doc_lengths(RULE_DOCS))
    ids = np.arange(0, RULE_DOCS, 4, dtype=np.uint64)
    assert ids.size <= IDS[2] and RULE_BREAK % 4 == 0 and (RULE_DOCS - 1) % 4 == 0
    return int(off[-1]), off, ids


def broken_offsets(off, how):
    """`off` with one rule broken: "decrease" -- document RULE_BREAK ends one byte in front of its start (its length was
    at least 1, and the offsets around it are untouched); "past_end" -- the last document ends one byte past n_bytes."""
    bad = off.copy()
    if how == "decrease":
        assert off[RULE_BREAK + 1] > off[RULE_BREAK] > 0
        bad[RULE_BREAK + 1] = off[RULE_BREAK] - np.uint64(1)
    else:
        bad[-1] = off[-1] + np.uint64(1)
    return bad


# ---------------------------------------------------------------------------
# the split

ALL_DELIMS = 8 * 1024 * 1024 + 17        # every byte a delimiter: 4096 offsets per tile, 262 144 per group, 33 groups
TILED_BYTES = 1025 * SPLIT_GROUP         # 1025 groups of 64 tiles
TILED_PERIOD = b"the quick brown fox\njumps over\n\nthe lazy dog, twice: the lazy dog"     # 65 bytes (odd: a tile starts at every phase)
TILED_PHASE = 7                          # the input ends inside "jumps": an unterminated last document


class Periodic:
    """The split of n bytes of `pattern` repeated from `phase` on, by arithmetic: the k-th document end is the e[k % c]
    of period k // c."""

    def __init__(self, n, pattern, phase, delim=NL):
        pat = np.frombuffer(pattern, dtype=np.uint8)
        self.n, self.P = n, pat.size
        self.e = np.flatnonzero(np.roll(pat, -phase) == delim).astype(np.int64) + 1       # ends inside one period, ascending
        self.c = self.e.size
        full, rest = divmod(n, self.P)
        self.n_ends = full * self.c + int((self.e <= rest).sum())
        last = int(self.end(np.array([self.n_ends - 1]))[0]) if self.n_ends else 0
        self.open_tail = last < n
        self.n_docs = self.n_ends + (1 if self.open_tail else 0)
        self.tail_start = last if self.open_tail else n

    def end(self, k):
        k = np.asarray(k, dtype=np.int64)
        return k // self.c * self.P + self.e[k % self.c]

    def offsets(self, first, count):
        """offsets [first, first + count) of the n_docs + 1."""
        i = np.arange(first, first + count, dtype=np.int64)
        assert count == 0 or (first >= 0 and int(i[-1]) <= self.n_docs)
        out = np.where(i == 0, 0, self.end(np.maximum(i - 1, 0)))
        out[i > self.n_ends] = self.n
        return out.astype(np.uint64)

    def index_at(self, byte):
        """The number of offsets below `byte`: the index of the first offset at or past it."""
        q, r = divmod(int(byte) - 1, self.P) if byte > 0 else (0, -1)
        below = (q * self.c + int((self.e <= r).sum()) if byte > 0 else 0) + (1 if byte > 0 else 0)
        return min(below, self.n_docs + 1)


def split_windows(p, width=6):
    """(first, count) of the offset windows to fetch: the start, `width` offsets on either side of every 64-tile group
    edge, and the end."""
    out = [(0, min(2 * width, p.n_docs + 1))]
    for edge in range(SPLIT_GROUP, p.n, SPLIT_GROUP):
        at = p.index_at(edge)
        lo = max(at - width, 0)
        out.append((lo, min(at + width, p.n_docs + 1) - lo))
    lo = max(p.n_docs + 1 - 2 * width, 0)
    out.append((lo, p.n_docs + 1 - lo))
    return out


# ---------------------------------------------------------------------------
# the checks: arrays only; the first differing index and how many differ

def _same(got, want, what, name):
    got, want = np.asarray(got), np.asarray(want)
    assert got.size == want.size, f"{what}: {got.size} {name}s, want {want.size}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {name} {int(bad[0])} is {int(got[bad[0]])}, want {int(want[bad[0]])} "
                           f"({bad.size} of {want.size} differ, the last at {int(bad[-1])})")


def assert_ids(ids, n_matching, want, what=""):
    """The compaction: the count, then every id."""
    assert n_matching == want.size, f"{what}: n_matching {n_matching}, want {want.size}"
    _same(np.asarray(ids, dtype=np.uint64), want, what, "id")


def assert_top(ids, pairs, n_top, sc, want_ids, what=""):
    """The rank: the count, every id in its order, and every winner's pair."""
    assert n_top == want_ids.size, f"{what}: n_top {n_top}, want {want_ids.size}"
    _same(np.asarray(ids, dtype=np.uint64), want_ids, what, "id")
    if pairs is not None:
        want = sc[want_ids.astype(np.int64)]
        _same(pairs["score"], want["score"], what, "score")
        _same(pairs["count"], want["count"], what, "count")


def assert_gather(out_bytes, out_off, out, want, want_off, fill=None, what=""):
    """The gather, plain or formatted: the count, every offset (the total among them), every byte and, with `fill`, that
    the bytes of `out` at and past out_bytes still hold it."""
    assert out_bytes == want.size, f"{what}: out_bytes {out_bytes}, want {want.size}"
    _same(np.asarray(out_off, dtype=np.uint64), want_off, what, "output offset")
    out = np.asarray(out, dtype=np.uint8)
    assert out.size >= want.size, f"{what}: {out.size} output bytes fetched, want {want.size}"
    _same(out[:want.size], want, what, "output byte")
    if fill is not None:
        bad = np.flatnonzero(out[want.size:] != fill)
        assert bad.size == 0, f"{what}: a byte at out_bytes + {int(bad[0])} was written ({bad.size} past the output's end)"


def assert_split(n_docs, tail_start, fetch, want_docs, want_tail, windows, want_window, what=""):
    """The split: n_docs, tail_start, and the offsets of every window.  fetch(first, n) -> the offsets as the code under
    test reports them; want_window(first, n) -> the reference's."""
    assert n_docs == want_docs, f"{what}: n_docs {n_docs}, want {want_docs}"
    assert tail_start == want_tail, f"{what}: tail_start {tail_start}, want {want_tail}"
    for first, n in windows:
        got, want = np.asarray(fetch(first, n), dtype=np.uint64), want_window(first, n)
        assert got.size == want.size, f"{what}: window [{first}, {first + n}): {got.size} offsets, want {want.size}"
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"{what}: offset {first + int(bad[0])} is {int(got[bad[0]])}, want {int(want[bad[0]])} "
                               f"({bad.size} of the window [{first}, {first + n}) differ)")


# ---------------------------------------------------------------------------
# the heap-driven passes: one scanned input of more than five million documents

SPACE = 0x20
HEAP_TEXT = 2 * SPLIT_GROUP              # bytes of text in front
HEAP_SHORT = 30 * SPLIT_GROUP            # bytes of one-, two- and a few three-byte documents behind it
HEAP_BLANK_TILES = 70                    # tiles of "# " behind those: no record of any table, more than one group of tiles
HEAP_EMPTY_RUN = 600_000                 # empty documents in a run: more than the 262 144 that 64 tiles of one-byte documents hold
HEAP_EMPTY_AT = (3 * SPLIT_GROUP, 5 * SPLIT_GROUP + 12_345)     # the runs' byte positions: on a 64-tile group edge, off one
HEAP_BREAK = 5_000_000                   # the offset index at which the rule is broken "at depth"
HEAP_WEIGHTS = (3, 0, -3, 1, -2, 7, -1)  # per pattern id, in turn: a zero and a cancelling pair; sums stay far from a wrap
WORDS3 = (b"in ", b"at ", b"on ", b"he ", b"an ")


class HeapInput:
    """The input and its offsets.  The bytes: passguard's text; then seeded documents " ", "x " (x of "iatehn#") and now
    and then one of WORDS3; then HEAP_BLANK_TILES tiles of "# "; then text again, its last word unterminated.  The
    offsets: a cut behind every space (splitref.split_offsets), one behind every 97th byte of the text in front (inside
    words: records cross those ends), and the two runs of HEAP_EMPTY_RUN empty documents."""

    def __init__(self):
        from passguard import cpu
        from splitref import split_offsets
        text = cpu().input("text")
        rng = np.random.default_rng(0x48454150)
        kinds = rng.choice(3, HEAP_SHORT // 2 + 1000, p=(0.3, 0.6, 0.1))
        lens = kinds + 1
        end = np.cumsum(lens)
        n_tok = int(np.searchsorted(end, HEAP_SHORT, side="right"))
        kinds, lens, end = kinds[:n_tok], lens[:n_tok], end[:n_tok]
        short = np.full(HEAP_SHORT, SPACE, dtype=np.uint8)                       # (what the tokens leave is spaces)
        start = end - lens
        letters = np.frombuffer(b"iatehn#", dtype=np.uint8)
        two = kinds == 1
        short[start[two]] = letters[rng.integers(0, letters.size, int(two.sum()))]
        three = np.flatnonzero(kinds == 2)
        w = np.frombuffer(b"".join(WORDS3), dtype=np.uint8).reshape(len(WORDS3), 3)[rng.integers(0, len(WORDS3), three.size)]
        short[start[three]], short[start[three] + 1] = w[:, 0], w[:, 1]
        blank = np.frombuffer(b"# " * (HEAP_BLANK_TILES * TILE // 2), dtype=np.uint8)
        tail = text[:SPLIT_GROUP + 777]
        while tail[-1] == SPACE:
            tail = tail[:-1]
        self.data = np.ascontiguousarray(np.concatenate([text[:HEAP_TEXT], short, blank, tail]))
        self.n = int(self.data.size)
        self.blank = (HEAP_TEXT + HEAP_SHORT, HEAP_TEXT + HEAP_SHORT + blank.size)
        self.split = split_offsets(self.data, SPACE)                              # (offsets, n_docs, tail_start): the chain's
        inside = np.arange(97, HEAP_TEXT, 97, dtype=np.uint64)
        runs = [np.full(HEAP_EMPTY_RUN, at, dtype=np.uint64) for at in HEAP_EMPTY_AT]
        off = np.sort(np.concatenate([np.union1d(self.split[0], inside)] + runs))
        self.offsets = off
        self.n_docs = int(off.size) - 1

    def storage(self):
        s = np.zeros((self.n + 16 + TILE - 1) // TILE * TILE, dtype=np.uint8)
        s[:self.n] = self.data
        return s

    def records(self, matcher, ll):
        """(pos, ids, lens) of the CPU oracle's records over the whole input."""
        pos, ids = matcher.scan_spec(self.data, None)
        pos, ids = pos.astype(np.int64), ids.astype(np.int64)
        return pos, ids, np.asarray(ll, dtype=np.int64)[ids]

    def broken(self, how):
        """The offsets with one rule broken: "decrease" at index HEAP_BREAK, "past_end" at the very end."""
        bad = self.offsets.copy()
        if how == "decrease":
            k = HEAP_BREAK
            assert self.n_docs > k + 1 and bad[k + 1] > bad[k] > 0
            bad[k + 1] = bad[k] - np.uint64(1)
        else:
            bad[-1] = np.uint64(self.n + 1)
        return bad


_HEAP = None


def heap_input():
    global _HEAP
    if _HEAP is None:
        _HEAP = HeapInput()
    return _HEAP


def heap_weights(n_ids):
    """The `weights` argument of PfacTable.state_weights for ids 1..n_ids (entry 0 unused)."""
    return [0] + [HEAP_WEIGHTS[(i - 1) % len(HEAP_WEIGHTS)] for i in range(1, n_ids + 1)]


def cut_records(pos, ids, lens, off):
    """passguard.cut_by_hand: (doc_first, pos relative to the document, ids, keep mask, document of every kept)."""
    from passguard import cut_by_hand
    return cut_by_hand(pos, ids, lens, off)


# the table of distinct single bytes: a selection is exactly the kept records, a replace is a byte map
BYTE_PATTERNS = (b"i", b"#", b"e", b"t")
BYTE_REPS = {1: b"", 2: b"<hash>", 3: b"E", 4: b"tt"}


def byte_records(data):
    """(pos, ids, lens) of BYTE_PATTERNS in `data`, by comparison -- tests/test_manydocs_cases.py holds it to the oracle."""
    ids = np.zeros(data.size, dtype=np.int64)
    for i, p in enumerate(BYTE_PATTERNS, 1):
        ids[data == p[0]] = i
    pos = np.flatnonzero(ids)
    return pos, ids[pos], np.ones(pos.size, dtype=np.int64)


def byte_replace(data, off):
    """(out, out_off) of the replace per document under BYTE_REPS: every byte maps to its replacement or to itself, and
    a document's output starts where the output of the bytes in front of it ends."""
    rep = np.frombuffer(b"".join(BYTE_REPS[i] for i in sorted(BYTE_REPS)), dtype=np.uint8)
    rlen = np.array([1] + [len(BYTE_REPS[i]) for i in sorted(BYTE_REPS)], dtype=np.int64)
    roff = np.concatenate([[0, 0], np.cumsum(rlen[1:])])           # roff[i]: where id i's replacement starts in rep
    ids = np.zeros(data.size, dtype=np.int64)
    for i, p in enumerate(BYTE_PATTERNS, 1):
        ids[data == p[0]] = i
    ln = rlen[ids]
    cum = np.concatenate([np.zeros(1, np.int64), np.cumsum(ln)])
    src = np.repeat(np.arange(data.size, dtype=np.int64), ln)
    within = np.arange(int(cum[-1]), dtype=np.int64) - cum[src]
    sid = ids[src]
    out = np.where(sid > 0, rep[np.minimum(roff[sid] + within, max(rep.size - 1, 0))], data[src]).astype(np.uint8)
    return out, cum[np.asarray(off, dtype=np.int64)].astype(np.uint64)


def _same_records(rec, pos, ids, idmap, what):
    _same(rec["pos"].astype(np.int64), pos, what, "record position")
    st = rec["state"].astype(np.int64)
    assert st.size == 0 or int(st.max()) < idmap.size, f"{what}: a state past num_final"
    _same(idmap[st], ids, what, "record pattern id")


def assert_segment(first, rec, n_kept, want_first, want_pos, want_ids, idmap, what=""):
    """The segment pass and the per-document selection: the count, every doc_first, every record."""
    assert n_kept == want_pos.size, f"{what}: {n_kept} records kept, want {want_pos.size}"
    _same(np.asarray(first, dtype=np.uint64), want_first, what, "doc_first")
    _same_records(rec, want_pos, want_ids, np.asarray(idmap, dtype=np.int64), what)


def assert_masks(masks, any_mask, want, what=""):
    _same(np.asarray(masks, dtype=np.uint64), want, what, "group mask")
    assert any_mask == int(np.bitwise_or.reduce(want)) if want.size else any_mask == 0, f"{what}: the OR of all masks is {any_mask:#x}"


def assert_scores(sc, totals, want, what=""):
    _same(sc["score"], want["score"], what, "score")
    _same(sc["count"], want["count"], what, "count")
    if totals is not None:
        t = (int(want["score"].sum()), int(want["count"].sum()))
        assert tuple(totals) == t, f"{what}: totals {tuple(totals)}, want {t}"
