"""Host reference for the proximity rules of pfac_documents_near (the checker, never the product), and the host-made
cases of tests/test_gpu_near.py with the preconditions that make them test what they are named for.  Nothing comes from
the device, and no case depends on a scan.

The rule of include/pfac.h is held twice, written differently: `near_brute` (per document and rule, every record pair
i < j) and `near_masks` (per rule, the previous A / previous B index of every record by numpy.maximum.accumulate over
masked indices, clipped at doc_first); tests/test_near_ref.py holds one against the other on every case.

A case is (states, pos, doc_first, rules) over the 16 final states of passguard.TABLES[2], whose groups are GMASK:
state 0 is an A (group 0), state 1 a B (group 1), state 2 both, state 3 is in no group, state 4 is group 63, states 5..15
are groups 2..12.  The kernels work on chunks of 64 records and blocks of 4096."""
import numpy as np

REC = np.dtype([("pos", "<u4"), ("state", "<u4")])
RULE = np.dtype([("a_groups", "<u8"), ("b_groups", "<u8"), ("max_dist", "<u4"), ("flags", "<u4"), ("reserved", "<u8")])
CHUNK, BLOCK = 64, 4096
MAX_RULES = 64
ORDERED, ANY_DIST = 1, 0xFFFFFFFF
NUM_FINAL = 16
A, B, AB, NONE, TOP = 0, 1, 2, 3, 4      # states by what they are
GA, GB, GTOP = 1 << 0, 1 << 1, 1 << 63
GMASK = np.array([GA, GB, GA | GB, 0, GTOP] + [1 << g for g in range(2, 13)], dtype=np.uint64)
assert GMASK.size == NUM_FINAL
N_SEEDS = 64


def rule(a, b, max_dist, ordered=False):
    out = np.zeros((), dtype=RULE)
    out["a_groups"], out["b_groups"], out["max_dist"], out["flags"] = a, b, max_dist, ORDERED if ordered else 0
    return out


def rules_array(rules):
    out = np.zeros(len(rules), dtype=RULE)
    for k, r in enumerate(rules):
        out[k] = r[()]
    return out


# ---------------------------------------------------------------------------
# the rule, twice

def near_brute(states, pos, first, rules, gmask=GMASK):
    """The header's words: per document and rule, every pair of distinct records i < j."""
    g = [int(x) for x in np.asarray(gmask)[np.asarray(states, dtype=np.int64)]] if len(states) else []
    p = [int(x) for x in np.asarray(pos)]
    f = [int(x) for x in np.asarray(first)]
    out = np.zeros(len(f) - 1, dtype=np.uint64)
    for d in range(len(f) - 1):
        lo, hi = f[d], f[d + 1]
        if hi - lo < 2:
            continue
        gd, pd = np.array(g[lo:hi], dtype=np.uint64), np.array(p[lo:hi], dtype=np.int64)
        for r, ru in enumerate(rules):
            a, b, md, ordered = np.uint64(ru["a_groups"]), np.uint64(ru["b_groups"]), int(ru["max_dist"]), bool(int(ru["flags"]) & ORDERED)
            isa, isb = (gd & a) != 0, (gd & b) != 0
            fired = False
            for i in range(hi - lo - 1):                        # the pairs (i, j), j behind i: the inner loop as one vector
                if not (isa[i] or (isb[i] and not ordered)):
                    continue
                near = pd[i + 1:] - pd[i] <= md
                hit = near & isb[i + 1:] if isa[i] else np.zeros(near.size, dtype=bool)
                if not ordered and isb[i]:
                    hit = hit | (near & isa[i + 1:])
                if hit.any():
                    fired = True
                    break
            if fired:
                out[d] |= np.uint64(1) << np.uint64(r)
    return out


def near_masks(states, pos, first, rules, gmask=GMASK):
    """THE reference: with a maximum distance only, the nearest earlier partner decides."""
    f = np.asarray(first, dtype=np.int64)
    n_docs, n = f.size - 1, int(f[-1]) if f.size else 0
    out = np.zeros(max(n_docs, 0), dtype=np.uint64)
    if n == 0:
        return out
    st = np.asarray(states, dtype=np.int64)
    assert st.size == n and f[0] == 0 and (np.diff(f) >= 0).all()
    g, p = np.asarray(gmask, dtype=np.uint64)[st], np.asarray(pos, dtype=np.int64)
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(f))
    start, idx = f[doc], np.arange(n, dtype=np.int64)
    assert ((np.diff(p) >= 0) | (np.diff(doc) != 0)).all(), "a position decreases inside a document"

    def partner(mine, other):
        """records j of `mine` with a record i < j of `other` in the same document"""
        prev = np.concatenate([[-1], np.maximum.accumulate(np.where(other, idx, -1))[:-1]])
        ok = mine & (prev >= start)
        return ok, prev
    for r, ru in enumerate(rules):
        isa, isb = (g & np.uint64(ru["a_groups"])) != 0, (g & np.uint64(ru["b_groups"])) != 0
        ok, prev = partner(isb, isa)
        fire = ok & (p - p[np.maximum(prev, 0)] <= int(ru["max_dist"]))
        if not int(ru["flags"]) & ORDERED:
            ok, prev = partner(isa, isb)
            fire |= ok & (p - p[np.maximum(prev, 0)] <= int(ru["max_dist"]))
        hit = np.zeros(n_docs, dtype=bool)
        hit[doc[fire]] = True
        out[hit] |= np.uint64(1) << np.uint64(r)
    return out


# ---------------------------------------------------------------------------
# the cases

class Case:
    """`sizes[d]` records in document d; `states` and `pos` in record order; `fires`: the case is meant to set a bit (and
    to leave one clear); `pre`: the precondition, asserted by `precondition()`."""

    def __init__(self, name, sizes, states, pos, rules, fires=True, pre=None):
        self.name, self.fires, self.pre = name, fires, pre
        sizes = np.asarray(sizes, dtype=np.int64)
        self.n_docs = int(sizes.size)
        self.first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        self.states = np.asarray(states, dtype=np.uint32)
        self.pos = np.asarray(pos, dtype=np.int64)
        assert self.states.size == self.pos.size == int(self.first[-1])
        assert self.pos.size == 0 or (0 <= int(self.pos.min()) and int(self.pos.max()) < 2 ** 32)
        self.rules = rules_array(rules)
        assert self.rules.size <= MAX_RULES
        self._want = None

    @property
    def n(self):
        return int(self.states.size)

    def sel(self):
        rec = np.zeros(self.n, dtype=REC)
        rec["pos"], rec["state"] = self.pos, self.states
        return rec

    def want(self):
        if self._want is None:
            self._want = near_masks(self.states, self.pos, self.first, self.rules)
        return self._want

    def doc_of(self, i):
        return int(np.searchsorted(self.first.astype(np.int64), i, side="right") - 1)

    def at(self, state):
        return np.flatnonzero(self.states == state)

    def precondition(self):
        assert self.n <= 3 * BLOCK and self.n_docs <= 10000, "a named case stays within three blocks and 10 000 documents"
        if self.pre is not None:
            held = self.pre(self)                               # (a lambda returns its condition, a function asserts)
            assert held is None or held, f"{self.name}: the precondition does not hold"


def _filled(n, gap=1):
    """n records of state NONE, `gap` bytes apart"""
    return np.full(n, NONE, dtype=np.int64), np.arange(n, dtype=np.int64) * gap


AB_ORDERED = [rule(GA, GB, 10, True), rule(GB, GA, 10, True)]      # bit 0: an A, then a B within 10; bit 1: the other way round


def _pair(name, n, ia, ib, rules=None, sizes=None, gap=1, pre=None):
    st, pos = _filled(n, gap)
    st[ia], st[ib] = A, B

    def check(c):
        assert c.at(A).tolist() == [ia] and c.at(B).tolist() == [ib]
        if pre:
            pre(c)
    return Case(name, [n] if sizes is None else sizes, st, pos, AB_ORDERED if rules is None else rules, pre=check)


def _boundary(name, at):
    """The A is the last record of document 0 (index at - 1), the B the first of document 1, one byte apart by their
    stream-relative positions: no rule fires there.  Document 2 holds a pair that does."""
    n = at + 40
    st, pos = _filled(n)
    st[at - 1], st[at] = A, B
    st[at + 20], st[at + 21] = A, B

    def check(c):
        assert c.doc_of(at - 1) == 0 and c.doc_of(at) == 1 and int(c.first[1]) == at
        assert 0 <= c.pos[at] - c.pos[at - 1] <= int(c.rules["max_dist"].min())
        assert c.want().tolist() == [0, 0, 1]
    return Case(name, [at, 10, 30], st, pos, [rule(GA, GB, 10), rule(GB, GA, 10, True)], pre=check)


def _named():
    out = []
    # the pair on both sides of a chunk edge, of a block edge, and with a whole block between them that holds no A
    out.append(_pair("lanes63-64", 200, 63, 64))
    out.append(_pair("records4095-4096", BLOCK + 100, BLOCK - 1, BLOCK))

    def far(c):
        ia, ib = int(c.at(A)[0]), int(c.at(B)[0])
        assert ia // BLOCK == 0 and ib // BLOCK == 2 and not (c.states[BLOCK:] == A).any() and c.n == 3 * BLOCK
    out.append(_pair("carry-through-blocks", 3 * BLOCK, 100, 3 * BLOCK - 1, pre=far,
                     rules=[rule(GA, GB, 3 * BLOCK, True), rule(GB, GA, 3 * BLOCK, True), rule(GA, GB, 3 * BLOCK - 102, True)]))
    out += [_boundary("boundary-in-chunk", 31), _boundary("boundary-chunk-edge", CHUNK), _boundary("boundary-block-edge", BLOCK)]
    # more than 4096 empty documents between an A and a B
    st, pos = _filled(42)
    st[0], st[1], st[20], st[21] = A, B, A, B
    sizes = np.concatenate([[1], np.zeros(5000, dtype=np.int64), [1, 40]])

    def empties(c):
        assert c.doc_of(0) == 0 and c.doc_of(1) == 5001 and (np.diff(c.first.astype(np.int64))[1:5001] == 0).all()
        assert c.want()[:5002].max() == 0 and int(c.want()[5002]) == 1
    out.append(Case("empty-run-5000", sizes, st, pos, AB_ORDERED, pre=empties))
    # one document of 10 000 records
    rng = np.random.default_rng([0x6E656172, 1])
    st = rng.choice([A, B, NONE, 5, 6], 10000, p=[0.01, 0.01, 0.9, 0.04, 0.04])
    st[rng.integers(0, 10000)] = TOP
    pos = np.cumsum(rng.integers(0, 9, 10000))
    out.append(Case("one-document-10000", [10000], st, pos, [rule(GA, GB, 50), rule(GTOP, GTOP, ANY_DIST), rule(1 << 2, 1 << 3, 0, True),
                                                               rule(1 << 2, 1 << 3, 3, True)],
                    pre=lambda c: c.n_docs == 1 and (c.states == TOP).sum() == 1))
    # 9000 documents of one record each
    st = np.tile([A, B, AB], 3000)
    out.append(Case("singletons-9000", np.ones(9000, dtype=np.int64), st, np.arange(9000), [rule(GA, GB, ANY_DIST), rule(GA, GA, ANY_DIST)],
                    fires=False, pre=lambda c: (np.diff(c.first.astype(np.int64)) == 1).all() and c.want().max() == 0))
    # exactly max_dist, and one more
    out.append(Case("distance-exact", [2, 2], [A, B, A, B], [100, 160, 100, 161], [rule(GA, GB, 60)],
                    pre=lambda c: c.want().tolist() == [1, 0]))
    out.append(Case("distance-zero", [2, 2], [A, B, A, B], [5, 5, 5, 6], [rule(GA, GB, 0), rule(GA, GB, 0, True)],
                    pre=lambda c: c.want().tolist() == [3, 0] and c.pos[0] == c.pos[1]))
    # anywhere in a document of three blocks, whose positions use all 32 bits
    st, pos = _filled(3 * BLOCK, 300000)
    st[0], st[-1] = A, B
    out.append(Case("any-distance-3-blocks", [3 * BLOCK], st, pos,
                    [rule(GA, GB, ANY_DIST, True), rule(GB, GA, ANY_DIST, True), rule(GA, GB, 2 ** 31), rule(GA, GB, ANY_DIST)],
                    pre=lambda c: c.want().tolist() == [0b1001] and int(c.pos[-1]) > 2 ** 31))
    # ties: an A and a B at one start, the B the shorter pattern and so the earlier record
    out.append(Case("tie-b-first", [2], [B, A], [7, 7], [rule(GA, GB, 5, True), rule(GB, GA, 5, True), rule(GA, GB, 5)],
                    pre=lambda c: c.want().tolist() == [0b110]))
    # A == B: two occurrences
    out.append(Case("a-equals-b", [1, 2, 3], [A, A, A, B, A, B], [0, 0, 3, 0, 1, 2], [rule(GA, GA, 3)],
                    pre=lambda c: c.want().tolist() == [0, 1, 0]))
    # a state in both classes of an ordered rule never pairs with itself
    out.append(Case("state-in-both", [1, 2, 2, 2], [AB, AB, AB, AB, B, A, AB], [4, 0, 1, 0, 1, 0, 1], [rule(GA, GB, 3, True)],
                    pre=lambda c: c.want().tolist() == [0, 1, 1, 1]))
    out.append(Case("a-groups-zero", [3], [A, B, B], [0, 1, 2], [rule(0, GB, 9), rule(GB, 0, 9), rule(GB, GB, 9)],
                    pre=lambda c: c.want().tolist() == [0b100]))
    out.append(Case("mask-zero-between", [3, 3], [A, NONE, B, B, NONE, A], [0, 1, 2, 0, 1, 2], AB_ORDERED,
                    pre=lambda c: c.want().tolist() == [1, 2] and int(GMASK[NONE]) == 0))
    # 64 rules at once, bit 63 among the fired ones; the same input with none and with one
    rng = np.random.default_rng([0x6E656172, 2])
    sizes = rng.integers(0, 60, 40)
    n = int(sizes.sum())
    st = rng.integers(0, NUM_FINAL, n)
    pos = np.cumsum(rng.integers(0, 6, n))
    groups = [GA, GB, GTOP] + [1 << g for g in range(2, 13)]
    many = [rule(groups[r % 14], groups[(r * 5 + 3) % 14], [0, 2, 7, 30, ANY_DIST][r % 5], r % 3 == 0) for r in range(63)]
    many.append(rule(GTOP, GB, 12, True))

    def top_bit(c):
        w = c.want()
        assert c.rules.size == 64 and int(w.max()) >> 63 == 1 and (w >> np.uint64(63) == 0).any()
    out.append(Case("rules-64", sizes, st, pos, many, pre=top_bit))
    out.append(Case("rules-1", sizes, st, pos, many[63:], pre=lambda c: c.rules.size == 1))
    out.append(Case("rules-0", sizes, st, pos, [], fires=False, pre=lambda c: c.rules.size == 0 and c.want().max() == 0))
    out.append(Case("no-records", np.zeros(5, dtype=np.int64), [], [], AB_ORDERED, fires=False, pre=lambda c: c.n == 0 and c.n_docs == 5))
    out.append(Case("no-documents", [], [], [], AB_ORDERED, fires=False, pre=lambda c: c.n_docs == 0))
    # one cut with the segment's document-relative positions and with the selection's stream-relative ones
    rng = np.random.default_rng([0x6E656172, 3])
    sizes = rng.integers(0, 30, 300)
    n = int(sizes.sum())
    st = rng.choice([A, B, NONE], n, p=[0.15, 0.15, 0.7])
    stream = np.cumsum(rng.integers(1, 9, n))
    doc = np.repeat(np.arange(300), sizes)
    base = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    rel = stream - stream[base[doc]]
    rr = [rule(GA, GB, 6), rule(GA, GB, 6, True), rule(GB, GB, 20)]

    def same(c):
        other = by_name()["positions-stream" if c.name == "positions-document" else "positions-document"]
        assert (c.pos != other.pos).any() and np.array_equal(c.want(), other.want())
        assert np.array_equal(c.first, other.first) and np.array_equal(c.states, other.states)
    out.append(Case("positions-document", sizes, st, rel, rr, pre=same))
    out.append(Case("positions-stream", sizes, st, stream, rr, pre=same))
    return out


def seeded(seed):
    """One of the N_SEEDS random cases: a few documents of up to some hundred records, now and then across a block edge;
    the densities keep most cases between "nothing fires" and "everything fires"."""
    rng = np.random.default_rng([0x6E656172, 0x53454544, seed])
    n_docs = int(rng.integers(2, 80))
    big = seed % 8 == 0
    sizes = rng.integers(0, 400 if big else 40, n_docs)
    sizes[rng.random(n_docs) < 0.2] = 0
    n = int(sizes.sum())
    st = np.where(rng.random(n) < 0.6, NONE, rng.integers(0, NUM_FINAL, n))
    gaps = rng.integers(0, 12, n)
    if seed % 2:                                                # stream-relative
        pos = np.cumsum(gaps)
    else:
        doc = np.repeat(np.arange(n_docs), sizes)
        c = np.cumsum(gaps)
        base = np.concatenate([[0], np.cumsum(sizes)])[:-1]
        pos = c - c[np.minimum(base[doc], max(n - 1, 0))] if n else c
    groups = [GA, GB, GA | GB, GTOP] + [1 << g for g in range(2, 13)]
    n_rules = int(rng.choice([1, 2, 3, 5, 8, 17, 64]))
    rules = [rule(groups[int(rng.integers(0, len(groups)))], groups[int(rng.integers(0, len(groups)))],
                  int(rng.choice([0, 1, 4, 15, 60, ANY_DIST])), bool(rng.integers(0, 2))) for _ in range(n_rules)]
    return Case(f"seed{seed}", sizes, st, pos, rules, fires=False)


_NAMED, _SEEDED = None, {}


def by_name():
    global _NAMED
    if _NAMED is None:
        _NAMED = {c.name: c for c in _named()}
    return _NAMED


NAMES = ("lanes63-64", "records4095-4096", "carry-through-blocks", "boundary-in-chunk", "boundary-chunk-edge", "boundary-block-edge",
         "empty-run-5000", "one-document-10000", "singletons-9000", "distance-exact", "distance-zero", "any-distance-3-blocks",
         "tie-b-first", "a-equals-b", "state-in-both", "a-groups-zero", "mask-zero-between", "rules-64", "rules-1", "rules-0",
         "no-records", "no-documents", "positions-document", "positions-stream")
ALL = NAMES + tuple(f"seed{s}" for s in range(N_SEEDS))


def case(name):
    """A named case, or seed<k>."""
    if name.startswith("seed"):
        k = int(name[4:])
        if k not in _SEEDED:
            _SEEDED[k] = seeded(k)
        return _SEEDED[k]
    return by_name()[name]


def check(want, got, what="near masks"):
    want, got = np.asarray(want), np.asarray(got)
    assert got.dtype == np.uint64 and got.size == want.size, f"{what}: {got.size} masks ({got.dtype}), want {want.size}"
    ne = np.flatnonzero(got != want)
    assert ne.size == 0, (f"{what}: {ne.size} of {want.size} documents differ, first {int(ne[0])}: 0x{int(got[ne[0]]):x}, "
                          f"want 0x{int(want[ne[0]]):x}")
