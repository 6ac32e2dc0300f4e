"""Host reference for term counts per document (the checker, never the product): the distinct (document, state) pairs of
a record array that is cut per document, with their multiplicities, as the three CSR arrays of
pfac_documents_term_counts -- and the host-made cases of tests/test_gpu_terms.py with the preconditions that make them
test what they are named for.  Nothing comes from the device, and no case depends on a scan.

The rule is held twice: `term_counts` (numpy.unique of packed keys, row_ptr by searchsorted) and `term_counts_by_counter`
(a collections.Counter per document); tests/test_terms_ref.py holds one against the other on every case.  `check` is
what a device result is compared with; the same file shows that it refuses four kinds of wrong result.

A case is (sel, doc_first, n_docs, num_final): `W` names the table whose num_final it is made for -- passguard.TABLES[2]
(16 lines, 16 final states: 4 state bits) or passguard.TABLES[4] (the dictionary: 13 state bits)."""
import collections

import numpy as np

REC = np.dtype([("pos", "<u4"), ("state", "<u4")])
BLOCK, SORT_BLOCK, GROUP = 64, 1024, 4096       # a head ballot's records, a sort chunk's keys, a compaction group's records
SORT_ROWS = 4096                                # PFAC_TERMS_SORT_ROWS: the most workgroups of a sort pass
EDGES = (BLOCK, SORT_BLOCK, GROUP)
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 4096 + 5, 16454)
BIG_N = 1025 * 4096 + 1                         # more than 1024 groups of 4096, and a sort of more than 4 workgroups
EMPTY_RUNS = (230, 70000)
PASS_DOCS = (1, 2, 16, 17, 2048, 2049, 524288, 524289)
PASS_N = 3000                                   # records of a pass-count case (several sort blocks) ...
PASS_N_ONE = 700                                # ... and of its twin that one workgroup sorts
CHUNKED_ROWS = 3                                # the GPU test's limit on the workgroups of a sort pass, ...
CHUNKED = ("n4097", "n16454", "run3000", "big")       # ... for these cases: several chunks per workgroup
WANT_PASSES = {2: (1, 1, 1, 2, 2, 2, 3, 3), 4: (2, 2, 3, 3, 3, 4, 4, 5)}      # per PASS_DOCS entry


def bit_width(v):
    return int(v).bit_length()


def state_bits(num_final):
    return bit_width(max(int(num_final) - 1, 0))


def sort_passes(n_docs, num_final):
    """Passes of 8 bits over the packed key doc << sbits | state (the header's formula)."""
    return (state_bits(num_final) + bit_width(max(int(n_docs) - 1, 0)) + 7) // 8


def sort_shape(n, rows=SORT_ROWS):
    """(chunks per workgroup, workgroups, trips of 256 counts of the prefix over a digit's row) of the sort of n keys, by
    the header's rule; (0, 0, 0) where one workgroup sorts alone.  `rows`: the limit on the workgroups."""
    if n <= SORT_BLOCK:
        return 0, 0, 0
    n_chunks = -(-n // SORT_BLOCK)
    chunks = max(1, -(-n_chunks // rows))
    n_blocks = -(-n_chunks // chunks)
    return chunks, n_blocks, -(-n_blocks // 256)


# ---------------------------------------------------------------------------
# the rule, twice

def docs_of(first):
    f = np.asarray(first, dtype=np.int64)
    return np.repeat(np.arange(f.size - 1, dtype=np.int64), np.diff(f))


def term_counts(states, first, num_final):
    """THE reference: (row_ptr uint64[n_docs + 1], states uint32[n_terms], counts uint32[n_terms])."""
    f = np.asarray(first, dtype=np.int64)
    st = np.asarray(states, dtype=np.int64)
    assert f[0] == 0 and f[-1] == st.size and (np.diff(f) >= 0).all()
    assert st.size == 0 or (0 <= int(st.min()) and int(st.max()) < num_final)
    sb = state_bits(num_final)
    uniq, cnt = np.unique(docs_of(f) << sb | st, return_counts=True)
    row = np.searchsorted(uniq >> sb, np.arange(f.size, dtype=np.int64), side="left")
    return row.astype(np.uint64), (uniq & ((1 << sb) - 1)).astype(np.uint32), cnt.astype(np.uint32)


def term_counts_by_counter(states, first, num_final):
    """The same in the header's words, one document at a time."""
    f = [int(x) for x in np.asarray(first)]
    st = np.asarray(states).tolist()
    row, out_s, out_c = [0], [], []
    for d in range(len(f) - 1):
        if f[d + 1] > f[d]:
            for s, c in sorted(collections.Counter(st[f[d]:f[d + 1]]).items()):
                assert 0 <= s < num_final
                out_s.append(s)
                out_c.append(c)
        row.append(len(out_s))
    return np.array(row, dtype=np.uint64), np.array(out_s, dtype=np.uint32), np.array(out_c, dtype=np.uint32)


def dense(row, states, counts, num_final):
    """The matrix (n_docs, num_final) as int64, for the smallest cases."""
    r = np.asarray(row, dtype=np.int64)
    out = np.zeros((r.size - 1, num_final), dtype=np.int64)
    out[np.repeat(np.arange(r.size - 1), np.diff(r)), np.asarray(states, dtype=np.int64)] = np.asarray(counts, dtype=np.int64)
    return out


def check(want, row, states, counts, what="term counts"):
    """AssertionError unless (row, states, counts) is `want` (a triple of `term_counts`): the structure first, in words,
    then every entry."""
    wr, ws, wc = want
    row, states, counts = np.asarray(row), np.asarray(states), np.asarray(counts)
    assert row.size == wr.size, f"{what}: row_ptr has {row.size} entries, want {wr.size}"
    assert states.size == ws.size and counts.size == wc.size, f"{what}: {states.size} states and {counts.size} counts, want {ws.size}"
    r = row.astype(np.int64)
    assert r[0] == 0 and r[-1] == ws.size, f"{what}: row_ptr runs from {int(r[0])} to {int(r[-1])}, want 0 to {ws.size}"
    assert (np.diff(r) >= 0).all(), f"{what}: row_ptr decreases at document {int(np.flatnonzero(np.diff(r) < 0)[0])}"
    ne = np.flatnonzero(row != wr)
    assert ne.size == 0, f"{what}: row_ptr differs at {ne.size} documents, first {int(ne[0])}: {int(row[ne[0]])}, want {int(wr[ne[0]])}"
    if ws.size:
        inner = np.ones(ws.size, dtype=bool)                    # entry j and j - 1 lie in one document
        inner[r[:-1][r[:-1] < ws.size]] = False
        up = np.diff(states.astype(np.int64), prepend=-1) > 0
        bad = np.flatnonzero(inner & ~up)
        assert bad.size == 0, f"{what}: the states do not strictly ascend inside a document, first at entry {int(bad[0])}"
    ne = np.flatnonzero(states != ws)
    assert ne.size == 0, f"{what}: {ne.size} states differ, first at entry {int(ne[0])}: {int(states[ne[0]])}, want {int(ws[ne[0]])}"
    ne = np.flatnonzero(counts != wc)
    assert ne.size == 0, f"{what}: {ne.size} counts differ, first at entry {int(ne[0])}: {int(counts[ne[0]])}, want {int(wc[ne[0]])}"


# ---------------------------------------------------------------------------
# the cases

_NUM_FINAL = {2: 16}


def num_final(W):
    """num_final of passguard.TABLES[W] (2: the 16 lines; 4: the dictionary, built on the host)."""
    if W not in _NUM_FINAL:
        import passguard
        _NUM_FINAL[W] = int(passguard.cpu().table(W).num_final)
    return _NUM_FINAL[W]


class Case:
    """`sizes[d]` records in document d, `states` in input order; positions are junk, since the pass does not read them."""

    def __init__(self, name, W, sizes, states):
        self.name, self.W = name, W
        sizes = np.asarray(sizes, dtype=np.int64)
        self.n_docs = int(sizes.size)
        self.first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        self.states = np.asarray(states, dtype=np.uint32)
        assert self.states.size == int(self.first[-1])
        self._want = None

    @property
    def n(self):
        return int(self.states.size)

    @property
    def num_final(self):
        return num_final(self.W)

    @property
    def passes(self):
        return sort_passes(self.n_docs, self.num_final)

    def sel(self):
        rec = np.zeros(self.n, dtype=REC)
        rec["pos"] = (np.arange(self.n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
        rec["state"] = self.states
        return rec

    def want(self):
        if self._want is None:
            self._want = term_counts(self.states, self.first, self.num_final)
        return self._want

    def sorted_keys(self):
        sb = state_bits(self.num_final)
        return np.sort(docs_of(self.first) << sb | self.states.astype(np.int64))

    def runs_across(self, edge):
        """Runs of equal (document, state) records of two or more that lie on both sides of a multiple of `edge` in
        the sorted order."""
        k = self.sorted_keys()
        at = np.arange(edge, k.size, edge)
        return int((k[at] == k[at - 1]).sum()) if at.size else 0

    def empty_runs(self):
        """[(first document, length, record index)] of the maximal runs of empty documents."""
        empty = np.diff(self.first.astype(np.int64)) == 0
        edge = np.flatnonzero(np.diff(np.concatenate([[False], empty, [False]]).astype(np.int8)))
        return [(int(a), int(b - a), int(self.first[a])) for a, b in zip(edge[::2], edge[1::2])]


def _rng(*key):
    return np.random.default_rng([0x7465726D, *key])


def _states(rng, n, nf):
    """n states below nf: half from a pool of seven (so that pairs repeat under a large table too), the last one nf - 1."""
    pool = np.concatenate([rng.integers(0, nf, 6), [nf - 1]])
    st = np.where(rng.random(n) < 0.5, pool[rng.integers(0, pool.size, n)], rng.integers(0, nf, n))
    if n:
        st[-1] = nf - 1
    return st


def _random(name, W, n_docs, n, seed):
    """n records over n_docs documents at random; the last document and the last state are used."""
    rng = _rng(seed, n_docs, n)
    sizes = np.bincount(rng.integers(0, n_docs, n), minlength=n_docs) if n_docs else np.empty(0, dtype=np.int64)
    if n and sizes[-1] == 0:
        sizes[int(np.flatnonzero(sizes)[-1])] -= 1
        sizes[-1] = 1
    return Case(name, W, sizes, _states(rng, n, num_final(W)))


def _empties(run):
    """Runs of `run` empty documents at the front, in the middle of a block of 64 records, where a block of 64 records
    begins, and at the end; three to nine records in the documents between them."""
    rng = _rng(3, run)
    parts, total = [np.zeros(run, dtype=np.int64)], 0

    def filled(until_multiple_of_block):
        nonlocal total
        s = rng.integers(3, 10, 40)
        if until_multiple_of_block:
            s[-1] += (-(total + int(s.sum()))) % BLOCK
        total += int(s.sum())
        return s
    parts += [filled(False), np.zeros(run, dtype=np.int64)]
    assert total % BLOCK
    parts += [filled(True), np.zeros(run, dtype=np.int64)]
    assert total % BLOCK == 0
    parts += [filled(False), np.zeros(run, dtype=np.int64)]
    sizes = np.concatenate(parts)
    return Case(f"empty{run}", 2, sizes, _states(rng, int(sizes.sum()), 16))


_CASES = {}


def cases(W):
    """The cases made for passguard.TABLES[W], by name."""
    if W in _CASES:
        return _CASES[W]
    out = []
    nf = num_final(W)
    if W == 2:
        for n in SIZES:
            out.append(_random(f"n{n}", 2, max(3, n // 5), n, 1))
        out.append(Case("nodocs", 2, [], []))
        out.append(_random("big", 2, 300000, BIG_N, 2))
        # one (document, state) run of 3000 records behind 4000 records of four runs of 1000: it starts at 4000 and lies
        # across a 64, a 1024 and a 4096 boundary; the input order is shuffled inside document 0
        rng = _rng(4)
        out.append(Case("run3000", 2, [4000, 3000, 100], np.concatenate([rng.permutation(np.repeat([0, 1, 2, 3], 1000)),
                                                                          np.full(3000, 5), rng.integers(0, 16, 100)])))
        out.append(Case("distinct", 2, np.full(300, 16), np.concatenate([_rng(5, d).permutation(16) for d in range(300)])))
        out.append(Case("equal", 2, [5000], np.full(5000, 3)))
        out += [_empties(run) for run in EMPTY_RUNS]
        rng = _rng(6)
        desc = [np.sort(rng.integers(0, 16, int(k)))[::-1] for k in rng.integers(0, 40, 200)]
        out.append(Case("descending", 2, [d.size for d in desc], np.concatenate(desc)))
        out.append(Case("same", 2, np.full(500, 4), np.tile([7, 2, 11, 7], 500)))
    for n_docs in PASS_DOCS:
        out.append(_random(f"passes-d{n_docs}", W, n_docs, PASS_N, 7))
    for n_docs in (17, 524289):
        out.append(_random(f"passes-one-d{n_docs}", W, n_docs, PASS_N_ONE, 8))
    assert all(int(c.states.max(initial=0)) < nf for c in out)
    _CASES[W] = {c.name: c for c in out}
    return _CASES[W]


def names(W):
    """The case names of a table without building a case (parametrize ids)."""
    out = []
    if W == 2:
        out += [f"n{n}" for n in SIZES] + ["nodocs", "big", "run3000", "distinct", "equal"] + [f"empty{r}" for r in EMPTY_RUNS]
        out += ["descending", "same"]
    return out + [f"passes-d{d}" for d in PASS_DOCS] + [f"passes-one-d{d}" for d in (17, 524289)]
