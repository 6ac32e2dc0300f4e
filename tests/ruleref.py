"""Host reference for rule sets per document (the checker, never the product): which rules of a rule table fire in each
row of a document-term matrix, as the CSR of pfac_documents_rules -- and the host-made cases of tests/test_gpu_rules.py
with the preconditions that make them test what they are named for.  Nothing comes from the device, and no case depends
on a scan.

Rule r = (P_r, N_r, need_r) fires in document d with states S_d iff |P_r & S_d| >= need_r and N_r & S_d is empty.  The
rule is held three times: `fired_sets` (Python sets, one document at a time, in the header's words), `fired_dense`
(presence @ positive >= need and presence @ negative == 0, for small shapes) and `fired` (numpy over the expanded
(document, rule) entries, which is what the large cases are judged by); tests/test_rules_ref.py holds them against each
other.  `check` is what a device result is compared with; the same file shows that it refuses five kinds of wrong result.

A case is a matrix (row_ptr, states) and a rule table (rule_ptr, terms, need); `W` names the table whose num_final it
is made for -- passguard.TABLES[2] (16 final states) or passguard.TABLES[4] (the dictionary)."""
import numpy as np

from termref import bit_width, docs_of, num_final

NOT = 0x80000000
BLOCK, SORT_BLOCK, GROUP = 64, 1024, 4096       # a ballot's entries, a sort chunk's keys, a group's pairs or entries
EDGES = (BLOCK, SORT_BLOCK, GROUP)
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 4096 + 5)
BIG_E = 1025 * 4096 + 1                         # the group prefix of the fired tails runs past 1024 groups
EMPTY_RUNS = (230, 70000)
PASS_RULES = (1, 2, 64, 65, 2 ** 15 + 1)
PASS_DOCS = (1, 2, 17, 2049, 524289)
PASS_E = 40000                                  # keys of a pass-count case, about (several sort chunks)
FAN = 3000                                      # rules that name one state (more than the expand's 256 lanes, across blocks)
CHUNKED_ROWS = 3                                # the GPU test's limit on the workgroups of a sort pass, ...
CHUNKED = ("E4097", "E12293", "fan3000", "big")         # ... for these cases: several chunks per workgroup


def sort_passes(n_docs, n_rules):
    """Passes of 8 bits over the key doc << (rbits + 1) | rule << 1 | negated (the header's formula)."""
    return (bit_width(max(int(n_docs) - 1, 0)) + bit_width(max(int(n_rules) - 1, 0)) + 1 + 7) // 8


# ---------------------------------------------------------------------------
# the rule table

class Rules:
    """rule-major (rule_ptr uint64, terms uint32 with bit 31 = negated, need uint32) and its state-major inverse."""

    def __init__(self, rules, nf):
        """`rules`: [(positive states, negated states, need)]."""
        self.nf = int(nf)
        ptr, terms, need = [0], [], []
        for p, n, k in rules:
            p, n = [int(s) for s in p], [int(s) for s in n]
            assert p and 1 <= int(k) <= len(p) and len(set(p + n)) == len(p) + len(n) and all(0 <= s < nf for s in p + n)
            terms += p + [s | NOT for s in n]
            need.append(int(k))
            ptr.append(len(terms))
        self.rule_ptr = np.array(ptr, dtype=np.uint64)
        self.terms = np.array(terms, dtype=np.uint32)
        self.need = np.array(need, dtype=np.uint32)
        self._inv = None

    @classmethod
    def from_arrays(cls, rule_ptr, terms, need, nf):
        self = cls([], nf)
        self.rule_ptr, self.terms, self.need = rule_ptr.astype(np.uint64), terms.astype(np.uint32), need.astype(np.uint32)
        return self

    @property
    def n_rules(self):
        return int(self.need.size)

    def as_sets(self):
        ptr = self.rule_ptr.astype(np.int64)
        out = []
        for r in range(self.n_rules):
            t = self.terms[ptr[r]:ptr[r + 1]].astype(np.int64)
            out.append((set((t[t < NOT]).tolist()), set((t[t >= NOT] - NOT).tolist()), int(self.need[r])))
        return out

    def inverse(self):
        """(state_ptr int64[nf + 1], entries int64 = rule << 1 | negated, the rules ascending inside a state)."""
        if self._inv is None:
            t = self.terms.astype(np.int64)
            rule = np.repeat(np.arange(self.n_rules, dtype=np.int64), np.diff(self.rule_ptr.astype(np.int64)))
            st, neg = t & (NOT - 1), t >> 31
            order = np.lexsort((rule, st))
            sptr = np.concatenate([[0], np.cumsum(np.bincount(st, minlength=self.nf))]).astype(np.int64)
            self._inv = (sptr, (rule << 1 | neg)[order])
        return self._inv

    def degree(self):
        return np.diff(self.inverse()[0])


# ---------------------------------------------------------------------------
# the rule, three times

def expand(row, states, rules):
    """(document, entry) of every key, in pair order: what the device sorts."""
    sptr, ent = rules.inverse()
    st = np.asarray(states, dtype=np.int64)
    c = sptr[st + 1] - sptr[st]
    pair = np.repeat(np.arange(st.size, dtype=np.int64), c)
    within = np.arange(int(c.sum()), dtype=np.int64) - np.repeat(np.cumsum(c) - c, c)
    return docs_of(row)[pair], ent[sptr[st[pair]] + within]


def fired(row, states, rules, bug=None):
    """THE reference: (row_ptr uint64[n_docs + 1], rules uint32[n_fired]).  `bug` makes it wrong on purpose, for the
    checker's own test: "noneg" ignores negated terms, "need" asks for one term too few, "merge" counts a rule's terms
    over pairs of neighbouring documents."""
    r = np.asarray(row, dtype=np.int64)
    st = np.asarray(states, dtype=np.int64)
    assert r[0] == 0 and r[-1] == st.size and (np.diff(r) >= 0).all()
    inner = np.ones(st.size, dtype=bool)
    inner[r[:-1][r[:-1] < st.size]] = False
    assert (np.diff(st, prepend=-1)[inner] > 0).all() and (st.size == 0 or (st.min() >= 0 and st.max() < rules.nf))
    doc, ent = expand(r, st, rules)
    nr = max(rules.n_rules, 1)
    gdoc = doc // 2 if bug == "merge" else doc
    key = gdoc * nr + (ent >> 1)
    uniq, inv = np.unique(key, return_inverse=True)
    neg = (ent & 1).astype(np.int64)
    pos_n = np.bincount(inv, weights=1 - neg, minlength=uniq.size).astype(np.int64)
    neg_n = np.bincount(inv, weights=neg, minlength=uniq.size).astype(np.int64)
    need = rules.need.astype(np.int64)[uniq % nr] if uniq.size else np.empty(0, dtype=np.int64)
    if bug == "need":
        need = np.maximum(need - 1, 1)
    fire = pos_n >= need
    if bug != "noneg":
        fire &= neg_n == 0
    hit = uniq[fire]
    hd = hit // nr * (2 if bug == "merge" else 1)
    out_row = np.searchsorted(hd, np.arange(r.size, dtype=np.int64), side="left")
    return out_row.astype(np.uint64), (hit % nr).astype(np.uint32)


def fired_sets(row, states, rules):
    """The same in the header's words, one document at a time."""
    r = [int(x) for x in np.asarray(row)]
    st = np.asarray(states).tolist()
    table = rules.as_sets()
    touching = {}
    for k, (p, n, _) in enumerate(table):
        for s in p | n:
            touching.setdefault(s, []).append(k)
    out_row, out = [0], []
    for d in range(len(r) - 1):
        S = set(st[r[d]:r[d + 1]])
        for k in sorted({k for s in S for k in touching.get(s, ())}):
            p, n, need = table[k]
            if len(p & S) >= need and not (n & S):
                out.append(k)
        out_row.append(len(out))
    return np.array(out_row, dtype=np.uint64), np.array(out, dtype=np.uint32)


def dense(row, cols, n_cols):
    """A CSR of ones as an int64 matrix (n_docs, n_cols), for the smallest cases."""
    r = np.asarray(row, dtype=np.int64)
    out = np.zeros((r.size - 1, n_cols), dtype=np.int64)
    out[np.repeat(np.arange(r.size - 1), np.diff(r)), np.asarray(cols, dtype=np.int64)] = 1
    return out


def fired_dense(row, states, rules):
    """presence @ positive >= need and presence @ negative == 0, as the int64 matrix (n_docs, n_rules)."""
    presence = dense(row, states, rules.nf)
    pos = np.zeros((rules.nf, rules.n_rules), dtype=np.int64)
    neg = np.zeros((rules.nf, rules.n_rules), dtype=np.int64)
    for k, (p, n, _) in enumerate(rules.as_sets()):
        pos[list(p), k] = 1
        neg[list(n), k] = 1
    return ((presence @ pos >= rules.need.astype(np.int64)[None, :]) & (presence @ neg == 0)).astype(np.int64)


def check(want, row, fired_rules, what="rules"):
    """AssertionError unless (row, fired_rules) is `want` (a pair of `fired`): the structure first, in words, then
    every entry."""
    wr, wf = want
    row, got = np.asarray(row), np.asarray(fired_rules)
    assert row.size == wr.size, f"{what}: row_ptr has {row.size} entries, want {wr.size}"
    assert got.size == wf.size, f"{what}: {got.size} fired rules, want {wf.size}"
    r = row.astype(np.int64)
    assert r[0] == 0 and r[-1] == wf.size, f"{what}: row_ptr runs from {int(r[0])} to {int(r[-1])}, want 0 to {wf.size}"
    assert (np.diff(r) >= 0).all(), f"{what}: row_ptr decreases at document {int(np.flatnonzero(np.diff(r) < 0)[0])}"
    ne = np.flatnonzero(row != wr)
    assert ne.size == 0, f"{what}: row_ptr differs at {ne.size} documents, first {int(ne[0])}: {int(row[ne[0]])}, want {int(wr[ne[0]])}"
    if wf.size:
        inner = np.ones(wf.size, dtype=bool)
        inner[r[:-1][r[:-1] < wf.size]] = False
        bad = np.flatnonzero(inner & ~(np.diff(got.astype(np.int64), prepend=-1) > 0))
        assert bad.size == 0, f"{what}: the rule ids do not strictly ascend inside a document, first at entry {int(bad[0])}"
    ne = np.flatnonzero(got != wf)
    assert ne.size == 0, f"{what}: {ne.size} rule ids differ, first at entry {int(ne[0])}: {int(got[ne[0]])}, want {int(wf[ne[0]])}"


# ---------------------------------------------------------------------------
# the cases

class Case:
    def __init__(self, name, W, row, states, rules):
        self.name, self.W, self.rules = name, W, rules
        self.row = np.asarray(row, dtype=np.uint64)
        self.states = np.asarray(states, dtype=np.uint32)
        assert int(self.row[-1]) == self.states.size and rules.nf == num_final(W)
        self._want = self._keys = None

    @property
    def n_docs(self):
        return int(self.row.size - 1)

    @property
    def n(self):
        return int(self.states.size)

    @property
    def num_final(self):
        return self.rules.nf

    @property
    def passes(self):
        return sort_passes(self.n_docs, self.rules.n_rules)

    def want(self):
        if self._want is None:
            self._want = fired(self.row, self.states, self.rules)
        return self._want

    def sorted_keys(self):
        """The device's sorted keys, as (document, rule, negated) packed into int64."""
        if self._keys is None:
            doc, ent = expand(self.row, self.states, self.rules)
            self._keys = np.sort(doc << (bit_width(max(self.rules.n_rules - 1, 0)) + 1) | ent)
        return self._keys

    @property
    def E(self):
        return int(self.sorted_keys().size)

    def firing_tails(self):
        """[(tail index, need)] of the runs that fire, in sorted order."""
        k = self.sorted_keys()
        rb = bit_width(max(self.rules.n_rules - 1, 0))
        run = k >> 1
        tail = np.flatnonzero(np.concatenate([run[1:] != run[:-1], [True]])) if k.size else np.empty(0, dtype=np.int64)
        need = self.rules.need.astype(np.int64)[run[tail] & ((1 << rb) - 1)]
        ok = ((k[tail] & 1) == 0) & (tail >= need - 1)
        ok[ok] = run[tail[ok] - (need[ok] - 1)] == run[tail[ok]]
        return tail[ok], need[ok]

    def reaches_back_over(self, edge):
        """Firing runs whose tail lies at or past a multiple of `edge` and whose need-th entry from the tail in front of it."""
        t, need = self.firing_tails()
        return int(((t // edge) != ((t - (need - 1)) // edge)).sum())

    def empty_runs(self):
        """[(first document, length)] of the maximal runs of documents without a pair."""
        empty = np.diff(self.row.astype(np.int64)) == 0
        edge = np.flatnonzero(np.diff(np.concatenate([[False], empty, [False]]).astype(np.int8)))
        return [(int(a), int(b - a)) for a, b in zip(edge[::2], edge[1::2])]


def _rng(*key):
    return np.random.default_rng([0x72756C65, *key])


def random_rules(rng, n_rules, nf, lo=2, hi=4, negated=0.25, spare=()):
    """n_rules rules of lo..hi distinct states not in `spare`, the first term positive, the others negated with
    probability `negated`; need uniform in 1..|P|.  Vectorised: 2^15 + 1 rules are made at once."""
    pool = np.setdiff1d(np.arange(nf), np.asarray(spare, dtype=np.int64))
    hi = min(hi, pool.size)
    lo = min(lo, hi)
    size = rng.integers(lo, hi + 1, n_rules)
    if pool.size <= 64:                                         # a permutation of the pool per rule
        pick = pool[np.argsort(rng.random((n_rules, pool.size)), axis=1)[:, :hi]]
    else:                                                       # one state per residue class mod hi: distinct without one
        pick = pool[rng.integers(0, pool.size // hi, (n_rules, hi)) * hi + np.arange(hi)[None, :]]
    keep = np.arange(hi)[None, :] < size[:, None]
    neg = (rng.random((n_rules, hi)) < negated) & keep
    neg[:, 0] = False
    order = np.argsort(neg, axis=1, kind="stable")                  # positives first inside a rule
    pick, neg, keep2 = np.take_along_axis(pick, order, 1), np.take_along_axis(neg, order, 1), np.take_along_axis(keep, order, 1)
    n_pos = (keep2 & ~neg).sum(axis=1)
    need = 1 + (rng.integers(0, 1 << 30, n_rules) % n_pos)
    terms = (pick | np.where(neg, NOT, 0))[keep2]
    ptr = np.concatenate([[0], np.cumsum(keep2.sum(axis=1))])
    return Rules.from_arrays(ptr, terms, need, nf)


def random_matrix(rng, n_docs, n_pairs, nf, hot=None):
    """About n_pairs distinct (document, state) pairs, sorted: (row_ptr, states).  `hot`: half the states from this pool."""
    if n_docs == 0 or n_pairs == 0:
        return np.zeros(n_docs + 1, dtype=np.uint64), np.empty(0, dtype=np.uint32)
    st = rng.integers(0, nf, n_pairs)
    if hot is not None:
        st = np.where(rng.random(n_pairs) < 0.5, np.asarray(hot)[rng.integers(0, len(hot), n_pairs)], st)
    key = np.unique(rng.integers(0, n_docs, n_pairs) * nf + st)
    row = np.searchsorted(key // nf, np.arange(n_docs + 1), side="left")
    return row.astype(np.uint64), (key % nf).astype(np.uint32)


def from_docs(name, W, docs, rules):
    """A case from a list of per-document state collections."""
    docs = [sorted(set(int(s) for s in d)) for d in docs]
    row = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    return Case(name, W, row, np.array([s for d in docs for s in d], dtype=np.uint32), rules)


def _sized(name, W, E, seed):
    """Exactly E keys: random rules in which the last state is in ONE rule and the state before it in none; a random
    matrix cut where its keys reach E, topped up with documents that hold the last state alone (one key each)."""
    nf = num_final(W)
    rng = _rng(seed, E)
    rules = random_rules(rng, 64 if nf <= 16 else 4096, nf, spare=(nf - 2, nf - 1))
    one = Rules([([nf - 1], [], 1)], nf)
    rules = Rules.from_arrays(np.concatenate([rules.rule_ptr, [rules.rule_ptr[-1] + np.uint64(1)]]), np.concatenate([rules.terms, one.terms]),
                              np.concatenate([rules.need, one.need]), nf)
    deg = rules.degree()
    assert deg[nf - 1] == 1 and deg[nf - 2] == 0 and deg.max() > 1
    mean = max(float(deg.mean()), 0.5)
    n_pairs = int(E / mean * 1.3) + 8
    row, st = random_matrix(rng, max(3, n_pairs // 4), n_pairs, nf)
    cum = np.cumsum(deg[st.astype(np.int64)])
    keep = int(np.searchsorted(cum, E, side="right"))             # the longest prefix with at most E keys
    assert keep < st.size, "the random matrix is too small"
    d_cut = int(np.searchsorted(row.astype(np.int64), keep, side="right"))     # documents [0, d_cut) lie inside it, whole or cut
    rem = E - (int(cum[keep - 1]) if keep else 0)
    sizes = np.diff(np.minimum(row[: d_cut + 1].astype(np.int64), keep))
    sizes = np.concatenate([sizes, np.ones(rem + 5, dtype=np.int64)])      # ... and five that hold the state in no rule
    c = Case(name, W, np.concatenate([[0], np.cumsum(sizes)]), np.concatenate([st[:keep], np.full(rem, nf - 1), np.full(5, nf - 2)]), rules)
    assert c.E == E and c.n >= 5
    return c


def _edge(edge):
    """Rule 0 names all 16 states and needs them all; rule 1 is state 0 alone.  Documents with state 0 alone (two keys
    each: rule 0 does not fire, rule 1 does) in front of a full document whose run of 16 starts 8 keys in front of `edge`."""
    rules = Rules([(range(16), [], 16), ([0], [], 1)], 16)
    c = from_docs(f"edge{edge}", 2, [[0]] * ((edge - 8) // 2) + [range(16)] + [[0]] * 3, rules)
    t, need = c.firing_tails()
    assert ((need == 16) & (t == edge + 7)).sum() == 1 and c.reaches_back_over(edge) >= 1
    return c


def _empties(run):
    """Runs of `run` empty documents at the front, inside, where a block of 64 keys begins, and at the end.  One rule per
    state, need 1: a pair is one key, so key indices are pair indices."""
    rng = _rng(3, run)
    rules = Rules([([s], [], 1) for s in range(16)], 16)
    parts, total = [np.zeros(run, dtype=np.int64)], 0

    def filled(until_multiple_of_block):
        nonlocal total
        s = rng.integers(3, 10, 40).tolist()
        pad = (-(total + sum(s))) % BLOCK if until_multiple_of_block else 0
        while pad:                                              # (a document holds 16 distinct states at most)
            s.append(min(pad, 16))
            pad -= s[-1]
        total += sum(s)
        return np.array(s, dtype=np.int64)
    parts += [filled(False), np.zeros(run, dtype=np.int64)]
    assert total % BLOCK
    parts += [filled(True), np.zeros(run, dtype=np.int64)]
    assert total % BLOCK == 0
    parts += [filled(False), np.zeros(run, dtype=np.int64)]
    sizes = np.concatenate(parts)
    st = np.concatenate([np.sort(rng.permutation(16)[:k]) for k in sizes[sizes > 0]])
    c = Case(f"empty{run}", 2, np.concatenate([[0], np.cumsum(sizes)]), st, rules)
    runs = c.empty_runs()
    assert [ln for _, ln in runs] == [run] * 4 and runs[0][0] == 0 and runs[-1][0] + run == c.n_docs
    assert int(c.row[runs[2][0]]) % BLOCK == 0 and int(c.row[runs[1][0]]) % BLOCK and c.E == c.n
    return c


_CASES = {}


def cases(W):
    """The cases made for passguard.TABLES[W], by name."""
    if W in _CASES:
        return _CASES[W]
    nf = num_final(W)
    out = []
    for E in SIZES if W == 2 else (0, 1025, 4097):
        out.append(_sized(f"E{E}", W, E, 1))
    rng = _rng(5, W)
    out.append(Case("random", W, *random_matrix(rng, 700, 6000, nf, hot=rng.integers(0, nf, 12)),
                    random_rules(rng, 500, nf, negated=0.3)))
    # need = 1, k of n, all, over every subset of four states; a negated term present, absent, and alone
    a, b, c_, d_ = (0, 1, 2, 3) if W == 2 else (5, nf // 3, nf // 2, nf - 1)
    subsets = [[s for k, s in enumerate((a, b, c_, d_)) if m >> k & 1] for m in range(16)]
    out.append(from_docs("need", W, subsets, Rules([((a, b, c_, d_), [], k) for k in (1, 2, 3, 4)], nf)))
    out.append(from_docs("negated", W, [[a, b], [a], [b], [a, c_], [b, c_], []],
                         Rules([([a], [b], 1), ([a, c_], [b], 1), ([c_], [a, b], 1)], nf)))
    if W == 2:
        out.append(_sized("big", 2, BIG_E, 2))
        out += [_edge(e) for e in EDGES]
        # document 0 holds one term of rule 0 (entry 0: t < need - 1), document 1 two, document 2 one: only 1 fires
        out.append(from_docs("neighbours", 2, [[1], [1, 2], [3], [1, 2, 3]], Rules([([1, 2, 3], [], 2)], 16)))
        # state 5 in FAN rules (each with a second term), state 9 in none
        fan = Rules([([5, 1 + k % 3], [], 1 + k % 2) for k in range(FAN)], 16)
        assert fan.degree()[5] == FAN and fan.degree()[9] == 0
        out.append(from_docs("fan3000", 2, [[5], [9], [5, 1], [5, 2, 9], [3, 9], [5, 1, 2, 3]], fan))
        out += [_empties(run) for run in EMPTY_RUNS]
        rng = _rng(6)
        every = Rules([([0, 1 + k % 15], [], 1) for k in range(40)], 16)
        out.append(from_docs("allfire", 2, [[0] + rng.integers(1, 16, 3).tolist() for _ in range(300)], every))
        out.append(from_docs("nothing", 2, [[int(s)] for s in rng.integers(0, 8, 300)],
                             Rules([([k % 8, 8 + k % 8], [], 2) for k in range(40)], 16)))
        out.append(Case("nodocs", 2, [0], [], every))
        out.append(Case("nopairs", 2, np.zeros(101, dtype=np.uint64), [], every))
        for nr in PASS_RULES:
            for nd in PASS_DOCS:
                rng = _rng(7, nr, nd)
                rules = random_rules(rng, nr, 16)
                rules.need[0] = 1                               # rule 0: any of its terms, none negated -- it fires somewhere
                rules.terms[: int(rules.rule_ptr[1])] &= np.uint32(NOT - 1)
                n_pairs = int(min(3000, max(8, PASS_E / float(rules.degree().mean()))))    # about PASS_E keys at the most
                out.append(Case(f"passes-r{nr}-d{nd}", 2, *random_matrix(rng, nd, n_pairs, 16), rules))
    _CASES[W] = {c.name: c for c in out}
    return _CASES[W]


def names(W):
    """The case names of a table without building a case (parametrize ids)."""
    out = [f"E{E}" for E in (SIZES if W == 2 else (0, 1025, 4097))] + ["random", "need", "negated"]
    if W == 2:
        out += ["big"] + [f"edge{e}" for e in EDGES] + ["neighbours", "fan3000"] + [f"empty{r}" for r in EMPTY_RUNS]
        out += ["allfire", "nothing", "nodocs", "nopairs"] + [f"passes-r{nr}-d{nd}" for nr in PASS_RULES for nd in PASS_DOCS]
    return out


def seeded(seed):
    """A small random case over 16 states (no table is built): for the references' own test."""
    rng = _rng(9, seed)
    rules = random_rules(rng, int(rng.integers(1, 40)), 16, lo=1, hi=int(rng.integers(2, 6)), negated=0.3)
    row, st = random_matrix(rng, int(rng.integers(1, 60)), int(rng.integers(1, 400)), 16)
    return Case(f"seed{seed}", 2, row, st, rules)
