"""Seeded random cases for the three passes that landed behind the late fuzz -- document scores (pfac_documents_scores,
pfac_selection_document_scores, pfac_documents_matching_scores), the rank (pfac_documents_top_scores) and the formatted
gather (pfac_documents_gather_format) -- and their composition behind a real scan and a real filter, shared by
tests/test_rankfuzz_cases.py (host only: pins the generator and asserts what the inputs reach),
tests/test_gpu_rank_fuzz.py and tools/fuzz.py rank.  Every expectation (`Expect`) comes from the CPU oracle's records
(nocaseref.expected for a folded table) with lengths from the pattern file's own lines, passed through wordref / spanref,
scoreref, llref, topref, gatherref and fmtref -- never from the device, PfacTable.final_lengths, state_weights or any
product function.

The document shapes are the generator's own: a document count from a ladder around the kernels' edges (one ballot of 64,
one group of 4 096, one workgroup of 16 384 documents of the compaction, a third workgroup), line lengths that keep the
input at or below about 300 KB, half the cases cut on the device, half with explicit offsets.  What a draw alone would
meet too rarely is planted: a dense document (more than 64 kept records from one tile), a document with kept records on
both sides of every 64-tile edge, a match in the first and in the last document."""
import functools
import os

import numpy as np

import scoreref
import spanref
import topref
import wordref
from fmtref import Fmt, format_ref
from gatherref import context_ids, gather_ref
from latefuzz import KNOBS, LETTERS, LINE_COUNTS, LateCase, _records, _same
from llref import greedy, line_lengths
from nocaseref import expected as folded_expected
from orc import Oracle
from passfuzz import GROUP, TILE, knob_label, record_width

TAG = 0x52414E4B                         # this generator's RNG stream: np.random.default_rng([seed, TAG])
KNOB_NAMES = sorted({k for d in KNOBS for k in d})
SEEDS = list(range(48))                  # the suite's cases: every knob set eight times
# the document ladder: one ballot less / more than one, about 1 000, a group and a bit, three groups and a bit, a
# workgroup and a bit, a third workgroup.  Slot (seed // 6 + 3 * (seed % 6)) % 8: every knob set meets every slot.
DOC_LADDER = (1, 63, 65, 1000, 4097, 3 * 4096 + 5, 16384 + 70, 40000)
MAX_BYTES = 300007                       # the late fuzz's largest input
FILTERS = ("none", "words", "spans")
CONTEXT = (0, 1, 2, 5, None)             # None: n_docs
DENSE_REPS = 150                         # planted matches of the dense document: a tile of it holds more than 64
MAX_GROUP_SEP = 8                        # PFAC_LINE_MAX_GROUP_SEP, written apart from the product's
U64_MAX = 2 ** 64 - 1
BY = ("score", "count")


def case_id(seed):
    return f"s{seed}-{knob_label(KNOBS[seed % len(KNOBS)])}"


def flags_of(by, lowest, ranked):
    return (topref.BY_COUNT if by == "count" else 0) | (topref.LOWEST if lowest else 0) | (topref.RANKED if ranked else 0)


class RankCase(LateCase):
    """`seed` alone fixes everything; `knobs` defaults to KNOBS[seed % len(KNOBS)].  (A LateCase for its methods --
    _plant, patterns_bytes, write_patterns, table -- with draws of its own.)"""

    def __init__(self, seed, knobs=None):              # noqa: super().__init__ is LateCase's generator, not this one's
        self.seed = seed
        self.knobs = KNOBS[seed % len(KNOBS)] if knobs is None else knobs
        rng = np.random.default_rng([seed, TAG])
        i, k = (seed // 6) % 8, seed % 6
        self.folded = (i + 2 * k) % 3 == 0
        self.filter = FILTERS[(i + k) % 3]
        self.small_weights = (2 * i + k) % 3 == 0
        self.lines_half = bool(rng.random() < 0.5)
        alpha = int(rng.choice([2, 3, 4, 8, 26, 60, 200]))
        if self.folded:                                         # letters in both cases, and a few bytes that do not fold
            pool = np.frombuffer(LETTERS + b"0_ .\xc1\xe1", dtype=np.uint8)
        else:
            pool = np.array([b for b in range(256) if b != 10], dtype=np.uint8)
        alpha = max(min(alpha, pool.size), 3)
        symbols = rng.permutation(pool)[:alpha]
        self.delim = (10, 0, int(symbols[0]))[int(rng.integers(0, 3))]
        self.delim_arg = self.delim
        if not self.lines_half and rng.random() < 1 / 8:
            self.delim_arg = None
        psym = symbols[symbols != self.delim]
        if self.folded:
            def fold(b):
                return b | 0x20 if 0x41 <= b <= 0x5A else b
            psym = psym[np.array([fold(int(b)) != fold(self.delim) for b in psym], dtype=bool)]
        self.alpha = alpha
        # a byte that is in no word and is not the delimiter: between the planted matches, so that each stands alone
        self.gap = next(b for b in (0x20, 0x2E, 0x2D, 0x01) if b != self.delim)
        # -- the pattern set (LateCase's shape; a few lines only on two ladder rows: 16-bit records) ------------
        n_lines = int(rng.choice([1, 3, 8, 16])) if i % 4 == 0 else int(rng.choice(LINE_COUNTS))
        maxlen = int(rng.choice([1, 2, 4, 8, 14])) if rng.random() < 0.85 else 40
        while sum(min(psym.size ** L, 1 << 20) for L in range(1, maxlen + 1)) < 2 * n_lines and maxlen < 40:
            maxlen += 1
        n_dup = int(rng.integers(1, 4)) if rng.random() < 0.3 and n_lines > 3 else 0
        pats = set()
        for _ in range(n_lines * 20):
            if len(pats) >= n_lines - n_dup:
                break
            pats.add(bytes(psym[rng.integers(0, psym.size, int(rng.integers(1, maxlen + 1)))]))
        plist = sorted(pats)
        lines = [plist[j] for j in rng.permutation(len(plist))]
        for _ in range(n_dup):
            lines.insert(int(rng.integers(0, len(lines) + 1)), lines[int(rng.integers(0, len(lines)))])
        self.lines = lines
        self.M = max(len(p) for p in lines)
        self.width = int(rng.choice([64, 256, 256, 1024]))
        n_ids = len(lines)
        # -- span rules (the filter "spans" reads them); the shortest pattern stays free: the plants use it -------
        self.free = min(plist, key=lambda p: (len(p), p))
        self.rules = [None] + [None if lines[j] == self.free else self._rule(rng) for j in range(n_ids)]
        # -- weights per pattern id ------------------------------------------------------------------------------
        self.weights = self._weights(rng, n_ids)
        # -- the documents and the input -------------------------------------------------------------------------
        target = DOC_LADDER[(i + 3 * k) % 8]
        if target == 1000:
            target += int(rng.integers(-30, 31))
        elif target == 40000:
            target += int(rng.integers(-500, 501))
        self.target = target
        self.psym, self.symbols = psym, symbols
        if self.lines_half:
            self._make_lines(rng, plist, target)
        else:
            self._make_offsets(rng, plist, target)
        assert self.off[0] == 0 and self.off[-1] == self.n_owned and self.off.size - 1 == target
        nd = target
        # -- the score rule, the top draws, the context window, the formats ----------------------------------
        self.score_rule = self._score_rule(rng)
        x = seed % 8
        self.tops = []
        for t in range(3):                                      # flags x, x + 3, x + 6 (mod 8): one of them is ranked
            f = (x + 3 * t) % 8
            rule = None if rng.random() < 0.3 else self._score_rule(rng)
            self.tops.append((self._k(rng, nd), BY[f & 1], bool(f & 2), bool(f & 4), rule))
        ctx = [CONTEXT[int(rng.integers(0, len(CONTEXT)))] for _ in range(2)]
        self.context = tuple(nd if v is None else v for v in ctx)
        self.fmts = [self._fmt(rng, nd, t) for t in range(2)]

    # -- draws ------------------------------------------------------------------------------
    def _weights(self, rng, n_ids):
        """[unused, w(1), ..., w(n_ids)] in the style of scoreref.weights_for: a zero, a cancelling pair, both int32
        extremes, small values otherwise; with `small_weights` nothing but small values (and the zero, the pair)."""
        w = [int(x) for x in rng.integers(-3, 6, n_ids)]
        must = [0, 2, -2] if self.small_weights else [0, 3, -3, -(2 ** 31), 2 ** 31 - 1]
        for j, v in zip(rng.permutation(n_ids).tolist(), must):
            w[j] = v
        return [0] + w

    def _score_rule(self, rng):
        kw = {}
        if rng.random() < 0.5:
            kw["min_count"] = int(rng.choice([1, 1, 2, 3]))
        if rng.random() < 0.25:
            kw["max_count"] = int(rng.choice([0, 1, 3, 10, 200]))
        if rng.random() < 0.3:
            kw["min_score"] = int(rng.choice([-3, -1, 0, 1, 2, -(2 ** 31)]))
        if rng.random() < 0.25:
            kw["max_score"] = int(rng.choice([-1, 0, 1, 5, 2 ** 31 - 1]))
        if rng.random() < 0.25:
            kw["density"] = (int(rng.integers(-3, 4)), int(rng.choice([1, 2, 7, 50, 1000])))
        if rng.random() < 0.25:
            kw["invert"] = True
        if rng.random() < 0.06:                                 # admits no document
            kw = dict(min_count=2 ** 63, max_count=2 ** 63 - 1)
        return kw

    @staticmethod
    def _k(rng, nd):
        """k: beyond every candidate count now and then, else from one of the ranges of n_top at which the sort changes
        shape (one wave, one block of 1 024, two blocks, more) that the document count leaves room for."""
        if rng.random() < 0.12:
            return U64_MAX if rng.random() < 0.5 else nd + int(rng.integers(1, 100))
        ranges = [(lo, min(hi, nd)) for lo, hi in ((0, 64), (65, 1024), (1025, 2048), (2049, nd)) if lo <= nd]
        lo, hi = ranges[int(rng.integers(0, len(ranges)))]
        return int(rng.integers(lo, hi + 1))

    def _fmt(self, rng, nd, t):
        """One Fmt draw: a flag subset (a label in most draws), bases that put a power of ten among the printed values,
        a group separator of 0 .. 8 bytes (never empty for the second draw: the context path's)."""
        r = rng.random()
        number, byte_offset = (r < 0.7), (0.45 <= r < 0.9)
        terminate = (None, self.delim, 10)[int(rng.integers(0, 3))]
        n_sep = int(rng.integers(1 if t else 0, MAX_GROUP_SEP + 1))
        sep = rng.integers(0, 256, n_sep).astype(np.uint8).tobytes()
        p = int(rng.choice([1, 2, 3, 4, 9, 17]))
        number_base = 10 ** p - int(rng.integers(0, nd + 1)) if 10 ** p > nd else int(rng.integers(0, 2))
        q = int(rng.choice([2, 4, 5, 9, 17]))
        offset_base = 10 ** q - int(rng.integers(0, self.n_owned + 1)) if 10 ** q > self.n_owned else 0
        two = rng.permutation(np.frombuffer(b":-=|#\x00\xff", dtype=np.uint8))[:2]
        seps = (b":", b"-") if rng.random() < 0.6 else (bytes([two[0]]), bytes([two[1]]))
        return Fmt(number=number, byte_offset=byte_offset, terminate=terminate, group_sep=sep, sep_first=bool(rng.random() < 0.4),
                   number_base=number_base, offset_base=offset_base, sep_match=seps[0], sep_context=seps[1])

    # -- the input --------------------------------------------------------------------------
    def _size(self, rng, nd):
        """The owned bytes to aim at: across a 64-tile edge in a third of the draws, else a few bytes to a few hundred
        per document, never above MAX_BYTES."""
        if rng.random() < 0.36:
            return int(rng.choice([GROUP + 6000, MAX_BYTES - 1500]))
        per = int(rng.choice([3, 7, 20, 90, 400, 3000]))
        return int(min(max(nd * per, 40), MAX_BYTES - 1500))

    def _fill(self, rng, plist, n, body):
        data = body[rng.integers(0, body.size, n)]
        if self.folded:
            low = (data >= 0x61) & (data <= 0x7A) & (rng.random(n) < 0.3)
            data[low] &= 0xDF
        for at in rng.integers(0, max(n - 1, 1), max(n // 50, 1)):
            self._plant(rng, data, int(at), plist[int(rng.integers(0, len(plist)))], n)
        return data

    def _plant_run(self, rng, a, e, reps):
        """`reps` copies of the free pattern, a gap byte behind each, from byte a on and never past e."""
        unit = len(self.free) + 1
        for r in range(reps):
            at = a + r * unit
            if at + unit > e:
                break
            self._plant(rng, self.data, at, self.free, e)
            self.data[at + unit - 1] = self.gap

    def _plant_special(self, rng, off, term, dense):
        """Behind the delimiters: the dense run in the bytes `dense` = (a, e); the free pattern on either side of every
        64-tile edge inside the document that lies across it; a match in the first and in the last document in most
        seeds."""
        nd, L = off.size - 1, len(self.free)
        if dense is not None:
            self._plant_run(rng, dense[0], dense[1], DENSE_REPS)
        for edge in range(GROUP, self.n_owned - L - 2, GROUP):
            d = int(np.searchsorted(off, edge, side="right")) - 1
            a, e = int(off[d]), int(off[d + 1]) - int(term[d])
            if a + L + 1 <= edge and edge + L + 1 <= e:
                self._plant_run(rng, edge - L - 1, edge, 1)
                self._plant_run(rng, edge, e, 1)
        for d in (0, nd - 1):
            a, e = int(off[d]), int(off[d + 1]) - int(term[d])
            if rng.random() < 0.7 and e - a >= L:
                self._plant(rng, self.data, a + int(rng.integers(0, e - a - L + 1)), self.free, e)

    def _make_lines(self, rng, plist, nd):
        """nd lines cut at the delimiter: empty lines among them, lines that are a pattern and no more, one dense line, a
        line across every 64-tile edge, the last line unterminated in half the seeds, a tail beyond n_owned in some."""
        unit = len(self.free) + 1
        want = self._size(rng, nd)
        mean = max(want / nd - 1, 0.6)
        hi = int(2 * mean) + 1
        if hi < 60 or rng.random() < 0.5:
            lens = rng.integers(0, hi + 1, nd)
        else:
            lens = np.minimum(rng.geometric(1 / (mean + 1), nd) - 1, 20000)
        lens = lens.astype(np.int64)
        lens[rng.random(nd) < 0.05] = 0
        as_pat = np.flatnonzero(rng.random(nd) < 0.1)
        pat_of = rng.integers(0, len(plist), as_pat.size)
        lens[as_pat] = [len(plist[j]) for j in pat_of]
        dense = int(rng.integers(0, nd)) if rng.random() < 0.75 else None
        if dense is not None:
            lens[dense] = DENSE_REPS * unit + int(rng.integers(0, 6))
        self.terminated = bool(rng.random() < 0.5)
        cut = 0 if self.terminated else 1

        def fix_last():
            if not self.terminated and lens[-1] == 0:
                lens[-1] = 1
        fix_last()
        while int(lens.sum()) + nd - cut > MAX_BYTES:           # (the drawn lengths overshoot: halve the longest lines)
            big = np.argsort(lens)[-max(nd // 10, 1):]
            lens[big[big != (-1 if dense is None else dense)]] //= 2
            fix_last()
        edge = GROUP
        while True:                                             # the line in front of every 64-tile edge runs across it
            start = np.concatenate(([0], np.cumsum(lens + 1)))
            if edge + unit + 4 >= int(start[nd]) - cut:
                break
            d = int(np.searchsorted(start, edge - unit - 2, side="right")) - 1
            if d != dense:
                lens[d] = max(int(lens[d]), edge - int(start[d]) + unit + 2 + int(rng.integers(0, 700)))
            edge += GROUP
        self.n_owned = int(start[nd]) - cut
        self.n = self.n_owned + (int(rng.integers(1, 5000)) if rng.random() < 0.4 else 0)
        self.data = self._fill(rng, plist, self.n, self.psym)
        off = start[:nd + 1].copy()
        off[-1] = self.n_owned
        for d, j in zip(as_pat.tolist(), pat_of.tolist()):
            if lens[d] == len(plist[j]):
                self._plant(rng, self.data, int(off[d]), plist[j], int(off[d]) + int(lens[d]))
        self.data[(off[1:] - 1)[:nd - cut]] = self.delim
        term = np.ones(nd, dtype=bool)
        term[-1] = self.terminated
        self._plant_special(rng, off, term, None if dense is None else (int(off[dense]), int(off[dense]) + int(lens[dense])))
        assert np.array_equal(spanref.split_offsets(self.data[:self.n_owned], self.delim), off)
        self.off = off.astype(np.uint64)

    def _make_offsets(self, rng, plist, nd):
        """nd documents by explicit offsets over the owned range: random cuts (empty documents where two coincide, and a
        few more on purpose), cuts around tile edges, one dense document, one document across every 64-tile edge, a
        delimiter at some documents' ends, a tail beyond n_owned in most seeds."""
        unit = len(self.free) + 1
        no = max(self._size(rng, nd), 1 if nd == 1 else 8)
        self.n_owned = no
        self.n = no if rng.random() < 0.4 else no + int(rng.integers(1, 5000))
        self.data = self._fill(rng, plist, self.n, self.symbols)
        cuts = rng.integers(0, no + 1, nd - 1).astype(np.int64)
        if cuts.size >= 12:
            for t in rng.integers(1, max(no // TILE, 1) + 1, 3):
                cuts[rng.integers(0, cuts.size, 3)] = np.clip([int(t) * TILE - 1, int(t) * TILE, int(t) * TILE + 1], 0, no)
            at = rng.integers(0, cuts.size, int(rng.integers(0, 5)))
            cuts[at] = cuts[(at + 1) % cuts.size]               # empty documents on purpose
        whole = []                                              # [a, b): one document each, where the cuts allow
        dense = None
        if rng.random() < 0.75 and no >= DENSE_REPS * unit + 8:
            a = int(rng.integers(0, no - DENSE_REPS * unit - 4))
            dense = (a, a + DENSE_REPS * unit + int(rng.integers(0, 5)))
            whole.append(dense)
        for edge in range(GROUP, no - unit - 2, GROUP):
            whole.append((edge - unit - 1 - int(rng.integers(0, 300)), min(edge + unit + 2 + int(rng.integers(0, 300)), no)))
        ends = [x for ab in whole for x in ab]
        for a, b in whole:
            inside = (cuts > a) & (cuts < b)
            cuts[inside] = a if rng.random() < 0.5 else b       # (empty documents in front of it or behind it)
        spare = np.flatnonzero(~np.isin(cuts, ends))
        if spare.size >= len(ends):
            cuts[spare[:len(ends)]] = ends
        off = np.concatenate(([0], np.sort(cuts), [no])).astype(np.int64)
        for _ in range(30 if nd > 1 else 0):                    # a document that is one pattern, where one fits exactly
            d = int(rng.integers(0, nd))
            fit = [p for p in plist if len(p) == off[d + 1] - off[d]]
            if fit:
                self._plant(rng, self.data, int(off[d]), fit[int(rng.integers(0, len(fit)))], int(off[d + 1]))
        term = (np.diff(off) > 0) & (rng.random(nd) < 0.5)
        self.data[off[1:][term] - 1] = self.delim
        self._plant_special(rng, off, term, None if dense is None else (dense[0], dense[1] - 1))
        self.terminated = bool(term[-1])
        self.off = off.astype(np.uint64)

    # -- the rest ----------------------------------------------------------------------------
    def describe(self):
        tops = "; ".join(f"k {k} by {by}{' lowest' if lo else ''}{' ranked' if rk else ''} rule {rule}" for k, by, lo, rk, rule in self.tops)
        return (f"RankCase({self.seed}) knobs {knob_label(self.knobs)} {'folded' if self.folded else 'exact'} alpha {self.alpha} "
                f"lines {len(self.lines)} M {self.M} width {self.width} n {self.n} n_owned {self.n_owned} "
                f"{'lines' if self.lines_half else 'offsets'} docs {self.off.size - 1} delimiter {self.delim} (passed {self.delim_arg}) "
                f"terminated {self.terminated} filter {self.filter} {'small' if self.small_weights else 'full'} weights "
                f"score rule {self.score_rule} tops [{tops}] context {self.context}")

    def fingerprint(self):
        """A hash of the patterns, the data, the offsets and every draw."""
        import hashlib
        h = hashlib.sha256()
        for part in (self.patterns_bytes(), self.data.tobytes(), self.off.tobytes(),
                     repr((self.n, self.n_owned, self.width, self.delim, self.delim_arg, self.terminated, self.filter, self.rules,
                           self.weights, self.score_rule, self.tops, self.context, [sorted(f.kwargs().items()) for f in self.fmts],
                           sorted(self.knobs.items()), self.folded, self.lines_half)).encode()):
            h.update(part)
        return h.hexdigest()[:16]


# ---------------------------------------------------------------------------
class TopWant:
    """What one top draw reports over scores `sc`: the candidates, the ranking, the ids, n_top and the winners' pairs."""

    def __init__(self, sc, off, draw):
        k, by, lowest, ranked, rule = draw
        self.flags = flags_of(by, lowest, ranked)
        self.kw = dict(k=k, by=by, lowest=lowest, ranked=ranked, **(rule or {}))
        self.cand = scoreref.predicate(sc, off, **rule) if rule is not None else np.arange(sc.size, dtype=np.uint64)
        self.rank = topref.ranking(sc, self.cand, self.flags)
        self.ids, self.n_top = topref.top(self.rank, k, self.flags)
        self.pairs = sc[self.ids.astype(np.int64)]


def with_context_sep(fmt):
    kw = fmt.kwargs()
    kw["context_sep"] = True
    return Fmt(**kw)


class Expect:
    """What the CPU says for a case, every step of run_rank_case (never reads the device)."""

    def __init__(self, case, path):
        c = case
        self.ll = line_lengths(path)
        if c.folded:
            pos, ids = folded_expected(c.patterns_bytes(), c.data, c.n_owned)
        else:
            o = Oracle(path, 1, 1)
            pos, ids = o.scan_spec(c.data, None)
            o.close()
            own = pos < c.n_owned
            pos, ids = pos[own], ids[own]
        self.pos, self.ids = pos.astype(np.int64), ids.astype(np.int64)
        self.lens = self.ll[self.ids]
        off = c.off.astype(np.int64)
        self.off, self.n_docs = off, off.size - 1
        if c.lines_half:
            self.split = spanref.split_offsets(c.data[:c.n_owned], c.delim)
        # the filter in front of the score pass
        if c.filter == "words":
            self.keep = wordref.filter_words(c.data, self.pos, self.lens, off=off)
        elif c.filter == "spans":
            dl = -1 if c.delim_arg is None else c.delim_arg
            self.keep = spanref.filter_spans(c.data, self.pos, self.lens, *spanref.record_spans(c.rules, self.ids), dl, off, c.n)
        else:
            self.keep = np.ones(self.pos.size, dtype=bool)
        kpos, kids, klens = self.pos[self.keep], self.ids[self.keep], self.lens[self.keep]
        self.kpos, self.kids, self.klens = kpos, kids, klens
        # scores, the rule, the gather
        self.by_id = scoreref.w_by_id(c.weights)
        self.sc = scoreref.scores_cut(kpos, kids, klens, off, self.by_id)
        self.totals = scoreref.totals(self.sc)
        self.rule_ids = scoreref.predicate(self.sc, off, **c.score_rule)
        self.gathered, self.gathered_off = gather_ref(c.data, off, self.rule_ids)
        # the rank, and the formatted gather of the first ranked draw
        self.tops = [TopWant(self.sc, off, d) for d in c.tops]
        self.ranked = next(j for j, d in enumerate(c.tops) if d[3])
        self.fmt_ranked = format_ref(c.data, off, self.tops[self.ranked].ids, c.fmts[0])
        # the context path
        self.doc_first = np.concatenate(([0], np.cumsum(self.sc["count"].astype(np.int64)))).astype(np.uint64)
        self.ctx_ids = context_ids(self.doc_first, *c.context)
        self.fmt_ctx = format_ref(c.data, off, self.ctx_ids, with_context_sep(c.fmts[1]), self.doc_first)
        # the selection path.  The records that end inside their document, greedily from 0 in ONE walk: a pick ends at or
        # before its document's end and the next document's records start there or later, so the cursor never reaches
        # into a later document -- the walk is llref.greedy per document, back to back (test_rankfuzz_cases.py holds it
        # against the per-document loop).
        doc = np.minimum(np.searchsorted(off, kpos, side="right") - 1, self.n_docs - 1)
        fits = kpos + klens <= off[doc + 1]
        self.kdoc, self.fits = doc, fits
        pick, ex = greedy(kpos[fits], klens[fits], 0, c.n_owned)
        assert ex == 0
        self.sel_pos, self.sel_ids, self.sel_doc = kpos[fits][pick], kids[fits][pick], doc[fits][pick]
        self.sel_first = np.concatenate(([0], np.cumsum(np.bincount(self.sel_doc, minlength=self.n_docs)))).astype(np.uint64)
        self.sel_sc = scoreref.scores_of_selection(self.sel_first, self.sel_ids, self.by_id)
        self.sel_totals = scoreref.totals(self.sel_sc)
        self.sel_top = TopWant(self.sel_sc, off, c.tops[0])


@functools.lru_cache(maxsize=None)
def expectation(seed, tmp_dir):
    """(case, Expect) of a suite seed, made once per process."""
    c = RankCase(seed)
    return c, Expect(c, c.write_patterns(os.path.join(tmp_dir, f"rank_{seed}.pat")))


# ---------------------------------------------------------------------------
def run_rank_case(g_factory, case, tmp_dir, want=None, g=None, before_weights=None):
    """One case on the GPU, one context: scan, offsets, the drawn filter, the scores (twice), the score rule and the
    gather, three top draws (the first ranked one into the formatted gather), the context path (segment, matching
    documents with context, the formatted gather under context_sep), the selection's scores and their rank; for
    seed % 4 == 3 the scores and the rank again into the caller's buffers -- each step bit for bit against `Expect`.
    `g`: a live context to run on instead of a fresh one (it is left open); `before_weights(g, n_docs)` runs behind the
    filter, in front of set_pattern_weights: the one thing the score pass then lacks is the uploaded table's weights.  Returns (records, document entries, bytes) compared."""
    c = case
    path = c.write_patterns(os.path.join(tmp_dir, f"rank_{c.seed}.pat"))
    w = Expect(c, path) if want is None else want
    try:
        if g is not None:
            return _run(g, c, path, w, before_weights)
        with g_factory() as own:
            return _run(own, c, path, w, before_weights)
    except AssertionError as e:
        raise AssertionError(f"{c.describe()}: {e}") from e


def _pairs(got, want, what):
    _same(got["score"], want["score"], f"{what}: scores")
    _same(got["count"], want["count"], f"{what}: counts")


def _top(g, nd, tw, what, **buffers):
    n_top = g.top_documents(nd, **tw.kw, **buffers)
    assert n_top == tw.n_top, f"{what}: n_top {n_top}, want {tw.n_top} of {tw.cand.size} candidates"
    return n_top


def _formatted(g, c, nd, n_ids, fmt, want, what, **more):
    ob = g.gather_documents_formatted(nd, n_ids, c.n, **fmt.kwargs(), **more)
    assert ob == want[0].size, f"{what}: {ob} bytes out, want {want[0].size}"
    _same(g.gathered_offsets_to_host(n_ids), want[1], f"{what}: offsets")
    _same(g.gathered_to_host(ob), want[0], f"{what}: bytes")
    return ob


def _run(g, c, path, w, before_weights):
    table = c.table(path)
    assert table.max_pat_len == c.M
    nd = w.n_docs
    n_rec = n_doc = n_bytes = 0
    g.load_table(table)
    g.set_final_lengths(table.final_lengths())
    if c.filter == "spans":
        g.set_pattern_spans(c.rules)
    g.reserve(0, max(c.n, 1), max(c.n // 8, 4096))
    g.h2d(c.data)
    # 1 scan
    total = g.scan_resident(c.n_owned, c.n)
    assert total == w.pos.size, f"step 1, scan: {total} records, want {w.pos.size}"
    _records(table, g.records_to_host(total), w.pos, w.ids, "step 1, scan")
    fmt = g.scan_format()
    assert fmt[0] == record_width(table.num_final, c.knobs), f"step 1: record width {fmt[0]}"
    n_rec += total
    # 2 offsets
    if c.lines_half:
        got_docs, _ = g.split_documents(c.n_owned, c.delim)
        assert got_docs == w.split.size - 1, f"step 2, split: {got_docs} documents, want {w.split.size - 1}"
        _same(g.doc_offsets_to_host(got_docs).astype(np.int64), w.split, "step 2, split offsets")
        _same(w.split, w.off, "step 2, the case's offsets")
        n_doc += got_docs
    else:
        g.set_doc_offsets(c.off)
    # 3 the drawn filter
    if c.filter == "words":
        n = g.filter_whole_words(n_docs=nd)
    elif c.filter == "spans":
        n = g.filter_spans(delimiter=c.delim_arg, n_docs=nd)
    else:
        n = total
    assert n == w.kpos.size, f"step 3, filter {c.filter}: {n} records kept, want {w.kpos.size} of {w.pos.size}"
    assert g.last_count() == n and g.scan_format() == fmt, f"step 3, filter {c.filter}: count or format"
    _records(table, g.records_to_host(n), w.kpos, w.kids, f"step 3, filter {c.filter}")
    n_rec += n
    # 4 weights, scores twice
    if before_weights is not None:
        before_weights(g, nd)
    g.set_pattern_weights(c.weights)
    for turn in (1, 2):
        tot = g.document_scores(nd)
        assert tot == w.totals, f"step 4, document_scores (call {turn}): totals {tot}, want {w.totals}"
        _pairs(g.document_scores_to_host(nd), w.sc, f"step 4, document_scores (call {turn})")
        n_doc += nd
    # 5 the score rule and the gather
    n_ids = g.matching_documents_scored(nd, **c.score_rule)
    _same(g.matching_documents_to_host(n_ids), w.rule_ids, "step 5, matching_documents_scored")
    ob = g.gather_documents(nd, n_ids, c.n)
    _same(g.gathered_offsets_to_host(n_ids), w.gathered_off, "step 5, gather: offsets")
    _same(g.gathered_to_host(ob), w.gathered, "step 5, gather: bytes")
    n_doc += n_ids
    n_bytes += ob
    # 6 the top draws
    for j, tw in enumerate(w.tops):
        what = f"step 6, top draw {j} ({tw.kw})"
        n_top = _top(g, nd, tw, what)
        _same(g.matching_documents_to_host(n_top), tw.ids, f"{what}: ids")
        _pairs(g.top_scores_to_host(n_top), tw.pairs, what)
        n_doc += 2 * n_top
        if j == w.ranked:
            n_bytes += _formatted(g, c, nd, n_top, c.fmts[0], w.fmt_ranked, f"step 6, formatted gather of top draw {j}")
    # 7 the context path
    kept = g.segment_records(nd)
    first, _ = g.segment_to_host(kept, nd)
    _same(first, w.doc_first, "step 7, segment_records: doc_first")
    _same(np.diff(first.astype(np.int64)), w.sc["count"].astype(np.int64), "step 7, segment_records: records per document")
    before, after = c.context
    n_ctx = g.matching_documents(nd, before=before, after=after)
    _same(g.matching_documents_to_host(n_ctx), w.ctx_ids, f"step 7, matching_documents before={before} after={after}")
    n_bytes += _formatted(g, c, nd, n_ctx, with_context_sep(c.fmts[1]), w.fmt_ctx, "step 7, formatted gather with context")
    assert g.last_count() == n and g.scan_format() == fmt, "step 7: the heap's count or format changed"
    _records(table, g.records_to_host(n), w.kpos, w.kids, "step 7, the heap behind the context path")
    n_doc += nd + 1 + n_ctx
    n_rec += n
    # 8 the selection path
    n_sel = g.select_leftmost_longest_documents(nd)
    sfirst, sel = g.doc_selection_to_host(n_sel, nd)
    _same(sfirst, w.sel_first, "step 8, per-document selection: doc_first")
    _records(table, sel, w.sel_pos, w.sel_ids, "step 8, per-document selection")
    tot = g.selection_document_scores(nd)
    assert tot == w.sel_totals, f"step 8, selection_document_scores: totals {tot}, want {w.sel_totals}"
    _pairs(g.document_scores_to_host(nd), w.sel_sc, "step 8, selection_document_scores")
    tw = w.sel_top
    n_top = _top(g, nd, tw, f"step 8, top over the selection's scores ({tw.kw})")
    _same(g.matching_documents_to_host(n_top), tw.ids, "step 8, top over the selection's scores: ids")
    _pairs(g.top_scores_to_host(n_top), tw.pairs, "step 8, top over the selection's scores")
    n_rec += n_sel
    n_doc += nd + 2 * n_top
    # 9 steps 4 and 6 into the caller's buffers
    if c.seed % 4 == 3:
        import torch
        d_sc = torch.empty(nd * 16, dtype=torch.uint8, device="cuda:0")
        tot = g.document_scores(nd, d_out=d_sc)
        torch.cuda.synchronize()
        assert tot == w.totals, f"step 9, document_scores into d_out: totals {tot}, want {w.totals}"
        _pairs(d_sc.cpu().numpy().view(scoreref.SCORE), w.sc, "step 9, document_scores into d_out")
        n_doc += nd
        for j, tw in enumerate(w.tops):
            what = f"step 9, top draw {j} into the caller's buffers ({tw.kw})"
            if tw.n_top == 0:
                _top(g, nd, tw, what, d_scores=d_sc)
                continue
            d_ids = torch.empty(tw.n_top * 8, dtype=torch.uint8, device="cuda:0")
            d_prs = torch.empty(tw.n_top * 16, dtype=torch.uint8, device="cuda:0")
            _top(g, nd, tw, what, d_scores=d_sc, d_out=d_ids, d_top_scores=d_prs, out_cap=tw.n_top)
            torch.cuda.synchronize()
            _same(d_ids.cpu().numpy().view(np.uint64), tw.ids, f"{what}: ids")
            _pairs(d_prs.cpu().numpy().view(scoreref.SCORE), tw.pairs, what)
            n_doc += 2 * tw.n_top
            if j == w.ranked:
                n_bytes += _formatted(g, c, nd, tw.n_top, c.fmts[0], w.fmt_ranked, f"step 9, formatted gather of top draw {j}", d_ids=d_ids)
    return n_rec, n_doc, n_bytes
