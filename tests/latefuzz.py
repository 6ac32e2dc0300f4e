"""Seeded random cases for the four passes behind the scan that the older fuzzers do not reach -- the span filter, the
group masks, replacement templates and match extraction -- and their composition, shared by
tests/test_latefuzz_cases.py (host only: pins the generator), tests/test_gpu_late_fuzz.py and tools/fuzz.py late.
Every expectation (`Expect`) comes from the CPU oracle's records (nocaseref.expected for a folded table) with lengths
from the pattern file's own lines, passed through spanref, groupref, llref, tplref, replref and gatherref -- never from
the device, PfacTable.final_lengths, state_spans or template_table.  The module also holds the directed inputs of the
GPU file: the template piece ladder and the broken document offsets."""
import functools
import os

import numpy as np

import groupref
import spanref
import tplref
from docref import random_offsets
from gatherref import gather_ref
from llref import greedy, line_lengths
from nocaseref import expected as folded_expected
from orc import Oracle
from passfuzz import GROUP, TILE, knob_label, record_width
from replref import rep_table, splice

KNOBS = [{}, {"PFAC_WIDE": "1"}, {"PFAC_REC_BYTES": "4"}, {"PFAC_FORCE_L2": "1"}, {"PFAC_DENSE": "1"},
         {"PFAC_FORCE_L2": "1", "PFAC_DENSE": "1"}]
KNOB_NAMES = sorted({k for d in KNOBS for k in d})
SEEDS = list(range(48))                  # the suite's cases: every knob set eight times
LINE_COUNTS = [1, 3, 16, 17, 60, 64, 65, 300, 1500]
SIZES = [1, 17, 4095, 4097, 12289, 70001, GROUP - 1, GROUP + 1, 300007]
SIZE_P = [.03, .03, .08, .1, .14, .16, .1, .1, .26]
N_GROUPS = [1, 2, 7, 63, 64]
RULES = [None, "^", "$", "^$"]
WIN = 1024                               # output bytes per window of the shared writer, four windows per workgroup
LETTERS = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def case_id(seed):
    return f"s{seed}-{knob_label(KNOBS[seed % len(KNOBS)])}"


class LateCase:
    """`seed` alone fixes everything; `knobs` defaults to KNOBS[seed % len(KNOBS)]."""

    def __init__(self, seed, knobs=None):
        self.seed = seed
        self.knobs = KNOBS[seed % len(KNOBS)] if knobs is None else knobs
        rng = np.random.default_rng([seed, 0x4C415445])
        self.folded = bool(rng.random() < 1 / 3)
        self.lines_half = bool(rng.random() < 0.5)
        alpha = int(rng.choice([2, 3, 4, 8, 26, 60, 200]))       # (passfuzz's alphabets)
        if self.folded:                                         # letters in both cases, and a few bytes that do not fold
            pool = np.frombuffer(LETTERS + b"0_ .\xc1\xe1", dtype=np.uint8)
        else:
            pool = np.array([b for b in range(256) if b != 10], dtype=np.uint8)
        alpha = max(min(alpha, pool.size), 3)
        symbols = rng.permutation(pool)[:alpha]
        dk = int(rng.integers(0, 3))
        self.delim = (10, 0, int(symbols[0]))[dk]
        self.delim_arg = self.delim                            # what filter_spans is given (None: no delimiter)
        if not self.lines_half and rng.random() < 1 / 8:
            self.delim_arg = None
        psym = symbols[symbols != self.delim]                   # no pattern holds the delimiter (nor byte 10)
        if self.folded:                                         # ... in either case: the scan would fold it
            def fold(b):
                return b | 0x20 if 0x41 <= b <= 0x5A else b
            psym = psym[np.array([fold(int(b)) != fold(self.delim) for b in psym], dtype=bool)]
        self.alpha = alpha
        # -- the pattern set ----------------------------------------------------------------
        n_lines = int(rng.choice(LINE_COUNTS))
        maxlen = int(rng.choice([1, 2, 4, 8, 14])) if rng.random() < 0.85 else 40
        while sum(min(psym.size ** L, 1 << 20) for L in range(1, maxlen + 1)) < 2 * n_lines and maxlen < 40:
            maxlen += 1
        n_dup = int(rng.integers(1, 4)) if rng.random() < 0.3 and n_lines > 3 else 0
        pats = set()
        for _ in range(n_lines * 20):
            if len(pats) >= n_lines - n_dup:
                break
            pats.add(bytes(psym[rng.integers(0, psym.size, int(rng.integers(1, maxlen + 1)))]))
        plist = sorted(pats)                                    # (never the set's own order: bytes hash differently per process)
        lines = [plist[i] for i in rng.permutation(len(plist))]
        for _ in range(n_dup):                                  # duplicate lines: unreachable final states
            lines.insert(int(rng.integers(0, len(lines) + 1)), lines[int(rng.integers(0, len(lines)))])
        self.lines = lines
        self.M = max(len(p) for p in lines)
        self.width = int(rng.choice([64, 256, 256, 1024]))
        n_ids = len(lines)
        # -- rules, groups, templates, replacements: one per pattern id ----------------------
        self.line_match = bool(rng.random() < 1 / 6)
        self.rules = [None] + [self._rule(rng) for _ in range(n_ids)]
        self.n_groups = int(rng.choice(N_GROUPS))
        self.ready_masks = seed % 8 == 5
        groups = [None]
        for _ in range(n_ids):
            r = rng.random()
            if r < 0.15:
                groups.append(None)
            elif r < 0.8:
                groups.append(int(rng.integers(0, self.n_groups)))
            else:
                groups.append(tuple(int(x) for x in rng.integers(0, self.n_groups, int(rng.integers(2, 5)))))
        self.group_masks = groupref.masks_by_id(groups)         # uint64 per id, made by the checker's own function
        if self.ready_masks:                                    # ready masks, bit 63 set on every other grouped id
            self.group_masks[1::2] |= np.where(self.group_masks[1::2] != 0, np.uint64(1) << np.uint64(63), np.uint64(0))
            self.groups = self.group_masks.copy()
        else:
            self.groups = groups
        used = [g for g in range(64) if int(np.bitwise_or.reduce(self.group_masks)) >> g & 1]

        def some(k):
            return sum({1 << int(g) for g in rng.choice(used, min(k, len(used)), replace=False)}) if used and k else 0
        self.predicate = dict(all_of=some(int(rng.integers(0, 3))), any_of=some(int(rng.integers(0, 4))),
                              none_of=some(int(rng.integers(0, 2))), invert=bool(rng.random() < 0.3))
        self.templates = {}
        for i in range(1, n_ids + 1):
            def part():
                return b"" if rng.random() < 0.25 else rng.integers(0, 256, int(rng.integers(1, 41))).astype(np.uint8).tobytes()
            if rng.random() < 0.4:
                self.templates[i] = part()
            else:
                self.templates[i] = (part(), part())
                if rng.random() < 0.01 and alpha >= 8 and len(lines[i - 1]) >= 3:      # longer than an output window
                    self.templates[i] = (rng.integers(0, 256, int(rng.integers(1000, 5001))).astype(np.uint8).tobytes(),
                                         self.templates[i][1])
        self.reps = {}                                          # (passfuzz.Case.replacements' lengths)
        for i in range(1, n_ids + 1):
            L = int(rng.integers(1000, 5001)) if rng.random() < 0.01 and alpha >= 8 else int(rng.integers(0, 65))
            self.reps[i] = rng.integers(0, 256, L).astype(np.uint8).tobytes()
        # -- the input --------------------------------------------------------------------
        n = int(rng.choice(SIZES, p=SIZE_P))
        self.n = n
        self.n_owned = n if rng.random() < 0.6 else int(rng.integers(1, n + 1))
        self.entry = int(rng.integers(0, self.M + 1))
        body = psym if self.lines_half else symbols             # (explicit offsets: the delimiter may be an input byte)
        data = body[rng.integers(0, body.size, n)]
        if self.folded:                                         # mixed case whatever the alphabet drew
            low = (data >= 0x61) & (data <= 0x7A) & (rng.random(n) < 0.3)
            data[low] &= 0xDF
        for at in rng.integers(0, max(n - 1, 1), max(n // 50, 1)):          # planted as passfuzz plants them
            self._plant(rng, data, int(at), plist[int(rng.integers(0, len(plist)))], n)
        self.data = data
        if self.lines_half:
            self._cut_lines(rng, plist)
        else:
            self._cut_offsets(rng, plist)
        assert self.off[0] == 0 and self.off[-1] == self.n_owned

    # -- draws ------------------------------------------------------------------------------
    @staticmethod
    def _rule(rng):
        r = rng.random()
        if r < 0.65:
            return RULES[int(rng.choice(4, p=[.45, .2, .2, .15]))]
        lo = int(rng.integers(0, 41))
        hi = None if rng.random() < 0.4 else lo + int(rng.integers(0, 41))
        tail = None if rng.random() < 0.5 else int(rng.integers(0, 41))
        if rng.random() < 0.06:
            hi = lo - 1                                         # admits nothing
        return (lo, hi, tail)

    def _plant(self, rng, data, at, pat, limit):
        pt = np.frombuffer(pat, dtype=np.uint8).copy()
        if self.folded:                                         # in the other case here and there
            up = (pt >= 0x61) & (pt <= 0x7A) & (rng.random(pt.size) < 0.4)
            pt[up] &= 0xDF
        m = min(pt.size, limit - at)
        if m > 0 and at >= 0:
            data[at:at + m] = pt[:m]

    def _by_rule(self, plist):
        """Patterns whose rule judges the start / the tail (what a plant at a document's start / end is for)."""
        idx = {p: i for i, p in enumerate(self.lines, 1)}       # (the last of equal lines wins)
        def judged(p, k):
            r = spanref.rule_bounds(self.rules[idx[p]])
            return r[1] < spanref.INF if k == 0 else r[2] != spanref.ANY
        heads = [p for p in plist if judged(p, 0)] or plist
        tails = [p for p in plist if judged(p, 1)] or plist
        return heads, tails

    def _plant_edges(self, rng, plist, off, term, across):
        """Patterns at the first byte of a document, ending at its last byte in front of its delimiter, as the whole
        document, and (`across`) over a document's end."""
        data, no = self.data, self.n_owned
        heads, tails = self._by_rule(plist)
        n_docs = off.size - 1
        for d in rng.permutation(n_docs)[:max(min(n_docs // 2, 4000), min(n_docs, 8))]:
            a, b = int(off[d]), int(off[d + 1])
            e = b - 1 if term[d] else b                         # where `$` sits
            kind = int(rng.integers(0, 4))
            p = (heads, tails, plist, plist)[kind][int(rng.integers(0, 1 << 30)) % len((heads, tails, plist, plist)[kind])]
            if kind == 0 and a + len(p) <= e:
                self._plant(rng, data, a, p, e)
            elif kind == 1 and e - len(p) >= a:
                self._plant(rng, data, e - len(p), p, e)
            elif kind == 3 and across and len(p) > 1 and b < self.n and b - 1 >= a:
                self._plant(rng, data, b - int(rng.integers(1, len(p))), p, self.n)

    def _straddlers(self, rng):
        """[(k, a, b)]: a document [k - a, k + b) across every multiple k of 64 tiles inside the owned range, short in
        half the draws (so that rules with a bounded start still admit records on the far side)."""
        out = []
        for k in range(GROUP, self.n_owned - 1500, GROUP):
            far = 40 if rng.random() < 0.5 else 700
            out.append((k, int(rng.integers(3, far + 1)), int(rng.integers(4, far + 1))))
        return out

    def _plant_straddlers(self, rng, plist, straddlers, off, term):
        """A grouped pattern that its rule admits on either side of the 64-tile edge inside a straddling document."""
        idx = {p: i for i, p in enumerate(self.lines, 1)}
        grouped = [p for p in plist if self.group_masks[idx[p]] != 0]
        for k, a, b in straddlers:
            d = int(np.searchsorted(off, k, side="right")) - 1
            s, e = int(off[d]), int(off[d + 1]) - int(term[d])
            assert s == k - a and int(off[d + 1]) == k + b
            left = [p for p in grouped if len(p) <= a and self._admits(idx[p], 0, e - s - len(p))]
            right = [p for p in grouped if len(p) <= e - k and self._admits(idx[p], e - len(p) - s, 0)]
            if left:
                p = left[int(rng.integers(0, len(left)))]
                self._plant(rng, self.data, s, p, k)
                # a group behind the edge that the bytes in front of it do not carry, where the set has one: the wave
                # behind the edge must add it to the mask that the wave in front of it writes
                right = [q for q in right if self.group_masks[idx[q]] & ~self.group_masks[idx[p]]] or right
            if right:
                p = right[int(rng.integers(0, len(right)))]
                self._plant(rng, self.data, e - len(p), p, e)

    def _admits(self, pid, rel, tail):
        if self.line_match:
            return rel == 0 and tail == 0
        lo, hi, mt = spanref.rule_bounds(self.rules[pid])
        return lo <= rel <= hi and (mt == spanref.ANY or tail <= mt)

    def _cut_lines(self, rng, plist):
        """Lines of the owned range: delimiters written into the input, runs of them, lines that are a pattern and no
        more, a line across every multiple of 64 tiles, the last line unterminated in half the seeds."""
        data, no, dl = self.data, self.n_owned, self.delim
        mode = int(rng.integers(0, 3))                          # mostly short, mid, long lines
        ends, at = [], 0
        while at < no:
            r = rng.random()
            if r < 0.06:
                for _ in range(int(rng.integers(1, 6))):        # a run of delimiters
                    ends.append(at)
                    at += 1
                continue
            if r < 0.2:
                p = plist[int(rng.integers(0, len(plist)))]     # the line is a pattern
                self._plant(rng, data, at, p, self.n)
                L = len(p)
            elif r < 0.2 + (0.001, 0.01, 0.03)[mode]:
                L = int(rng.integers(1000, 20000))
            else:
                L = int(rng.integers(1, (12, 120, 1500)[mode]))
            at += L
            ends.append(at)
            at += 1
        ends = np.array([e for e in ends if e < no], dtype=np.int64)
        strad = self._straddlers(rng)
        for k, a, b in strad:                                   # one line across every 64-tile edge
            ends = np.append(ends[(ends < k - 700) | (ends >= k + 700)], [k - a - 1, k + b - 1])
        ends = np.unique(ends)
        self.terminated = bool(rng.random() < 0.5)
        ends = ends[ends < no - 1]
        data[ends] = dl
        if self.terminated:
            data[no - 1] = dl
        elif data[no - 1] == dl:
            data[no - 1] = plist[0][0]
        off = spanref.split_offsets(data[:no], dl)              # (the generator's own view; the device's is checked against
        term = data[np.maximum(off[1:] - 1, 0)] == dl           # the same function over the final bytes in Expect)
        self._plant_edges(rng, plist, off, term, across=False)
        self._plant_straddlers(rng, plist, strad, off, term)
        assert np.array_equal(spanref.split_offsets(data[:no], dl), off)
        self.off = off.astype(np.uint64)

    def _cut_offsets(self, rng, plist):
        """Explicit offsets over the owned range (docref.random_offsets, cuts around tile edges, a run of 70 to 200 cuts
        inside one tile in 40 % of the seeds, documents that are one pattern), a delimiter at some documents' ends."""
        data, no, dl = self.data, self.n_owned, self.delim
        off = random_offsets(rng, no, int(rng.integers(1, 400)), empties=int(rng.integers(0, 5)))
        extra = []
        for k in rng.integers(1, max(no // TILE, 1) + 1, 3):
            extra += [int(k) * TILE - 1, int(k) * TILE, int(k) * TILE + 1]
        if rng.random() < 0.4:                                  # more than 63 documents in one tile: the searched path
            c = int(rng.integers(0, max(no // TILE, 1))) * TILE
            for _ in range(int(rng.integers(70, 200))):
                c += int(rng.integers(0, 30))
                extra.append(c)
        for _ in range(30):                                     # a document that is one pattern (and its delimiter)
            p = plist[int(rng.integers(0, len(plist)))]
            a = int(rng.integers(0, max(no - len(p) - 1, 1)))
            if a + len(p) + 1 <= no:
                self._plant(rng, data, a, p, no)
                extra += [a, a + len(p) + int(rng.integers(0, 2))]
        off = np.sort(np.concatenate([off.astype(np.int64), np.array([c for c in extra if 0 <= c <= no], dtype=np.int64)]))
        strad = self._straddlers(rng)
        for k, a, b in strad:                                   # one document across every 64-tile edge
            off = np.sort(np.append(off[(off < k - 700) | (off >= k + 700)], [k - a, k + b]))
        term = np.zeros(off.size - 1, dtype=bool)
        some = (np.diff(off) > 0) & (rng.random(off.size - 1) < 0.5)
        term[some] = True
        self._plant_edges(rng, plist, off, term, across=True)
        self._plant_straddlers(rng, plist, strad, off, term)
        data[off[1:][term] - 1] = dl                            # (behind the plants: `$` sits in front of these)
        self.terminated = bool(term[-1]) if term.size else False
        self.off = off.astype(np.uint64)

    # -- the rest ----------------------------------------------------------------------------
    def patterns_bytes(self):
        return b"".join(p + b"\n" for p in self.lines)

    def describe(self):
        return (f"LateCase({self.seed}) knobs {knob_label(self.knobs)} {'folded' if self.folded else 'exact'} alpha {self.alpha} "
                f"lines {len(self.lines)} M {self.M} width {self.width} n {self.n} n_owned {self.n_owned} entry {self.entry} "
                f"{'lines' if self.lines_half else 'offsets'} docs {self.off.size - 1} delimiter {self.delim} (passed {self.delim_arg}) "
                f"terminated {self.terminated} line_match {self.line_match} n_groups {self.n_groups} "
                f"ready_masks {self.ready_masks} predicate {self.predicate}")

    def write_patterns(self, path):
        with open(path, "wb") as f:
            f.write(self.patterns_bytes())
        return path

    def table(self, path):
        from phfpfac_amd import PfacTable
        if self.folded:
            return PfacTable.from_bytes(self.patterns_bytes(), self.width, ignore_case=True)
        return PfacTable.from_file(path, self.width)


# ---------------------------------------------------------------------------
# piece boundaries of the shared writer's outputs, from the picks and the templates alone

def template_parts(templates, ids):
    """(prefix length, suffix length, quoting) per pick; a plain template counts as a prefix of all its bytes."""
    tpl = tplref.by_id(templates)
    pre = np.array([len(tpl[i]) if isinstance(tpl[i], bytes) else len(tpl[i][0]) for i in ids], dtype=np.int64)
    suf = np.array([0 if isinstance(tpl[i], bytes) else len(tpl[i][1]) for i in ids], dtype=np.int64)
    quoting = np.array([not isinstance(tpl[i], bytes) for i in ids], dtype=bool)
    return pre, suf, quoting


def pick_layout(pos, lens, ids, templates, entry, n_owned, extract=False):
    """Per pick: (o, E, pre, suf, quoting, gap, after) -- the output offset o at which the rewritten pick begins, its
    length E, its template's parts, the gap bytes in front of it and the bytes of the piece that follows it (the next
    gap or the tail; the extraction: the next pick)."""
    pos, lens = np.asarray(pos, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    pre, suf, quoting = template_parts(templates, np.asarray(ids).tolist())
    E = pre + suf + np.where(quoting, lens, 0)
    ends = pos + lens
    prev = np.concatenate(([int(entry)], ends[:-1])) if pos.size else pos
    gap = np.zeros_like(pos) if extract else pos - prev
    o = np.cumsum(gap + E) - E
    if extract:
        after = np.append(E[1:], 0)[:pos.size]                  # the next pick's bytes follow at once
    else:
        after = np.append(gap[1:], max(int(n_owned) - int(ends[-1]), 0) if pos.size else 0)[:pos.size]
    return o, E, pre, suf, quoting, gap, after


def piece_boundaries(pos, lens, ids, templates, entry, n_owned, extract=False):
    """The output offsets at which one piece of the writer ends and the next, non-empty one begins: a list of four int64
    arrays -- gap -> prefix (or a plain replacement), prefix -> match, match -> suffix, suffix (or a plain replacement)
    -> gap; the extraction has no gaps, its last kind is suffix -> the next pick.  Only boundaries between two
    non-empty pieces count."""
    o, E, pre, suf, quoting, gap, after = pick_layout(pos, lens, ids, templates, entry, n_owned, extract)
    lens = np.asarray(lens, dtype=np.int64)
    first_piece = np.where(pre > 0, pre, np.where(quoting, lens, 0))           # the first non-empty piece of E exists iff E > 0
    last_piece = np.where(suf > 0, suf, np.where(quoting, lens, pre))
    return [o[(gap > 0) & (first_piece > 0)], (o + pre)[quoting & (pre > 0)], (o + pre + lens)[quoting & (suf > 0)],
            (o + E)[(last_piece > 0) & (E > 0) & (after > 0)]]


# ---------------------------------------------------------------------------
class Expect:
    """What the CPU says for a case, every step of run_late_case (never reads the device)."""

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
        dl = -1 if c.delim_arg is None else c.delim_arg
        spans = spanref.line_spans(pos.size) if c.line_match else spanref.record_spans(c.rules, self.ids)
        self.spans = spans
        self.keep = spanref.filter_spans(c.data, self.pos, self.lens, *spans, dl, off, c.n)
        self.keep_nodocs = spanref.filter_spans(c.data, self.pos, self.lens, *spans, dl, None, c.n) if c.n_owned == c.n else None
        kpos, kids, klens = self.pos[self.keep], self.ids[self.keep], self.lens[self.keep]
        self.kpos, self.kids, self.klens = kpos, kids, klens
        # groups
        self.masks = groupref.masks_cut(kpos, kids, klens, off, c.group_masks)
        self.any_mask = int(np.bitwise_or.reduce(self.masks)) if self.masks.size else 0
        self.match_ids = groupref.predicate(self.masks, **c.predicate)
        if c.lines_half:
            self.gathered, self.gathered_off = gather_ref(c.data, off, self.match_ids)
        # per-document selection, templated replace and extraction
        doc = np.searchsorted(off, kpos, side="right") - 1
        self.kdoc = doc
        fits = kpos + klens <= off[np.minimum(doc + 1, self.n_docs)]
        fp, fl, fi, fd = kpos[fits], klens[fits], kids[fits], doc[fits]
        cut = np.searchsorted(fd, np.arange(self.n_docs + 1), side="left")
        raw = bytes(c.data)
        dpos, dids, dlens, outs, exts, poff = [], [], [], [], [], [np.zeros(1, dtype=np.uint64)]
        picks_per_doc = np.zeros(self.n_docs, dtype=np.int64)
        out_len = np.diff(off).copy()
        at, ext_at = 0, 0
        for d in np.flatnonzero(np.diff(cut)):
            a, b = int(off[d]), int(off[d + 1])
            k0, k1 = int(cut[d]), int(cut[d + 1])
            pick, ex = greedy(fp[k0:k1] - a, fl[k0:k1], 0, b - a)
            assert ex == 0
            p, l, i = fp[k0:k1][pick], fl[k0:k1][pick], fi[k0:k1][pick]
            mine = {int(x): c.templates[int(x)] for x in set(i.tolist())}       # (assemble copies the dict it is given)
            r = tplref.assemble(np.frombuffer(raw[a:b], dtype=np.uint8), 0, b - a, p - a, l, i, mine)
            outs.append(raw[at:a])                              # the documents without a pick: their own bytes
            outs.append(r.replaced)
            at = b
            exts.append(r.extracted)
            poff.append(r.pick_off[1:] + np.uint64(ext_at))
            ext_at += len(r.extracted)
            dpos.append(p); dids.append(i); dlens.append(l)
            picks_per_doc[d] = pick.size
            out_len[d] = len(r.replaced)
        outs.append(raw[at:c.n_owned])
        cat = lambda xs: np.concatenate(xs) if xs else np.empty(0, dtype=np.int64)      # noqa: E731
        self.doc_pos, self.doc_ids, self.doc_lens = cat(dpos), cat(dids), cat(dlens)
        self.doc_first = np.concatenate(([0], np.cumsum(picks_per_doc))).astype(np.uint64)
        self.doc_replaced, self.doc_extracted = b"".join(outs), b"".join(exts)
        self.doc_out_off = np.concatenate(([0], np.cumsum(out_len))).astype(np.uint64)
        self.doc_pick_off = np.concatenate(poff)
        # the whole stream from the case's entry
        sel, self.exit = greedy(kpos, klens, c.entry, c.n_owned)
        self.sel = (kpos[sel], klens[sel], kids[sel])
        self.whole = tplref.assemble(c.data, c.entry, c.n_owned, *self.sel, c.templates)
        assert self.whole.exit == self.exit
        self.plain = splice(c.data, c.entry, c.n_owned, *self.sel, rep_table(c.reps))


@functools.lru_cache(maxsize=None)
def expectation(seed, tmp_dir):
    """(case, Expect) of a suite seed, made once per process."""
    c = LateCase(seed)
    return c, Expect(c, c.write_patterns(os.path.join(tmp_dir, f"late_{seed}.pat")))


def _same(got, want, what):
    got, want = np.asarray(got), np.frombuffer(want, dtype=np.uint8) if isinstance(want, bytes) else np.asarray(want)
    assert got.size == want.size, f"{what}: {got.size} entries, want {want.size}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: entry {int(bad[0])} is {got[bad[0]]}, want {want[bad[0]]} ({bad.size} differ)"


def _records(table, rec, pos, ids, what):
    assert rec.size == pos.size, f"{what}: {rec.size} records, want {pos.size}"
    _same(rec["pos"].astype(np.int64), pos, f"{what}: positions")
    _same(table.idmap[rec["state"]], ids, f"{what}: pattern ids")


def run_late_case(g_factory, case, tmp_dir, want=None):
    """One case on the GPU, one context: scan, offsets, span filter, group masks and gather, per-document selection,
    templated replace and extraction per document and over the whole stream, the plain replace and the templates
    again -- each step bit for bit against `Expect`.  Returns (records compared, bytes compared)."""
    c = case
    path = c.write_patterns(os.path.join(tmp_dir, f"late_{c.seed}.pat"))
    try:
        return _run(g_factory, c, path, Expect(c, path) if want is None else want)
    except AssertionError as e:
        raise AssertionError(f"{c.describe()}: {e}") from e


def _scan(g, c, w):
    total = g.scan_resident(c.n_owned, c.n)
    assert total == w.pos.size, f"scan: {total} records, want {w.pos.size}"
    return total


def _run(g_factory, c, path, w):
    table = c.table(path)
    assert table.max_pat_len == c.M
    nd = w.n_docs
    n_rec = n_bytes = 0
    with g_factory() as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        if not c.line_match:
            g.set_pattern_spans(c.rules)
        g.set_pattern_groups(c.groups)
        g.set_replacement_templates(c.templates)
        g.reserve(0, max(c.n, 1), max(c.n // 8, 4096))
        g.h2d(c.data)
        # 1 scan
        total = _scan(g, c, w)
        _records(table, g.records_to_host(total), w.pos, w.ids, "scan")
        fmt = g.scan_format()
        assert fmt[0] == record_width(table.num_final, c.knobs), f"record width {fmt[0]}"
        n_rec += total
        # 2 offsets
        if c.lines_half:
            got_docs, tail = g.split_documents(c.n_owned, c.delim)
            assert got_docs == w.split.size - 1, f"split: {got_docs} documents, want {w.split.size - 1}"
            _same(g.doc_offsets_to_host(got_docs).astype(np.int64), w.split, "split offsets")
            _same(w.split, w.off, "the case's offsets")
        else:
            g.set_doc_offsets(c.off)
        # 3 span filter
        n = g.filter_spans(delimiter=c.delim_arg, line_match=c.line_match, n_docs=nd)
        assert n == w.kpos.size, f"span filter: {n} records kept, want {w.kpos.size} of {w.pos.size}"
        assert g.last_count() == n and g.scan_format() == fmt, "span filter: count or format"
        _records(table, g.records_to_host(n), w.kpos, w.kids, "span filter")
        n_rec += n
        # 4 group masks, the predicate, the gather
        any_mask = g.document_group_masks(nd)
        _same(g.group_masks_to_host(nd), w.masks, "group masks")
        assert any_mask == w.any_mask, f"group masks: any_mask {any_mask:#x}, want {w.any_mask:#x}"
        n_ids = g.matching_documents_where(nd, **c.predicate)
        _same(g.matching_documents_to_host(n_ids), w.match_ids, "matching_documents_where")
        n_rec += nd + n_ids
        if c.lines_half:
            ob = g.gather_documents(nd, n_ids, c.n)
            _same(g.gathered_offsets_to_host(n_ids), w.gathered_off, "gather: offsets")
            _same(g.gathered_to_host(ob), w.gathered, "gather: bytes")
            n_bytes += ob
        # 5 per-document selection
        n_sel = g.select_leftmost_longest_documents(nd)
        first, sel = g.doc_selection_to_host(n_sel, nd)
        _same(first, w.doc_first, "per-document selection: doc_first")
        _records(table, sel, w.doc_pos, w.doc_ids, "per-document selection")
        n_rec += n_sel
        # 6 templated replace and extraction per document
        ob = g.replace_selection_documents()
        first_doc_out = g.replacement_to_host(ob)
        _same(first_doc_out, w.doc_replaced, "templated replace per document")
        _same(g.replacement_doc_offsets_to_host(nd), w.doc_out_off, "templated replace per document: output offsets")
        eb = g.extract_selection()
        _same(g.extracted_to_host(eb), w.doc_extracted, "extraction per document")
        _same(g.extract_offsets_to_host(n_sel), w.doc_pick_off, "extraction per document: pick offsets")
        n_bytes += ob + eb
        # 7 the whole stream
        n_sel, ex = g.select_leftmost_longest(c.entry)
        _records(table, g.selection_to_host(n_sel), w.sel[0], w.sel[2], "selection")
        assert ex == w.exit, f"selection: exit {ex}, want {w.exit}"
        ob = g.replace_selection()
        first_out = g.replacement_to_host(ob)
        _same(first_out, w.whole.replaced, "templated replace")
        eb = g.extract_selection()
        _same(g.extracted_to_host(eb), w.whole.extracted, "extraction")
        _same(g.extract_offsets_to_host(n_sel), w.whole.pick_off, "extraction: pick offsets")
        n_rec += n_sel
        n_bytes += ob + eb
        # 8 plain replacements on the same selection, then the templates again
        g.set_replacements(c.reps)
        pb = g.replace_selection()
        _same(g.replacement_to_host(pb), w.plain, "plain replace")
        g.set_replacement_templates(c.templates)
        ob2 = g.replace_selection()
        assert ob2 == ob and np.array_equal(g.replacement_to_host(ob2), first_out), "the templated replace behind a plain one differs"
        n_bytes += pb + ob2
        # 3 again without documents: the one document [0, n_avail)
        if w.keep_nodocs is not None:
            _scan(g, c, w)
            n = g.filter_spans(delimiter=c.delim_arg, line_match=c.line_match, n_docs=0)
            assert n == int(w.keep_nodocs.sum()) and g.last_count() == n and g.scan_format() == fmt, \
                f"span filter without documents: {n} kept, want {int(w.keep_nodocs.sum())}"
            _records(table, g.records_to_host(n), w.pos[w.keep_nodocs], w.ids[w.keep_nodocs], "span filter without documents")
            n_rec += n
    return n_rec, n_bytes


# ---------------------------------------------------------------------------
# the template piece ladder: one pattern `ab`, input lead + (gap + ab) ... + tail

LADDER_PATTERNS = [b"ab"]
LADDER_MODES = ("plain", "templated", "extract", "documents")
LADDER_EDGES = (WIN - 1, WIN, WIN + 1, 4 * WIN - 1, 4 * WIN, 4 * WIN + 1)
LADDER_TOTALS = (4 * WIN - 1, 4 * WIN, 4 * WIN + 1)          # a chunk's, a window's and a workgroup's end, and a byte either side


class LadderCase:
    def __init__(self, name, pre, suf, gaps, lead=0, tail=0):
        self.name, self.pre, self.suf, self.gaps, self.lead, self.tail = name, pre, suf, list(gaps), lead, tail
        self.prefix = bytes(65 + k % 26 for k in range(pre))
        self.suffix = bytes(48 + k % 10 for k in range(suf))
        self.data = np.frombuffer(b"x" * lead + b"".join(b"." * g + b"ab" for g in self.gaps) + b"y" * tail, dtype=np.uint8)
        at = lead + np.cumsum(np.array(self.gaps, dtype=np.int64) + 2) - 2
        self.pos = at                                           # where every `ab` is, by construction
        # documents: a cut in front of every third unit's gap, never inside a pick
        starts = np.concatenate(([lead], lead + np.cumsum(np.array(self.gaps, dtype=np.int64) + 2)[:-1]))
        self.off = np.unique(np.concatenate(([0], starts[::3], [self.data.size]))).astype(np.uint64)

    def templates(self, mode):
        return {1: self.prefix + self.suffix} if mode == "plain" else {1: (self.prefix, self.suffix)}

    def want(self, mode):
        """(output bytes, pick offsets or None, the boundaries of piece_boundaries) from tplref.assemble."""
        n = self.data.size
        lens, ids = np.full(self.pos.size, 2, dtype=np.int64), np.ones(self.pos.size, dtype=np.int64)
        r = tplref.assemble(self.data, 0, n, self.pos, lens, ids, self.templates(mode))
        b = piece_boundaries(self.pos, lens, ids, self.templates(mode), 0, n, extract=mode == "extract")
        return (r.extracted, r.pick_off, b) if mode == "extract" else (r.replaced, None, b)

    def __repr__(self):
        return self.name


def _unit_gaps(rot):
    return [(g + rot) % 18 for g in range(18)] * 2


@functools.lru_cache(maxsize=None)
def ladder_cases():
    out = []
    for pre in range(18):                                       # every length 0..17 of the gap, the prefix and the suffix
        out.append(LadderCase(f"steps-pre{pre}", pre, (7 * pre + 3) % 18, _unit_gaps(pre), lead=pre % 3, tail=3))
    # a named edge under every boundary of every instantiation: the lead (the extraction: the number of picks in
    # front and the template's lengths) is solved from the boundary's offset without it
    gaps = [4, 2, 7, 1, 9, 3, 5, 6]
    for mode in ("plain", "templated"):
        base = LadderCase("base", 5, 3, gaps)
        for kind, bs in enumerate(base.want(mode)[2]):
            if bs.size == 0:
                continue
            for T in LADDER_EDGES:
                out.append(LadderCase(f"edge-{mode}-kind{kind}-at{T}", 5, 3, gaps, lead=T - int(bs[1]), tail=2))
    for T in LADDER_EDGES:
        for kind in (1, 2, 3):
            pre, suf, k = next((p, s, (T - d) // (p + s + 2)) for p in range(1, 18) for s in range(1, 18)
                               for d in ((0, p, p + 2, p + s + 2)[kind],) if (T - d) % (p + s + 2) == 0)
            out.append(LadderCase(f"edge-extract-kind{kind}-at{T}", pre, suf, [1] * (k + 3)))
    # the total output ends at 4 KiB (a chunk's, a window's and a workgroup's end), and one byte either side
    for T in LADDER_TOTALS:
        for mode in ("plain", "templated"):
            base = LadderCase("base", 5, 3, gaps * 8, lead=3)
            out.append(LadderCase(f"total-{mode}-{T}", 5, 3, gaps * 8, lead=3, tail=T - len(base.want(mode)[0])))
        pre, suf = next((p, s) for p in range(1, 18) for s in range(1, 18) if T % (p + s + 2) == 0)
        out.append(LadderCase(f"total-extract-{T}", pre, suf, [2] * (T // (pre + suf + 2))))
    return tuple(out)


# ---------------------------------------------------------------------------
# the offsets rule: 70 000 documents over a scan of 70 001 bytes, one bad pair each

RULE_DOCS, RULE_BYTES = 70_000, 70_001
RULE_PATTERNS = [b"ab", b"b", b"abc", b"ca"]
RULE_GROUPS = [None, 0, 5, 63, (1, 2)]
RULE_SPANS = [None, "^", "^", (0, 5, None), (1, None, None)]


def rule_input():
    return np.frombuffer(b"abc", dtype=np.uint8)[np.random.default_rng(70001).integers(0, 3, RULE_BYTES)]


def rule_offsets(bad=None):
    """Good offsets (0, 2, 2, 4, 4, ...: documents of two bytes and empty ones in turn, the last one of one byte), or the
    same with one bad pair."""
    off = (2 * ((np.arange(RULE_DOCS + 1) + 1) // 2)).astype(np.uint64)
    off[-1] = RULE_BYTES
    if bad == "decrease-0":
        off[0] = 3
    elif bad == "decrease-255":
        off[255] = off[256] + np.uint64(1)
    elif bad == "decrease-65535":
        off[65535] = off[65536] + np.uint64(1)
    elif bad == "decrease-last":
        off[RULE_DOCS - 1] = RULE_BYTES + 1
    elif bad == "first-not-0":
        off[0] = 1
    elif bad == "last-not-n_owned":
        off[RULE_DOCS] = RULE_BYTES - 1
    else:
        assert bad is None
    return off


def rule_expect(path):
    """What the CPU says for the good offsets: the records, the masks, the segment cut, the whole-word filter with the
    documents as boundaries and the span filter (delimiter `c`) behind it."""
    import types
    import wordref
    data, good = rule_input(), rule_offsets().astype(np.int64)
    o = Oracle(path, 1, 1)
    pos, ids = o.scan_spec(data, None)
    o.close()
    pos, ids = pos.astype(np.int64), ids.astype(np.int64)
    lens = line_lengths(path)[ids]
    masks = groupref.masks_cut(pos, ids, lens, good, groupref.masks_by_id(RULE_GROUPS))
    doc = np.searchsorted(good, pos, side="right") - 1
    fits = pos + lens <= good[doc + 1]
    words = wordref.filter_words(data, pos, lens, off=good)
    spans = np.zeros(pos.size, dtype=bool)
    spans[words] = spanref.filter_spans(data, pos[words], lens[words], *spanref.record_spans(RULE_SPANS, ids[words]), ord("c"), good)
    return types.SimpleNamespace(data=data, pos=pos, ids=ids, lens=lens, masks=masks, fits=fits, words=words, spans=spans)


RULE_BAD = ("decrease-0", "decrease-255", "decrease-65535", "decrease-last", "first-not-0", "last-not-n_owned")
