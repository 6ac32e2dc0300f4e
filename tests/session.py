"""Model-based session tests: ONE context driven through a random sequence of calls, the way a long-running service
drives it -- many tables, many sizes, two slots, passes in any order, results fetched late.

Three parts, none of which needs a GPU to import:

  Pool / Expectations  a small pool of tables, inputs and whole-word filters, and what the CPU says about them (the CPU
                       oracle, its records passed through wordref for a filtered scan, then llref, replref, docref,
                       docreplref, orc.match_checksum -- as passfuzz.Expect, never the device, never
                       PfacTable.final_lengths), cached by (table, input, n_owned, ..., filter state).
  Model                what include/pfac.h PROMISES for every call given the calls before it: a value or a
                       PfacError.status.  It mirrors the header, not pfac_hip.hip; its state holds only keys into the cache.
  plan / run / shrink  plan(seed) draws about 60 operations, asking the model which are legal and picking an illegal one
                       about one time in eight; run(g, plan, model) performs them on a GpuMatcher (or anything shaped like
                       one) and compares bit for bit; shrink(seed, k) is the plan cut before operation k.
                       plan(seed, words=True) is a second family with the whole-word filter among the operations,
                       plan(seed, counts=True) a third with the per-pattern counts as well (pfac_records_count_states,
                       pfac_selection_count_states, pfac_state_counts_d2h: slot-owned counts that belong to a table
                       generation, are shared by two producers, can be added to and outlive everything else); the first
                       three are pinned to what they were before.  plan(seed, lines=True) is a fourth with the line
                       path as well: the delimiter split, the matching documents with and without context lines and
                       the gather of their bytes (split, doc_fetch, matching, context, ids_fetch, gather, ga_fetch,
                       gaoff_fetch), whose values come from splitref and gatherref.
                       plan(seed, fold=True) is a fifth with the case fold as well (set_fold, get_fold, an upload of
                       the image alone through load_table_device): the setting belongs to the uploaded table, a scan
                       keeps the mode it was queued with, and its expectation is the same CPU matcher over
                       nocaseref.fold(input) while every pass behind it keeps reading the original bytes.  It draws from
                       POOL: the nine tables of the other families and the four nocase tables of FOLD_TABLES.

The device under test hands out final STATES; they are mapped to pattern ids with the idmap of the table the scan ran
with (a stand-in that already works in ids says so with ``states_are_ids``)."""
import atexit
import copy
import os
import tempfile

import numpy as np

import countref
import nocaseref
import wordref
from classfuzz import ClassMatcher as _ClassMatcher
from docref import oracle_per_doc, random_offsets
from docreplref import per_doc
from gatherref import context_ids, gather_ref
from llref import greedy
from orc import Oracle, match_checksum
from passfuzz import GROUP, KNOB_NAMES, KNOBS, record_width
from phfpfac_amd import PfacError, PfacTable
from replref import rep_table, splice
from splitref import matching_ids, split_offsets

OK, E_ARG, E_STATE, E_OVERFLOW = 0, -1, -7, -8
STATUS_NAMES = {OK: "OK", E_ARG: "PFAC_E_ARG", E_STATE: "PFAC_E_STATE", E_OVERFLOW: "PFAC_E_OVERFLOW", None: "UNDEFINED"}
TILE = 4096
N_SLOTS = 2
SEEDS = list(range(24))                 # the suite's plans
WORD_SEEDS = list(range(24))            # ... and the seeds of its plans with the whole-word filter: plan(seed, words=True)
COUNT_SEEDS = list(range(24))           # ... and of its plans with the per-pattern counts as well: plan(seed, counts=True)
LINE_SEEDS = list(range(24))            # ... and of its plans with the line path as well: plan(seed, lines=True)
PLAN_OPS = 60
LINE_PLAN_OPS = 160                     # (a line plan is longer: its histories need a scan, offsets, a segment and ids first)
U64_MAX = 2**64 - 1
IN_STEP, REC_STEP = 8 << 20, 4 << 20    # reserve_grow number k asks for k * IN_STEP bytes / k * REC_STEP records: above
                                        # anything a plan's scans reserve (inputs <= 2 000 003 bytes, heaps below 4 Mi records)
REC = np.dtype([("pos", np.uint32), ("state", np.uint32)])

CCLASS = (b"[a-c]x\n" b"ax\n" b"[^a-z0-9 ]\n" b"q[0-9][0-9]\n" b"[a-c]\n" b"\\x41[\\x42-\\x44]\\n\n" b"[-a]z\n" b"ax[xy]\n"
          b"[a-c]x\n")
CCLASS_ALPHABET = b"abcxyzq0123456789 AB\nCD-Z!"
CCNEG = b"[^a]\n" b"ab[^c]\n" b"[^b]\n" b"[a-c][\\x00-\\xff]y\n" b"a\\n[^\\n]\n"      # one-byte negated classes: a record or two per byte
ESCNL = b"\\n\n" b"a\\nb\n" b"\\nx\n" b"x\\n\n" b"\\x00\\n\\x00\n" b"\\x61\\x0ab\n" b"q\\012\n" b"\\n\\n\n"   # newline as first, middle, last byte; a duplicate


def _k(**knobs):
    return KNOBS.index(knobs)


# name -> how the table is made, which entries of passfuzz.KNOBS it may be installed under, and its inputs (name, bytes,
# style).  Together: 2-, 4- and 8-byte records, tables in LDS and through L2, dense mode's second form, a character-class
# table, duplicate lines; every size of passfuzz.Case; one dense and one matchless input of >= 64 tiles for a table with
# no knob pinned, so the staging mode can flip; a class table whose one-byte negated classes give a record or two per byte
# and an escaped table with newline edges, both in LDS, through L2 and in dense mode.
TABLES = {
    "abc2": dict(lines=[b"a", b"ab", b"abc"], knobs=[_k()],
                 inputs=[("dense", 300_007, "abc:0.3"), ("none", 300_007, "abc:0"), ("thin", GROUP + 1, "abc:0.02"), ("s17", 17, "abc:0.3")]),
    "mid4": dict(gen=(101, 26, 150, 8, 0), knobs=[_k(), _k(PFAC_LAG="1"), _k(PFAC_LAG="2"), _k(PFAC_L2F="0"), _k(PFAC_L2F="2"),
                                                   _k(PFAC_L2F="3"), _k(PFAC_NWB="4"), _k(PFAC_TICKET_WAYS="1"), _k(PFAC_TICKET_WAYS="2")],
                 inputs=[("big", 2_000_003, "plant"), ("t4097", 4097, "plant"), ("g1", GROUP + 1, "plant")]),
    "wide8": dict(gen=(102, 8, 40, 6, 0), knobs=[_k(PFAC_WIDE="1")],
                  inputs=[("t4095", 4095, "plant"), ("gm1", GROUP - 1, "plant"), ("one", 1, "plant")]),
    "l2": dict(gen=(103, 4, 40, 14, 0), knobs=[_k(PFAC_FORCE_L2="1"), _k(PFAC_FORCE_L2="1", PFAC_NO_FUSE="1"),
                                                _k(PFAC_FORCE_L2="1", PFAC_NO_D1="1"), _k(PFAC_L2F="3", PFAC_FORCE_L2="1"),
                                                _k(PFAC_NO_SECF="1", PFAC_FORCE_L2="1")],
               inputs=[("m300", 300_007, "plant"), ("t4097", 4097, "plant"), ("s17", 17, "plant")]),
    "dense2": dict(gen=(104, 3, 20, 3, 0), knobs=[_k(PFAC_FORCE_L2="1", PFAC_DENSE="1"), _k(PFAC_FORCE_L2="1", PFAC_DENSE="1", PFAC_D2_LOGCAP="64"),
                                                   _k(PFAC_FORCE_L2="1", PFAC_DENSE="1", PFAC_NWB="5"),
                                                   _k(PFAC_FORCE_L2="1", PFAC_NO_NW4="1", PFAC_DENSE="1"),
                                                   _k(PFAC_FORCE_L2="1", PFAC_DENSE="1", PFAC_NO_DENSE2="1")],
                   inputs=[("g1", GROUP + 1, "plant"), ("t4095", 4095, "plant"), ("empty", 0, "plant")]),
    "cclass": dict(cclass=CCLASS, knobs=[_k(), _k(PFAC_REC_BYTES="4")],
                   inputs=[("gm1", GROUP - 1, "cc"), ("t4097", 4097, "cc"), ("one", 1, "cc")]),
    "negcc": dict(cclass=CCNEG, knobs=[_k(), _k(PFAC_FORCE_L2="1"), _k(PFAC_FORCE_L2="1", PFAC_DENSE="1"), _k(PFAC_DENSE="1")],
                  inputs=[("t4095", 4095, "cc"), ("m70", 70_001, "cc")]),
    "nlesc": dict(escaped=ESCNL, knobs=[_k(), _k(PFAC_FORCE_L2="1"), _k(PFAC_FORCE_L2="1", PFAC_DENSE="1"), _k(PFAC_DENSE="1")],
                  inputs=[("g1", GROUP + 1, "cc0"), ("s17", 17, "cc0")]),
    "dups": dict(gen=(105, 3, 9, 4, 3), knobs=[_k(), _k(PFAC_DENSE="1")],
                 inputs=[("m300", 300_007, "plant"), ("t4095", 4095, "plant"), ("empty", 0, "plant")]),
}
# The tables of the fold family (plan(seed, fold=True)), next to the nine above, which the pinned plans index and which
# stay as they are: four small tables with `nocase` -- built with ignore_case=True, so that GpuMatcher.load_table leaves
# the case fold ON after the upload -- whose inputs are mixed-case text.  wordsi: words and letters of paragraph402 in
# Title and UPPER case, fifteen lines (two-byte records), one dense and one matchless input of >= 64 tiles, so that the
# staging mode flips with the fold on; symi: nocaseref.symbol_patterns(); cclassi: a class file through
# from_charclass(..., ignore_case=True); root1i: the one-edge root of nocaseref.root1_cases().
WORDSI = (b"A\n" b"I\n" b"E\n" b"T\n" b"O\n" b"N\n" b"The\n" b"AND\n" b"In\n" b"ENGLAND\n" b"Cricket\n" b"WITH\n" b"Over\n" b"Team\n"
          b"TEAM\n")                                              # (fifteen lines: two-byte records hold sixteen final states)
CCLASSI = b"[A-C]x\n" b"[^A]b\n" b"[^a-z0-9 ]\n" b"q[0-9][0-9]\n" b"Ax\n" b"B[x-z]\n" b"[a-c]X\n"     # (the last: the first in the other case)
CCLASSI_UNIT = b"Ax bX cx.AB ab Q12 q07-b Zb!aX By,q1x CX;bb.Cz Q99 "
ROOT1I = b"Qa\nQb\nQax\nQbY\n"
ROOT1I_UNIT = b"..Qa..QA.QAB.xa.QABC,QB;QBY QAX-QCZ.xcz..QC" + b"." * 21      # (nocaseref.root1_cases: no lower-case q anywhere)
NOMATCH_UNIT = b"0123456789 .,;-\n"                              # (no letter: matchless for wordsi, folded or not)
FOLD_TABLES = {
    "wordsi": dict(patterns=WORDSI, nocase=True,
                   knobs=[_k(), _k(PFAC_LAG="1"), _k(PFAC_LAG="2"), _k(PFAC_L2F="3"), _k(PFAC_TICKET_WAYS="1"), _k(PFAC_NWB="4")],
                   inputs=[("dense", 300_007, "mixed"), ("none", 300_007, "nomatch"), ("g1", GROUP + 1, "mixed"), ("t4097", 4097, "mixed"),
                           ("s17", 17, "mixed")]),
    "symi": dict(patterns=nocaseref.symbol_patterns(), nocase=True,
                 knobs=[_k(PFAC_FORCE_L2="1"), _k(PFAC_FORCE_L2="1", PFAC_DENSE="1"), _k(PFAC_FORCE_L2="1", PFAC_DENSE="1", PFAC_D2_LOGCAP="64"),
                        _k(PFAC_REC_BYTES="4")],
                 inputs=[("m70", 70_001, "mixedsym"), ("t4095", 4095, "mixedsym"), ("one", 1, "mixedsym")]),
    "cclassi": dict(cclass=CCLASSI, nocase=True, knobs=[_k(), _k(PFAC_REC_BYTES="4"), _k(PFAC_FORCE_L2="1"), _k(PFAC_DENSE="1")],
                    inputs=[("gm1", GROUP - 1, "ccunit"), ("t4097", 4097, "ccunit")]),
    "root1i": dict(patterns=ROOT1I, nocase=True, knobs=[_k(), _k(PFAC_FORCE_L2="1"), _k(PFAC_L2F="0"), _k(PFAC_L2F="2")],
                   inputs=[("t3", 3 * TILE + 11, "root1"), ("s17", 17, "root1")]),
}
# One more input for each of the nine old tables, which only the fold family scans (TABLES itself stays byte for byte):
# the table's own input 0 (input 1 where that is the large one) with a seeded half of its lower-case letters in upper
# case -- for abc2, whose inputs hold a, b and c only, that is the one input the fold changes anything for.
FOLD_INPUTS = {t: ("upper", TABLES[t]["inputs"][1 if t == "mid4" else 0][1], "upper:%d" % (1 if t == "mid4" else 0)) for t in TABLES}
POOL = {t: dict(d, inputs=d["inputs"] + [FOLD_INPUTS[t]]) for t, d in TABLES.items()}
POOL.update(FOLD_TABLES)
FOLD_SEEDS = list(range(24))            # ... and of its plans with the case fold as well: plan(seed, fold=True)
FOLD_PLAN_OPS = 120


def _tix(t):
    """The number of table `t` in the seeds of what is drawn for it (the nine old tables keep theirs)."""
    return sorted(TABLES).index(t) if t in TABLES else len(TABLES) + sorted(FOLD_TABLES).index(t)


REP_KEYS = ("r0", "r1", "redact")
DOC_KEYS = ("d0", "d1", "bad_end", "bad_order")
TEXT_BASES = (0, 999_999_990)

# The whole-word filters a session may apply: a small fixed pool, so that the expectations of a filtered scan are shared
# between plans.  ws: "def" = NULL ([0-9A-Za-z_]), "hi" = that and 0x80..0xFF, "tab" = a part of the table's own alphabet
# (WORD_TAB; the gen tables draw their symbols from all 256 bytes, where the default set says next to nothing).
# prev / next: -1 = no byte, "w" = a word byte of the set, "n" = a byte outside it.  doc: "none" = n_docs 0, "slot" = the
# slot's document offsets (whatever set_doc left there: d0, d1, bad_end, bad_order, or none) and their n_docs, "wrong_n" =
# the slot's offsets with an n_docs that is not theirs.
FILTERS = (
    dict(edges="both", ws="def", prev=-1, next=-1, doc="none"),
    dict(edges="both", ws="tab", prev=-1, next=-1, doc="none"),
    dict(edges="left", ws="tab", prev="w", next="n", doc="none"),
    dict(edges="right", ws="tab", prev="n", next="w", doc="none"),
    dict(edges="both", ws="hi", prev="w", next="w", doc="none"),
    dict(edges="left", ws="tab", prev=-1, next="w", doc="slot"),
    dict(edges="right", ws="tab", prev="w", next=-1, doc="slot"),
    dict(edges="both", ws="tab", prev="n", next="n", doc="slot"),
    dict(edges="both", ws="hi", prev="w", next="n", doc="slot"),
    dict(edges="left", ws="def", prev="n", next="w", doc="slot"),
    dict(edges="both", ws="tab", prev=-1, next=-1, doc="wrong_n"),
)
EDGE_BITS = {"left": wordref.LEFT, "right": wordref.RIGHT, "both": wordref.BOTH}
# The count knobs a table may be installed under in the count family (read at the upload, like passfuzz.KNOBS, which the
# pinned plans index and which therefore stays as it is): with 3 to 150 final states the pool's automata then run the
# cache regime with collisions (num_final above the bins) and the grid-stride loop.
CKNOBS = ({}, {"PFAC_COUNT_BINS": "1"}, {"PFAC_COUNT_BINS": "16"}, {"PFAC_COUNT_GRID": "2"}, {"PFAC_COUNT_BINS": "16", "PFAC_COUNT_THREADS": "256"})
CKNOB_NAMES = ("PFAC_COUNT_BINS", "PFAC_COUNT_GRID", "PFAC_COUNT_THREADS")
COUNT_DIRECT_MAX = 8192                 # final states a workgroup's LDS table holds (include/pfac.h); fewer under PFAC_COUNT_BINS
CNT_FILL = 0x11                         # a fresh caller's count buffer: every entry CNT_ENTRY, so that an accumulate that
CNT_ENTRY = CNT_FILL * 0x0101010101010101   # zeroes, or a plain count that does not, shows at the first use
OUT_FILL = 0xC7                         # every byte of a fresh caller's pass output and of the guard bands around it
MAX_FILTERS = 3                         # distinct filters on one scan: more would only thin out the cache
WORD_TAB = {"cclass": b"abcxyz", "negcc": b"abcy", "nlesc": b"abxq\n"}     # (the other tables: the first half of their symbols)
WORD_TAB.update({t: b"abcdefghijklmnopqrstuvwxyz" for t in FOLD_TABLES})       # lower-case letters only: the set separates the cases


def _gen_lines(seed, alpha, npat, maxlen, dups):
    rng = np.random.default_rng([seed, 0x53455353])
    symbols = rng.permutation(np.array([b for b in range(256) if b != 10], dtype=np.uint8))[:alpha]
    pats = set()
    for _ in range(npat * 4):
        if len(pats) >= npat:
            break
        pats.add(bytes(symbols[rng.integers(0, alpha, int(rng.integers(1, maxlen + 1)))]))
    lines = sorted(sorted(pats), key=lambda x: rng.random())     # (sorted first: a set of bytes iterates in another order in every process)
    for _ in range(dups):                                      # duplicate lines: unreachable final states
        lines.insert(int(rng.integers(0, len(lines) + 1)), lines[int(rng.integers(0, len(lines)))])
    return lines, symbols


class Expectations:
    """What the CPU says, computed once per key."""

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="pfac_session_")
        self._c = {}

    def _memo(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    # -- tables -------------------------------------------------------------
    def _table(self, t):
        d = POOL[t]
        if "cclass" in d and d.get("nocase"):                   # (the reference: the class image with its listed sets folded, nocaseref.folded_classes)
            m = _ClassMatcher(d["cclass"], parsed=nocaseref.folded_classes(d["cclass"]))
            return dict(table=PfacTable.from_charclass(d["cclass"], 256, ignore_case=True), matcher=m, ll=m.lens, symbols=None, lines=None)
        if "cclass" in d:
            m = _ClassMatcher(d["cclass"])
            return dict(table=PfacTable.from_charclass(d["cclass"], 256), matcher=m, ll=m.lens, symbols=None, lines=None)
        if "patterns" in d:                                     # a nocase table: the file as written goes to the builder, its numpy fold to the CPU oracle
            assert d["nocase"]
            path = os.path.join(self.dir, t + ".pat")
            with open(path, "wb") as f:
                f.write(d["patterns"])
            with open(path + ".folded", "wb") as f:
                f.write(nocaseref.fold_bytes(d["patterns"]))
            ll = np.array([0] + [len(p) for p in d["patterns"][:-1].split(b"\n")], dtype=np.int64)
            return dict(table=PfacTable.from_file(path, 256, ignore_case=True), matcher=Oracle(path + ".folded", 1, 1), ll=ll, symbols=None, lines=None)
        if "escaped" in d:                                      # (lengths from the parsed lines; the matcher is the CPU oracle's escape-aware reader)
            path = os.path.join(self.dir, t + ".pat")
            with open(path, "wb") as f:
                f.write(d["escaped"])
            return dict(table=PfacTable.from_file(path, 256, escapes=True), matcher=Oracle(path, 1, 1, escapes=True),
                        ll=_ClassMatcher(d["escaped"], "last").lens, symbols=None, lines=None)
        lines, symbols = (d["lines"], np.frombuffer(b"abc", dtype=np.uint8)) if "lines" in d else _gen_lines(*d["gen"])
        path = os.path.join(self.dir, t + ".pat")
        with open(path, "wb") as f:
            f.write(b"".join(p + b"\n" for p in lines))
        ll = np.array([0] + [len(p) for p in lines], dtype=np.int64)      # the file's own lines
        return dict(table=PfacTable.from_file(path, 256), matcher=Oracle(path, 1, 1), ll=ll, symbols=symbols, lines=lines)

    def tinfo(self, t):
        return self._memo(("table", t), lambda: self._table(t))

    def close(self):
        """Frees the CPU oracles of the tables made so far (they serve every later expectation, so not before)."""
        for key in [k for k in self._c if k[0] == "table"]:
            m = self._c.pop(key)["matcher"]
            if hasattr(m, "close"):
                m.close()

    def table(self, t):
        return self.tinfo(t)["table"]

    def M(self, t):
        return int(self.table(t).max_pat_len)

    def width(self, t, knob):
        return record_width(int(self.table(t).num_final), KNOBS[knob])

    # -- inputs -------------------------------------------------------------
    def _input(self, t, i):
        name, n, style = POOL[t]["inputs"][i]
        if style in ("mixed", "mixedsym"):
            return nocaseref.mixed_text(n, seed=402 + i, symbols=style == "mixedsym")
        if style in ("nomatch", "ccunit", "root1"):
            return nocaseref.tiled(n, {"nomatch": NOMATCH_UNIT, "ccunit": CCLASSI_UNIT, "root1": ROOT1I_UNIT}[style])
        if style.startswith("upper:"):                          # (the fold family's extra input of an old table)
            buf = self.input(t, int(style[6:])).copy()
            if t == "abc2":
                buf = buf[:n].copy()
            lower = (buf >= 0x61) & (buf <= 0x7A)
            buf[lower & (np.random.default_rng([_tix(t), 0x5550]).random(buf.size) < 0.5)] &= 0xDF
            return buf
        rng = np.random.default_rng([_tix(t), i, 0x494E])
        if style.startswith("abc:"):
            d = float(style[4:])
            u = rng.random(n)
            return np.where(u < d, ord("a"), np.where(u < d + 0.3, ord("b"), ord("c"))).astype(np.uint8)
        if style in ("cc", "cc0"):                              # (cc0: with byte 0, which the escaped table's lines hold)
            alphabet = np.frombuffer(CCLASS_ALPHABET + (b"\x00\x00\x00" if style == "cc0" else b""), dtype=np.uint8)
            return alphabet[rng.integers(0, alphabet.size, n)]
        info = self.tinfo(t)
        sym = info["symbols"]
        data = sym[rng.integers(0, sym.size, n)]
        plist = sorted(set(info["lines"]))
        for at in rng.integers(0, max(n - 1, 1), n // 50):
            pt = np.frombuffer(plist[int(rng.integers(0, len(plist)))], dtype=np.uint8)
            m = min(len(pt), n - int(at))
            data[int(at):int(at) + m] = pt[:m]
        return data

    def input(self, t, i):
        return self._memo(("input", t, i), lambda: self._input(t, i))

    def input_size(self, t, i):
        return POOL[t]["inputs"][i][1]

    # -- whole-word filters ---------------------------------------------------
    def word_bytes(self, t, ws):
        """The bytes of word set `ws` for table `t` (None: the call's NULL, the default set)."""
        if ws == "def":
            return None
        if ws == "hi":
            return wordref.DEFAULT_WORD + bytes(range(0x80, 0x100))
        sym = self.tinfo(t)["symbols"]
        return WORD_TAB[t] if sym is None else bytes(sym[:(sym.size + 1) // 2])

    def neighbour(self, t, ws, which):
        """The prev_byte / next_byte of a descriptor: -1, or the smallest byte inside ("w") / outside ("n") the set."""
        if which == -1:
            return -1
        inside = set(self.word_bytes(t, ws) or wordref.DEFAULT_WORD)
        return min(b for b in range(256) if (b in inside) == (which == "w"))

    def applied(self, t, f, dkey):
        """Descriptor FILTERS[f] as applied to a scan of table `t`: (edge bits, ws, prev_byte, next_byte, dkey or "").
        A scan's filter state is the sorted tuple of the distinct ones applied to it."""
        d = FILTERS[f]
        return (EDGE_BITS[d["edges"]], d["ws"], self.neighbour(t, d["ws"], d["prev"]), self.neighbour(t, d["ws"], d["next"]), dkey or "")

    def _keep(self, t, i, no, one, fold=False):
        """The keep mask of ONE applied filter over the unfiltered records of the scan (composition is intersection).
        The filter judges the ORIGINAL bytes, whatever the scan's fold."""
        def make():
            edges, ws, prev, nxt, dkey = one
            chars = self.word_bytes(t, ws)
            bits = None
            if chars is not None:
                bits = np.zeros(4, dtype=np.uint64)
                for b in chars:
                    bits[b >> 6] |= np.uint64(1 << (b & 63))
            pos, _, lens = self.scan(t, i, no, fold=fold)
            off = self.offsets(t, i, no, dkey) if dkey else None
            return wordref.filter_words(self.input(t, i), pos, lens, bits, edges, prev, nxt, off)   # (n_avail: the whole input)
        return self._memo(("keep", t, i, no, fold, one), make)

    # -- the scan -----------------------------------------------------------
    def scan(self, t, i, no, f=(), fold=False):
        """(pos, ids, lens) of the records that start in [0, no); walks may read the whole input (the halo).  `f`: the
        scan's filter state (`applied`), whose filters the records have passed.  `fold`: a case-insensitive scan -- the
        header's sentence and nothing else: the same matcher (the same pattern file) over nocaseref.fold(input).  The
        cache keys a scan by (table, input, n_owned, fold, filter state)."""
        def make():
            info = self.tinfo(t)
            data = nocaseref.fold(self.input(t, i)) if fold else self.input(t, i)
            pos, ids = self._memo(("whole", t, i, fold), lambda: info["matcher"].scan_spec(data, None))
            own = pos < no
            pos, ids = pos[own].astype(np.int64), ids[own].astype(np.int64)
            return pos, ids, info["ll"][ids]

        def filtered():
            pos, ids, lens = self.scan(t, i, no, fold=fold)
            keep = np.ones(pos.size, dtype=bool)
            for one in f:
                keep &= self._keep(t, i, no, one, fold)
            return pos[keep], ids[keep], lens[keep]
        return self._memo(("scan", t, i, no, fold, f), filtered) if f else self._memo(("scan", t, i, no, fold), make)

    def fold_differs(self, t, i):
        """Whether the fold changes the records of the whole input `i` of table `t` (the same matcher, folded or not)."""
        def make():
            a, b = self.scan(t, i, self.input_size(t, i)), self.scan(t, i, self.input_size(t, i), fold=True)
            return a[0].size != b[0].size or not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
        return self._memo(("differs", t, i), make)

    def count(self, t, i, no, f=(), fold=False):
        return int(self.scan(t, i, no, f, fold)[0].size)

    def text(self, t, i, no, base, f=(), fold=False):
        def make():
            pos, ids, _ = self.scan(t, i, no, f, fold)
            return "".join("At position %4d, match pattern %d\n" % (p + base, k) for p, k in zip(pos.tolist(), ids.tolist())).encode()
        return self._memo(("text", t, i, no, fold, base, f), make)

    def checksum(self, t, i, no, base, f=(), fold=False):
        pos, ids, _ = self.scan(t, i, no, f, fold)
        return match_checksum(pos + base, ids)

    # -- selection and replace ------------------------------------------------
    def sel(self, t, i, no, entry, f=(), fold=False):
        """(pos, ids, exit) of the leftmost-longest selection from `entry`."""
        def make():
            pos, ids, lens = self.scan(t, i, no, f, fold)
            idx, ex = greedy(pos, lens, entry, no)
            return pos[idx], ids[idx], int(ex)
        return self._memo(("sel", t, i, no, fold, entry, f), make)

    def reps(self, t, rkey):
        def make():
            ll = self.tinfo(t)["ll"]
            if rkey == "redact":
                return {k: b"#" * int(ll[k]) for k in range(1, ll.size)}
            rng = np.random.default_rng([_tix(t), REP_KEYS.index(rkey), 0x5245])
            return {k: rng.integers(0, 256, int(rng.integers(1000, 3000)) if rng.random() < 0.02 else int(rng.integers(0, 33))).astype(np.uint8).tobytes()
                    for k in range(1, ll.size)}
        return self._memo(("reps", t, rkey), make)

    def replace(self, t, i, no, entry, rkey, f=(), fold=False):
        def make():                                             # (the splice copies the ORIGINAL bytes between the picks)
            spos, sids, _ = self.sel(t, i, no, entry, f, fold)
            return splice(self.input(t, i), entry, no, spos, self.tinfo(t)["ll"][sids], sids, rep_table(self.reps(t, rkey)))
        return self._memo(("replace", t, i, no, fold, entry, rkey, f), make)

    # -- documents ----------------------------------------------------------
    def delims(self, t, i):
        """The delimiters a session splits input `i` of table `t` at: (its most frequent byte, its rarest byte that
        occurs, a byte that does not occur) -- for the empty input, three newlines."""
        def make():
            h = np.bincount(self.input(t, i), minlength=256)
            if not h.any():
                return (10, 10, 10)
            present = np.flatnonzero(h)
            assert (h == 0).any(), "every byte occurs: no delimiter without a document end"
            return int(np.argmax(h)), int(present[np.argmin(h[present])]), int(np.flatnonzero(h == 0)[0])
        return self._memo(("delims", t, i), make)

    def split(self, t, i, nb, delim):
        """(offsets, n_docs, tail_start) of the first `nb` bytes of the input cut at `delim` (splitref.split_offsets)."""
        return self._memo(("split", t, i, nb, delim), lambda: split_offsets(self.input(t, i)[:nb], delim))

    def offsets(self, t, i, no, dkey):
        """The document offsets `dkey` of the first `no` bytes of input `i`: one of DOC_KEYS (seeded cuts), or
        "split:<byte>" -- what the device-side split at that delimiter leaves in the slot."""
        if dkey.startswith("split:"):
            return self.split(t, i, no, int(dkey[6:]))[0]

        def make():
            rng = np.random.default_rng([_tix(t), i, no, DOC_KEYS.index(dkey), 0x444F])
            off = random_offsets(rng, no, int(rng.integers(1, 60)), empties=int(rng.integers(0, 4)))
            cuts = [c for k in rng.integers(1, max(no // TILE, 1) + 1, 2) for c in (int(k) * TILE - 1, int(k) * TILE, int(k) * TILE + 1) if c <= no]
            off = np.sort(np.concatenate([off, np.array(cuts, dtype=np.uint64)]))
            if dkey == "d1":                                   # empty documents at the very end
                off = np.concatenate([off, np.array([no, no], dtype=np.uint64)])
            if dkey == "bad_end":
                off = off.copy()
                off[-1] = no + 1
            if dkey == "bad_order":
                tail = [no + 2, no] if no < 2 else [no - 1, no - 2, no]
                off = np.concatenate([off[:1] if no < 2 else off[:-1], np.array(tail, dtype=np.uint64)])
            return off.astype(np.uint64)
        return self._memo(("off", t, i, no, dkey), make)

    def _doc_matcher(self, t, i, no, dkey, f, fold=False):
        """What docref / docreplref scan every document with: the CPU oracle (under the fold: the oracle over the folded
        bytes of the document it is handed), or for a filtered scan the scan's kept records cut at the documents (the
        filter judged them in the whole buffer, which no scan of a document repeats)."""
        if f:
            return _DocCut(self.scan(t, i, no, f, fold), self.offsets(t, i, no, dkey))
        return _Folding(self.tinfo(t)["matcher"]) if fold else self.tinfo(t)["matcher"]

    def seg(self, t, i, no, dkey, f=(), fold=False):
        """(doc_first, pos relative to the document, ids) of every document scanned on its own."""
        def make():
            first, pos, ids = oracle_per_doc(self._doc_matcher(t, i, no, dkey, f, fold), self.input(t, i)[:no], self.offsets(t, i, no, dkey))
            return first, pos.astype(np.int64), ids.astype(np.int64)
        return self._memo(("seg", t, i, no, fold, dkey, f), make)

    def docsel(self, t, i, no, dkey, f=(), rkey=None, fold=False):
        """(doc_first, pos relative to the SCAN, ids, out_off, out) of every document's own selection (and output, spliced
        from the ORIGINAL bytes)."""
        def make():
            off = self.offsets(t, i, no, dkey)
            tab = None if rkey is None else rep_table(self.reps(t, rkey))
            first, pos, ids, out_off, out = per_doc(self._doc_matcher(t, i, no, dkey, f, fold), self.input(t, i)[:no], off, self.tinfo(t)["ll"], tab)
            doc = np.repeat(np.arange(off.size - 1, dtype=np.int64), np.diff(first.astype(np.int64)))
            return first, pos.astype(np.int64) + off[doc].astype(np.int64), ids.astype(np.int64), out_off, out
        return self._memo(("docsel", t, i, no, fold, dkey, f, rkey), make)


    # -- lines: matching documents and their bytes ---------------------------
    def doc_first(self, src, key):
        """The doc_first a matching call reads: of the segment ("seg") or of the per-document selection ("docsel") `key`."""
        return self.seg(*key)[0] if src == "seg" else self.docsel(*key[:5], None, key[5])[0]

    def doc_ids(self, spec):
        """The ids of a matching call.  spec = (src, key, "m", invert) or (src, key, "c", before, after):
        splitref.matching_ids / gatherref.context_ids over doc_first(src, key)."""
        def make():
            first = self.doc_first(spec[0], spec[1])
            return matching_ids(first, spec[3]) if spec[2] == "m" else context_ids(first, spec[3], spec[4])
        return self._memo(("ids",) + spec, make)

    def id_list(self, spec, form, n_docs):
        """The ids a gather is given.  form "own": those of matching call `spec`; else a caller's list made from them
        (from 0 .. min(n_docs, 40) - 1 without a matching call): "same", a permutation ("perm"), reversed ("rev"), every
        id twice ("twice"), none ("empty"), or with one entry replaced by n_docs ("bad_id"); "all": every document."""
        if form == "all":
            return np.arange(n_docs, dtype=np.uint64)
        base = self.doc_ids(spec) if spec is not None else np.arange(min(n_docs, 40), dtype=np.uint64)
        if form in ("own", "same"):
            return base
        if form == "perm":
            return base[np.random.default_rng([base.size, 0x504D]).permutation(base.size)]
        if form == "rev":
            return base[::-1].copy()
        if form == "twice":
            return np.repeat(base, 2)
        if form == "empty":
            return base[:0]
        assert form == "bad_id"
        bad = np.append(base, np.uint64(0))[:max(base.size, 1)].copy()
        bad[bad.size // 2] = n_docs
        return bad

    def gather(self, t, i, nb, doc, spec, form):
        """(out, out_off) of gatherref.gather_ref over the first `nb` bytes of input `i` of table `t`, the offsets `doc`
        (an argument tuple of `offsets`) and id_list(spec, form)."""
        def make():
            off = self.offsets(*doc)
            return gather_ref(self.input(t, i)[:nb], off, self.id_list(spec, form, int(off.size) - 1))
        return self._memo(("gather", t, i, nb, doc, spec, form), make)

    # -- counts per pattern ---------------------------------------------------
    # A contribution to a count buffer ("part"): ("scan", t, i, no, f, fold), ("sel", t, i, no, entry, f, fold) or
    # ("docsel", t, i, no, dkey, f, fold) -- the arguments of scan / sel / docsel above.
    def n_ids(self, t):
        return int(self.tinfo(t)["ll"].size)

    def injective(self, t):
        """Whether no two final states of table `t` report the same pattern id (then counts compare per state too)."""
        idmap = np.asarray(self.table(t).idmap)
        return int(np.unique(idmap).size) == int(self.table(t).num_final)

    def part_ids(self, part):
        return {"scan": lambda: self.scan(*part[1:])[1], "sel": lambda: self.sel(*part[1:])[1], "docsel": lambda: self.docsel(*part[1:6], None, part[6])[2]}[part[0]]()

    def part_counts(self, part):
        """uint64[n_ids]: the histogram by pattern id of one contribution (numpy.bincount over the CPU's records)."""
        return self._memo(("cnt",) + part, lambda: np.bincount(self.part_ids(part), minlength=self.n_ids(part[1])).astype(np.uint64))

    def part_states(self, part):
        """uint64[num_final]: the same by final state, for a table whose idmap is injective (countref.state_counts)."""
        assert self.injective(part[1])
        return self._memo(("cnts",) + part, lambda: countref.state_counts(self.table(part[1]), self.part_ids(part)))

    def state_counts(self, t, i, no, f=(), fold=False):
        """Counts by pattern id of Expectations.scan(t, i, no, f, fold)."""
        return self.part_counts(("scan", t, i, no, f, fold))

    def sel_counts(self, t, i, no, entry=0, f=(), dkey=None, fold=False):
        """Counts by pattern id of the picks of sel(t, i, no, entry, f), or with `dkey` of docsel(t, i, no, dkey, f)."""
        return self.part_counts(("sel", t, i, no, entry, f, fold) if dkey is None else ("docsel", t, i, no, dkey, f, fold))

    def sum_counts(self, t, parts, by_state=False):
        out = np.zeros(int(self.table(t).num_final) if by_state else self.n_ids(t), dtype=np.uint64)
        for part in parts:
            out = out + (self.part_states(part) if by_state else self.part_counts(part))
        return out


class _Folding:
    """The CPU matcher over the folded bytes of whatever it is handed (the documents of a folded scan, one at a time)."""

    def __init__(self, matcher):
        self.matcher = matcher

    def scan_spec(self, buf, *rest):
        return self.matcher.scan_spec(nocaseref.fold(buf), *rest)


class _DocCut:
    """Stands where the CPU oracle stands in docref.oracle_per_doc for a FILTERED scan: asked for the non-empty documents
    in turn, it answers with the scan's kept records that lie inside each one, positions relative to the document."""

    def __init__(self, rows, off):
        self.rows = rows
        off = off.astype(np.int64)
        self.ranges = iter([(int(a), int(b)) for a, b in zip(off[:-1], off[1:]) if b > a])

    def scan_spec(self, buf, *_):
        a, b = next(self.ranges)
        assert buf.size == b - a
        pos, ids, lens = self.rows
        lo, hi = np.searchsorted(pos, [a, b], side="left")
        inside = pos[lo:hi] + lens[lo:hi] <= b
        return pos[lo:hi][inside] - a, ids[lo:hi][inside]


_EXP = None


def expectations():
    global _EXP
    if _EXP is None:
        _EXP = Expectations()
        atexit.register(_EXP.close)
    return _EXP


def offsets_ok(off, n_owned):
    off = off.astype(np.int64)
    return bool(off[0] == 0 and off[-1] == n_owned and (np.diff(off) >= 0).all())


# ---------------------------------------------------------------------------
# the model

class Exp:
    """What the contract says about one operation: a status and, for OK, the value (computed on demand); `count` is the
    exact figure an overflow error must carry; `tab` the table whose idmap the device's states belong to."""
    __slots__ = ("status", "fn", "count", "tab")

    def __init__(self, status=OK, fn=None, count=None, tab=None):
        self.status, self.fn, self.count, self.tab = status, fn, count, tab

    def value(self):
        return self.fn() if self.fn else None


class _Slot:
    def __init__(self):
        self.scan = None          # the slot's last scan: dict(tab, knob, gen, inp, no, over, pending, ext, seq, filt)
        self.seq = 0              # scans issued
        self.has_in = self.has_rec = False      # the slot owns an input buffer / a record heap
        self.grow = 0             # reserve_grow calls so far
        self.doc = None           # (tab, inp, no, dkey) of the slot's document offsets, and how often they were set
        self.doc_gen = 0
        self.sel = self.seg = self.rp = self.rpd = None     # what each slot-owned output holds
        self.text = None
        self.shared = False
        self.cnt = None           # the slot-owned counts: dict(tab, gen, parts) -- their value is the sum of the parts' histograms
        self.cbuf = None          # the caller's count buffer of this slot: dict(tab, serial, base, parts); base: CNT_ENTRY is still in every entry
        # the line path (all tuples: a copy of the model shares them)
        self.up = None            # (tab, inp, n) of the bytes last uploaded into the slot's input buffer; None: unknown
        self.segc = None          # the key of the last segment whose doc_first went to the caller's buffer (still the caller's)
        self.dm = None            # (spec, own) of the slot's last matching / context call: Expectations.doc_ids(spec)
        self.ga = None            # (args of Expectations.gather, own_out, own_off) of the slot's last gather


PASSES = ("segment", "select", "select_docs", "replace", "replace_docs")
FETCH_OF = {"segment": "seg_fetch", "select": "sel_fetch", "select_docs": "docsel_fetch", "replace": "rp_fetch", "replace_docs": "rpd_fetch"}


class Model:
    """What include/pfac.h promises for a history of calls (never what pfac_hip.hip does): `apply(op)` moves the state and
    returns the Exp of the operation, `predict(op)` the same on a copy.  The state holds keys into the Expectations only.
    For the line path it also tracks the BYTES of each slot's input buffer -- those of the last upload and their length
    (`_Slot.up`).  A plan never asks a split or a gather of the slot's input for n_bytes beyond the last upload, or after
    a reserve_grow that replaced the input buffer: the header promises nothing about those bytes, and the model answers
    UNDEFINED (status None), which no plan may contain."""

    def __init__(self, exps=None):
        self.x = exps or expectations()
        self.tab = None
        self.knob = 0
        self.gen = 0
        self.flen = False
        self.reps = None
        self.cknob = 0            # the entry of CKNOBS the table was installed under
        self.fold = False         # the case fold of the scans to come: the uploaded table's setting (pfac_table_set_case_fold)
        self.pool = TABLES        # the tables and inputs a PLAN draws from (POOL for the fold family); the model itself asks nothing of it
        self.serial = 0           # caller's count buffers handed out
        self.slots = [_Slot() for _ in range(N_SLOTS)]

    def predict(self, op):
        return copy.deepcopy(self).apply(op)

    def apply(self, op):
        fn = getattr(self, "_op_" + op["op"], None) or getattr(self, "_" + op["op"])
        return fn(op, self.slots[op.get("slot", 0)])

    def __deepcopy__(self, memo):
        m = Model.__new__(Model)
        m.__dict__.update(self.__dict__)                        # (the cache is shared, not copied)
        m.slots = []
        for s in self.slots:
            c = _Slot()
            c.__dict__.update(s.__dict__)
            for name in ("scan", "sel", "seg", "rp", "rpd"):
                v = getattr(s, name)
                setattr(c, name, dict(v) if v is not None else None)
            for name in ("cnt", "cbuf"):
                v = getattr(s, name)
                setattr(c, name, dict(v, parts=list(v["parts"])) if v is not None else None)
            m.slots.append(c)
        return m

    # -- tables -------------------------------------------------------------
    def _load_table(self, op, s):
        """via: "host" = GpuMatcher.load_table, which turns the fold on behind the upload of a table built with
        ignore_case; "device" = load_table_device of the image without host_table -- pfac_table_upload_device and nothing
        else, which like every upload leaves the fold off."""
        self.tab, self.knob, self.cknob = op["tab"], op["knob"], op.get("cknob", 0)
        self.gen += 1
        self.flen, self.reps = False, None                      # lengths and replacements go with the old table
        self.fold = bool(POOL[op["tab"]].get("nocase")) and op.get("via", "host") == "host"      # ... and so does the fold
        return Exp()

    def _set_fold(self, op, s):
        """pfac_table_set_case_fold(mode): modes 0 and 1 through GpuMatcher.set_case_fold, anything else through the raw
        entry point."""
        if self.tab is None:
            return Exp(E_STATE)
        if op["mode"] not in (0, 1):
            return Exp(E_ARG)                                   # ... and the setting stays as it was
        self.fold = bool(op["mode"])
        return Exp()

    def _get_fold(self, op, s):
        if self.tab is None:
            return Exp(E_STATE)
        mode = int(self.fold)
        return Exp(OK, lambda: mode)

    def _set_flen(self, op, s):
        if self.tab is None:
            return Exp(E_STATE)
        self.flen = True
        return Exp()

    def _set_reps(self, op, s):
        if self.tab is None:
            return Exp(E_STATE)
        self.reps = op["rkey"]
        return Exp()

    # -- scans --------------------------------------------------------------
    def _new_scan(self, s, op, pending, ext, over=False):
        s.seq += 1
        s.scan = dict(tab=self.tab, knob=self.knob, gen=self.gen, inp=op["inp"], no=op["no"], over=over, pending=pending, ext=ext, seq=s.seq,
                      filt=(),                                  # (filt: the filters applied to it, Expectations.applied, sorted)
                      fold=self.fold)                           # (the mode at the moment it was queued: nothing later changes it)

    @staticmethod
    def _sk(sc):
        """The scan as the expectations take it: table, input, n_owned, filter state and fold."""
        return sc["tab"], sc["inp"], sc["no"], sc["filt"], sc["fold"]

    def _count(self, sc):
        return self.x.count(*self._sk(sc))

    def _rec_fn(self, sc, first=0, n=None):
        key = self._sk(sc)

        def fn():
            pos, ids, _ = self.x.scan(*key)
            return (pos[first:], ids[first:]) if n is None else (pos[first:first + n], ids[first:first + n])
        return fn

    def _uploaded(self, op, s):
        """A scan of a host buffer reserves the slot's input and uploads the WHOLE buffer before it asks for a table."""
        tab = self.tab or "abc2"
        s.up = (tab, op["inp"], self.x.input_size(tab, op["inp"]))

    def _scan_bytes(self, op, s):
        self._uploaded(op, s)
        s.has_in = s.has_rec = True                             # (scan_bytes reserves both before it scans)
        if self.tab is None:
            return Exp(E_STATE)
        self._new_scan(s, op, False, False)
        return Exp(OK, self._rec_fn(s.scan), tab=self.tab)

    def _scan_start(self, op, s):
        self._uploaded(op, s)
        s.has_in = s.has_rec = True
        if self.tab is None:
            return Exp(E_STATE)
        self._new_scan(s, op, True, False)
        return Exp()

    def _scan_finish(self, op, s):
        if s.scan is None:
            return Exp(E_STATE)
        s.scan["pending"] = False
        sc = s.scan
        n = self._count(sc)
        return Exp(OK, lambda: (n, sc["over"]))

    def _scan_ext(self, op, s):
        if self.tab is None:
            return Exp(E_STATE)
        n = self.x.count(self.tab, op["inp"], op["no"], (), self.fold)
        fit = n + n // 4 + 65536                                # the slack the header asks for, and more
        assert op["cap"] >= fit or op["cap"] < n, "a capacity the contract does not decide"
        self._new_scan(s, op, False, True, over=op["cap"] < n)
        sc = s.scan
        return Exp(OK, lambda: (n, sc["over"]))

    def _records(self, op, s):
        if op["n"] == 0:
            return Exp(OK, lambda: (np.empty(0, np.int64), np.empty(0, np.int64)), tab=self.tab)
        if s.scan is None or s.scan["pending"]:
            return Exp(E_STATE)
        sc = s.scan
        if op["first"] + op["n"] > self._count(sc):
            return Exp(E_ARG)
        if sc["over"]:
            return Exp(E_OVERFLOW)
        return Exp(OK, self._rec_fn(sc, op["first"], op["n"]), tab=sc["tab"])

    def _packed(self, op, s):
        if s.scan is None:
            return Exp(E_STATE)
        sc = s.scan
        if sc["pending"] or sc["over"]:
            return Exp(None)                                    # (the compact form of an unfinished or overflowed scan: no promise)
        if self.x.width(sc["tab"], sc["knob"]) == 8:
            return Exp(E_STATE)
        return Exp(OK, self._rec_fn(sc), tab=sc["tab"])

    def _checksum(self, op, s):
        if self.tab is None:
            return Exp(E_STATE)
        sc = s.scan
        if sc is not None and self._count(sc) == 0:
            return Exp(OK, lambda: 0)                           # (n = 0: the checksum of nothing, whatever the slot holds)
        if sc is None or sc["pending"] or sc["gen"] != self.gen:
            return Exp(E_STATE)
        if sc["over"]:
            return Exp(E_OVERFLOW)
        key = self._sk(sc)
        return Exp(OK, lambda: self.x.checksum(*key[:3], op["base"], key[3], key[4]))

    def _text(self, op, s):
        s.text = None
        if self.tab is None:
            return Exp(E_STATE)
        sc = s.scan
        if sc is None or sc["pending"] or sc["gen"] != self.gen:
            return Exp(E_STATE)
        if sc["over"]:
            return Exp(E_OVERFLOW)
        s.text = (sc["tab"], sc["inp"], sc["no"], op["base"], sc["filt"], sc["fold"])      # (the filter state at emission: a later filter leaves the text alone)
        key = s.text
        return Exp(OK, lambda: self.x.text(*key))

    def _text_fetch(self, op, s):
        if s.text is None:
            return Exp(None)
        key = s.text
        if op["first"] + op["n"] > len(self.x.text(*key)):
            return Exp(E_ARG)
        return Exp(OK, lambda: self.x.text(*key)[op["first"]:op["first"] + op["n"]])

    # -- documents ----------------------------------------------------------
    def _set_doc(self, op, s):
        s.doc = (op["tab"], op["inp"], op["no"], op["dkey"])
        s.doc_gen += 1
        return Exp()

    def _pass_state(self, s, overflow_status):
        """The checks every pass makes on the slot's last scan, in the header's order."""
        if s.scan is None or s.scan["pending"]:
            return E_STATE
        if not self.flen or s.scan["gen"] != self.gen:
            return E_STATE
        return overflow_status if s.scan["over"] else OK

    def _doc_state(self, s):
        if s.doc is None:
            return E_STATE
        return OK if offsets_ok(self.x.offsets(*s.doc), s.scan["no"]) else E_ARG

    def _doc_value_key(self, s):
        """Offsets that fit the scan: the plan makes them for (table, input, n_owned), and only those are keyed."""
        sc = s.scan
        if s.doc[:3] != (sc["tab"], sc["inp"], sc["no"]):
            return None
        return (sc["tab"], sc["inp"], sc["no"], s.doc[3], sc["filt"], sc["fold"])

    # -- the whole-word filter ------------------------------------------------
    def _filter(self, op, s):
        """pfac_records_filter_words with descriptor FILTERS[op["f"]]; op["heap"]: "own" = the heap the scan wrote (NULL
        for a slot-owned one), "none" / "slot" = NULL / the slot's own heap, which for a scan into a caller's heap is
        not the scan's.  The scan's state is judged before the arguments; among the arguments the header promises no
        order, so a heap that is not the scan's (PFAC_E_ARG) together with an n_docs that is not the slot's
        (PFAC_E_STATE) is undecided.  On any error the scan stays as it was."""
        d = FILTERS[op["f"]]
        sc = s.scan
        st = self._pass_state(s, E_OVERFLOW)
        bad_heap = sc is not None and sc["ext"] and op["heap"] != "own"
        if st:
            return Exp(st)
        arg = {E_ARG} if bad_heap else set()
        dkey = ""
        if d["doc"] != "none":
            if s.doc is None or d["doc"] == "wrong_n":
                arg.add(E_STATE)                                # (offsets that are not this n_docs' are not looked at)
            elif self.x.offsets(*s.doc).size == 1:
                pass                                            # (a split of nothing left no document: n_docs 0 is "no documents")
            elif not offsets_ok(self.x.offsets(*s.doc), sc["no"]):
                arg.add(E_ARG)
            elif s.doc[:3] != (sc["tab"], sc["inp"], sc["no"]):
                return Exp(None)                                # (another scan's offsets that happen to fit: not keyed)
            else:
                dkey = s.doc[3]
        if arg:
            return Exp(arg.pop() if len(arg) == 1 else None)
        filt = tuple(sorted(set(sc["filt"]) | {self.x.applied(sc["tab"], op["f"], dkey)}))
        if len(filt) > MAX_FILTERS:
            return Exp(None)                                    # (legal, but a plan stops at MAX_FILTERS)
        s.seq += 1                                              # a new record set: a selection made before is stale for both
        sc["seq"], sc["filt"] = s.seq, filt                     # replaces, as after a new scan; it stays fetchable
        n = self._count(sc)
        return Exp(OK, lambda: n)

    def _segment(self, op, s):
        s.seg = None
        st = self._pass_state(s, E_OVERFLOW) or self._doc_state(s)
        if st:
            return Exp(st)
        key = self._doc_value_key(s)
        if key is None:
            return Exp(None)
        n = int(self.x.seg(*key)[0][-1])
        if not op["own"] and op["small"]:
            return Exp(E_OVERFLOW if n > 0 else None, count=n)
        s.seg = dict(key=key, own=op["own"], tab=s.scan["tab"])
        if op["own"]:
            return Exp(OK, lambda: n)
        s.segc = key
        return Exp(OK, lambda: (n,) + self.x.seg(*key), tab=s.scan["tab"])

    def _seg_fetch(self, op, s):
        if s.seg is None or not s.seg["own"]:
            return Exp(E_STATE)
        key = s.seg["key"]
        return Exp(OK, lambda: self.x.seg(*key), tab=s.seg["tab"])

    # -- selection ----------------------------------------------------------
    def _select(self, op, s):
        s.sel = None
        st = self._pass_state(s, E_STATE)
        if st:
            return Exp(st)
        sc = s.scan
        if op["entry"] > self.x.M(sc["tab"]):
            return Exp(E_ARG)
        key = (sc["tab"], sc["inp"], sc["no"], op["entry"], sc["filt"], sc["fold"])
        n = int(self.x.sel(*key)[0].size)
        if not op["own"] and op["small"]:
            return Exp(E_OVERFLOW if n > 0 else None, count=n)
        s.sel = dict(kind="whole", key=key, own=op["own"], tab=sc["tab"], seq=sc["seq"], entry=op["entry"])
        if op["own"]:
            return Exp(OK, lambda: (n, self.x.sel(*key)[2]))
        return Exp(OK, lambda: (n, self.x.sel(*key)[2]) + self.x.sel(*key)[:2], tab=sc["tab"])

    def _ds(self, key, rkey=None):
        """Expectations.docsel of a per-document selection's key (table, input, n_owned, dkey, filter state, fold)."""
        return self.x.docsel(*key[:5], rkey, key[5])

    def _select_docs(self, op, s):
        s.sel = None
        st = self._pass_state(s, E_STATE) or self._doc_state(s)
        if st:
            return Exp(st)
        key = self._doc_value_key(s)
        if key is None:
            return Exp(None)
        n = int(self._ds(key)[0][-1])
        if not op["own"] and op["small"]:
            return Exp(E_OVERFLOW if n > 0 else None, count=n)
        s.sel = dict(kind="docs", key=key, own=op["own"], tab=s.scan["tab"], seq=s.scan["seq"], entry=0, doc_gen=s.doc_gen)
        if op["own"]:
            return Exp(OK, lambda: n)
        return Exp(OK, lambda: (n,) + self._ds(key)[:3], tab=s.scan["tab"])

    def _sel_fetch(self, op, s):
        if s.sel is None or not s.sel["own"]:
            return Exp(E_STATE)
        sel = s.sel
        if sel["kind"] == "whole":
            return Exp(OK, lambda: self.x.sel(*sel["key"])[:2], tab=sel["tab"])
        return Exp(OK, lambda: self._ds(sel["key"])[1:3], tab=sel["tab"])

    def _docsel_fetch(self, op, s):
        if s.sel is None or s.sel["kind"] != "docs" or not s.sel["own"]:
            return Exp(E_STATE)
        sel = s.sel
        return Exp(OK, lambda: self._ds(sel["key"])[:3], tab=sel["tab"])

    # -- replace ------------------------------------------------------------
    def _rp_state(self, s, docs, reps=True):
        if s.scan is None or s.sel is None or s.sel["seq"] != s.scan["seq"] or (docs and s.sel["kind"] != "docs"):
            return E_STATE
        if s.scan["gen"] != self.gen or (reps and self.reps is None) or not self.flen:
            return E_STATE
        if docs and s.sel["doc_gen"] != s.doc_gen:
            return E_STATE
        return OK

    def _rp_out(self, sel, rkey):
        if sel["kind"] == "whole":
            t, i, no, entry, f, fold = sel["key"]
            return lambda: self.x.replace(t, i, no, entry, rkey, f, fold)
        return lambda: self._ds(sel["key"], rkey)[4]

    def _replace(self, op, s, docs=False):
        s.rp = s.rpd = None
        st = self._rp_state(s, docs)
        if st:
            return Exp(st)
        sel, rkey = s.sel, self.reps
        out = self._rp_out(sel, rkey)
        n = int(out().size)
        if not op["own"] and op["small"]:
            return Exp(E_OVERFLOW if n > 0 else None, count=n)
        s.rp = dict(out=out, own=op["own"])
        if docs:
            off = lambda: self._ds(sel["key"], rkey)[3]                      # noqa: E731
            s.rpd = dict(off=off, own=op["own"])
            return Exp(OK, (lambda: n) if op["own"] else (lambda: (n, out(), off())))
        return Exp(OK, (lambda: n) if op["own"] else (lambda: (n, out())))

    def _replace_docs(self, op, s):
        return self._replace(op, s, docs=True)

    def _rp_fetch(self, op, s):
        if s.rp is None or not s.rp["own"]:
            return Exp(E_STATE)
        out = s.rp["out"]
        if op["first"] + op["n"] > out().size:
            return Exp(E_ARG)
        return Exp(OK, lambda: out()[op["first"]:op["first"] + op["n"]])

    def _rpd_fetch(self, op, s):
        if s.rpd is None or not s.rpd["own"]:
            return Exp(E_STATE)
        return Exp(OK, s.rpd["off"])

    # -- counts per pattern ---------------------------------------------------
    def _cbuf_for(self, op, s):
        """The caller's count buffer of the slot: exactly num_final x 8 bytes of the CURRENT table, so a fresh one
        (every entry CNT_ENTRY) whenever the table is not the one it was sized for -- before the call, refused or not."""
        if op["dst"] != "own" and (s.cbuf is None or s.cbuf["tab"] != self.tab):
            self.serial += 1
            s.cbuf = dict(tab=self.tab, serial=self.serial, base=True, parts=[])

    def _count_done(self, op, s, part, n):
        """The effects of a count that succeeded, and its value: n_counted, and for a caller's buffer its content."""
        if op["dst"] == "own":
            if op["acc"] and s.cnt is not None:
                s.cnt["parts"].append(part)
            else:
                s.cnt = dict(tab=part[1], gen=self.gen, parts=[part])
            return Exp(OK, lambda: n)
        if op["acc"]:
            s.cbuf["parts"].append(part)
        else:
            s.cbuf.update(base=False, parts=[part])
        tab, parts = part[1], list(s.cbuf["parts"])
        return Exp(OK, lambda: (n, self.x.sum_counts(tab, parts)), tab=tab)

    def _count_faults(self, op, s, faults):
        """The argument faults both count calls share, and what several faults are worth: the header promises no order
        among two argument faults, nor between one and the accumulate onto counts of an earlier table."""
        if op["dst"] == "misaligned":
            faults.append(E_ARG)
        if op["dst"] == "own" and op["acc"] and s.cnt is not None and s.cnt["gen"] != self.gen:
            faults.append(E_STATE)
        if len(faults) > 1:
            return Exp(None)
        return Exp(faults[0]) if faults else None

    def _op_count(self, op, s):
        """pfac_records_count_states.  dst: "own" = d_counts NULL, "caller" = the slot's caller's buffer ("misaligned":
        four bytes into it); acc: PFAC_COUNT_ACCUMULATE; heap as in _filter; ns: n_states = num_final ("ok"), one less,
        one more, or 0.  The scan's state is judged first: PFAC_E_STATE, PFAC_E_OVERFLOW, then the arguments."""
        self._cbuf_for(op, s)
        sc = s.scan
        if sc is None or sc["pending"] or sc["gen"] != self.gen:
            return Exp(E_STATE)
        if sc["over"]:
            return Exp(E_OVERFLOW)
        faults = []
        if sc["ext"] and op["heap"] != "own":
            if sc["no"] == 0:
                return Exp(None)                                # (a scan of nothing wrote no heap: no pointer is "another")
            faults.append(E_ARG)
        if op["ns"] != "ok":
            faults.append(E_ARG)
        bad = self._count_faults(op, s, faults)
        if bad is not None:
            return bad
        return self._count_done(op, s, ("scan",) + self._sk(sc), self._count(sc))

    def _op_count_sel(self, op, s):
        """pfac_selection_count_states.  sel: "own" = d_sel NULL, "caller" = the d_out the selection was given, "junk" =
        a buffer that holds no selection of this table, "misaligned".  The selection's state by the rules of the
        replace's d_sel (without the replacements), judged before the arguments; new document offsets do not make a
        per-document selection stale for a count."""
        self._cbuf_for(op, s)
        if self._rp_state(s, False, reps=False):
            return Exp(E_STATE)
        sel = s.sel
        if op["sel"] == "own" and not sel["own"]:
            return Exp(E_STATE)
        if op["sel"] == "caller" and sel["own"]:
            return Exp(None)                                    # (there is no caller's d_out to pass)
        part = (("sel",) if sel["kind"] == "whole" else ("docsel",)) + sel["key"]
        n = int(self.x.part_ids(part).size)
        faults = []
        if op["sel"] == "junk":
            if n == 0:
                return Exp(None)                                # (no picks: every buffer holds this selection)
            faults.append(E_ARG)
        if op["sel"] == "misaligned":
            faults.append(E_ARG)
        bad = self._count_faults(op, s, faults)
        if bad is not None:
            return bad
        return self._count_done(op, s, part, n)

    def _cnt_fetch(self, op, s):
        if s.cnt is None:
            return Exp(E_STATE)
        tab, parts = s.cnt["tab"], list(s.cnt["parts"])
        return Exp(OK, lambda: self.x.sum_counts(tab, parts), tab=tab)

    # -- lines: split, matching documents, gather -------------------------------
    # The model of the line path knows the BYTES of the slot's input buffer: those of the last upload (`up`: every scan
    # of a host buffer uploads the whole buffer), and their length.  A plan never asks a split or a gather of the slot's
    # input for n_bytes beyond that upload, or after a reserve_grow that replaced the input buffer: the header promises
    # nothing about those bytes, and the model answers UNDEFINED.  Among several broken rules the header promises no
    # order: an illegal operation breaks exactly one (two faults with different statuses are UNDEFINED).
    @staticmethod
    def _one(faults):
        return Exp(None) if len(faults) > 1 else Exp(next(iter(faults)))

    def _op_split(self, op, s):
        """pfac_slot_doc_offsets_split.  src: "slot" = d_input NULL, "caller" = a caller's copy of input (tab, inp), "odd" =
        four bytes into it; nb: n_bytes, or "over" = more than the slot's input buffer holds; delim: 0..255, or 256 / -1.
        Needs no table and no scan; on success the slot's offsets are the split's, as after set_doc.  Every error leaves
        the slot's offsets as they were."""
        faults = set()
        if not 0 <= op["delim"] <= 255:
            faults.add(E_ARG)
        if op["src"] == "odd":
            faults.add(E_ARG)
        if op["nb"] == "over":
            if op["src"] != "slot" or not s.has_in:
                return Exp(None)
            faults.add(E_ARG)
        elif op["src"] == "slot":
            if not s.has_in or s.up is None or s.up[:2] != (op["tab"], op["inp"]) or op["nb"] > s.up[2]:
                return Exp(None)
        elif op["nb"] > self.x.input_size(op["tab"], op["inp"]):
            return Exp(None)
        if faults:
            return self._one(faults)
        key = (op["tab"], op["inp"], op["nb"], op["delim"])
        s.doc = key[:3] + (f"split:{op['delim']}",)
        s.doc_gen += 1
        return Exp(OK, lambda: self.x.split(*key)[1:])

    def _doc_fetch(self, op, s):
        if s.doc is None:
            return Exp(E_STATE)
        doc = s.doc
        if op["first"] + op["n"] > self.x.offsets(*doc).size:
            return Exp(E_ARG)
        return Exp(OK, lambda: self.x.offsets(*doc)[op["first"]:op["first"] + op["n"]])

    def _first_of(self, op, s):
        """(src, key) of the doc_first a matching call is given, "none" where the slot holds none for NULL, or None where
        there is no such caller's buffer to pass."""
        if op["first"] == "own":
            return ("seg", s.seg["key"]) if s.seg is not None and s.seg["own"] else "none"
        if op["first"] == "seg":
            return ("seg", s.segc) if s.segc is not None else None
        sel = s.sel
        return ("docsel", sel["key"]) if sel is not None and sel["kind"] == "docs" and not sel["own"] else None

    def _op_matching(self, op, s, context=False):
        """pfac_documents_matching / _context.  first: "own" = d_doc_first NULL, "seg" / "docsel" = the caller's doc_first
        of an earlier segment / per-document selection; nd: n_docs of that doc_first ("ok") or one more; flags; out:
        "own" = d_ids_out NULL, "caller" = exactly *n_matching entries, "small" = one fewer, "odd" = misaligned.  The
        slot-owned ids are dropped at the start of either call, whatever it returns; nothing else drops them."""
        s.dm = None
        src = self._first_of(op, s)
        if src is None:
            return Exp(None)
        faults = set()
        if src == "none":
            faults.add(E_STATE)
        if op["nd"] != "ok":
            if op["first"] != "own" or src == "none":
                return Exp(None)                                # (a caller's doc_first of another length: nothing can tell)
            faults.add(E_ARG)
        if op["flags"] > 1 or (context and op["flags"]):
            faults.add(E_ARG)
        if op["out"] == "odd":
            faults.add(E_ARG)
        if faults:
            return Exp(None) if op["out"] == "small" else self._one(faults)
        spec = src + (("c", op["before"], op["after"]) if context else ("m", bool(op["flags"])))
        n = int(self.x.doc_ids(spec).size)
        if op["out"] == "small":
            return Exp(E_OVERFLOW if n > 0 else None, count=n)
        s.dm = (spec, op["out"] == "own")
        if op["out"] == "own":
            return Exp(OK, lambda: n)
        return Exp(OK, lambda: (n, self.x.doc_ids(spec)))

    def _op_context(self, op, s):
        return self._op_matching(op, s, context=True)

    def _ids_fetch(self, op, s):
        if s.dm is None or not s.dm[1]:
            return Exp(E_STATE)
        spec = s.dm[0]
        return Exp(OK, lambda: self.x.doc_ids(spec))

    def _op_gather(self, op, s):
        """pfac_documents_gather.  src / nb as in split (tab, inp: the caller's input); off: "slot" = d_doc_offsets NULL,
        "caller" = a caller's copy of the slot's offsets; nd: n_docs of the offsets or one more; ids: "own" = d_ids NULL,
        else a caller's list (Expectations.id_list); ni: n_ids of the list or one more; out / oo: d_out ("own", "caller" at
        exactly *out_bytes, "small", "odd") and d_out_offsets ("own", "caller").  The slot-owned outputs are dropped at the
        start of every gather."""
        s.ga = None
        x = self.x
        faults = set()
        if op["src"] == "slot":
            if not s.has_in or s.up is None or op["nb"] > s.up[2]:
                return Exp(None)
            t, i = s.up[:2]
        else:
            t, i = op["tab"], op["inp"]
            if op["nb"] > x.input_size(t, i):
                return Exp(None)
            if op["src"] == "odd":
                faults.add(E_ARG)
        doc = s.doc
        if doc is None:
            if op["off"] != "slot" or op["nd"] != "ok":
                return Exp(None)
            faults.add(E_STATE)
        elif op["nd"] != "ok":
            if op["off"] != "slot":
                return Exp(None)
            faults.add(E_STATE)
        spec = s.dm[0] if s.dm is not None else None
        if op["ids"] == "own":
            if s.dm is None or not s.dm[1]:
                faults.add(E_STATE)
                if op["ni"] != "ok":
                    return Exp(None)
            elif op["ni"] != "ok":
                faults.add(E_ARG)
        elif op["ni"] != "ok":
            return Exp(None)                                    # (a caller's list of another length: nothing can tell)
        if op["out"] == "odd":
            faults.add(E_ARG)
        known = doc is not None and not (op["ids"] == "own" and (s.dm is None or not s.dm[1]))
        if known:                                               # what the device checks: the ids, and the SELECTED documents
            off = x.offsets(*doc).astype(np.int64)
            ids = x.id_list(spec, op["ids"], int(off.size) - 1).astype(np.int64)
            good = ids < off.size - 1
            a, b = off[ids[good]], off[ids[good] + 1]
            if not good.all() or (a > b).any() or (b > op["nb"]).any():
                faults.add(E_ARG)
        if faults:
            return Exp(None) if op["out"] == "small" else self._one(faults)
        args = (t, i, op["nb"], doc, spec, op["ids"])
        n = int(x.gather(*args)[0].size)
        if op["out"] == "small":
            return Exp(E_OVERFLOW if n > 0 else None, count=n)
        own_out, own_off = op["out"] == "own", op["oo"] == "own"
        s.ga = (args, own_out, own_off)
        return Exp(OK, lambda: (n,) + (() if own_out else (x.gather(*args)[0],)) + (() if own_off else (x.gather(*args)[1],)))

    def _ga_fetch(self, op, s):
        if s.ga is None or not s.ga[1]:
            return Exp(E_STATE)
        args = s.ga[0]
        if op["first"] + op["n"] > self.x.gather(*args)[0].size:
            return Exp(E_ARG)
        return Exp(OK, lambda: self.x.gather(*args)[0][op["first"]:op["first"] + op["n"]])

    def _gaoff_fetch(self, op, s):
        if s.ga is None or not s.ga[2]:
            return Exp(E_STATE)
        args = s.ga[0]
        return Exp(OK, lambda: self.x.gather(*args)[1])

    # -- plumbing -----------------------------------------------------------
    def _set_stream(self, op, s):
        s.shared = op["share"]
        return Exp()

    def _sync(self, op, s):
        return Exp()

    def _reserve_grow(self, op, s):
        """A reserve above everything the slot holds: a buffer it already has is replaced, and the slot then has no
        finished scan."""
        s.grow = op["k"]
        grow_in, grow_rec = op["which"] in ("input", "both"), op["which"] in ("records", "both")
        if (grow_in and s.has_in) or (grow_rec and s.has_rec):
            s.scan = None
        if grow_in:
            s.up = None                                         # (a new input buffer: the header promises nothing about its bytes)
        s.has_in, s.has_rec = s.has_in or grow_in, s.has_rec or grow_rec
        return Exp()


# ---------------------------------------------------------------------------
# plans

def fmt(op):
    return op["op"] + "(" + ", ".join(f"{k}={v}" for k, v in op.items() if k != "op") + ")"


def _window(rng, total):
    """A [first, first + n) window of `total` items: all, a slice, or (now and then) one past the end."""
    r = rng.random()
    if r < 0.35 or total == 0:
        return (0, total) if r < 0.3 or total == 0 and r < 0.9 else (0, total + 1)
    if r < 0.9:
        first = int(rng.integers(0, total))
        return first, int(rng.integers(0, total - first + 1))
    return int(rng.integers(0, total + 1)), total + 1


KINDS = {"load_table": 4, "set_flen": 1, "set_reps": 2, "scan_bytes": 9, "scan_start": 5, "scan_finish": 2, "scan_ext": 6, "records": 7,
         "packed": 4, "checksum": 4, "text": 5, "text_fetch": 3, "set_doc": 4, "segment": 4, "select": 4, "select_docs": 4, "replace": 4,
         "replace_docs": 4, "seg_fetch": 3, "sel_fetch": 3, "docsel_fetch": 3, "rp_fetch": 3, "rpd_fetch": 3, "set_stream": 2, "sync": 1,
         "reserve_grow": 3}
WORD_KINDS = dict(KINDS, filter=9)      # the kinds of a plan with the whole-word filter (plan(seed, words=True))
COUNT_KINDS = dict(WORD_KINDS, scan_ext=10, count=9, count_sel=5, cnt_fetch=4)      # ... and of one with the counts as well (plan(seed, counts=True))
# ... and of one with the line path as well (plan(seed, lines=True))
LINE_KINDS = dict(COUNT_KINDS, sync=2, split=14, doc_fetch=8, matching=10, context=10, ids_fetch=5, gather=14, ga_fetch=7, gaoff_fetch=5)
# ... and of one with the case fold as well (plan(seed, fold=True))
FOLD_KINDS = dict(LINE_KINDS, load_table=6, scan_bytes=12, set_fold=7, get_fold=4)
FOLD_OPS = ("set_fold", "get_fold")
LINE_OPS = ("split", "doc_fetch", "matching", "context", "ids_fetch", "gather", "ga_fetch", "gaoff_fetch")
READERS = ("records", "packed", "checksum", "text", "scan_finish")          # what reads a finished scan, besides the passes


def _propose(rng, m, kinds=KINDS):
    """One candidate operation, drawn with an eye on the model's state (so most candidates have real data behind them)
    but never filtered by it: the caller asks the model what the candidate is worth."""
    x = m.x
    slot = int(rng.integers(0, N_SLOTS))
    s = m.slots[slot]
    sc = s.scan
    w = np.array(list(kinds.values()), dtype=float)
    kind = str(rng.choice(list(kinds), p=w / w.sum()))
    op = dict(op=kind, slot=slot)
    if kind == "load_table":
        op.pop("slot")
        op["tab"] = str(rng.choice(sorted(m.pool)))
        op["knob"] = int(rng.choice(POOL[op["tab"]]["knobs"]))
        if "count" in kinds:
            op["cknob"] = int(rng.integers(0, len(CKNOBS)))
        if "set_fold" in kinds and rng.random() < 0.3:
            op["via"] = "device"                                # (the image alone: pfac_table_upload_device, no host_table)
    elif kind == "set_fold":
        op.pop("slot")
        op["mode"] = int(rng.choice([0, 1, 2, 0xFFFFFFFF], p=[.4, .4, .1, .1]))
    elif kind == "get_fold":
        op.pop("slot")
    elif kind == "set_flen":
        op.pop("slot")
    elif kind == "set_reps":
        op.pop("slot")
        op["rkey"] = str(rng.choice(REP_KEYS))
    elif kind in ("scan_bytes", "scan_start", "scan_ext"):
        tab = m.tab or "abc2"
        op["inp"] = int(rng.integers(0, len(m.pool[tab]["inputs"])))
        if m.fold and "set_fold" in kinds:
            op["inp"] = _fold_input(rng, m, op["inp"])
        n = x.input_size(tab, op["inp"])
        op["no"] = n if rng.random() < 0.6 else (n * 5) // 8
        if kind != "scan_bytes":
            cnt = x.count(tab, op["inp"], op["no"], (), m.fold)
            op["cap"] = cnt // 2 if (kind == "scan_ext" and cnt >= 64 and rng.random() < 0.3) else cnt + cnt // 4 + 65536
    elif kind == "records":
        total = m._count(sc) if sc else 5
        op["first"], op["n"] = _window(rng, total)
    elif kind in ("checksum", "text"):
        op["base"] = int(rng.choice(TEXT_BASES))
    elif kind == "text_fetch":
        total = len(x.text(*s.text)) if s.text else 0
        op["first"], op["n"] = _window(rng, total)
    elif kind == "set_doc":
        if sc is None:
            return None
        op.update(tab=sc["tab"], inp=sc["inp"], no=sc["no"], dkey=str(rng.choice(DOC_KEYS, p=[.4, .4, .1, .1] if kinds is KINDS else [.3, .3, .2, .2])))
    elif kind in PASSES:
        op["own"] = bool(rng.random() < 0.6)
        op["small"] = bool(not op["own"] and rng.random() < 0.25)
        if kind == "select":
            M = x.M(sc["tab"]) if sc else 1
            op["entry"] = int(rng.choice([0, 0, 1, M, M + 1], p=[.3, .2, .2, .2, .1]))
    elif kind == "rp_fetch":
        total = int(s.rp["out"]().size) if s.rp else 3
        op["first"], op["n"] = _window(rng, total)
    elif kind == "filter":
        op["f"] = int(rng.integers(0, len(FILTERS)))
        op["heap"] = str(rng.choice(["none", "slot"])) if sc and sc["ext"] and rng.random() < 0.3 else "own"
    elif kind == "count":
        op.update(_count_op(slot, dst=str(rng.choice(["own", "caller", "misaligned"], p=[.5, .45, .05])), acc=bool(rng.random() < 0.4),
                            heap=str(rng.choice(["none", "slot"])) if sc and sc["ext"] and rng.random() < 0.3 else "own",
                            ns=str(rng.choice(["ok", "minus", "plus", "zero"], p=[.85, .05, .05, .05]))))
    elif kind == "count_sel":
        mine = ("own" if s.sel["own"] else "caller") if s.sel else "own"
        op.update(_count_sel_op(slot, dst=str(rng.choice(["own", "caller"])), acc=bool(rng.random() < 0.4),
                                sel=mine if rng.random() < 0.75 else str(rng.choice(["own", "junk", "misaligned"]))))
    elif kind == "split":
        op.update(_draw_split(rng, m, slot))
    elif kind == "doc_fetch":
        total = int(x.offsets(*s.doc).size) if s.doc else 2
        op["first"], op["n"] = _window(rng, total)
    elif kind in ("matching", "context"):
        op.update(_draw_matching(rng, m, slot, kind == "context"))
    elif kind == "gather":
        op.update(_draw_gather(rng, m, slot))
    elif kind == "ga_fetch":
        total = int(x.gather(*s.ga[0])[0].size) if s.ga else 3
        op["first"], op["n"] = _window(rng, total)
    elif kind == "set_stream":
        op["slot"] = 1
        op["share"] = not m.slots[1].shared
    elif kind == "reserve_grow":
        op["which"] = str(rng.choice(["input", "records", "both"]))
        op["k"] = s.grow + 1
    return op


def _fold_input(rng, m, inp):
    """The fold family, fold on: nine times in ten an input whose records the fold changes, where the table has one
    (so that the family's folded scans are mostly worth their name)."""
    good = [i for i in range(len(m.pool[m.tab]["inputs"])) if m.x.fold_differs(m.tab, i)]
    return int(rng.choice(good)) if good and rng.random() < 0.9 else inp


def _draw_split(rng, m, slot):
    """The arguments of a split on `slot`: mostly the slot's own input up to the scan's n_owned, at one of the input's
    three delimiters; now and then fewer bytes, none, a caller's copy, or one of the documented errors."""
    s = m.slots[slot]
    tab, inp = s.up[:2] if s.up else (m.tab or "abc2", 0)
    size = m.x.input_size(tab, inp)
    no = s.scan["no"] if s.scan and s.up and (s.scan["tab"], s.scan["inp"]) == (tab, inp) else size
    r = rng.random()
    nb = no if r < 0.65 else size if r < 0.75 else (no * 3) // 4 if r < 0.88 else 0
    op = dict(src="slot" if rng.random() < 0.7 else "caller", tab=tab, inp=inp, nb=nb,
              delim=int(rng.choice(m.x.delims(tab, inp), p=[.5, .3, .2])))
    r = rng.random()
    if r < 0.04:
        op["delim"] = int(rng.choice([256, -1]))
    elif r < 0.08:
        op.update(src="slot", nb="over")
    elif r < 0.12:
        op["src"] = "odd"
    return op


CONTEXTS = ((0, 0), (1, 0), (0, 1), (2, 3), (0, U64_MAX), (U64_MAX, U64_MAX), (1 << 33, 0), (5, 1 << 33))    # (2^33: more than any n_docs)


def _draw_matching(rng, m, slot, context):
    s = m.slots[slot]
    have = ["own"] * 3 + (["seg"] if s.segc else []) + (["docsel"] if s.sel and s.sel["kind"] == "docs" and not s.sel["own"] else [])
    op = dict(first=str(rng.choice(have)), nd="ok", flags=0 if context else int(rng.random() < 0.35),
              out=str(rng.choice(["own", "caller", "small", "odd"], p=[.55, .3, .1, .05])))
    if context:
        op["before"], op["after"] = CONTEXTS[int(rng.integers(0, len(CONTEXTS)))]
    r = rng.random()
    if r < 0.04:
        op["flags"] = 1 if context else 2
    elif r < 0.08:
        op["nd"] = "plus"
    return op


ID_FORMS = ("own", "same", "perm", "rev", "twice", "empty", "bad_id", "all")


def _draw_gather(rng, m, slot):
    s = m.slots[slot]
    tab, inp = s.up[:2] if s.up else (m.tab or "abc2", 0)
    if s.doc is not None and rng.random() < 0.85:                # mostly the input the offsets were made for
        tab, inp = s.doc[:2]
    size = m.x.input_size(tab, inp)
    nb = min(s.doc[2], size) if s.doc is not None and rng.random() < 0.85 else size
    mine = s.up is not None and s.up[:2] == (tab, inp)
    op = dict(src="slot" if mine and rng.random() < 0.7 else "caller", tab=tab, inp=inp, nb=nb, off=str(rng.choice(["slot", "caller"], p=[.7, .3])), nd="ok",
              ids=str(rng.choice(ID_FORMS, p=[.4, .1, .1, .1, .1, .07, .08, .05])), ni="ok",
              out=str(rng.choice(["own", "caller", "small", "odd"], p=[.55, .3, .1, .05])), oo=str(rng.choice(["own", "caller"], p=[.6, .4])))
    r = rng.random()
    if r < 0.04:
        op["nd"] = "plus"
    elif r < 0.08:
        op["ni"] = "plus"
    elif r < 0.12:
        op["src"] = "odd"
    elif r < 0.16 and nb > 0:
        op["nb"] = nb - 1                                       # the last document then passes n_bytes: PFAC_E_ARG if it is selected
    return op


def _matching_op(slot, first="own", out="own", flags=0, context=None):
    op = dict(op="context" if context else "matching", slot=slot, first=first, nd="ok", flags=flags, out=out)
    if context:
        op["before"], op["after"] = context
    return op


def _gather_op(slot, m, **kw):
    """A gather of the slot's own input, offsets and ids into slot-owned outputs, up to the end of the offsets."""
    s = m.slots[slot]
    if s.up is None or s.doc is None:
        return None
    op = dict(op="gather", slot=slot, src="slot", tab=s.up[0], inp=s.up[1], nb=min(s.doc[2], s.up[2]), off="slot", nd="ok", ids="own", ni="ok",
              out="own", oo="own")
    op.update(kw)
    return op


def _split_step(rng, slot, part=1.0):
    """A split of the slot's own input up to the scan's n_owned (`part`: up to that part of it), at a delimiter drawn now."""
    which = int(rng.choice(3, p=[.5, .3, .2]))

    def step(m):
        s = m.slots[slot]
        if s.up is None or s.scan is None or (s.scan["tab"], s.scan["inp"]) != s.up[:2]:
            return None
        return dict(op="split", slot=slot, src="slot", tab=s.up[0], inp=s.up[1], nb=int(s.scan["no"] * part), delim=m.x.delims(*s.up[:2])[which])
    return step


def _line_prepare(rng, slot, upto):
    """What a session does so that `upto` ("segment", "matching" or "gather") has something to work on: a scan of a host
    buffer, offsets for it (a split, or set_doc), the segment into the slot's buffers, a matching call."""
    use_split = rng.random() < 0.7

    def offsets(m):
        s = m.slots[slot]
        sc = s.scan
        if sc is None or sc["ext"] and use_split:
            return None
        if s.doc is not None and s.doc[:3] == (sc["tab"], sc["inp"], sc["no"]) and not s.doc[3].startswith("bad"):
            return None
        if use_split and s.up is not None and s.up[:2] == (sc["tab"], sc["inp"]):
            return _split_step(rng, slot)(m)
        return dict(op="set_doc", slot=slot, tab=sc["tab"], inp=sc["inp"], no=sc["no"], dkey=str(rng.choice(DOC_KEYS[:2])))

    def segment(m):
        s = m.slots[slot]
        if s.seg is None or not s.seg["own"] or s.doc is None or s.seg["key"][:4] != s.doc:
            return _pass_op("segment", slot)

    def ids(m):
        if m.slots[slot].dm is None or not m.slots[slot].dm[1]:
            return _matching_op(slot, flags=int(rng.random() < 0.3))

    steps = _prepare(rng, "select", slot) + [offsets]
    if upto in ("matching", "gather"):
        steps.append(segment)
    if upto == "gather":
        steps.append(ids)
    return steps


# what may come between a producer of the line path and the late fetch of its result (the reach test wants every pair)
BETWEEN = ("split", "set_doc", "segment", "matching", "context", "gather", "scan", "upload", "grow", "filter")
LATE = {"split": ("doc_fetch",), "set_doc": ("doc_fetch",), "matching": ("ids_fetch",), "context": ("ids_fetch",), "gather": ("ga_fetch", "gaoff_fetch")}


def _between_steps(rng, slot, what, pool=TABLES):
    """One intervening call `what` on `slot`, meant to succeed."""
    if what == "split":
        return [_split_step(rng, slot)]
    if what == "set_doc":
        return [lambda m: dict(op="set_doc", slot=slot, tab=m.slots[slot].scan["tab"], inp=m.slots[slot].scan["inp"], no=m.slots[slot].scan["no"],
                               dkey=str(DOC_KEYS[int(rng.integers(0, 2))])) if m.slots[slot].scan else None]
    if what == "segment":
        return _line_prepare(rng, slot, "segment") + [_pass_op("segment", slot, own=bool(rng.random() < 0.7))]
    if what in ("matching", "context"):
        ctx = CONTEXTS[int(rng.integers(0, len(CONTEXTS)))] if what == "context" else None
        return _line_prepare(rng, slot, "matching") + [_matching_op(slot, out=str(rng.choice(["own", "caller"])), context=ctx)]
    if what == "gather":
        return _line_prepare(rng, slot, "gather") + [lambda m: _gather_op(slot, m)]
    if what == "scan":
        return [_scan_step(rng, slot, other=True)]
    if what == "upload":
        tab = str(rng.choice(sorted(pool)))
        return [dict(op="load_table", tab=tab, knob=int(rng.choice(POOL[tab]["knobs"])), cknob=int(rng.integers(0, len(CKNOBS))))]
    if what == "grow":
        which = str(rng.choice(["records", "input", "both"]))
        return [lambda m: dict(op="reserve_grow", slot=slot, which=which, k=m.slots[slot].grow + 1)]
    assert what == "filter"
    return _prepare(rng, "filter", slot) + [_filter_step(rng, slot)]


def _late_fetch(rng, slot, kind, beyond=False):
    """The fetch of a slot-owned result: all of it from a place drawn now (`beyond`: one entry more than there is)."""
    at = rng.random()

    def step(m):
        s = m.slots[slot]
        if kind in ("doc_fetch", "ga_fetch"):
            total = (int(m.x.offsets(*s.doc).size) if s.doc else 0) if kind == "doc_fetch" else (int(m.x.gather(*s.ga[0])[0].size) if s.ga else 0)
            first = int(at * total) if at < 0.7 else 0
            return dict(op=kind, slot=slot, first=first, n=total - first + beyond)
        return dict(op=kind, slot=slot)
    return step


class _Quiet:
    """An agenda step whose operation the line agenda does not follow up: what comes between a producer and its late
    fetch must not make the producer's pass run again."""

    def __init__(self, step):
        self.step = step


# the refused variants of a call that has just succeeded (one broken rule each), tried right behind it
REFUSED = {"split": (dict(delim=256), dict(delim=-1), dict(src="slot", nb="over"), dict(src="odd")),
           "matching": (dict(out="small"), dict(flags=2), dict(nd="plus"), dict(out="odd")),
           "context": (dict(out="small"), dict(flags=1), dict(nd="plus"), dict(out="odd")),
           "gather": (dict(out="small"), dict(nd="plus"), dict(ni="plus"), dict(src="odd"), dict(out="odd"), dict(ids="bad_id"), dict(nb=-1))}


def _next(turn, key):
    """The next value of the plan's counter `key` (it starts at five times the seed: every plan elsewhere in a cycle of 2,
    3, 4, 7, 8, 9 or 32)."""
    turn[key] = turn.get(key, turn["seed"] * 5 + len(key)) + 1
    return turn[key] - 1


def _refused(chosen, turn):
    err = dict(REFUSED[chosen["op"]][_next(turn, "refused " + chosen["op"]) % len(REFUSED[chosen["op"]])])
    if err.get("nb") == -1:
        err["nb"] = max(chosen["nb"] - 1, 0)
    if "nd" in err and chosen["op"] == "gather":
        err["off"] = "slot"                                     # (only the slot's offsets have an n_docs of their own)
    if "ni" in err:
        err["ids"] = "own"                                      # (... and only the slot's ids a count)
    return dict(chosen, **err)


def _line_agenda(rng, m, chosen, st, agenda, turn):
    """The histories the line family aims at (the rules of plan(seed, lines=True)); returns the new agenda.  `turn`
    holds counters that walk BETWEEN, the 32 combinations of NULL and caller's arguments of the gather, and
    REFUSED, so that every (producer, intervening call, late fetch) order, every combination and every refusal comes up
    in the suite's plans and not only the likely ones."""
    kind, slot = chosen["op"], chosen.get("slot", 0)
    s = m.slots[slot]
    if st != OK:
        return agenda
    fetches = [f for f in LATE.get(kind, ()) if kind in ("split", "set_doc") or chosen["oo" if f == "gaoff_fetch" else "out"] == "own"]
    follow = []
    if kind in ("matching", "context"):
        # the ids are there to be gathered: every combination of NULL and caller's arguments in turn
        for c in (_next(turn, "combination"), _next(turn, "combination")):
            form = "own" if chosen["out"] == "own" and c & 4 else str(rng.choice(("same", "perm", "rev", "twice", "empty", "all")))
            follow.append(lambda m, c=c, form=form: _gather_op(slot, m, src="slot" if c & 1 else "caller", off="slot" if c & 2 else "caller", ids=form,
                                                               out="own" if c & 8 else "caller", oo="own" if c & 16 else "caller"))
    if kind == "split" and chosen["nb"] != "over" and s.scan is not None and chosen["nb"] != s.scan["no"]:
        # offsets that do not end at the scan's n_owned: the document passes and the filter answer PFAC_E_ARG
        what = ("segment", "select_docs", "filter")[_next(turn, "other bytes") % 3]
        follow = [lambda m: None if m.flen else dict(op="set_flen"),
                  dict(op="filter", slot=slot, f=int(rng.integers(5, 10)), heap="own") if what == "filter" else _pass_op(what, slot)]
    if fetches and len(agenda) < 40 and rng.random() < 0.95:
        # a producer, one or two other calls, then the late fetch
        between = [b for b in BETWEEN if b not in {"split": ("split", "set_doc"), "set_doc": ("split", "set_doc"), "matching": ("matching", "context"),
                                                    "context": ("matching", "context"), "gather": ("gather",)}[kind]]
        steps = _between_steps(rng, slot, between[_next(turn, "between " + kind) % len(between)], m.pool)
        if rng.random() < 0.25:
            steps += _between_steps(rng, slot, str(rng.choice([b for b in between if b not in ("grow", "upload")])), m.pool)
        if kind == "gather" and fetches == list(LATE[kind]) and rng.random() < 0.35:
            # a larger gather first: the slot-owned outputs regrow while nothing has fetched the first
            steps = [lambda m: _gather_op(slot, m, ids="twice", src="caller"), _late_fetch(rng, slot, "ga_fetch")] + steps
        steps = [_Quiet(step) for step in steps]
        late = [_late_fetch(rng, slot, f) for f in fetches]
        if fetches[0] != "ids_fetch" and rng.random() < 0.25:
            late = [_late_fetch(rng, slot, fetches[0], beyond=True)] + late
        again = [_refused(chosen, turn)] if kind in REFUSED and rng.random() < 0.4 else []    # (refused once nothing needs the result any more)
        if kind == "gather" and chosen["src"] == "slot" and rng.random() < 0.3:
            # the slot's input is what was uploaded last, whatever the slot has scanned since: a scan of a caller's buffer, the gather again
            again = [_Quiet(_ext_step(rng, slot)), _Quiet(dict(chosen)), _Quiet(_late_fetch(rng, slot, fetches[0]))] + again
        return (follow + steps + late if kind == "split" else steps + late + follow) + again + agenda
    if kind in REFUSED and rng.random() < 0.5:
        agenda = [_refused(chosen, turn)] + agenda
    if kind == "segment" and chosen["own"] and rng.random() < 0.4:
        # segment, filter, segment, matching: the ids are those of the filtered scan's doc_first -- not of the unfiltered
        # one, and not of a per-document selection made before the filter
        before = [_pass_op("select_docs", slot, own=bool(rng.random() < 0.5))] if rng.random() < 0.5 else []
        agenda = before + [_filter_step(rng, slot), _pass_op("segment", slot), _matching_op(slot, flags=int(rng.random() < 0.3)),
                           dict(op="ids_fetch", slot=slot)] + agenda
    elif kind == "segment" and chosen["own"] and rng.random() < 0.25:
        # the doc_first of a per-document selection in the caller's buffer gives the same ids
        ctx = CONTEXTS[int(rng.integers(0, len(CONTEXTS)))] if rng.random() < 0.4 else None
        agenda = [_pass_op("select_docs", slot, own=False), _matching_op(slot, first="docsel", out=str(rng.choice(["own", "caller"])), context=ctx)] + agenda
    elif kind == "segment" and chosen["own"] and rng.random() < 0.25:
        agenda = [_pass_op("segment", slot, own=False)] + agenda  # the same again into the caller's buffers
    elif kind == "segment" and chosen["own"]:
        ctx = CONTEXTS[int(rng.integers(0, len(CONTEXTS)))] if rng.random() < 0.65 else None
        agenda = [_matching_op(slot, out=str(rng.choice(["own", "caller"], p=[.85, .15])), flags=int(ctx is None and rng.random() < 0.3), context=ctx)] + agenda
    elif kind == "segment" and not chosen["own"]:
        # the segment went to the caller's buffers: NULL is refused, the caller's doc_first is not
        ctx = CONTEXTS[int(rng.integers(0, len(CONTEXTS)))] if _next(turn, "caller's segment") % 2 else None
        agenda = [_matching_op(slot, context=ctx), _matching_op(slot, first="seg", out=str(rng.choice(["own", "caller"])), context=ctx)] + agenda
    elif kind == "select_docs" and not chosen["own"] and rng.random() < 0.7:
        agenda = [_matching_op(slot, first="docsel", context=CONTEXTS[int(rng.integers(0, len(CONTEXTS)))] if rng.random() < 0.5 else None)] + agenda
    elif follow:
        agenda = follow + agenda
    elif kind == "scan_bytes" and rng.random() < 0.08:
        # the split needs no finished scan: it runs while the next one is pending
        agenda = [_ext_step(rng, slot, start=True), _split_step(rng, slot), dict(op="scan_finish", slot=slot)] + agenda
    elif kind in ("scan_bytes", "scan_finish") and s.scan is not None and rng.random() < 0.25:
        agenda = [_split_step(rng, slot, part=float(rng.choice([0.75, 0.0])))] + agenda      # a split of fewer bytes than the scan owns, or of none
    elif kind in ("scan_bytes", "scan_finish") and s.scan is not None and rng.random() < 0.3:
        agenda = _line_prepare(rng, slot, "matching") + agenda
    elif kind in ("scan_bytes", "scan_finish") and s.scan is not None and rng.random() < 0.5:
        agenda = _line_prepare(rng, slot, "gather") + [lambda m: _gather_op(slot, m)] + agenda
    elif kind == "set_doc" and chosen["dkey"].startswith("bad") and rng.random() < 0.7:
        # offsets that break the rules: refused once a document that breaks them is selected
        agenda = [lambda m: _gather_op(slot, m, ids="all", nb=m.slots[slot].up[2] if m.slots[slot].up else 0)] + agenda
    elif kind == "scan_start" and rng.random() < 0.5:
        agenda = [_split_step(rng, slot)] + agenda              # a split while the scan is pending
    if kind == "select_docs" and rng.random() < 0.3:
        # a split makes the per-document selection stale for replace_docs with NULL offsets
        agenda = [_split_step(rng, slot), _pass_op("replace_docs", slot)] + agenda
    return agenda


def _pass_op(kind, slot, own=True):
    op = dict(op=kind, slot=slot, own=own, small=False)
    if kind == "select":
        op["entry"] = 0
    return op


def _count_op(slot, dst="own", acc=False, heap="own", ns="ok"):
    return dict(op="count", slot=slot, dst=dst, acc=acc, heap=heap, ns=ns)


def _count_sel_op(slot, dst="own", acc=False, sel="own"):
    return dict(op="count_sel", slot=slot, dst=dst, acc=acc, sel=sel)


PRODUCER_OF = {v: k for k, v in FETCH_OF.items()}


def _prepare(rng, kind, slot, docs=False):
    """What a session does before pass `kind` on `slot` (or before a filter, with `docs` when it reads the slot's
    offsets) so that it has something to work on: steps that look at the model when their turn comes and return an
    operation, or None when nothing is missing."""
    def table(m):
        if m.tab is None:
            tab = str(rng.choice(sorted(m.pool)))
            return dict(op="load_table", tab=tab, knob=int(rng.choice(POOL[tab]["knobs"])))

    def scan(m):
        sc = m.slots[slot].scan
        if sc is not None and sc["pending"]:
            return dict(op="scan_finish", slot=slot)
        if sc is None or sc["over"] or sc["gen"] != m.gen:
            inp = int(rng.integers(0, len(m.pool[m.tab]["inputs"])))
            if m.fold and m.pool is POOL:
                inp = _fold_input(rng, m, inp)
            n = m.x.input_size(m.tab, inp)
            return dict(op="scan_bytes", slot=slot, inp=inp, no=n if rng.random() < 0.6 else (n * 5) // 8)

    def doc(m):
        s = m.slots[slot]
        sc = s.scan
        if sc is not None and (s.doc is None or s.doc[:3] != (sc["tab"], sc["inp"], sc["no"]) or s.doc[3].startswith("bad")):
            return dict(op="set_doc", slot=slot, tab=sc["tab"], inp=sc["inp"], no=sc["no"], dkey=str(rng.choice(DOC_KEYS[:2])))

    def sel(m):
        s = m.slots[slot]
        want = "docs" if kind == "replace_docs" else None
        if s.scan is None or s.sel is None or s.sel["seq"] != s.scan["seq"] or (want and (s.sel["kind"] != want or s.sel["doc_gen"] != s.doc_gen)):
            return _pass_op("select_docs" if want or rng.random() < 0.3 else "select", slot, own=bool(rng.random() < 0.7))

    steps = [table, lambda m: None if m.flen else dict(op="set_flen")]
    if kind in ("replace", "replace_docs"):
        steps.append(lambda m: None if m.reps else dict(op="set_reps", rkey=str(rng.choice(REP_KEYS))))
    steps.append(scan)
    if kind in ("segment", "select_docs", "replace_docs", "replace") or docs:
        steps.append(doc)
    if kind in ("replace", "replace_docs"):
        steps.append(sel)
    return steps


def _after_filter(rng, slot):
    """What a session does with a filtered scan: a reader of the scan, or a pass and the fetch of its result."""
    what = str(rng.choice(READERS + PASSES))
    if what in PASSES:
        fetch = dict(op=FETCH_OF[what], slot=slot, **({"first": 0, "n": 1} if what == "replace" else {}))
        return _prepare(rng, what, slot) + [_pass_op(what, slot), fetch]
    if what == "records":
        return [lambda m: dict(op="records", slot=slot, first=0, n=m._count(m.slots[slot].scan)) if m.slots[slot].scan else None]
    if what in ("checksum", "text"):
        return [dict(op=what, slot=slot, base=int(rng.choice(TEXT_BASES)))]
    return [dict(op=what, slot=slot)]


def _filter_step(rng, slot):
    """A filter the session means to succeed: a descriptor drawn now; when its turn comes and the slot's offsets do
    not allow it, one without documents instead."""
    first, second = int(rng.integers(0, len(FILTERS))), int(rng.integers(0, 5))
    assert all(FILTERS[k]["doc"] == ("none" if k < 5 else "slot") for k in range(10))

    def step(m):
        op = dict(op="filter", slot=slot, f=first, heap="own")
        return op if m.predict(op).status == OK else dict(op, f=second)
    return step


def _scan_step(rng, slot, other=False):
    """A scan of the current table the session means to succeed (`other`: of another input than the slot's last)."""
    def step(m):
        if m.tab is None:
            return None
        n_in = len(m.pool[m.tab]["inputs"])
        inp = int(rng.integers(0, n_in))
        sc = m.slots[slot].scan
        if m.fold and m.pool is POOL:
            inp = _fold_input(rng, m, inp)
        if other and sc is not None and sc["inp"] == inp:
            inp = (inp + 1) % n_in
        n = m.x.input_size(m.tab, inp)
        return dict(op="scan_bytes", slot=slot, inp=inp, no=n if rng.random() < 0.6 else (n * 5) // 8)
    return step


def _ext_step(rng, slot, start=False):
    """A scan of the current table into a caller's heap: one that fits, or (two times in five) one half the size.
    `start`: a scan_start into the slot's own heap instead, which fits."""
    def step(m):
        if m.tab is None:
            return None
        inp = int(rng.integers(0, len(m.pool[m.tab]["inputs"])))
        if m.fold and m.pool is POOL:
            inp = _fold_input(rng, m, inp)
        no = m.x.input_size(m.tab, inp)
        cnt = m.x.count(m.tab, inp, no, (), m.fold)
        if start:
            return dict(op="scan_start", slot=slot, inp=inp, no=no, cap=cnt + cnt // 4 + 65536)
        return dict(op="scan_ext", slot=slot, inp=inp, no=no, cap=cnt // 2 if cnt >= 64 and rng.random() < 0.4 else cnt + cnt // 4 + 65536)
    return step


def _between_count_and_fetch(rng, slot, pool=TABLES):
    """What happens between a count into the slot-owned buffer and the fetch of it: the counts outlive all of it."""
    what = str(rng.choice(["scan", "upload", "grow", "filter", "pass", "caller", "refused"]))
    if what == "scan":
        return [_scan_step(rng, slot, other=True)]
    if what == "upload":
        tab = str(rng.choice(sorted(pool)))
        return [dict(op="load_table", tab=tab, knob=int(rng.choice(POOL[tab]["knobs"])), cknob=int(rng.integers(0, len(CKNOBS))))]
    if what == "grow":
        which = str(rng.choice(["records", "both"]))
        return [lambda m: dict(op="reserve_grow", slot=slot, which=which, k=m.slots[slot].grow + 1)]
    if what == "filter":
        return _prepare(rng, "filter", slot) + [_filter_step(rng, slot)]
    if what == "pass":
        kind = str(rng.choice(PASSES))
        return _prepare(rng, kind, slot) + [_pass_op(kind, slot)]
    if what == "caller":
        return [_count_op(slot, dst="caller", acc=bool(rng.random() < 0.5))]
    return [_count_op(slot, ns=str(rng.choice(["minus", "plus", "zero"])))]


def _count_agenda(rng, m, chosen, st, agenda):
    """The histories the count family aims at (the rules of plan(seed, counts=True)); returns the new agenda."""
    if st != OK:
        return agenda
    kind, slot = chosen["op"], chosen.get("slot", 0)
    sc = m.slots[slot].scan
    dst = lambda: str(rng.choice(["own", "caller"]))            # noqa: E731
    fetch = dict(op="cnt_fetch", slot=slot)
    if kind in ("scan_bytes", "scan_finish") and rng.random() < 0.5:
        # a fresh scan is counted, then read by something else
        reader = str(rng.choice(["checksum", "text", "records"]))
        read = (lambda m: dict(op="records", slot=slot, first=0, n=m._count(m.slots[slot].scan)) if m.slots[slot].scan else None) \
            if reader == "records" else dict(op=reader, slot=slot, base=int(rng.choice(TEXT_BASES)))
        odd = []
        if rng.random() < 0.3:                                  # a refused call first: a misaligned d_counts, a wrong n_states
            what = str(rng.choice(["misaligned", "minus", "plus", "zero"]))
            odd = [_count_op(slot, dst="misaligned") if what == "misaligned" else _count_op(slot, dst=dst(), acc=bool(rng.random() < 0.5), ns=what)]
        agenda = odd + [_count_op(slot, dst=dst(), acc=bool(rng.random() < 0.3)), read] + agenda
    elif kind in ("checksum", "text", "records") and sc is not None and not sc["ext"] and rng.random() < 0.3:
        agenda = [_ext_step(rng, slot)] + agenda                # the next scan goes to a caller's heap
    elif kind in ("checksum", "text", "records") and sc is not None and rng.random() < 0.2:
        # the next scan is counted while it is pending (PFAC_E_STATE), and by the other slot's rules once it has finished
        agenda = [_ext_step(rng, slot, start=True), _count_op(slot, dst=dst(), acc=bool(rng.random() < 0.5))] + agenda
    elif kind == "scan_start" and rng.random() < 0.5:
        agenda = [_count_op(slot, dst=dst())] + agenda          # a scan that is not finished: PFAC_E_STATE
    elif kind == "reserve_grow" and sc is None and rng.random() < 0.6:
        agenda = [_count_op(slot, dst=dst())] + agenda          # a reserve that dropped the scan: PFAC_E_STATE
    elif kind == "scan_ext":
        # a caller's heap: the right pointer, now and then a wrong one first; an overflowed one is PFAC_E_OVERFLOW
        wrong = [_count_op(slot, dst=dst(), heap=str(rng.choice(["none", "slot"])))] if not sc["over"] and rng.random() < 0.4 else []
        agenda = wrong + [_count_op(slot, dst=dst(), acc=bool(rng.random() < 0.3))] + agenda
    elif kind == "filter" and rng.random() < 0.6:
        agenda = [_count_op(slot, dst=dst(), acc=bool(rng.random() < 0.4))] + agenda
    elif kind in ("select", "select_docs") and rng.random() < 0.12:
        # a selection made with an earlier table: PFAC_E_STATE
        tab = str(rng.choice(sorted(m.pool)))
        agenda = [dict(op="load_table", tab=tab, knob=int(rng.choice(POOL[tab]["knobs"])), cknob=int(rng.integers(0, len(CKNOBS)))),
                  _count_sel_op(slot, dst=dst(), sel="own" if chosen["own"] else "caller")] + agenda
    elif kind in ("select", "select_docs") and rng.random() < 0.7:
        # NULL for a selection in the caller's d_out, a buffer that holds none, a misaligned one: refused, then the count
        null = [_count_sel_op(slot, dst=dst(), sel="own")] if not chosen["own"] and rng.random() < 0.4 else []
        bad = [_count_sel_op(slot, dst=dst(), acc=bool(rng.random() < 0.5), sel=str(rng.choice(["junk", "misaligned"])))] if rng.random() < 0.3 else []
        agenda = null + bad + [_count_sel_op(slot, dst=dst(), acc=bool(rng.random() < 0.4), sel="own" if chosen["own"] else "caller")] + agenda
    elif kind == "load_table" and rng.random() < 0.5:
        # an accumulate onto the slot's counts of the table before is PFAC_E_STATE; a plain count replaces them
        slot = int(rng.integers(0, N_SLOTS))
        agenda = [_scan_step(rng, slot), _count_op(slot, acc=True), _count_op(slot), dict(op="cnt_fetch", slot=slot)] + agenda
    elif kind in ("count", "count_sel") and chosen["dst"] == "own" and not chosen["acc"] and rng.random() < 0.3:
        # two or three accumulating counts over different scans of one table, then the fetch
        more = []
        for _ in range(int(rng.integers(2, 4))):
            more += [_scan_step(rng, slot, other=True), _count_op(slot, acc=True)]
        if rng.random() < 0.5:
            more += _prepare(rng, "select", slot)[1:] + [_pass_op("select", slot), _count_sel_op(slot, acc=True)]
        agenda = more + [fetch] + agenda
    elif kind in ("count", "count_sel") and chosen["dst"] == "own" and rng.random() < 0.7:
        agenda = agenda + _between_count_and_fetch(rng, slot, m.pool) + [fetch]
    if kind == "count_sel" and rng.random() < 0.25:
        # a new scan or a filter makes the selection stale: the same count again is PFAC_E_STATE
        agenda = [_scan_step(rng, slot) if rng.random() < 0.5 else _filter_step(rng, slot), dict(chosen, acc=bool(rng.random() < 0.5))] + agenda
    return agenda


def _fold_agenda(rng, m, chosen, st, agenda):
    """The histories the fold family aims at (the rules of plan(seed, fold=True)); returns the new agenda."""
    if st != OK:
        return agenda
    kind, slot = chosen["op"], chosen.get("slot", 0)
    sc = m.slots[slot].scan
    toggle = lambda m: dict(op="set_fold", mode=int(not m.fold))        # noqa: E731

    def scan_unless_pending(slot):
        step = _scan_step(rng, slot)
        return lambda m: None if m.slots[slot].scan is not None and m.slots[slot].scan["pending"] else step(m)

    if kind == "load_table":
        if m.fold and rng.random() < 0.8:
            # the upload of a nocase table through load_table left the fold on: a scan before anything toggles
            agenda = [_scan_step(rng, int(rng.integers(0, N_SLOTS)))] + agenda
        elif not m.fold and rng.random() < 0.8:
            # a table whose fold is off after its upload (an old table, or an image through load_table_device): on, by hand
            agenda = [dict(op="get_fold"), dict(op="set_fold", mode=1)] + agenda
    elif kind == "scan_start" and rng.random() < 0.8:
        agenda = [toggle] + agenda                              # the toggle comes while this scan is pending: it keeps its mode
    elif kind == "set_fold" and rng.random() < 0.75:
        # the new mode applies to the scans queued from now on, on EVERY slot
        first = int(rng.integers(0, N_SLOTS))
        agenda = [scan_unless_pending(first), scan_unless_pending(1 - first)] + agenda
    elif kind in ("scan_bytes", "scan_finish", "scan_ext") and sc is not None and (sc["fold"] or POOL[sc["tab"]].get("nocase")) and not sc["over"] \
            and not sc["pending"] and m._count(sc) >= 16 and rng.random() < 0.5:
        # a folded scan with something to drop (or the exact scan of a table whose fold is otherwise on): the filter judges the ORIGINAL bytes (the word set `tab` of a nocase table
        # is the lower-case letters only), then a selection and its replace, which copies them, or a count
        flt = dict(op="filter", slot=slot, f=int(rng.choice([1, 2, 3])), heap="own")
        whole = lambda m: dict(op="rp_fetch", slot=slot, first=0, n=int(m.slots[slot].rp["out"]().size)) if m.slots[slot].rp else None      # noqa: E731
        picks = lambda m: _count_sel_op(slot, dst=dst, sel="own" if m.slots[slot].sel is None or m.slots[slot].sel["own"] else "caller")   # noqa: E731
        dst, r = str(rng.choice(["own", "caller"])), rng.random()
        if r < 0.2:
            after = [_count_op(slot, dst=dst)]
        elif r < 0.45:
            after = _prepare(rng, "replace", slot) + [picks, _pass_op("replace", slot), whole]
        elif r < 0.65:
            # the matching lines with one line of context each side, and their bytes as they were written
            after = _line_prepare(rng, slot, "matching") + [_matching_op(slot, context=(1, 1)), lambda m: _gather_op(slot, m), _late_fetch(rng, slot, "ga_fetch")]
        else:
            after = _prepare(rng, "replace_docs", slot) + [picks, _pass_op("replace_docs", slot), whole, dict(op="rpd_fetch", slot=slot)]
        agenda = _prepare(rng, "filter", slot) + [flt] + after + agenda
    elif kind in ("scan_bytes", "scan_finish") and sc is not None and sc["fold"] and not sc["pending"] and rng.random() < 0.25:
        # the same table uploaded again: the fold is off, and the folded scan's records are fetched late
        again = dict(op="load_table", tab=m.tab, knob=m.knob, cknob=m.cknob, **({"via": "device"} if rng.random() < 0.4 else {}))
        agenda = [again, dict(op="get_fold"), lambda m: dict(op="records", slot=slot, first=0, n=m._count(m.slots[slot].scan)) if m.slots[slot].scan else None,
                  dict(op="packed", slot=slot)] + agenda
    elif kind == "count" and chosen["dst"] == "own" and not chosen["acc"] and rng.random() < 0.5:
        # counts accumulated over an exact and a folded scan of one table generation
        # (the first one counts the scan that is there, made in the other mode: the counts are the SCAN's, not the setting's)
        agenda = [_Quiet(toggle), _count_op(slot, acc=True), _scan_step(rng, slot), _count_op(slot, acc=True), dict(op="cnt_fetch", slot=slot)] + agenda
    return agenda


def plan(seed, n_ops=None, words=False, counts=False, lines=False, fold=False):
    """The plan of `seed`: a list of operations (dicts).  Deterministic; the model decides what each one is worth.
    `words`: the second family of plans, in which the whole-word filter is one of the operations (the first family is
    what it was before the filter existed, seed for seed).  `counts`: the third family, the second one's operations and
    the per-pattern counts (count, count_sel, cnt_fetch; tables installed under an entry of CKNOBS).  `lines`: the
    fourth family, the third one's operations and the line path (LINE_OPS), LINE_PLAN_OPS operations long.  `fold`:
    the fifth family, the fourth one's operations and the case fold (set_fold, get_fold, the upload of an image through
    load_table_device), drawn from POOL -- the nine old tables, each with one more input, and the four nocase tables
    of FOLD_TABLES -- and FOLD_PLAN_OPS operations long."""
    n_ops = n_ops or (FOLD_PLAN_OPS if fold else LINE_PLAN_OPS if lines else PLAN_OPS)
    rng = np.random.default_rng([seed, 0x53455353494F4E] + ([0x464F4C44] if fold else [0x4C494E4553] if lines else [0x434F554E54] if counts else
                                                             [0x574F5244] if words else []))
    kinds = FOLD_KINDS if fold else LINE_KINDS if lines else COUNT_KINDS if counts else WORD_KINDS if words else KINDS
    lines = lines or fold                                       # (the fold family works the line path like the line family)
    counts = counts or lines                                    # (the line family counts like the count family)
    words = words or counts                                     # (the count family filters like the word family)
    turn = {"seed": seed}                                       # (the line family's walks start elsewhere in every plan)
    m = Model()
    if fold:
        m.pool = POOL
    ops, agenda = [], []
    if counts:                                                  # (a fetch before any count: PFAC_E_STATE)
        agenda = [dict(op="cnt_fetch", slot=int(rng.integers(0, N_SLOTS)))] if rng.random() < 0.3 else []
    if lines and rng.random() < 0.5:                            # (a fetch before anything was made: PFAC_E_STATE)
        early = str(rng.choice(["doc_fetch", "ids_fetch", "gaoff_fetch"]))
        agenda.append(dict(op=early, slot=int(rng.integers(0, N_SLOTS)), **({"first": 0, "n": 1} if early == "doc_fetch" else {})))
    if lines and rng.random() < 0.5:                            # (half of the line plans begin with slot 1 on slot 0's stream)
        agenda.append(dict(op="set_stream", slot=1, share=True))
    if fold and rng.random() < 0.4:                             # (the setting before any upload: PFAC_E_STATE)
        agenda.append(dict(op="set_fold", mode=1) if rng.random() < 0.5 else dict(op="get_fold"))
    while len(ops) < n_ops:
        want_err = rng.random() < (1 / 16 if words else 1 / 8)   # (words: the filter between a selection and its replace adds errors of its own)
        chosen, quiet, proposed = None, False, False
        while agenda and chosen is None and not want_err:      # what the session set out to do comes first
            cand = agenda.pop(0)
            quiet = isinstance(cand, _Quiet)
            cand = cand.step if quiet else cand
            cand = cand(m) if callable(cand) else cand
            if cand is not None and m.predict(cand).status is not None:
                chosen = cand
        for _ in range(60):
            if chosen is not None:
                break
            cand = _propose(rng, m, kinds)
            if cand is None:
                continue
            st = m.predict(cand).status
            if st is None:
                continue
            if (st != OK) == want_err:
                chosen, proposed = cand, True
            elif st != OK and not agenda and (cand["op"] in PASSES or cand["op"] in PRODUCER_OF):
                # a pass (or the fetch of one) with nothing to work on: do what is missing first, then the pass
                if cand["op"] in PASSES:
                    agenda = _prepare(rng, cand["op"], cand["slot"]) + [cand]
                else:
                    prod = PRODUCER_OF[cand["op"]]
                    agenda = _prepare(rng, prod, cand["slot"]) + [_pass_op(prod, cand["slot"]), cand]
            elif st != OK and not agenda and cand["op"] == "filter" and cand["heap"] == "own":
                agenda = _prepare(rng, "filter", cand["slot"], docs=FILTERS[cand["f"]]["doc"] == "slot") + [cand]
            elif st != OK and not agenda and cand["op"] in ("matching", "context", "gather", "ids_fetch", "ga_fetch", "gaoff_fetch"):
                # the line path with nothing to work on: a scan, offsets, a segment and ids first
                upto = "matching" if cand["op"] in ("matching", "context") else "gather"
                made = {"ids_fetch": [_matching_op(cand["slot"])], "ga_fetch": [lambda m, c=cand: _gather_op(c["slot"], m)],
                        "gaoff_fetch": [lambda m, c=cand: _gather_op(c["slot"], m)]}.get(cand["op"], [])
                agenda = _line_prepare(rng, cand["slot"], upto) + made + ([] if cand["op"] == "ga_fetch" else [cand])
        if chosen is None:
            continue
        if fold and chosen["op"] == "load_table" and proposed:
            # the uploads a fold plan draws walk the pool and each table's knobs, so that the suite's plans fold them all
            tab = sorted(POOL)[_next(turn, "table") % len(POOL)]
            chosen = dict(chosen, tab=tab, knob=POOL[tab]["knobs"][_next(turn, "knob of " + tab) % len(POOL[tab]["knobs"])])
        if counts and chosen["op"] == "load_table" and "cknob" not in chosen:
            chosen = dict(chosen, cknob=int(rng.integers(0, len(CKNOBS))))
        st = m.apply(chosen).status
        ops.append(chosen)
        if words:
            slot = chosen.get("slot", 0)
            f = _filter_step(rng, slot)
            # a filtered scan is there to be read: most filters are followed by a reader or a pass ...
            if st == OK and chosen["op"] == "filter" and rng.random() < 0.75:
                agenda = _after_filter(rng, slot) + agenda
            # ... results made before a filter are fetched after it ...
            elif st == OK and chosen["op"] in PASSES and chosen.get("own") and rng.random() < 0.35:
                agenda += [f, dict(op=FETCH_OF[chosen["op"]], slot=slot, **({"first": 0, "n": 1} if chosen["op"] == "replace" else {}))]
            elif st == OK and chosen["op"] == "text" and rng.random() < 0.5:
                agenda += [f, lambda m, slot=slot: dict(op="text_fetch", slot=slot, first=0, n=len(m.x.text(*m.slots[slot].text))) if m.slots[slot].text else None]
            # ... an overflowed scan is PFAC_E_OVERFLOW ...
            elif st == OK and chosen["op"] == "scan_ext" and m.slots[slot].scan["over"]:
                agenda = [lambda m: None if m.flen else dict(op="set_flen"), dict(op="filter", slot=slot, f=int(rng.integers(0, 5)), heap="own")] + agenda
            # ... bad offsets, then good ones ...
            elif st == OK and chosen["op"] == "set_doc" and chosen["dkey"].startswith("bad") and rng.random() < 0.8:
                good = dict(chosen, dkey=str(rng.choice(DOC_KEYS[:2])))
                agenda = _prepare(rng, "filter", slot) + [dict(op="filter", slot=slot, f=int(rng.integers(5, 10)), heap="own"), good,
                                                           dict(op="filter", slot=slot, f=int(rng.integers(5, 10)), heap="own")] + agenda
            # ... and a fresh scan (mostly one with something to drop) is filtered before anything else looks at it, a
            # caller's heap with the wrong pointer first
            elif st == OK and chosen["op"] in ("scan_bytes", "scan_ext", "scan_finish") and not m.slots[slot].scan["over"] and rng.random() < (0.6 if m._count(m.slots[slot].scan) >= 16 else 0.15):
                wrong = [dict(op="filter", slot=slot, f=int(rng.integers(0, 5)), heap=str(rng.choice(["none", "slot"])))] if chosen["op"] == "scan_ext" and rng.random() < 0.5 else []
                agenda = _prepare(rng, "filter", slot, docs=rng.random() < 0.5) + wrong + [f] + agenda
        # a pass that left a slot-owned result: now and then another pass first, then the late fetch of this one's output
        if st == OK and chosen["op"] in PASSES and chosen.get("own") and rng.random() < 0.4:
            other = str(rng.choice([p for p in PASSES if p != chosen["op"]]))
            slot = chosen["slot"]
            agenda += _prepare(rng, other, slot) + [_pass_op(other, slot), dict(op=FETCH_OF[chosen["op"]], slot=slot,
                                                                                **({"first": 0, "n": 1} if chosen["op"] == "replace" else {}))]
        # histories the header has a sentence for: a replace of a selection made before a table upload; records of a
        # scan that overflowed its heap; ...
        if st == OK and chosen["op"] in ("select", "select_docs") and rng.random() < 0.15:
            tab = str(rng.choice(sorted(m.pool)))
            agenda = [dict(op="load_table", tab=tab, knob=int(rng.choice(POOL[tab]["knobs"]))), dict(op="set_flen"),
                      dict(op="set_reps", rkey=str(rng.choice(REP_KEYS))), _pass_op("replace", chosen["slot"])] + agenda
        if st == OK and chosen["op"] == "select_docs" and rng.random() < 0.15:     # ... a per-document replace after new offsets
            sc = m.slots[chosen["slot"]].scan
            agenda = [dict(op="set_doc", slot=chosen["slot"], tab=sc["tab"], inp=sc["inp"], no=sc["no"], dkey=str(rng.choice(DOC_KEYS[:2]))),
                      _pass_op("replace_docs", chosen["slot"])] + agenda
        if st == OK and chosen["op"] == "scan_ext" and m.slots[chosen["slot"]].scan["over"] and rng.random() < 0.7:
            agenda = [dict(op="records", slot=chosen["slot"], first=0, n=int(rng.integers(1, 33)))] + agenda
        if st == OK and chosen["op"] == "load_table" and rng.random() < 0.75:   # after an upload most sessions set lengths and replacements again
            agenda = [dict(op="set_flen"), dict(op="set_reps", rkey=str(rng.choice(REP_KEYS)))] + agenda
        if st == OK and chosen["op"] == "scan_start" and rng.random() < 0.7:    # the other slot works while this scan is pending
            agenda = [dict(op="scan_bytes", slot=1 - chosen["slot"], inp=chosen["inp"], no=chosen["no"]),
                      dict(op="scan_finish", slot=chosen["slot"])] + agenda
        if counts and (not lines or rng.random() < 0.25):           # (the line family has an agenda of its own to get through)
            agenda = _count_agenda(rng, m, chosen, st, agenda)
        if lines and not quiet and (not fold or rng.random() < 0.5):
            agenda = _line_agenda(rng, m, chosen, st, agenda, turn)
        if fold and not (quiet and chosen["op"] == "set_fold"):
            agenda = _fold_agenda(rng, m, chosen, st, agenda)
    return ops


def shrink(seed, k, n_ops=None, words=False, counts=False, lines=False, fold=False):
    """The plan of `seed` with operation k onwards removed: cut a failing history down by hand."""
    return plan(seed, n_ops, words, counts, lines, fold)[:k]


# ---------------------------------------------------------------------------
# the executor

class _SlotBufs:
    def __init__(self):
        self.inp = self.rec = None                              # caller-owned device buffers the slot's state refers to
        self.sel = self.first = None                            # ... and the guarded outputs (_OutBuf) of its last selection
        self.last_sel = None                                    # the d_out of the last selection that went to the caller
        self.cnt = None                                         # the caller's count buffer (_CountBuf) and the model's serial of it
        self.cnt_serial = 0
        self.seg_first = None                                   # the d_doc_first (_OutBuf) of the last segment into the caller's buffers


class Odd:
    """A pointer four bytes into `buf`, for a stand-in device whose buffers have no addresses."""

    def __init__(self, buf):
        self.buf = buf


class _CountBuf:
    """The caller's d_counts: exactly n x 8 bytes between guard bands, every byte CNT_FILL (heapguard.GuardedBuffer; on
    a stand-in device one of its buffers, the bands behind the payload)."""

    def __init__(self, g, n):
        self.n = int(n)
        if hasattr(g, "alloc"):
            self.guard, self.buf = None, g.alloc(self.n * 8 + 64)
            self.buf.a[:] = CNT_FILL
            self.ptr, self.odd = self.buf, Odd(self.buf)
        else:
            from heapguard import GuardedBuffer
            self.guard = GuardedBuffer(self.n * 8, fill=CNT_FILL, device=f"cuda:{g.device}")
            self.ptr, self.odd = self.guard.ptr, self.guard.ptr + 4

    def read(self):
        raw = self.guard.host() if self.guard is not None else self.buf.a[:self.n * 8]
        return raw.view(np.uint64).copy()

    def check(self, what):
        if self.guard is not None:
            self.guard.check(what=what)
        else:
            assert (self.buf.a[self.n * 8:] == CNT_FILL).all(), f"bytes behind {what} changed"


class _OutBuf:
    """A pass's caller-owned output (d_out, d_doc_first, d_out_offsets): exactly n_bytes -- what the ABI asks for, not a
    byte of slack -- between guard bands, every byte OUT_FILL (heapguard.GuardedBuffer; on a stand-in device one of its
    buffers, the band behind the payload).  `ptr` is what the call is given."""

    def __init__(self, g, n_bytes):
        self.n = int(n_bytes)
        if hasattr(g, "alloc"):
            self.guard, self.buf = None, g.alloc(self.n + 64)
            self.buf.a[:] = OUT_FILL
            self.ptr = self.buf
        else:
            from heapguard import GuardedBuffer
            self.guard = GuardedBuffer(self.n, fill=OUT_FILL, device=f"cuda:{g.device}")
            self.ptr = self.guard.ptr

    def read(self, dtype, count):
        nb = int(count) * np.dtype(dtype).itemsize
        assert nb <= self.n, f"the call reports {count} entries, the buffer was sized for {self.n // np.dtype(dtype).itemsize}"
        raw = self.guard.host(nb) if self.guard is not None else self.buf.a[:nb]
        return raw.view(dtype).copy()

    def check(self, what, untouched=False):
        """The guard bands hold; with `untouched` the payload is still the fill too (a refused call wrote nothing)."""
        if self.guard is not None:
            self.guard.check(payload_untouched=untouched, what=what)
        else:
            assert (self.buf.a[self.n:] == OUT_FILL).all(), f"bytes behind {what} changed"
            assert not untouched or (self.buf.a[:self.n] == OUT_FILL).all(), f"payload of {what} changed"


def _raw_count(g, slot, d_records, d_counts, n_states, flags):
    """pfac_records_count_states itself, for an n_states the wrapper would not pass."""
    if hasattr(g, "raw_count_states"):
        return g.raw_count_states(slot, d_records, d_counts, n_states, flags)
    import ctypes as C
    from phfpfac_amd.matcher import _ptr
    n = C.c_uint64(0)
    g._check(g._L.pfac_records_count_states(g._ctx, slot, _ptr(d_records), _ptr(d_counts), int(n_states), int(flags), C.byref(n)))
    return n.value


def _raw_matching(g, slot, context, d_first, n_docs, before, after, flags, d_out, out_cap):
    """pfac_documents_matching / _context themselves, for the flags the wrapper would not pass."""
    if hasattr(g, "raw_matching"):
        return g.raw_matching(slot, context, d_first, n_docs, before, after, flags, d_out, out_cap)
    import ctypes as C
    from phfpfac_amd.matcher import _ptr
    n = C.c_uint64(0)
    if context:
        rc = g._L.pfac_documents_matching_context(g._ctx, slot, _ptr(d_first), int(n_docs), int(before), int(after), int(flags), _ptr(d_out),
                                                  int(out_cap), C.byref(n))
    else:
        rc = g._L.pfac_documents_matching(g._ctx, slot, _ptr(d_first), int(n_docs), int(flags), _ptr(d_out), int(out_cap), C.byref(n))
    if rc:
        e = PfacError(rc, (g._L.pfac_last_error(g._ctx) or b"").decode())
        e.n_matching = n.value
        raise e
    return n.value


def _odd(g, buf):
    """Four bytes into a caller's buffer: a misaligned pointer."""
    if hasattr(g, "alloc"):
        return Odd(buf)
    return (buf if isinstance(buf, int) else int(buf.data_ptr())) + 4


def _alloc(g, n_bytes):
    if hasattr(g, "alloc"):
        return g.alloc(n_bytes)
    import torch
    return torch.empty(max(int(n_bytes), 16), dtype=torch.uint8, device=f"cuda:{g.device}")


def _upload(g, arr):
    if hasattr(g, "upload"):
        return g.upload(arr)
    import torch
    buf = _alloc(g, arr.nbytes + 4096)
    if arr.nbytes:
        buf[:arr.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()))
    torch.cuda.synchronize(g.device)
    return buf


def _same(got, want, what="value"):
    if isinstance(want, tuple):
        assert isinstance(got, tuple) and len(got) == len(want), f"{what}: got {got!r:.80}, want {len(want)} parts"
        for k, (a, b) in enumerate(zip(got, want)):
            _same(a, b, f"{what}[{k}]")
    elif isinstance(want, np.ndarray):
        got = np.asarray(got)
        assert got.size == want.size, f"{what}: {got.size} entries, want {want.size}"
        if got.size:
            ne = np.flatnonzero(got.astype(np.uint64) != want.astype(np.uint64))
            assert ne.size == 0, f"{what}: first difference at index {int(ne[0])}: {got[ne[0]]} != {want[ne[0]]} ({ne.size} differ)"
    elif isinstance(want, (bytes, bytearray)):
        got = bytes(got)
        assert len(got) == len(want), f"{what}: {len(got)} bytes, want {len(want)}"
        if got != want:
            ne = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
            raise AssertionError(f"{what}: first difference at byte {int(ne[0])} ({ne.size} differ)")
    else:
        assert got == want and (got is None) == (want is None), f"{what}: {got}, want {want}"


class Executor:
    def __init__(self, g, model):
        self.g, self.m = g, model
        self.x = model.x
        self.bufs = [_SlotBufs() for _ in range(N_SLOTS)]
        self.stats = dict(ops=0, errors=0, compared=0, filters=0, counts=0, widths=set(), staging=set(), variants=set(), statuses=set(),
                          regimes=set(),                        # (regimes: (entry of CKNOBS, "direct" / "cache") of every count that ran)
                          splits=0, matchings=0, gathers=0, ids=0,   # (the line path: calls that succeeded, document ids compared)
                          folded=0, toggles=0, modes=0)         # (the fold: scans queued with it on, set_fold calls that succeeded, modes compared)
        self.inputs = {}                                        # (tab, inp) -> a caller's device copy of that input
        self.ids_direct = getattr(g, "states_are_ids", False)

    def ids(self, tab, states):
        st = np.asarray(states).astype(np.int64)
        return st if self.ids_direct or tab is None else np.asarray(self.x.table(tab).idmap, dtype=np.int64)[st]

    def recs(self, tab, rec):
        self.stats["compared"] += int(rec.size)
        return rec["pos"].astype(np.int64), self.ids(tab, rec["state"])

    def note_fold(self, slot):
        self.stats["folded"] += bool(self.m.slots[slot].scan["fold"])

    def note_scan(self, slot):
        self.stats["widths"].add(int(self.g.scan_format(slot)[0]))
        info = self.g.info()
        self.stats["staging"].add((info["staging_buffers"], info["staging_records"]))
        self.stats["variants"].add(info["variant"])

    def step(self, op):
        """Perform one operation and compare with the model.  Returns the model's status."""
        s = self.m.slots[op.get("slot", 0)]
        before = dict(scan=dict(s.scan) if s.scan else None, sel=dict(s.sel) if s.sel else None)
        exp = self.m.apply(op)
        assert exp.status is not None, "the contract does not decide this operation: a plan must not contain it"
        self.stats["ops"] += 1
        self.stats["statuses"].add(exp.status)
        try:
            got = getattr(self, "do_" + op["op"])(op, exp, before)
        except PfacError as e:
            assert e.status == exp.status, f"raised {e} (status {e.status}), want {STATUS_NAMES[exp.status]}"
            if exp.count is not None:
                n = [getattr(e, a) for a in ("n_kept", "n_selected", "out_bytes", "n_matching") if hasattr(e, a)]
                assert n == [exp.count], f"the overflow error carries {n}, want [{exp.count}]"
            self.stats["errors"] += 1
            return exp.status
        assert exp.status == OK, f"returned normally, want {STATUS_NAMES[exp.status]}"
        _same(got, exp.value())
        return OK

    # -- tables -------------------------------------------------------------
    def do_load_table(self, op, exp, before):
        saved = {k: os.environ.get(k) for k in KNOB_NAMES + list(CKNOB_NAMES)}
        for k in saved:
            os.environ.pop(k, None)
        os.environ.update(KNOBS[op["knob"]])                    # knobs are read when a table is installed
        os.environ.update(CKNOBS[op.get("cknob", 0)])
        try:
            table = self.x.table(op["tab"])
            if op.get("via", "host") == "device":               # the image alone, as after a broadcast: no host_table, so no fold
                blob = table.blob()
                self.g.load_table_device(_upload(self.g, blob), int(blob.size))
                self.g.table = table                            # (the wrapper's lengths and replacements come from the host table)
            else:
                self.g.load_table(table)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v

    def do_set_fold(self, op, exp, before):
        g = self.g
        if op["mode"] in (0, 1):
            g.set_case_fold(bool(op["mode"]))
        elif hasattr(g, "raw_set_case_fold"):
            g.raw_set_case_fold(op["mode"])
        else:                                                   # (a mode the wrapper would not pass)
            g._check(g._L.pfac_table_set_case_fold(g._ctx, op["mode"]))
        self.stats["toggles"] += 1

    def do_get_fold(self, op, exp, before):
        self.stats["modes"] += 1
        return int(self.g.case_fold)

    def do_set_flen(self, op, exp, before):
        t = self.m.tab
        self.g.set_final_lengths(self.x.table(t).final_lengths() if t else np.ones(1, np.int32))

    def do_set_reps(self, op, exp, before):
        if op["rkey"] == "redact":
            self.g.set_redaction(b"#")
        else:
            self.g.set_replacements(self.x.reps(self.m.tab, op["rkey"]) if self.m.tab else {})

    # -- scans --------------------------------------------------------------
    def _data(self, op):
        return self.x.input(self.m.tab or "abc2", op["inp"])

    def _own_scan(self, slot):
        self.bufs[slot].inp = self.bufs[slot].rec = None

    def do_scan_bytes(self, op, exp, before):
        self._own_scan(op["slot"])
        rec = self.g.scan_bytes(self._data(op), op["no"], slot=op["slot"])
        self.note_scan(op["slot"])
        self.note_fold(op["slot"])
        return self.recs(exp.tab, rec)

    def do_scan_start(self, op, exp, before):
        g, data, slot = self.g, self._data(op), op["slot"]
        self._own_scan(slot)
        g.reserve(slot, max(data.size, 1), max(op["cap"], 1))
        if data.size:
            g.h2d(data, slot)
        g.scan_async(op["no"], data.size, slot=slot)
        self.note_fold(slot)

    def do_scan_finish(self, op, exp, before):
        n, over = self.g.scan_finish(op["slot"], allow_overflow=True)
        self.note_scan(op["slot"])
        return int(n), bool(over)

    def do_scan_ext(self, op, exp, before):
        g, data, slot = self.g, self._data(op), op["slot"]
        d_in, d_rec = _upload(g, data), _alloc(g, max(op["cap"], 1) * 8 + 64)
        g.scan_async(op["no"], data.size, d_input=d_in, d_records=d_rec, capacity=op["cap"], slot=slot)
        self.bufs[slot].inp, self.bufs[slot].rec = d_in, d_rec
        n, over = g.scan_finish(slot, allow_overflow=True)
        self.note_scan(slot)
        self.note_fold(slot)
        return int(n), bool(over)

    def do_records(self, op, exp, before):
        rec = self.g.records_to_host(op["n"], op["slot"], d_records=self.bufs[op["slot"]].rec, first=op["first"])
        return self.recs(exp.tab, rec)

    def do_packed(self, op, exp, before):
        from phfpfac_amd.dist import packed_to_records
        words, tix = self.g.packed_to_host(op["slot"], d_records=self.bufs[op["slot"]].rec)
        return self.recs(exp.tab, packed_to_records(words, tix, self.g.scan_format(op["slot"])[0]))

    def do_checksum(self, op, exp, before):
        sc = before["scan"]
        n = self.x.count(sc["tab"], sc["inp"], sc["no"], sc["filt"], sc["fold"]) if sc else 1
        return int(self.g.checksum(n, op["base"], op["slot"], d_records=self.bufs[op["slot"]].rec))

    def do_text(self, op, exp, before):
        n = self.g.emit_text_device(op["base"], op["slot"], d_records=self.bufs[op["slot"]].rec)
        self.stats["compared"] += int(n)
        return self.g.text_to_host(n, op["slot"])

    def do_text_fetch(self, op, exp, before):
        return self.g.text_to_host(op["n"], op["slot"], first=op["first"])

    # -- documents ----------------------------------------------------------
    def do_set_doc(self, op, exp, before):
        self.g.set_doc_offsets(self.x.offsets(op["tab"], op["inp"], op["no"], op["dkey"]), op["slot"])

    def _n_docs(self, slot):
        doc = self.m.slots[slot].doc
        return int(self.x.offsets(*doc).size - 1) if doc else 1

    def _cap(self, op, exp):
        if exp.status == OK:
            return exp.value()[0]
        return exp.count // 2 if exp.count is not None else 0   # (an overflow the model expects, else the call fails before it looks)

    def do_filter(self, op, exp, before):
        g, slot = self.g, op["slot"]
        d, b, sc = FILTERS[op["f"]], self.bufs[slot], before["scan"]
        tab = sc["tab"] if sc else (self.m.tab or "abc2")
        heap = {"own": b.rec, "none": None, "slot": g.records_ptr(slot) or None}[op["heap"]]
        nd = 0 if d["doc"] == "none" else self._n_docs(slot) + (d["doc"] == "wrong_n")
        fmt = g.scan_format(slot) if exp.status == OK else None
        n = int(g.filter_whole_words(slot, self.x.word_bytes(tab, d["ws"]), d["edges"], self.x.neighbour(tab, d["ws"], d["prev"]),
                                     self.x.neighbour(tab, d["ws"], d["next"]), n_docs=nd, d_input=b.inp, d_records=heap))
        assert fmt is None or g.scan_format(slot) == fmt, f"scan_format changed from {fmt} to {g.scan_format(slot)}"
        assert g.last_count(slot) == n, f"last_count {g.last_count(slot)} after a filter that kept {n}"
        self.stats["filters"] += 1
        return n

    def do_segment(self, op, exp, before):
        g, slot = self.g, op["slot"]
        nd = self._n_docs(slot)
        if op["own"]:
            return int(g.segment_records(nd, slot=slot, d_records=self.bufs[slot].rec))
        cap = self._cap(op, exp)
        d_out, d_first = _OutBuf(g, cap * 8), _OutBuf(g, (nd + 1) * 8)
        n = int(self._guarded(slot, {"d_out": d_out, "d_doc_first": d_first}, "segment_records", lambda: g.segment_records(
            nd, d_out=d_out.ptr, out_cap=cap, d_doc_first=d_first.ptr, slot=slot, d_records=self.bufs[slot].rec)))
        self.bufs[slot].seg_first = d_first
        return (n, d_first.read(np.uint64, nd + 1)) + self.recs(exp.tab, d_out.read(REC, n))

    def do_seg_fetch(self, op, exp, before):
        seg = self.m.slots[op["slot"]].seg
        n, nd = (int(self.x.seg(*seg["key"])[0][-1]), int(self.x.offsets(*seg["key"][:4]).size - 1)) if seg else (0, 1)
        first, rec = self.g.segment_to_host(n, nd, op["slot"])
        return (first,) + self.recs(exp.tab, rec)

    # -- selection ----------------------------------------------------------
    def _guarded(self, slot, outs, what, call):
        """One pass call into the caller's outputs `outs` ({name: _OutBuf}, each exactly as long as the ABI asks for): the
        guard bands hold after it, and after a refused call every payload is byte for byte what it was."""
        try:
            got = call()
        except PfacError:
            self.g.sync(slot)
            for name, b in outs.items():
                b.check(f"the caller's {name} after a refused {what}", untouched=True)
            raise
        self.g.sync(slot)
        for name, b in outs.items():
            b.check(f"the caller's {name} of {what}")
        return got

    def _check_kept(self, slot, when):
        """The outputs of the slot's last selection that later operations still refer to: their guard bands hold."""
        b = self.bufs[slot]
        for name, buf in (("d_out", b.sel), ("d_doc_first", b.first), ("d_out", b.last_sel)):
            if buf is not None:
                buf.check(f"the caller's {name} of the last selection, {when}")

    def _drop_selection(self, slot):
        self._check_kept(slot, "when it is replaced")
        self.bufs[slot].sel = self.bufs[slot].first = None

    def finish(self):
        for slot in range(N_SLOTS):
            self._check_kept(slot, "at the end of the session")

    def do_select(self, op, exp, before):
        g, slot = self.g, op["slot"]
        self._drop_selection(slot)
        if op["own"]:
            n, ex = g.select_leftmost_longest(op["entry"], slot=slot, d_records=self.bufs[slot].rec)
            return int(n), int(ex)
        cap = self._cap(op, exp)
        d_out = _OutBuf(g, cap * 8)
        n, ex = self._guarded(slot, {"d_out": d_out}, "select_leftmost_longest", lambda: g.select_leftmost_longest(
            op["entry"], d_out=d_out.ptr, out_cap=cap, slot=slot, d_records=self.bufs[slot].rec))
        self.bufs[slot].sel = self.bufs[slot].last_sel = d_out
        return (int(n), int(ex)) + self.recs(exp.tab, d_out.read(REC, int(n)))

    def do_select_docs(self, op, exp, before):
        g, slot = self.g, op["slot"]
        nd = self._n_docs(slot)
        self._drop_selection(slot)
        if op["own"]:
            return int(g.select_leftmost_longest_documents(nd, slot=slot, d_records=self.bufs[slot].rec))
        cap = self._cap(op, exp)
        d_out, d_first = _OutBuf(g, cap * 8), _OutBuf(g, (nd + 1) * 8)
        n = int(self._guarded(slot, {"d_out": d_out, "d_doc_first": d_first}, "select_leftmost_longest_documents",
                              lambda: g.select_leftmost_longest_documents(nd, d_out=d_out.ptr, out_cap=cap, d_doc_first=d_first.ptr, slot=slot,
                                                                          d_records=self.bufs[slot].rec)))
        self.bufs[slot].sel, self.bufs[slot].first = d_out, d_first
        self.bufs[slot].last_sel = d_out
        return (n, d_first.read(np.uint64, nd + 1)) + self.recs(exp.tab, d_out.read(REC, n))

    def _sel_n(self, slot):
        sel = self.m.slots[slot].sel
        if sel is None:
            return 0, 1
        if sel["kind"] == "whole":
            return int(self.x.sel(*sel["key"])[0].size), 1
        return int(self.m._ds(sel["key"])[0][-1]), int(self.x.offsets(*sel["key"][:4]).size - 1)

    def do_sel_fetch(self, op, exp, before):
        return self.recs(exp.tab, self.g.selection_to_host(self._sel_n(op["slot"])[0], op["slot"]))

    def do_docsel_fetch(self, op, exp, before):
        n, nd = self._sel_n(op["slot"])
        first, rec = self.g.doc_selection_to_host(n, nd, op["slot"])
        return (first,) + self.recs(exp.tab, rec)

    # -- replace ------------------------------------------------------------
    def do_replace(self, op, exp, before, docs=False):
        g, slot = self.g, op["slot"]
        b, sel = self.bufs[slot], before["sel"]
        kw = dict(d_input=b.inp, slot=slot, d_sel=b.sel.ptr if b.sel is not None else None)
        if docs:
            kw["d_doc_first"] = b.first.ptr if b.first is not None else None
        call = g.replace_selection_documents if docs else g.replace_selection
        if op["own"]:
            return int(call(**kw))
        cap = self._cap(op, exp)
        outs = {"d_out": _OutBuf(g, cap)}
        nd = int(self.x.offsets(*sel["key"][:4]).size - 1) if docs and sel is not None and sel["kind"] == "docs" else 1
        if docs:
            outs["d_out_offsets"] = _OutBuf(g, (nd + 1) * 8)
            kw["d_out_offsets"] = outs["d_out_offsets"].ptr
        try:
            n = int(self._guarded(slot, outs, "replace_selection_documents" if docs else "replace_selection",
                                  lambda: call(d_out=outs["d_out"].ptr, out_cap=cap, **kw)))
        finally:
            self._check_kept(slot, "after a replace that read it")
        self.stats["compared"] += n
        out = (n, outs["d_out"].read(np.uint8, n))
        return out + (outs["d_out_offsets"].read(np.uint64, nd + 1),) if docs else out

    def do_replace_docs(self, op, exp, before):
        return self.do_replace(op, exp, before, docs=True)

    def do_rp_fetch(self, op, exp, before):
        self.stats["compared"] += op["n"]
        return self.g.replacement_to_host(op["n"], op["slot"], first=op["first"])

    def do_rpd_fetch(self, op, exp, before):
        rpd = self.m.slots[op["slot"]].rpd
        return self.g.replacement_doc_offsets_to_host(int(rpd["off"]().size - 1) if rpd else 1, op["slot"])

    # -- counts per pattern ---------------------------------------------------
    def n_entries(self, tab):
        """Entries of a count buffer of table `tab`: its final states (its pattern ids, on a device that works in ids)."""
        if tab is None:
            return 1
        return self.x.n_ids(tab) if self.ids_direct else int(self.x.table(tab).num_final)

    def by_id(self, tab, counts, parts):
        """Device counts per state, summed into their pattern ids; where no two states share an id they are first
        compared state for state, so that two states swapping counts cannot cancel."""
        counts = np.asarray(counts, dtype=np.uint64)
        assert counts.size == self.n_entries(tab), f"{counts.size} counts, want {self.n_entries(tab)}"
        self.stats["compared"] += int(counts.size)
        if self.ids_direct:
            return counts
        if self.x.injective(tab):
            _same(counts, self.x.sum_counts(tab, parts, by_state=True), "counts per state")
        out = np.zeros(self.x.n_ids(tab), dtype=np.uint64)
        np.add.at(out, np.asarray(self.x.table(tab).idmap, dtype=np.int64), counts)
        return out

    def _counted(self, op, call):
        """One count call: into the slot's caller's buffer (allocated afresh when the model says so) or the slot-owned
        one.  The guard bands hold after every call; after a refused one the payload is byte for byte what it was."""
        slot = op["slot"]
        s, b = self.m.slots[slot], self.bufs[slot]
        if op["dst"] == "own":
            was = b.cnt.read() if b.cnt is not None else None
            try:
                n = int(call(None))
            finally:                                            # (the caller's buffer of an earlier call: not this call's to touch)
                if was is not None:
                    self.g.sync(slot)
                    b.cnt.check("the caller's d_counts after a count into the slot-owned buffer")
                    assert np.array_equal(b.cnt.read(), was), "a count into the slot-owned buffer changed the caller's d_counts"
            self.stats["counts"] += 1
            return n
        if b.cnt is None or b.cnt_serial != s.cbuf["serial"]:
            b.cnt, b.cnt_serial = _CountBuf(self.g, self.n_entries(self.m.tab)), s.cbuf["serial"]
        was = b.cnt.read()
        try:
            n = int(call(b.cnt.odd if op["dst"] == "misaligned" else b.cnt.ptr))
        except PfacError:
            self.g.sync(slot)
            b.cnt.check("the caller's d_counts after a refused count")
            assert np.array_equal(b.cnt.read(), was), "a refused count changed the caller's d_counts"
            raise
        self.g.sync(slot)
        b.cnt.check("the caller's d_counts")
        got = b.cnt.read()
        if s.cbuf["base"]:
            got = got - np.uint64(CNT_ENTRY)                    # (an accumulate onto the fresh buffer: its constant is still there)
        self.stats["counts"] += 1
        return n, self.by_id(s.cbuf["tab"], got, s.cbuf["parts"])

    def do_count(self, op, exp, before):
        g, slot = self.g, op["slot"]
        b = self.bufs[slot]
        heap = {"own": b.rec, "none": None, "slot": g.records_ptr(slot) or None}[op["heap"]]
        if op["ns"] == "ok" or self.m.tab is None:
            out = self._counted(op, lambda d: g.count_states(slot, d_records=heap, d_counts=d, accumulate=op["acc"]))
        else:
            nf = self.n_entries(self.m.tab)
            ns = {"minus": nf - 1, "plus": nf + 1, "zero": 0}[op["ns"]]
            out = self._counted(op, lambda d: _raw_count(g, slot, heap, d, ns, int(op["acc"])))
        bins = int(CKNOBS[self.m.cknob].get("PFAC_COUNT_BINS", 0))
        direct = int(self.x.table(self.m.tab).num_final) <= (min(bins, COUNT_DIRECT_MAX) if bins else COUNT_DIRECT_MAX)
        self.stats["regimes"].add((self.m.cknob, "direct" if direct else "cache"))
        assert g.last_count(slot) == (out if op["dst"] == "own" else out[0]), "n_counted is not the scan's match count"
        return out

    def do_count_sel(self, op, exp, before):
        g, slot = self.g, op["slot"]
        b, n_sel = self.bufs[slot], self._sel_n(slot)[0]
        if op["sel"] in ("junk", "misaligned"):
            junk = _alloc(g, max(n_sel, 1) * 8 + 16)
            if hasattr(junk, "fill_"):
                junk.fill_(0xFF)                                # states past any n_states
            else:
                junk.a[:] = 0xFF
                junk.junk = True
            d_sel = junk if op["sel"] == "junk" else Odd(junk) if hasattr(g, "alloc") else int(junk.data_ptr()) + 4
        else:
            kept = b.sel if b.sel is not None else b.last_sel  # (after a failed select: the one before)
            d_sel = None if op["sel"] == "own" or kept is None else kept.ptr
        return self._counted(op, lambda d: g.count_selection_states(slot, d_sel=d_sel, d_counts=d, accumulate=op["acc"]))

    def do_cnt_fetch(self, op, exp, before):
        cnt = self.m.slots[op["slot"]].cnt
        got = self.g.state_counts_to_host(op["slot"])
        return self.by_id(cnt["tab"], got, cnt["parts"]) if cnt else got

    # -- lines: split, matching documents, gather -------------------------------
    def _caller_input(self, tab, inp):
        if (tab, inp) not in self.inputs:
            self.inputs[(tab, inp)] = _upload(self.g, self.x.input(tab, inp))
        return self.inputs[(tab, inp)]

    def _d_input(self, op):
        if op["src"] == "slot":
            return None
        buf = self._caller_input(op["tab"], op["inp"])
        return _odd(self.g, buf) if op["src"] == "odd" else buf

    def do_split(self, op, exp, before):
        nb = (1 << 31) if op["nb"] == "over" else op["nb"]       # (2 GiB: above every input buffer of a session, below the 2^32 limit)
        n_docs, tail = self.g.split_documents(nb, op["delim"], d_input=self._d_input(op), slot=op["slot"])
        self.stats["splits"] += 1
        return int(n_docs), int(tail)

    def do_doc_fetch(self, op, exp, before):
        doc = self.m.slots[op["slot"]].doc
        nd = int(self.x.offsets(*doc).size) - 1 if doc else 0
        self.stats["ids"] += op["n"]
        return self.g.doc_offsets_to_host(nd, op["slot"], first=op["first"], n=op["n"])

    def do_matching(self, op, exp, before, context=False):
        g, slot = self.g, op["slot"]
        b, s = self.bufs[slot], self.m.slots[slot]
        # n_docs and the pointer of the doc_first the call is given (the model has judged them already)
        if op["first"] == "own":
            nd, d_first = (int(self.x.offsets(*s.seg["key"][:4]).size) - 1 if s.seg else 1), None
        elif op["first"] == "seg":
            nd, d_first = int(self.x.offsets(*s.segc[:4]).size) - 1, b.seg_first.ptr
        else:
            nd, d_first = int(self.x.offsets(*s.sel["key"][:4]).size) - 1, b.first.ptr
        nd += op["nd"] != "ok"
        n = int(exp.value() if op["out"] == "own" else exp.value()[0]) if exp.status == OK else (exp.count or 0)
        cap = n - 1 if op["out"] == "small" else n
        out = None if op["out"] == "own" else _OutBuf(g, (cap + (op["out"] == "odd")) * 8)
        d_out = None if out is None else _odd(g, out.ptr) if op["out"] == "odd" else out.ptr
        bef, aft = (op["before"], op["after"]) if context else (0, 0)
        if op["flags"] > 1 or (context and (op["flags"] or not (bef or aft))):     # (what the wrapper would not pass, or not to this call)
            call = lambda: _raw_matching(g, slot, context, d_first, nd, bef, aft, op["flags"], d_out, cap)      # noqa: E731
        else:
            call = lambda: g.matching_documents(nd, invert=bool(op["flags"]), d_doc_first=d_first, d_out=d_out, out_cap=cap, slot=slot,   # noqa: E731
                                                before=bef, after=aft)
        got = int(call() if out is None else self._guarded(slot, {"d_ids_out": out}, "matching_documents", call))
        self.stats["matchings"] += 1
        if out is None:
            return got
        self.stats["ids"] += got
        return got, out.read(np.uint64, got)

    def do_context(self, op, exp, before):
        return self.do_matching(op, exp, before, context=True)

    def do_ids_fetch(self, op, exp, before):
        dm = self.m.slots[op["slot"]].dm
        n = int(self.x.doc_ids(dm[0]).size) if dm else 0
        self.stats["ids"] += n
        return self.g.matching_documents_to_host(n, op["slot"])

    def do_gather(self, op, exp, before):
        g, slot, x = self.g, op["slot"], self.x
        s = self.m.slots[slot]
        doc, dm = s.doc, s.dm
        off = x.offsets(*doc) if doc else np.zeros(2, np.uint64)
        nd = int(off.size) - 1
        own_ids = op["ids"] == "own"
        ids = x.id_list(dm[0] if dm else None, op["ids"], nd) if not own_ids or dm else np.zeros(0, np.uint64)
        d_off = None if op["off"] == "slot" else _upload(g, off)
        d_ids = None if own_ids else _upload(g, ids)
        n = int(exp.value()[0]) if exp.status == OK else (exp.count or 0)
        cap = n - 1 if op["out"] == "small" else n
        outs = {}
        if op["out"] != "own":
            outs["d_out"] = _OutBuf(g, cap + 16 * (op["out"] == "odd"))
        if op["oo"] != "own":
            outs["d_out_offsets"] = _OutBuf(g, (int(ids.size) + (op["ni"] != "ok") + 1) * 8)
        d_out = None if op["out"] == "own" else _odd(g, outs["d_out"].ptr) if op["out"] == "odd" else outs["d_out"].ptr
        d_oo = outs["d_out_offsets"].ptr if "d_out_offsets" in outs else None
        got = int(self._guarded(slot, outs, "gather_documents", lambda: g.gather_documents(
            nd + (op["nd"] != "ok"), int(ids.size) + (op["ni"] != "ok"), op["nb"], d_input=self._d_input(op), d_doc_offsets=d_off, d_ids=d_ids,
            d_out=d_out, out_cap=cap, d_out_offsets=d_oo, slot=slot)))
        self.stats["gathers"] += 1
        res = (got,)
        if "d_out" in outs:
            self.stats["compared"] += got
            res += (outs["d_out"].read(np.uint8, got),)
        if d_oo is not None:
            self.stats["ids"] += int(ids.size) + 1
            res += (outs["d_out_offsets"].read(np.uint64, int(ids.size) + 1),)
        return res

    def do_ga_fetch(self, op, exp, before):
        self.stats["compared"] += op["n"]
        return self.g.gathered_to_host(op["n"], op["slot"], first=op["first"])

    def do_gaoff_fetch(self, op, exp, before):
        ga = self.m.slots[op["slot"]].ga
        n_ids = int(self.x.gather(*ga[0])[1].size) - 1 if ga else 0
        self.stats["ids"] += n_ids + 1
        return self.g.gathered_offsets_to_host(n_ids, op["slot"])

    # -- plumbing -----------------------------------------------------------
    def do_set_stream(self, op, exp, before):
        self.g.set_stream(1, self.g.stream_handle(0) if op["share"] else 0)

    def do_sync(self, op, exp, before):
        self.g.sync(op["slot"])

    def do_reserve_grow(self, op, exp, before):
        self.g.reserve(op["slot"], op["k"] * IN_STEP if op["which"] in ("input", "both") else 0,
                       op["k"] * REC_STEP if op["which"] in ("records", "both") else 0)
        if self.m.slots[op["slot"]].scan is None:
            self._own_scan(op["slot"])


def run(g, ops, model=None, seed=None):
    """Performs `ops` on `g` (one context, never re-created), comparing every result with `model` bit for bit.  Returns
    the executor's statistics; raises AssertionError naming the seed, the operation and the ten before it."""
    ex = Executor(g, model or Model())
    for k, op in enumerate(ops):
        try:
            ex.step(op)
        except AssertionError as e:
            hist = "\n".join(f"    {j:3d}  {fmt(ops[j])}" for j in range(max(0, k - 10), k + 1))
            e2 = AssertionError(f"session seed {seed}, operation {k} {fmt(op)}: {e}\n  the operations up to it (cut the plan with shrink({seed}, k)):\n{hist}")
            e2.op_index = k
            raise e2 from e
    try:
        ex.finish()                                             # the outputs the slots still refer to: their guard bands
    except AssertionError as e:
        raise AssertionError(f"session seed {seed}, behind the last operation: {e}") from e
    return ex.stats
