"""Model-based session tests for the verdict calls: pattern groups and their masks, document scores, the rank and both
gathers -- ONE context driven through a random sequence of these calls, the way tests/session.py drives the scan, the
passes and the line path.  It stands beside session.py and changes nothing of it.

Three parts, none of which needs a GPU to import:

  Pool        three tables whose records are 2, 4 and 8 bytes wide (entries of session.TABLES under knob sets of
              passfuzz.KNOBS: the literal abc2, the dictionary-like mid4, the class table cclass with its multi-id
              state), three inputs each (3, 65 and 130 tiles, cut into lines of about 16 or about 1 500 bytes, a line
              across every 64-tile edge), six forms of document offsets, two group assignments, two weight vectors, and
              what the CPU says about them: the oracle's records (classfuzz.ClassMatcher for the class table) through
              wordref, the header's document cut, llref.greedy, groupref, scoreref, topref, gatherref, fmtref and
              splitref -- never the device, never PfacTable.final_lengths.  Cached by key.
  Model       what include/pfac.h PROMISES for every call given the calls before it: a value or a PfacError.status.
              It mirrors the header, not pfac_hip.hip; its state holds only keys into the cache.  The rules it encodes
              are named R1 .. R10 (see `RULES`); an expectation carries the tags of the rules that decided it.
  plan / run / shrink
              plan(seed) draws PLAN_OPS operations, asking the model which are legal and picking a refused one about
              one time in eight; consumers are weighted so that a result is often read late, behind something that could
              have destroyed it, and an agenda forces the rare histories.  run(g, ops, model) performs them on a
              GpuMatcher (or anything shaped like one) and compares bit for bit, skipping nothing; shrink(seed, k) is the
              plan cut before operation k.

A stand-in device that already works in pattern ids needs nothing special here: no record leaves the device in these
sessions, only counts, masks, scores, ids, offsets and bytes."""
import copy

import numpy as np

import groupref
import scoreref
import session as S
import topref
import wordref
from fmtref import Fmt, format_ref
from gatherref import context_ids, gather_ref
from llref import greedy
from passfuzz import GROUP, KNOB_NAMES, KNOBS, TILE, record_width
from phfpfac_amd import PfacError
from session import (E_ARG, E_OVERFLOW, E_STATE, IN_STEP, N_SLOTS, OK, REC_STEP, STATUS_NAMES, U64_MAX, _alloc, _odd, _OutBuf,
                     _same, _upload, fmt, offsets_ok)
from splitref import matching_ids, split_offsets

SEEDS = list(range(24))
PLAN_OPS = 160
MIN_VERDICT_OPS = 40
SORT_BLOCK = 1024                        # PFAC_TOP_SORT_BLOCK, written apart from the product's

RULES = {
    "R1": "any of the five id producers discards the slot's ids first, also when it fails; only d_ids_out == NULL leaves any",
    "R2": "the ids reach the fetch and the gathers unchanged, whichever producer made them, ranked ids in rank order",
    "R3": "only top_scores discards the top pairs; a failed one discards the pairs and the ids; windows past n_top are E_ARG",
    "R4": "a mask call discards the slot's masks, also when it fails; one into the caller's buffer leaves none",
    "R5": "the scores likewise; documents_scores and selection_document_scores are one pass",
    "R6": "gather and gather_format are one pass; the all-zero fmt and NULL give the plain gather's bytes",
    "R7": "groups and weights belong to the uploaded table; a wrong n_states changes nothing; a result keeps the values it was made with",
    "R8": "the error order of the mask and score passes: E_STATE, then E_OVERFLOW, then E_ARG; a caller's buffer untouched",
    "R9": "a slot-owned result stays fetchable and byte-identical until the next call of its own pass",
    "R10": "selection_document_scores(NULL, NULL) follows the rules of pfac_selection_count_states' d_sel; one NULL is E_ARG",
}
R9_EVENTS = ("scan", "filter", "upload", "reserve", "offsets", "stream", "other_slot")
RESULTS = ("ids", "masks", "scores", "top", "ga")

# ---------------------------------------------------------------------------
# the pool

def _k(**knobs):
    return KNOBS.index(knobs)


VTABLES = {"abc2": [_k()], "mid4": [_k(), _k(PFAC_LAG="1")], "cclass": [_k(PFAC_WIDE="1")]}      # 2-, 4- and 8-byte records
WIDTHS = {"abc2": 2, "mid4": 4, "cclass": 8}
TILES = (3, 65, 130)                     # one wave of the mask / score kernel; a second wave; the largest of test_gpu_pass_bounds.py
# mean line length of input i of every table: across the pool the split gives fewer than 64 documents (mid4, 3 tiles),
# between 1 024 and 4 096 (abc2, 3 tiles: lines of about 10 bytes, since 12 KiB hold no 1 024 lines of 16) and more than
# 16 384 (the short-line inputs of 65 and 130 tiles)
LINE_MEAN = {"abc2": (10, 1500, 16), "mid4": (1500, 16, 1500), "cclass": (16, 1500, 16)}
PLANT = {"abc2": b"abc", "cclass": b"ax"}                       # on either side of every 64-tile edge (mid4: its shortest line)
FORMS = ("split", "host", "one", "zero", "bad_end", "bad_order")
GKEYS, WKEYS = ("g0", "g1"), ("w0", "w1")
PREDS = (dict(any_of=groupref.ALL), dict(all_of=1), dict(any_of=(1 << 63) | (1 << 7), none_of=1), dict(all_of=6, invert=True),
         dict(any_of=groupref.ALL, invert=True))
SCORE_RULES = (None, dict(min_count=1), dict(min_score=-2, max_score=5), dict(density=(1, 50)), dict(min_count=1, invert=True))
KS = (0, 1, 64, 65, SORT_BLOCK - 1, SORT_BLOCK + 1, U64_MAX)
FMTS = (Fmt(), Fmt(number=True), Fmt(number=True, byte_offset=True, group_sep=b"--\n", context_sep=True), Fmt(terminate=10),
        Fmt(number=True, byte_offset=True, number_base=999_999_990, offset_base=99_999, group_sep=b"==", sep_first=True))
CONTEXTS = ((1, 0), (0, 2), (U64_MAX, U64_MAX))
ID_FORMS = ("own", "perm", "twice", "bad_id")


class Pool:
    """What the CPU says, computed once per key.  Tables, matchers and line lengths are session.Expectations' own."""

    def __init__(self):
        self.x = S.expectations()
        self._c = {}

    def _memo(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    def table(self, t):
        return self.x.table(t)

    def n_ids(self, t):
        return int(self.x.tinfo(t)["ll"].size) - 1

    def input_size(self, t, i):
        return TILES[i] * TILE

    def plant(self, t):
        return PLANT.get(t) or min(self.x.tinfo(t)["lines"], key=lambda p: (len(p), p))

    def input(self, t, i):
        def make():
            n = self.input_size(t, i)
            rng = np.random.default_rng([sorted(VTABLES).index(t), i, 0x56455244])
            if t == "abc2":
                u = rng.random(n)
                data = np.where(u < 0.12, ord("a"), np.where(u < 0.5, ord("b"), ord("c"))).astype(np.uint8)
            elif t == "cclass":
                alphabet = np.frombuffer(S.CCLASS_ALPHABET.replace(b"\n", b""), dtype=np.uint8)
                data = alphabet[rng.integers(0, alphabet.size, n)]
            else:
                info = self.x.tinfo(t)
                data = info["symbols"][rng.integers(0, info["symbols"].size, n)]
                plist = sorted(set(info["lines"]))
                for at in rng.integers(0, n - 1, n // 50):
                    pt = np.frombuffer(plist[int(rng.integers(0, len(plist)))], dtype=np.uint8)
                    m = min(len(pt), n - int(at))
                    data[int(at):int(at) + m] = pt[:m]
            mean = LINE_MEAN[t][i]
            ends = np.cumsum(rng.integers(0, 2 * mean + 1, n // mean + 64) + 1) - 1
            ends = ends[ends < n]
            p = np.frombuffer(self.plant(t), dtype=np.uint8)
            for edge in range(GROUP, n, GROUP):                 # one line lies across every 64-tile edge, a match on either side
                ends = ends[(ends < edge - 24) | (ends >= edge + 24)]
                data[edge - 1 - p.size:edge - 1] = p
                data[edge + 1:edge + 1 + p.size] = p
            data[ends] = 10
            return data
        return self._memo(("input", t, i), make)

    # -- the scan -----------------------------------------------------------
    def _whole(self, t, i):
        """Every record of the whole input: (pos, lens, starts, fids) -- record r ends the patterns
        fids[starts[r]:starts[r + 1]] (one for a literal table, several for a multi-id state of the class table)."""
        def make():
            info, data = self.x.tinfo(t), self.input(t, i)
            if hasattr(info["matcher"], "full"):
                fpos, fids = info["matcher"].full(data)
                fpos, fids = fpos.astype(np.int64), fids.astype(np.int64)
                ln = info["ll"][fids]
                starts = np.flatnonzero(np.append(True, (fpos[1:] != fpos[:-1]) | (ln[1:] != ln[:-1]))) if fpos.size else np.zeros(0, np.int64)
                return fpos[starts], ln[starts], starts, fids
            pos, ids = info["matcher"].scan_spec(data, None)
            pos, ids = pos.astype(np.int64), ids.astype(np.int64)
            return pos, info["ll"][ids], np.arange(pos.size), ids
        return self._memo(("whole", t, i), make)

    def rows(self, sk):
        """(pos, lens, idx) of scan `sk` = (table, input, n_owned, filtered): idx names the records of `_whole`."""
        def make():
            t, i, no, filt = sk
            pos, lens, _, _ = self._whole(t, i)
            keep = pos < no
            if filt:
                keep = keep & wordref.filter_words(self.input(t, i), pos, lens)
            idx = np.flatnonzero(keep)
            return pos[idx], lens[idx], idx
        return self._memo(("rows", sk), make)

    def by_id(self, t, key):
        n = self.n_ids(t)
        if key == "g0":
            return groupref.masks_by_id(groupref.groups_for(n))
        if key == "g1":
            return groupref.masks_by_id([None] + [j % 3 for j in range(1, n + 1)])
        if key == "w0":                                         # zero and cancelling weights, the int32 extremes
            return scoreref.w_by_id(scoreref.weights_for(n))
        return scoreref.w_by_id([0] + [1 + j % 4 for j in range(1, n + 1)])

    def setter_arg(self, t, key):
        """What GpuMatcher.set_pattern_groups / set_pattern_weights is given for `key`."""
        n = self.n_ids(t)
        if key == "g0":
            return groupref.groups_for(n)
        if key == "g1":
            return [None] + [j % 3 for j in range(1, n + 1)]
        if key == "w0":
            return scoreref.weights_for(n)
        return [0] + [1 + j % 4 for j in range(1, n + 1)]

    def per_record(self, t, i, key):
        """The mask (g*) or weight (w*) of every record of `_whole`: the OR / the sum over the patterns it ends."""
        def make():
            _, _, starts, fids = self._whole(t, i)
            v = self.by_id(t, key)[fids]
            if starts.size == 0:
                return v[:0]
            return np.bitwise_or.reduceat(v, starts) if key[0] == "g" else np.add.reduceat(v, starts)
        return self._memo(("per", t, i, key), make)

    # -- offsets ------------------------------------------------------------
    def offsets(self, dk):
        def make():
            t, i, form = dk
            n = self.input_size(t, i)
            if form == "split":
                return split_offsets(self.input(t, i), 10)[0]
            if form == "one":
                return np.array([0, n], dtype=np.uint64)
            if form == "zero":
                return np.zeros(1, dtype=np.uint64)
            rng = np.random.default_rng([sorted(VTABLES).index(t), i, 0x4F4646])
            cuts = np.sort(rng.integers(0, n + 1, 300))
            cuts[rng.integers(1, 300, 12)] = cuts[rng.integers(0, 299, 12)]      # empty documents
            off = np.concatenate([[0], np.sort(cuts), [n, n]]).astype(np.uint64)
            if form == "bad_end":
                off[-1] = n + 1
            if form == "bad_order":
                off[-3:] = [n - 1, n - 2, n]
            return off
        return self._memo(("off", dk), make)

    def n_docs(self, dk):
        return int(self.offsets(dk).size) - 1

    # -- results ------------------------------------------------------------
    def value(self, key):
        return self._memo(key, lambda: getattr(self, "_v_" + key[0])(*key[1:]))

    def _cut(self, sk, dk):
        pos, lens, idx = self.rows(sk)
        return pos, np.arange(pos.size), lens, self.offsets(dk).astype(np.int64), idx

    def _v_masks(self, sk, dk, gkey):
        pos, r, lens, off, idx = self._cut(sk, dk)
        return groupref.masks_cut(pos, r, lens, off, self.per_record(sk[0], sk[1], gkey)[idx])

    def _v_scores(self, sk, dk, wkey):
        pos, r, lens, off, idx = self._cut(sk, dk)
        return scoreref.scores_cut(pos, r, lens, off, self.per_record(sk[0], sk[1], wkey)[idx])

    def _v_seg(self, sk, dk):
        """doc_first of the segment pass: the records the header's rule keeps, per document."""
        pos, r, lens, off, idx = self._cut(sk, dk)
        sc = scoreref.scores_cut(pos, r, lens, off, np.zeros(pos.size, dtype=np.int64))
        return np.concatenate(([0], np.cumsum(sc["count"].astype(np.int64)))).astype(np.uint64)

    def _v_sel(self, sk, dk):
        """(doc_first, idx) of the per-document leftmost-longest selection: the records that end inside their document,
        greedily from 0 in one walk (a pick ends at or before its document's end, so the cursor never reaches into a
        later document: llref.greedy per document, back to back -- held against docreplref.per_doc in
        tests/test_verdict_plan.py)."""
        pos, _, lens, off, idx = self._cut(sk, dk)
        return select_walk(pos, lens, off, idx, sk[2])

    def _v_selscores(self, sk, dk, wkey):
        first, idx = self.value(("sel", sk, dk))
        return scoreref.scores_of_selection(first, idx, self.per_record(sk[0], sk[1], wkey))

    def _v_m(self, segkey, invert):
        return matching_ids(self.value(segkey), invert)

    def _v_c(self, segkey, before, after):
        return context_ids(self.value(segkey), before, after)

    def _v_g(self, mkey, pred):
        return groupref.predicate(self.value(mkey), **PREDS[pred])

    def _v_s(self, sckey, rule, dk):
        return scoreref.predicate(self.value(sckey), None if dk is None else self.offsets(dk), **SCORE_RULES[rule])

    def _v_t(self, sckey, rule, dk, k, flags):
        """(ids, pairs) of a top call."""
        sc = self.value(sckey)
        cand = np.arange(sc.size, dtype=np.uint64) if SCORE_RULES[rule] is None else self.value(("s", sckey, rule, dk))
        ids, _ = topref.top(topref.ranking(sc, cand, flags), k, flags)
        return ids, sc[ids.astype(np.int64)]

    def ids_of(self, key):
        v = self.value(key)
        return v[0] if key[0] == "t" else v

    def id_list(self, idkey, form, n_docs):
        """A caller's id list: a seeded permutation of a third of the documents, the slot's ids twice over, or a list
        with n_docs in it."""
        if form == "own":
            return self.ids_of(idkey)
        rng = np.random.default_rng([n_docs, ID_FORMS.index(form), 0x494453])
        if form == "perm":
            return rng.permutation(n_docs)[:max(n_docs // 3, 1)].astype(np.uint64) if n_docs else np.zeros(0, np.uint64)
        if form == "twice":
            base = rng.integers(0, max(n_docs, 1), 40).astype(np.uint64) if n_docs else np.zeros(0, np.uint64)
            return np.concatenate([base, base[::-1]])
        return np.array([0, n_docs, 0], dtype=np.uint64)

    def _v_ga(self, inp, dk, idkey, form, f, segkey):
        """(out, out_off) of a gather (f None) or a formatted gather (f: index into FMTS)."""
        off = self.offsets(dk)
        ids = self.id_list(idkey, form, int(off.size) - 1)
        if f is None or FMTS[f].plain():
            return gather_ref(self.input(*inp), off, ids)
        return format_ref(self.input(*inp), off, ids, FMTS[f], None if segkey is None else self.value(segkey))


def select_walk(pos, lens, off, idx, n_owned):
    nd = off.size - 1
    doc = np.minimum(np.searchsorted(off, pos, side="right") - 1, nd - 1)
    fits = pos + lens <= off[doc + 1]
    pick, ex = greedy(pos[fits], lens[fits], 0, n_owned)
    assert ex == 0
    first = np.concatenate(([0], np.cumsum(np.bincount(doc[fits][pick], minlength=nd)))).astype(np.uint64)
    return first, idx[fits][pick]


_POOL = None


def pool():
    global _POOL
    if _POOL is None:
        _POOL = Pool()
    return _POOL


def pairs(sc):
    """A pfac_doc_score array as two unsigned arrays, for the bitwise compare."""
    sc = np.asarray(sc)
    return sc["score"].astype(np.int64).view(np.uint64), sc["count"].astype(np.uint64)


# ---------------------------------------------------------------------------
# the model

class Exp:
    """What the header promises for one operation: a status (None: the contract does not decide this call), the value
    of a successful call, the exact count an overflow error carries, the rules that decided it and, for a late fetch,
    the (result, event) pairs of R9 it crosses."""

    def __init__(self, status=OK, fn=None, count=None, rules=(), late=()):
        self.status, self.fn, self.count, self.rules, self.late = status, fn, count, tuple(rules), tuple(late)

    def value(self):
        return None if self.fn is None else self.fn()


class _Slot:
    def __init__(self):
        self.inp = None                  # (table, input) of the bytes in the slot's input buffer
        self.scan = None                 # dict(sk, gen, over, ext)
        self.serial = 0                  # counts scans and filters: a selection is of one serial
        self.docs = None                 # dk
        self.seg = None                  # the slot-owned doc_first of the last segment: its key
        self.sel = None                  # dict(key, serial, gen, own, nd)
        self.ids = self.masks = self.scores = self.top = self.ga = None     # slot-owned results: dict(key, n, seen)
        self.cmasks = self.cscores = None                       # what the caller's buffer of the last call into one holds: (key, n)
        self.grow = 0


VERDICT_OPS = ("set_groups", "set_weights", "masks", "masks_fetch", "match_groups", "scores", "sel_scores", "scores_fetch", "match_scores",
               "top", "top_fetch", "matching", "context", "ids_fetch", "gather", "gather_format", "ga_fetch", "gaoff_fetch")
PRODUCERS = ("matching", "context", "match_groups", "match_scores", "top")
CONSUMERS = ("ids_fetch", "gather", "gather_format")
OTHER_OPS = ("load_table", "set_flen", "scan", "scan_over", "filter", "split", "set_doc", "segment", "select_docs", "reserve_grow",
             "set_stream", "sync")


class Model:
    def __init__(self, p=None):
        self.x = p or pool()
        self.tab = self.knob = None
        self.gen = 0
        self.flen = False
        self.groups = self.weights = None
        self.shared = False
        self.slots = [_Slot() for _ in range(N_SLOTS)]

    def clone(self):
        m = copy.copy(self)
        m.slots = [copy.copy(s) for s in self.slots]
        for s in m.slots:
            for r in RESULTS:
                if getattr(s, r) is not None:
                    setattr(s, r, dict(getattr(s, r), seen=set(getattr(s, r)["seen"])))
        return m

    def predict(self, op):
        return self.clone().apply(op)

    def apply(self, op):
        s = self.slots[op.get("slot", 0)]
        e = getattr(self, "_" + op["op"])(op, s)
        if "slot" in op and op["op"] not in ("sync",) and not op["op"].endswith("_fetch"):
            self._event(self.slots[1 - op["slot"]], "other_slot")
        return e

    # -- helpers ------------------------------------------------------------
    @staticmethod
    def _one(faults):
        return Exp(next(iter(faults))) if len(faults) == 1 else Exp(None)

    def _event(self, s, what):
        """R9: every slot-owned result of `s` has now lived through `what`."""
        for r in RESULTS:
            if getattr(s, r) is not None:
                getattr(s, r)["seen"].add(what)

    @staticmethod
    def _res(key, n):
        return dict(key=key, n=int(n), seen=set())

    def _late(self, s, r):
        return tuple((r, e) for e in sorted(getattr(s, r)["seen"]))

    def _nd(self, s):
        return None if s.docs is None else self.x.n_docs(s.docs)

    def _pass_faults(self, s, need=None):
        """R8: the rungs a pass over the slot's scan and offsets stands on, in the header's order: (E_STATE faults,
        E_OVERFLOW, E_ARG for the offsets)."""
        state = s.scan is None or s.scan["gen"] != self.gen or not self.flen or s.docs is None
        if need == "groups":
            state = state or self.groups is None
        if need == "weights":
            state = state or self.weights is None
        over = s.scan is not None and s.scan["over"]
        arg = s.scan is not None and s.docs is not None and not offsets_ok(self.x.offsets(s.docs), s.scan["sk"][2])
        return state, over, arg

    # -- tables, scans, offsets: what the verdicts stand on -----------------
    def _load_table(self, op, s):
        self.tab, self.knob = op["tab"], op["knob"]
        self.gen += 1
        self.flen, self.groups, self.weights = False, None, None              # R7: an upload clears them
        for t in self.slots:
            self._event(t, "upload")
        return Exp()

    def _set_flen(self, op, s):
        if self.tab is None:
            return Exp(E_STATE)
        self.flen = True
        return Exp()

    def _setter(self, op, attr):
        """R7: pfac_table_set_state_groups / _weights."""
        if self.tab is None:
            return Exp(E_STATE, rules=["R7"])
        if op["ns"] != "ok":
            return Exp(E_ARG, rules=["R7"])                     # the earlier values stay in force
        setattr(self, attr, (self.tab, self.gen, op["key"]))
        return Exp(rules=["R7"])

    def _set_groups(self, op, s):
        return self._setter(op, "groups")

    def _set_weights(self, op, s):
        return self._setter(op, "weights")

    def _scan(self, op, s):
        if self.tab is None:
            return Exp(None)
        t, i = self.tab, op["inp"]
        no = self.x.input_size(t, i) if op["no"] == "all" else 0
        s.inp = (t, i)
        s.scan = dict(sk=(t, i, no, False), gen=self.gen, over=False, ext=False)
        s.serial += 1
        self._event(s, "scan")
        sk = s.scan["sk"]
        return Exp(OK, lambda: int(self.x.rows(sk)[0].size))

    def _scan_over(self, op, s):
        """A scan of a caller's input into a caller's heap of 16 records: it overflows."""
        if self.tab is None:
            return Exp(None)
        t, i = self.tab, op["inp"]
        sk = (t, i, self.x.input_size(t, i), False)
        s.scan = dict(sk=sk, gen=self.gen, over=True, ext=True)
        s.serial += 1
        self._event(s, "scan")
        return Exp(OK, lambda: (int(self.x.rows(sk)[0].size), True))

    def _filter(self, op, s):
        if s.scan is None or s.scan["gen"] != self.gen or not self.flen:
            return Exp(E_STATE)
        if s.scan["over"]:
            return Exp(E_OVERFLOW)
        if s.scan["sk"][:2] != s.inp:
            return Exp(None)
        s.scan = dict(s.scan, sk=s.scan["sk"][:3] + (True,))
        s.serial += 1
        self._event(s, "filter")
        sk = s.scan["sk"]
        return Exp(OK, lambda: int(self.x.rows(sk)[0].size))

    def _split(self, op, s):
        if s.inp is None:
            return Exp(None)
        s.docs = s.inp + ("split",)
        self._event(s, "offsets")
        dk = s.docs
        return Exp(OK, lambda: split_offsets(self.x.input(*dk[:2]), 10)[1:])

    def _set_doc(self, op, s):
        s.docs = (op["tab"], op["inp"], op["form"])
        self._event(s, "offsets")
        return Exp()

    def _cut_faults(self, s):
        """The status of a segment pass or a per-document selection over the slot's scan and offsets: the scan's state,
        its overflow, then the offsets (session.Model._segment)."""
        if s.scan is None or s.scan["gen"] != self.gen or not self.flen:
            return E_STATE
        if s.scan["over"]:
            return E_OVERFLOW
        if s.docs is None:
            return E_STATE
        return OK if offsets_ok(self.x.offsets(s.docs), s.scan["sk"][2]) else E_ARG

    def _segment(self, op, s):
        s.seg = None
        st = self._cut_faults(s)
        if st:
            return Exp(st)
        s.seg = ("seg", s.scan["sk"], s.docs)
        key = s.seg
        return Exp(OK, lambda: int(self.x.value(key)[-1]))

    def _select_docs(self, op, s):
        s.sel = None                                            # a selection call that failed leaves no selection
        st = self._cut_faults(s)
        if st:
            return Exp(st)
        key = ("sel", s.scan["sk"], s.docs)
        s.sel = dict(key=key, serial=s.serial, gen=self.gen, own=op["out"] == "own", nd=self._nd(s))
        return Exp(OK, lambda: int(self.x.value(key)[0][-1]))

    def _reserve_grow(self, op, s):
        """A reserve above everything the slot holds: the input and record buffers are replaced, and the slot then has
        no finished scan."""
        s.grow = op["k"]
        if s.scan is not None or s.inp is not None:
            s.scan = None
        s.inp = None
        self._event(s, "reserve")
        return Exp()

    def _set_stream(self, op, s):
        self.shared = op["share"]
        for t in self.slots:
            self._event(t, "stream")
        return Exp()

    def _sync(self, op, s):
        return Exp()

    # -- masks (R4) and scores (R5) -----------------------------------------
    def _heap_pass(self, op, s, res, need, table_attr, vkind):
        had = getattr(s, res) is not None
        setattr(s, res, None)                                   # discarded first, whatever the call returns
        state, over, arg = self._pass_faults(s, need)
        rules = ["R4" if res == "masks" else "R5"] if had else []
        if op.get("nd") == "more" and not state:
            state = True                                        # d_doc_offsets NULL with an n_docs that is not theirs
        if state or over or arg or op["out"] == "odd" or op["heap"] == "foreign":
            st = E_STATE if state else E_OVERFLOW if over else E_ARG
            if need in ("groups", "weights") and getattr(self, need) is None:
                rules.append("R7")
            return Exp(st, rules=rules + ["R8"])
        key = (vkind, s.scan["sk"], s.docs, getattr(self, table_attr)[2])
        nd = self._nd(s)
        if op["out"] == "own":
            setattr(s, res, self._res(key, nd))
        else:
            setattr(s, "c" + res, (key, nd))
        return key, rules

    def _masks(self, op, s):
        r = self._heap_pass(op, s, "masks", "groups", "groups", "masks")
        if isinstance(r, Exp):
            return r
        key, rules = r
        own = op["out"] == "own"
        return Exp(OK, lambda: (int(np.bitwise_or.reduce(self.x.value(key), initial=np.uint64(0))),) + (() if own else (self.x.value(key),)), rules=rules)

    def _scores(self, op, s):
        r = self._heap_pass(op, s, "scores", "weights", "weights", "scores")
        if isinstance(r, Exp):
            return r
        key, rules = r
        own = op["out"] == "own"
        return Exp(OK, lambda: scoreref.totals(self.x.value(key)) + (() if own else pairs(self.x.value(key))), rules=rules)

    def _sel_scores(self, op, s):
        """R10 (and R5: one pass with pfac_documents_scores).  src: "own" = both pointers NULL, "half" = d_doc_first alone,
        "caller" = the caller's buffers of the last selection into them."""
        if op["src"] == "caller" and (s.sel is None or s.sel["own"] or s.sel["gen"] != self.gen):
            return Exp(None)                                    # (no such buffers to pass, or picks of another table in them)
        had = s.scores is not None
        s.scores = None
        rules = (["R5"] if had else []) + ["R10"]
        if self.tab is None or self.weights is None:
            return Exp(E_STATE, rules=rules + ["R7"])
        sel = s.sel
        if op["src"] == "half":
            return Exp(E_ARG, rules=rules)
        if op["src"] == "own":
            if sel is None or sel["serial"] != s.serial or sel["gen"] != self.gen or not sel["own"]:
                return Exp(E_STATE, rules=rules)
        key = ("selscores",) + sel["key"][1:] + (self.weights[2],)
        if op["out"] == "own":
            s.scores = self._res(key, sel["nd"])
        else:
            s.cscores = (key, sel["nd"])
        own = op["out"] == "own"
        return Exp(OK, lambda: scoreref.totals(self.x.value(key)) + (() if own else pairs(self.x.value(key))), rules=rules)

    def _window(self, op, s, res, rule, as_pairs=False):
        r = getattr(s, res)
        if r is None:
            return Exp(E_STATE if op["n"] else None, rules=[rule])      # ("n == 0 does nothing": with nothing to fetch, undecided)
        if op["first"] + op["n"] > r["n"]:
            return Exp(E_ARG, rules=[rule])
        key, a, b = r["key"], op["first"], op["first"] + op["n"]
        late = self._late(s, res)
        rules = [rule] + (["R9"] if late else [])
        if res in ("masks", "scores"):
            now = self.groups if res == "masks" else self.weights
            if now is None or now[2] != key[3] or now[0] != key[1][0]:
                rules.append("R7")                              # the values of the masks / weights it was made with
        take = (lambda v: v[1]) if res == "top" else (lambda v: v)
        return Exp(OK, (lambda: pairs(take(self.x.value(key))[a:b])) if as_pairs else (lambda: take(self.x.value(key))[a:b]), rules=rules, late=late)

    def _masks_fetch(self, op, s):
        return self._window(op, s, "masks", "R4")

    def _scores_fetch(self, op, s):
        return self._window(op, s, "scores", "R5", as_pairs=True)

    def _top_fetch(self, op, s):
        return self._window(op, s, "top", "R3", as_pairs=True)

    # -- the five producers of ids (R1) -------------------------------------
    def _produce(self, op, s, faults, idkey, rules, top=False):
        """The common end of a producer: `faults` so far; out: "own", "caller" (exactly the count), "small" (one fewer)."""
        if faults:
            return Exp(None) if op["out"] == "small" else Exp(self._one(faults).status, rules=rules)
        n = int(self.x.ids_of(idkey).size)
        if op["out"] == "small":
            return Exp(E_OVERFLOW if n > 0 else None, count=n, rules=rules)
        own = op["out"] == "own"
        if own:
            s.ids = self._res(idkey, n)
            if top:
                s.top = self._res(idkey, n)
        if top:
            return Exp(OK, lambda: (n,) + (() if own else (self.x.value(idkey)[0],) + pairs(self.x.value(idkey)[1])), rules=rules)
        return Exp(OK, lambda: (n,) + (() if own else (self.x.value(idkey),)), rules=rules)

    def _drop_ids(self, s):
        had = s.ids is not None
        s.ids = None
        return ["R1"] if had else []

    def _first_faults(self, op, s):
        faults = set()
        if s.seg is None:
            faults.add(E_STATE)
        elif op.get("nd") == "more":
            faults.add(E_ARG)
        return faults

    def _matching(self, op, s):
        rules = self._drop_ids(s)
        faults = self._first_faults(op, s)
        return self._produce(op, s, faults, None if faults else ("m", s.seg, bool(op["invert"])), rules)

    def _context(self, op, s):
        rules = self._drop_ids(s)
        faults = self._first_faults(op, s)
        return self._produce(op, s, faults, None if faults else ("c", s.seg, op["before"], op["after"]), rules)

    def _src(self, op, s, res, rule):
        """The masks / scores a consumer is given: (key, n, faults, rules); key None where the call is undefined."""
        faults, rules = set(), []
        if op["src"] == "own":
            r = getattr(s, res)
            rules.append(rule)
            if r is None:
                return "none", 0, {E_STATE}, rules
            if op.get("nd") == "more":
                faults.add(E_ARG)
            if r["seen"]:
                rules.append("R9")
            return r["key"], r["n"], faults, rules
        c = getattr(s, "c" + res)
        if c is None or op.get("nd") == "more":
            return None, 0, faults, rules
        return c[0], c[1], faults, rules

    def _match_groups(self, op, s):
        rules = self._drop_ids(s)
        key, n, faults, more = self._src(op, s, "masks", "R4")
        if key is None:
            return Exp(None)
        late = self._late(s, "masks") if op["src"] == "own" and s.masks is not None and not faults else ()
        e = self._produce(op, s, faults, None if faults else ("g", key, op["pred"]), rules + more)
        e.late = late if e.status == OK else ()
        return e

    def _score_src(self, op, s, rules):
        key, n, faults, more = self._src(op, s, "scores", "R5")
        if key is None:
            return None
        dk = None
        if SCORE_RULES[op["rule"]] is not None and "density" in SCORE_RULES[op["rule"]]:
            if s.docs is None:
                faults = faults | {E_STATE}
            elif s.docs[2].startswith("bad") or key == "none":
                return None
            elif self.x.n_docs(s.docs) != n:
                faults = faults | {E_ARG}
            dk = s.docs
        late = self._late(s, "scores") if op["src"] == "own" and s.scores is not None and not faults else ()
        return key, dk, faults, rules + more, late

    def _match_scores(self, op, s):
        rules = self._drop_ids(s)
        if SCORE_RULES[op["rule"]] is None:
            return Exp(None)                                    # (rule NULL is E_ARG: GpuMatcher always passes one)
        r = self._score_src(op, s, rules)
        if r is None:
            return Exp(None)
        key, dk, faults, rules, late = r
        e = self._produce(op, s, faults, None if faults else ("s", key, op["rule"], dk), rules)
        e.late = late if e.status == OK else ()
        return e

    def _top(self, op, s):
        rules = self._drop_ids(s)
        if s.top is not None:
            rules.append("R3")
        s.top = None                                            # R3: discarded by every top call, also a failed one
        r = self._score_src(op, s, rules)
        if r is None:
            return Exp(None)
        key, dk, faults, rules, late = r
        e = self._produce(op, s, faults, None if faults else ("t", key, op["rule"], dk, op["k"], op["flags"]), rules, top=True)
        e.late = late if e.status == OK else ()
        return e

    def _ids_fetch(self, op, s):
        if s.ids is None:
            return Exp(E_STATE, rules=["R1"])
        key, late = s.ids["key"], self._late(s, "ids")
        return Exp(OK, lambda: self.x.ids_of(key), rules=["R2"] + (["R9"] if late else []), late=late)

    # -- the two gathers (R6) -------------------------------------------------
    def _gather(self, op, s, f=None):
        """ids: "own" = d_ids NULL, else a caller's list; ni: n_ids of the list or one more; out: "own" (bytes and offsets
        slot-owned), "caller" (both the caller's, exactly as large as the ABI names), "small"."""
        had = s.ga is not None
        s.ga = None                                             # discarded by either call, also a failed one
        rules = ["R6"] if had or f is not None else []
        if s.inp is None:
            return Exp(None)
        faults = set()
        if s.docs is None:
            faults.add(E_STATE)
        if op["ids"] == "own":
            if s.ids is None:
                faults.add(E_STATE)
                rules.append("R1")
                if op["ni"] != "ok":
                    return Exp(None)
            elif op["ni"] != "ok":
                faults.add(E_ARG)
                rules.append("R1")
        elif op["ni"] != "ok":
            return Exp(None)
        segkey = None
        if f is not None and FMTS[f].context_sep:
            if s.seg is None:
                faults.add(E_STATE)
            elif s.docs is not None and self.x.n_docs(s.docs) != int(self.x.value(s.seg).size) - 1:
                faults.add(E_ARG)
            segkey = s.seg
        nb = self.x.input_size(*s.inp)
        idkey = s.ids["key"] if op["ids"] == "own" and s.ids is not None else None
        if s.docs is not None and not (op["ids"] == "own" and s.ids is None):
            off = self.x.offsets(s.docs).astype(np.int64)
            ids = self.x.id_list(idkey, op["ids"], int(off.size) - 1).astype(np.int64)
            good = ids < off.size - 1
            a, b = off[ids[good]], off[ids[good] + 1]
            if not good.all() or (a > b).any() or (b > nb).any():
                faults.add(E_ARG)
        if faults:
            return Exp(None) if op["out"] == "small" or len(faults) > 1 else Exp(next(iter(faults)), rules=rules)
        key = ("ga", s.inp, s.docs, idkey, op["ids"], f, segkey)
        n = int(self.x.value(key)[0].size)
        if op["out"] == "small":
            return Exp(E_OVERFLOW if n > 0 else None, count=n, rules=rules)
        late = self._late(s, "ids") if op["ids"] == "own" else ()
        if op["ids"] == "own":
            rules = rules + ["R2"] + (["R9"] if late else [])
        own = op["out"] == "own"
        if own:
            s.ga = self._res(key, n)
        return Exp(OK, lambda: (n,) + (() if own else (self.x.value(key)[0].tobytes(), self.x.value(key)[1])), rules=rules, late=late)

    def _gather_format(self, op, s):
        return self._gather(op, s, op["f"])

    def _ga_fetch(self, op, s):
        if s.ga is None:
            return Exp(E_STATE if op["n"] else None, rules=["R6"])
        if op["first"] + op["n"] > s.ga["n"]:
            return Exp(E_ARG, rules=["R6"])
        key, a, b, late = s.ga["key"], op["first"], op["first"] + op["n"], self._late(s, "ga")
        return Exp(OK, lambda: self.x.value(key)[0][a:b].tobytes(), rules=["R6"] + (["R9"] if late else []), late=late)

    def _gaoff_fetch(self, op, s):
        if s.ga is None:
            return Exp(E_STATE, rules=["R6"])
        key, late = s.ga["key"], self._late(s, "ga")
        return Exp(OK, lambda: self.x.value(key)[1], rules=["R6"] + (["R9"] if late else []), late=late)


# ---------------------------------------------------------------------------
# plans

KINDS = {"load_table": 3, "set_flen": 1, "scan": 7, "scan_over": 1, "filter": 3, "split": 5, "set_doc": 5, "segment": 5, "select_docs": 4,
         "reserve_grow": 2, "set_stream": 1, "sync": 1, "set_groups": 4, "set_weights": 4, "masks": 8, "masks_fetch": 7, "match_groups": 7,
         "scores": 9, "sel_scores": 5, "scores_fetch": 7, "match_scores": 7, "top": 10, "top_fetch": 8, "matching": 5, "context": 4,
         "ids_fetch": 8, "gather": 7, "gather_format": 8, "ga_fetch": 7, "gaoff_fetch": 5}


def _window(rng, total):
    if total == 0 or rng.random() < 0.5:
        return 0, total
    first = int(rng.integers(0, total))
    return first, int(rng.integers(0, total - first + 1))


def _out(rng, p_small=0.08):
    u = rng.random()
    return "small" if u < p_small else "caller" if u < 0.3 else "own"


def _propose(rng, m):
    names = sorted(KINDS)
    w = np.array([KINDS[k] for k in names], dtype=float)
    kind = names[int(rng.choice(len(names), p=w / w.sum()))]
    slot = int(rng.integers(0, N_SLOTS))
    s = m.slots[slot]
    op = dict(op=kind, slot=slot)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]      # noqa: E731
    if kind == "load_table":
        tab = pick(sorted(VTABLES))
        return dict(op=kind, tab=tab, knob=pick(VTABLES[tab]))
    if kind == "set_flen":
        return dict(op=kind)
    if kind in ("set_groups", "set_weights"):
        return dict(op=kind, key=pick(GKEYS if kind == "set_groups" else WKEYS), ns="wrong" if rng.random() < 0.12 else "ok")
    if kind == "set_stream":
        return dict(op=kind, slot=1, share=not m.shared)
    if kind == "scan":
        return dict(op, inp=int(rng.choice(3, p=[0.5, 0.3, 0.2])), no=0 if rng.random() < 0.06 else "all")
    if kind == "scan_over":
        return dict(op, inp=int(rng.integers(0, 3)))
    if kind == "set_doc":
        t, i = s.inp or (m.tab or "abc2", 0)
        form = pick(FORMS[1:]) if rng.random() < 0.8 else "split"
        return dict(op, tab=t, inp=i, form=form)
    if kind == "select_docs":
        return dict(op, out="own" if rng.random() < 0.7 else "caller")
    if kind == "reserve_grow":
        return dict(op, k=s.grow + 1)
    if kind in ("masks", "scores"):
        u = rng.random()
        return dict(op, out="odd" if u < 0.05 else "caller" if u < 0.3 else "own", heap="foreign" if rng.random() < 0.05 else "own",
                    nd="more" if rng.random() < 0.04 else "ok")
    if kind == "sel_scores":
        u = rng.random()
        return dict(op, src="half" if u < 0.1 else "caller" if u < 0.3 else "own", out="own" if rng.random() < 0.75 else "caller")
    if kind in ("masks_fetch", "scores_fetch", "top_fetch"):
        r = getattr(s, kind[:-6])
        total = r["n"] if r is not None else 1
        first, n = _window(rng, total)
        if r is not None and rng.random() < 0.1:
            n = total - first + 1                               # a window past the end: PFAC_E_ARG
        return dict(op, first=first, n=n)
    nd = "more" if rng.random() < 0.05 else "ok"
    if kind == "matching":
        return dict(op, invert=bool(rng.random() < 0.3), nd=nd, out=_out(rng))
    if kind == "context":
        b, a = pick(CONTEXTS)
        return dict(op, before=b, after=a, nd=nd, out=_out(rng))
    src = "caller" if rng.random() < 0.25 else "own"
    if kind == "match_groups":
        return dict(op, src=src, pred=int(rng.integers(0, len(PREDS))), nd=nd, out=_out(rng))
    if kind == "match_scores":
        return dict(op, src=src, rule=int(rng.integers(1, len(SCORE_RULES))), nd=nd, out=_out(rng))
    if kind == "top":
        return dict(op, src=src, rule=int(rng.integers(0, len(SCORE_RULES))), k=pick(KS), flags=int(rng.integers(0, 8)), nd=nd, out=_out(rng))
    if kind in ("gather", "gather_format"):
        form = "own" if rng.random() < 0.7 else pick(ID_FORMS[1:])
        op = dict(op, ids=form, ni="more" if rng.random() < 0.05 else "ok", out=_out(rng))
        return dict(op, f=int(rng.integers(0, len(FMTS)))) if kind == "gather_format" else op
    if kind == "ga_fetch":
        total = s.ga["n"] if s.ga is not None else 1
        first, n = _window(rng, total)
        if s.ga is not None and rng.random() < 0.1:
            n = total - first + 1
        return dict(op, first=first, n=n)
    return op                                                   # filter, split, segment, sync, ids_fetch, gaoff_fetch


def _ground(rng, slot, upto="docs", big=None):
    """Agenda steps that give `slot` whatever a verdict call stands on and lacks: a table with lengths, groups and
    weights, a finished scan of it that did not overflow, offsets that fit it, and (upto "seg") a segment."""
    def table(m):
        return dict(op="load_table", tab=sorted(VTABLES)[int(rng.integers(0, 3))], knob=0) if m.tab is None else None

    def flen(m):
        return None if m.flen else dict(op="set_flen")

    def groups(m):
        return None if m.groups is not None else dict(op="set_groups", key=GKEYS[int(rng.integers(0, 2))], ns="ok")

    def weights(m):
        return None if m.weights is not None else dict(op="set_weights", key=WKEYS[int(rng.integers(0, 2))], ns="ok")

    def scan(m):
        s = m.slots[slot]
        if s.scan is not None and s.scan["gen"] == m.gen and not s.scan["over"] and s.scan["sk"][:2] == s.inp and (big is None or s.inp[1] == big):
            return None
        return dict(op="scan", slot=slot, inp=int(rng.choice(3, p=[0.5, 0.3, 0.2])) if big is None else big, no="all")

    def docs(m):
        s = m.slots[slot]
        if s.scan is None:
            return None
        if s.docs is not None and offsets_ok(m.x.offsets(s.docs), s.scan["sk"][2]) and s.docs[:2] == s.inp:
            return None
        if rng.random() < 0.5:
            return dict(op="split", slot=slot)
        return dict(op="set_doc", slot=slot, tab=s.inp[0], inp=s.inp[1], form=("host", "one", "split")[int(rng.integers(0, 3))])

    def seg(m):
        s = m.slots[slot]
        return None if s.scan is None or s.docs is None or s.seg == ("seg", s.scan["sk"], s.docs) else dict(op="segment", slot=slot)
    steps = [table, flen, groups, weights, scan, docs]
    return steps + ([seg] if upto == "seg" else [])


def _fix_table(op):
    """load_table drawn by `_ground` names knob 0: the table's first knob set."""
    return dict(op, knob=VTABLES[op["tab"]][0]) if op["op"] == "load_table" and op["knob"] == 0 and 0 not in VTABLES[op["tab"]] else op


FETCH_OF = {"masks": "masks_fetch", "scores": "scores_fetch", "sel_scores": "scores_fetch", "top": "top_fetch", "gather": "ga_fetch",
            "gather_format": "ga_fetch", "matching": "ids_fetch", "context": "ids_fetch", "match_groups": "ids_fetch", "match_scores": "ids_fetch"}


def _late_fetch(rng, kind, slot):
    """The whole of a slot-owned result, or a window of it."""
    def step(m):
        s = m.slots[slot]
        if kind in ("ids_fetch", "gaoff_fetch"):
            return dict(op=kind, slot=slot)
        r = getattr(s, "ga" if kind == "ga_fetch" else kind[:-6])
        total = r["n"] if r is not None else 1
        first, n = _window(rng, total)
        return dict(op=kind, slot=slot, first=first, n=n)
    return step


def _event_steps(rng, slot, what):
    """Something that could have destroyed a slot-owned result of `slot` (an event of R9)."""
    if what == "scan":
        return [lambda m: dict(op="scan", slot=slot, inp=int(rng.integers(0, 2)), no="all") if m.tab else None]
    if what == "filter":
        return _ground(rng, slot)[:5] + [dict(op="filter", slot=slot)]
    if what == "upload":
        def up(m):
            tab = sorted(t for t in VTABLES if t != m.tab)[int(rng.integers(0, 2))]
            return dict(op="load_table", tab=tab, knob=VTABLES[tab][0])
        return [up]
    if what == "reserve":
        return [lambda m: dict(op="reserve_grow", slot=slot, k=m.slots[slot].grow + 1)]
    if what == "offsets":
        return [lambda m: dict(op="set_doc", slot=slot, tab=(m.slots[slot].inp or ("abc2", 0))[0], inp=(m.slots[slot].inp or ("abc2", 0))[1],
                               form=FORMS[1 + int(rng.integers(0, 5))])]
    if what == "stream":
        return [lambda m: dict(op="set_stream", slot=1, share=not m.shared)]
    other = 1 - slot
    return _ground(rng, other) + [dict(op="scores", slot=other, out="own", heap="own", nd="ok"),
                                  dict(op="top", slot=other, src="own", rule=0, k=65, flags=4, nd="ok", out="own")]


def _agenda(rng, m, chosen, st, agenda, turn):
    """What a plan sets out to do behind the operation it has just drawn: read a result late, behind an event of R9;
    hand every producer's ids to every consumer; change groups or weights between a pass and its fetch; fail a producer
    and look at what it left."""
    if st != OK or agenda:
        return agenda
    kind, slot = chosen["op"], chosen.get("slot", 0)
    own = chosen.get("out") == "own"
    if kind == "load_table" and rng.random() < 0.4:             # R7: an upload clears groups and weights; all else is there
        z = int(rng.integers(0, N_SLOTS))
        return [dict(op="set_flen"), dict(op="scan", slot=z, inp=int(rng.integers(0, 2)), no="all"), dict(op="split", slot=z),
                dict(op="scores", slot=z, out="own", heap="own", nd="ok"), dict(op="masks", slot=z, out="own", heap="own", nd="ok")]
    if kind in PRODUCERS and own and rng.random() < 0.7:
        turn["pc"] = turn.get("pc", 0) + 1
        cons = CONSUMERS[(turn["pc"] + turn["seed"]) % 3]
        if cons == "ids_fetch":
            step = dict(op="ids_fetch", slot=slot)
        else:
            step = dict(op=cons, slot=slot, ids="own", ni="ok", out="own" if rng.random() < 0.7 else "caller")
            if cons == "gather_format":
                step["f"] = int(rng.integers(0, len(FMTS)))
        mid = []
        if rng.random() < 0.5:
            what = R9_EVENTS[(turn["pc"] + 3 * turn["seed"]) % len(R9_EVENTS)]
            mid = _event_steps(rng, slot, what) if what not in ("reserve", "scan", "offsets", "upload", "filter") or cons == "ids_fetch" else []
        return mid + [step] + ([_late_fetch(rng, "ga_fetch", slot), dict(op="gaoff_fetch", slot=slot)] if cons != "ids_fetch" and step["out"] == "own" else [])
    if kind in FETCH_OF and (own or kind in ("gather", "gather_format") and own) and rng.random() < 0.6:
        turn["ev"] = turn.get("ev", 0) + 1
        what = R9_EVENTS[(turn["ev"] + turn["seed"]) % len(R9_EVENTS)]
        fetches = [_late_fetch(rng, FETCH_OF[kind], slot)]
        if kind in ("gather", "gather_format"):
            fetches.append(dict(op="gaoff_fetch", slot=slot))
        if kind == "top":
            fetches.append(dict(op="ids_fetch", slot=slot))
        return _event_steps(rng, slot, what) + fetches
    if kind in ("masks", "scores") and own and rng.random() < 0.5:     # R7: a setter between the pass and its fetch
        g = kind == "masks"
        cur = (m.groups if g else m.weights)[2]
        other = [k for k in (GKEYS if g else WKEYS) if k != cur][0]
        return [dict(op="set_groups" if g else "set_weights", key=other, ns="ok"), _late_fetch(rng, FETCH_OF[kind], slot),
                dict(op=kind, slot=slot, out="own", heap="own", nd="ok"), _late_fetch(rng, FETCH_OF[kind], slot)]
    if kind == "select_docs" and own and rng.random() < 0.8:            # R10
        return [dict(op="sel_scores", slot=slot, src="own", out="own"), dict(op="top", slot=slot, src="own", rule=0, k=65, flags=4, nd="ok", out="own"),
                _late_fetch(rng, "scores_fetch", slot)]
    if kind == "top" and own and rng.random() < 0.4:                    # R3: a matching call leaves the pairs alone
        return [dict(op="match_scores", slot=slot, src="own", rule=1, nd="ok", out="own"), _late_fetch(rng, "top_fetch", slot)]
    return agenda


NEEDS_SEG = ("matching", "context")


def plan(seed, n_ops=PLAN_OPS):
    """The plan of `seed`: a list of operations (dicts).  Deterministic; the model decides what each one is worth.  A
    plan with fewer than MIN_VERDICT_OPS verdict operations is rejected here."""
    rng = np.random.default_rng([seed, 0x56455244494354])
    m = Model()
    turn = {"seed": seed}
    ops = []
    agenda = []
    if rng.random() < 0.5:                                      # a fetch, a setter or a pass before anything was made: PFAC_E_STATE
        agenda.append([dict(op="ids_fetch", slot=0), dict(op="set_weights", key="w0", ns="ok"), dict(op="top_fetch", slot=1, first=0, n=1),
                       dict(op="set_groups", key="g1", ns="ok")][int(rng.integers(0, 4))])
    if rng.random() < 0.5:
        agenda.append(dict(op="set_stream", slot=1, share=True))
    agenda += _ground(rng, 0)
    if rng.random() < 0.35:                                     # zero documents on an empty owned range, through every pass
        z = int(rng.integers(0, N_SLOTS))
        agenda += [lambda m: dict(op="scan", slot=z, inp=0, no=0), lambda m: dict(op="set_doc", slot=z, tab=m.tab, inp=0, form="zero"),
                   dict(op="masks", slot=z, out="own", heap="own", nd="ok"), dict(op="scores", slot=z, out="own", heap="own", nd="ok"),
                   dict(op="top", slot=z, src="own", rule=0, k=U64_MAX, flags=4, nd="ok", out="own"),
                   dict(op="gather_format", slot=z, ids="own", ni="ok", out="own", f=2 if rng.random() < 0.5 else 1),
                   dict(op="ga_fetch", slot=z, first=0, n=0), dict(op="gaoff_fetch", slot=z)]
    tries = 0
    while len(ops) < n_ops:
        tries += 1
        assert tries < 40 * n_ops, "the plan does not advance"
        want_err = rng.random() < 1 / 8
        chosen = None
        while agenda and chosen is None and not want_err:
            cand = agenda.pop(0)
            cand = cand(m) if callable(cand) else cand
            if cand is not None:
                cand = _fix_table(cand)
                if m.predict(cand).status is not None:
                    chosen = cand
        for _ in range(60):
            if chosen is not None:
                break
            cand = _propose(rng, m)
            st = m.predict(cand).status
            if st is None:
                continue
            if (st != OK) == want_err:
                chosen = cand
            elif st != OK and not agenda and cand["op"] in VERDICT_OPS and cand["op"] not in ("set_groups", "set_weights") and not cand["op"].endswith("_fetch"):
                # a verdict call with nothing to stand on: do what is missing first, then the call
                agenda = _ground(rng, cand["slot"], "seg" if cand["op"] in NEEDS_SEG else "docs") + [cand]
        if chosen is None:
            continue
        st = m.apply(chosen).status
        ops.append(chosen)
        agenda = _agenda(rng, m, chosen, st, agenda, turn)
    n_verdict = sum(op["op"] in VERDICT_OPS for op in ops)
    assert n_verdict >= MIN_VERDICT_OPS, f"plan {seed} holds {n_verdict} verdict operations, fewer than {MIN_VERDICT_OPS}"
    return ops


def shrink(seed, k, n_ops=PLAN_OPS):
    """The plan of `seed` with operation k onwards removed: cut a failing history down by hand."""
    return plan(seed, n_ops)[:k]


# ---------------------------------------------------------------------------
# the executor

class _Bufs:
    def __init__(self):
        self.inp = self.rec = None                              # the caller's input and heap of a scan_over
        self.sel = self.sel_first = None                        # the caller's buffers of the last selection into them
        self.masks = self.scores = None                         # ... of the last mask / score call into one
        self.live = []                                          # every guarded buffer a later call may still read


def _flags(flags):
    return dict(by="count" if flags & topref.BY_COUNT else "score", lowest=bool(flags & topref.LOWEST), ranked=bool(flags & topref.RANKED))


class Executor:
    def __init__(self, g, model):
        self.g, self.m = g, model
        self.x = model.x
        self.bufs = [_Bufs() for _ in range(N_SLOTS)]
        self.stats = dict(ops=0, errors=0, verdict=0, statuses=set(), widths=set(), rules={r: 0 for r in RULES}, late=set(), docs=0, bytes=0)

    def step(self, op):
        exp = self.m.apply(op)
        assert exp.status is not None, "the contract does not decide this operation: a plan must not contain it"
        self.stats["ops"] += 1
        self.stats["verdict"] += op["op"] in VERDICT_OPS
        self.stats["statuses"].add(exp.status)
        try:
            got = getattr(self, "do_" + op["op"])(op, exp)
        except PfacError as e:
            assert e.status == exp.status, f"raised {e} (status {e.status}), want {STATUS_NAMES[exp.status]}"
            if exp.count is not None:
                n = [getattr(e, a) for a in ("n_matching", "n_top", "out_bytes") if hasattr(e, a)]
                assert n == [exp.count], f"the overflow error carries {n}, want [{exp.count}]"
            self.stats["errors"] += 1
            self._observed(exp)
            return exp.status
        assert exp.status == OK, f"returned normally, want {STATUS_NAMES[exp.status]}"
        _same(got, exp.value())
        self._observed(exp)
        return OK

    def _observed(self, exp):
        for r in exp.rules:
            self.stats["rules"][r] += 1
        self.stats["late"].update(exp.late)

    def _guarded(self, outs, call):
        """Run `call` with the caller's outputs `outs` (name -> _OutBuf): their guard bands hold whatever it returns, and
        a refused call leaves their payload as it was."""
        try:
            r = call()
        except PfacError:
            for name, b in outs.items():
                b.check(name, untouched=True)
            raise
        self.g.sync(0)
        self.g.sync(1)
        for name, b in outs.items():
            b.check(name)
        return r

    # -- what the verdicts stand on -----------------------------------------
    def do_load_table(self, op, exp):
        import os
        saved = {k: os.environ.get(k) for k in KNOB_NAMES}
        for k in saved:
            os.environ.pop(k, None)
        os.environ.update(KNOBS[op["knob"]])                    # knobs are read when a table is installed
        try:
            self.g.load_table(self.x.table(op["tab"]))
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v

    def do_set_flen(self, op, exp):
        t = self.m.tab                                          # (an argument of the call, as a caller makes it; no expectation reads it)
        self.g.set_final_lengths(self.x.table(t).final_lengths() if t else np.ones(1, np.int32))

    def _setter(self, op, fn, raw):
        tab = self.m.tab or "abc2"
        if op["ns"] == "ok" and self.m.tab is not None:
            return fn(self.x.setter_arg(tab, op["key"]))
        return raw(tab, op["key"], op["ns"])

    def do_set_groups(self, op, exp):
        def raw(tab, key, ns):
            masks = self.x.table(tab).state_group_masks(self.x.setter_arg(tab, key))
            return _raw_setter(self.g, "groups", np.append(masks, np.uint64(0)) if ns != "ok" else masks)
        self._setter(op, self.g.set_pattern_groups, raw)

    def do_set_weights(self, op, exp):
        def raw(tab, key, ns):
            w = np.ascontiguousarray(self.x.table(tab).state_weights(self.x.setter_arg(tab, key)), dtype=np.int32)
            return _raw_setter(self.g, "weights", np.append(w, np.int32(0)) if ns != "ok" else w)
        self._setter(op, self.g.set_pattern_weights, raw)

    def do_scan(self, op, exp):
        g, slot = self.g, op["slot"]
        t, i = self.m.slots[slot].inp
        data = self.x.input(t, i)
        self.bufs[slot].inp = self.bufs[slot].rec = None
        g.reserve(slot, data.size, max(data.size // 8, 4096))
        g.h2d(data, slot)
        n = g.scan_resident(0 if op["no"] == 0 else data.size, data.size, slot=slot)
        self.stats["widths"].add(int(g.scan_format(slot)[0]))
        assert int(g.scan_format(slot)[0]) == record_width(int(self.x.table(t).num_final), KNOBS[self.m.knob]), "record width"
        return int(n)

    def do_scan_over(self, op, exp):
        g, slot = self.g, op["slot"]
        data = self.x.input(*self.m.slots[slot].scan["sk"][:2])
        b = self.bufs[slot]
        b.inp, b.rec = _upload(g, data), _alloc(g, 16 * 8 + 64)
        g.scan_async(data.size, data.size, d_input=b.inp, d_records=b.rec, capacity=16, slot=slot)
        n, over = g.scan_finish(slot, allow_overflow=True)
        return int(n), bool(over)

    def do_filter(self, op, exp):
        b = self.bufs[op["slot"]]
        return int(self.g.filter_whole_words(op["slot"], d_input=b.inp, d_records=b.rec))

    def do_split(self, op, exp):
        slot = op["slot"]
        return tuple(int(v) for v in self.g.split_documents(self.x.input_size(*self.m.slots[slot].inp), b"\n", slot=slot))

    def do_set_doc(self, op, exp):
        self.g.set_doc_offsets(self.x.offsets((op["tab"], op["inp"], op["form"])), op["slot"])

    def do_segment(self, op, exp):
        return int(self.g.segment_records(self.nd, slot=op["slot"], d_records=self.bufs[op["slot"]].rec))

    def do_select_docs(self, op, exp):
        g, slot, nd = self.g, op["slot"], self.nd
        b = self.bufs[slot]
        if op["out"] == "own" or exp.status != OK:
            return int(g.select_leftmost_longest_documents(nd, slot=slot, d_records=b.rec))
        n = int(exp.value())
        b.sel, b.sel_first = _OutBuf(g, n * 8), _OutBuf(g, (nd + 1) * 8)
        return int(self._guarded({"d_out": b.sel, "d_doc_first": b.sel_first}, lambda: g.select_leftmost_longest_documents(
            nd, d_out=b.sel.ptr, out_cap=n, d_doc_first=b.sel_first.ptr, slot=slot, d_records=b.rec)))

    def do_reserve_grow(self, op, exp):
        self.g.reserve(op["slot"], op["k"] * IN_STEP, op["k"] * REC_STEP)
        self.bufs[op["slot"]].inp = self.bufs[op["slot"]].rec = None

    def do_set_stream(self, op, exp):
        self.g.set_stream(1, self.g.stream_handle(0) if op["share"] else 0)

    def do_sync(self, op, exp):
        self.g.sync(op["slot"])

    # -- masks and scores ---------------------------------------------------
    def _heap(self, op):
        b = self.bufs[op["slot"]]
        return _alloc(self.g, 4096) if op["heap"] == "foreign" else b.rec

    def _pass_out(self, op, exp, width, call, read, attr):
        """A mask / score pass: out "own" = NULL, "caller" = a guarded buffer of exactly n_docs x width bytes, "odd" = four
        bytes into one."""
        g, nd = self.g, self.nd + (op.get("nd") == "more")
        if op["out"] == "own":
            return call(nd, None)
        buf = _OutBuf(g, max(nd, 1) * width if op["out"] == "odd" else nd * width)
        r = self._guarded({"d_out": buf}, lambda: call(nd, _odd(g, buf.ptr) if op["out"] == "odd" else buf.ptr))
        setattr(self.bufs[op["slot"]], attr, buf)
        return r, read(buf, nd)

    def do_masks(self, op, exp):
        g, slot, heap = self.g, op["slot"], self._heap(op)
        r = self._pass_out(op, exp, 8, lambda nd, out: int(g.document_group_masks(nd, d_out=out, slot=slot, d_records=heap)),
                           lambda buf, nd: buf.read(np.uint64, nd), "masks")
        self.stats["docs"] += self.nd
        return (r,) if op["out"] == "own" else (r[0], r[1])

    def do_scores(self, op, exp):
        g, slot, heap = self.g, op["slot"], self._heap(op)
        r = self._pass_out(op, exp, 16, lambda nd, out: tuple(int(v) for v in g.document_scores(nd, d_out=out, slot=slot, d_records=heap)),
                           lambda buf, nd: buf.read(scoreref.SCORE, nd), "scores")
        self.stats["docs"] += self.nd
        return r if op["out"] == "own" else r[0] + pairs(r[1])

    def do_sel_scores(self, op, exp):
        g, slot = self.g, op["slot"]
        b, sel = self.bufs[slot], self.sel_before
        nd = sel["nd"] if sel is not None else max(self.nd, 1)
        d_sel, d_first = (None, None)
        if op["src"] == "half":
            d_first = (b.sel_first.ptr if b.sel_first is not None else _alloc(g, (nd + 1) * 8))
        elif op["src"] == "caller":
            d_sel, d_first = b.sel.ptr, b.sel_first.ptr
        if op["out"] == "own":
            return tuple(int(v) for v in g.selection_document_scores(nd, d_sel=d_sel, d_doc_first=d_first, slot=slot))
        buf = _OutBuf(g, nd * 16)
        tot = self._guarded({"d_out": buf}, lambda: tuple(int(v) for v in g.selection_document_scores(nd, d_sel=d_sel, d_doc_first=d_first, d_out=buf.ptr, slot=slot)))
        b.scores = buf
        return tot + pairs(buf.read(scoreref.SCORE, nd))

    def do_masks_fetch(self, op, exp):
        return self.g.group_masks_to_host(0, op["slot"], first=op["first"], n=op["n"])

    def do_scores_fetch(self, op, exp):
        return pairs(self.g.document_scores_to_host(0, op["slot"], first=op["first"], n=op["n"]))

    def do_top_fetch(self, op, exp):
        return pairs(self.g.top_scores_to_host(op["n"], op["slot"], first=op["first"]))

    # -- producers ------------------------------------------------------------
    def _ids_out(self, op, exp, call, width2=0):
        """A producer: out "own" = NULL, "caller" = guarded buffers of exactly the count (ids, and `width2` > 0: pairs),
        "small" = one entry fewer."""
        g = self.g
        if op["out"] == "own":
            return (int(call(None, 0, None)),)
        want = exp.count if exp.count is not None else (int(exp.value()[0]) if exp.status == OK else 4)
        cap = want - 1 if op["out"] == "small" else want
        ids, prs = _OutBuf(g, cap * 8), _OutBuf(g, cap * 16) if width2 else None
        outs = {"d_ids_out": ids, **({"d_top_scores": prs} if prs is not None else {})}
        n = int(self._guarded(outs, lambda: call(ids.ptr, cap, prs.ptr if prs is not None else None)))
        self.stats["docs"] += n
        return (n, ids.read(np.uint64, n)) + (pairs(prs.read(scoreref.SCORE, n)) if prs is not None else ())

    def _n(self, op, n):
        return n + (op.get("nd") == "more")

    def do_matching(self, op, exp):
        g, slot, nd = self.g, op["slot"], self._n(op, self.seg_nd)
        return self._ids_out(op, exp, lambda out, cap, _: g.matching_documents(nd, invert=op["invert"], d_out=out, out_cap=cap, slot=slot))

    def do_context(self, op, exp):
        g, slot, nd = self.g, op["slot"], self._n(op, self.seg_nd)
        return self._ids_out(op, exp, lambda out, cap, _: g.matching_documents(nd, d_out=out, out_cap=cap, slot=slot, before=op["before"], after=op["after"]))

    def _given(self, op, res):
        """(device pointer or None, n_docs) of the masks / scores a consumer is given."""
        slot = op["slot"]
        if op["src"] == "own":
            r = self.res_before[res]
            return None, self._n(op, r["n"] if r is not None else 1)
        return getattr(self.bufs[slot], res).ptr, self.c_before[res][1]

    def do_match_groups(self, op, exp):
        g, slot = self.g, op["slot"]
        d_masks, nd = self._given(op, "masks")
        return self._ids_out(op, exp, lambda out, cap, _: g.matching_documents_where(nd, **PREDS[op["pred"]], d_masks=d_masks, d_out=out, out_cap=cap, slot=slot))

    def do_match_scores(self, op, exp):
        g, slot = self.g, op["slot"]
        d_scores, nd = self._given(op, "scores")
        return self._ids_out(op, exp, lambda out, cap, _: g.matching_documents_scored(nd, **SCORE_RULES[op["rule"]], d_scores=d_scores, d_out=out, out_cap=cap, slot=slot))

    def do_top(self, op, exp):
        g, slot = self.g, op["slot"]
        d_scores, nd = self._given(op, "scores")
        kw = dict(_flags(op["flags"]), **(SCORE_RULES[op["rule"]] or {}))
        return self._ids_out(op, exp, lambda out, cap, prs: g.top_documents(nd, op["k"], **kw, d_scores=d_scores, d_out=out, out_cap=cap, d_top_scores=prs, slot=slot), 16)

    def do_ids_fetch(self, op, exp):
        r = self.res_before["ids"]
        got = self.g.matching_documents_to_host(r["n"] if r is not None else 1, op["slot"])
        self.stats["docs"] += int(got.size)
        return got

    # -- the gathers ----------------------------------------------------------
    def do_gather(self, op, exp, f=None):
        g, slot = self.g, op["slot"]
        nd, nb = max(self.nd, 0) if self.m_docs is not None else 1, self.x.input_size(*self.m.slots[slot].inp)
        r = self.res_before["ids"]
        if op["ids"] == "own":
            d_ids, n_ids = None, (r["n"] if r is not None else 1) + (op["ni"] != "ok")
        else:
            ids = self.x.id_list(None, op["ids"], nd)
            d_ids, n_ids = _upload(g, ids), int(ids.size)
            self.bufs[slot].live.append(d_ids)
        kw = {} if f is None else {k: v for k, v in FMTS[f].kwargs().items()}
        call = g.gather_documents if f is None else g.gather_documents_formatted
        if op["out"] == "own":
            n = int(call(nd, n_ids, nb, d_ids=d_ids, slot=slot, **kw))
            self.stats["bytes"] += n
            return (n,)
        want = exp.count if exp.count is not None else (int(exp.value()[0]) if exp.status == OK else 64)
        cap = want - 1 if op["out"] == "small" else want
        out, oo = _OutBuf(g, cap), _OutBuf(g, (n_ids + 1) * 8)
        n = int(self._guarded({"d_out": out, "d_out_offsets": oo}, lambda: call(nd, n_ids, nb, d_ids=d_ids, d_out=out.ptr, out_cap=cap,
                                                                                  d_out_offsets=oo.ptr, slot=slot, **kw)))
        self.stats["bytes"] += n
        return n, out.read(np.uint8, n).tobytes(), oo.read(np.uint64, n_ids + 1)

    def do_gather_format(self, op, exp):
        return self.do_gather(op, exp, op["f"])

    def do_ga_fetch(self, op, exp):
        return self.g.gathered_to_host(op["n"], op["slot"], first=op["first"]).tobytes()

    def do_gaoff_fetch(self, op, exp):
        r = self.res_before["ga"]
        n_ids = int(self.x.value(r["key"])[1].size) - 1 if r is not None else 1
        return self.g.gathered_offsets_to_host(n_ids, op["slot"])


def _raw_setter(g, what, arr):
    """pfac_table_set_state_groups / _weights themselves, for an n_states the wrapper would not pass and before any
    upload."""
    if hasattr(g, "raw_setter"):
        return g.raw_setter(what, arr)
    fn = g._L.pfac_table_set_state_groups if what == "groups" else g._L.pfac_table_set_state_weights
    g._check(fn(g._ctx, arr.ctypes.data if arr.size else None, arr.size))


def run(g, ops, model=None, seed=None):
    """Performs `ops` on `g` (one context, never re-created), comparing every result with `model` bit for bit; no
    operation is skipped.  Returns the executor's statistics; raises AssertionError naming the seed, the operation and
    the ten before it."""
    ex = Executor(g, model or Model())
    for k, op in enumerate(ops):
        s = ex.m.slots[op.get("slot", 0)]
        # what the call's arguments are made from: the slot's state BEFORE the call
        ex.m_docs = s.docs
        ex.nd = ex.x.n_docs(s.docs) if s.docs is not None else 1
        ex.seg_nd = int(ex.x.value(s.seg).size) - 1 if s.seg is not None else 1
        ex.sel_before = s.sel
        ex.res_before = {r: getattr(s, r) for r in RESULTS}
        ex.c_before = dict(masks=s.cmasks, scores=s.cscores)
        try:
            ex.step(op)
        except AssertionError as e:
            hist = "\n".join(f"    {j:3d}  {fmt(ops[j])}" for j in range(max(0, k - 10), k + 1))
            e2 = AssertionError(f"verdict session seed {seed}, operation {k} {fmt(op)}: {e}\n  the operations up to it (cut the plan with "
                                f"verdictsession.shrink({seed}, k)):\n{hist}")
            e2.op_index = k
            raise e2 from e
    return ex.stats
