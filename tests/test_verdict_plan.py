"""CPU side of the verdict session tests (tests/verdictsession.py): the 24 plans are pinned by digest, hold what they
must (every operation kind legal and refused, every producer of ids in front of every consumer, every rule R1 .. R10
deciding an outcome in at least three plans, every slot-owned result read behind every event of R9), and run -- through
the same `run` as on the GPU -- against CpuVerdictDevice, a stand-in for GpuMatcher that implements the contract of
include/pfac.h in the most obvious way from the same references.  Each of the stand-in's switchable defects, one per
rule at least, makes a committed plan fail: the harness has teeth without a kernel being mutated.  The reach table and
the plan and operation that caught each defect are printed (pytest -s shows them)."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest

import groupref
import scoreref
import session as S
import topref
import verdictsession as V
from docreplref import per_doc
from fmtref import Fmt, format_ref
from gatherref import context_ids, gather_ref
from passfuzz import KNOBS, record_width
from phfpfac_amd import PfacError
from splitref import matching_ids, split_offsets

X = V.pool()


def _err(status, msg, **attrs):
    e = PfacError(status, msg)
    for k, v in attrs.items():
        setattr(e, k, v)
    return e


class CpuBuf:
    def __init__(self, n_bytes, src=None):
        self.a = np.zeros(max(int(n_bytes), 16), dtype=np.uint8)
        self.src = src

    def put(self, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
        self.a[:raw.size] = raw

    def get(self, dtype, n):
        return self.a[:int(n) * np.dtype(dtype).itemsize].view(dtype).copy()


class _Slot:
    def __init__(self):
        self.in_cap = self.rec_cap = 0
        self.data = self.scan = self.off = self.seg = self.sel = None
        self.serial = 0
        self.ids = self.masks = self.scores = self.top = self.ga = None
        self.heap = CpuBuf(16)


DEFECTS = {
    "failed_producer_keeps_the_ids": "R1", "gather_sorts_ranked_ids": "R2", "top_returns_tied_ids_unordered": "R2",
    "matching_drops_the_top_pairs": "R3", "caller_mask_call_leaves_slot_masks_own": "R4", "caller_score_call_leaves_slot_scores_own": "R5",
    "sel_scores_keep_the_heap_scores": "R5", "gather_format_keeps_plain_offsets": "R6", "upload_keeps_the_weights": "R7",
    "setter_reaches_a_queued_pass": "R7", "wrong_n_states_clears_the_groups": "R7", "arg_judged_before_state": "R8",
    "fetch_behind_reserve_returns_zeros": "R9", "ids_lost_at_new_offsets": "R9", "sel_scores_accept_a_stale_selection": "R10",
}


class CpuVerdictDevice:
    """GpuMatcher's surface, as far as the verdict sessions use it, on the CPU.  `defects`: names from DEFECTS."""
    states_are_ids = True
    device = 0

    def __init__(self, defects=()):
        self.defects = set(defects)
        self.hit = False
        self.tab = self.table = None
        self.gen = 0
        self.width = 4
        self.flen = False
        self.groups = self.weights = None                       # (key-free: the arrays by pattern id)
        self.slots = [_Slot() for _ in range(S.N_SLOTS)]

    def _defect(self, name):
        if name in self.defects:
            self.hit = True
            return True
        return False

    def alloc(self, n_bytes):
        return CpuBuf(n_bytes)

    def upload(self, arr):
        b = CpuBuf(arr.nbytes + 64, src=arr)
        b.put(arr)
        return b

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    # -- the table and what belongs to it -------------------------------------
    def load_table(self, table):
        self.tab = next(t for t in V.VTABLES if X.table(t) is table)
        self.table = table
        self.gen += 1
        knobs = {k: os.environ[k] for d in KNOBS for k in d if k in os.environ}
        self.width = record_width(int(table.num_final), knobs)
        self.flen, self.groups = False, None
        if self.weights is not None and self._defect("upload_keeps_the_weights"):
            self.weights = np.resize(self.weights, X.n_ids(self.tab) + 1)     # (the stale array, read at the new table's length)
        else:
            self.weights = None

    def set_final_lengths(self, lengths):
        if self.tab is None:
            raise _err(S.E_STATE, "no table")
        self.flen = True

    def set_pattern_groups(self, groups):
        if self.tab is None:
            raise _err(S.E_STATE, "no table")
        self.groups = groupref.masks_by_id(groups)
        if "setter_reaches_a_queued_pass" in self.defects:
            self._requeue("masks")

    def set_pattern_weights(self, weights):
        if self.tab is None:
            raise _err(S.E_STATE, "no table")
        self.weights = scoreref.w_by_id(weights)
        if "setter_reaches_a_queued_pass" in self.defects:
            self._requeue("scores")

    def _requeue(self, res):
        for s in self.slots:
            r = getattr(s, res)
            if r is not None and r.get("again") is not None:
                v = r["again"]()
                if v is not None and (v.size != r["v"].size or v.tobytes() != r["v"].tobytes()):
                    self.hit = True
                    r["v"] = v

    def raw_setter(self, what, arr):
        if self.tab is None:
            raise _err(S.E_STATE, "no table")
        assert arr.size != int(self.table.num_final)
        if what == "groups" and self.groups is not None and self._defect("wrong_n_states_clears_the_groups"):
            self.groups = None
        raise _err(S.E_ARG, "n_states is not num_final")

    # -- plumbing ---------------------------------------------------------------
    def reserve(self, slot=0, input_bytes=0, record_capacity=0):
        s = self.slots[slot]
        if (input_bytes > s.in_cap and s.in_cap) or (record_capacity > s.rec_cap and s.rec_cap):
            s.scan = s.data = None
            if "fetch_behind_reserve_returns_zeros" in self.defects:
                for r in V.RESULTS:
                    if getattr(s, r) is not None:
                        getattr(s, r)["zero"] = True
        s.in_cap, s.rec_cap = max(s.in_cap, input_bytes), max(s.rec_cap, record_capacity)

    def h2d(self, host, slot=0, dst_offset=0):
        self.slots[slot].data = host

    def sync(self, slot=0):
        pass

    def stream_handle(self, slot=0):
        return 1 + slot

    def set_stream(self, slot, handle):
        pass

    # -- scans --------------------------------------------------------------------
    def _scan(self, s, data, no, cap, heap, ext):
        if self.tab is None:
            raise _err(S.E_STATE, "scan before a table upload")
        i = next(i for i in range(3) if X.input(self.tab, i) is data)
        sk = (self.tab, i, no, False)
        s.serial += 1
        s.scan = dict(sk=sk, gen=self.gen, width=self.width, over=X.rows(sk)[0].size > cap, heap=heap, ext=ext)
        return int(X.rows(sk)[0].size)

    def scan_resident(self, n_owned, n_avail=None, d_input=None, slot=0):
        s = self.slots[slot]
        return self._scan(s, s.data, n_owned, 1 << 62, s.heap, False)

    def scan_async(self, n_owned, n_avail=None, d_input=None, d_records=None, capacity=0, slot=0):
        self._scan(self.slots[slot], d_input.src, n_owned, capacity, d_records, True)

    def scan_finish(self, slot=0, allow_overflow=False):
        sc = self.slots[slot].scan
        return int(X.rows(sc["sk"])[0].size), sc["over"]

    def scan_format(self, slot=0):
        sc = self.slots[slot].scan
        return sc["width"], (sc["sk"][2] + 4095) // 4096, 0

    def _ladder(self, s, n_docs, need=None, d_records=None, out=None, cut=False):
        """The rungs of a pass over the slot's scan and offsets, in the header's order (`cut`: the segment pass and the
        selection, which judge the scan's overflow before they look for offsets)."""
        sc = s.scan
        if cut and sc is not None and sc["gen"] == self.gen and self.flen and sc["over"]:
            raise _err(S.E_OVERFLOW, "the scan overflowed")
        state = (sc is None or sc["gen"] != self.gen or not self.flen or (need == "groups" and self.groups is None)
                 or (need == "weights" and self.weights is None) or s.off is None or n_docs != s.off.size - 1)
        arg = isinstance(out, S.Odd) or (sc is not None and not (d_records is sc["heap"] or (d_records is None and not sc["ext"])))
        if state and arg and self._defect("arg_judged_before_state"):
            raise _err(S.E_ARG, "bad argument")
        if state:
            raise _err(S.E_STATE, "call order")
        if sc["over"]:
            raise _err(S.E_OVERFLOW, "the scan overflowed")
        if arg or not S.offsets_ok(s.off, sc["sk"][2]):
            raise _err(S.E_ARG, "bad argument")
        pos, lens, idx = X.rows(sc["sk"])
        return pos, lens, idx, s.off.astype(np.int64)

    def filter_whole_words(self, slot=0, word_bytes=None, edges="both", prev_byte=-1, next_byte=-1, n_docs=0, d_doc_offsets=None,
                           d_input=None, d_records=None):
        s = self.slots[slot]
        sc = s.scan
        if sc is None or sc["gen"] != self.gen or not self.flen:
            raise _err(S.E_STATE, "call order")
        if sc["over"]:
            raise _err(S.E_OVERFLOW, "the scan overflowed")
        s.scan = dict(sc, sk=sc["sk"][:3] + (True,))
        s.serial += 1
        return int(X.rows(s.scan["sk"])[0].size)

    # -- offsets, segment, selection ------------------------------------------------
    def split_documents(self, n_bytes, delimiter=b"\n", d_input=None, slot=0):
        s = self.slots[slot]
        off, nd, tail = split_offsets(s.data[:n_bytes], 10)
        self._new_offsets(s, off)
        return nd, tail

    def set_doc_offsets(self, offsets, slot=0):
        self._new_offsets(self.slots[slot], np.ascontiguousarray(offsets, dtype=np.uint64))

    def _new_offsets(self, s, off):
        s.off = off
        if s.ids is not None and self._defect("ids_lost_at_new_offsets"):
            s.ids = None

    def segment_records(self, n_docs, d_doc_offsets=None, d_out=None, out_cap=0, d_doc_first=None, slot=0, d_records=None):
        s = self.slots[slot]
        s.seg = None
        pos, lens, idx, off = self._ladder(s, n_docs, d_records=d_records, cut=True)
        sc = scoreref.scores_cut(pos, np.arange(pos.size), lens, off, np.zeros(pos.size, dtype=np.int64))
        s.seg = np.concatenate(([0], np.cumsum(sc["count"].astype(np.int64)))).astype(np.uint64)
        return int(s.seg[-1])

    def select_leftmost_longest_documents(self, n_docs, d_doc_offsets=None, d_out=None, out_cap=0, d_doc_first=None, slot=0, d_records=None):
        s = self.slots[slot]
        s.sel = None
        pos, lens, idx, off = self._ladder(s, n_docs, d_records=d_records, cut=True)
        first, idx = V.select_walk(pos, lens, off, idx, s.scan["sk"][2])
        own = d_out is None
        if not own:
            d_out.put(idx.astype(np.uint64))                    # (the stand-in's records: the index of each pick)
            d_doc_first.put(first)
        s.sel = dict(first=first, idx=idx, serial=s.serial, gen=self.gen, own=own, t=s.scan["sk"][:2])
        return int(first[-1])

    # -- masks and scores ---------------------------------------------------------------
    def _per_record(self, t, i, by_id, is_mask):
        _, _, starts, fids = X._whole(t, i)
        v = by_id[fids]
        if starts.size == 0:
            return v[:0]
        return np.bitwise_or.reduceat(v, starts) if is_mask else np.add.reduceat(v, starts)

    def document_group_masks(self, n_docs, d_doc_offsets=None, d_out=None, slot=0, d_records=None):
        s = self.slots[slot]
        old, s.masks = s.masks, None
        pos, lens, idx, off = self._ladder(s, n_docs, "groups", d_records, d_out)
        t, i = s.scan["sk"][:2]
        gen = self.gen

        def make():
            if self.groups is None or gen != self.gen:
                return None
            return groupref.masks_cut(pos, np.arange(pos.size), lens, off, self._per_record(t, i, self.groups, True)[idx])
        m = make()
        if d_out is None:
            s.masks = dict(v=m, again=make)
        else:
            d_out.put(m)
            if old is not None and self._defect("caller_mask_call_leaves_slot_masks_own"):
                s.masks = old
        return int(np.bitwise_or.reduce(m, initial=np.uint64(0)))

    def document_scores(self, n_docs, d_doc_offsets=None, d_out=None, slot=0, d_records=None):
        s = self.slots[slot]
        old, s.scores = s.scores, None
        pos, lens, idx, off = self._ladder(s, n_docs, "weights", d_records, d_out)
        t, i = s.scan["sk"][:2]
        gen = self.gen

        def make():
            if self.weights is None or gen != self.gen:
                return None
            return scoreref.scores_cut(pos, np.arange(pos.size), lens, off, self._per_record(t, i, self.weights, False)[idx])
        sc = make()
        if d_out is None:
            s.scores = dict(v=sc, again=make)
        else:
            d_out.put(sc)
            if old is not None and self._defect("caller_score_call_leaves_slot_scores_own"):
                s.scores = old
        return scoreref.totals(sc)

    def selection_document_scores(self, n_docs, d_sel=None, d_doc_first=None, d_out=None, slot=0):
        s = self.slots[slot]
        old = s.scores
        if not (old is not None and "sel" not in old and self._defect("sel_scores_keep_the_heap_scores")):
            s.scores = None
        else:
            old = None
        if self.tab is None or self.weights is None:
            raise _err(S.E_STATE, "no weights")
        if (d_sel is None) != (d_doc_first is None):
            raise _err(S.E_ARG, "one pointer NULL and the other not")
        sel = s.sel
        if d_sel is None:
            stale = sel is not None and sel["own"] and sel["gen"] == self.gen and sel["serial"] != s.serial
            if sel is None or not sel["own"] or sel["gen"] != self.gen or (stale and not self._defect("sel_scores_accept_a_stale_selection")):
                raise _err(S.E_STATE, "no selection")
            first, idx = sel["first"], sel["idx"]
        else:
            first = d_doc_first.get(np.uint64, n_docs + 1)
            idx = d_sel.get(np.uint64, int(first[-1])).astype(np.int64)
        sc = scoreref.scores_of_selection(first, idx, self._per_record(sel["t"][0], sel["t"][1], self.weights, False))
        if d_out is None:
            s.scores = dict(v=sc, again=None, sel=True)
        else:
            d_out.put(sc)
        return scoreref.totals(sc)

    def _fetch(self, s, res, first, n, take=lambda v: v):
        r = getattr(s, res)
        if r is None:
            raise _err(S.E_STATE, "nothing to fetch")
        v = take(r["v"])
        if first + n > v.size:
            raise _err(S.E_ARG, "window past the end")
        out = v[first:first + n].copy()
        if r.get("zero") and out.size and out.tobytes() != bytes(out.nbytes):
            self.hit = True
            out = np.zeros_like(out)
        return out

    def group_masks_to_host(self, n_docs, slot=0, first=0, n=None):
        return self._fetch(self.slots[slot], "masks", first, n)

    def document_scores_to_host(self, n_docs, slot=0, first=0, n=None):
        return self._fetch(self.slots[slot], "scores", first, n)

    def top_scores_to_host(self, n, slot=0, first=0):
        return self._fetch(self.slots[slot], "top", first, n)

    # -- the producers of ids -------------------------------------------------------------
    def _produce(self, s, old, fn, d_out, out_cap, attr, d_top=None):
        try:
            ids, prs = fn()
            if (d_out is not None or d_top is not None) and out_cap < ids.size:
                raise _err(S.E_OVERFLOW, "out_cap too small", **{attr: int(ids.size)})
        except PfacError:
            if old is not None and self._defect("failed_producer_keeps_the_ids"):
                s.ids = old
            raise
        if d_out is None:
            s.ids = dict(v=ids, ranked=prs is not None and bool(np.any(ids[1:] < ids[:-1])))
            if prs is not None:
                s.top = dict(v=prs)
        else:
            d_out.put(ids)
            if prs is not None:
                d_top.put(prs)
        return int(ids.size)

    def matching_documents(self, n_docs, invert=False, d_doc_first=None, d_out=None, out_cap=0, slot=0, before=0, after=0):
        s = self.slots[slot]
        old, s.ids = s.ids, None
        if s.top is not None and self._defect("matching_drops_the_top_pairs"):
            s.top = None

        def fn():
            if s.seg is None:
                raise _err(S.E_STATE, "no segment")
            if n_docs != s.seg.size - 1:
                raise _err(S.E_ARG, "n_docs")
            return (context_ids(s.seg, before, after) if before or after else matching_ids(s.seg, invert)), None
        return self._produce(s, old, fn, d_out, out_cap, "n_matching")

    def _given(self, s, res, d, n_docs, dtype):
        if d is not None:
            return d.get(dtype, n_docs)
        r = getattr(s, res)
        if r is None:
            raise _err(S.E_STATE, "no slot-owned " + res)
        if n_docs != r["v"].size:
            raise _err(S.E_ARG, "n_docs")
        return r["v"]

    def matching_documents_where(self, n_docs, all_of=0, any_of=0, none_of=0, invert=False, d_masks=None, d_out=None, out_cap=0, slot=0):
        s = self.slots[slot]
        old, s.ids = s.ids, None
        return self._produce(s, old, lambda: (groupref.predicate(self._given(s, "masks", d_masks, n_docs, np.uint64), all_of, any_of, none_of, invert), None),
                             d_out, out_cap, "n_matching")

    def _candidates(self, s, sc, n_docs, rule):
        off = None
        if rule.get("density") is not None:
            if s.off is None:
                raise _err(S.E_STATE, "no offsets")
            if s.off.size - 1 != n_docs:
                raise _err(S.E_ARG, "n_docs")
            off = s.off
        return scoreref.predicate(sc, off, **rule)

    def matching_documents_scored(self, n_docs, min_score=None, max_score=None, min_count=None, max_count=None, density=None, invert=False,
                                  d_scores=None, d_doc_offsets=None, d_out=None, out_cap=0, slot=0):
        s = self.slots[slot]
        old, s.ids = s.ids, None
        rule = dict(min_score=min_score, max_score=max_score, min_count=min_count, max_count=max_count, density=density, invert=invert)
        return self._produce(s, old, lambda: (self._candidates(s, self._given(s, "scores", d_scores, n_docs, scoreref.SCORE), n_docs, rule), None),
                             d_out, out_cap, "n_matching")

    def top_documents(self, n_docs, k, by="score", lowest=False, ranked=True, min_score=None, max_score=None, min_count=None, max_count=None,
                      density=None, invert=False, d_scores=None, d_doc_offsets=None, d_out=None, out_cap=0, d_top_scores=None, slot=0):
        s = self.slots[slot]
        old, s.ids, s.top = s.ids, None, None
        rule = dict(min_score=min_score, max_score=max_score, min_count=min_count, max_count=max_count, density=density, invert=invert)
        ruled = any(v is not None for v in list(rule.values())[:5]) or invert
        flags = (topref.BY_COUNT if by == "count" else 0) | (topref.LOWEST if lowest else 0) | (topref.RANKED if ranked else 0)

        def fn():
            sc = self._given(s, "scores", d_scores, n_docs, scoreref.SCORE)
            cand = self._candidates(s, sc, n_docs, rule) if ruled else np.arange(sc.size, dtype=np.uint64)
            ids, _ = topref.top(topref.ranking(sc, cand, flags), k, flags)
            if ranked and "top_returns_tied_ids_unordered" in self.defects:
                w = topref.key_word(sc, flags)[ids.astype(np.int64)]
                other = ids[np.lexsort((-ids.astype(np.int64), w))]
                if not np.array_equal(other, ids):
                    self.hit = True
                    ids = other
            return ids, sc[ids.astype(np.int64)]
        return self._produce(s, old, fn, d_out, out_cap, "n_top", d_top_scores)

    def matching_documents_to_host(self, n, slot=0):
        return self._fetch(self.slots[slot], "ids", 0, self.slots[slot].ids["v"].size if self.slots[slot].ids else 0)

    # -- the gathers --------------------------------------------------------------------------
    def _gather(self, slot, n_docs, n_ids, n_bytes, d_ids, d_out, out_cap, d_out_offsets, f):
        s = self.slots[slot]
        old, s.ga = s.ga, None
        try:
            if s.off is None or s.off.size - 1 != n_docs:
                raise _err(S.E_STATE, "no offsets of that n_docs")
            if d_ids is None:
                if s.ids is None:
                    raise _err(S.E_STATE, "no slot-owned ids")
                if n_ids != s.ids["v"].size:
                    raise _err(S.E_ARG, "n_ids")
                ids = s.ids["v"]
                if s.ids.get("zero"):
                    ids = self._fetch(s, "ids", 0, ids.size)
                if np.any(ids[1:] < ids[:-1]) and self._defect("gather_sorts_ranked_ids"):
                    ids = np.sort(ids)
            else:
                ids = np.asarray(d_ids.src, dtype=np.uint64)
            first = None
            if f is not None and f.context_sep:
                if s.seg is None:
                    raise _err(S.E_STATE, "no segment")
                if s.seg.size - 1 != n_docs:
                    raise _err(S.E_ARG, "n_docs is not the segment's")
                first = s.seg
            off, i = s.off.astype(np.int64), ids.astype(np.int64)
            good = i < n_docs
            if not good.all() or (off[i[good]] > off[i[good] + 1]).any() or (off[i[good] + 1] > n_bytes).any():
                raise _err(S.E_ARG, "an id or a selected document breaks the rules")
            out, oo = gather_ref(s.data, s.off, ids) if f is None or f.plain() else format_ref(s.data, s.off, ids, f, first)
            if d_out is not None and out_cap < out.size:
                raise _err(S.E_OVERFLOW, "out_cap too small", out_bytes=int(out.size))
        except PfacError:
            if f is not None and old is not None and self._defect("gather_format_keeps_plain_offsets"):
                s.ga = dict(v=old["v"], off=old["off"])
            raise
        if d_out is None:
            s.ga = dict(v=out, off=oo)
        else:
            d_out.put(out)
            d_out_offsets.put(oo)
        return int(out.size)

    def gather_documents(self, n_docs, n_ids, n_bytes, d_input=None, d_doc_offsets=None, d_ids=None, d_out=None, out_cap=0, d_out_offsets=None, slot=0):
        return self._gather(slot, n_docs, n_ids, n_bytes, d_ids, d_out, out_cap, d_out_offsets, None)

    def gather_documents_formatted(self, n_docs, n_ids, n_bytes, d_input=None, d_doc_offsets=None, d_ids=None, d_doc_first=None, d_out=None,
                                   out_cap=0, d_out_offsets=None, slot=0, **fmt):
        return self._gather(slot, n_docs, n_ids, n_bytes, d_ids, d_out, out_cap, d_out_offsets, Fmt(**fmt))

    def gathered_to_host(self, n, slot=0, first=0):
        return self._fetch(self.slots[slot], "ga", first, n)

    def gathered_offsets_to_host(self, n_ids, slot=0):
        s = self.slots[slot]
        if s.ga is None:
            raise _err(S.E_STATE, "no gather")
        return s.ga["off"]


# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plans():
    return {seed: V.plan(seed) for seed in V.SEEDS}


def _digest(ops):
    return hashlib.sha256(json.dumps(ops, sort_keys=True, default=int).encode()).hexdigest()[:16]


PINNED = "732d2407fdc44b59"


def test_the_plans_are_pinned(plans):
    got = hashlib.sha256("".join(_digest(plans[s]) for s in V.SEEDS).encode()).hexdigest()[:16]
    assert got == PINNED, f"the 24 verdict plans changed: digest {got}"


def test_plans_are_deterministic_and_well_formed(plans):
    for seed in (0, 7, 23):
        assert _digest(V.plan(seed)) == _digest(plans[seed])
        assert V.shrink(seed, 40) == plans[seed][:40]
    for seed, ops in plans.items():
        assert len(ops) == V.PLAN_OPS
        assert sum(op["op"] in V.VERDICT_OPS for op in ops) >= V.MIN_VERDICT_OPS
        assert all(op["op"] in V.VERDICT_OPS + V.OTHER_OPS for op in ops)


def _walk(plans):
    """Every (seed, index, operation, expectation, model before the call) of the suite."""
    for seed, ops in plans.items():
        m = V.Model()
        for k, op in enumerate(ops):
            before = m.clone()
            yield seed, k, op, m.apply(op), before


@pytest.fixture(scope="module")
def reach(plans):
    r = dict(kinds=collections.defaultdict(set), pairs=collections.Counter(), rules=collections.defaultdict(set), late=collections.Counter(),
             statuses=set(), tables=set(), sizes=set(), docs=set(), forms=set(), slots=set(), shared=set(), ks=set(), flags=set(), fmts=set())
    last = {}
    for seed, k, op, exp, before in _walk(plans):
        assert exp.status is not None, f"plan {seed}, operation {k}: the contract does not decide {V.fmt(op)}"
        slot = op.get("slot", 0)
        r["kinds"][op["op"]].add(exp.status == V.OK)
        r["statuses"].add(exp.status)
        for rule in exp.rules:
            r["rules"][rule].add(seed)
        for pair in exp.late:
            r["late"][pair] += 1
        if op["op"] in V.PRODUCERS and exp.status == V.OK and op["out"] == "own":
            last[(seed, slot)] = op["op"]
        elif op["op"] in V.PRODUCERS:
            last.pop((seed, slot), None)
        if op["op"] in V.CONSUMERS and exp.status == V.OK and op.get("ids", "own") == "own":
            r["pairs"][(last[(seed, slot)], op["op"])] += 1
        if op["op"] == "scan":
            r["tables"].add(before.tab)
            r["sizes"].add((before.tab, op["inp"]))
        if op["op"] in ("masks", "scores") and exp.status == V.OK:
            r["docs"].add(X.n_docs(before.slots[slot].docs))
            r["forms"].add(before.slots[slot].docs[2])
        if op["op"] in ("set_doc",):
            r["forms"].add(op["form"])
        if op["op"] == "top" and exp.status == V.OK:
            r["ks"].add(op["k"])
            r["flags"].add(op["flags"])
        if op["op"] == "gather_format" and exp.status == V.OK:
            r["fmts"].add(op["f"])
        r["slots"].add(slot)
        r["shared"].add(before.shared)
    return r


def test_plans_reach_everything(reach):
    r = reach
    print("\nreach of the 24 verdict plans")
    print("  operation kinds (legal / refused): " + ", ".join(f"{k} {'L' if True in v else '-'}{'R' if False in v else '-'}" for k, v in sorted(r["kinds"].items())))
    print("  producer x consumer (times): " + ", ".join(f"{p}>{c} {n}" for (p, c), n in sorted(r["pairs"].items())))
    print("  rules (plans): " + ", ".join(f"{k} {len(r['rules'][k])}" for k in V.RULES))
    print("  R9, result behind event (reads): " + ", ".join(f"{a}/{e} {n}" for (a, e), n in sorted(r["late"].items())))
    never_refused = {"load_table", "set_flen", "set_doc", "reserve_grow", "set_stream", "sync", "scan", "scan_over", "split"}
    for kind in V.VERDICT_OPS + V.OTHER_OPS:
        assert True in r["kinds"][kind], f"{kind} is never legal"
        assert kind in never_refused or False in r["kinds"][kind], f"{kind} is never refused"
    for p in V.PRODUCERS:
        for c in V.CONSUMERS:
            assert r["pairs"][(p, c)] >= 1, f"the ids of {p} never reach {c}"
    for rule in V.RULES:
        assert len(r["rules"][rule]) >= 3, f"{rule} decides an outcome in {len(r['rules'][rule])} plans"
    for res in V.RESULTS:
        for ev in V.R9_EVENTS:
            assert r["late"][(res, ev)] >= 1, f"{res} is never read behind {ev}"
    assert r["statuses"] == {V.OK, V.E_ARG, V.E_STATE, V.E_OVERFLOW}
    assert r["tables"] == set(V.VTABLES) and r["sizes"] == {(t, i) for t in V.VTABLES for i in range(3)}
    assert min(r["docs"]) == 0 and any(0 < d < 64 for d in r["docs"]) and any(1024 <= d <= 4096 for d in r["docs"]) and max(r["docs"]) > 16384
    assert r["forms"] == set(V.FORMS)
    assert r["ks"] == set(V.KS) and r["flags"] == set(range(8)) and r["fmts"] == set(range(len(V.FMTS)))
    assert r["slots"] == {0, 1} and r["shared"] == {False, True}


def test_the_pool_is_what_the_kernels_change_at():
    for t, knobs in V.VTABLES.items():
        assert all(record_width(int(X.table(t).num_final), KNOBS[k]) == V.WIDTHS[t] for k in knobs)
        assert all(k in S.TABLES[t]["knobs"] or t == "cclass" for k in knobs)
        for i in range(3):
            data, off = X.input(t, i), X.offsets((t, i, "split")).astype(np.int64)
            assert data.size == V.TILES[i] * V.TILE and off[-1] == data.size
            pos, lens, _ = X.rows((t, i, data.size, False))
            assert pos.size > 16                                # (scan_over overflows its 16 records)
            for edge in range(V.GROUP, data.size, V.GROUP):     # the line across the edge keeps a record on either side
                d = int(np.searchsorted(off, edge, side="right")) - 1
                assert off[d] < edge < off[d + 1]
                kept = (pos >= off[d]) & (pos + lens <= off[d + 1])
                assert (kept & (pos + lens <= edge)).any() and (kept & (pos >= edge)).any()
    table = X.table("cclass")
    assert any(table.out_first[s + 1] - table.out_first[s] > 1 for s in range(table.num_final))
    _, _, starts, fids = X._whole("cclass", 0)
    assert fids.size > starts.size                              # ... and a record of the pool ends several patterns
    w0 = X.by_id("abc2", "w0")
    assert (w0 == 0).sum() >= 2 and 3 in w0 and -3 in w0
    nd = [X.n_docs((t, i, "split")) for t in V.VTABLES for i in range(3)]
    assert min(nd) < 64 and any(1024 <= n <= 4096 for n in nd) and max(nd) > 16384
    for form in ("bad_end", "bad_order"):
        assert not S.offsets_ok(X.offsets(("mid4", 0, form)), X.input_size("mid4", 0))
    assert np.any(np.diff(X.offsets(("mid4", 0, "host")).astype(np.int64)) == 0)


def test_the_selection_walk_against_the_per_document_reference():
    """Pool._v_sel (one greedy walk over the records that fit their document) against docreplref.per_doc, which selects
    every document on its own with the oracle, on the 3-tile inputs of the literal tables."""
    for t in ("abc2", "mid4"):
        data = X.input(t, 0)
        for form in ("split", "host", "one"):
            off = X.offsets((t, 0, form))
            first, idx = X.value(("sel", (t, 0, data.size, False), (t, 0, form)))
            want_first, want_pos, _, _, _ = per_doc(X.x.tinfo(t)["matcher"], data, off, X.x.tinfo(t)["ll"])
            np.testing.assert_array_equal(first, want_first)
            pos = X._whole(t, 0)[0][idx]
            doc = np.repeat(np.arange(off.size - 1), np.diff(first.astype(np.int64)))
            np.testing.assert_array_equal(pos - off.astype(np.int64)[doc], want_pos)


@pytest.mark.parametrize("seed", V.SEEDS)
def test_plan_passes_on_the_cpu_device(seed, plans):
    stats = V.run(CpuVerdictDevice(), plans[seed], seed=seed)
    assert stats["ops"] == V.PLAN_OPS and stats["verdict"] >= V.MIN_VERDICT_OPS


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_every_defect_is_caught(defect, plans):
    caught = []
    for seed in V.SEEDS:
        dev = CpuVerdictDevice([defect])
        try:
            V.run(dev, plans[seed], seed=seed)
        except AssertionError as e:
            assert dev.hit, f"plan {seed} failed before the defect did anything: {e}"
            caught.append((seed, e.op_index))
    assert caught, f"no committed plan notices the defect {defect} (rule {DEFECTS[defect]})"
    seed, k = caught[0]
    print(f"\n  defect {defect} ({DEFECTS[defect]}): caught by plan {seed} at operation {k} {V.fmt(plans[seed][k])}; {len(caught)} plans in all")


def test_every_rule_has_a_defect():
    assert set(DEFECTS.values()) == set(V.RULES)


def test_shrink_keeps_a_failure(plans):
    for seed in V.SEEDS:
        try:
            V.run(CpuVerdictDevice(["failed_producer_keeps_the_ids"]), plans[seed], seed=seed)
        except AssertionError as e:
            k = e.op_index
            with pytest.raises(AssertionError):
                V.run(CpuVerdictDevice(["failed_producer_keeps_the_ids"]), V.shrink(seed, k + 1), seed=seed)
            V.run(CpuVerdictDevice(["failed_producer_keeps_the_ids"]), V.shrink(seed, k), seed=seed)
            return
    raise AssertionError("no plan fails")


def _named_sessions():
    import test_gpu_verdict_session as G
    out = []
    for name in sorted(vars(G)):
        fn = getattr(G, name)
        if name.startswith("test_") and name != "test_session" and callable(fn):
            marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
            for values in (marks[0].args[1] if marks else [None]):
                out.append(pytest.param(name, values, id=name[5:] + ("" if values is None else f"-{values}")))
    return out


@pytest.mark.parametrize("name,arg", _named_sessions())
def test_named_session_passes_on_the_cpu_device(name, arg, monkeypatch):
    """The named sessions of tests/test_gpu_verdict_session.py, the same operation lists through the same run, on the
    stand-in: what they expect is what the header says, before a GPU sees them."""
    import test_gpu_verdict_session as G
    monkeypatch.setattr(G, "GpuMatcher", lambda *a: CpuVerdictDevice())
    getattr(G, name)(*(() if arg is None else (arg,)))
