"""CPU side of the session tests (tests/session.py): the suite's plans are deterministic, well formed and together reach
every operation, table, record width, status, slot and stream arrangement, and every (producer pass, other pass, late
fetch) order; the executor and the model run every plan against CpuDevice, a stand-in for GpuMatcher that implements the
contract of include/pfac.h in the most obvious way; and each of CpuDevice's switchable defects makes a plan fail at or
after the first operation the defect touches -- the harness has teeth without a kernel being mutated.  The plans come in
two families: those of S.SEEDS, pinned by a digest to what they were before the whole-word filter existed, and those of
S.WORD_SEEDS, in which the filter is an operation like any other, pinned likewise since the counts joined; and those
of S.COUNT_SEEDS, which add the per-pattern counts (count, count_sel, cnt_fetch) under the count knobs of S.CKNOBS,
pinned likewise since the line path joined; and those of S.LINE_SEEDS, which add the delimiter split, the matching
documents with and without context lines and the gather of their bytes (S.LINE_OPS), and have their own reach test,
their own defects (LINE_DEFECTS) and a digest of their own; and those of S.FOLD_SEEDS, which add the case fold as a
setting with a life of its own (set_fold, get_fold, uploads that set or reset it) over the larger pool S.POOL, with
their own reach test, the cap that three quarters of their folded scans differ from the exact ones, FOLD_DEFECTS and a
digest."""
import collections
import copy
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nocaseref
import session as S
from llref import greedy
from orc import match_checksum
from passfuzz import KNOBS, record_width
from phfpfac_amd import GpuMatcher, PfacError
from phfpfac_amd.table import RECORD_DTYPE
from replref import rep_table, splice


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


class _CpuSlot:
    def __init__(self):
        self.in_cap = self.rec_cap = 0
        self.data = None
        self.scan = None
        self.seq = 0
        self.doc = None
        self.doc_gen = 0
        self.sel = self.seg = self.rp = self.rpd = None
        self.text = b""
        self.text_base = 0
        self.prev_first = 0
        self.heap = CpuBuf(16)     # stands for the slot's own record heap where a pointer is compared
        self.last_n = 0
        self.cnt = None            # the slot-owned counts: dict(gen, a)
        self.dm = None             # the ids of the last matching call: dict(ids, own)
        self.dm_before = None      # ... and of the one before it
        self.ga = None             # the last gather: dict(out, off, own_out, own_off)


DEFECTS = ("stale_selection_survives_upload", "late_segment_returns_selection", "smaller_scan_returns_tail",
           "overflowed_scan_hands_out_records", "stale_doc_first_of_empty_trailing_document", "slot1_exit_is_slot0s")
# ... and those of the whole-word filter, which only the plans of S.WORD_SEEDS can meet
WORD_DEFECTS = ("count_stays_the_unfiltered_one", "selection_survives_filter", "refused_filter_filters_anyway",
                "second_filter_replaces_first", "filter_ignores_neighbour_bytes", "filter_ignores_document_offsets",
                "slot1_filter_changes_slot0", "text_follows_a_later_filter")


# ... and those of the per-pattern counts, which only the plans of S.COUNT_SEEDS can meet
COUNT_DEFECTS = ("accumulate_zeroes_first", "plain_count_does_not_zero", "counts_ignore_the_filter", "n_counted_stays_the_unfiltered_count",
                 "refused_count_zeroes_its_destination", "caller_count_replaces_the_slots_counts", "counts_lost_at_upload",
                 "counts_lost_at_reserve", "accumulate_across_upload_allowed", "stale_selection_still_counted",
                 "docsel_counted_as_whole_stream", "slots_share_one_count_buffer", "count_disturbs_the_selection")


# ... and those of the line path, which only the plans of S.LINE_SEEDS can meet
LINE_DEFECTS = ("failed_split_clears_the_offsets", "split_keeps_the_offsets_generation", "failed_matching_keeps_the_ids",
                "context_and_matching_keep_separate_ids", "matching_null_first_is_the_selections", "matching_follows_a_segment_to_the_caller",
                "gather_uses_the_count_before_last", "gather_writes_offsets_on_an_error", "gather_lost_at_upload", "gather_lost_at_reserve",
                "ids_lost_at_a_new_scan", "slot1_gather_reads_slot0s_offsets", "unterminated_tail_offset_dropped",
                "gather_reads_the_input_of_the_last_scan")


# ... and those of the case fold, which only the plans of S.FOLD_SEEDS can meet
FOLD_DEFECTS = ("fold_survives_upload", "fold_survives_device_upload", "fold_is_per_slot", "toggle_reaches_pending_scan", "ext_scan_ignores_fold",
                "bad_mode_clears_fold", "filter_judges_folded_bytes", "replace_copies_folded_bytes", "doc_replace_copies_folded_bytes",
                "gather_copies_folded_bytes", "counts_follow_current_mode", "dense_staging_ignores_fold")
DENSE_PER_TILE = 1024                     # the stand-in's staging mode: dense after a scan of >= 64 tiles with more records per tile


class CpuDevice:
    """GpuMatcher's surface on the CPU: every result recomputed from the oracle's records, outputs kept in dicts.  Works
    in pattern ids (``states_are_ids``).  `defects`: names from DEFECTS to switch on."""
    states_are_ids = True
    device = 0

    def __init__(self, defects=()):
        self.x = S.expectations()
        self.defects = set(defects)
        self.tab = None
        self.gen = 0
        self.width = 4
        self.flen = False
        self.reps = None
        self.slots = [_CpuSlot() for _ in range(S.N_SLOTS)]
        self.hit = False
        self.table = None
        self.fold = False                   # pfac_table_set_case_fold: the uploaded table's setting, read when a scan is queued
        self.fold_slot1 = False             # (defect fold_is_per_slot: what slot 1 goes by)
        self.dense = self.dense_pinned = False

    def _defect(self, name):
        if name in self.defects:
            self.hit = True
            return True
        return False

    # -- buffers ------------------------------------------------------------
    def alloc(self, n_bytes):
        return CpuBuf(n_bytes)

    def upload(self, arr):
        return CpuBuf(16, src=arr)

    def download(self, buf, dtype, count):
        return buf.a[:count * np.dtype(dtype).itemsize].view(dtype).copy()

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    # -- tables -------------------------------------------------------------
    def load_table(self, table):
        self._install(next(t for t in S.POOL if self.x.table(t) is table), "fold_survives_upload")
        if table.ignore_case:               # (GpuMatcher.load_table: the upload leaves the fold off, the wrapper turns it on)
            self.set_case_fold(True)

    def load_table_device(self, d_blob, n_words, stream=0, host_table=None):
        blob = np.asarray(d_blob.src).ravel()
        tab = next(t for t in S.POOL if ("table", t) in self.x._c and self.x.table(t).blob().size == blob.size and np.array_equal(self.x.table(t).blob(), blob))
        self._install(tab, "fold_survives_device_upload")
        if host_table is not None and host_table.ignore_case:
            self.set_case_fold(True)

    def _install(self, tab, fold_defect):
        table = self.x.table(tab)
        self.tab = tab
        if not (self.fold and self._defect(fold_defect)):
            self.fold = False               # every upload resets the fold
        self.fold_slot1 = self.fold
        self.dense_pinned = "PFAC_DENSE" in os.environ
        self.dense = os.environ.get("PFAC_DENSE") == "1"
        knobs = {k: os.environ[k] for d in KNOBS for k in d if k in os.environ}
        self.width = record_width(int(table.num_final), knobs)
        self.gen += 1
        self.flen, self.reps = False, None
        for s in self.slots:
            if s.cnt is not None and s.cnt["a"].any() and self._defect("counts_lost_at_upload"):
                s.cnt = None
            if s.ga is not None and (s.ga["own_out"] or s.ga["own_off"]) and self._defect("gather_lost_at_upload"):
                s.ga = None

    def info(self):
        return {"variant": "cpu", "staging_buffers": 1 if self.dense else 2, "staging_records": 0}

    def raw_set_case_fold(self, mode):
        if self.tab is None:
            raise _err(S.E_STATE, "pfac_table_set_case_fold before a table upload")
        if mode not in (0, 1):
            if self.fold and self._defect("bad_mode_clears_fold"):
                self.fold = self.fold_slot1 = False
            raise _err(S.E_ARG, "mode must be PFAC_FOLD_NONE or PFAC_FOLD_ASCII")
        if self.fold_slot1 != bool(mode) and self._defect("fold_is_per_slot"):
            self.fold = bool(mode)          # (slot 1 keeps the mode it had)
            return
        self.fold = self.fold_slot1 = bool(mode)

    def set_case_fold(self, on):
        self.raw_set_case_fold(int(bool(on)))

    @property
    def case_fold(self):
        if self.tab is None:
            raise _err(S.E_STATE, "pfac_table_case_fold before a table upload")
        return self.fold

    def set_final_lengths(self, lengths):
        if self.tab is None:
            raise _err(S.E_STATE, "no table")
        self.flen = True

    def set_replacements(self, reps):
        if self.tab is None:
            raise _err(S.E_STATE, "no table")
        self.reps = dict(reps)

    def set_redaction(self, fill=b"*"):
        if self.tab is None:
            raise _err(S.E_STATE, "no table")
        ll = self.x.tinfo(self.tab)["ll"]
        self.reps = {k: fill * int(ll[k]) for k in range(1, ll.size)}

    # -- plumbing -----------------------------------------------------------
    def reserve(self, slot=0, input_bytes=0, record_capacity=0):
        s = self.slots[slot]
        if (input_bytes > s.in_cap and s.in_cap) or (record_capacity > s.rec_cap and s.rec_cap):
            s.scan = None                                       # a buffer is replaced: no finished scan
            if s.cnt is not None and self._defect("counts_lost_at_reserve"):
                s.cnt = None
            if s.ga is not None and (s.ga["own_out"] or s.ga["own_off"]) and self._defect("gather_lost_at_reserve"):
                s.ga = None
        if input_bytes > s.in_cap:
            s.in_cap = (input_bytes + 4095) // 4096 * 4096 + 1280
        s.rec_cap = max(s.rec_cap, record_capacity)

    def h2d(self, host, slot=0, dst_offset=0):
        self.slots[slot].data = host

    def sync(self, slot=0):
        pass

    def stream_handle(self, slot=0):
        return 1 + slot

    def records_ptr(self, slot=0):
        return self.slots[slot].heap if self.slots[slot].rec_cap else 0

    def set_stream(self, slot, handle):
        pass

    # -- scans --------------------------------------------------------------
    def scan_async(self, n_owned, n_avail=None, d_input=None, d_records=None, capacity=0, slot=0):
        if self.tab is None:
            raise _err(S.E_STATE, "scan before a table upload")
        s = self.slots[slot]
        data = d_input.src if d_input is not None else s.data
        n_avail = n_owned if n_avail is None else n_avail
        if n_avail == 0:
            inp = next(i for i, d in enumerate(S.POOL[self.tab]["inputs"]) if d[1] == 0)
        else:
            inp = next(i for i in range(len(S.POOL[self.tab]["inputs"])) if self.x.input(self.tab, i) is data)
        fold = self.fold_slot1 if slot == 1 else self.fold       # the mode of THIS launch (fold_slot1 differs under a defect only)
        changes = lambda: not all(np.array_equal(a, b) for a, b in zip(self.x.scan(self.tab, inp, n_owned), self.x.scan(self.tab, inp, n_owned, (), True)))   # noqa: E731
        if fold and d_records is not None and changes() and self._defect("ext_scan_ignores_fold"):
            fold = False
        if fold and self.dense and changes() and self._defect("dense_staging_ignores_fold"):
            fold = False
        pos, ids, lens = self.x.scan(self.tab, inp, n_owned, (), fold)
        cap = capacity if d_records is not None else s.rec_cap
        prev = s.scan
        if s.dm is not None and s.dm["own"] and self._defect("ids_lost_at_a_new_scan"):
            s.dm = None
        s.seq += 1
        s.scan = dict(tab=self.tab, width=self.width, gen=self.gen, data=self.x.input(self.tab, inp), no=n_owned, pos=pos, ids=ids, lens=lens,
                      over=pos.size > cap, pending=True, seq=s.seq, prev=(prev["pos"], prev["ids"]) if prev else None,
                      heap=d_records if d_records is not None else s.heap, full=(pos, ids, lens), fold=fold, inp=inp, cap=cap,
                      tiles=(n_avail + 4095) // 4096)

    def scan_finish(self, slot=0, allow_overflow=False):
        s = self.slots[slot]
        if s.scan is None:
            raise _err(S.E_STATE, "no scan")
        sc = s.scan
        if sc["pending"] and sc["fold"] != self.fold and "toggle_reaches_pending_scan" in self.defects:
            pos, ids, lens = self.x.scan(sc["tab"], sc["inp"], sc["no"], (), self.fold)      # (the mode read at the finish, not at the launch)
            if (pos.size != sc["pos"].size or not np.array_equal(pos, sc["pos"])) and self._defect("toggle_reaches_pending_scan"):
                sc.update(pos=pos, ids=ids, lens=lens, full=(pos, ids, lens), over=pos.size > sc["cap"], fold=self.fold)
        if sc["pending"] and not self.dense_pinned and sc["tiles"] >= 64 and sc["width"] != 8:
            self.dense = sc["pos"].size > DENSE_PER_TILE * sc["tiles"] // 4       # (the next scans of the context run in this mode)
        s.scan["pending"] = False
        if s.scan["over"] and not allow_overflow:
            raise _err(S.E_OVERFLOW, "overflow")
        n = int(s.scan["pos"].size)
        if n != s.scan["full"][0].size and self._defect("count_stays_the_unfiltered_one"):
            n = int(s.scan["full"][0].size)
        s.last_n = n
        return n, s.scan["over"]

    def last_count(self, slot=0):
        return self.slots[slot].last_n

    def capacity_hint(self, slot=0):
        n = int(self.slots[slot].scan["pos"].size)
        return n + n // 4 + 65536

    scan_resident = GpuMatcher.scan_resident
    scan_bytes = GpuMatcher.scan_bytes

    def scan_format(self, slot=0):
        sc = self.slots[slot].scan
        if sc is None:
            raise _err(S.E_STATE, "no scan yet")
        return sc["width"], (sc["no"] + 4095) // 4096, int(sc["full"][0].size)      # (used: what the scan wrote, filtered or not)

    def _finished(self, slot, overflow_status):
        sc = self.slots[slot].scan
        if sc is None or sc["pending"]:
            raise _err(S.E_STATE, "needs a finished scan")
        if sc["over"] and overflow_status:
            raise _err(overflow_status, "the scan overflowed")
        return sc

    @staticmethod
    def _rec(pos, ids):
        out = np.empty(pos.size, dtype=RECORD_DTYPE)
        out["pos"], out["state"] = pos, ids
        return out

    def records_to_host(self, n, slot=0, d_records=None, first=0):
        if n == 0:
            return np.empty(0, dtype=RECORD_DTYPE)
        sc = self._finished(slot, 0)
        bound = sc["pos"].size
        if bound != sc["full"][0].size and first + n > bound and self._defect("count_stays_the_unfiltered_one"):
            bound = sc["full"][0].size
        if first + n > bound:
            raise _err(S.E_ARG, "beyond the match count")
        if sc["over"] and not self._defect("overflowed_scan_hands_out_records"):
            raise _err(S.E_OVERFLOW, "the scan overflowed")
        pos, ids = sc["pos"], sc["ids"]
        if sc["prev"] is not None and sc["prev"][0].size > pos.size and self._defect("smaller_scan_returns_tail"):
            pos, ids = sc["prev"][0][-pos.size:], sc["prev"][1][-pos.size:]
        return self._rec(pos[first:first + n], ids[first:first + n])

    def packed_to_host(self, slot=0, d_records=None):
        rb, nt, used = self.scan_format(slot)
        if rb == 8:
            raise _err(S.E_STATE, "not compact")
        sc = self.slots[slot].scan
        pos, ids = sc["pos"], sc["ids"]
        full = np.bincount(sc["full"][0] >> 12, minlength=nt)
        start = np.cumsum(full) - full                          # every tile's run begins where the scan put it
        cnt = np.bincount(pos >> 12, minlength=nt)
        words = np.zeros(used, dtype=np.uint16 if rb == 2 else np.uint32)
        words[start[pos >> 12] + np.arange(pos.size) - (np.cumsum(cnt) - cnt)[pos >> 12]] = (pos & 4095) | (ids << 12)
        return words, start.astype(np.uint64) | (cnt.astype(np.uint64) << np.uint64(40))

    def checksum(self, n, base=0, slot=0, d_records=None):
        if self.tab is None:
            raise _err(S.E_STATE, "no table")
        if n == 0:
            return 0
        sc = self._finished(slot, 0)
        if sc["gen"] != self.gen:
            raise _err(S.E_STATE, "earlier table")
        if sc["over"]:
            raise _err(S.E_OVERFLOW, "overflow")
        return match_checksum(sc["pos"] + base, sc["ids"])

    def emit_text_device(self, base=0, slot=0, d_records=None):
        if self.tab is None:
            raise _err(S.E_STATE, "no table")
        sc = self._finished(slot, 0)
        if sc["gen"] != self.gen:
            raise _err(S.E_STATE, "earlier table")
        if sc["over"]:
            raise _err(S.E_OVERFLOW, "overflow")
        self.slots[slot].text = self._text(sc, base)
        self.slots[slot].text_base = base
        return len(self.slots[slot].text)

    @staticmethod
    def _text(sc, base):
        return "".join("At position %4d, match pattern %d\n" % (p + base, k) for p, k in zip(sc["pos"].tolist(), sc["ids"].tolist())).encode()

    def text_to_host(self, n_bytes, slot=0, first=0):
        if first + n_bytes > len(self.slots[slot].text):
            raise _err(S.E_ARG, "beyond the text")
        return self.slots[slot].text[first:first + n_bytes]

    # -- counts per pattern ---------------------------------------------------
    def _cnt_slot(self, slot):
        if slot == 1 and self._defect("slots_share_one_count_buffer"):
            return self.slots[0]
        return self.slots[slot]

    def _count(self, slot, ids, n, d_counts, n_states, flags):
        """The arguments both count calls share, then the histogram of `ids` into the destination."""
        own, acc = d_counts is None, bool(flags & 1)
        cs = self._cnt_slot(slot)
        n_ids = self.x.n_ids(self.tab)
        if flags > 1 or n_states != n_ids or isinstance(d_counts, S.Odd):
            raise _err(S.E_ARG, "flags, n_states or a misaligned d_counts")
        if own and acc and cs.cnt is not None and cs.cnt["gen"] != self.gen and not self._defect("accumulate_across_upload_allowed"):
            raise _err(S.E_STATE, "the slot's counts belong to an earlier table")
        hist = np.bincount(ids, minlength=n_ids).astype(np.uint64)
        if own:
            old = cs.cnt["a"] if cs.cnt is not None and cs.cnt["a"].size == n_ids else np.zeros(n_ids, np.uint64)
        else:
            old = d_counts.a[:n_ids * 8].view(np.uint64).copy()
        if acc and old.any() and self._defect("accumulate_zeroes_first"):
            acc = False
        if not acc and old.any() and hist.any() and self._defect("plain_count_does_not_zero"):
            acc = True
        new = old + hist if acc else hist
        if own:
            cs.cnt = dict(gen=self.gen, a=new)
        else:
            d_counts.put(new)
            if self._defect("caller_count_replaces_the_slots_counts"):
                cs.cnt = dict(gen=self.gen, a=hist)
        sel = self.slots[slot].sel
        if sel is not None and sel["own"] and sel["rec"].size and self._defect("count_disturbs_the_selection"):
            sel["rec"] = sel["rec"].copy()
            sel["rec"]["state"][0] += 1
        return int(n)

    def _refused(self, slot, d_counts, fn):
        try:
            return fn()
        except PfacError:
            buf = d_counts.buf if isinstance(d_counts, S.Odd) else d_counts
            if "refused_count_zeroes_its_destination" in self.defects:
                cs = self.slots[slot]
                if buf is None and cs.cnt is not None and cs.cnt["a"].any() and self._defect("refused_count_zeroes_its_destination"):
                    cs.cnt["a"] = np.zeros_like(cs.cnt["a"])
                if buf is not None and self._defect("refused_count_zeroes_its_destination"):
                    buf.a[:buf.a.size - 64] = 0
            raise

    def raw_count_states(self, slot, d_records, d_counts, n_states, flags):
        def call():
            s = self.slots[slot]
            sc = self._finished(slot, 0)
            if self.tab is None or sc["gen"] != self.gen:
                raise _err(S.E_STATE, "a scan made with an earlier table")
            if sc["over"]:
                raise _err(S.E_OVERFLOW, "the scan overflowed")
            if (d_records if d_records is not None else s.heap) is not sc["heap"]:
                raise _err(S.E_ARG, "not the heap of the slot's last scan")
            ids, n = sc["ids"], sc["ids"].size
            if sc["fold"] != self.fold and ids.size == sc["full"][1].size and "counts_follow_current_mode" in self.defects:
                other = self.x.scan(sc["tab"], sc["inp"], sc["no"], (), self.fold)[1]
                if not np.array_equal(np.bincount(other, minlength=1), np.bincount(ids, minlength=1)) and self._defect("counts_follow_current_mode"):
                    ids, n = other, other.size
            if ids.size != sc["full"][1].size and self._defect("counts_ignore_the_filter"):
                ids = sc["full"][1]
            if n != sc["full"][1].size and self._defect("n_counted_stays_the_unfiltered_count"):
                n = sc["full"][1].size
            return self._count(slot, ids, n, d_counts, n_states, flags)
        return self._refused(slot, d_counts, call)

    def count_states(self, slot=0, d_records=None, d_counts=None, accumulate=False):
        if self.tab is None:
            raise _err(S.E_STATE, "no table")
        return self.raw_count_states(slot, d_records, d_counts, self.x.n_ids(self.tab), int(accumulate))

    def count_selection_states(self, slot=0, d_sel=None, d_counts=None, accumulate=False):
        def call():
            s = self.slots[slot]
            sc, sel = s.scan, s.sel
            if sc is None or sc["pending"] or sel is None:
                raise _err(S.E_STATE, "no selection since the slot's last scan")
            if sel["seq"] != sc["seq"] and not (sel["gen"] == self.gen and self._defect("stale_selection_still_counted")):
                raise _err(S.E_STATE, "no selection since the slot's last scan")
            if self.tab is None or sc["gen"] != self.gen or sel["gen"] != self.gen:
                raise _err(S.E_STATE, "earlier table")
            if d_sel is None and not sel["own"]:
                raise _err(S.E_STATE, "the selection went to the caller's buffer")
            if isinstance(d_sel, S.Odd):
                raise _err(S.E_ARG, "misaligned d_sel")
            ids = sel["rec"]["state"].astype(np.int64)
            if d_sel is not None and ids.size and (getattr(d_sel, "junk", False) or d_sel is not sel["buf"]):
                raise _err(S.E_ARG, "not a selection of this scan and table")
            if sel["kind"] == "docs" and "docsel_counted_as_whole_stream" in self.defects:
                idx, _ = greedy(sc["pos"], sc["lens"], 0, sc["no"])
                if not np.array_equal(sc["ids"][idx], ids) and self._defect("docsel_counted_as_whole_stream"):
                    ids = sc["ids"][idx]
            return self._count(slot, ids, ids.size, d_counts, self.x.n_ids(self.tab), int(accumulate))
        return self._refused(slot, d_counts, call)

    def state_counts_to_host(self, slot=0):
        cs = self._cnt_slot(slot)
        if cs.cnt is None:
            raise _err(S.E_STATE, "the slot holds no counts")
        return cs.cnt["a"].copy()

    # -- documents ----------------------------------------------------------
    def set_doc_offsets(self, offsets, slot=0):
        s = self.slots[slot]
        s.doc = np.array(offsets, dtype=np.uint64)
        s.doc_gen += 1

    def _pass_scan(self, slot, overflow_status):
        sc = self.slots[slot].scan
        if sc is None or sc["pending"] or not self.flen or sc["gen"] != self.gen:
            raise _err(S.E_STATE, "needs a finished scan of the current table and its lengths")
        if sc["over"]:
            raise _err(overflow_status, "the scan overflowed")
        return sc

    def _docs(self, slot, sc):
        s = self.slots[slot]
        if s.doc is None:
            raise _err(S.E_STATE, "no document offsets")
        if not S.offsets_ok(s.doc, sc["no"]):
            raise _err(S.E_ARG, "bad offsets")
        off = s.doc.astype(np.int64)
        doc = np.searchsorted(off, sc["pos"], side="right") - 1
        keep = sc["pos"] + sc["lens"] <= off[doc + 1]
        return off, doc[keep], sc["pos"][keep], sc["ids"][keep], sc["lens"][keep]

    # -- lines: split, matching documents, gather -------------------------------
    def _input(self, slot, d_input, n_bytes, what):
        """The bytes a call reads: the slot's input (d_input None) or a caller's buffer."""
        s = self.slots[slot]
        if isinstance(d_input, S.Odd):
            raise _err(S.E_ARG, what + ": misaligned d_input")
        if d_input is not None:
            return d_input.src
        if n_bytes > s.in_cap:
            raise _err(S.E_ARG, what + ": n_bytes exceeds the slot's input buffer")
        return s.data if s.data is not None else np.zeros(0, np.uint8)

    def split_documents(self, n_bytes, delimiter=b"\n", d_input=None, slot=0):
        s = self.slots[slot]
        try:
            delim = delimiter[0] if isinstance(delimiter, (bytes, bytearray)) else int(delimiter)
            if not 0 <= delim <= 255:
                raise _err(S.E_ARG, "the delimiter is one byte")
            data = self._input(slot, d_input, n_bytes, "split")[:n_bytes]
        except PfacError:
            if s.doc is not None and self._defect("failed_split_clears_the_offsets"):
                s.doc = None
            raise
        ends = [i + 1 for i, b in enumerate(data.tobytes()) if b == delim]
        off = [0] + ends + ([n_bytes] if n_bytes and (not ends or ends[-1] != n_bytes) else [])
        tail = n_bytes if not n_bytes or (ends and ends[-1] == n_bytes) else (ends[-1] if ends else 0)
        if len(off) >= 3 and tail != n_bytes and self._defect("unterminated_tail_offset_dropped"):
            off = off[:-1]
        s.doc = np.array(off, dtype=np.uint64)
        if not (s.sel is not None and s.sel["kind"] == "docs" and self._defect("split_keeps_the_offsets_generation")):
            s.doc_gen += 1
        return len(off) - 1, tail

    def doc_offsets_to_host(self, n_docs, slot=0, first=0, n=None):
        s = self.slots[slot]
        if s.doc is None:
            raise _err(S.E_STATE, "the slot holds no document offsets")
        n = int(n_docs) + 1 - first if n is None else n
        if first + n > s.doc.size:
            raise _err(S.E_ARG, "beyond the offsets")
        return s.doc[first:first + n].copy()

    def raw_matching(self, slot, context, d_first, n_docs, before, after, flags, d_out, out_cap):
        s = self.slots[slot]
        old, s.dm = s.dm, None
        try:
            return self._matching(s, old, context, d_first, n_docs, before, after, flags, d_out, out_cap)
        except PfacError:
            if old is not None and old["own"] and self._defect("failed_matching_keeps_the_ids"):
                s.dm = old
            raise

    def _matching(self, s, old, context, d_first, n_docs, before, after, flags, d_out, out_cap):
        if d_first is None:
            seg = s.seg
            if seg is not None and not seg["own"] and self._defect("matching_follows_a_segment_to_the_caller"):
                first = seg["first"]
            elif seg is None or not seg["own"]:
                raise _err(S.E_STATE, "the slot holds no doc_first of a segment")
            else:
                first = seg["first"]
                sel = s.sel
                if (sel is not None and sel["kind"] == "docs" and sel["first"].size == first.size
                        and not np.array_equal(np.diff(sel["first"].astype(np.int64)) > 0, np.diff(first.astype(np.int64)) > 0)
                        and self._defect("matching_null_first_is_the_selections")):
                    first = sel["first"]
            if n_docs != first.size - 1:
                raise _err(S.E_ARG, "n_docs differs from the segment's")
        else:
            first = d_first.a[:(n_docs + 1) * 8].view(np.uint64)
        if flags > 1 or (context and flags) or isinstance(d_out, S.Odd):
            raise _err(S.E_ARG, "flags or a misaligned d_ids_out")
        has = [int(first[d + 1]) > int(first[d]) for d in range(n_docs)]
        if context:                                             # (matching documents before d, so that a window costs two lookups)
            seen = [0]
            for h in has:
                seen.append(seen[-1] + h)
            ids = [d for d in range(n_docs) if seen[min(d + min(before, n_docs), n_docs - 1) + 1] > seen[max(d - min(after, n_docs), 0)]]
        else:
            ids = [d for d in range(n_docs) if has[d] != bool(flags)]
        ids = np.array(ids, dtype=np.uint64)
        if d_out is not None and ids.size > out_cap:
            raise _err(S.E_OVERFLOW, "out_cap too small", n_matching=int(ids.size))
        if d_out is not None:
            d_out.put(ids)
        s.dm_before = old
        s.dm = dict(ids=ids, own=d_out is None, context=context)
        if (d_out is None and old is not None and old["own"] and old["context"] != context and not np.array_equal(old["ids"], ids)
                and self._defect("context_and_matching_keep_separate_ids")):
            s.dm = dict(old, kept=True)                           # (the fetch and the gather go on reading the other call's buffer)
        return int(ids.size)

    def matching_documents(self, n_docs, invert=False, d_doc_first=None, d_out=None, out_cap=0, slot=0, before=0, after=0):
        return self.raw_matching(slot, bool(before or after), d_doc_first, n_docs, before, after, int(invert), d_out, out_cap)

    def matching_documents_to_host(self, n, slot=0):
        s = self.slots[slot]
        if s.dm is None or not s.dm["own"]:
            raise _err(S.E_STATE, "no slot-owned ids")
        return s.dm["ids"].copy()

    def gather_documents(self, n_docs, n_ids, n_bytes, d_input=None, d_doc_offsets=None, d_ids=None, d_out=None, out_cap=0, d_out_offsets=None,
                         slot=0):
        s = self.slots[slot]
        s.ga = None
        data = self._input(slot, d_input, n_bytes, "gather")
        sc = s.scan
        if d_input is None and sc is not None and sc["data"] is not data and sc["data"].size >= n_bytes and self._defect("gather_reads_the_input_of_the_last_scan"):
            data = sc["data"]
        if d_doc_offsets is None:
            ds = self.slots[0] if slot == 1 and self.slots[0].doc is not None and self._defect("slot1_gather_reads_slot0s_offsets") else s
            if ds.doc is None or n_docs != ds.doc.size - 1:
                raise _err(S.E_STATE, "the slot has no document offsets for this n_docs")
            off = ds.doc
        else:
            off = d_doc_offsets.src
        if d_ids is None:
            if s.dm is None or not s.dm["own"]:
                raise _err(S.E_STATE, "the slot holds no ids")
            count = s.dm["ids"].size
            if s.dm_before is not None and s.dm_before["ids"].size != count and self._defect("gather_uses_the_count_before_last"):
                count = s.dm_before["ids"].size
            if n_ids != count:
                raise _err(S.E_ARG, "n_ids differs from the last matching call's count")
            ids = s.dm["ids"]
        else:
            ids = d_ids.src
        if isinstance(d_out, S.Odd):
            raise _err(S.E_ARG, "misaligned d_out")
        pieces, out_off = [], [0]
        for k in ids.tolist():
            if k >= n_docs or not int(off[k]) <= int(off[k + 1]) <= n_bytes:
                if d_out_offsets is not None and self._defect("gather_writes_offsets_on_an_error"):
                    d_out_offsets.put(np.array(out_off, dtype=np.uint64))
                raise _err(S.E_ARG, "an id beyond n_docs, or a selected document whose offsets break the rules")
            pieces.append(data[int(off[k]):int(off[k + 1])])
            out_off.append(out_off[-1] + pieces[-1].size)
        out = np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)
        if d_input is None and sc is not None and sc["fold"] and sc["data"] is data and "gather_copies_folded_bytes" in self.defects:
            if not np.array_equal(nocaseref.fold(out), out) and self._defect("gather_copies_folded_bytes"):
                out = nocaseref.fold(out)                        # (as if the folded scan had folded the slot's input in place)
        out_off = np.array(out_off, dtype=np.uint64)
        if d_out is not None and out.size > out_cap:
            raise _err(S.E_OVERFLOW, "out_cap too small", out_bytes=int(out.size))
        if d_out is not None:
            d_out.put(out)
        if d_out_offsets is not None:
            d_out_offsets.put(out_off)
        s.ga = dict(out=out, off=out_off, own_out=d_out is None, own_off=d_out_offsets is None)
        return int(out.size)

    def gathered_to_host(self, n, slot=0, first=0):
        s = self.slots[slot]
        if s.ga is None or not s.ga["own_out"]:
            raise _err(S.E_STATE, "no slot-owned gather output")
        if first + n > s.ga["out"].size:
            raise _err(S.E_ARG, "beyond the output")
        return s.ga["out"][first:first + n].copy()

    def gathered_offsets_to_host(self, n_ids, slot=0):
        s = self.slots[slot]
        if s.ga is None or not s.ga["own_off"]:
            raise _err(S.E_STATE, "no slot-owned output offsets")
        return s.ga["off"].copy()

    # -- the whole-word filter ------------------------------------------------
    def filter_whole_words(self, slot=0, word_bytes=None, edges="both", prev_byte=-1, next_byte=-1, n_docs=0, d_doc_offsets=None,
                           d_input=None, d_records=None):
        s = self.slots[slot]
        sc = self._pass_scan(slot, S.E_OVERFLOW)
        if (d_records if d_records is not None else s.heap) is not sc["heap"]:
            raise _err(S.E_ARG, "not the heap of the slot's last scan")
        sc.pop("judged", None)
        if sc["fold"] and "filter_judges_folded_bytes" in self.defects:
            isw = np.zeros(256, dtype=bool)
            isw[list(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ_abcdefghijklmnopqrstuvwxyz" if word_bytes is None else word_bytes)] = True
            if not np.array_equal(isw[nocaseref.fold(sc["data"])], isw[sc["data"]]) and self._defect("filter_judges_folded_bytes"):
                sc["judged"] = nocaseref.fold(sc["data"])
        off = None
        if n_docs:
            if s.doc is None or n_docs != s.doc.size - 1:
                raise _err(S.E_STATE, "no document offsets with this n_docs")
            if not S.offsets_ok(s.doc, sc["no"]):
                if sc["pos"].size and self._defect("refused_filter_filters_anyway"):
                    self._apply_filter(s, sc, word_bytes, edges, -1, -1, None)
                raise _err(S.E_ARG, "bad offsets")
            off = s.doc.astype(np.int64)
            if self._cuts(sc, word_bytes, prev_byte, next_byte, None)[off].any() and self._defect("filter_ignores_document_offsets"):
                off = None
        if (prev_byte, next_byte) != (-1, -1) and self._defect("filter_ignores_neighbour_bytes"):
            prev_byte = next_byte = -1
        n = self._apply_filter(s, sc, word_bytes, edges, prev_byte, next_byte, off)
        if not (s.sel is not None and s.sel["seq"] == sc["seq"] and self._defect("selection_survives_filter")):
            s.seq += 1                                          # a new record set: what selected from the old one is stale
            sc["seq"] = s.seq
        other = self.slots[0].scan
        if slot == 1 and other is not None and other["pos"].size and self._defect("slot1_filter_changes_slot0"):
            half = other["pos"].size // 2
            other["pos"], other["ids"], other["lens"] = other["pos"][:half], other["ids"][:half], other["lens"][:half]
        if s.text and "text_follows_a_later_filter" in self.defects and self._text(sc, s.text_base) != s.text and self._defect("text_follows_a_later_filter"):
            s.text = self._text(sc, s.text_base)
        s.last_n = n
        return n

    @staticmethod
    def _cuts(sc, word_bytes, prev_byte, next_byte, off):
        """bool[n_avail + 1]: a word runs on across i (W of the byte before i and of the byte at i), no document starts there."""
        isw = np.zeros(256, dtype=bool)
        isw[list(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ_abcdefghijklmnopqrstuvwxyz" if word_bytes is None else word_bytes)] = True
        w = isw[sc.get("judged", sc["data"])]
        cut = np.concatenate(([prev_byte >= 0 and isw[prev_byte]], w)) & np.concatenate((w, [next_byte >= 0 and isw[next_byte]]))
        if off is not None:
            cut[off] = False
        return cut

    def _apply_filter(self, s, sc, word_bytes, edges, prev_byte, next_byte, off):
        cut = self._cuts(sc, word_bytes, prev_byte, next_byte, off)
        pos, ids, lens = sc["pos"], sc["ids"], sc["lens"]
        if pos.size != sc["full"][0].size and self._defect("second_filter_replaces_first"):
            pos, ids, lens = sc["full"]
        keep = np.ones(pos.size, dtype=bool)
        if edges in ("left", "both"):
            keep &= ~cut[pos]
        if edges in ("right", "both"):
            keep &= ~cut[pos + lens]
        sc["pos"], sc["ids"], sc["lens"] = pos[keep], ids[keep], lens[keep]
        return int(keep.sum())

    def _first(self, s, first):
        if first.size >= 3 and first.size and self.slots[s].doc[-1] == self.slots[s].doc[-2] and self._defect("stale_doc_first_of_empty_trailing_document"):
            first = first.copy()
            first[-2] = self.slots[s].prev_first
        self.slots[s].prev_first = int(first[-1]) + 1
        return first

    def _deliver(self, what, n, rec, first, d_out, out_cap, d_first, attr):
        if d_out is not None and n > out_cap:
            raise _err(S.E_OVERFLOW, "out_cap too small", **{attr: n})
        if d_out is not None:
            d_out.put(rec)
            if d_first is not None:
                d_first.put(first)
        return dict(rec=rec, first=first, own=d_out is None, buf=d_out)

    def segment_records(self, n_docs, d_doc_offsets=None, d_out=None, out_cap=0, d_doc_first=None, slot=0, d_records=None):
        s = self.slots[slot]
        s.seg = None
        sc = self._pass_scan(slot, S.E_OVERFLOW)
        off, doc, pos, ids, _ = self._docs(slot, sc)
        first = self._first(slot, np.searchsorted(doc, np.arange(off.size), side="left").astype(np.uint64))
        s.seg = self._deliver("seg", pos.size, self._rec(pos - off[doc], ids), first, d_out, out_cap, d_doc_first, "n_kept")
        s.seg["after_sel"] = False
        return int(pos.size)

    def segment_to_host(self, n_kept, n_docs, slot=0):
        s = self.slots[slot]
        if s.seg is None or not s.seg["own"]:
            raise _err(S.E_STATE, "no slot-owned segment result")
        if s.seg["after_sel"] and s.sel is not None and self._defect("late_segment_returns_selection"):
            return s.seg["first"], s.sel["rec"]
        return s.seg["first"], s.seg["rec"]

    # -- selection ----------------------------------------------------------
    def select_leftmost_longest(self, entry=0, d_out=None, out_cap=0, slot=0, d_records=None):
        s = self.slots[slot]
        s.sel = None
        sc = self._pass_scan(slot, S.E_STATE)
        if entry > self.x.M(sc["tab"]):
            raise _err(S.E_ARG, "entry > max_pat_len")
        idx, ex = greedy(sc["pos"], sc["lens"], entry, sc["no"])
        s.sel = self._deliver("sel", idx.size, self._rec(sc["pos"][idx], sc["ids"][idx]), None, d_out, out_cap, None, "n_selected")
        s.sel.update(kind="whole", seq=sc["seq"], gen=sc["gen"], entry=entry, exit=int(ex), lens=sc["lens"][idx])
        if s.seg is not None:
            s.seg["after_sel"] = True
        if slot == 1 and self.slots[0].sel is not None and self._defect("slot1_exit_is_slot0s"):
            return int(idx.size), self.slots[0].sel["exit"]
        return int(idx.size), int(ex)

    def select_leftmost_longest_documents(self, n_docs, d_doc_offsets=None, d_out=None, out_cap=0, d_doc_first=None, slot=0, d_records=None):
        s = self.slots[slot]
        s.sel = None
        sc = self._pass_scan(slot, S.E_STATE)
        off, doc, pos, ids, lens = self._docs(slot, sc)
        picks = []
        bounds = np.searchsorted(doc, np.arange(off.size), side="left")
        for d in range(off.size - 1):
            a, b = int(bounds[d]), int(bounds[d + 1])
            if b > a:
                idx, _ = greedy(pos[a:b], lens[a:b], int(off[d]), int(off[d + 1]))
                picks.append(idx + a)
        idx = np.concatenate(picks) if picks else np.empty(0, np.int64)
        first = self._first(slot, np.searchsorted(doc[idx], np.arange(off.size), side="left").astype(np.uint64))
        s.sel = self._deliver("sel", idx.size, self._rec(pos[idx], ids[idx]), first, d_out, out_cap, d_doc_first, "n_selected")
        s.sel.update(kind="docs", seq=sc["seq"], gen=sc["gen"], entry=0, exit=0, lens=lens[idx], doc_gen=s.doc_gen, off=off)
        if s.seg is not None:
            s.seg["after_sel"] = True
        return int(idx.size)

    def selection_to_host(self, n_selected, slot=0):
        s = self.slots[slot]
        if s.sel is None or not s.sel["own"]:
            raise _err(S.E_STATE, "no slot-owned selection")
        return s.sel["rec"]

    def doc_selection_to_host(self, n_selected, n_docs, slot=0):
        s = self.slots[slot]
        if s.sel is None or s.sel["kind"] != "docs" or not s.sel["own"]:
            raise _err(S.E_STATE, "no slot-owned per-document selection")
        return s.sel["first"], s.sel["rec"]

    # -- replace ------------------------------------------------------------
    def _replace(self, slot, docs, d_out, out_cap, d_out_offsets):
        s = self.slots[slot]
        s.rp = s.rpd = None
        sc, sel = s.scan, s.sel
        if sc is None or sel is None or sel["seq"] != sc["seq"] or (docs and sel["kind"] != "docs"):
            raise _err(S.E_STATE, "no selection since the slot's last scan")
        stale = sc["gen"] != self.gen
        if stale and not self._defect("stale_selection_survives_upload"):
            raise _err(S.E_STATE, "earlier table")
        if self.reps is None or not self.flen:
            raise _err(S.E_STATE, "no replacements or lengths")
        if docs and sel["doc_gen"] != s.doc_gen:
            raise _err(S.E_STATE, "the offsets changed since the selection")
        table = rep_table(self.reps if not stale else {k: b"?" for k in range(1, 4096)})
        pos, ids, lens = sel["rec"]["pos"].astype(np.int64), sel["rec"]["state"].astype(np.int64), sel["lens"]
        src = sc["data"]
        if sc["fold"] and not np.array_equal(nocaseref.fold(src[:sc["no"]]), src[:sc["no"]]) and self._defect("doc_replace_copies_folded_bytes" if docs else "replace_copies_folded_bytes"):
            src = nocaseref.fold(src)
        if sel["kind"] == "whole":
            out = splice(src, sel["entry"], sc["no"], pos, lens, ids, table)
            out_off = None
        else:
            off, first = sel["off"], sel["first"].astype(np.int64)
            parts = [splice(src[int(off[d]):int(off[d + 1])], 0, int(off[d + 1] - off[d]), pos[first[d]:first[d + 1]] - off[d],
                            lens[first[d]:first[d + 1]], ids[first[d]:first[d + 1]], table) for d in range(off.size - 1)]
            out = np.concatenate(parts) if parts else np.empty(0, np.uint8)
            out_off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
        if d_out is not None and out.size > out_cap:
            raise _err(S.E_OVERFLOW, "out_cap too small", out_bytes=int(out.size))
        if d_out is not None:
            d_out.put(out)
        s.rp = dict(out=out, own=d_out is None)
        if docs:
            if d_out_offsets is not None:
                d_out_offsets.put(out_off)
            s.rpd = dict(off=out_off, own=d_out_offsets is None)
        return int(out.size)

    def replace_selection(self, d_input=None, d_out=None, out_cap=0, slot=0, d_sel=None):
        return self._replace(slot, False, d_out, out_cap, None)

    def replace_selection_documents(self, d_input=None, d_out=None, out_cap=0, d_out_offsets=None, slot=0, d_sel=None, d_doc_offsets=None,
                                    d_doc_first=None):
        return self._replace(slot, True, d_out, out_cap, d_out_offsets)

    def replacement_to_host(self, n, slot=0, first=0):
        s = self.slots[slot]
        if s.rp is None or not s.rp["own"]:
            raise _err(S.E_STATE, "no slot-owned replace output")
        if first + n > s.rp["out"].size:
            raise _err(S.E_ARG, "beyond the output")
        return s.rp["out"][first:first + n]

    def replacement_doc_offsets_to_host(self, n_docs, slot=0):
        s = self.slots[slot]
        if s.rpd is None or not s.rpd["own"]:
            raise _err(S.E_STATE, "no slot-owned output offsets")
        return s.rpd["off"]


# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plans():
    return {seed: S.plan(seed) for seed in S.SEEDS}


@pytest.fixture(scope="module")
def word_plans():
    return {seed: S.plan(seed, words=True) for seed in S.WORD_SEEDS}


@pytest.fixture(scope="module")
def count_plans():
    return {seed: S.plan(seed, counts=True) for seed in S.COUNT_SEEDS}


# SHA-256 of json.dumps([plan(seed) for seed in SEEDS], sort_keys=True) at the commit before the filter joined the
# harness (with the pool's pattern lines in a fixed order, see _gen_lines): the first family has not moved.
OLD_PLANS_SHA256 = "e756864a7526abf17871316573c9079f43bc1106d0403266a50f5130050b937a"


def test_the_plans_without_the_filter_are_what_they_were(plans):
    assert [seed for seed in plans] == S.SEEDS and len(S.SEEDS) == 24
    assert hashlib.sha256(json.dumps([plans[seed] for seed in S.SEEDS], sort_keys=True).encode()).hexdigest() == OLD_PLANS_SHA256
    assert not any(op["op"] == "filter" for ops in plans.values() for op in ops)


@pytest.fixture(scope="module")
def line_plans():
    return {seed: S.plan(seed, lines=True) for seed in S.LINE_SEEDS}


# ... and of json.dumps([plan(seed, words=True) for seed in WORD_SEEDS], sort_keys=True) at the commit before the counts
# joined the harness: the second family has not moved either.
WORD_PLANS_SHA256 = "5cbdcad3040302c5db5d67f19c7157018a74c11ca9fbfca3e56f190d3e672657"
COUNT_OPS = ("count", "count_sel", "cnt_fetch")


def test_the_plans_with_the_filter_are_what_they_were(word_plans):
    assert [seed for seed in word_plans] == S.WORD_SEEDS and len(S.WORD_SEEDS) == 24
    assert hashlib.sha256(json.dumps([word_plans[seed] for seed in S.WORD_SEEDS], sort_keys=True).encode()).hexdigest() == WORD_PLANS_SHA256
    assert not any(op["op"] in COUNT_OPS or "cknob" in op for ops in word_plans.values() for op in ops)


# ... and of json.dumps([plan(seed, counts=True) for seed in COUNT_SEEDS], sort_keys=True) at the commit before the line path
# joined the harness: the third family has not moved either.
COUNT_PLANS_SHA256 = "70c235477764f42868f257baa0e6032d0772d3b0cc86025bd3d64149ad34018a"


def test_the_plans_with_the_counts_are_what_they_were(count_plans):
    assert [seed for seed in count_plans] == S.COUNT_SEEDS and len(S.COUNT_SEEDS) == 24
    assert hashlib.sha256(json.dumps([count_plans[seed] for seed in S.COUNT_SEEDS], sort_keys=True).encode()).hexdigest() == COUNT_PLANS_SHA256
    assert not any(op["op"] in S.LINE_OPS for ops in count_plans.values() for op in ops)


def test_plans_are_deterministic_and_well_formed(plans, word_plans):
    for seed in S.SEEDS[:4]:
        assert S.plan(seed) == plans[seed]
        assert S.shrink(seed, 17) == plans[seed][:17]
    for seed in S.WORD_SEEDS[:4]:
        assert S.plan(seed, words=True) == word_plans[seed] != plans[seed]
        assert S.shrink(seed, 17, words=True) == word_plans[seed][:17]
    assert plans[0] != plans[1] and word_plans[0] != word_plans[1]
    for seed, ops in list(plans.items()) + list(word_plans.items()):
        assert len(ops) == S.PLAN_OPS
        m = S.Model()
        for k, op in enumerate(ops):
            assert hasattr(S.Executor, "do_" + op["op"]), f"seed {seed} op {k}: the executor cannot perform {S.fmt(op)}"
            st = m.apply(op).status
            assert st in (S.OK, S.E_ARG, S.E_STATE, S.E_OVERFLOW), f"seed {seed} op {k}: the contract does not decide {S.fmt(op)}"


def test_suite_plans_reach_everything(plans):
    x = S.expectations()
    kinds, tables, widths, statuses, slots, streams, pairs, errs, inputs = set(), set(), set(), set(), set(), set(), set(), 0, set()
    pending_other = False
    total = 0
    for seed, ops in plans.items():
        m = S.Model()
        made = {}                                               # (slot, pass) -> (index of its last OK slot-owned run, passes since)
        for k, op in enumerate(ops):
            st = m.apply(op).status
            total += 1
            errs += st != S.OK
            kinds.add(op["op"])
            statuses.add(st)
            slots.add(op.get("slot"))
            for s in m.slots:
                streams.add(s.shared)
                if s.scan is not None and op["op"].startswith("scan") and st == S.OK:
                    tables.add(s.scan["tab"])
                    widths.add(x.width(s.scan["tab"], s.scan["knob"]))
                    inputs.add((s.scan["tab"], s.scan["inp"]))
            if op["op"] == "scan_bytes" and st == S.OK and (m.slots[1 - op["slot"]].scan or {}).get("pending"):
                pending_other = True
            if op["op"] in S.PASSES:
                for key in made:
                    if key[0] == op["slot"] and key[1] != op["op"]:
                        made[key].add(op["op"])
                if st == S.OK and op["own"]:
                    made[(op["slot"], op["op"])] = set()
                else:
                    made.pop((op["slot"], op["op"]), None)
            if op["op"] in S.PRODUCER_OF and st == S.OK:
                prod = S.PRODUCER_OF[op["op"]]
                for other in made.get((op["slot"], prod), ()):
                    pairs.add((prod, other))
    assert kinds == set(S.KINDS), set(S.KINDS) - kinds
    assert tables == set(S.TABLES) and widths == {2, 4, 8}
    assert inputs == {(t, i) for t in S.TABLES for i in range(len(S.TABLES[t]["inputs"]))}, "an input of the pool is never scanned"
    assert statuses == {S.OK, S.E_ARG, S.E_STATE, S.E_OVERFLOW}
    assert slots >= {0, 1} and streams == {True, False} and pending_other
    assert 0.08 < errs / total < 0.2, f"{errs} of {total} operations are illegal: about one in eight was the plan"
    # the two selections share a buffer, and so do the two replaces: the later one discards the earlier one's result
    shared = {("select", "select_docs"), ("select_docs", "select"), ("replace", "replace_docs"), ("replace_docs", "replace")}
    want = {(a, b) for a in S.PASSES for b in S.PASSES if a != b} - shared
    assert pairs >= want, sorted(want - pairs)
    sizes = {d[1] for t in S.TABLES.values() for d in t["inputs"]}
    assert sizes >= {0, 1, 17, 4095, 4097, S.GROUP - 1, S.GROUP + 1, 300_007, 2_000_003}


def _walk(plans):
    """(seed, k, op, status, model after the operation, the slot's scan before it) over the plans."""
    for seed, ops in plans.items():
        m = S.Model()
        for k, op in enumerate(ops):
            sc = m.slots[op.get("slot", 0)].scan
            before = dict(sc) if sc else None
            yield seed, k, op, m.apply(op).status, m, before


def test_word_plans_reach_everything(word_plans):
    """The filter-bearing family: every table filtered under every record width it can have, a caller's heap, both slots,
    both stream arrangements, every document key, every status from a filter; after an OK filter every pass and every
    reader; every slot-owned result kind (and the text) made before an OK filter and fetched after it."""
    x = S.expectations()
    kinds, filtered, ext, slots, streams, dkeys, statuses, after, late, used = set(), set(), set(), set(), set(), set(), set(), set(), set(), set()
    errs = total = 0
    fresh = {}                                                  # slot -> operations since its last OK filter, None before one
    made = {}                                                   # (slot, fetch kind) -> an OK filter has run since the result was made
    seed_now = None
    for seed, k, op, st, m, before in _walk(word_plans):
        if seed != seed_now:
            seed_now, fresh, made = seed, {}, {}
        total += 1
        errs += st != S.OK
        kinds.add(op["op"])
        slot = op.get("slot", 0)
        if op["op"] == "filter":
            statuses.add(st)
            if st == S.OK:
                sc = m.slots[slot].scan
                filtered.add((sc["tab"], x.width(sc["tab"], sc["knob"])))
                ext.add(sc["ext"])
                slots.add(slot)
                streams.add(m.slots[1].shared)
                dkeys |= {one[4] for one in sc["filt"]}
                used.add(op["f"])
                fresh[slot] = 0
                for key in made:
                    if key[0] == slot:
                        made[key] = True
        elif st == S.OK and fresh.get(slot) is not None and ("slot" in op or op["op"] in S.READERS):
            if op["op"] in S.PASSES + S.READERS and fresh[slot] <= 3 and m.slots[slot].scan and m.slots[slot].scan["filt"]:
                after.add(op["op"])
            fresh[slot] += 1
        if st == S.OK and op["op"] in S.PASSES and op["own"]:
            made[(slot, S.FETCH_OF[op["op"]])] = False
            if op["op"] == "select_docs":
                made[(slot, "sel_fetch")] = False
            if op["op"] == "replace_docs":
                made[(slot, "rp_fetch")] = False
        if st == S.OK and op["op"] == "text":
            made[(slot, "text_fetch")] = False
        if st == S.OK and made.get((slot, op["op"])):
            late.add(op["op"])
    assert kinds == set(S.WORD_KINDS), set(S.WORD_KINDS) - kinds
    want = {(t, x.width(t, knob)) for t in S.TABLES for knob in S.TABLES[t]["knobs"]}
    assert {w for _, w in want} == {2, 4, 8} and filtered == want, sorted(want - filtered)
    assert ext == {True, False} and slots == {0, 1} and streams == {True, False}
    assert dkeys >= {"", "d0", "d1"}, dkeys
    assert statuses == {S.OK, S.E_ARG, S.E_STATE, S.E_OVERFLOW}, statuses
    assert used == {f for f, d in enumerate(S.FILTERS) if d["doc"] != "wrong_n"}, "a descriptor of the pool is never applied"
    assert after >= set(S.PASSES + S.READERS), sorted(set(S.PASSES + S.READERS) - after)
    assert late >= set(S.FETCH_OF.values()) | {"text_fetch"}, sorted((set(S.FETCH_OF.values()) | {"text_fetch"}) - late)
    assert 0.08 < errs / total < 0.2, f"{errs} of {total} operations are illegal: about one in eight was the plan"
    # the bad offsets reach the filter too: each refused with PFAC_E_ARG at least once
    refused = {m.slots[op["slot"]].doc[3] for _, _, op, st, m, _ in _walk(word_plans)
               if op["op"] == "filter" and st == S.E_ARG and S.FILTERS[op["f"]]["doc"] == "slot" and m.slots[op["slot"]].doc}
    assert refused >= {"bad_end", "bad_order"}, refused


def test_word_plans_filter_something_but_not_everything(word_plans):
    """By the reference alone: at least half of the suite's OK filter operations keep a count strictly between 0 and the
    scan's unfiltered count, and for every table at least one does -- the filter is neither the identity nor a wipe."""
    x = S.expectations()
    ok, mid = collections.Counter(), collections.Counter()
    for seed, k, op, st, m, before in _walk(word_plans):
        if op["op"] == "filter" and st == S.OK:
            sc = m.slots[op["slot"]].scan
            ok[sc["tab"]] += 1
            mid[sc["tab"]] += 0 < m._count(sc) < x.count(sc["tab"], sc["inp"], sc["no"])
    print({t: (mid[t], ok[t]) for t in sorted(ok)})
    assert 2 * sum(mid.values()) >= sum(ok.values()) > 100, (sum(mid.values()), sum(ok.values()))
    assert all(mid[t] >= 1 for t in S.TABLES), {t: mid[t] for t in S.TABLES}


def test_filters_compose_by_intersection_in_the_reference():
    """The model's filter state: sorted distinct descriptors, the same records in whatever order they were applied."""
    x = S.expectations()
    t, i, no = "abc2", 2, S.GROUP + 1
    a, b = x.applied(t, 2, ""), x.applied(t, 3, "")
    full, fa, fb, fab = x.scan(t, i, no), x.scan(t, i, no, (a,)), x.scan(t, i, no, (b,)), x.scan(t, i, no, tuple(sorted((a, b))))
    assert 0 < fab[0].size < min(fa[0].size, fb[0].size) < full[0].size
    assert set(zip(fab[0].tolist(), fab[1].tolist())) == set(zip(fa[0].tolist(), fa[1].tolist())) & set(zip(fb[0].tolist(), fb[1].tolist()))
    m = S.Model()
    for op in [dict(op="load_table", tab=t, knob=S.TABLES[t]["knobs"][0]), dict(op="set_flen"), dict(op="scan_bytes", slot=0, inp=i, no=no),
               dict(op="filter", slot=0, f=3, heap="own"), dict(op="filter", slot=0, f=2, heap="own"), dict(op="filter", slot=0, f=3, heap="own")]:
        assert m.apply(op).status == S.OK
    assert m.slots[0].scan["filt"] == tuple(sorted((a, b)))


@pytest.mark.parametrize("seed", S.SEEDS)
def test_plan_passes_on_the_cpu_device(seed, plans):
    stats = S.run(CpuDevice(), plans[seed], S.Model(), seed=seed)
    assert stats["ops"] == S.PLAN_OPS and stats["errors"] > 0


@pytest.mark.parametrize("seed", S.WORD_SEEDS)
def test_word_plan_passes_on_the_cpu_device(seed, word_plans):
    stats = S.run(CpuDevice(), word_plans[seed], S.Model(), seed=f"{seed} (words)")
    assert stats["ops"] == S.PLAN_OPS and stats["errors"] > 0 and stats["filters"] > 0


def first_touch(seed, ops, defect):
    """(index of the first operation the defect changes, index of the operation the executor fails at or None)."""
    dev = CpuDevice([defect])
    ex = S.Executor(dev, S.Model())
    touched = None
    for k, op in enumerate(ops):
        try:
            ex.step(op)
        except AssertionError:
            return (k if touched is None and dev.hit else touched), k
        if dev.hit and touched is None:
            touched = k
    return touched, None


@pytest.mark.parametrize("defect", DEFECTS + WORD_DEFECTS + COUNT_DEFECTS)
def test_every_defect_is_caught(defect, plans, word_plans, count_plans):
    caught = []
    family = {f"{seed} (words)": ops for seed, ops in word_plans.items()} if defect in WORD_DEFECTS else plans
    if defect in COUNT_DEFECTS:
        family = {f"{seed} (counts)": ops for seed, ops in count_plans.items()}
    for seed, ops in family.items():
        touched, failed = first_touch(seed, ops, defect)
        assert failed is None or (touched is not None and failed >= touched), f"seed {seed}: failed at {failed} before the defect acted ({touched})"
        if failed is not None:
            with pytest.raises(AssertionError) as e:
                S.run(CpuDevice([defect]), ops, S.Model(), seed=seed)
            assert f"session seed {seed}, operation {failed} " in str(e.value) and e.value.op_index == failed
            caught.append((seed, touched, failed))
            if len(caught) == 2:                                # (two plans are proof enough; every plan costs a second)
                break
    assert caught, f"no suite plan notices {defect}"
    print(f"{defect}: caught by plans (seed, first touched, failed at) {caught}")


def test_shrink_keeps_a_failure(plans):
    """A failing history cut just past the failing operation still fails there; cut before it, it passes."""
    defect = "overflowed_scan_hands_out_records"
    for seed, ops in plans.items():
        touched, failed = first_touch(seed, ops, defect)
        if failed is not None:
            with pytest.raises(AssertionError):
                S.run(CpuDevice([defect]), S.shrink(seed, failed + 1), S.Model(), seed=seed)
            S.run(CpuDevice([defect]), S.shrink(seed, failed), S.Model(), seed=seed)
            return
    raise AssertionError("no plan to shrink")


# ---------------------------------------------------------------------------
# the third family: the per-pattern counts

def test_the_pool_tables_with_an_injective_idmap():
    """Counts of these tables are compared state for state as well as by pattern id: all the literal tables (the
    unreachable states of `dups` report the losing lines' ids), not the two class tables."""
    x = S.expectations()
    assert {t for t in S.TABLES if x.injective(t)} == set(S.TABLES) - {"cclass", "negcc"}
    for t in S.TABLES:
        assert x.n_ids(t) > int(np.asarray(x.table(t).idmap).max())
        if x.injective(t):
            part = ("scan", t, 0, x.input_size(t, 0), ())
            assert int(x.part_states(part).sum()) == int(x.part_counts(part).sum()) == x.count(*part[1:])


def test_count_plans_are_deterministic_and_well_formed(count_plans, word_plans):
    for seed in S.COUNT_SEEDS[:3]:
        assert S.plan(seed, counts=True) == count_plans[seed] != word_plans[seed]
        assert S.shrink(seed, 23, counts=True) == count_plans[seed][:23]
    assert count_plans[0] != count_plans[1]
    for seed, ops in count_plans.items():
        assert len(ops) == S.PLAN_OPS
        m = S.Model()
        for k, op in enumerate(ops):
            assert hasattr(S.Executor, "do_" + op["op"]), f"seed {seed} op {k}: the executor cannot perform {S.fmt(op)}"
            assert ("cknob" in op) == (op["op"] == "load_table")
            st = m.apply(op).status
            assert st in (S.OK, S.E_ARG, S.E_STATE, S.E_OVERFLOW), f"seed {seed} op {k}: the contract does not decide {S.fmt(op)}"


def test_count_plans_are_the_same_in_another_process(count_plans):
    """The plans replay between processes (another hash seed: no set or dict order leaks into them)."""
    seeds = S.COUNT_SEEDS[:3]
    code = ("import hashlib, json, session as S; print(hashlib.sha256(json.dumps([S.plan(s, counts=True) for s in %r], sort_keys=True).encode()).hexdigest())" % seeds)
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONHASHSEED="12345", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True, timeout=300).stdout.split()[-1]
    assert out == hashlib.sha256(json.dumps([count_plans[s] for s in seeds], sort_keys=True).encode()).hexdigest()


def _walk_models(plans):
    """(seed, k, op, status, the model before the operation, the model after it) over the plans."""
    for seed, ops in plans.items():
        m = S.Model()
        for k, op in enumerate(ops):
            was = copy.deepcopy(m)
            yield seed, k, op, m.apply(op).status, was, m


def test_count_plans_reach_everything(count_plans):
    """Conditions, not measurements: the histories the count family exists for all occur in the suite's 24 plans."""
    x = S.expectations()
    kinds, ok, sel_ok, late, errs, overlays = set(), set(), set(), set(), set(), set()
    most_parts, mixed, errors, total = 0, False, 0, 0
    since = {}                                                  # (seed, slot) -> what happened since the slot's last OK own count
    dropped = {}                                                # (seed, slot) -> its scan was dropped by a reserve_grow
    for seed, k, op, st, was, m in _walk_models(count_plans):
        kind, slot = op["op"], op.get("slot", 0)
        kinds.add(kind)
        total += 1
        errors += st != S.OK
        ws, s = was.slots[slot], m.slots[slot]
        sc = ws.scan
        ev = since.get((seed, slot))
        if kind == "load_table":
            for key in since:
                if key[0] == seed:
                    since[key].add("upload")
        elif ev is not None and st == S.OK:
            if kind in ("scan_bytes", "scan_ext", "scan_start"):
                ev.add("scan")
            elif kind == "reserve_grow" and sc is not None and s.scan is None:
                ev.add("grow")
            elif kind == "filter":
                ev.add("filter")
            elif kind in S.PASSES:
                ev.add("pass")
            elif kind in COUNT_OPS[:2] and op["dst"] == "caller":
                ev.add("caller")
        elif ev is not None and kind in COUNT_OPS[:2]:
            ev.add("refused")
        if kind == "reserve_grow":
            dropped[(seed, slot)] = sc is not None and s.scan is None
        elif kind.startswith("scan") and st == S.OK:
            dropped[(seed, slot)] = False
        if kind == "count" and st == S.OK:
            ok |= {("dst", op["dst"], op["acc"]), ("slot", slot), ("ext", sc["ext"]), ("filtered", bool(sc["filt"])),
                   ("empty", was._count(sc) == 0), ("width", x.width(sc["tab"], sc["knob"])), ("shared", slot == 1 and ws.shared)}
            bins = int(S.CKNOBS[was.cknob].get("PFAC_COUNT_BINS", 0))
            overlays.add((was.cknob, bool(bins) and int(x.table(sc["tab"]).num_final) > bins))
        if kind == "count_sel" and st == S.OK:
            sel_ok |= {("kind", ws.sel["kind"]), ("sel", op["sel"]), ("dst", op["dst"], op["acc"])}
        if kind in COUNT_OPS[:2] and st == S.OK and op["dst"] == "own":
            since[(seed, slot)] = set()
            parts = s.cnt["parts"]
            most_parts = max(most_parts, len(parts))
            mixed |= len({p[0] == "scan" for p in parts}) == 2
        if kind == "cnt_fetch":
            if st == S.OK:
                late |= ev
            else:
                errs.add(("cnt_fetch", "E_STATE"))
        if kind == "count" and st != S.OK:
            if sc is None:
                errs.add(("count", "E_STATE after reserve" if dropped.get((seed, slot)) else "E_STATE no scan"))
            elif sc["pending"]:
                errs.add(("count", "E_STATE pending"))
            elif sc["gen"] != was.gen:
                errs.add(("count", "E_STATE earlier table"))
            elif st == S.E_OVERFLOW:
                errs.add(("count", "E_OVERFLOW"))
            elif st == S.E_STATE:
                errs.add(("count", "E_STATE accumulate onto an earlier generation"))
            else:
                assert st == S.E_ARG
                errs.add(("count", "E_ARG " + ("n_states " + op["ns"] if op["ns"] != "ok" else "d_counts" if op["dst"] == "misaligned" else "heap")))
        if kind == "count_sel" and st != S.OK:
            if st == S.E_ARG:
                errs.add(("count_sel", "E_ARG " + op["sel"]))
            elif ws.sel is None or sc is None:
                errs.add(("count_sel", "E_STATE no selection"))
            elif ws.sel["seq"] != sc["seq"]:
                errs.add(("count_sel", "E_STATE stale"))
            elif sc["gen"] != was.gen:
                errs.add(("count_sel", "E_STATE earlier table"))
            elif op["sel"] == "own" and not ws.sel["own"]:
                errs.add(("count_sel", "E_STATE NULL for a caller's selection"))
            else:
                errs.add(("count_sel", "E_STATE accumulate onto an earlier generation"))
    assert kinds == set(S.COUNT_KINDS), set(S.COUNT_KINDS) - kinds
    want = {("dst", d, a) for d in ("own", "caller") for a in (False, True)} | {("slot", 0), ("slot", 1), ("ext", True), ("ext", False),
            ("filtered", True), ("filtered", False), ("empty", True), ("width", 2), ("width", 4), ("width", 8), ("shared", True)}
    assert ok >= want, sorted(want - ok, key=str)
    want = {(c, "PFAC_COUNT_BINS" in d) for c, d in enumerate(S.CKNOBS)}     # every overlay; where it sets the bins, the cache regime
    assert overlays >= want, sorted(want - overlays)
    want = {("kind", "whole"), ("kind", "docs"), ("sel", "own"), ("sel", "caller")} | {("dst", d, a) for d in ("own", "caller") for a in (False, True)}
    assert sel_ok >= want, sorted(want - sel_ok, key=str)
    want = {"scan", "upload", "grow", "filter", "pass", "caller", "refused"}
    assert late >= want, sorted(want - late)
    assert most_parts >= 3 and mixed, (most_parts, mixed)
    want = {("count", e) for e in ("E_STATE no scan", "E_STATE pending", "E_STATE earlier table", "E_STATE after reserve", "E_OVERFLOW",
                                   "E_ARG n_states minus", "E_ARG n_states plus", "E_ARG n_states zero", "E_ARG heap", "E_ARG d_counts",
                                   "E_STATE accumulate onto an earlier generation")}
    want |= {("count_sel", e) for e in ("E_STATE no selection", "E_STATE stale", "E_STATE earlier table", "E_STATE NULL for a caller's selection",
                                       "E_ARG junk", "E_ARG misaligned")} | {("cnt_fetch", "E_STATE")}
    assert errs >= want, sorted(want - errs)
    assert 0.08 < errors / total < 0.25, f"{errors} of {total} operations are illegal"


def test_count_plans_count_something(count_plans):
    """By the reference alone: the count vectors the plans compare are not trivial."""
    x = S.expectations()
    rich = set()
    filtered = selected = summed = False
    for seed, k, op, st, was, m in _walk_models(count_plans):
        if st != S.OK or op["op"] not in COUNT_OPS:
            continue
        s = m.slots[op["slot"]]
        if op["op"] == "cnt_fetch" or op["dst"] == "caller":
            held = s.cnt if op["op"] == "cnt_fetch" else s.cbuf
            parts = held["parts"]
            vec = x.sum_counts(held["tab"], parts)
            if int((vec > 0).sum()) >= 2:
                rich.add(seed)
            summed |= len(parts) > 1 and not np.array_equal(vec, x.part_counts(parts[-1]))
        if op["op"] == "cnt_fetch":
            continue
        part = (s.cnt if op["dst"] == "own" else s.cbuf)["parts"][-1]
        if part[0] == "scan" and part[4]:
            filtered |= not np.array_equal(x.part_counts(part), x.state_counts(*part[1:4]))
        if part[0] != "scan":
            selected |= not np.array_equal(x.part_counts(part), x.state_counts(part[1], part[2], part[3], part[5]))
    assert 2 * len(rich) >= len(count_plans), sorted(rich)
    assert filtered and selected and summed, (filtered, selected, summed)


@pytest.mark.parametrize("seed", S.COUNT_SEEDS)
def test_count_plan_passes_on_the_cpu_device(seed, count_plans):
    stats = S.run(CpuDevice(), count_plans[seed], S.Model(), seed=f"{seed} (counts)")
    assert stats["ops"] == S.PLAN_OPS and stats["errors"] > 0 and stats["counts"] > 0


def test_shrink_keeps_a_count_failure(count_plans):
    defect = "plain_count_does_not_zero"
    for seed, ops in count_plans.items():
        touched, failed = first_touch(seed, ops, defect)
        if failed is not None:
            with pytest.raises(AssertionError):
                S.run(CpuDevice([defect]), S.shrink(seed, failed + 1, counts=True), S.Model(), seed=seed)
            S.run(CpuDevice([defect]), S.shrink(seed, failed, counts=True), S.Model(), seed=seed)
            return
    raise AssertionError("no plan to shrink")


# ---------------------------------------------------------------------------
# the fourth family: the line path (split, matching documents, context lines, gather)

# SHA-256 of json.dumps([plan(seed, lines=True) for seed in LINE_SEEDS], sort_keys=True): the line plans are pinned too, so
# that a later family, or a change to the planner, cannot move them unnoticed.
LINE_PLANS_SHA256 = "6ed0d24f240ed2d015f4c4cd11eadae22bbe72f6e6aa636af66fee9a15bb946a"


def test_the_plans_with_the_line_path_are_pinned(line_plans):
    assert [seed for seed in line_plans] == S.LINE_SEEDS and len(S.LINE_SEEDS) == 24
    assert hashlib.sha256(json.dumps([line_plans[seed] for seed in S.LINE_SEEDS], sort_keys=True).encode()).hexdigest() == LINE_PLANS_SHA256


def test_line_plans_are_deterministic_and_well_formed(line_plans, count_plans):
    for seed in S.LINE_SEEDS[:3]:
        assert S.plan(seed, lines=True) == line_plans[seed] != count_plans[seed]
        assert S.shrink(seed, 23, lines=True) == line_plans[seed][:23]
    assert line_plans[0] != line_plans[1]
    for seed, ops in line_plans.items():
        assert len(ops) == S.LINE_PLAN_OPS
        m = S.Model()
        for k, op in enumerate(ops):
            assert hasattr(S.Executor, "do_" + op["op"]), f"seed {seed} op {k}: the executor cannot perform {S.fmt(op)}"
            st = m.apply(op).status
            assert st in (S.OK, S.E_ARG, S.E_STATE, S.E_OVERFLOW), f"seed {seed} op {k}: the contract does not decide {S.fmt(op)}"


def test_line_plans_are_the_same_in_another_process(line_plans):
    seeds = S.LINE_SEEDS[:3]
    code = ("import hashlib, json, session as S; print(hashlib.sha256(json.dumps([S.plan(s, lines=True) for s in %r], sort_keys=True).encode()).hexdigest())" % seeds)
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONHASHSEED="54321", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True, timeout=300).stdout.split()[-1]
    assert out == hashlib.sha256(json.dumps([line_plans[s] for s in seeds], sort_keys=True).encode()).hexdigest()


LINE_STATUSES = {"split": {S.OK, S.E_ARG}, "doc_fetch": {S.OK, S.E_STATE, S.E_ARG}, "matching": {S.OK, S.E_ARG, S.E_STATE, S.E_OVERFLOW},
                 "context": {S.OK, S.E_ARG, S.E_STATE, S.E_OVERFLOW}, "ids_fetch": {S.OK, S.E_STATE},
                 "gather": {S.OK, S.E_ARG, S.E_STATE, S.E_OVERFLOW}, "ga_fetch": {S.OK, S.E_ARG, S.E_STATE}, "gaoff_fetch": {S.OK, S.E_STATE}}


def _between_kind(op, st, was, m):
    """The name in S.BETWEEN of an operation that succeeded, or None."""
    kind, slot = op["op"], op.get("slot", 0)
    if st != S.OK:
        return None
    if kind in ("scan_bytes", "scan_ext", "scan_start"):
        return "scan"
    if kind == "load_table":
        return "upload"
    if kind == "reserve_grow":
        return "grow"
    return kind if kind in S.BETWEEN else None


def test_line_plans_reach_everything(line_plans):
    """Conditions, not measurements: over S.LINE_SEEDS every new operation meets every documented status, every argument
    form, both slots and the shared stream; every (producer, intervening call, late fetch) order occurs; and the splits
    produce every line shape."""
    x = S.expectations()
    kinds, seen, forms, where, orders, shapes, errs = set(), collections.defaultdict(set), set(), set(), set(), set(), set()
    errors = total = 0
    since = {}                                                  # (seed, slot, fetch) -> (producer, what has happened on the slot since)
    for seed, k, op, st, was, m in _walk_models(line_plans):
        kind, slot = op["op"], op.get("slot", 0)
        kinds.add(kind)
        total += 1
        errors += st != S.OK
        ws, s = was.slots[slot], m.slots[slot]
        b = _between_kind(op, st, was, m)
        for key, (prod, mid) in since.items():
            if key[0] == seed and b is not None and (kind == "load_table" or key[1] == slot):
                mid.add(b)
        if kind in S.LINE_OPS:
            seen[kind].add(st)
            where |= {(kind, "slot", slot), (kind, "shared", slot == 1 and ws.shared)}
        if kind in S.LATE and st == S.OK:
            own = kind in ("split", "set_doc") or op["out"] == "own"
            for f in S.LATE[kind]:
                if own and (f != "gaoff_fetch" or op["oo"] == "own"):
                    since[(seed, slot, f)] = (kind, set())
                else:
                    since.pop((seed, slot, f), None)
        elif kind in S.LATE or kind in ("matching", "context", "gather"):
            for f in S.LATE.get(kind, ()):                       # (a refused call of the same pass discards the result)
                if kind not in ("split", "set_doc"):
                    since.pop((seed, slot, f), None)
        if kind in ("doc_fetch", "ids_fetch", "ga_fetch", "gaoff_fetch") and st == S.OK and (seed, slot, kind) in since:
            prod, mid = since[(seed, slot, kind)]
            orders |= {(prod, b2, kind) for b2 in mid}
        # -- the split
        if kind == "split":
            sc = ws.scan
            if st == S.OK:
                off, nd, tail = x.split(op["tab"], op["inp"], op["nb"], op["delim"])
                d = x.delims(op["tab"], op["inp"])
                forms |= {("split", "src", op["src"]), ("split", "delim", "frequent" if op["delim"] == d[0] else "rare" if op["delim"] == d[1] else "absent")}
                if sc is not None:
                    forms.add(("split", "nb", "n_owned" if op["nb"] == sc["no"] else "zero" if op["nb"] == 0 else "smaller" if op["nb"] < sc["no"] else "larger"))
                    forms.add(("split", "pending", sc["pending"]))
                forms.add(("split", "table", was.tab is not None))
                lens = np.diff(off.astype(np.int64))
                if (lens == 1).sum() >= 2 and nd >= 3:
                    shapes.add("runs of delimiters")
                if op["nb"] and tail != op["nb"]:
                    shapes.add("unterminated tail")
                if op["nb"] and tail == op["nb"]:
                    shapes.add("terminated last line")
                if op["nb"] and nd == 1 and tail == 0:
                    shapes.add("no delimiter")
                if nd > 64 * 64:
                    shapes.add("more than 64 x 64 documents")
                if op["nb"] > 64 * S.TILE:
                    shapes.add("more than 64 tiles")
            else:
                errs.add(("split", "delim %d" % op["delim"] if not 0 <= op["delim"] <= 255 else "over" if op["nb"] == "over" else op["src"]))
                assert (s.doc, s.doc_gen) == (ws.doc, ws.doc_gen)
        # -- what the split's offsets do to the document passes
        if kind in ("segment", "select_docs", "filter") and ws.doc is not None and ws.doc[3].startswith("split:") and ws.scan is not None:
            if st == S.OK and ws.doc[2] == ws.scan["no"] and (kind != "filter" or S.FILTERS[op["f"]]["doc"] == "slot"):
                forms.add(("after a split", kind, "NULL offsets"))
            if st == S.E_ARG and ws.doc[2] != ws.scan["no"] and (kind != "filter" or S.FILTERS[op["f"]]["doc"] == "slot"):
                errs.add(("after a split of other bytes", kind))
        if kind == "replace_docs" and st == S.E_STATE and ws.sel is not None and ws.sel["kind"] == "docs" and ws.doc is not None \
                and ws.doc[3].startswith("split:") and ws.sel["doc_gen"] != ws.doc_gen and ws.scan is not None and ws.sel["seq"] == ws.scan["seq"]:
            errs.add(("replace_docs", "stale after a split"))
        if kind == "doc_fetch":
            if st == S.OK:
                forms.add(("doc_fetch", "after", "split" if ws.doc[3].startswith("split:") else "set_doc"))
                forms.add(("doc_fetch", "window", "all" if op["first"] == 0 and op["n"] == x.offsets(*ws.doc).size else "part"))
        # -- matching and context
        if kind in ("matching", "context"):
            if st == S.OK:
                forms |= {(kind, "first", op["first"]), (kind, "out", op["out"]), (kind, "flags", op["flags"])}
                if kind == "context":
                    nd = int(x.doc_first(*s.dm[0][:2]).size) - 1
                    for v in (op["before"], op["after"]):
                        forms.add(("context", "window", "0" if v == 0 else "1" if v == 1 else "2^64-1" if v == S.U64_MAX else "> n_docs" if v > nd else "some"))
            elif st == S.E_OVERFLOW:
                errs.add((kind, "small"))
            elif st == S.E_STATE:
                errs.add((kind, "no slot-owned doc_first" + (" (it went to the caller)" if ws.seg is not None else "")))
            else:
                errs.add((kind, "flags %d" % op["flags"] if op["flags"] > (0 if kind == "context" else 1) else "n_docs" if op["nd"] != "ok" else "misaligned"))
            assert st == S.OK or s.dm is None
        elif kind not in ("ids_fetch",) and st is not None:
            assert s.dm == ws.dm, f"seed {seed} op {k}: {kind} dropped the ids"
        # -- the gather
        if kind == "gather":
            if st == S.OK:
                forms.add(("gather", "args", op["src"] == "slot", op["off"] == "slot", op["ids"] == "own", op["out"] == "own", op["oo"] == "own"))
                forms.add(("gather", "ids", op["ids"]))
            elif st == S.E_OVERFLOW:
                errs.add(("gather", "small"))
            elif st == S.E_STATE:
                errs.add(("gather", "n_docs" if op["nd"] != "ok" else "no offsets" if ws.doc is None else
                          "the ids went to the caller" if ws.dm is not None else "no ids"))
            else:
                off = x.offsets(*ws.doc).astype(np.int64) if ws.doc is not None else None
                errs.add(("gather", "n_ids" if op["ni"] != "ok" else "misaligned input" if op["src"] == "odd" else "misaligned output" if op["out"] == "odd" else
                          "bad id" if op["ids"] == "bad_id" else "a selected document passes n_bytes" if off is not None and op["nb"] < off[-1] else
                          "selected offsets"))
    missing = {"kinds": sorted(set(S.LINE_KINDS) - kinds),
               "statuses": sorted((k2, S.STATUS_NAMES[v]) for k2 in LINE_STATUSES for v in LINE_STATUSES[k2] - seen[k2])}
    assert all(seen[k2] <= LINE_STATUSES[k2] for k2 in seen), "a status the header does not document"
    want = {(k, "slot", sl) for k in S.LINE_OPS for sl in (0, 1)} | {(k, "shared", True) for k in S.LINE_OPS}
    missing["slots and streams"] = sorted(want - where, key=str)
    want = {("split", "src", v) for v in ("slot", "caller")} | {("split", "delim", v) for v in ("frequent", "rare", "absent")}
    want |= {("split", "nb", v) for v in ("n_owned", "smaller", "zero")} | {("split", "pending", True), ("split", "table", False)}
    want |= {("after a split", k2, "NULL offsets") for k2 in ("segment", "select_docs", "filter")}
    want |= {("doc_fetch", "after", "split"), ("doc_fetch", "after", "set_doc"), ("doc_fetch", "window", "all"), ("doc_fetch", "window", "part")}
    want |= {(k2, "first", v) for k2 in ("matching", "context") for v in ("own", "seg", "docsel")}
    want |= {(k2, "out", v) for k2 in ("matching", "context") for v in ("own", "caller")} | {("matching", "flags", 0), ("matching", "flags", 1)}
    want |= {("context", "window", v) for v in ("0", "1", "> n_docs", "2^64-1")}
    want |= {("gather", "args") + tuple(bool(c >> j & 1) for j in range(5)) for c in range(32)}
    want |= {("gather", "ids", v) for v in S.ID_FORMS if v != "bad_id"}
    missing["argument forms"] = sorted(want - forms, key=str)
    want = {("split", v) for v in ("delim 256", "delim -1", "over", "odd")}
    want |= {("after a split of other bytes", k2) for k2 in ("segment", "select_docs", "filter")} | {("replace_docs", "stale after a split")}
    want |= {(k2, v) for k2 in ("matching", "context") for v in ("small", "no slot-owned doc_first", "no slot-owned doc_first (it went to the caller)",
                                                                  "n_docs", "misaligned")}
    want |= {("matching", "flags 2"), ("context", "flags 1")}
    want |= {("gather", v) for v in ("small", "n_docs", "no offsets", "the ids went to the caller", "no ids", "n_ids", "misaligned input",
                                     "misaligned output", "bad id", "a selected document passes n_bytes", "selected offsets")}
    missing["errors"] = sorted(want - errs)
    want = {(p, b2, f) for p, fs in S.LATE.items() for f in fs for b2 in S.BETWEEN
            if b2 not in {"doc_fetch": ("split", "set_doc"), "ids_fetch": ("matching", "context"), "ga_fetch": ("gather",), "gaoff_fetch": ("gather",)}[f]}
    missing["orders"] = sorted(want - orders)
    want = {"runs of delimiters", "unterminated tail", "terminated last line", "no delimiter", "more than 64 x 64 documents", "more than 64 tiles"}
    missing["line shapes"] = sorted(want - shapes)
    missing = {k2: v for k2, v in missing.items() if v}
    assert not missing, "the line plans never reach:\n" + "\n".join(f"  {k2}: {v}" for k2, v in missing.items())
    assert 0.08 < errors / total < 0.25, f"{errors} of {total} operations are illegal"


@pytest.mark.parametrize("seed", S.LINE_SEEDS)
def test_line_plan_passes_on_the_cpu_device(seed, line_plans):
    stats = S.run(CpuDevice(), line_plans[seed], S.Model(), seed=f"{seed} (lines)")
    assert stats["ops"] == S.LINE_PLAN_OPS and stats["errors"] > 0 and stats["splits"] + stats["matchings"] + stats["gathers"] > 0


@pytest.mark.parametrize("defect", LINE_DEFECTS)
def test_every_line_defect_is_caught(defect, line_plans):
    caught = []
    for seed, ops in line_plans.items():
        seed = f"{seed} (lines)"
        touched, failed = first_touch(seed, ops, defect)
        assert failed is None or (touched is not None and failed >= touched), f"seed {seed}: failed at {failed} before the defect acted ({touched})"
        if failed is not None:
            with pytest.raises(AssertionError) as e:
                S.run(CpuDevice([defect]), ops, S.Model(), seed=seed)
            assert f"session seed {seed}, operation {failed} " in str(e.value) and e.value.op_index == failed
            caught.append((seed, touched, failed))
            if len(caught) == 2:
                break
    assert caught, f"no line plan notices {defect}"
    print(f"{defect}: caught by plans (seed, first touched, failed at) {caught}")


def test_shrink_keeps_a_line_failure(line_plans):
    defect = "failed_matching_keeps_the_ids"
    for seed, ops in line_plans.items():
        touched, failed = first_touch(seed, ops, defect)
        if failed is not None:
            with pytest.raises(AssertionError):
                S.run(CpuDevice([defect]), S.shrink(seed, failed + 1, lines=True), S.Model(), seed=seed)
            S.run(CpuDevice([defect]), S.shrink(seed, failed, lines=True), S.Model(), seed=seed)
            return
    raise AssertionError("no plan to shrink")


# ---------------------------------------------------------------------------
# the fifth family: the case fold (pfac_table_set_case_fold as a piece of context state with a life of its own)

@pytest.fixture(scope="module")
def fold_plans():
    return {seed: S.plan(seed, fold=True) for seed in S.FOLD_SEEDS}


# SHA-256 of json.dumps([plan(seed, fold=True) for seed in FOLD_SEEDS], sort_keys=True): pinned like the four before it.
FOLD_PLANS_SHA256 = "f014f6014658aca7e43593b13a03e94e3b839eb6e46f7302d91fc5d6b0162f0b"


def test_the_plans_with_the_fold_are_pinned(fold_plans):
    assert [seed for seed in fold_plans] == S.FOLD_SEEDS and len(S.FOLD_SEEDS) == 24
    assert hashlib.sha256(json.dumps([fold_plans[seed] for seed in S.FOLD_SEEDS], sort_keys=True).encode()).hexdigest() == FOLD_PLANS_SHA256


def test_fold_plans_are_deterministic_and_well_formed(fold_plans, line_plans):
    for seed in S.FOLD_SEEDS[:3]:
        assert S.plan(seed, fold=True) == fold_plans[seed] != line_plans[seed]
        assert S.shrink(seed, 23, fold=True) == fold_plans[seed][:23]
    assert fold_plans[0] != fold_plans[1]
    for seed, ops in fold_plans.items():
        assert len(ops) == S.FOLD_PLAN_OPS
        m = S.Model()
        for k, op in enumerate(ops):
            assert hasattr(S.Executor, "do_" + op["op"]), f"seed {seed} op {k}: the executor cannot perform {S.fmt(op)}"
            st = m.apply(op).status
            assert st in (S.OK, S.E_ARG, S.E_STATE, S.E_OVERFLOW), f"seed {seed} op {k}: the contract does not decide {S.fmt(op)}"


def test_fold_plans_are_the_same_in_another_process(fold_plans):
    seeds = S.FOLD_SEEDS[:3]
    code = ("import hashlib, json, session as S; print(hashlib.sha256(json.dumps([S.plan(s, fold=True) for s in %r], sort_keys=True).encode()).hexdigest())" % seeds)
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONHASHSEED="2468", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True, timeout=300).stdout.split()[-1]
    assert out == hashlib.sha256(json.dumps([fold_plans[s] for s in seeds], sort_keys=True).encode()).hexdigest()


def _rows(scan):
    return set(zip(scan[0].tolist(), scan[1].tolist()))


def test_the_old_pool_is_what_it_was_and_the_new_tables_say_nocase():
    assert list(S.POOL)[:9] == list(S.TABLES) and set(S.POOL) - set(S.TABLES) == set(S.FOLD_TABLES) == {"wordsi", "symi", "cclassi", "root1i"}
    x = S.expectations()
    for t in S.TABLES:
        assert S.POOL[t]["inputs"][:-1] == S.TABLES[t]["inputs"] and S.POOL[t]["knobs"] == S.TABLES[t]["knobs"]
        assert not x.table(t).ignore_case
    for t in S.FOLD_TABLES:
        assert x.table(t).ignore_case and S.POOL[t]["nocase"]
        assert set(S.WORD_TAB[t]) == set(range(0x61, 0x7B))
    assert x.width("wordsi", S.FOLD_TABLES["wordsi"]["knobs"][0]) == 2 and x.width("symi", S.FOLD_TABLES["symi"]["knobs"][0]) == 4
    sizes = {t: [d[1] for d in S.FOLD_TABLES[t]["inputs"]] for t in S.FOLD_TABLES}
    assert sizes["wordsi"] == [300_007, 300_007, S.GROUP + 1, 4097, 17] and sizes["symi"] == [70_001, 4095, 1]
    assert sizes["root1i"] == [3 * S.TILE + 11, 17] and x.count("wordsi", 1, 300_007, (), True) == 0 and 300_007 >= 64 * S.TILE


def test_the_fold_adds_records_on_every_input_of_the_new_tables():
    """By the references alone: folded = the table's CPU matcher over nocaseref.fold(input), exact = the same matcher over
    the input as written.  For the three literal tables an exact match is a run of bytes the fold leaves alone, so the
    folded records CONTAIN the exact ones; they contain them strictly on every input with a letter in it (not on the
    matchless input of wordsi, and not on the one byte of symi, an E, where both are empty).  cclassi is no superset and
    cannot be: its one-byte negated class [^a-z0-9 ] reports every upper-case letter of the exact scan and none of them
    once the input is folded -- there the fold both adds records ([A-C]x over Ax, Bx, aX ...) and takes some away."""
    x = S.expectations()
    for t in S.FOLD_TABLES:
        for i, (name, n, style) in enumerate(S.FOLD_TABLES[t]["inputs"]):
            exact, folded = _rows(x.scan(t, i, n)), _rows(x.scan(t, i, n, (), True))
            print(t, name, len(exact), len(folded))
            if t == "cclassi":
                assert folded - exact and exact - folded, (t, name)
                lost = {p for p, k in exact - folded}
                assert all(0x41 <= int(x.input(t, i)[p]) <= 0x5A or 0x41 <= int(x.input(t, i)[p + 1]) <= 0x5A for p in lost)
            elif style == "nomatch" or n == 1:
                assert folded == exact == set(), (t, name)
            else:
                assert folded > exact, (t, name)


def test_every_old_table_has_an_input_the_fold_changes():
    """... except dense2, whose three symbols are 0xDE, 0xEB and 0xAC: no line of it holds a letter, so no input exists
    for which the fold changes its records (a letter of the input is outside the alphabet folded or not)."""
    x = S.expectations()
    for t in S.TABLES:
        differs = [i for i in range(len(S.POOL[t]["inputs"])) if x.fold_differs(t, i)]
        if t == "dense2":
            letters = set(range(0x41, 0x5B)) | set(range(0x61, 0x7B))
            assert not letters & set(b"".join(x.tinfo(t)["lines"])) and not differs
        else:
            assert differs, t
    assert not any(x.fold_differs("abc2", i) for i in range(4)) and x.fold_differs("abc2", 4)


def test_the_folded_class_reference_against_the_oracle():
    """nocaseref.folded_classes on the class file of cclassi: element for element the sets oracle/charclass_oracle.py
    parses from the same file with its letters written in lower case by hand ([^A] -> [^a]: the LISTED set is folded, the
    negation complements it), and the lengths ClassMatcher takes from them."""
    cco = S._ClassMatcher.__init__.__globals__["cco"]
    by_hand = b"[a-c]x\n" b"[^a]b\n" b"[^a-z0-9 ]\n" b"q[0-9][0-9]\n" b"ax\n" b"b[x-z]\n" b"[a-c]x\n"
    got, want = nocaseref.folded_classes(S.CCLASSI), cco.parse(by_hand)
    assert [len(p) for p in got] == [len(p) for p in want]
    for a, b in zip(got, want):
        for sa, sb in zip(a, b):
            np.testing.assert_array_equal(sa, sb)
    assert not any(s[0x41:0x5B].any() for p in got[:1] + got[3:] for s in p)       # (no listed upper-case letter is left)
    np.testing.assert_array_equal(np.flatnonzero(~got[1][0]), [ord("a")])          # [^A]: everything but a
    assert got[2][0][0x41:0x5B].all()                                              # [^a-z0-9 ]: A-Z pass -- but a folded input has none
    np.testing.assert_array_equal(nocaseref.fold_class_set(cco.parse(b"[Z-a]\n")[0][0]).nonzero()[0], [0x5B, 0x5C, 0x5D, 0x5E, 0x5F, 0x60, 0x61, 0x7A])
    x = S.expectations()
    assert x.tinfo("cclassi")["matcher"].parsed is not None and x.tinfo("cclassi")["ll"].tolist() == [0, 2, 2, 1, 3, 2, 2, 2]


@pytest.mark.parametrize("seed", S.FOLD_SEEDS)
def test_fold_plan_passes_on_the_cpu_device(seed, fold_plans):
    stats = S.run(CpuDevice(), fold_plans[seed], S.Model(), seed=f"{seed} (fold)")
    assert stats["ops"] == S.FOLD_PLAN_OPS and stats["errors"] > 0 and stats["folded"] > 0 and stats["toggles"] + stats["modes"] > 0


@pytest.mark.parametrize("defect", FOLD_DEFECTS)
def test_every_fold_defect_is_caught(defect, fold_plans):
    caught = []
    for seed, ops in fold_plans.items():
        seed = f"{seed} (fold)"
        touched, failed = first_touch(seed, ops, defect)
        assert failed is None or (touched is not None and failed >= touched), f"seed {seed}: failed at {failed} before the defect acted ({touched})"
        if failed is not None:
            with pytest.raises(AssertionError) as e:
                S.run(CpuDevice([defect]), ops, S.Model(), seed=seed)
            assert f"session seed {seed}, operation {failed} " in str(e.value) and e.value.op_index == failed
            caught.append((seed, touched, failed, S.fmt(ops[failed])))
            if len(caught) == 2:
                break
    assert caught, f"no fold plan notices {defect}"
    print(f"{defect}: caught by plans (seed, first touched, failed at, the failing operation) {caught}")


def test_shrink_keeps_a_fold_failure(fold_plans):
    defect = "toggle_reaches_pending_scan"
    for seed, ops in fold_plans.items():
        touched, failed = first_touch(seed, ops, defect)
        if failed is not None:
            with pytest.raises(AssertionError):
                S.run(CpuDevice([defect]), S.shrink(seed, failed + 1, fold=True), S.Model(), seed=seed)
            S.run(CpuDevice([defect]), S.shrink(seed, failed, fold=True), S.Model(), seed=seed)
            return
    raise AssertionError("no plan to shrink")


def _est_dense(dense, knob, width, n_avail, count):
    """The stand-in's staging rule (CpuDevice.scan_finish), for the reach test: the mode after a scan's finish."""
    tiles = (n_avail + 4095) // 4096
    if "PFAC_DENSE" in KNOBS[knob] or tiles < 64 or width == 8:
        return dense
    return count > DENSE_PER_TILE * tiles // 4


BEHIND = ("filter",) + S.PASSES + ("count", "count_sel", "split", "matching", "context", "gather")


def test_fold_plans_reach_everything(fold_plans):
    """Conditions, not measurements, over S.FOLD_SEEDS."""
    x = S.expectations()
    kinds, where, tables, widths, placed, behind, fold_statuses = set(), set(), set(), set(), set(), set(), set()
    toggle_while_pending = off_after_upload = late_records = flipped = False
    errors = total = 0
    seed_now = None
    for seed, k, op, st, was, m in _walk_models(fold_plans):
        if seed != seed_now:
            seed_now, dense, last_mode, on_at_upload, pending_mode = seed, False, None, False, {}
        kind, slot = op["op"], op.get("slot", 0)
        kinds.add(kind)
        total += 1
        errors += st != S.OK
        ws = was.slots[slot]
        if kind == "load_table":
            on_at_upload = was.fold
            dense = KNOBS[op["knob"]].get("PFAC_DENSE") == "1"
        if kind == "set_fold":
            fold_statuses.add(st)
            on_at_upload = False
            if st == S.OK and op["mode"] != int(was.fold) and any(s.scan is not None and s.scan["pending"] for s in was.slots):
                toggle_while_pending = True
        if kind == "get_fold" and st == S.OK:
            fold_statuses.add("read")
            off_after_upload |= on_at_upload and not was.fold
        if kind in ("scan_bytes", "scan_ext", "scan_start") and st == S.OK:
            sc = m.slots[slot].scan
            width = x.width(sc["tab"], sc["knob"])
            where |= {(sc["fold"], "slot", slot), (sc["fold"], "shared", slot == 1 and ws.shared)}
            if sc["fold"]:
                tables.add(sc["tab"])
                widths.add(width)
                knobs = KNOBS[sc["knob"]]
                placed.add("through L2" if "PFAC_FORCE_L2" in knobs else "in LDS")
                if dense:
                    placed.add("dense staging")
                flipped |= last_mode is not None and last_mode != dense
            last_mode = dense
            if kind == "scan_start":
                pending_mode[slot] = True
            else:
                dense = _est_dense(dense, sc["knob"], width, x.input_size(sc["tab"], sc["inp"]), m._count(sc))
        if kind == "scan_finish" and st == S.OK and pending_mode.pop(slot, False):
            sc = m.slots[slot].scan
            dense = _est_dense(dense, sc["knob"], x.width(sc["tab"], sc["knob"]), x.input_size(sc["tab"], sc["inp"]), m._count(sc))
        sc = ws.scan
        if kind in BEHIND and st == S.OK and sc is not None and not sc["pending"] and sc["gen"] == was.gen:
            if sc["fold"]:
                behind.add((kind, "folded"))
            elif S.POOL[sc["tab"]].get("nocase"):
                behind.add((kind, "exact scan of a nocase table"))
        if kind == "records" and st == S.OK and op["n"] and sc["fold"] and sc["gen"] != was.gen:
            late_records = True
    missing = {"kinds": sorted(set(S.FOLD_KINDS) - kinds)}
    want = {(f, "slot", sl) for f in (False, True) for sl in (0, 1)} | {(f, "shared", True) for f in (False, True)}
    missing["modes on slots and the shared stream"] = sorted(want - where, key=str)
    missing["set_fold / get_fold statuses"] = sorted({S.OK, S.E_STATE, S.E_ARG, "read"} - fold_statuses, key=str)
    missing["tables folded"] = sorted(set(S.POOL) - tables)
    missing["widths folded"] = sorted({2, 4, 8} - widths)
    missing["placements folded"] = sorted({"in LDS", "through L2", "dense staging"} - placed)
    missing["behind"] = sorted({(b, w) for b in BEHIND for w in ("folded", "exact scan of a nocase table")} - behind)
    missing["histories"] = [name for name, seen in (("a toggle while a scan is pending", toggle_while_pending),
                                                   ("get_fold reads off after an upload that followed an on", off_after_upload),
                                                   ("a folded scan in another staging mode than the scan before it", flipped),
                                                   ("records of a folded scan fetched after a later upload", late_records)) if not seen]
    missing = {k2: v for k2, v in missing.items() if v}
    assert not missing, "the fold plans never reach:\n" + "\n".join(f"  {k2}: {v}" for k2, v in missing.items())
    assert 0.06 < errors / total < 0.25, f"{errors} of {total} operations are illegal"


def test_three_quarters_of_the_folded_scans_differ_from_the_exact_ones(fold_plans):
    """By the reference alone: the family does not hide behind inputs the fold changes nothing for."""
    x = S.expectations()
    folded = differ = 0
    for seed, k, op, st, was, m in _walk_models(fold_plans):
        if op["op"] in ("scan_bytes", "scan_ext", "scan_start") and st == S.OK and m.slots[op["slot"]].scan["fold"]:
            sc = m.slots[op["slot"]].scan
            a, b = x.scan(sc["tab"], sc["inp"], sc["no"]), x.scan(sc["tab"], sc["inp"], sc["no"], (), True)
            folded += 1
            differ += not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    print(f"{differ} of {folded} folded scans differ from the exact scan of the same input")
    assert folded >= 4 * len(fold_plans) and 4 * differ >= 3 * folded, (differ, folded)       # (four folded scans a plan at the least)
