"""GPU matcher: the host-side mirror of the reference's device seam.

``GpuMatcher`` owns one ``pfac_ctx`` (one GPU) and plays the role of
``GPU_Malloc_Memory`` / ``GPU_TraceTable`` / ``GPU_Free_memory``
(main.cc:35-37, master_kernel.cu:188-524) through the C-ABI of
``libpfac_hip.so``.  Nothing here computes matches on the host: every scan is a
launch of the HIP kernel, and a missing library or GPU raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from ._ffi import (PFAC_COUNT_ACCUMULATE, PFAC_DOCS_INVERT, PFAC_E_OVERFLOW, PFAC_FOLD_ASCII, PFAC_FOLD_NONE, PFAC_SPANS_LINE, PFAC_WORD_LEFT, PFAC_WORD_RIGHT, CRecord, PfacError,
                   hip_lib)
from ._ffi import (PFAC_LINE_CONTEXT_SEP, PFAC_LINE_MAX_GROUP_SEP, PFAC_LINE_NUMBER, PFAC_LINE_OFFSET, PFAC_LINE_SEP_FIRST,
                   PFAC_LINE_TERMINATE, CDocScore, CLineFormat, CScoreRule)
from ._ffi import PFAC_TOP_BY_COUNT, PFAC_TOP_LOWEST, PFAC_TOP_RANKED
from ._ffi import PFAC_TERMS_SELECTION
from ._ffi import PFAC_TOKENS_POSITIONS
from ._ffi import PFAC_NEAR_SELECTION
from ._ffi import PFAC_E_STATE
from .table import UNIGRAM_PIECE_DTYPE, UNIGRAM_SPACE
from .table import BPE_PIECE_DTYPE
from .table import NEAR_RULE_DTYPE, RECORD_DTYPE,SCORE_DTYPE, TEMPLATE_PLAIN, TOKEN_DROP, WORD_BYTES, PfacTable, redaction_table, replacement_table, template_table, token_table, _state_lengths


def device_count() -> int:
    n = C.c_int(0)
    rc = hip_lib().pfac_device_count(C.byref(n))
    if rc:
        raise PfacError(rc, (hip_lib().pfac_last_error(None) or b"").decode())
    return n.value


def word_set(chars: bytes) -> np.ndarray:
    """The 256-bit set of ``pfac_records_filter_words`` (uint64[4]: byte b at bit b & 63 of word b >> 6) that holds the
    bytes of ``chars``."""
    w = [0, 0, 0, 0]
    for b in bytes(chars):
        w[b >> 6] |= 1 << (b & 63)
    return np.array(w, dtype=np.uint64)


_EDGES = {"both": PFAC_WORD_LEFT | PFAC_WORD_RIGHT, "left": PFAC_WORD_LEFT, "right": PFAC_WORD_RIGHT}


def _word_bytes(whole_words):
    """The ``word_bytes`` of ``filter_whole_words`` for a ``whole_words`` keyword: True = the default set."""
    return None if whole_words is True else whole_words


def _delimiter_byte(delimiter) -> int:
    """The delimiter of the ``*_lines`` calls and ``split_documents``: one byte (``b"\\n"``) or its value."""
    if isinstance(delimiter, (bytes, bytearray)):
        if len(delimiter) != 1:
            raise ValueError("the delimiter is a single byte")
        return delimiter[0]
    return int(delimiter)


def _ptr(x) -> int:
    """Device pointer of a torch tensor / int / None."""
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return int(x.data_ptr())
    raise TypeError(f"cannot take a device pointer from {type(x)!r}")


def _near_rules(rules) -> np.ndarray:
    """The ``rules`` of the proximity calls as one contiguous ``NEAR_RULE_DTYPE`` array: an array of them as it is, or
    the ``near_rule`` records of a list."""
    if isinstance(rules, np.ndarray):
        return np.ascontiguousarray(rules, dtype=NEAR_RULE_DTYPE).ravel()
    given = list(rules)
    out = np.zeros(len(given), dtype=NEAR_RULE_DTYPE)
    for k, r in enumerate(given):
        out[k] = np.asarray(r, dtype=NEAR_RULE_DTYPE).reshape(())[()]
    return out


class GpuMatcher:
    """One GPU, ``n_streams`` pipeline slots (the reference's "streams per GPU", argv[2])."""

    def __init__(self, device: int = 0, n_streams: int = 1):
        self._L = hip_lib()
        self._ctx = C.c_void_p()
        self.device = device
        self.n_streams = n_streams
        self.table: Optional[PfacTable] = None
        self._keep = {}
        self._keep_mark = {}            # per slot: how many of its kept h2d sources were queued before its last scan_async
        self._last_n = {}
        self._flen_set = False          # final-state lengths on the device for the uploaded table (scan_documents)
        self._n_rules = 0               # rules of the uploaded table (set_rules; an upload drops them)
        self._cnt_n = {}                # per slot: entries of its slot-owned state counts (count_states)
        rc = self._L.pfac_ctx_create(int(device), int(n_streams), C.byref(self._ctx))
        if rc:
            self._ctx = C.c_void_p()
            raise PfacError(rc, (self._L.pfac_last_error(None) or b"").decode())

    # -- plumbing ---------------------------------------------------------
    def _check(self, rc: int, allow_overflow: bool = False) -> int:
        if rc and not (allow_overflow and rc == PFAC_E_OVERFLOW):
            raise PfacError(rc, (self._L.pfac_last_error(self._ctx) or b"").decode())
        return rc

    def _counted(self, rc: int, n, attr: str) -> int:
        """The count ``n`` a pass returned through its pointer; a failed pass raises PfacError with that count (exact
        after an overflow) as its attribute ``attr``."""
        if rc:
            e = PfacError(rc, (self._L.pfac_last_error(self._ctx) or b"").decode())
            setattr(e, attr, n.value)
            raise e
        return n.value

    def _to_host(self, slot: int, fetch, *shapes):
        """One fetch of a slot-owned result into new host arrays, one per ``(n, dtype)`` of ``shapes``: ``fetch`` gets
        their data pointers (None for an empty array), is checked, and the slot is synchronised.  Returns the array, or
        the tuple of them."""
        out = tuple(np.empty(int(n), dtype=dt) for n, dt in shapes)
        self._check(fetch(*(a.ctypes.data if a.size else None for a in out)))
        self.sync(slot)
        return out[0] if len(out) == 1 else out

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.pfac_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- table ------------------------------------------------------------
    def load_table(self, table) -> None:
        """Upload a ``PfacTable`` (or its int32 image) -- master_kernel.cu:365-383."""
        if isinstance(table, PfacTable):
            self.table = table
            blob = table.blob()
        else:
            blob = np.ascontiguousarray(table, dtype=np.int32)
            self.table = PfacTable.from_blob(blob)
        self._flen_set = False
        self._n_rules = 0
        self._check(self._L.pfac_table_upload(self._ctx, blob.ctypes.data, blob.size))
        if self.table.ignore_case:          # (an upload leaves the fold off)
            self.set_case_fold(True)

    def load_table_device(self, d_blob, n_words: int, stream: int = 0, host_table: Optional[PfacTable] = None) -> None:
        """Install a table image that already sits in this GPU's memory (e.g. after an RCCL broadcast)."""
        self._flen_set = False
        self._n_rules = 0
        self._check(self._L.pfac_table_upload_device(self._ctx, _ptr(d_blob), int(n_words), stream))
        if host_table is not None:
            self.table = host_table
            if host_table.ignore_case:
                self.set_case_fold(True)

    def set_case_fold(self, on: bool) -> None:
        """Case-insensitive scans (``pfac_table_set_case_fold``): every scan queued from now on, on every slot, matches
        as if A-Z of the input were a-z; scans already queued keep their mode.  The input buffer is never written, and
        the passes behind the scan (whole-word filter, replaces, split, gather) see the bytes as they are.  Meant for a
        table of folded patterns (``ignore_case=True``); the next table upload turns it off."""
        self._check(self._L.pfac_table_set_case_fold(self._ctx, PFAC_FOLD_ASCII if on else PFAC_FOLD_NONE))

    @property
    def case_fold(self) -> bool:
        mode = C.c_uint32()
        self._check(self._L.pfac_table_case_fold(self._ctx, C.byref(mode)))
        return mode.value == PFAC_FOLD_ASCII

    def info(self) -> dict:
        v, t, g, l = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._check(self._L.pfac_scan_info(self._ctx, C.byref(v), C.byref(t), C.byref(g), C.byref(l)))
        nb, cap = C.c_int(), C.c_uint32()
        self._check(self._L.pfac_scan_staging(self._ctx, C.byref(nb), C.byref(cap)))
        return {"variant": "tables_in_lds" if v.value == 0 else "tables_via_l2", "tile_bytes": t.value,
                "grid_blocks": g.value, "lds_bytes": l.value, "staging_buffers": nb.value, "staging_records": cap.value}

    # -- buffers ----------------------------------------------------------
    def reserve(self, slot: int = 0, input_bytes: int = 0, record_capacity: int = 0) -> None:
        self._check(self._L.pfac_slot_reserve(self._ctx, slot, int(input_bytes), int(record_capacity)))

    def input_ptr(self, slot: int = 0) -> int:
        return int(self._L.pfac_slot_input(self._ctx, slot) or 0)

    def records_ptr(self, slot: int = 0) -> int:
        return int(self._L.pfac_slot_records(self._ctx, slot) or 0)

    def stream_handle(self, slot: int = 0) -> int:
        return int(self._L.pfac_slot_stream(self._ctx, slot) or 0)

    def set_stream(self, slot: int, stream_handle: int) -> None:
        self._check(self._L.pfac_slot_set_stream(self._ctx, slot, stream_handle))

    def h2d(self, host: np.ndarray, slot: int = 0, dst_offset: int = 0) -> None:
        host = np.ascontiguousarray(host, dtype=np.uint8)
        self._keep.setdefault(slot, []).append(host)   # the copy is asynchronous: released by sync()/scan_finish()
        self._check(self._L.pfac_slot_h2d(self._ctx, slot, host.ctypes.data, host.size, int(dst_offset)))

    def h2d_done(self, slot: int = 0) -> bool:
        """Whether the slot's last ``h2d`` has left its host array (``pfac_slot_h2d_done``; never blocks)."""
        rc = self._L.pfac_slot_h2d_done(self._ctx, slot)
        if rc < 0:
            self._check(rc)
        return rc == 1

    def sync(self, slot: int = 0) -> None:
        self._check(self._L.pfac_slot_sync(self._ctx, slot))
        self._keep.pop(slot, None)
        self._keep_mark.pop(slot, None)

    # -- the scan ---------------------------------------------------------
    def scan_async(self, n_owned: int, n_avail: Optional[int] = None, d_input=None, d_records=None,
                   capacity: int = 0, slot: int = 0) -> None:
        """Launch the kernel (master_kernel.cu:406).  ``d_input`` / ``d_records`` None = the slot's buffers."""
        n_avail = n_owned if n_avail is None else n_avail
        self._check(self._L.pfac_scan_async(self._ctx, slot, _ptr(d_input), int(n_owned), int(n_avail),
                                            _ptr(d_records), int(capacity)))
        self._keep_mark[slot] = len(self._keep.get(slot, ()))

    def scan_finish(self, slot: int = 0, allow_overflow: bool = False) -> Tuple[int, bool]:
        n = C.c_uint64(0)
        rc = self._check(self._L.pfac_scan_finish(self._ctx, slot, C.byref(n)), allow_overflow=allow_overflow)
        # the scan's end event is ordered after the H2D copies queued BEFORE its scan_async: their host arrays can go
        # (a streaming caller that never calls sync() would otherwise keep every chunk it ever uploaded alive).  A copy
        # queued after scan_async -- the next chunk -- may not have started: its array stays until a later
        # scan_finish / sync.
        kept = self._keep.get(slot)
        if kept:
            del kept[:self._keep_mark.get(slot, 0)]
        self._keep_mark[slot] = 0
        self._last_n[slot] = n.value
        return n.value, rc == PFAC_E_OVERFLOW

    def last_count(self, slot: int = 0) -> int:
        """Match count of the slot's last finished scan."""
        return self._last_n[slot]

    def elapsed_ms(self, slot: int = 0) -> float:
        ms = C.c_float(0)
        self._check(self._L.pfac_scan_elapsed_ms(self._ctx, slot, C.byref(ms)))
        return ms.value

    def records_to_host(self, n: int, slot: int = 0, d_records=None, first: int = 0) -> np.ndarray:
        out = np.empty(int(n), dtype=RECORD_DTYPE)
        if n:
            self._check(self._L.pfac_records_d2h(self._ctx, slot, _ptr(d_records), out.ctypes.data, int(first), int(n)))
            self.sync(slot)
        return out

    def scan_format(self, slot: int = 0) -> Tuple[int, int, int]:
        """(record_bytes, n_tiles, used) of the slot's last scan: record_bytes = 2 or 4 (compact words in the record
        heap) or 8 (pfac_record), n_tiles = entries of the tile index, used = heap records in use (gaps included)."""
        rb, nt, used = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.pfac_scan_format(self._ctx, slot, C.byref(rb), C.byref(nt), C.byref(used)))
        return rb.value, nt.value, used.value

    def capacity_hint(self, slot: int = 0) -> int:
        """A record capacity the slot's last scan fits (after an overflow)."""
        c = C.c_uint64(0)
        self._check(self._L.pfac_scan_capacity_hint(self._ctx, slot, C.byref(c)))
        return c.value

    def expand_records(self, n: int, d_out, slot: int = 0, d_records=None, first: int = 0) -> None:
        """Records [first, first+n) of the slot's last scan as 8-byte ``pfac_record`` into the DEVICE buffer ``d_out``
        (asynchronous on the slot's stream) -- what the RCCL record gather sends."""
        self._check(self._L.pfac_records_expand(self._ctx, slot, _ptr(d_records), int(first), int(n), _ptr(d_out)))

    def packed_to_host(self, slot: int = 0, d_records=None) -> Tuple[np.ndarray, np.ndarray]:
        """The compact device form itself: (uint16 or uint32 heap words [used], uint64 tile index [n_tiles])."""
        rb, nt, used = self.scan_format(slot)
        words = np.empty(int(used), dtype=np.uint16 if rb == 2 else np.uint32)
        tix = np.empty(max(nt, 1), dtype=np.uint64)
        self._check(self._L.pfac_records_d2h_packed(self._ctx, slot, _ptr(d_records), words.ctypes.data, int(used), tix.ctypes.data))
        self.sync(slot)
        return words, tix[:nt]

    def packed_to_host_into(self, host_words, host_tile_index, slot: int = 0, d_records=None) -> Tuple[int, int, int]:
        """``packed_to_host`` into buffers the caller owns (e.g. pinned torch tensors: uint8[used * record_bytes],
        int64[n_tiles]); synchronous.  Returns (record_bytes, n_tiles, used)."""
        rb, nt, used = self.scan_format(slot)
        self._check(self._L.pfac_records_d2h_packed(self._ctx, slot, _ptr(d_records), _ptr(host_words), int(used),
                                                    _ptr(host_tile_index)))
        self.sync(slot)
        return rb, nt, used

    def packed_to_device(self, d_words_out, d_tile_index_out, slot: int = 0, d_records=None) -> Tuple[int, int, int]:
        """The compact form into DEVICE buffers the caller owns (torch tensors): heap words [0, used) -> ``d_words_out``
        (None: leave them where the scan wrote them) and the tile index -> ``d_tile_index_out`` (int64[n_tiles]).
        Asynchronous on the slot's stream.  Returns (record_bytes, n_tiles, used) -- what ``dist.gather_packed`` sends."""
        rb, nt, used = self.scan_format(slot)
        self._check(self._L.pfac_records_packed_device(self._ctx, slot, _ptr(d_records), _ptr(d_words_out), int(used),
                                                       _ptr(d_tile_index_out)))
        return rb, nt, used

    def emit_text_device(self, base: int = 0, slot: int = 0, d_records=None) -> int:
        """Format the slot's last finished scan into ``GPU_match_result.txt`` lines ON THE GPU (main.cc:335-350); returns
        the byte count.  ``text_to_host`` fetches them."""
        n = C.c_uint64(0)
        self._check(self._L.pfac_emit_text_device(self._ctx, slot, _ptr(d_records), int(base), C.byref(n)))
        return n.value

    def text_to_host(self, n_bytes: int, slot: int = 0, first: int = 0) -> bytes:
        out = np.empty(int(n_bytes), dtype=np.uint8)
        if n_bytes:
            self._check(self._L.pfac_text_d2h(self._ctx, slot, out.ctypes.data, int(first), int(n_bytes)))
            self.sync(slot)
        return out.tobytes()

    def checksum(self, n: int, base: int = 0, slot: int = 0, d_records=None) -> int:
        s = C.c_uint64(0)
        self._check(self._L.pfac_records_checksum(self._ctx, slot, _ptr(d_records), int(n), int(base), C.byref(s)))
        return s.value

    def scan_resident(self, n_owned: int, n_avail: Optional[int] = None, d_input=None, slot: int = 0) -> int:
        """Scan input already in HBM into the slot's record buffer, growing it on overflow.  Returns #matches."""
        n_avail = n_owned if n_avail is None else n_avail
        self.scan_async(n_owned, n_avail, d_input=d_input, slot=slot)
        n, over = self.scan_finish(slot, allow_overflow=True)
        cap = 0
        for _ in range(4):
            if not over:
                break
            cap = max(self.capacity_hint(slot), 2 * cap)
            self.reserve(slot, 0, cap)
            self.scan_async(n_owned, n_avail, d_input=d_input, slot=slot)
            n, over = self.scan_finish(slot, allow_overflow=True)
        if over:
            raise PfacError(PFAC_E_OVERFLOW, "record heap still too small after four attempts")
        return n

    def scan_bytes(self, data, n_owned: Optional[int] = None, slot: int = 0, whole_words=False, prev_byte: int = -1,
                   next_byte: int = -1) -> np.ndarray:
        """H2D + scan + D2H of one host buffer.  ``n_owned`` < len(data) leaves the rest as read-only halo.
        ``whole_words`` (True, or the word bytes) keeps the whole-word matches only (``filter_whole_words``);
        ``prev_byte`` / ``next_byte`` are then the bytes around ``data`` when it is one range of a longer text."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        n_avail = int(buf.size)
        n_owned = n_avail if n_owned is None else int(n_owned)
        if whole_words is not False:
            self._ensure_final_lengths()
        self.reserve(slot, max(n_avail, 1), max(n_avail // 8, 4096))
        if n_avail:
            self.h2d(buf, slot)
        n = self.scan_resident(n_owned, n_avail, slot=slot)
        if whole_words is not False:
            n = self.filter_whole_words(slot, _word_bytes(whole_words), prev_byte=prev_byte, next_byte=next_byte)
        return self.records_to_host(n, slot)

    # -- whole-word matches -------------------------------------------------
    def filter_whole_words(self, slot: int = 0, word_bytes=None, edges: str = "both", prev_byte: int = -1,
                           next_byte: int = -1, n_docs: int = 0, d_doc_offsets=None, d_input=None, d_records=None) -> int:
        """Drops, in place on the GPU, the records of the slot's last finished scan that split a word
        (``pfac_records_filter_words``): everything that reads the scan afterwards -- the fetches, the text, the
        checksum, the document cut, the selections, the replaces -- sees whole-word matches only.  ``word_bytes``: the
        bytes that make up words (None = ``[0-9A-Za-z_]``; or a ``word_set`` array); ``edges``: "both", or only the
        "left" / "right" end of a match; ``prev_byte`` / ``next_byte``: the byte in front of / behind the scanned
        buffer (-1: the text starts / ends there); ``n_docs`` > 0: document offsets are boundaries too
        (``d_doc_offsets`` None = the slot's).  Returns the number of records kept, which ``last_count`` reports
        from then on."""
        if edges not in _EDGES:
            raise ValueError(f"edges must be one of {sorted(_EDGES)}")
        if word_bytes is None:
            ws = None
        elif isinstance(word_bytes, np.ndarray) and word_bytes.dtype == np.uint64:
            ws = np.ascontiguousarray(word_bytes)
            if ws.size != 4:
                raise ValueError("a word set holds four 64-bit words")
        else:
            ws = word_set(word_bytes)
        n = C.c_uint64(0)
        self._check(self._L.pfac_records_filter_words(self._ctx, slot, _ptr(d_input), _ptr(d_records),
                                                      ws.ctypes.data if ws is not None else None, _EDGES[edges],
                                                      int(prev_byte), int(next_byte), _ptr(d_doc_offsets), int(n_docs),
                                                      C.byref(n)))
        self._last_n[slot] = n.value
        return n.value

    # -- anchored matches: where in a line a pattern may match ----------------
    def set_pattern_spans(self, rules) -> None:
        """The span of every pattern of the uploaded table (``PfacTable.state_spans``: one entry per 1-based pattern id
        -- None, ``"^"``, ``"$"``, ``"^$"`` or ``(min_start, max_start, max_tail)``; ``strip_anchors`` makes them from
        grep's pattern lines), kept on the device until the next table upload (``pfac_table_set_state_spans``)."""
        if self.table is None:
            raise PfacError(-7, "no host table to map pattern ids to states (load_table first)")
        spans = self.table.state_spans(rules)
        self._check(self._L.pfac_table_set_state_spans(self._ctx, spans.ctypes.data if spans.size else None, spans.size))

    def filter_spans(self, slot: int = 0, delimiter=None, line_match: bool = False, n_docs: int = 0, d_doc_offsets=None,
                     d_input=None, d_records=None) -> int:
        """Drops, in place on the GPU, the records of the slot's last finished scan that their pattern's span does not
        admit (``pfac_records_filter_spans``): a match must start ``min_start .. max_start`` bytes into its document and
        end at most ``max_tail`` bytes in front of the document's end -- in front of its ``delimiter`` (a byte or its
        value; None = none) where the document ends in one.  ``line_match``: every pattern must cover its whole line
        (``grep -x``), whatever spans are set.  ``n_docs`` 0: the scanned buffer is the one document; else
        ``d_doc_offsets`` (None = the slot's) cut it.  Everything that reads the scan afterwards sees the kept records
        only.  Returns their number, which ``last_count`` reports from then on."""
        n = C.c_uint64(0)
        self._check(self._L.pfac_records_filter_spans(self._ctx, slot, _ptr(d_input), _ptr(d_records),
                                                      -1 if delimiter is None else _delimiter_byte(delimiter),
                                                      PFAC_SPANS_LINE if line_match else 0, _ptr(d_doc_offsets), int(n_docs),
                                                      C.byref(n)))
        self._last_n[slot] = n.value
        return n.value

    # -- counts per pattern --------------------------------------------------
    def _n_states(self) -> int:
        if self.table is None:
            raise PfacError(-7, "no host table to take num_final from (load_table first)")
        return int(self.table.num_final)

    def count_states(self, slot: int = 0, d_records=None, d_counts=None, accumulate: bool = False) -> int:
        """Histogram of the final states of the slot's last finished scan, on the GPU (``pfac_records_count_states``):
        ``counts[s]`` = records whose state is s, after ``filter_whole_words`` the kept ones.  ``d_counts`` None = a
        slot-owned buffer (``state_counts_to_host``), else a device buffer of ``num_final`` uint64.  ``accumulate`` adds
        onto the counts already there -- how chained ranges and chunked streams sum up on the device.  Returns the
        number of records counted (= ``last_count``).  ``PfacTable.counts_by_pattern`` maps states to pattern ids."""
        n = C.c_uint64(0)
        ns = self._n_states()
        self._check(self._L.pfac_records_count_states(self._ctx, slot, _ptr(d_records), _ptr(d_counts), ns,
                                                      PFAC_COUNT_ACCUMULATE if accumulate else 0, C.byref(n)))
        if d_counts is None:
            self._cnt_n[slot] = ns
        return n.value

    def count_selection_states(self, slot: int = 0, d_sel=None, d_counts=None, accumulate: bool = False) -> int:
        """``count_states`` over the slot's last leftmost-longest selection (``select_leftmost_longest`` or
        ``select_leftmost_longest_documents``): how many of each pattern a replace rewrites.  ``d_sel`` None = the
        slot-owned selection, else the ``d_out`` the selection was given.  Returns the number of picks."""
        n = C.c_uint64(0)
        ns = self._n_states()
        self._check(self._L.pfac_selection_count_states(self._ctx, slot, _ptr(d_sel), _ptr(d_counts), ns,
                                                        PFAC_COUNT_ACCUMULATE if accumulate else 0, C.byref(n)))
        if d_counts is None:
            self._cnt_n[slot] = ns
        return n.value

    def state_counts_to_host(self, slot: int = 0) -> np.ndarray:
        """The slot-owned counts of ``count_states`` / ``count_selection_states``: uint64[num_final] of the table they
        were counted with."""
        return self._to_host(slot, lambda p: self._L.pfac_state_counts_d2h(self._ctx, slot, p),
                             (self._cnt_n.get(slot, 0), np.uint64))     # (no counts yet: the call says PFAC_E_STATE)

    def count_patterns(self, data, n_owned: Optional[int] = None, slot: int = 0, whole_words=False, prev_byte: int = -1,
                       next_byte: int = -1, accumulate: bool = False) -> np.ndarray:
        """H2D + scan + count of one host buffer: how often every pattern matches, as uint64 counts indexed by the
        1-based pattern id (``PfacTable.counts_by_pattern``); only the counts cross the link.  ``n_owned``,
        ``whole_words``, ``prev_byte`` / ``next_byte`` as in ``scan_bytes``.  ``accumulate``: add onto the slot's counts
        of the calls before -- over consecutive owned ranges (each with the halo behind it) the last call returns the
        counts of the whole text."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        n_avail = int(buf.size)
        n_owned = n_avail if n_owned is None else int(n_owned)
        if whole_words is not False:
            self._ensure_final_lengths()
        self.reserve(slot, max(n_avail, 1), max(n_avail // 8, 4096))
        if n_avail:
            self.h2d(buf, slot)
        self.scan_resident(n_owned, n_avail, slot=slot)
        if whole_words is not False:
            self.filter_whole_words(slot, _word_bytes(whole_words), prev_byte=prev_byte, next_byte=next_byte)
        self.count_states(slot, accumulate=accumulate)
        return self.table.counts_by_pattern(self.state_counts_to_host(slot))

    def scan_partitioned(self, tables, data, slot: int = 0) -> np.ndarray:
        """Pattern-partition mode on ONE GPU: the input is copied once, every partition's table (``tables[k]`` =
        ``PfacTable.from_file_part(..., k, len(tables))``) scans it in turn, and the per-partition record lists are
        merged as main.cc:304-324 does.  Returns records ordered by (position, pattern length) whose ``state``
        field holds the PATTERN ID (emit with ``idmap=None``)."""
        from .table import merge_partitions
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        n = int(buf.size)
        self.reserve(slot, max(n, 1), max(n // 8, 4096))
        if n:
            self.h2d(buf, slot)
        lists = []
        for t in tables:
            self.load_table(t)
            cnt = self.scan_resident(n, n, slot=slot)
            lists.append(self.records_to_host(cnt, slot))
        return merge_partitions(lists, [t.idmap for t in tables])

    # -- batches of documents ---------------------------------------------
    def set_final_lengths(self, lengths) -> None:
        """Pattern length of every final state of the uploaded table (``PfacTable.final_lengths()``); kept on the
        device until the next table upload."""
        lens = np.ascontiguousarray(lengths, dtype=np.int32)
        self._check(self._L.pfac_table_set_final_lengths(self._ctx, lens.ctypes.data, lens.size))
        self._flen_set = True

    def set_doc_offsets(self, offsets, slot: int = 0) -> None:
        """Document boundaries of the slot (n_docs + 1 offsets: 0, ends of documents ..., n_owned)."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        if off.size < 1:
            raise ValueError("need n_docs + 1 >= 1 offsets")
        self._check(self._L.pfac_slot_doc_offsets(self._ctx, slot, off.ctypes.data, off.size - 1))

    def segment_records(self, n_docs: int, d_doc_offsets=None, d_out=None, out_cap: int = 0, d_doc_first=None,
                        slot: int = 0, d_records=None) -> int:
        """Cut the slot's last finished scan into documents [off[d], off[d+1]) on the GPU: drop the records that run
        past their document's end, rebase the others to it, index them per document.  ``d_doc_offsets`` None = the
        slot's (``set_doc_offsets``); ``d_out`` / ``d_doc_first`` None = slot-owned buffers (``segment_to_host``).
        Returns the number of records kept.  A too small ``out_cap`` raises PfacError(PFAC_E_OVERFLOW) whose
        ``n_kept`` attribute holds the exact count."""
        n = C.c_uint64(0)
        rc = self._L.pfac_records_segment(self._ctx, slot, _ptr(d_records), _ptr(d_doc_offsets), int(n_docs), _ptr(d_out),
                                          int(out_cap), _ptr(d_doc_first), C.byref(n))
        return self._counted(rc, n, "n_kept")

    def segment_to_host(self, n_kept: int, n_docs: int, slot: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """(doc_first uint64[n_docs + 1], records) of the slot's last ``segment_records`` into slot-owned buffers."""
        rec, first = self._to_host(slot, lambda r, f: self._L.pfac_segment_d2h(self._ctx, slot, r, f),
                                   (n_kept, RECORD_DTYPE), (int(n_docs) + 1, np.uint64))
        return first, rec

    def _ensure_final_lengths(self) -> None:
        if self._flen_set:
            return
        if self.table is None:
            raise PfacError(-7, "no host table to take the final-state lengths from (load_table first)")
        lens = getattr(self.table, "_final_lengths", None)
        if lens is None:
            lens = self.table.final_lengths()
            self.table._final_lengths = lens          # once per table
        self.set_final_lengths(lens)

    def _scan_docs(self, docs, slot: int, whole_words=False, spans: bool = False, line_match: bool = False) -> Tuple[np.ndarray, int]:
        """Upload and scan a batch of documents (``docs`` as ``scan_documents`` takes it) and set its offsets on the
        slot; with ``whole_words`` the whole-word filter follows, document ends being boundaries; with ``spans`` (the
        rules of ``set_pattern_spans``) or ``line_match`` (every pattern covers its whole document) the span filter
        follows that, without a delimiter.  Returns (offsets uint64[n_docs + 1], n_docs)."""
        buf, offsets = _docs_buffer(docs)
        n = int(buf.size)
        self._ensure_final_lengths()
        self.reserve(slot, max(n, 1), max(n // 8, 4096))
        if n:
            self.h2d(buf, slot)
        self.scan_resident(n, n, slot=slot)
        self.set_doc_offsets(offsets, slot)
        if whole_words is not False and offsets.size > 1:
            self.filter_whole_words(slot, _word_bytes(whole_words), n_docs=int(offsets.size) - 1)
        if (spans or line_match) and offsets.size > 1:
            self.filter_spans(slot, None, line_match, n_docs=int(offsets.size) - 1)
        return offsets, int(offsets.size) - 1

    def scan_documents(self, docs, slot: int = 0, whole_words=False, spans: bool = False, line_match: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Match a batch of independent documents in one scan.  ``docs`` is a sequence of bytes-like objects, or a
        ``(buffer, offsets)`` pair whose offsets (an integer array or list, n_docs + 1 of them, from 0 to len(buffer))
        cut ``buffer`` into documents.  Returns (doc_first uint64[n_docs + 1], records): the records of document d are
        ``records[doc_first[d]:doc_first[d + 1]]``, positions relative to the document, in (offset, pattern length)
        order -- what scanning each document on its own yields (and, with ``whole_words``, filtering it on its own).
        ``spans``: only the matches that the patterns' spans (``set_pattern_spans``) admit in their document;
        ``line_match``: only those that cover their whole document (``filter_spans``, behind the whole-word filter)."""
        _, n_docs = self._scan_docs(docs, slot, whole_words, spans, line_match)
        kept = self.segment_records(n_docs, slot=slot)
        return self.segment_to_host(kept, n_docs, slot)

    # -- lines: documents cut at a delimiter, on the device ------------------
    def split_documents(self, n_bytes: int, delimiter=b"\n", d_input=None, slot: int = 0) -> Tuple[int, int]:
        """Document offsets from a delimiter byte, made on the GPU from bytes that are already there
        (``pfac_slot_doc_offsets_split``): a document ends after every delimiter, an unterminated rest is the last
        document.  ``d_input`` None = the slot's input buffer.  The offsets become the slot's, as after
        ``set_doc_offsets``.  Returns (n_docs, tail_start): ``tail_start`` is where the unterminated last document
        starts (``n_bytes`` if there is none) -- what a chunked reader carries over."""
        n, tail = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.pfac_slot_doc_offsets_split(self._ctx, slot, _ptr(d_input), int(n_bytes),
                                                        _delimiter_byte(delimiter), C.byref(n), C.byref(tail)))
        return n.value, tail.value

    def doc_offsets_to_host(self, n_docs: int, slot: int = 0, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Offsets [first, first + n) of the slot's document offsets (default: all ``n_docs + 1``), whichever call set
        them."""
        n = int(n_docs) + 1 - int(first) if n is None else int(n)
        return self._to_host(slot, lambda p: self._L.pfac_slot_doc_offsets_d2h(self._ctx, slot, p, int(first), n),
                             (max(n, 0), np.uint64))

    def matching_documents(self, n_docs: int, invert: bool = False, d_doc_first=None, d_out=None, out_cap: int = 0,
                           slot: int = 0, before: int = 0, after: int = 0) -> int:
        """The documents that hold a match (``invert``: that hold none), ascending, on the GPU
        (``pfac_documents_matching``).  ``d_doc_first`` None = the slot-owned doc_first of the slot's last
        ``segment_records``, else a device array of ``n_docs + 1`` entries (of the segment pass or of
        ``select_leftmost_longest_documents``); ``d_out`` None = a slot-owned buffer (``matching_documents_to_host``).
        ``before`` / ``after`` (grep's ``-B`` / ``-A``; any value up to 2^64 - 1 clamps) add the documents around a
        matching one (``pfac_documents_matching_context``), each id once; they do not combine with ``invert``
        (ValueError).  Returns the number of documents.  A too small ``out_cap`` raises PfacError(PFAC_E_OVERFLOW)
        whose ``n_matching`` attribute holds the exact count."""
        n = C.c_uint64(0)
        if before or after:
            if invert:
                raise ValueError("context lines (before / after) do not combine with invert")
            if before < 0 or after < 0:
                raise ValueError("before and after must not be negative")
            rc = self._L.pfac_documents_matching_context(self._ctx, slot, _ptr(d_doc_first), int(n_docs), int(before),
                                                         int(after), 0, _ptr(d_out), int(out_cap), C.byref(n))
        else:
            rc = self._L.pfac_documents_matching(self._ctx, slot, _ptr(d_doc_first), int(n_docs),
                                                 PFAC_DOCS_INVERT if invert else 0, _ptr(d_out), int(out_cap), C.byref(n))
        return self._counted(rc, n, "n_matching")

    def matching_documents_to_host(self, n: int, slot: int = 0) -> np.ndarray:
        """The ids (uint64[n]) of the slot's last ``matching_documents`` into its slot-owned buffer."""
        return self._to_host(slot, lambda p: self._L.pfac_documents_matching_d2h(self._ctx, slot, p), (n, np.uint64))

    def gather_documents(self, n_docs: int, n_ids: int, n_bytes: int, d_input=None, d_doc_offsets=None, d_ids=None,
                         d_out=None, out_cap: int = 0, d_out_offsets=None, slot: int = 0) -> int:
        """The bytes of documents ``ids[0 .. n_ids)`` of ``d_input[0 .. n_bytes)``, back to back, on the GPU
        (``pfac_documents_gather``), with the output offset of each.  ``d_input`` None = the slot's input buffer,
        ``d_doc_offsets`` None = the slot's offsets (``set_doc_offsets`` / ``split_documents``), ``d_ids`` None = the
        slot-owned ids of the slot's last ``matching_documents`` (else any ids, in any order, repeats allowed);
        ``d_out`` / ``d_out_offsets`` None = slot-owned buffers (``gathered_to_host`` /
        ``gathered_offsets_to_host``).  Returns the output's length.  A too small ``out_cap`` raises
        PfacError(PFAC_E_OVERFLOW) whose ``out_bytes`` attribute holds the exact length."""
        n = C.c_uint64(0)
        rc = self._L.pfac_documents_gather(self._ctx, slot, _ptr(d_input), int(n_bytes), _ptr(d_doc_offsets), int(n_docs),
                                           _ptr(d_ids), int(n_ids), _ptr(d_out), int(out_cap), _ptr(d_out_offsets), C.byref(n))
        return self._counted(rc, n, "out_bytes")

    def gathered_to_host(self, n: int, slot: int = 0, first: int = 0) -> np.ndarray:
        """Bytes [first, first + n) of the slot's last ``gather_documents`` into its slot-owned buffer."""
        return self._to_host(slot, lambda p: self._L.pfac_documents_gather_d2h(self._ctx, slot, p, int(first), int(n)),
                             (n, np.uint8))

    def gathered_offsets_to_host(self, n_ids: int, slot: int = 0) -> np.ndarray:
        """The output offsets (uint64[n_ids + 1]) of the slot's last ``gather_documents`` into its slot-owned buffer."""
        return self._to_host(slot, lambda p: self._L.pfac_documents_gather_offsets_d2h(self._ctx, slot, p),
                             (int(n_ids) + 1, np.uint64))

    def gather_documents_formatted(self, n_docs: int, n_ids: int, n_bytes: int, number: bool = False, byte_offset: bool = False,
                                   terminate=None, context_sep: bool = False, group_sep: bytes = b"", sep_first: bool = False,
                                   number_base: int = 1, offset_base: int = 0, sep_match=b":", sep_context=b"-",
                                   d_input=None, d_doc_offsets=None, d_ids=None, d_doc_first=None, d_out=None, out_cap: int = 0,
                                   d_out_offsets=None, slot: int = 0) -> int:
        """``gather_documents`` with grep's labels, made on the GPU (``pfac_documents_gather_format``): in front of
        every document ``group_sep`` where its id does not follow the id before it (``sep_first``: also in front of the
        first), with ``number`` the decimal of ``id + number_base`` and a label separator, with ``byte_offset`` the
        decimal of its offset ``+ offset_base`` and a label separator; behind it, with ``terminate`` (one byte or its
        value), that byte where the document is empty or does not end in it.  The label separator is ``sep_match``,
        and with ``context_sep`` it is ``sep_context`` for a document without a kept record (``d_doc_first`` None =
        the slot's last ``segment_records``).  The buffer keywords, the result and the fetches are those of
        ``gather_documents``; the two share one slot-owned result."""
        group_sep = bytes(group_sep)
        if len(group_sep) > PFAC_LINE_MAX_GROUP_SEP:
            raise ValueError(f"group_sep holds at most {PFAC_LINE_MAX_GROUP_SEP} bytes")
        fmt = CLineFormat()
        fmt.flags = ((PFAC_LINE_NUMBER if number else 0) | (PFAC_LINE_OFFSET if byte_offset else 0) |
                     (PFAC_LINE_TERMINATE if terminate is not None else 0) | (PFAC_LINE_CONTEXT_SEP if context_sep else 0) |
                     (PFAC_LINE_SEP_FIRST if sep_first else 0))
        fmt.sep_match, fmt.sep_context = _delimiter_byte(sep_match), _delimiter_byte(sep_context)
        fmt.terminator = _delimiter_byte(terminate) if terminate is not None else 0
        fmt.group_sep_len = len(group_sep)
        for i, b in enumerate(group_sep):
            fmt.group_sep[i] = b
        fmt.number_base, fmt.offset_base = int(number_base), int(offset_base)
        n = C.c_uint64(0)
        rc = self._L.pfac_documents_gather_format(self._ctx, slot, _ptr(d_input), int(n_bytes), _ptr(d_doc_offsets), int(n_docs),
                                                  _ptr(d_ids), int(n_ids), _ptr(d_doc_first), C.byref(fmt), _ptr(d_out),
                                                  int(out_cap), _ptr(d_out_offsets), C.byref(n))
        return self._counted(rc, n, "out_bytes")

    def _scan_lines(self, data, delimiter, slot: int, whole_words=False, fetch_offsets: bool = True, spans: bool = False,
                    line_match: bool = False) -> Tuple[Optional[np.ndarray], int]:
        """``_scan_docs`` for one buffer whose documents end at ``delimiter``: upload, scan, offsets made on the device
        (only they come back, for the caller -- not even they with ``fetch_offsets`` False), then the whole-word filter
        and the span filter (with the lines' ``delimiter``: ``$`` sits in front of it) if asked for.  Returns (offsets
        uint64[n_docs + 1] or None, n_docs)."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        n = int(buf.size)
        self._ensure_final_lengths()
        self.reserve(slot, max(n, 1), max(n // 8, 4096))
        if n:
            self.h2d(buf, slot)
        self.scan_resident(n, n, slot=slot)
        n_docs, _ = self.split_documents(n, delimiter, slot=slot)
        if whole_words is not False and n_docs:
            self.filter_whole_words(slot, _word_bytes(whole_words), n_docs=n_docs)
        if (spans or line_match) and n_docs:
            self.filter_spans(slot, delimiter, line_match, n_docs=n_docs)
        return (self.doc_offsets_to_host(n_docs, slot) if fetch_offsets else None), n_docs

    def scan_lines(self, data, delimiter=b"\n", slot: int = 0, whole_words=False, spans: bool = False, line_match: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``scan_documents`` of one buffer cut into lines at ``delimiter`` on the device (a line keeps its
        delimiter).  Returns (doc_first, records, offsets uint64[n_docs + 1])."""
        offsets, n_docs = self._scan_lines(data, delimiter, slot, whole_words, spans=spans, line_match=line_match)
        kept = self.segment_records(n_docs, slot=slot)
        first, rec = self.segment_to_host(kept, n_docs, slot)
        return first, rec, offsets

    def select_lines(self, data, delimiter=b"\n", slot: int = 0, whole_words=False, spans: bool = False, line_match: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``select_documents`` of one buffer cut into lines at ``delimiter`` on the device.  Returns (doc_first,
        records with positions relative to the line, offsets)."""
        offsets, n_docs = self._scan_lines(data, delimiter, slot, whole_words, spans=spans, line_match=line_match)
        n = self.select_leftmost_longest_documents(n_docs, slot=slot)
        first, rec = self.doc_selection_to_host(n, n_docs, slot)
        if n:
            doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(first.astype(np.int64)))
            rec["pos"] -= offsets[doc].astype(np.uint32)
        return first, rec, offsets

    def replace_lines(self, data, delimiter=b"\n", slot: int = 0, whole_words=False, spans: bool = False, line_match: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``replace_documents`` of one buffer cut into lines at ``delimiter`` on the device.  Returns (out_offsets,
        out, offsets)."""
        offsets, n_docs = self._scan_lines(data, delimiter, slot, whole_words, spans=spans, line_match=line_match)
        self.select_leftmost_longest_documents(n_docs, slot=slot)
        n = self.replace_selection_documents(slot=slot)
        out_off = self.replacement_doc_offsets_to_host(n_docs, slot)
        return out_off, self.replacement_to_host(n, slot), offsets

    def matching_lines(self, data, delimiter=b"\n", invert: bool = False, slot: int = 0, whole_words=False, spans: bool = False,
                       line_match: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Which lines of ``data`` hold a match (``invert``: hold none) -- ``grep -F -f patterns``, ``-v``: scan, split,
        document cut and compaction on the device; only the ids and the offsets come back.  Returns (ids uint64,
        offsets uint64[n_docs + 1]): line k is ``data[offsets[ids[k]]:offsets[ids[k] + 1]]``."""
        offsets, n_docs = self._scan_lines(data, delimiter, slot, whole_words, spans=spans, line_match=line_match)
        self.segment_records(n_docs, slot=slot)
        n = self.matching_documents(n_docs, invert=invert, slot=slot)
        return self.matching_documents_to_host(n, slot), offsets

    def grep_lines(self, data, delimiter=b"\n", invert: bool = False, before: int = 0, after: int = 0, slot: int = 0,
                   whole_words=False, spans: bool = False, line_match: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The lines of ``data`` that hold a match, as bytes -- what ``grep -F -f patterns`` prints (``invert``: ``-v``;
        ``before`` / ``after``: ``-B`` / ``-A``, without the ``--`` separators): scan, split, document cut, compaction
        and gather on the device, from the slot's own input, offsets and ids.  Only the selected lines' bytes, their
        offsets and their ids come back.  Returns (out uint8[out_bytes], out_offsets uint64[n + 1], ids uint64[n]):
        selected line k is ``out[out_offsets[k]:out_offsets[k + 1]]``, line ``ids[k]`` of the input.  ``spans``: the
        patterns match only where their spans admit them (``set_pattern_spans``: ``^pat``, ``pat$``, offset / depth;
        ``$`` sits in front of the line's delimiter); ``line_match``: ``grep -x``, a pattern must be the whole line."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        if invert and (before or after):
            raise ValueError("context lines (before / after) do not combine with invert")
        _, n_docs = self._scan_lines(buf, delimiter, slot, whole_words, fetch_offsets=False, spans=spans, line_match=line_match)
        self.segment_records(n_docs, slot=slot)
        n = self.matching_documents(n_docs, invert=invert, slot=slot, before=before, after=after)
        out_bytes = self.gather_documents(n_docs, n, int(buf.size), slot=slot)
        return (self.gathered_to_host(out_bytes, slot), self.gathered_offsets_to_host(n, slot),
                self.matching_documents_to_host(n, slot))

    def grep_text(self, data, delimiter=b"\n", number: bool = False, byte_offset: bool = False, invert: bool = False,
                  before: int = 0, after: int = 0, whole_words=False, spans: bool = False, line_match: bool = False,
                  number_base: int = 1, offset_base: int = 0, sep_first: bool = False, slot: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``grep_lines`` with grep's output formatting made on the device: byte for byte what ``grep -F -f patterns``
        prints with ``-n`` (``number``), ``-b`` (``byte_offset``), ``-v``, ``-B`` / ``-A`` (a ``-`` behind the label
        of a context line, ``--`` and the delimiter between groups of lines that are not adjacent) and a delimiter
        behind an unterminated last line.  A chunked reader passes the lines and bytes in front of ``data`` as
        ``number_base`` - 1 and ``offset_base``, and ``sep_first`` where the chunk before printed a line that the first
        one here does not follow.  Returns (text uint8[], out_offsets uint64[n + 1], ids uint64[n]): printed line k,
        its ``--`` line included, is ``text[out_offsets[k]:out_offsets[k + 1]]``."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        if invert and (before or after):
            raise ValueError("context lines (before / after) do not combine with invert")
        context = bool(before or after)
        delim = _delimiter_byte(delimiter)
        _, n_docs = self._scan_lines(buf, delimiter, slot, whole_words, fetch_offsets=False, spans=spans, line_match=line_match)
        self.segment_records(n_docs, slot=slot)
        n = self.matching_documents(n_docs, invert=invert, slot=slot, before=before, after=after)
        out_bytes = self.gather_documents_formatted(n_docs, n, int(buf.size), number=number, byte_offset=byte_offset,
                                                    terminate=delim, context_sep=context,
                                                    group_sep=b"--" + bytes([delim]) if context else b"", sep_first=sep_first,
                                                    number_base=number_base, offset_base=offset_base, slot=slot)
        return (self.gathered_to_host(out_bytes, slot), self.gathered_offsets_to_host(n, slot),
                self.matching_documents_to_host(n, slot))

    # -- pattern groups: a group bitmask per document ------------------------
    def set_pattern_groups(self, groups) -> None:
        """The groups of every pattern of the uploaded table (``PfacTable.state_group_masks``: one entry per 1-based
        pattern id -- a group index 0..63, an iterable of them, None, or a uint64 array of ready masks), kept on the
        device until the next table upload (``pfac_table_set_state_groups``)."""
        if self.table is None:
            raise PfacError(-7, "no host table to map pattern ids to states (load_table first)")
        masks = self.table.state_group_masks(groups)
        self._check(self._L.pfac_table_set_state_groups(self._ctx, masks.ctypes.data if masks.size else None, masks.size))

    def document_group_masks(self, n_docs: int, d_doc_offsets=None, d_out=None, slot: int = 0, d_records=None) -> int:
        """Which pattern groups occur in each document of the slot's last finished scan, on the GPU
        (``pfac_documents_group_masks``): ``mask[d]`` ORs the groups of the records the document cut would keep, straight
        from the record heap -- no segment pass.  ``d_doc_offsets`` None = the slot's (``set_doc_offsets`` /
        ``split_documents``); ``d_out`` None = a slot-owned buffer (``group_masks_to_host``), else a device buffer of
        ``n_docs`` uint64.  Returns the OR of all masks: the groups that occurred at all."""
        m = C.c_uint64(0)
        self._check(self._L.pfac_documents_group_masks(self._ctx, slot, _ptr(d_records), _ptr(d_doc_offsets), int(n_docs),
                                                       _ptr(d_out), C.byref(m)))
        return m.value

    def group_masks_to_host(self, n_docs: int, slot: int = 0, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Masks [first, first + n) of the slot's last ``document_group_masks`` into its slot-owned buffer (default:
        all ``n_docs``)."""
        n = int(n_docs) - int(first) if n is None else int(n)
        return self._to_host(slot, lambda p: self._L.pfac_group_masks_d2h(self._ctx, slot, p, int(first), n),
                             (max(n, 0), np.uint64))

    def matching_documents_where(self, n_docs: int, all_of: int = 0, any_of: int = 0, none_of: int = 0, invert: bool = False,
                                 d_masks=None, d_out=None, out_cap: int = 0, slot: int = 0) -> int:
        """The documents whose group mask holds every group of ``all_of``, some group of ``any_of`` (0: no such demand)
        and none of ``none_of`` (``invert``: the others), ascending, on the GPU (``pfac_documents_matching_groups``).
        ``d_masks`` None = the slot-owned masks of the slot's last ``document_group_masks``, else a device array of
        ``n_docs`` uint64.  The ids go where ``matching_documents`` puts them (``d_out`` None = the slot-owned buffer,
        ``matching_documents_to_host``; ``gather_documents`` consumes them).  Returns the number of documents; a too
        small ``out_cap`` raises PfacError(PFAC_E_OVERFLOW) whose ``n_matching`` attribute holds the exact count."""
        n = C.c_uint64(0)
        full = 2**64 - 1
        rc = self._L.pfac_documents_matching_groups(self._ctx, slot, _ptr(d_masks), int(n_docs), int(all_of) & full,
                                                    int(any_of) & full, int(none_of) & full,
                                                    PFAC_DOCS_INVERT if invert else 0, _ptr(d_out), int(out_cap), C.byref(n))
        return self._counted(rc, n, "n_matching")

    def tag_documents(self, docs, whole_words=False, slot: int = 0, spans: bool = False, line_match: bool = False) -> np.ndarray:
        """The group mask of every document of a batch (``docs`` as ``scan_documents`` takes it) in one scan: uint64
        [n_docs], bit g set iff a pattern of group g (``set_pattern_groups``) matches inside the document.  Only the
        masks come back."""
        _, n_docs = self._scan_docs(docs, slot, whole_words, spans, line_match)
        self.document_group_masks(n_docs, slot=slot)
        return self.group_masks_to_host(n_docs, slot)

    def tag_lines(self, data, delimiter=b"\n", whole_words=False, slot: int = 0, spans: bool = False, line_match: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """``tag_documents`` of one buffer cut into lines at ``delimiter`` on the device.  Returns (offsets uint64
        [n_docs + 1], masks uint64[n_docs])."""
        offsets, n_docs = self._scan_lines(data, delimiter, slot, whole_words, spans=spans, line_match=line_match)
        self.document_group_masks(n_docs, slot=slot)
        return offsets, self.group_masks_to_host(n_docs, slot)

    def grep_lines_where(self, data, all_of: int = 0, any_of: int = 0, none_of: int = 0, invert: bool = False,
                         delimiter=b"\n", whole_words=False, slot: int = 0, spans: bool = False,
                         line_match: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The lines of ``data`` whose pattern groups satisfy the predicate of ``matching_documents_where``, as bytes --
        several ``grep -e`` groups joined by AND and NOT: scan, split, the mask pass, the predicate and the gather on
        the device, with no document cut in between.  Returns what ``grep_lines`` returns: (out uint8[out_bytes],
        out_offsets uint64[n + 1], ids uint64[n])."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        _, n_docs = self._scan_lines(buf, delimiter, slot, whole_words, fetch_offsets=False, spans=spans, line_match=line_match)
        self.document_group_masks(n_docs, slot=slot)
        n = self.matching_documents_where(n_docs, all_of, any_of, none_of, invert=invert, slot=slot)
        out_bytes = self.gather_documents(n_docs, n, int(buf.size), slot=slot)
        return (self.gathered_to_host(out_bytes, slot), self.gathered_offsets_to_host(n, slot),
                self.matching_documents_to_host(n, slot))

    # -- document scores: a weighted match sum and a count per document -----
    def set_pattern_weights(self, weights) -> None:
        """The weight of every pattern of the uploaded table (``PfacTable.state_weights``: one integer per 1-based
        pattern id, entry 0 unused), kept on the device until the next table upload
        (``pfac_table_set_state_weights``)."""
        if self.table is None:
            raise PfacError(-7, "no host table to map pattern ids to states (load_table first)")
        w = self.table.state_weights(weights)
        self._check(self._L.pfac_table_set_state_weights(self._ctx, w.ctypes.data if w.size else None, w.size))

    def document_scores(self, n_docs: int, d_doc_offsets=None, d_out=None, slot: int = 0, d_records=None) -> Tuple[int, int]:
        """How much of the pattern set each document of the slot's last finished scan holds, on the GPU
        (``pfac_documents_scores``): ``count[d]`` = the records the document cut would keep, ``score[d]`` = the sum of
        their patterns' weights (``set_pattern_weights``; int64, wrapping), straight from the record heap -- no segment
        pass.  ``d_doc_offsets`` None = the slot's; ``d_out`` None = a slot-owned buffer
        (``document_scores_to_host``), else a device buffer of ``n_docs`` x 16 bytes.  Returns the totals over all
        documents, (score, count)."""
        t = CDocScore(0, 0)
        self._check(self._L.pfac_documents_scores(self._ctx, slot, _ptr(d_records), _ptr(d_doc_offsets), int(n_docs),
                                                  _ptr(d_out), C.byref(t)))
        return t.score, t.count

    def selection_document_scores(self, n_docs: int, d_sel=None, d_doc_first=None, d_out=None, slot: int = 0) -> Tuple[int, int]:
        """``document_scores`` over records that are already cut per document (``pfac_selection_document_scores``):
        ``d_sel`` and ``d_doc_first`` both None = the picks of the slot's last
        ``select_leftmost_longest_documents`` -- non-overlapping matches, so "ass" inside "assassin" is not counted
        three times; else the device arrays of a selection or of ``segment_records``.  Returns the totals."""
        t = CDocScore(0, 0)
        self._check(self._L.pfac_selection_document_scores(self._ctx, slot, _ptr(d_sel), _ptr(d_doc_first), int(n_docs),
                                                           _ptr(d_out), C.byref(t)))
        return t.score, t.count

    def document_scores_to_host(self, n_docs: int, slot: int = 0, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Scores [first, first + n) of the slot's last score pass into its slot-owned buffer (default: all
        ``n_docs``): a structured array of ``SCORE_DTYPE`` (``score`` int64, ``count`` uint64)."""
        n = int(n_docs) - int(first) if n is None else int(n)
        return self._to_host(slot, lambda p: self._L.pfac_document_scores_d2h(self._ctx, slot, p, int(first), n),
                             (max(n, 0), SCORE_DTYPE))

    def matching_documents_scored(self, n_docs: int, min_score=None, max_score=None, min_count=None, max_count=None,
                                  density=None, invert: bool = False, d_scores=None, d_doc_offsets=None, d_out=None,
                                  out_cap: int = 0, slot: int = 0) -> int:
        """The documents whose score lies in [``min_score``, ``max_score``] and whose count lies in [``min_count``,
        ``max_count``] (None: that end is open) and, with ``density`` = (num, den), whose score is at least num / den
        per byte -- ``score * den >= num * length``, compared exactly (``invert``: the others), ascending, on the GPU
        (``pfac_documents_matching_scores``).  ``d_scores`` None = the slot-owned scores of the slot's last score
        pass; ``d_doc_offsets`` (read for a density only) None = the slot's offsets.  The ids go where
        ``matching_documents`` puts them.  Returns the number of documents; a too small ``out_cap`` raises
        PfacError(PFAC_E_OVERFLOW) whose ``n_matching`` attribute holds the exact count."""
        num, den = (0, 0) if density is None else (int(density[0]), int(density[1]))
        if density is not None and den <= 0:
            raise ValueError("the density's denominator must be positive")
        rule = CScoreRule(-(2 ** 63) if min_score is None else int(min_score), 2 ** 63 - 1 if max_score is None else int(max_score),
                          0 if min_count is None else int(min_count), 2 ** 64 - 1 if max_count is None else int(max_count), num, den)
        n = C.c_uint64(0)
        rc = self._L.pfac_documents_matching_scores(self._ctx, slot, _ptr(d_scores), _ptr(d_doc_offsets), int(n_docs),
                                                    C.byref(rule), PFAC_DOCS_INVERT if invert else 0, _ptr(d_out),
                                                    int(out_cap), C.byref(n))
        return self._counted(rc, n, "n_matching")

    def _score_pass(self, n_docs: int, slot: int, non_overlapping: bool) -> None:
        if non_overlapping:
            self.select_leftmost_longest_documents(n_docs, slot=slot)
            self.selection_document_scores(n_docs, slot=slot)
        else:
            self.document_scores(n_docs, slot=slot)

    def score_documents(self, docs, whole_words=False, slot: int = 0, spans: bool = False, line_match: bool = False,
                        non_overlapping: bool = False) -> np.ndarray:
        """The score and match count of every document of a batch (``docs`` as ``scan_documents`` takes it) in one
        scan: ``SCORE_DTYPE[n_docs]``.  ``non_overlapping``: over the leftmost-longest picks of each document instead
        of every match.  Only the scores come back."""
        _, n_docs = self._scan_docs(docs, slot, whole_words, spans, line_match)
        self._score_pass(n_docs, slot, non_overlapping)
        return self.document_scores_to_host(n_docs, slot)

    def score_lines(self, data, delimiter=b"\n", whole_words=False, slot: int = 0, spans: bool = False, line_match: bool = False,
                    non_overlapping: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """``score_documents`` of one buffer cut into lines at ``delimiter`` on the device -- ``grep -c`` per line, or
        a weighted sum.  Returns (offsets uint64[n_docs + 1], scores ``SCORE_DTYPE[n_docs]``)."""
        offsets, n_docs = self._scan_lines(data, delimiter, slot, whole_words, spans=spans, line_match=line_match)
        self._score_pass(n_docs, slot, non_overlapping)
        return offsets, self.document_scores_to_host(n_docs, slot)

    def grep_lines_scored(self, data, min_score=None, max_score=None, min_count=None, max_count=None, density=None,
                          invert: bool = False, delimiter=b"\n", whole_words=False, slot: int = 0, spans: bool = False,
                          line_match: bool = False, non_overlapping: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The lines of ``data`` whose score satisfies the rule of ``matching_documents_scored``, as bytes -- "the
        lines with at least three hits", "the lines whose weights sum to 5 or more": scan, split, the score pass, the
        rule and the gather on the device, with no document cut in between.  Returns what ``grep_lines`` returns: (out
        uint8[out_bytes], out_offsets uint64[n + 1], ids uint64[n])."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        _, n_docs = self._scan_lines(buf, delimiter, slot, whole_words, fetch_offsets=False, spans=spans, line_match=line_match)
        self._score_pass(n_docs, slot, non_overlapping)
        n = self.matching_documents_scored(n_docs, min_score, max_score, min_count, max_count, density, invert=invert, slot=slot)
        out_bytes = self.gather_documents(n_docs, n, int(buf.size), slot=slot)
        return (self.gathered_to_host(out_bytes, slot), self.gathered_offsets_to_host(n, slot),
                self.matching_documents_to_host(n, slot))

    # -- rank: the k best documents by score or count -----------------------
    def top_documents(self, n_docs: int, k: int, by: str = "score", lowest: bool = False, ranked: bool = True, min_score=None,
                      max_score=None, min_count=None, max_count=None, density=None, invert: bool = False, d_scores=None,
                      d_doc_offsets=None, d_out=None, out_cap: int = 0, d_top_scores=None, slot: int = 0) -> int:
        """The ``k`` best documents, on the GPU (``pfac_documents_top_scores``): by ``"score"`` (signed) or by
        ``"count"``, the largest first (``lowest``: the smallest), ties to the smaller id.  With ``ranked`` the ids come
        in rank order, else the same ids ascending.  The windows, ``density`` and ``invert`` are the rule of
        ``matching_documents_scored`` and choose the candidates; with none of them every document is one
        (``min_count=1``: matched documents only).  ``d_scores`` None = the slot-owned scores of the slot's last score
        pass.  The ids go where ``matching_documents`` puts them (``matching_documents_to_host``,
        ``gather_documents(d_ids=None)``), the winners' pairs to ``d_top_scores`` or a slot-owned buffer
        (``top_scores_to_host``); both caller's buffers hold ``out_cap`` entries.  Returns min(k, candidates); a too
        small ``out_cap`` raises PfacError(PFAC_E_OVERFLOW) whose ``n_top`` attribute holds the exact count."""
        if by not in ("score", "count"):
            raise ValueError('by is "score" or "count"')
        if k < 0:
            raise ValueError("k must not be negative")
        flags = (PFAC_TOP_BY_COUNT if by == "count" else 0) | (PFAC_TOP_LOWEST if lowest else 0) | (PFAC_TOP_RANKED if ranked else 0)
        ruled = not (min_score is None and max_score is None and min_count is None and max_count is None and density is None
                     and not invert)
        num, den = (0, 0) if density is None else (int(density[0]), int(density[1]))
        if density is not None and den <= 0:
            raise ValueError("the density's denominator must be positive")
        rule = CScoreRule(-(2 ** 63) if min_score is None else int(min_score), 2 ** 63 - 1 if max_score is None else int(max_score),
                          0 if min_count is None else int(min_count), 2 ** 64 - 1 if max_count is None else int(max_count), num, den)
        n = C.c_uint64(0)
        rc = self._L.pfac_documents_top_scores(self._ctx, slot, _ptr(d_scores), _ptr(d_doc_offsets), int(n_docs),
                                               C.byref(rule) if ruled else None, PFAC_DOCS_INVERT if invert else 0,
                                               min(int(k), 2 ** 64 - 1), flags, _ptr(d_out), int(out_cap), _ptr(d_top_scores),
                                               C.byref(n))
        return self._counted(rc, n, "n_top")

    def top_scores_to_host(self, n: int, slot: int = 0, first: int = 0) -> np.ndarray:
        """Pairs [first, first + n) of the slot's last ``top_documents`` into its slot-owned buffer, in the order of
        its ids: ``SCORE_DTYPE[n]``."""
        return self._to_host(slot, lambda p: self._L.pfac_documents_top_scores_d2h(self._ctx, slot, p, int(first), int(n)),
                             (n, SCORE_DTYPE))

    def top_scored_documents(self, docs, k: int, by: str = "score", lowest: bool = False, ranked: bool = True, min_score=None,
                             max_score=None, min_count=None, max_count=None, density=None, invert: bool = False,
                             whole_words=False, slot: int = 0, spans: bool = False, line_match: bool = False,
                             non_overlapping: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """The ``k`` best documents of a batch (``docs`` as ``scan_documents`` takes it): scan, the score pass and
        ``top_documents`` on the device.  Returns (ids uint64[n], scores ``SCORE_DTYPE[n]``), n = min(k, candidates)."""
        _, n_docs = self._scan_docs(docs, slot, whole_words, spans, line_match)
        self._score_pass(n_docs, slot, non_overlapping)
        n = self.top_documents(n_docs, k, by, lowest, ranked, min_score, max_score, min_count, max_count, density, invert, slot=slot)
        return self.matching_documents_to_host(n, slot), self.top_scores_to_host(n, slot)

    def top_lines(self, data, k: int, by: str = "score", lowest: bool = False, ranked: bool = True, min_score=None, max_score=None,
                  min_count=None, max_count=None, density=None, invert: bool = False, delimiter=b"\n", whole_words=False,
                  slot: int = 0, spans: bool = False, line_match: bool = False,
                  non_overlapping: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The ``k`` best lines of ``data``, as bytes -- "the 100 most suspicious lines of this log": scan, split, the
        score pass, ``top_documents`` and the gather on the device; neither the scores of all lines nor the ids travel.
        Returns (out uint8[out_bytes], out_offsets uint64[n + 1], ids uint64[n], scores ``SCORE_DTYPE[n]``): the
        lines back to back in the order of the ids (rank order with ``ranked``)."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        _, n_docs = self._scan_lines(buf, delimiter, slot, whole_words, fetch_offsets=False, spans=spans, line_match=line_match)
        self._score_pass(n_docs, slot, non_overlapping)
        n = self.top_documents(n_docs, k, by, lowest, ranked, min_score, max_score, min_count, max_count, density, invert, slot=slot)
        out_bytes = self.gather_documents(n_docs, n, int(buf.size), slot=slot)
        return (self.gathered_to_host(out_bytes, slot), self.gathered_offsets_to_host(n, slot),
                self.matching_documents_to_host(n, slot), self.top_scores_to_host(n, slot))

    # -- term counts: the document-term matrix in CSR form --------------------
    def document_term_counts(self, n_docs: int, d_sel=None, d_doc_first=None, selection: bool = False, d_row_ptr=None,
                             d_states=None, d_counts=None, out_cap: int = 0, slot: int = 0) -> int:
        """Which final states each document holds and how often, on the GPU (``pfac_documents_term_counts``): the
        distinct (document, state) pairs of a record array that is already cut per document, as a CSR matrix --
        ``row_ptr`` uint64[n_docs + 1], ``states`` and ``counts`` uint32[n_terms], the states of a document
        ascending.  ``d_sel`` and ``d_doc_first`` both None = the slot-owned result of the slot's last
        ``segment_records`` (``selection``: of its last ``select_leftmost_longest_documents``); else the device arrays
        of either.  ``d_row_ptr`` / ``d_states`` / ``d_counts`` None = slot-owned buffers (``term_counts_to_host``);
        else device buffers, the two entry arrays of ``out_cap`` entries.  Returns the number of pairs; a too small
        ``out_cap`` raises PfacError(PFAC_E_OVERFLOW) whose ``n_terms`` attribute holds the exact count."""
        n = C.c_uint64(0)
        rc = self._L.pfac_documents_term_counts(self._ctx, slot, _ptr(d_sel), _ptr(d_doc_first), int(n_docs),
                                                PFAC_TERMS_SELECTION if selection else 0, _ptr(d_row_ptr), _ptr(d_states),
                                                _ptr(d_counts), int(out_cap), C.byref(n))
        return self._counted(rc, n, "n_terms")

    def term_counts_to_host(self, n_docs: int, n_terms: int, slot: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(row_ptr uint64[n_docs + 1], states uint32[n_terms], counts uint32[n_terms]) of the slot's last
        ``document_term_counts`` into slot-owned buffers."""
        return self._to_host(slot, lambda r, s, c: self._L.pfac_documents_term_counts_d2h(self._ctx, slot, r, s, c),
                             (int(n_docs) + 1, np.uint64), (n_terms, np.uint32), (n_terms, np.uint32))

    def _term_pass(self, n_docs: int, slot: int, non_overlapping: bool) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        if non_overlapping:
            self.select_leftmost_longest_documents(n_docs, slot=slot)
        else:
            self.segment_records(n_docs, slot=slot)
        n_terms = self.document_term_counts(n_docs, selection=non_overlapping, slot=slot)
        return self.term_counts_to_host(n_docs, n_terms, slot)

    def term_counts_documents(self, docs, whole_words=False, spans: bool = False, line_match: bool = False,
                              non_overlapping: bool = False, slot: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The document-term matrix of a batch (``docs`` as ``scan_documents`` takes it) in one scan: the scan, the
        document cut (``non_overlapping``: the leftmost-longest picks of each document instead of every match) and
        ``document_term_counts`` on the device; only the three CSR arrays come back -- (row_ptr, states, counts).
        ``PfacTable.states_to_patterns`` turns the states into pattern ids."""
        _, n_docs = self._scan_docs(docs, slot, whole_words, spans, line_match)
        return self._term_pass(n_docs, slot, non_overlapping)

    def term_counts_lines(self, data, delimiter=b"\n", whole_words=False, spans: bool = False, line_match: bool = False,
                          non_overlapping: bool = False, slot: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``term_counts_documents`` of one buffer cut into lines at ``delimiter`` on the device: row d is line d."""
        _, n_docs = self._scan_lines(data, delimiter, slot, whole_words, fetch_offsets=False, spans=spans, line_match=line_match)
        return self._term_pass(n_docs, slot, non_overlapping)

    def term_matrix(self, n_docs: int, n_terms: int, d_row_ptr, d_states, d_counts):
        """The caller's device tensors of a ``document_term_counts`` (``d_row_ptr`` int64 or uint64 storage of n_docs + 1
        entries, ``d_states`` and ``d_counts`` 32-bit storage of at least ``n_terms``) as a ``torch.sparse_csr_tensor``
        of shape (n_docs, num_final) on their device.  The column indices are widened in torch; nothing is copied to
        the host.  The pass writes on the slot's stream: synchronise it (``sync``) before torch reads the matrix."""
        import torch
        row = d_row_ptr.view(torch.int64)[: int(n_docs) + 1]
        col = d_states.view(torch.int32)[: int(n_terms)].to(torch.int64)
        val = d_counts.view(torch.int32)[: int(n_terms)]
        return torch.sparse_csr_tensor(row, col, val, size=(int(n_docs), self._n_states()))

    # -- rule sets: which of many rules fired in each document ----------------
    def set_rules(self, rules) -> int:
        """The rule table of the uploaded table (``pfac_table_set_rules``): ``rules`` is what ``PfacTable.rule_table``
        takes (a list of rules over pattern ids) or what it returns (``rule_ptr``, ``terms``, ``need``).  Rule r fires
        in a document iff at least ``need[r]`` of its positive states and none of its negated ones occur there.  A
        table upload drops the rules; an empty list clears them.  Returns the number of rules."""
        if isinstance(rules, tuple) and len(rules) == 3 and all(isinstance(a, np.ndarray) for a in rules):
            ptr, terms, need = rules
        else:
            if self.table is None:
                raise PfacError(PFAC_E_STATE, "set_rules before load_table")
            ptr, terms, need = self.table.rule_table(rules)
        ptr = np.ascontiguousarray(ptr, dtype=np.uint64)
        terms = np.ascontiguousarray(terms, dtype=np.uint32)
        need = np.ascontiguousarray(need, dtype=np.uint32)
        if ptr.size != need.size + 1:
            raise ValueError("rule_ptr has one entry more than need")
        self._check(self._L.pfac_table_set_rules(self._ctx, ptr.ctypes.data, terms.ctypes.data if terms.size else None,
                                                 need.ctypes.data if need.size else None, int(need.size)))
        self._n_rules = int(need.size)
        return self._n_rules

    def document_rules(self, n_docs: int, d_row_ptr=None, d_states=None, d_row_ptr_out=None, d_rules=None, out_cap: int = 0,
                       slot: int = 0) -> int:
        """Which rules of ``set_rules`` fire in each document, on the GPU (``pfac_documents_rules``): the join of a
        document-term matrix with the rule table, as a CSR -- ``row_ptr`` uint64[n_docs + 1] and ``rules``
        uint32[n_fired], a document's rule ids strictly ascending.  ``d_row_ptr`` and ``d_states`` both None = the
        slot-owned result of the slot's last ``document_term_counts``; else the first two device arrays of one.
        ``d_row_ptr_out`` / ``d_rules`` None = slot-owned buffers (``rules_to_host``); else device buffers, ``d_rules``
        of ``out_cap`` entries.  Returns the number of fired (document, rule) pairs; a too small ``out_cap`` raises
        PfacError(PFAC_E_OVERFLOW) whose ``n_fired`` attribute holds the exact count."""
        n = C.c_uint64(0)
        rc = self._L.pfac_documents_rules(self._ctx, slot, _ptr(d_row_ptr), _ptr(d_states), int(n_docs), 0, _ptr(d_row_ptr_out),
                                          _ptr(d_rules), int(out_cap), C.byref(n))
        return self._counted(rc, n, "n_fired")

    def rules_to_host(self, n_docs: int, n_fired: int, slot: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """(row_ptr uint64[n_docs + 1], rules uint32[n_fired]) of the slot's last ``document_rules`` into slot-owned
        buffers."""
        return self._to_host(slot, lambda r, f: self._L.pfac_documents_rules_d2h(self._ctx, slot, r, f),
                             (int(n_docs) + 1, np.uint64), (n_fired, np.uint32))

    def _rules_pass(self, n_docs: int, slot: int, non_overlapping: bool) -> Tuple[np.ndarray, np.ndarray]:
        if non_overlapping:
            self.select_leftmost_longest_documents(n_docs, slot=slot)
        else:
            self.segment_records(n_docs, slot=slot)
        self.document_term_counts(n_docs, selection=non_overlapping, slot=slot)
        return self.rules_to_host(n_docs, self.document_rules(n_docs, slot=slot), slot)

    def rules_documents(self, docs, whole_words=False, spans: bool = False, line_match: bool = False,
                        non_overlapping: bool = False, slot: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """The fired rules of every document of a batch (``docs`` as ``scan_documents`` takes it) in one scan: the scan,
        the document cut (``non_overlapping``: the leftmost-longest picks of each document instead of every match),
        the term counts and ``document_rules`` on the device; only the CSR comes back -- (row_ptr, rules)."""
        _, n_docs = self._scan_docs(docs, slot, whole_words, spans, line_match)
        return self._rules_pass(n_docs, slot, non_overlapping)

    def rules_lines(self, data, delimiter=b"\n", whole_words=False, spans: bool = False, line_match: bool = False,
                    non_overlapping: bool = False, slot: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """``rules_documents`` of one buffer cut into lines at ``delimiter`` on the device: row d is line d."""
        _, n_docs = self._scan_lines(data, delimiter, slot, whole_words, fetch_offsets=False, spans=spans, line_match=line_match)
        return self._rules_pass(n_docs, slot, non_overlapping)

    def rule_matrix(self, n_docs: int, n_fired: int, d_row_ptr, d_rules, n_rules: Optional[int] = None):
        """The caller's device tensors of a ``document_rules`` (``d_row_ptr`` int64 or uint64 storage of n_docs + 1
        entries, ``d_rules`` 32-bit storage of at least ``n_fired``) as a ``torch.sparse_csr_tensor`` of shape (n_docs,
        n_rules) with values 1, on their device (``n_rules`` None: the rules of the last ``set_rules``).  The column
        indices are widened in torch; nothing is copied to the host.  The pass writes on the slot's stream:
        synchronise it (``sync``) before torch reads the matrix."""
        import torch
        row = d_row_ptr.view(torch.int64)[: int(n_docs) + 1]
        col = d_rules.view(torch.int32)[: int(n_fired)].to(torch.int64)
        val = torch.ones(int(n_fired), dtype=torch.int32, device=col.device)
        return torch.sparse_csr_tensor(row, col, val, size=(int(n_docs), int(self._n_rules if n_rules is None else n_rules)))

    # -- proximity rules: which pairs of pattern groups lie near each other ----
    def document_near_masks(self, n_docs: int, rules, d_sel=None, d_doc_first=None, selection: bool = False, d_out=None,
                            slot: int = 0) -> int:
        """Which proximity rules fire in each document, on the GPU (``pfac_documents_near``): ``rules`` is up to 64
        ``near_rule`` records (a list of them, or a ``NEAR_RULE_DTYPE`` array) over the pattern groups
        (``set_pattern_groups``); bit r of ``mask[d]`` is set iff document d holds two distinct records of rule r's two
        groups whose starts are at most its ``within`` bytes apart.  The input is a record array cut per document, as
        ``document_term_counts`` takes it: ``d_sel`` and ``d_doc_first`` both None = the slot-owned result of the slot's
        last ``segment_records`` (``selection``: of its last ``select_leftmost_longest_documents``).  ``d_out`` None = a
        slot-owned buffer (``near_masks_to_host``), else a device buffer of ``n_docs`` uint64.  Returns the OR of all
        masks: the rules that fired at all."""
        arr = _near_rules(rules)
        m = C.c_uint64(0)
        self._check(self._L.pfac_documents_near(self._ctx, slot, _ptr(d_sel), _ptr(d_doc_first), int(n_docs),
                                                PFAC_NEAR_SELECTION if selection else 0, arr.ctypes.data if arr.size else None,
                                                int(arr.size), _ptr(d_out), C.byref(m)))
        return m.value

    def near_masks_to_host(self, n_docs: int, slot: int = 0, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Masks [first, first + n) of the slot's last ``document_near_masks`` into its slot-owned buffer (default: all
        ``n_docs``)."""
        n = int(n_docs) - int(first) if n is None else int(n)
        return self._to_host(slot, lambda p: self._L.pfac_near_masks_d2h(self._ctx, slot, p, int(first), n),
                             (max(n, 0), np.uint64))

    def near_masks_ptr(self, slot: int = 0) -> int:
        """Device pointer of the slot-owned masks of the slot's last ``document_near_masks`` (0: none) -- what
        ``matching_documents_where`` takes as ``d_masks``."""
        return int(self._L.pfac_slot_near_masks(self._ctx, slot) or 0)

    def _near_pass(self, n_docs: int, rules, slot: int, non_overlapping: bool) -> int:
        if non_overlapping:
            self.select_leftmost_longest_documents(n_docs, slot=slot)
        else:
            self.segment_records(n_docs, slot=slot)
        return self.document_near_masks(n_docs, rules, selection=non_overlapping, slot=slot)

    def near_documents(self, docs, rules, non_overlapping: bool = False, whole_words=False, spans: bool = False,
                       line_match: bool = False, slot: int = 0) -> np.ndarray:
        """The proximity rules of every document of a batch (``docs`` as ``scan_documents`` takes it) in one scan: the
        scan, the document cut (``non_overlapping``: the leftmost-longest picks of each document instead of every
        match) and ``document_near_masks`` on the device; only the masks come back: uint64[n_docs]."""
        _, n_docs = self._scan_docs(docs, slot, whole_words, spans, line_match)
        self._near_pass(n_docs, rules, slot, non_overlapping)
        return self.near_masks_to_host(n_docs, slot)

    def near_lines(self, data, rules, delimiter=b"\n", non_overlapping: bool = False, whole_words=False, spans: bool = False,
                   line_match: bool = False, slot: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """``near_documents`` of one buffer cut into lines at ``delimiter`` on the device.  Returns (offsets uint64
        [n_docs + 1], masks uint64[n_docs])."""
        offsets, n_docs = self._scan_lines(data, delimiter, slot, whole_words, spans=spans, line_match=line_match)
        self._near_pass(n_docs, rules, slot, non_overlapping)
        return offsets, self.near_masks_to_host(n_docs, slot)

    def grep_lines_near(self, data, rules, all_of: int = 0, any_of: int = 0, none_of: int = 0, invert: bool = False,
                        delimiter=b"\n", non_overlapping: bool = False, whole_words=False, slot: int = 0, spans: bool = False,
                        line_match: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The lines of ``data`` on which the proximity rules satisfy the predicate of ``matching_documents_where``
        (bit r = rule r; all three 0: some rule fired), as bytes: scan, split, cut, the rule pass, the predicate and
        the gather on the device -- nothing but those lines crosses the link.  Returns what ``grep_lines_where``
        returns: (out uint8[out_bytes], out_offsets uint64[n + 1], ids uint64[n])."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        _, n_docs = self._scan_lines(buf, delimiter, slot, whole_words, fetch_offsets=False, spans=spans, line_match=line_match)
        self._near_pass(n_docs, rules, slot, non_overlapping)
        if not (all_of or any_of or none_of):
            any_of = 2**64 - 1
        n = self.matching_documents_where(n_docs, all_of, any_of, none_of, invert=invert,
                                          d_masks=self.near_masks_ptr(slot), slot=slot)
        out_bytes = self.gather_documents(n_docs, n, int(buf.size), slot=slot)
        return (self.gathered_to_host(out_bytes, slot), self.gathered_offsets_to_host(n, slot),
                self.matching_documents_to_host(n, slot))

    # -- leftmost-longest non-overlapping matches ---------------------------
    def select_leftmost_longest(self, entry: int = 0, d_out=None, out_cap: int = 0, slot: int = 0,
                                d_records=None) -> Tuple[int, int]:
        """Leftmost-longest, non-overlapping selection over the slot's last finished scan, on the GPU: from cursor
        ``entry`` take the first position with a record, its longest record, move the cursor past it, repeat.
        Returns (n_selected, exit): ``exit`` is how far the last pick runs past n_owned, the ``entry`` of the scan
        of the next owned range.  ``d_out`` None = a slot-owned buffer (``selection_to_host``).  A too small
        ``out_cap`` raises PfacError(PFAC_E_OVERFLOW) whose ``n_selected`` attribute holds the exact count."""
        n = C.c_uint64(0)
        ex = C.c_uint32(0)
        rc = self._L.pfac_records_leftmost_longest(self._ctx, slot, _ptr(d_records), int(entry), _ptr(d_out), int(out_cap),
                                                   C.byref(n), C.byref(ex))
        return self._counted(rc, n, "n_selected"), ex.value

    def selection_to_host(self, n_selected: int, slot: int = 0) -> np.ndarray:
        """The records of the slot's last ``select_leftmost_longest`` into its slot-owned buffer, ascending pos."""
        return self._to_host(slot, lambda p: self._L.pfac_leftmost_longest_d2h(self._ctx, slot, p), (n_selected, RECORD_DTYPE))

    def scan_leftmost_longest(self, data, n_owned: Optional[int] = None, entry: int = 0, slot: int = 0, whole_words=False,
                              prev_byte: int = -1, next_byte: int = -1) -> Tuple[np.ndarray, int]:
        """H2D + scan + selection of one host buffer (``n_owned`` < len(data) leaves the rest as halo).  Returns
        (records, exit): the leftmost-longest non-overlapping matches that start in the owned range, and the entry
        offset for the scan of the range that follows.  ``whole_words`` (True, or the word bytes): the selection
        chooses among whole-word matches only; ``prev_byte`` / ``next_byte`` are the bytes around ``data`` when it is
        one range of a longer text."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        n_avail = int(buf.size)
        n_owned = n_avail if n_owned is None else int(n_owned)
        self._ensure_final_lengths()
        self.reserve(slot, max(n_avail, 1), max(n_avail // 8, 4096))
        if n_avail:
            self.h2d(buf, slot)
        self.scan_resident(n_owned, n_avail, slot=slot)
        if whole_words is not False:
            self.filter_whole_words(slot, _word_bytes(whole_words), prev_byte=prev_byte, next_byte=next_byte)
        n, ex = self.select_leftmost_longest(entry, slot=slot)
        return self.selection_to_host(n, slot), ex

    def select_leftmost_longest_documents(self, n_docs: int, d_doc_offsets=None, d_out=None, out_cap: int = 0,
                                          d_doc_first=None, slot: int = 0, d_records=None) -> int:
        """Leftmost-longest selection of every document [off[d], off[d+1]) of the slot's last finished scan on its own,
        on the GPU (one call for the batch).  ``d_doc_offsets`` None = the slot's (``set_doc_offsets``); ``d_out`` /
        ``d_doc_first`` None = slot-owned buffers (``doc_selection_to_host``).  Positions stay relative to the scan.
        The call is the slot's last selection (entry 0, exit 0): ``replace_selection`` and
        ``replace_selection_documents`` consume it.  Returns the number of picks.  A too small ``out_cap`` raises
        PfacError(PFAC_E_OVERFLOW) whose ``n_selected`` attribute holds the exact count."""
        n = C.c_uint64(0)
        rc = self._L.pfac_records_leftmost_longest_documents(self._ctx, slot, _ptr(d_records), _ptr(d_doc_offsets),
                                                             int(n_docs), _ptr(d_out), int(out_cap), _ptr(d_doc_first),
                                                             C.byref(n))
        return self._counted(rc, n, "n_selected")

    def doc_selection_to_host(self, n_selected: int, n_docs: int, slot: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """(doc_first uint64[n_docs + 1], records) of the slot's last ``select_leftmost_longest_documents`` into
        slot-owned buffers; positions relative to the scan."""
        rec, first = self._to_host(slot, lambda r, f: self._L.pfac_leftmost_longest_documents_d2h(self._ctx, slot, r, f),
                                   (n_selected, RECORD_DTYPE), (int(n_docs) + 1, np.uint64))
        return first, rec

    def select_documents(self, docs, slot: int = 0, whole_words=False, spans: bool = False, line_match: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Leftmost-longest selection of a batch of independent documents (``docs`` as ``scan_documents`` takes it) in
        one scan.  Returns (doc_first uint64[n_docs + 1], records): the picks of document d are
        ``records[doc_first[d]:doc_first[d + 1]]``, positions relative to the document -- what
        ``scan_leftmost_longest`` of each document on its own returns."""
        offsets, n_docs = self._scan_docs(docs, slot, whole_words, spans, line_match)
        n = self.select_leftmost_longest_documents(n_docs, slot=slot)
        first, rec = self.doc_selection_to_host(n, n_docs, slot)
        if n:
            doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(first.astype(np.int64)))
            rec["pos"] -= offsets[doc].astype(np.uint32)
        return first, rec

    # -- find-and-replace over the leftmost-longest selection ---------------
    def _set_replacement_table(self, offsets, data: bytes) -> None:
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
        self._check(self._L.pfac_table_set_replacements(self._ctx, off.ctypes.data, off.size - 1, buf.ctypes.data,
                                                        len(data)))

    def set_replacements(self, replacements) -> None:
        """The replacement of every pattern of the uploaded table (``replacement_table``: a dict {id: bytes} or one
        entry per line), kept on the device until the next table upload."""
        if self.table is None:
            raise PfacError(-7, "no host table to map pattern ids to states (load_table first)")
        self._set_replacement_table(*replacement_table(self.table, replacements))

    def set_redaction(self, fill: bytes = b"*") -> None:
        """Replacements that mask every match: ``fill`` repeated to the pattern's length."""
        if self.table is None:
            raise PfacError(-7, "no host table to take the final-state lengths from (load_table first)")
        self._set_replacement_table(*redaction_table(self.table, fill))

    def _set_template_table(self, offsets, splits, data: bytes) -> None:
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        spl = np.ascontiguousarray(splits, dtype=np.uint32)
        buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
        self._check(self._L.pfac_table_set_replacement_templates(self._ctx, off.ctypes.data, spl.ctypes.data if spl.size else None,
                                                                 off.size - 1, buf.ctypes.data, len(data)))

    def set_replacement_templates(self, templates) -> None:
        """The replacement template of every pattern of the uploaded table (``template_table``: a dict {id: template}
        or one entry per line; a template is bytes, or (prefix, suffix) around the matched text as the input has it),
        kept on the device until the next table upload.  ``replace``, ``replace_lines``, ``replace_documents`` and the
        ``replace_selection*`` calls then write them; ``extract*`` writes the rewritten picks alone."""
        if self.table is None:
            raise PfacError(-7, "no host table to map pattern ids to states (load_table first)")
        self._set_template_table(*template_table(self.table, templates))

    def set_highlight(self, prefix: bytes, suffix: bytes) -> None:
        """Templates that wrap every match: ``prefix`` + the matched text + ``suffix`` (``<b>&</b>``, grep --color;
        with (b"", b"\n") ``extract_lines`` is grep -o)."""
        if self.table is None:
            raise PfacError(-7, "no host table to take the final-state lengths from (load_table first)")
        prefix, suffix = bytes(prefix), bytes(suffix)
        live = _state_lengths(self.table) >= 1
        r = prefix + suffix
        offsets = np.zeros(int(self.table.num_final) + 1, dtype=np.uint32)
        offsets[1:] = np.cumsum(np.where(live, len(r), 0), dtype=np.uint64)
        splits = np.where(live, len(prefix), TEMPLATE_PLAIN).astype(np.uint32)
        self._set_template_table(offsets, splits, r * int(live.sum()))

    def replace_selection(self, d_input=None, d_out=None, out_cap: int = 0, slot: int = 0, d_sel=None) -> int:
        """Rewrites the slot's last scan on the GPU: every pick of its last ``select_leftmost_longest`` replaced by its
        state's replacement, the bytes between copied, from the selection's entry to n_owned.  Returns the output's
        length.  ``d_out`` None = a slot-owned buffer (``replacement_to_host``); ``d_sel`` None = the slot-owned
        selection.  A too small ``out_cap`` raises PfacError(PFAC_E_OVERFLOW) whose ``out_bytes`` attribute holds the
        exact length."""
        n = C.c_uint64(0)
        rc = self._L.pfac_replace_leftmost_longest(self._ctx, slot, _ptr(d_input), _ptr(d_sel), _ptr(d_out), int(out_cap),
                                                   C.byref(n))
        return self._counted(rc, n, "out_bytes")

    def replacement_to_host(self, n: int, slot: int = 0, first: int = 0) -> np.ndarray:
        """Bytes [first, first + n) of the slot's last ``replace_selection`` into its slot-owned buffer."""
        return self._to_host(slot, lambda p: self._L.pfac_replace_d2h(self._ctx, slot, p, int(first), int(n)), (n, np.uint8))

    def replace(self, data, n_owned: Optional[int] = None, entry: int = 0, slot: int = 0, whole_words=False,
                prev_byte: int = -1, next_byte: int = -1) -> Tuple[np.ndarray, int]:
        """H2D + scan + selection + replacement of one host buffer (``n_owned`` < len(data) leaves the rest as halo).
        Returns (output bytes, exit): ``exit`` is the ``entry`` of the range that follows.  ``whole_words`` (True, or
        the word bytes): only whole-word matches are replaced; ``prev_byte`` / ``next_byte`` as in
        ``scan_leftmost_longest``."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        n_avail = int(buf.size)
        n_owned = n_avail if n_owned is None else int(n_owned)
        self._ensure_final_lengths()
        self.reserve(slot, max(n_avail, 1), max(n_avail // 8, 4096))
        if n_avail:
            self.h2d(buf, slot)
        self.scan_resident(n_owned, n_avail, slot=slot)
        if whole_words is not False:
            self.filter_whole_words(slot, _word_bytes(whole_words), prev_byte=prev_byte, next_byte=next_byte)
        _, ex = self.select_leftmost_longest(entry, slot=slot)
        n = self.replace_selection(slot=slot)
        return self.replacement_to_host(n, slot), ex

    # -- match extraction: the rewritten picks alone ------------------------
    def extract_selection(self, d_input=None, d_out=None, out_cap: int = 0, d_pick_offsets=None, slot: int = 0, d_sel=None) -> int:
        """The picks of the slot's last selection (whole-stream or per document) as their replacements or templates
        write them, back to back, on the GPU (``pfac_extract_leftmost_longest``).  Returns the output's length.
        ``d_out`` / ``d_pick_offsets`` None = slot-owned buffers of the extraction's own (``extracted_to_host`` /
        ``extract_offsets_to_host``); ``d_sel`` None = the slot-owned selection.  A too small ``out_cap`` raises
        PfacError(PFAC_E_OVERFLOW) whose ``out_bytes`` attribute holds the exact length."""
        n = C.c_uint64(0)
        rc = self._L.pfac_extract_leftmost_longest(self._ctx, slot, _ptr(d_input), _ptr(d_sel), _ptr(d_out), int(out_cap),
                                                   _ptr(d_pick_offsets), C.byref(n))
        return self._counted(rc, n, "out_bytes")

    def extracted_to_host(self, n: int, slot: int = 0, first: int = 0) -> np.ndarray:
        """Bytes [first, first + n) of the slot's last ``extract_selection`` into its slot-owned buffer."""
        return self._to_host(slot, lambda p: self._L.pfac_extract_d2h(self._ctx, slot, p, int(first), int(n)), (n, np.uint8))

    def extract_offsets_to_host(self, n_picks: int, slot: int = 0) -> np.ndarray:
        """The pick offsets (uint64[n_picks + 1]) of the slot's last ``extract_selection``."""
        return self._to_host(slot, lambda p: self._L.pfac_extract_offsets_d2h(self._ctx, slot, p),
                             (int(n_picks) + 1, np.uint64))

    def extract(self, data, n_owned: Optional[int] = None, entry: int = 0, slot: int = 0, whole_words=False,
                prev_byte: int = -1, next_byte: int = -1) -> Tuple[np.ndarray, np.ndarray, int]:
        """H2D + scan + selection + extraction of one host buffer, with the keywords of ``replace``.  Returns (bytes,
        pick_offsets uint64[n_picks + 1], exit): pick k is ``bytes[pick_offsets[k]:pick_offsets[k + 1]]``."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        n_avail = int(buf.size)
        n_owned = n_avail if n_owned is None else int(n_owned)
        self._ensure_final_lengths()
        self.reserve(slot, max(n_avail, 1), max(n_avail // 8, 4096))
        if n_avail:
            self.h2d(buf, slot)
        self.scan_resident(n_owned, n_avail, slot=slot)
        if whole_words is not False:
            self.filter_whole_words(slot, _word_bytes(whole_words), prev_byte=prev_byte, next_byte=next_byte)
        n_sel, ex = self.select_leftmost_longest(entry, slot=slot)
        n = self.extract_selection(slot=slot)
        return self.extracted_to_host(n, slot), self.extract_offsets_to_host(n_sel, slot), ex

    def extract_lines(self, data, delimiter=b"\n", whole_words=False, spans: bool = False, line_match: bool = False,
                      slot: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The matches of one buffer cut into lines at ``delimiter`` on the device, every line selected on its own
        (``select_lines``' path), then extracted.  Returns (bytes, pick_offsets uint64[n_picks + 1], doc_first uint64
        [n_docs + 1]): line d's matches are ``bytes[pick_offsets[doc_first[d]]:pick_offsets[doc_first[d + 1]]]``.  With
        ``set_highlight(b"", b"\n")`` the bytes are what grep -o prints."""
        _, n_docs = self._scan_lines(data, delimiter, slot, whole_words, fetch_offsets=False, spans=spans, line_match=line_match)
        n_sel = self.select_leftmost_longest_documents(n_docs, slot=slot)
        first, _ = self.doc_selection_to_host(0, n_docs, slot)
        n = self.extract_selection(slot=slot)
        return self.extracted_to_host(n, slot), self.extract_offsets_to_host(n_sel, slot), first

    def replace_selection_documents(self, d_input=None, d_out=None, out_cap: int = 0, d_out_offsets=None, slot: int = 0,
                                    d_sel=None, d_doc_offsets=None, d_doc_first=None) -> int:
        """``replace_selection`` over the slot's last ``select_leftmost_longest_documents``: every document's output,
        concatenated, and the output offsets of the documents (``d_out_offsets`` None = a slot-owned buffer,
        ``replacement_doc_offsets_to_host``).  ``d_doc_offsets`` / ``d_doc_first``: the buffers the selection was
        given (None = the slot's).  Returns the output's length; a too small ``out_cap`` raises
        PfacError(PFAC_E_OVERFLOW) whose ``out_bytes`` attribute holds the exact length."""
        n = C.c_uint64(0)
        rc = self._L.pfac_replace_documents(self._ctx, slot, _ptr(d_input), _ptr(d_sel), _ptr(d_doc_offsets),
                                            _ptr(d_doc_first), _ptr(d_out), int(out_cap), _ptr(d_out_offsets), C.byref(n))
        return self._counted(rc, n, "out_bytes")

    def replacement_doc_offsets_to_host(self, n_docs: int, slot: int = 0) -> np.ndarray:
        """The output offsets (uint64[n_docs + 1]) of the slot's last ``replace_selection_documents``."""
        return self._to_host(slot, lambda p: self._L.pfac_replace_documents_d2h(self._ctx, slot, p),
                             (int(n_docs) + 1, np.uint64))

    def replace_documents(self, docs, slot: int = 0, whole_words=False, spans: bool = False, line_match: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Find-and-replace in a batch of independent documents (``docs`` as ``scan_documents`` takes it) in one scan,
        every document on its own.  Returns (out_offsets uint64[n_docs + 1], out uint8[out_bytes]): document d's
        output is ``out[out_offsets[d]:out_offsets[d + 1]]`` -- what ``replace`` of each document alone returns."""
        _, n_docs = self._scan_docs(docs, slot, whole_words, spans, line_match)
        self.select_leftmost_longest_documents(n_docs, slot=slot)
        n = self.replace_selection_documents(slot=slot)
        out_off = self.replacement_doc_offsets_to_host(n_docs, slot)
        return out_off, self.replacement_to_host(n, slot)

    # -- tokenization: the token ids of the leftmost-longest picks -----------
    def set_token_ids(self, ids, byte_ids=None, byte_base: Optional[int] = None, drop_bytes: bytes = b"") -> None:
        """The token id of every pattern of the uploaded table (``token_table``: a dict {pattern id: token id} or one
        entry per line; patterns not named emit nothing) and of every byte outside a pick: ``byte_ids`` an explicit
        array of 256 entries, or ``byte_base=B`` for ``B + b``; neither = every byte is dropped.  ``drop_bytes``
        overrides the entries of those bytes to TOKEN_DROP (whitespace, say).  Kept on the device until the next table
        upload."""
        if self.table is None:
            raise PfacError(-7, "no host table to map pattern ids to states (load_table first)")
        if byte_ids is not None and byte_base is not None:
            raise ValueError("byte_ids and byte_base exclude each other")
        tok = np.ascontiguousarray(token_table(self.table, ids), dtype=np.int32)
        btok = None
        if byte_ids is not None:
            btok = np.array(byte_ids, dtype=np.int32)
            if btok.shape != (256,):
                raise ValueError("byte_ids holds 256 entries")
        elif byte_base is not None:
            btok = (int(byte_base) + np.arange(256, dtype=np.int64)).astype(np.int32)
        if btok is not None and len(drop_bytes):
            btok[np.frombuffer(bytes(drop_bytes), dtype=np.uint8)] = TOKEN_DROP
        self._check(self._L.pfac_table_set_token_ids(self._ctx, tok.ctypes.data if tok.size else None, tok.size,
                                                     btok.ctypes.data if btok is not None else None))

    def tokenize_selection(self, d_input=None, d_ids=None, out_cap: int = 0, d_pos=None, positions: bool = False,
                           slot: int = 0, d_sel=None) -> int:
        """The token ids of the slot's last ``select_leftmost_longest`` on the GPU (``pfac_tokenize_leftmost_longest``):
        a pick's token at its start, a byte's token outside every pick, from the selection's entry to n_owned.  Returns
        the number of tokens.  ``d_ids`` / ``d_pos`` None = slot-owned buffers (``tokens_to_host``); positions are
        written with ``positions`` (implied by ``d_pos``).  A too small ``out_cap`` raises PfacError(PFAC_E_OVERFLOW)
        whose ``n_tokens`` attribute holds the exact count."""
        n = C.c_uint64(0)
        flags = PFAC_TOKENS_POSITIONS if (positions or d_pos is not None) else 0
        rc = self._L.pfac_tokenize_leftmost_longest(self._ctx, slot, _ptr(d_input), _ptr(d_sel), flags, _ptr(d_ids),
                                                    int(out_cap), _ptr(d_pos), C.byref(n))
        return self._counted(rc, n, "n_tokens")

    def tokenize_selection_documents(self, d_input=None, d_ids=None, out_cap: int = 0, d_pos=None, positions: bool = False,
                                     d_tok_offsets=None, slot: int = 0, d_sel=None, d_doc_offsets=None, d_doc_first=None) -> int:
        """``tokenize_selection`` over the slot's last ``select_leftmost_longest_documents``, plus the documents' token
        offsets (``d_tok_offsets`` None = a slot-owned buffer, ``token_offsets_to_host``): document d's tokens are
        ``ids[tok_off[d]:tok_off[d + 1]]``.  ``d_doc_offsets`` / ``d_doc_first``: the buffers the selection was given
        (None = the slot's).  Returns the number of tokens; overflow as ``tokenize_selection``."""
        n = C.c_uint64(0)
        flags = PFAC_TOKENS_POSITIONS if (positions or d_pos is not None) else 0
        rc = self._L.pfac_tokenize_documents(self._ctx, slot, _ptr(d_input), _ptr(d_sel), _ptr(d_doc_offsets), _ptr(d_doc_first),
                                             flags, _ptr(d_ids), int(out_cap), _ptr(d_pos), _ptr(d_tok_offsets), C.byref(n))
        return self._counted(rc, n, "n_tokens")

    def tokens_to_host(self, n: int, positions: bool = False, slot: int = 0, first: int = 0):
        """Tokens [first, first + n) of the slot's last tokenize pass into its slot-owned buffers: ids int32[n], or
        (ids, pos uint32[n]) with ``positions``."""
        if positions:
            return self._to_host(slot, lambda a, b: self._L.pfac_tokens_d2h(self._ctx, slot, a, b, int(first), int(n)),
                                 (n, np.int32), (n, np.uint32))
        return self._to_host(slot, lambda a: self._L.pfac_tokens_d2h(self._ctx, slot, a, None, int(first), int(n)), (n, np.int32))

    def token_offsets_to_host(self, n_docs: int, slot: int = 0) -> np.ndarray:
        """The token offsets (uint64[n_docs + 1]) of the slot's last ``tokenize_selection_documents``."""
        return self._to_host(slot, lambda p: self._L.pfac_tokens_offsets_d2h(self._ctx, slot, p), (int(n_docs) + 1, np.uint64))

    def tokenize(self, data, n_owned: Optional[int] = None, entry: int = 0, whole_words=False, prev_byte: int = -1,
                 next_byte: int = -1, positions: bool = False, slot: int = 0):
        """H2D + scan + selection + tokenization of one host buffer (``n_owned`` < len(data) leaves the rest as halo).
        Returns (ids, exit), or (ids, pos, exit) with ``positions``: ``exit`` is the ``entry`` of the range that
        follows.  ``whole_words`` (True, or the word bytes): only whole-word matches become vocabulary tokens;
        ``prev_byte`` / ``next_byte`` as in ``scan_leftmost_longest``."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        n_avail = int(buf.size)
        n_owned = n_avail if n_owned is None else int(n_owned)
        self._ensure_final_lengths()
        self.reserve(slot, max(n_avail, 1), max(n_avail // 8, 4096))
        if n_avail:
            self.h2d(buf, slot)
        self.scan_resident(n_owned, n_avail, slot=slot)
        if whole_words is not False:
            self.filter_whole_words(slot, _word_bytes(whole_words), prev_byte=prev_byte, next_byte=next_byte)
        _, ex = self.select_leftmost_longest(entry, slot=slot)
        n = self.tokenize_selection(positions=positions, slot=slot)
        out = self.tokens_to_host(n, positions, slot)
        return (out[0], out[1], ex) if positions else (out, ex)

    def _tokenize_docs(self, offsets, n_docs: int, positions: bool, slot: int):
        self.select_leftmost_longest_documents(n_docs, slot=slot)
        n = self.tokenize_selection_documents(positions=positions, slot=slot)
        tok_off = self.token_offsets_to_host(n_docs, slot)
        if not positions:
            return self.tokens_to_host(n, False, slot), tok_off
        ids, pos = self.tokens_to_host(n, True, slot)
        if n:
            if offsets is None:
                offsets = self.doc_offsets_to_host(n_docs, slot)
            doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(tok_off.astype(np.int64)))
            pos -= offsets[doc].astype(np.uint32)
        return ids, pos, tok_off

    def tokenize_documents(self, docs, whole_words=False, spans: bool = False, line_match: bool = False,
                           positions: bool = False, slot: int = 0):
        """Tokenization of a batch of independent documents (``docs`` as ``scan_documents`` takes it) in one scan.
        Returns (ids, tok_off uint64[n_docs + 1]) -- document d's tokens are ``ids[tok_off[d]:tok_off[d + 1]]``, what
        ``tokenize`` of each document alone returns -- or (ids, pos, tok_off) with ``positions``, the positions relative
        to the document."""
        offsets, n_docs = self._scan_docs(docs, slot, whole_words, spans, line_match)
        return self._tokenize_docs(offsets, n_docs, positions, slot)

    def tokenize_lines(self, data, delimiter=b"\n", whole_words=False, spans: bool = False, line_match: bool = False,
                       positions: bool = False, slot: int = 0):
        """``tokenize_documents`` of one buffer cut into lines at ``delimiter`` on the device.  With ``whole_words`` only
        dictionary words on word boundaries become vocabulary tokens (the pre-tokenized MaxMatch)."""
        _, n_docs = self._scan_lines(data, delimiter, slot, whole_words, fetch_offsets=False, spans=spans, line_match=line_match)
        return self._tokenize_docs(None, n_docs, positions, slot)

    # -- WordPiece: ## continuation pieces and one [UNK] per word -------------
    def set_wordpiece(self, first_ids, cont_ids, byte_ids=None, unk_id: int = 0, word_bytes=None, max_word_bytes: int = 100) -> None:
        """The WordPiece ids of the uploaded table (``pfac_table_set_wordpiece``), as ``wordpiece_table`` returns them:
        ``first_ids`` / ``cont_ids`` int32[num_final], the id of a final state at a word's start / inside a word;
        ``byte_ids`` 256 entries for the bytes outside words (None = all dropped); ``unk_id`` the id of a word that
        cannot be tokenized; ``word_bytes`` the bytes that make up words (None = ``[0-9A-Za-z_]``, or a ``word_set``
        array); ``max_word_bytes`` (1..4095) the longest word that is not ``unk_id`` by its length alone.  Kept on the
        device until the next table upload; the ids of ``set_token_ids`` stay as they are."""
        fi = np.ascontiguousarray(first_ids, dtype=np.int32).ravel()
        ci = np.ascontiguousarray(cont_ids, dtype=np.int32).ravel()
        if fi.size != ci.size:
            raise ValueError("first_ids and cont_ids hold one entry per final state each")
        bt = None
        if byte_ids is not None:
            bt = np.ascontiguousarray(byte_ids, dtype=np.int32).ravel()
            if bt.shape != (256,):
                raise ValueError("byte_ids holds 256 entries")
        if word_bytes is None:
            ws = None
        elif isinstance(word_bytes, np.ndarray) and word_bytes.dtype == np.uint64:
            ws = np.ascontiguousarray(word_bytes)
            if ws.size != 4:
                raise ValueError("a word set holds four 64-bit words")
        else:
            ws = word_set(word_bytes)
        self._check(self._L.pfac_table_set_wordpiece(self._ctx, fi.ctypes.data if fi.size else None, ci.ctypes.data if ci.size else None,
                                                     fi.size, bt.ctypes.data if bt is not None else None, int(unk_id),
                                                     ws.ctypes.data if ws is not None else None, int(max_word_bytes)))
        self._wp_words = word_set(WORD_BYTES) if ws is None else ws.copy()

    def filter_roles(self, slot: int = 0, d_input=None, d_records=None) -> int:
        """Drops, in place on the GPU, the records of the slot's last finished scan whose pattern is not in the half of
        the WordPiece vocabulary that their position asks for (``pfac_records_filter_roles``): a record stays iff it
        starts on a word byte and its state has an id for its place -- the first id at a word's start, the continuation
        id behind another word byte.  Everything that reads the scan afterwards sees the kept records only.  Returns
        their number, which ``last_count`` reports from then on."""
        n = C.c_uint64(0)
        self._check(self._L.pfac_records_filter_roles(self._ctx, slot, _ptr(d_input), _ptr(d_records), C.byref(n)))
        self._last_n[slot] = n.value
        return n.value

    def wordpiece_selection(self, d_input=None, d_ids=None, out_cap: int = 0, d_pos=None, positions: bool = False,
                            slot: int = 0, d_sel=None) -> int:
        """The WordPiece ids of the slot's last ``select_leftmost_longest`` (entry 0) over a scan that went through
        ``filter_roles`` (``pfac_wordpiece_leftmost_longest``).  Arguments, result and overflow as
        ``tokenize_selection``; the slot-owned result is fetched with ``tokens_to_host``."""
        n = C.c_uint64(0)
        flags = PFAC_TOKENS_POSITIONS if (positions or d_pos is not None) else 0
        rc = self._L.pfac_wordpiece_leftmost_longest(self._ctx, slot, _ptr(d_input), _ptr(d_sel), flags, _ptr(d_ids),
                                                     int(out_cap), _ptr(d_pos), C.byref(n))
        return self._counted(rc, n, "n_tokens")

    def wordpiece_selection_documents(self, d_input=None, d_ids=None, out_cap: int = 0, d_pos=None, positions: bool = False,
                                      d_tok_offsets=None, slot: int = 0, d_sel=None, d_doc_offsets=None, d_doc_first=None) -> int:
        """``wordpiece_selection`` over the slot's last ``select_leftmost_longest_documents``, plus the documents' token
        offsets (``pfac_wordpiece_documents``); arguments as ``tokenize_selection_documents``.  Every document offset
        must be a word boundary (else PfacError, PFAC_E_ARG)."""
        n = C.c_uint64(0)
        flags = PFAC_TOKENS_POSITIONS if (positions or d_pos is not None) else 0
        rc = self._L.pfac_wordpiece_documents(self._ctx, slot, _ptr(d_input), _ptr(d_sel), _ptr(d_doc_offsets), _ptr(d_doc_first),
                                              flags, _ptr(d_ids), int(out_cap), _ptr(d_pos), _ptr(d_tok_offsets), C.byref(n))
        return self._counted(rc, n, "n_tokens")

    def wordpiece(self, data, n_owned: Optional[int] = None, positions: bool = False, slot: int = 0):
        """H2D + scan + role filter + selection + WordPiece of one host buffer (``n_owned`` < len(data) leaves the rest
        as halo; cut there at a byte outside words).  Returns (ids, exit), or (ids, pos, exit) with ``positions``, as
        ``tokenize`` does."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        n_avail = int(buf.size)
        n_owned = n_avail if n_owned is None else int(n_owned)
        self._ensure_final_lengths()
        self.reserve(slot, max(n_avail, 1), max(n_avail // 8, 4096))
        if n_avail:
            self.h2d(buf, slot)
        self.scan_resident(n_owned, n_avail, slot=slot)
        self.filter_roles(slot)
        _, ex = self.select_leftmost_longest(0, slot=slot)
        n = self.wordpiece_selection(positions=positions, slot=slot)
        out = self.tokens_to_host(n, positions, slot)
        return (out[0], out[1], ex) if positions else (out, ex)

    def _wordpiece_docs(self, offsets, n_docs: int, positions: bool, slot: int):
        self.filter_roles(slot)
        self.select_leftmost_longest_documents(n_docs, slot=slot)
        n = self.wordpiece_selection_documents(positions=positions, slot=slot)
        tok_off = self.token_offsets_to_host(n_docs, slot)
        if not positions:
            return self.tokens_to_host(n, False, slot), tok_off
        ids, pos = self.tokens_to_host(n, True, slot)
        if n:
            if offsets is None:
                offsets = self.doc_offsets_to_host(n_docs, slot)
            doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(tok_off.astype(np.int64)))
            pos -= offsets[doc].astype(np.uint32)
        return ids, pos, tok_off

    def wordpiece_documents(self, docs, positions: bool = False, slot: int = 0):
        """WordPiece of a batch of documents (``docs`` as ``scan_documents`` takes it) in one scan.  No word may run
        across a document end: two documents that meet between two word bytes raise PfacError (PFAC_E_ARG).  Returns
        what ``tokenize_documents`` returns."""
        offsets, n_docs = self._scan_docs(docs, slot)
        return self._wordpiece_docs(offsets, n_docs, positions, slot)

    def wordpiece_lines(self, data, delimiter=b"\n", positions: bool = False, slot: int = 0):
        """``wordpiece_documents`` of one buffer cut into lines at ``delimiter`` on the device.  The delimiter must not
        be a word byte (ValueError): a line then starts and ends on a word boundary by construction."""
        d = _delimiter_byte(delimiter)
        ws = getattr(self, "_wp_words", None)
        if ws is not None and 0 <= d <= 255 and (int(ws[d >> 6]) >> (d & 63)) & 1:
            raise ValueError("the delimiter is a word byte of the WordPiece attachment")
        _, n_docs = self._scan_lines(data, delimiter, slot, fetch_offsets=False)
        return self._wordpiece_docs(None, n_docs, positions, slot)

    # -- Unigram: the best-scoring pieces of every word (Viterbi over the record heap) --
    def set_unigram(self, pieces, byte_ids, byte_score: int, unk_id: int = 0, word_bytes=None,
                    max_word_bytes: int = 100) -> None:
        """The Unigram pieces of the uploaded table (``pfac_table_set_unigram``), as ``unigram_table`` returns them:
        ``pieces`` UNIGRAM_PIECE_DTYPE[num_final] (or int32[num_final, 4]): first id, continuation id, first score,
        continuation score of every final state, scores as integers; ``byte_ids`` 256 entries (None = all dropped);
        ``byte_score`` the integer score of a byte edge, in the pieces' fixed point (no default: it belongs below the
        lowest piece score, or byte edges beat the pieces); ``unk_id`` the id of a run of byte edges inside a word, or
        TOKEN_DROP for byte fallback (every such byte emits its ``byte_ids`` entry); ``word_bytes`` the bytes that make
        up words (None = every byte but ``\\t\\n\\v\\f\\r`` and space, or a ``word_set`` array); ``max_word_bytes``
        (1..4095) the longest word that is cut into pieces at all.  Kept on the device until the next table upload; the
        ids of ``set_token_ids`` and ``set_wordpiece`` stay as they are."""
        pc = np.asarray(pieces)
        if pc.dtype != UNIGRAM_PIECE_DTYPE:
            pc = np.ascontiguousarray(pc, dtype=np.int32)
            if pc.ndim != 2 or pc.shape[1] != 4:
                raise ValueError("pieces holds four int32 per final state")
        pc = np.ascontiguousarray(pc)
        n = int(pc.shape[0])
        bt = None
        if byte_ids is not None:
            bt = np.ascontiguousarray(byte_ids, dtype=np.int32).ravel()
            if bt.shape != (256,):
                raise ValueError("byte_ids holds 256 entries")
        if word_bytes is None:
            ws = None
        elif isinstance(word_bytes, np.ndarray) and word_bytes.dtype == np.uint64:
            ws = np.ascontiguousarray(word_bytes)
            if ws.size != 4:
                raise ValueError("a word set holds four 64-bit words")
        else:
            ws = word_set(word_bytes)
        self._check(self._L.pfac_table_set_unigram(self._ctx, pc.ctypes.data if n else None, n, bt.ctypes.data if bt is not None else None,
                                                   int(byte_score), int(unk_id), ws.ctypes.data if ws is not None else None,
                                                   int(max_word_bytes)))
        self._ug_words = word_set(UNIGRAM_SPACE) if ws is None else ws.copy()

    def unigram_records(self, d_input=None, d_ids=None, out_cap: int = 0, d_pos=None, positions: bool = False, slot: int = 0,
                        d_records=None) -> int:
        """The Unigram ids of the slot's last finished scan, straight from its record heap (``pfac_unigram_records``):
        no filter and no selection in between.  Arguments, result and overflow as ``tokenize_selection``; the
        slot-owned result is fetched with ``tokens_to_host``."""
        n = C.c_uint64(0)
        flags = PFAC_TOKENS_POSITIONS if (positions or d_pos is not None) else 0
        rc = self._L.pfac_unigram_records(self._ctx, slot, _ptr(d_input), _ptr(d_records), flags, _ptr(d_ids), int(out_cap),
                                          _ptr(d_pos), C.byref(n))
        return self._counted(rc, n, "n_tokens")

    def unigram_records_documents(self, n_docs: int, d_input=None, d_ids=None, out_cap: int = 0, d_pos=None, positions: bool = False,
                                  d_tok_offsets=None, slot: int = 0, d_records=None, d_doc_offsets=None) -> int:
        """``unigram_records`` plus the documents' token offsets (``pfac_unigram_documents``); ``d_doc_offsets`` None =
        the slot's offsets, which must hold ``n_docs`` documents.  Every document offset must be a word boundary (else
        PfacError, PFAC_E_ARG)."""
        n = C.c_uint64(0)
        flags = PFAC_TOKENS_POSITIONS if (positions or d_pos is not None) else 0
        rc = self._L.pfac_unigram_documents(self._ctx, slot, _ptr(d_input), _ptr(d_records), _ptr(d_doc_offsets), int(n_docs), flags,
                                            _ptr(d_ids), int(out_cap), _ptr(d_pos), _ptr(d_tok_offsets), C.byref(n))
        return self._counted(rc, n, "n_tokens")

    def unigram(self, data, n_owned: Optional[int] = None, positions: bool = False, slot: int = 0):
        """H2D + scan + Unigram of one host buffer (``n_owned`` < len(data) leaves the rest as halo; cut there at a byte
        outside words).  Returns ids, or (ids, pos) with ``positions``."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        n_avail = int(buf.size)
        n_owned = n_avail if n_owned is None else int(n_owned)
        self._ensure_final_lengths()
        self.reserve(slot, max(n_avail, 1), max(n_avail // 8, 4096))
        if n_avail:
            self.h2d(buf, slot)
        self.scan_resident(n_owned, n_avail, slot=slot)
        n = self.unigram_records(positions=positions, slot=slot)
        return self.tokens_to_host(n, positions, slot)

    def _unigram_docs(self, offsets, n_docs: int, positions: bool, slot: int):
        n = self.unigram_records_documents(n_docs, positions=positions, slot=slot)
        tok_off = self.token_offsets_to_host(n_docs, slot)
        if not positions:
            return self.tokens_to_host(n, False, slot), tok_off
        ids, pos = self.tokens_to_host(n, True, slot)
        if n:
            if offsets is None:
                offsets = self.doc_offsets_to_host(n_docs, slot)
            doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(tok_off.astype(np.int64)))
            pos -= offsets[doc].astype(np.uint32)
        return ids, pos, tok_off

    def unigram_documents(self, docs, positions: bool = False, slot: int = 0):
        """Unigram of a batch of documents (``docs`` as ``scan_documents`` takes it) in one scan.  No word may run
        across a document end: two documents that meet between two word bytes raise PfacError (PFAC_E_ARG).  Returns
        what ``tokenize_documents`` returns."""
        offsets, n_docs = self._scan_docs(docs, slot)
        return self._unigram_docs(offsets, n_docs, positions, slot)

    def unigram_lines(self, data, delimiter=b"\n", positions: bool = False, slot: int = 0):
        """``unigram_documents`` of one buffer cut into lines at ``delimiter`` on the device.  The delimiter must not
        be a word byte (ValueError): a line then starts and ends on a word boundary by construction."""
        d = _delimiter_byte(delimiter)
        ws = getattr(self, "_ug_words", None)
        if ws is not None and 0 <= d <= 255 and (int(ws[d >> 6]) >> (d & 63)) & 1:
            raise ValueError("the delimiter is a word byte of the Unigram attachment")
        _, n_docs = self._scan_lines(data, delimiter, slot, fetch_offsets=False)
        return self._unigram_docs(None, n_docs, positions, slot)

    # -- byte-level BPE: merges by rank over the record heap, per word --
    def set_bpe(self, pieces, byte_ids, lead=0x20, word_bytes=None, max_word_bytes: int = 64) -> None:
        """The BPE pieces of the uploaded table (``pfac_table_set_bpe``), as ``bpe_table`` returns them: ``pieces``
        BPE_PIECE_DTYPE[num_final] (or int32[num_final, 4]): id, merge rank, split (the byte length of the merge's left
        half, 0 = any) and 0 of every final state; ``byte_ids`` 256 entries (None = all dropped); ``lead`` the one byte
        outside words that a word takes from in front of it (a byte value, a one-byte ``bytes``, or None / -1 for
        none); ``word_bytes`` the bytes that make up words (None = every byte but ``\\t\\n\\v\\f\\r`` and space, or a
        ``word_set`` array); ``max_word_bytes`` (1..255) the longest word that is merged at all.  Kept on the device
        until the next table upload; the other token attachments stay as they are."""
        pc = np.asarray(pieces)
        if pc.dtype != BPE_PIECE_DTYPE:
            pc = np.ascontiguousarray(pc, dtype=np.int32)
            if pc.ndim != 2 or pc.shape[1] != 4:
                raise ValueError("pieces holds four 32-bit fields per final state")
        pc = np.ascontiguousarray(pc)
        n = int(pc.shape[0])
        bt = None
        if byte_ids is not None:
            bt = np.ascontiguousarray(byte_ids, dtype=np.int32).ravel()
            if bt.shape != (256,):
                raise ValueError("byte_ids holds 256 entries")
        if word_bytes is None:
            ws = None
        elif isinstance(word_bytes, np.ndarray) and word_bytes.dtype == np.uint64:
            ws = np.ascontiguousarray(word_bytes)
            if ws.size != 4:
                raise ValueError("a word set holds four 64-bit words")
        else:
            ws = word_set(word_bytes)
        if lead is None:
            lead = -1
        elif not isinstance(lead, (int, np.integer)):
            if len(bytes(lead)) != 1:
                raise ValueError("the lead is one byte")
            lead = bytes(lead)[0]
        self._check(self._L.pfac_table_set_bpe(self._ctx, pc.ctypes.data if n else None, n, bt.ctypes.data if bt is not None else None,
                                               ws.ctypes.data if ws is not None else None, int(lead), int(max_word_bytes)))
        self._bpe_words = word_set(UNIGRAM_SPACE) if ws is None else ws.copy()
        self._bpe_lead = int(lead)

    def bpe_records(self, d_input=None, d_ids=None, out_cap: int = 0, d_pos=None, positions: bool = False, slot: int = 0,
                    d_records=None) -> int:
        """The BPE ids of the slot's last finished scan, straight from its record heap (``pfac_bpe_records``).
        Arguments, result and overflow as ``unigram_records``; the slot-owned result is fetched with
        ``tokens_to_host``."""
        n = C.c_uint64(0)
        flags = PFAC_TOKENS_POSITIONS if (positions or d_pos is not None) else 0
        rc = self._L.pfac_bpe_records(self._ctx, slot, _ptr(d_input), _ptr(d_records), flags, _ptr(d_ids), int(out_cap),
                                      _ptr(d_pos), C.byref(n))
        return self._counted(rc, n, "n_tokens")

    def bpe_records_documents(self, n_docs: int, d_input=None, d_ids=None, out_cap: int = 0, d_pos=None, positions: bool = False,
                              d_tok_offsets=None, slot: int = 0, d_records=None, d_doc_offsets=None) -> int:
        """``bpe_records`` plus the documents' token offsets (``pfac_bpe_documents``); ``d_doc_offsets`` None = the
        slot's offsets, which must hold ``n_docs`` documents.  No document offset may lie inside a word, and between a
        lead byte and its run is inside (else PfacError, PFAC_E_ARG)."""
        n = C.c_uint64(0)
        flags = PFAC_TOKENS_POSITIONS if (positions or d_pos is not None) else 0
        rc = self._L.pfac_bpe_documents(self._ctx, slot, _ptr(d_input), _ptr(d_records), _ptr(d_doc_offsets), int(n_docs), flags,
                                        _ptr(d_ids), int(out_cap), _ptr(d_pos), _ptr(d_tok_offsets), C.byref(n))
        return self._counted(rc, n, "n_tokens")

    def bpe(self, data, n_owned: Optional[int] = None, positions: bool = False, slot: int = 0):
        """H2D + scan + BPE of one host buffer (``n_owned`` < len(data) leaves the rest as halo; cut there at a byte
        outside words that is not a lead).  Returns ids, or (ids, pos) with ``positions``."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        n_avail = int(buf.size)
        n_owned = n_avail if n_owned is None else int(n_owned)
        self._ensure_final_lengths()
        self.reserve(slot, max(n_avail, 1), max(n_avail // 8, 4096))
        if n_avail:
            self.h2d(buf, slot)
        self.scan_resident(n_owned, n_avail, slot=slot)
        n = self.bpe_records(positions=positions, slot=slot)
        return self.tokens_to_host(n, positions, slot)

    def _bpe_docs(self, offsets, n_docs: int, positions: bool, slot: int):
        n = self.bpe_records_documents(n_docs, positions=positions, slot=slot)
        tok_off = self.token_offsets_to_host(n_docs, slot)
        if not positions:
            return self.tokens_to_host(n, False, slot), tok_off
        ids, pos = self.tokens_to_host(n, True, slot)
        if n:
            if offsets is None:
                offsets = self.doc_offsets_to_host(n_docs, slot)
            doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(tok_off.astype(np.int64)))
            pos -= offsets[doc].astype(np.uint32)
        return ids, pos, tok_off

    def bpe_documents(self, docs, positions: bool = False, slot: int = 0):
        """BPE of a batch of documents (``docs`` as ``scan_documents`` takes it) in one scan.  No word may run across a
        document end, and none may end on a lead byte whose run opens the next: PfacError (PFAC_E_ARG).  Returns what
        ``tokenize_documents`` returns."""
        offsets, n_docs = self._scan_docs(docs, slot)
        return self._bpe_docs(offsets, n_docs, positions, slot)

    def bpe_lines(self, data, delimiter=b"\n", positions: bool = False, slot: int = 0):
        """``bpe_documents`` of one buffer cut into lines at ``delimiter`` on the device.  The delimiter must be neither
        a word byte nor the lead (ValueError): a line then starts and ends outside every word by construction."""
        d = _delimiter_byte(delimiter)
        ws = getattr(self, "_bpe_words", None)
        if ws is not None and 0 <= d <= 255 and ((int(ws[d >> 6]) >> (d & 63)) & 1 or d == self._bpe_lead):
            raise ValueError("the delimiter is a word byte or the lead of the BPE attachment")
        _, n_docs = self._scan_lines(data, delimiter, slot, fetch_offsets=False)
        return self._bpe_docs(None, n_docs, positions, slot)

    # -- synthetic inputs (device resident) --------------------------------
    def fill_tiled(self, d_dst, n: int, pattern: bytes, phase: int = 0, slot: int = 0) -> None:
        pat = np.frombuffer(pattern, dtype=np.uint8)
        self._check(self._L.pfac_fill_tiled(self._ctx, slot, _ptr(d_dst), int(n), pat.ctypes.data, pat.size, int(phase)))

    def fill_random(self, d_dst, n: int, seed: int, slot: int = 0) -> None:
        self._check(self._L.pfac_fill_random(self._ctx, slot, _ptr(d_dst), int(n), int(seed) & (2**64 - 1)))


def _docs_buffer(docs) -> Tuple[np.ndarray, np.ndarray]:
    """A batch of documents -> (buffer uint8, offsets uint64[n_docs + 1]).  ``docs`` is a sequence of bytes-like
    objects, or a ``(buffer, offsets)`` pair whose offsets (an integer array or list, n_docs + 1 of them, from 0 to
    len(buffer)) cut ``buffer`` into documents."""
    if (isinstance(docs, tuple) and len(docs) == 2 and isinstance(docs[1], (np.ndarray, list, range))
            and np.asarray(docs[1]).dtype != np.uint8):
        buf, offsets = docs
        buf = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf.view(np.uint8).ravel()
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    else:
        parts = [np.frombuffer(d, dtype=np.uint8) if not isinstance(d, np.ndarray) else d.view(np.uint8).ravel()
                 for d in docs]
        offsets = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            np.cumsum([p.size for p in parts], out=offsets[1:])
        buf = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return buf, offsets


def trace_table_compat(input_bytes: np.ndarray, table: PfacTable, device: int = 0) -> np.ndarray:
    """Call the reference-shaped one-shot seam (``pfac_trace_table_compat``) and return its dense
    ``input_size x max_pat_len`` result array (0xFFFFFFFF = empty), as ``GPU_TraceTable`` fills it."""
    from ._ffi import CThreadData
    L = hip_lib()
    inp = np.ascontiguousarray(input_bytes, dtype=np.uint8)
    n = int(inp.size)
    dense = np.empty((max(n, 1), table.max_pat_len), dtype=np.uint32)
    s0 = np.ascontiguousarray(table.s0); r = np.ascontiguousarray(table.r)
    HT = np.ascontiguousarray(table.HT); val = np.ascontiguousarray(table.val)
    d = CThreadData(inp.ctypes.data, n, table.state_num, table.num_final, dense.ctypes.data, table.ht_size,
                    table.width, s0.ctypes.data, table.max_pat_len, r.ctypes.data, HT.ctypes.data, val.ctypes.data)
    rc = L.pfac_trace_table_compat(C.byref(d), int(device))
    if rc:
        raise PfacError(rc, (L.pfac_last_error(None) or b"").decode())
    return dense[:n]


def splitmix64_bytes(n: int, seed: int) -> np.ndarray:
    """CPU twin of ``pfac_fill_random`` (byte i = byte i&7 of splitmix64(seed + i>>3)); test helper."""
    words = (n + 7) // 8
    x = (np.arange(words, dtype=np.uint64) + np.uint64(seed & (2**64 - 1)))
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x.view(np.uint8)[:n].copy()


def tiled_bytes(n: int, pattern: bytes, phase: int = 0) -> np.ndarray:
    """CPU twin of ``pfac_fill_tiled``."""
    pat = np.frombuffer(pattern, dtype=np.uint8)
    idx = (np.arange(n, dtype=np.int64) + phase) % pat.size
    return pat[idx]
