"""The contract of the eleven fetches of slot-owned pass outputs (run with -m gpu on an MI355X): one table, every
fetch through the same situations, status codes straight from the C ABI.

    before the pass has ever run                          PFAC_E_STATE
    after the pass wrote into the caller's buffers        PFAC_E_STATE
    after a good slot-owned run                           the contents of the caller's-buffer run of the same pass
    a window that ends exactly at the end                 OK                  (the windowed fetches)
    a window one past the end                             PFAC_E_ARG
    first == length with n == 0                           OK
    a NULL host pointer where elements are asked for      PFAC_E_ARG
    after a later refused call of the same pass           PFAC_E_STATE: the earlier slot-owned result is gone

What a fetch cannot reach, and why:
  * the halves of the two pair fetches (pfac_segment_d2h, pfac_leftmost_longest_documents_d2h) take NULL as "not this
    half": no NULL-pointer error; they and the other whole-result fetches have no window;
  * pfac_slot_doc_offsets_d2h and pfac_text_d2h have no caller's-buffer form (their outputs are always the slot's);
  * a refused pfac_slot_doc_offsets / _split leaves the slot's offsets as they were (the header says so), a refused
    pfac_emit_text_device is refused before it touches the text, and a refused count leaves the slot's counts (they
    accumulate across calls): for these three the table asks that the earlier result SURVIVES the refused call;
  * pfac_state_counts_d2h after a caller's-buffer count is PFAC_E_STATE only while the slot has no counts of its own;
  * pfac_text_d2h has no "never run" state: before a text was made its length is 0, so n == 0 is OK and n > 0 is
    PFAC_E_ARG.

The input is four lines, two of them with matches; three patterns with lengths and replacements; one slot.  Every row
starts from a fresh context."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch

from phfpfac_amd import GpuMatcher, PfacTable
from phfpfac_amd import _ffi
from phfpfac_amd.table import RECORD_DTYPE

pytestmark = pytest.mark.gpu

OK, E_ARG, E_STATE = _ffi.PFAC_OK, _ffi.PFAC_E_ARG, _ffi.PFAC_E_STATE
PATTERNS = b"ab\ncd\nabc\n"
REPLACEMENTS = [b"X", b"YY", b"ZZZZ"]
TEXT = b"xx ab yy\nnothing\ncd abc\nplain\n"
OFFSETS = np.array([0, 9, 17, 24, 30], dtype=np.uint64)
N_DOCS = 4
CAP = 256                                   # elements of every caller's buffer: far more than any output here
U64, U8 = np.dtype(np.uint64), np.dtype(np.uint8)
assert OFFSETS[-1] == len(TEXT) and TEXT.count(b"\n") == N_DOCS


def ptr(x):
    return None if x is None else int(x.data_ptr())


class Session:
    """A fresh context with the table, its lengths and replacements, and one finished scan of TEXT in slot 0."""

    def __init__(self):
        self.g = g = GpuMatcher(0, 1)
        self.L, self.ctx = g._L, g._ctx
        g.load_table(PfacTable.from_bytes(PATTERNS))
        g._ensure_final_lengths()
        g.set_replacements(REPLACEMENTS)
        g.reserve(0, len(TEXT), 4096)
        g.h2d(np.frombuffer(TEXT, dtype=np.uint8))
        self.n_matches = g.scan_resident(len(TEXT))
        self.n_states = int(g.table.num_final)
        self.n_ids = 0
        self.keep = []

    def bufs(self, k, caller):
        """k caller's device buffers of CAP x 8 bytes (or k times None: the slot's own)."""
        if not caller:
            return [None] * k
        ts = [torch.zeros(CAP, dtype=torch.int64, device="cuda:0") for _ in range(k)]
        torch.cuda.synchronize()            # (the slot's stream is not torch's)
        self.keep += ts
        return ts

    def rc(self, name, *args):
        """Status of a pass called with `args` and its count pointer(s) behind them."""
        outs = [C.byref(C.c_uint64(0))]
        if name == "pfac_records_leftmost_longest":
            outs.append(C.byref(C.c_uint32(0)))
        if name == "pfac_slot_doc_offsets_split":
            outs.append(C.byref(C.c_uint64(0)))
        return getattr(self.L, name)(self.ctx, 0, *args, *outs)

    def call(self, name, *args):
        """A pass that must succeed; -> its count."""
        n = C.c_uint64(0)
        outs = [C.byref(n)]
        if name == "pfac_records_leftmost_longest":
            outs.append(C.byref(C.c_uint32(0)))
        if name == "pfac_slot_doc_offsets_split":
            outs.append(C.byref(C.c_uint64(0)))
        rc = getattr(self.L, name)(self.ctx, 0, *args, *outs)
        assert rc == OK, (name, rc, self.L.pfac_last_error(self.ctx))
        return n.value

    def read(self, t, n, dtype):
        self.g.sync()
        return t.cpu().numpy().view(np.uint8)[:n * dtype.itemsize].view(dtype).copy()

    def close(self):
        self.g.close()


# ---------------------------------------------------------------------------
# the passes: run(s, caller) -> {output: (caller's tensor or None, elements, dtype)}

def set_offsets(s):
    s.g.set_doc_offsets(OFFSETS)


def run_segment(s, caller):
    out, first = s.bufs(2, caller)
    n = s.call("pfac_records_segment", None, None, N_DOCS, ptr(out), CAP, ptr(first))
    return {"records": (out, n, RECORD_DTYPE), "first": (first, N_DOCS + 1, U64)}


def run_select(s, caller):
    out, = s.bufs(1, caller)
    n = s.call("pfac_records_leftmost_longest", None, 0, ptr(out), CAP)
    return {"records": (out, n, RECORD_DTYPE)}


def run_select_docs(s, caller):
    out, first = s.bufs(2, caller)
    n = s.call("pfac_records_leftmost_longest_documents", None, None, N_DOCS, ptr(out), CAP, ptr(first))
    return {"records": (out, n, RECORD_DTYPE), "first": (first, N_DOCS + 1, U64)}


def run_replace(s, caller):
    out, = s.bufs(1, caller)
    n = s.call("pfac_replace_leftmost_longest", None, None, ptr(out), CAP * 8)
    return {"bytes": (out, n, U8)}


def run_replace_docs(s, caller):
    out, off = s.bufs(2, caller)
    n = s.call("pfac_replace_documents", None, None, None, None, ptr(out), CAP * 8, ptr(off))
    return {"bytes": (out, n, U8), "offsets": (off, N_DOCS + 1, U64)}


def run_matching(s, caller):
    out, = s.bufs(1, caller)
    n = s.call("pfac_documents_matching", None, N_DOCS, 0, ptr(out), CAP)
    if not caller:
        s.n_ids = n
    return {"ids": (out, n, U64)}


def run_gather(s, caller):
    out, off = s.bufs(2, caller)
    n = s.call("pfac_documents_gather", None, len(TEXT), None, N_DOCS, None, s.n_ids, ptr(out), CAP * 8, ptr(off))
    return {"bytes": (out, n, U8), "offsets": (off, s.n_ids + 1, U64)}


def run_split(s, caller):
    assert not caller
    assert s.call("pfac_slot_doc_offsets_split", None, len(TEXT), ord("\n")) == N_DOCS
    return {"offsets": (None, N_DOCS + 1, U64)}


def run_count(s, caller):
    out, = s.bufs(1, caller)
    assert s.call("pfac_records_count_states", None, ptr(out), s.n_states, 0) == s.n_matches
    return {"counts": (out, s.n_states, U64)}


def run_text(s, caller):
    assert not caller
    return {"text": (None, s.call("pfac_emit_text_device", None, 0), U8)}


def misaligned(s):
    return ptr(s.bufs(1, True)[0]) + 1


def whole(name, *halves):
    """A whole-result fetch: fetch(s, host pointer, first, n) ignores the window; `halves` places the pointer."""
    def fetch(s, host, first, n):
        args = [host if h else None for h in halves] if halves else [host]
        return getattr(s.L, name)(s.ctx, 0, *args)
    return fetch


def windowed(name):
    return lambda s, host, first, n: getattr(s.L, name)(s.ctx, 0, host, first, n)


Row = namedtuple("Row", "id fetch prepare run key refuse window null_is_error stateful caller discards")

ROWS = [
    Row("segment_records", whole("pfac_segment_d2h", 1, 0), [set_offsets], run_segment, "records",
        lambda s: s.rc("pfac_records_segment", None, None, N_DOCS + 1, None, 0, None), False, False, True, True, True),
    Row("segment_doc_first", whole("pfac_segment_d2h", 0, 1), [set_offsets], run_segment, "first",
        lambda s: s.rc("pfac_records_segment", None, None, N_DOCS + 1, None, 0, None), False, False, True, True, True),
    Row("leftmost_longest", whole("pfac_leftmost_longest_d2h"), [], run_select, "records",
        lambda s: s.rc("pfac_records_leftmost_longest", None, 1 << 20, None, 0), False, True, True, True, True),
    Row("leftmost_longest_documents_records", whole("pfac_leftmost_longest_documents_d2h", 1, 0), [set_offsets],
        run_select_docs, "records",
        lambda s: s.rc("pfac_records_leftmost_longest_documents", None, None, N_DOCS + 1, None, 0, None),
        False, False, True, True, True),
    Row("leftmost_longest_documents_doc_first", whole("pfac_leftmost_longest_documents_d2h", 0, 1), [set_offsets],
        run_select_docs, "first",
        lambda s: s.rc("pfac_records_leftmost_longest_documents", None, None, N_DOCS + 1, None, 0, None),
        False, False, True, True, True),
    Row("replace", windowed("pfac_replace_d2h"), [lambda s: run_select(s, False)], run_replace, "bytes",
        lambda s: s.rc("pfac_replace_leftmost_longest", None, None, misaligned(s), CAP), True, True, True, True, True),
    Row("replace_documents", whole("pfac_replace_documents_d2h"), [set_offsets, lambda s: run_select_docs(s, False)],
        run_replace_docs, "offsets",
        lambda s: s.rc("pfac_replace_documents", None, None, None, None, misaligned(s), CAP, None),
        False, True, True, True, True),
    Row("documents_matching", whole("pfac_documents_matching_d2h"), [set_offsets, lambda s: run_segment(s, False)],
        run_matching, "ids", lambda s: s.rc("pfac_documents_matching", None, N_DOCS, 2, None, 0),
        False, True, True, True, True),
    Row("documents_gather", windowed("pfac_documents_gather_d2h"),
        [set_offsets, lambda s: run_segment(s, False), lambda s: run_matching(s, False)], run_gather, "bytes",
        lambda s: s.rc("pfac_documents_gather", None, (1 << 32) + 1, None, N_DOCS, None, s.n_ids, None, 0, None),
        True, True, True, True, True),
    Row("documents_gather_offsets", whole("pfac_documents_gather_offsets_d2h"),
        [set_offsets, lambda s: run_segment(s, False), lambda s: run_matching(s, False)], run_gather, "offsets",
        lambda s: s.rc("pfac_documents_gather", None, (1 << 32) + 1, None, N_DOCS, None, s.n_ids, None, 0, None),
        False, True, True, True, True),
    Row("slot_doc_offsets", windowed("pfac_slot_doc_offsets_d2h"), [], run_split, "offsets",
        lambda s: s.rc("pfac_slot_doc_offsets_split", None, len(TEXT), 256), True, True, True, False, False),
    Row("state_counts", whole("pfac_state_counts_d2h"), [], run_count, "counts",
        lambda s: s.rc("pfac_records_count_states", None, None, s.n_states, 2), False, True, True, True, False),
    Row("text", windowed("pfac_text_d2h"), [], run_text, "text",
        lambda s: s.rc("pfac_emit_text_device", None, 10 ** 18), True, True, False, False, False),
]


@pytest.fixture
def s():
    sess = Session()
    yield sess
    sess.close()


def fetched(s, row, first, n, dtype):
    """Elements [first, first + n) through the row's fetch, which must succeed."""
    host = np.full(max(n, 1), 0xEE, dtype=np.uint8).repeat(dtype.itemsize).view(dtype)
    assert row.fetch(s, host.ctypes.data, first, n) == OK, (row.id, first, n, s.L.pfac_last_error(s.ctx))
    s.g.sync()
    return host[:n]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_fetch_contract(s, row):
    spare = np.zeros(CAP, dtype=np.uint64)                  # a host buffer for the fetches that must fail
    for step in row.prepare:
        step(s)
    # before the pass has ever run
    if row.stateful:
        assert row.fetch(s, spare.ctypes.data, 0, 1) == E_STATE
    else:
        assert row.fetch(s, spare.ctypes.data, 0, 0) == OK
        assert row.fetch(s, spare.ctypes.data, 0, 1) == E_ARG
    # after the pass wrote into the caller's buffers
    want = None
    if row.caller:
        t, n, dtype = row.run(s, True)[row.key]
        want = s.read(t, n, dtype)
        assert row.fetch(s, spare.ctypes.data, 0, min(n, 1)) == E_STATE
    # after a good slot-owned run: the same contents
    _, n, dtype = row.run(s, False)[row.key]
    assert n > 0, "the setup must reach a non-empty result"
    got = fetched(s, row, 0, n, dtype)
    if want is None and row.key == "offsets":
        want = OFFSETS
    if want is not None:
        assert want.size == n
        np.testing.assert_array_equal(got, want)
    else:                                                   # the text: one line per match
        assert bytes(got).count(b"\n") == s.n_matches and bytes(got).endswith(b"\n")
    if row.window:
        np.testing.assert_array_equal(fetched(s, row, 1, n - 1, dtype), got[1:])      # ends exactly at the end
        np.testing.assert_array_equal(fetched(s, row, n - 1, 1, dtype), got[n - 1:])
        assert row.fetch(s, spare.ctypes.data, 1, n) == E_ARG                          # one past the end
        assert row.fetch(s, spare.ctypes.data, n, 1) == E_ARG
        assert row.fetch(s, spare.ctypes.data, n, 0) == OK                             # first == length, n == 0
        assert row.fetch(s, None, n, 0) == OK
        assert row.fetch(s, spare.ctypes.data, n + 1, 0) == E_ARG
    if row.null_is_error:
        assert row.fetch(s, None, 0, 1) == E_ARG
    np.testing.assert_array_equal(fetched(s, row, 0, n, dtype), got)                   # the failures discarded nothing
    # after a later refused call of the same pass
    assert row.refuse(s) == E_ARG
    if row.discards:
        assert row.fetch(s, spare.ctypes.data, 0, 1) == E_STATE
    else:
        np.testing.assert_array_equal(fetched(s, row, 0, n, dtype), got)


def test_pair_fetches_take_the_halves_apart(s):
    """One half into the caller's buffer, the other slot-owned: each half of the pair fetch answers for itself."""
    set_offsets(s)
    out, = s.bufs(1, True)
    n = s.call("pfac_records_segment", None, None, N_DOCS, ptr(out), CAP, None)
    rec, first = np.zeros(CAP, dtype=RECORD_DTYPE), np.zeros(N_DOCS + 1, dtype=np.uint64)
    assert s.L.pfac_segment_d2h(s.ctx, 0, rec.ctypes.data, None) == E_STATE
    assert s.L.pfac_segment_d2h(s.ctx, 0, rec.ctypes.data, first.ctypes.data) == E_STATE
    assert s.L.pfac_segment_d2h(s.ctx, 0, None, first.ctypes.data) == OK
    s.g.sync()
    assert first[0] == 0 and first[-1] == n
    assert s.L.pfac_leftmost_longest_documents_d2h(s.ctx, 0, None, first.ctypes.data) == E_STATE    # no selection yet
    run_select(s, False)                                    # a plain selection is not a per-document one
    assert s.L.pfac_leftmost_longest_documents_d2h(s.ctx, 0, None, first.ctypes.data) == E_STATE
    assert s.L.pfac_leftmost_longest_d2h(s.ctx, 0, rec.ctypes.data) == OK
    s.g.sync()


def test_null_defaults_need_a_slot_owned_result(s):
    """What a pass takes from the slot when its argument is NULL is the previous pass's slot-owned output: PFAC_E_STATE
    when that went to the caller's buffer (or there is none), PFAC_E_ARG when its count is not the one given."""
    set_offsets(s)
    # pfac_documents_matching: doc_first of the segment pass
    assert s.rc("pfac_documents_matching", None, N_DOCS, 0, None, 0) == E_STATE          # none yet
    run_segment(s, True)
    assert s.rc("pfac_documents_matching", None, N_DOCS, 0, None, 0) == E_STATE          # the caller's buffer
    run_segment(s, False)
    assert s.rc("pfac_documents_matching", None, N_DOCS + 1, 0, None, 0) == E_ARG
    # pfac_documents_gather: the ids of the matching pass
    gather = lambda n_ids: s.rc("pfac_documents_gather", None, len(TEXT), None, N_DOCS, None, n_ids, None, 0, None)
    assert gather(0) == E_STATE                                                          # (the refused call left none)
    n_ids = run_matching(s, True)["ids"][1]
    assert gather(n_ids) == E_STATE
    assert run_matching(s, False)["ids"][1] == n_ids
    assert gather(n_ids + 1) == E_ARG
    assert gather(n_ids) == OK
    # d_sel of the replace and of the selection's counts: the selection
    replace = lambda: s.rc("pfac_replace_leftmost_longest", None, None, None, 0)
    count = lambda: s.rc("pfac_selection_count_states", None, None, s.n_states, 0)
    assert replace() == E_STATE and count() == E_STATE
    run_select(s, True)
    assert replace() == E_STATE and count() == E_STATE
    run_select(s, False)
    assert replace() == OK and count() == OK


def test_fetch_windows_do_not_wrap(s):
    """first = 2^64 - 1 with n = 2: first + n wraps to 1.  PFAC_E_ARG before anything is copied, and the fetch after
    it works."""
    n = s.call("pfac_emit_text_device", None, 0)
    host = np.zeros(n, dtype=np.uint8)
    assert s.L.pfac_text_d2h(s.ctx, 0, host.ctypes.data, 2 ** 64 - 1, 2) == E_ARG
    assert s.L.pfac_text_d2h(s.ctx, 0, host.ctypes.data, 0, n) == OK
    s.g.sync()
    assert bytes(host).count(b"\n") == s.n_matches
    out, = s.bufs(1, True)
    assert s.n_matches >= 2
    assert s.L.pfac_records_expand(s.ctx, 0, None, 2 ** 64 - 1, 2, ptr(out)) == E_ARG
    assert s.L.pfac_records_expand(s.ctx, 0, None, 0, s.n_matches, ptr(out)) == OK
    rec = s.read(out, s.n_matches, RECORD_DTYPE)
    np.testing.assert_array_equal(rec, s.g.records_to_host(s.n_matches))
