"""The matching lines' bytes gathered on the GPU, and context lines (run with -m gpu on an MI355X):
pfac_documents_gather and its fetches against tests/gatherref.py (the rule of include/pfac.h in numpy, pinned to a
slices-and-join form by tests/test_gather_ref.py) with guard bands of exactly out_bytes and (n_ids + 1) x 8 bytes around
the caller's buffers, its errors (each one answered by the host or by the first pass -- none provokes a fault),
pfac_documents_matching_context against gatherref.context_ids, and the line path end to end against a plain Python grep.
Integer work: bit-exact.  No expectation comes from the device."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from gatherref import all_gather_cases, assert_context, assert_gather, context_ids, context_windows, gather_ref
from heapguard import GuardedBuffer
from phfpfac_amd import GpuMatcher, PfacError, PfacTable
from phfpfac_amd import _ffi
from splitref import MATCH_DOCS, MATCH_KINDS, assert_matching, doc_first_case, matching_ids

pytestmark = pytest.mark.gpu

CASES = all_gather_cases()
SHIFT = 48                                  # a caller's input starts here in its allocation: 16-B aligned, not 256
PADS = (0x5A, 0xA5)                         # what the bytes from n_bytes to the next tile hold: a value, then its complement


@pytest.fixture(scope="module")
def g():
    with GpuMatcher(0, 1) as m:
        yield m


def status_of(fn):
    with pytest.raises(PfacError) as e:
        fn()
    return e.value.status


def device_bytes(host, shift=0):
    """A device tensor holding `host` from byte `shift` on; -> (tensor, pointer of the first byte of `host`)."""
    t = torch.zeros(shift + host.size + 16, dtype=torch.uint8, device="cuda:0")
    t[shift:shift + host.size] = torch.from_numpy(host)
    torch.cuda.synchronize()                # (the slot's stream is not torch's)
    return t, int(t.data_ptr()) + shift


def device_u64(a):
    """A device copy of uint64 values (one spare entry, so that an empty array still has an address)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    t = torch.from_numpy(np.append(a, np.uint64(0)).view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def place_input(g, case, pad, source):
    """The case's bytes in the slot's input buffer or in a caller's buffer; -> (keep-alive, d_input)."""
    storage = case.storage(pad)
    if source == "slot":
        g.reserve(0, storage.size)
        g.h2d(storage)
        return None, None
    keep, ptr = device_bytes(storage, SHIFT)
    assert ptr % 16 == 0 and ptr % 256 != 0
    return keep, ptr


def guards(out_bytes, n_ids):
    gb, go = GuardedBuffer(out_bytes), GuardedBuffer((n_ids + 1) * 8, fill=0x3C)
    torch.cuda.synchronize()                # the fills are done before the slot's stream writes
    return gb, go


# ---------------------------------------------------------------------------
# the gather

@pytest.mark.parametrize("source", ["slot", "caller"])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_gather_equals_reference(g, case, source):
    """Every named case from the slot's input and from a caller's buffer at a 16-B aligned offset of its allocation,
    into buffers of exactly out_bytes and (n_ids + 1) x 8 bytes: one byte short is an overflow that writes nothing, at
    exact capacity the count, every offset and every byte equal the reference and the guards are intact; the bytes
    behind n_bytes hold a value, then its complement, and the output is the same; the slot-owned form agrees."""
    want, _ = gather_ref(case.data, case.offsets, case.ids)
    g.set_doc_offsets(case.offsets)
    d_ids = device_u64(case.ids)
    seen = []
    for pad in PADS:
        keep, d_in = place_input(g, case, pad, source)
        what = f"({source}, padding 0x{pad:02x})"
        gb, go = guards(want.size, case.n_ids)
        args = dict(d_input=d_in, d_ids=d_ids, d_out=gb.ptr, d_out_offsets=go.ptr)
        if want.size:
            with pytest.raises(PfacError) as e:
                g.gather_documents(case.n_docs, case.n_ids, case.n, out_cap=want.size - 1, **args)
            assert e.value.status == _ffi.PFAC_E_OVERFLOW and e.value.out_bytes == want.size
            g.sync()
            gb.check(payload_untouched=True, what="d_out after the overflow")
            go.check(payload_untouched=True, what="d_out_offsets after the overflow")
        n = g.gather_documents(case.n_docs, case.n_ids, case.n, out_cap=want.size, **args)
        g.sync()
        whole = gb.tensor[gb.front:].cpu().numpy()                 # the payload and the back guard behind it
        assert_gather(case, n, go.host().view(np.uint64), whole, fill=gb.fill, what=what)
        gb.check(what="d_out at exactly out_bytes")
        go.check(what="d_out_offsets at exactly n_ids + 1 entries")
        assert status_of(lambda: g.gathered_to_host(n)) == _ffi.PFAC_E_STATE          # both went to the caller's buffers
        assert status_of(lambda: g.gathered_offsets_to_host(case.n_ids)) == _ffi.PFAC_E_STATE
        seen.append(whole[:n].copy())
        if pad == PADS[-1]:
            n = g.gather_documents(case.n_docs, case.n_ids, case.n, d_input=d_in, d_ids=d_ids)
            assert_gather(case, n, g.gathered_offsets_to_host(case.n_ids), g.gathered_to_host(n), what=what + " slot-owned")
        del keep
    assert np.array_equal(seen[0], seen[1]), "the bytes behind n_bytes changed the output"


def small_case():
    return next(c for c in CASES if c.name == "ids_all")


def test_gather_fetch_windows(g):
    case = small_case()
    want, want_off = gather_ref(case.data, case.offsets, case.ids)
    place_input(g, case, 0, "slot")
    g.set_doc_offsets(case.offsets)
    n = g.gather_documents(case.n_docs, case.n_ids, case.n, d_ids=device_u64(case.ids))
    assert n == want.size
    for first, k in ((0, n), (1, n - 1), (n - 1, 1), (n // 2, 17), (5, 0), (n, 0)):
        assert np.array_equal(g.gathered_to_host(k, first=first), want[first:first + k]), (first, k)
    assert status_of(lambda: g.gathered_to_host(1, first=n)) == _ffi.PFAC_E_ARG
    assert status_of(lambda: g.gathered_to_host(0, first=n + 1)) == _ffi.PFAC_E_ARG
    assert status_of(lambda: g.gathered_to_host(n + 1)) == _ffi.PFAC_E_ARG
    np.testing.assert_array_equal(g.gathered_offsets_to_host(case.n_ids), want_off)     # the windows discarded nothing


def test_gather_errors_leave_the_buffers_untouched_and_discard_the_slot_result(g):
    case = small_case()
    off = case.offsets
    n_docs, n_ids = case.n_docs, case.n_ids
    want, _ = gather_ref(case.data, off, case.ids)
    storage = case.storage(0)
    place_input(g, case, 0, "slot")
    keep, ptr = device_bytes(storage, SHIFT)
    g.set_doc_offsets(off)
    d_ids = device_u64(case.ids)
    gb, go = guards(want.size, n_ids)
    out = dict(d_out=gb.ptr, out_cap=want.size, d_out_offsets=go.ptr)

    k = next(d for d in range(1, n_docs - 1) if off[d] > 0 and off[d + 1] > off[d])
    descending = off.copy()
    descending[k + 1] = off[k] - np.uint64(1)                     # document k ends in front of its start; no other one does
    assert (np.diff(np.delete(descending.astype(np.int64), k + 1)) >= 0).all()
    d_desc = device_u64(descending)
    past = case.ids.copy()
    past[3] = n_docs
    d_past = device_u64(past)
    others = np.array([d for d in range(n_docs) if d != k], dtype=np.uint64)
    d_others = device_u64(others)

    def gather(n_docs=n_docs, n_ids=n_ids, n_bytes=case.n, **kw):
        return g.gather_documents(n_docs, n_ids, n_bytes, **{**dict(d_ids=d_ids), **out, **kw})

    errors = [
        ("an id equal to n_docs", lambda: gather(d_ids=d_past), _ffi.PFAC_E_ARG),
        ("offsets that descend at a selected document", lambda: gather(d_doc_offsets=d_desc), _ffi.PFAC_E_ARG),
        ("off[id + 1] > n_bytes", lambda: gather(n_bytes=case.n - 1), _ffi.PFAC_E_ARG),
        ("a misaligned d_input", lambda: gather(d_input=ptr + 8), _ffi.PFAC_E_ARG),
        ("a misaligned d_out", lambda: gather(d_out=gb.ptr + 8), _ffi.PFAC_E_ARG),
        ("a misaligned d_ids", lambda: gather(d_ids=int(d_ids.data_ptr()) + 4), _ffi.PFAC_E_ARG),
        ("a misaligned d_out_offsets", lambda: gather(d_out_offsets=go.ptr + 4), _ffi.PFAC_E_ARG),
        ("n_bytes past the slot's input", lambda: gather(n_bytes=1 << 31), _ffi.PFAC_E_ARG),
        ("n_bytes above 2^32", lambda: gather(n_bytes=(1 << 32) + 1, d_input=ptr), _ffi.PFAC_E_ARG),
        ("NULL offsets with a foreign n_docs", lambda: gather(n_docs=n_docs + 1), _ffi.PFAC_E_STATE),
        ("one byte short", lambda: gather(out_cap=want.size - 1), _ffi.PFAC_E_OVERFLOW),
    ]
    for name, call, status in errors:
        n = g.gather_documents(n_docs, n_ids, case.n, d_ids=d_ids)              # a slot-owned result to lose
        assert bytes(g.gathered_to_host(n)) == bytes(want)
        assert status_of(call) == status, name
        g.sync()
        gb.check(payload_untouched=True, what=f"d_out after {name}")
        go.check(payload_untouched=True, what=f"d_out_offsets after {name}")
        assert status_of(lambda: g.gathered_to_host(0)) == _ffi.PFAC_E_STATE, name          # the failed call discarded it
        assert status_of(lambda: g.gathered_offsets_to_host(n_ids)) == _ffi.PFAC_E_STATE, name
    # the same descending offsets at a document nobody selected: success
    got = g.gather_documents(n_docs, others.size, case.n, d_doc_offsets=d_desc, d_ids=d_others)
    rest, rest_off = gather_ref(case.data, descending, others)
    assert got == rest.size and bytes(g.gathered_to_host(got)) == bytes(rest)
    np.testing.assert_array_equal(g.gathered_offsets_to_host(others.size), rest_off)
    del keep


def test_gather_null_ids_are_the_last_matching_calls(g):
    case = small_case()
    place_input(g, case, 0, "slot")
    g.set_doc_offsets(case.offsets)
    with GpuMatcher(0, 1) as fresh:                                # no matching call yet
        fresh.reserve(0, case.storage(0).size)
        fresh.set_doc_offsets(case.offsets)
        assert status_of(lambda: fresh.gather_documents(case.n_docs, 0, case.n)) == _ffi.PFAC_E_STATE
        assert status_of(lambda: fresh.gathered_to_host(0)) == _ffi.PFAC_E_STATE
    first = doc_first_case("runs", case.n_docs)
    d_first = device_u64(first)
    for before, after, want_ids in ((0, 0, matching_ids(first)), (1, 2, context_ids(first, 1, 2))):
        k = g.matching_documents(case.n_docs, d_doc_first=d_first, before=before, after=after)
        assert k == want_ids.size and 0 < k < case.n_docs
        assert status_of(lambda: g.gather_documents(case.n_docs, k + 1, case.n)) == _ffi.PFAC_E_ARG     # not that call's count
        n = g.gather_documents(case.n_docs, k, case.n)
        want, want_off = gather_ref(case.data, case.offsets, want_ids)
        assert n == want.size and bytes(g.gathered_to_host(n)) == bytes(want)
        np.testing.assert_array_equal(g.gathered_offsets_to_host(k), want_off)
    ids_out = GuardedBuffer(int(matching_ids(first).size) * 8)
    torch.cuda.synchronize()
    k = g.matching_documents(case.n_docs, d_doc_first=d_first, d_out=ids_out.ptr, out_cap=matching_ids(first).size)
    assert status_of(lambda: g.gather_documents(case.n_docs, k, case.n)) == _ffi.PFAC_E_STATE           # the ids went to the caller


# ---------------------------------------------------------------------------
# context lines

def context_call(g, n_docs, before, after, d_first, d_out=None, out_cap=0, flags=0):
    """pfac_documents_matching_context itself (GpuMatcher.matching_documents takes the plain call for 0, 0)."""
    n = C.c_uint64(0)
    rc = g._L.pfac_documents_matching_context(g._ctx, 0, int(d_first.data_ptr()) if d_first is not None else None, n_docs,
                                              before, after, flags, d_out, out_cap, C.byref(n))
    return rc, n.value


@pytest.mark.parametrize("kind", MATCH_KINDS)
@pytest.mark.parametrize("n_docs", MATCH_DOCS)
def test_context_equals_reference(g, n_docs, kind):
    first = doc_first_case(kind, n_docs)
    d_first = device_u64(first)
    for before, after in context_windows(n_docs):
        want = context_ids(first, before, after)
        what = f"{kind} n_docs={n_docs}"
        gb = GuardedBuffer(want.size * 8)
        torch.cuda.synchronize()
        if want.size:                                              # one entry short: the exact count, nothing written
            rc, n = context_call(g, n_docs, before, after, d_first, gb.ptr, want.size - 1)
            assert rc == _ffi.PFAC_E_OVERFLOW and n == want.size, (what, before, after)
            g.sync()
            gb.check(payload_untouched=True, what="d_ids_out after the overflow")
        rc, n = context_call(g, n_docs, before, after, d_first, gb.ptr, want.size)
        assert rc == 0, (what, before, after)
        g.sync()
        assert_context(gb.host().view(np.uint64), n, first, before, after, what + " (caller's buffer)")
        gb.check(what="d_ids_out at exact capacity")
        assert status_of(lambda: g.matching_documents_to_host(n)) == _ffi.PFAC_E_STATE     # it went to the caller's buffer
        rc, n = context_call(g, n_docs, before, after, d_first)
        assert rc == 0
        ids = g.matching_documents_to_host(n)
        assert_context(ids, n, first, before, after, what + " (slot-owned)")
        if (before, after) == (0, 0):
            k = g.matching_documents(n_docs, d_doc_first=d_first)
            assert_matching(ids, k, first, False, what + ": context 0, 0 against the plain call")
            assert np.array_equal(g.matching_documents_to_host(k), ids)
    if n_docs:                                                     # the keyword arguments take the context call
        k = g.matching_documents(n_docs, d_doc_first=d_first, before=2, after=3)
        assert_context(g.matching_documents_to_host(k), k, first, 2, 3, "matching_documents(before=2, after=3)")


def test_context_arguments_and_the_shared_result(g):
    n_docs = 4097
    first = doc_first_case("runs", n_docs)
    d_first = device_u64(first)
    assert context_call(g, n_docs, 1, 1, d_first, flags=_ffi.PFAC_DOCS_INVERT) == (_ffi.PFAC_E_ARG, 0)
    assert context_call(g, n_docs, 1, 1, d_first, flags=2)[0] == _ffi.PFAC_E_ARG
    assert context_call(g, n_docs, 1, 1, d_first, d_out=12, out_cap=1 << 20)[0] == _ffi.PFAC_E_ARG
    assert context_call(g, 1 << 32, 1, 1, d_first)[0] == _ffi.PFAC_E_ARG
    with pytest.raises(ValueError):
        g.matching_documents(n_docs, invert=True, d_doc_first=d_first, before=1)
    # one slot-owned id buffer: a call of either discards the other's result, even a call that fails
    k = g.matching_documents(n_docs, d_doc_first=d_first)
    assert_matching(g.matching_documents_to_host(k), k, first, False, "the plain call")
    assert context_call(g, n_docs, 1, 1, d_first, flags=_ffi.PFAC_DOCS_INVERT)[0] == _ffi.PFAC_E_ARG
    assert status_of(lambda: g.matching_documents_to_host(k)) == _ffi.PFAC_E_STATE
    rc, n = context_call(g, n_docs, 1, 1, d_first)
    assert rc == 0 and n > k
    assert_context(g.matching_documents_to_host(n), n, first, 1, 1, "the context call")
    assert status_of(lambda: g.matching_documents(n_docs, d_doc_first=int(d_first.data_ptr()) + 4)) == _ffi.PFAC_E_ARG
    assert status_of(lambda: g.matching_documents_to_host(n)) == _ffi.PFAC_E_STATE
    rc, n = context_call(g, n_docs, 1, 1, d_first)
    k = g.matching_documents(n_docs, d_doc_first=d_first)         # a successful plain call replaces the context call's ids
    assert_matching(g.matching_documents_to_host(k), k, first, False, "the plain call after the context call")


# ---------------------------------------------------------------------------
# end to end: grep

def make_text(para):
    """A few KiB of lines of words, most of them without the letter of tests/golden/data/experimentpattern (a, aa, aaa,
    aaaa): empty lines, the word "a" on its own in some, the last line unterminated."""
    words = sorted(set(re.findall(rb"[A-Za-z]+", para)))
    plain = [w for w in words if b"a" not in w]
    hits = [w for w in words if b"a" in w and w != b"a"]
    hits += [b"a"] * (len(hits) // 2)
    rng = np.random.default_rng(14)
    lines = []
    for k in range(260):
        line = [plain[int(i)] for i in rng.integers(0, len(plain), int(rng.integers(0, 9)))]
        if rng.random() < 0.12:
            line.insert(int(rng.integers(0, len(line) + 1)), hits[int(rng.integers(0, len(hits)))])
        lines.append(b" ".join(line))
    data = b"\n".join(lines + [b"the end"])
    assert 4096 < len(data) < 16384 and b"\n\n" in data
    return data


@pytest.fixture(scope="module")
def text_case(resolve):
    data = make_text(open(resolve("paragraph402"), "rb").read())
    table = PfacTable.from_file(resolve("experimentpattern"), 256)
    patterns = open(resolve("experimentpattern"), "rb").read().split()
    return {"data": data, "table": table, "patterns": patterns}


def grep_ref(data, patterns, invert=False, before=0, after=0, whole_words=False):
    """(out, out_offsets, ids): grep -F in Python -- `before` lines in front of a matching line, `after` behind it."""
    lines = data.splitlines(keepends=True)
    if whole_words:
        word = re.compile(rb"(?<![0-9A-Za-z_])(?:" + b"|".join(re.escape(p) for p in patterns) + rb")(?![0-9A-Za-z_])")
        hit = [word.search(line) is not None for line in lines]
    else:
        hit = [any(p in line for p in patterns) for line in lines]
    keep = [h != invert for h in hit]
    sel = [d for d in range(len(lines)) if any(keep[max(d - after, 0):d + before + 1])]
    off = np.concatenate([[0], np.cumsum([len(lines[d]) for d in sel])]).astype(np.uint64)
    return b"".join(lines[d] for d in sel), off, sel, len(lines)


@pytest.mark.parametrize("whole_words", [False, True], ids=["substrings", "whole_words"])
@pytest.mark.parametrize("context", [(0, 0), (1, 2)], ids=["plain", "B1_A2"])
@pytest.mark.parametrize("invert", [False, True], ids=["grep", "grep_v"])
def test_grep_lines_on_text(text_case, invert, context, whole_words):
    c = text_case
    before, after = context
    with GpuMatcher(0, 1) as m:
        m.load_table(c["table"])
        if invert and (before or after):
            with pytest.raises(ValueError):
                m.grep_lines(c["data"], invert=True, before=before, after=after, whole_words=whole_words)
            return
        want, want_off, want_ids, n_lines = grep_ref(c["data"], c["patterns"], invert, before, after, whole_words)
        assert 0 < len(want_ids) < n_lines                         # the reference selects some lines, not all
        out, out_off, ids = m.grep_lines(c["data"], invert=invert, before=before, after=after, whole_words=whole_words)
    assert ids.tolist() == want_ids
    np.testing.assert_array_equal(out_off, want_off)
    assert bytes(out) == want


def test_gather_by_hand_reads_no_scan_state(text_case):
    """split, segment, matching and gather with the slot's NULL defaults, a second scan of other bytes' worth between
    them: the gather needs the input, the offsets and the ids, nothing of a scan."""
    c = text_case
    data = np.frombuffer(c["data"], dtype=np.uint8)
    want, want_off, want_ids, _ = grep_ref(c["data"], c["patterns"])
    with GpuMatcher(0, 1) as m:
        m.load_table(c["table"])
        m.set_final_lengths(c["table"].final_lengths())
        m.reserve(0, data.size, 1 << 16)
        m.h2d(data)
        m.scan_resident(data.size, data.size)
        n_docs, _ = m.split_documents(data.size)
        m.segment_records(n_docs)
        k = m.matching_documents(n_docs)
        m.scan_resident(100, 100)                                  # another scan on the slot: new records, new tile index
        n = m.gather_documents(n_docs, k, data.size)
        m.scan_resident(data.size // 2, data.size // 2)            # ... and one behind the gather, before its fetches
        assert m.matching_documents_to_host(k).tolist() == want_ids
        np.testing.assert_array_equal(m.gathered_offsets_to_host(k), want_off)
        assert bytes(m.gathered_to_host(n)) == want
