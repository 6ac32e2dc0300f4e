"""Document offsets cut on the GPU and the documents that matched (run with -m gpu on an MI355X):
pfac_slot_doc_offsets_split / pfac_slot_doc_offsets_d2h against tests/splitref.py (the rule of include/pfac.h in numpy,
pinned to a bytes.split form by tests/test_split_ref.py), their composition with the document passes against the CPU
oracle run per document on the HOST-derived offsets (docref, wordref, llref, docreplref), and pfac_documents_matching /
pfac_documents_matching_d2h against splitref.matching_ids with guard bands around the caller's buffer.  Integer work:
bit-exact.  No expectation comes from the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import wordref
from docref import oracle_per_doc
from docreplref import per_doc
from heapguard import GuardedBuffer
from llref import line_lengths
from orc import Oracle
from phfpfac_amd import GpuMatcher, PfacError, PfacTable
from phfpfac_amd import _ffi
from replref import rep_table
from splitref import (MATCH_DOCS, MATCH_KINDS, TILE, all_split_cases, assert_matching, assert_split, doc_first_case, matching_ids,
                      split_offsets)

pytestmark = pytest.mark.gpu

CASES = all_split_cases()
SHIFT = 48                                  # a caller's input starts here in its allocation: 16-B aligned, not 256


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


def split_case(g, case, pad, source):
    storage = case.storage(pad)
    keep = None
    if source == "slot":
        g.reserve(0, storage.size)
        g.h2d(storage)
        n_docs, tail = g.split_documents(case.n, case.delim)
    else:
        keep, ptr = device_bytes(storage, SHIFT)
        assert ptr % 16 == 0 and ptr % 256 != 0
        n_docs, tail = g.split_documents(case.n, case.delim, d_input=ptr)
    assert_split(case, pad, n_docs, tail, lambda first, n: g.doc_offsets_to_host(n_docs, first=first, n=n))
    del keep


# ---------------------------------------------------------------------------
# the split

@pytest.mark.parametrize("source", ["slot", "caller"])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_split_equals_reference(g, case, source):
    """Every length, delimiter, placement and adversarial case, from the slot's input and from a caller's buffer at a
    16-B aligned offset of its allocation; the bytes from n_bytes to the next tile hold the delimiter, then its
    complement: n_docs, tail_start and every offset equal the reference both times."""
    for pad in (case.delim, case.delim ^ 0xFF):
        split_case(g, case, pad, source)


def test_offsets_of_either_call_are_fetched(g):
    off = np.array([0, 5, 5, 9, 20], dtype=np.uint64)
    g.set_doc_offsets(off)
    np.testing.assert_array_equal(g.doc_offsets_to_host(4), off)
    np.testing.assert_array_equal(g.doc_offsets_to_host(4, first=2, n=2), off[2:4])
    assert g.doc_offsets_to_host(4, first=5, n=0).size == 0
    assert status_of(lambda: g.doc_offsets_to_host(4, first=4, n=2)) == _ffi.PFAC_E_ARG
    assert status_of(lambda: g.doc_offsets_to_host(4, first=6, n=0)) == _ffi.PFAC_E_ARG
    with GpuMatcher(0, 1) as fresh:
        assert status_of(lambda: fresh.doc_offsets_to_host(0)) == _ffi.PFAC_E_STATE
        assert fresh.split_documents(0) == (0, 0)              # no bytes, no buffer: the single offset 0
        assert fresh.doc_offsets_to_host(0).tolist() == [0]


def test_errors_leave_the_offsets_as_they_were(g):
    case = next(c for c in CASES if c.name == "len4097_d0a")
    storage = case.storage(case.delim)
    g.reserve(0, storage.size)
    g.h2d(storage)
    n_docs, _ = g.split_documents(case.n, case.delim)
    want = split_offsets(case.data, case.delim)[0]
    keep, ptr = device_bytes(storage, SHIFT)
    bad = [lambda: g.split_documents(case.n, -1), lambda: g.split_documents(case.n, 256),
           lambda: g.split_documents(case.n, 10, d_input=ptr + 8), lambda: g.split_documents(1 << 31, 10),
           lambda: g.split_documents((1 << 32) + 1, 10, d_input=ptr), lambda: g.split_documents(case.n, 10, slot=5)]
    for k, call in enumerate(bad):
        assert status_of(call) == _ffi.PFAC_E_ARG, k
        np.testing.assert_array_equal(g.doc_offsets_to_host(n_docs), want)
    with pytest.raises(ValueError):
        g.split_documents(case.n, b"\r\n")


# ---------------------------------------------------------------------------
# composition with the document passes

PATTERNS = [b"the", b"th", b"he", b"England", b"cricket", b"in", b"was", b"a", b"World Cup", b"of "]


@pytest.fixture(scope="module")
def lines_case(tmp_path_factory, resolve):
    """Three tiles and a ragged tail of text lines: empty ones, one longer than a tile, the last one unterminated."""
    path = tmp_path_factory.mktemp("split") / "p.pat"
    path.write_bytes(b"".join(p + b"\n" for p in PATTERNS))
    para = open(resolve("paragraph402"), "rb").read().replace(b"\n", b" ")
    words = para.split(b" ")
    rng = np.random.default_rng(5)
    lines, target = [], 3 * TILE + 321
    while sum(len(x) + 1 for x in lines) < target + 50:
        k = len(lines)
        if k in (0, 3, 4, 17):
            lines.append(b"")
        elif k == 9:
            lines.append((para * 12)[:TILE + 404])
        else:
            at = int(rng.integers(0, len(words) - 40))
            lines.append(b" ".join(words[at:at + int(rng.integers(1, 40))]))
    buf = np.frombuffer(b"\n".join(lines)[:target], dtype=np.uint8).copy()
    off, n_docs, tail = split_offsets(buf, 10)
    sizes = np.diff(off.astype(np.int64))
    assert buf.size == target and 24 <= n_docs <= 200 and (sizes == 1).sum() >= 4 and sizes.max() > TILE and tail < buf.size
    path = str(path)
    table = PfacTable.from_file(path, 256)
    ll = line_lengths(path)
    reps = {i: bytes(np.random.default_rng(i).integers(65, 91, i % 7).astype(np.uint8)) for i in range(1, len(PATTERNS) + 1)}
    o = Oracle(path, 1, 1)
    yield {"path": path, "table": table, "buf": buf, "off": off, "n_docs": n_docs, "ll": ll, "reps": reps, "o": o}
    o.close()


def lines_matcher(c):
    m = GpuMatcher(0, 1)
    m.load_table(c["table"])
    m.set_replacements(c["reps"])
    return m


def scan_and_split(m, c):
    buf = c["buf"]
    m.set_final_lengths(c["table"].final_lengths())
    m.reserve(0, buf.size, 1 << 16)
    m.h2d(buf)
    m.scan_resident(buf.size, buf.size)
    n_docs, tail = m.split_documents(buf.size)
    assert n_docs == c["n_docs"] and tail == int(c["off"][-2])
    np.testing.assert_array_equal(m.doc_offsets_to_host(n_docs), c["off"])
    return n_docs


def assert_docs(table, first, rec, want):
    wfirst, wpos, wids = want
    np.testing.assert_array_equal(first, wfirst)
    assert rec.size == wpos.size
    np.testing.assert_array_equal(rec["pos"].astype(np.int64), wpos)
    np.testing.assert_array_equal(table.idmap[rec["state"]], wids)


def filtered_per_doc(c):
    """docref.oracle_per_doc with wordref's filter applied to every document on its own."""
    buf, off, ll, o = c["buf"], c["off"], c["ll"], c["o"]
    first, pos, ids = [0], [], []
    for a, b in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64)):
        doc = np.ascontiguousarray(buf[a:b])
        p, i = o.scan_spec(doc)
        keep = wordref.filter_words(doc, p, ll[i])
        pos.append(p[keep])
        ids.append(i[keep])
        first.append(first[-1] + int(keep.sum()))
    return np.array(first, np.uint64), np.concatenate(pos), np.concatenate(ids)


def test_split_then_segment(lines_case):
    c = lines_case
    want = oracle_per_doc(c["o"], c["buf"], c["off"])
    assert want[1].size > 100
    with lines_matcher(c) as m:
        n_docs = scan_and_split(m, c)
        kept = m.segment_records(n_docs)
        assert_docs(c["table"], *m.segment_to_host(kept, n_docs), want)
        first, rec, off = m.scan_lines(c["buf"])
        np.testing.assert_array_equal(off, c["off"])
        assert_docs(c["table"], first, rec, want)


def test_split_then_whole_word_filter_then_segment(lines_case):
    c = lines_case
    want = filtered_per_doc(c)
    plain = oracle_per_doc(c["o"], c["buf"], c["off"])
    assert 0 < want[1].size < plain[1].size                        # the filter drops some records, not all
    with lines_matcher(c) as m:
        n_docs = scan_and_split(m, c)
        m.filter_whole_words(n_docs=n_docs)
        kept = m.segment_records(n_docs)
        assert_docs(c["table"], *m.segment_to_host(kept, n_docs), want)
        first, rec, _ = m.scan_lines(c["buf"], whole_words=True)
        assert_docs(c["table"], first, rec, want)


def test_split_then_selection_and_replace(lines_case):
    c = lines_case
    wfirst, wpos, wids, wout_off, wout = per_doc(c["o"], c["buf"], c["off"], c["ll"], rep_table(c["reps"]))
    assert wpos.size > 50
    with lines_matcher(c) as m:
        n_docs = scan_and_split(m, c)
        n = m.select_leftmost_longest_documents(n_docs)
        first, rec = m.doc_selection_to_host(n, n_docs)
        doc = np.repeat(np.arange(n_docs), np.diff(first.astype(np.int64)))
        rec["pos"] -= c["off"][doc].astype(np.uint32)
        assert_docs(c["table"], first, rec, (wfirst, wpos, wids))
        nb = m.replace_selection_documents()
        np.testing.assert_array_equal(m.replacement_doc_offsets_to_host(n_docs), wout_off)
        assert bytes(m.replacement_to_host(nb)) == bytes(wout)
        # a split after the per-document selection: new offsets, the selection's are gone
        assert m.split_documents(c["buf"].size)[0] == n_docs
        assert status_of(lambda: m.replace_selection_documents()) == _ffi.PFAC_E_STATE
        first, rec, _ = m.select_lines(c["buf"])
        assert_docs(c["table"], first, rec, (wfirst, wpos, wids))
        out_off, out, off = m.replace_lines(c["buf"])
        np.testing.assert_array_equal(out_off, wout_off)
        np.testing.assert_array_equal(off, c["off"])
        assert bytes(out) == bytes(wout)


def test_split_between_two_scans_keeps_the_segment_result(lines_case):
    c = lines_case
    want = oracle_per_doc(c["o"], c["buf"], c["off"])
    with lines_matcher(c) as m:
        n_docs = scan_and_split(m, c)
        kept = m.segment_records(n_docs)
        m.scan_async(c["buf"].size)                               # a scan in flight, ...
        assert m.split_documents(c["buf"].size, b" ")[0] > n_docs     # ... a split of the same bytes at another delimiter, ...
        m.scan_finish()
        m.scan_resident(c["buf"].size, c["buf"].size)             # ... and a scan behind it
        assert_docs(c["table"], *m.segment_to_host(kept, n_docs), want)
        by_space, n_space, _ = split_offsets(c["buf"], 32)
        np.testing.assert_array_equal(m.doc_offsets_to_host(n_space), by_space)


# ---------------------------------------------------------------------------
# the documents that matched

def device_u64(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("invert", [False, True], ids=["matching", "inverted"])
@pytest.mark.parametrize("kind", MATCH_KINDS)
@pytest.mark.parametrize("n_docs", MATCH_DOCS)
def test_matching_documents_equal_reference(g, n_docs, kind, invert):
    first = doc_first_case(kind, n_docs)
    want = matching_ids(first, invert)
    what = f"{kind} n_docs={n_docs} invert={invert}"
    gb = GuardedBuffer(want.size * 8)
    d_first = device_u64(first)                                    # (synchronises: the guard's fill is done before the slot's stream writes)
    if want.size:                                                  # one entry short: the exact count, nothing written
        with pytest.raises(PfacError) as e:
            g.matching_documents(n_docs, invert, d_doc_first=d_first, d_out=gb.ptr, out_cap=want.size - 1)
        assert e.value.status == _ffi.PFAC_E_OVERFLOW and e.value.n_matching == want.size
        g.sync()
        gb.check(payload_untouched=True, what="d_ids_out after the overflow")
    n = g.matching_documents(n_docs, invert, d_doc_first=d_first, d_out=gb.ptr, out_cap=want.size)
    g.sync()
    assert_matching(gb.host().view(np.uint64), n, first, invert, what + " (caller's buffer)")
    gb.check(what="d_ids_out at exact capacity")
    assert status_of(lambda: g.matching_documents_to_host(n)) == _ffi.PFAC_E_STATE     # it went to the caller's buffer
    n = g.matching_documents(n_docs, invert, d_doc_first=d_first)
    assert_matching(g.matching_documents_to_host(n), n, first, invert, what + " (slot-owned)")


def test_matching_arguments_and_lifetime(lines_case):
    c = lines_case
    with lines_matcher(c) as m:
        L, ctx = m._L, m._ctx
        n = C.c_uint64(7)
        assert status_of(lambda: m.matching_documents(3)) == _ffi.PFAC_E_STATE                 # no segment result yet
        n_docs = scan_and_split(m, c)
        d_first = torch.zeros(n_docs + 1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        m.segment_records(n_docs, d_doc_first=d_first)
        assert status_of(lambda: m.matching_documents(n_docs)) == _ffi.PFAC_E_STATE            # doc_first went to the caller
        kept = m.segment_records(n_docs)
        assert status_of(lambda: m.matching_documents(n_docs + 1)) == _ffi.PFAC_E_ARG          # not that call's n_docs
        assert L.pfac_documents_matching(ctx, 0, None, n_docs, 2, None, 0, C.byref(n)) == _ffi.PFAC_E_ARG and n.value == 0
        assert L.pfac_documents_matching(ctx, 0, d_first.data_ptr() + 4, n_docs, 0, None, 0, C.byref(n)) == _ffi.PFAC_E_ARG
        assert L.pfac_documents_matching(ctx, 0, d_first.data_ptr(), n_docs, 0, 12, 1 << 20, C.byref(n)) == _ffi.PFAC_E_ARG
        assert L.pfac_documents_matching(ctx, 3, None, n_docs, 0, None, 0, C.byref(n)) == _ffi.PFAC_E_ARG
        first, _ = m.segment_to_host(kept, n_docs)
        want = matching_ids(first)
        assert 0 < want.size < n_docs                              # some lines match, not all
        # the slot's doc_first, the caller's doc_first of the segment pass and that of the per-document selection agree
        k = m.matching_documents(n_docs)
        assert_matching(m.matching_documents_to_host(k), k, first, False, "slot-owned doc_first")
        k2 = m.matching_documents(n_docs, d_doc_first=d_first)
        assert_matching(m.matching_documents_to_host(k2), k2, first, False, "caller's doc_first")
        m.select_leftmost_longest_documents(n_docs, d_doc_first=d_first)
        k3 = m.matching_documents(n_docs, invert=True, d_doc_first=d_first)
        assert_matching(m.matching_documents_to_host(k3), k3, first, True, "the selection's doc_first, inverted")
        assert m.matching_documents(0, d_doc_first=d_first) == 0 and m.matching_documents_to_host(0).size == 0
        # fetchable after a new scan; dropped by the next call, even one that fails
        k = m.matching_documents(n_docs)
        m.scan_resident(c["buf"].size, c["buf"].size)
        assert_matching(m.matching_documents_to_host(k), k, first, False, "after a new scan")
        assert L.pfac_documents_matching(ctx, 0, None, n_docs, 2, None, 0, C.byref(n)) == _ffi.PFAC_E_ARG
        assert status_of(lambda: m.matching_documents_to_host(k)) == _ffi.PFAC_E_STATE


@pytest.mark.parametrize("invert", [False, True], ids=["grep", "grep_v"])
def test_matching_lines_on_text(lines_case, invert):
    c = lines_case
    data = c["buf"].tobytes()
    lines = data.split(b"\n")
    lines = [x + b"\n" for x in lines[:-1]] + ([lines[-1]] if lines[-1] else [])
    hit = [any(p in line for p in PATTERNS) for line in lines]
    assert any(hit) and not all(hit)
    with lines_matcher(c) as m:
        ids, off = m.matching_lines(c["buf"], invert=invert)
    np.testing.assert_array_equal(off, c["off"])
    assert ids.tolist() == [d for d, h in enumerate(hit) if h != invert]
    assert [data[int(off[d]):int(off[d + 1])] for d in ids.tolist()] == [x for x, h in zip(lines, hit) if h != invert]
