"""Pass outputs past 2^32 bytes (run with -m gpu on an MI355X): the gather, the find-and-replace, the per-document
find-and-replace and the text emitter each make between 2^32 + 2^20 and 1.25 x 2^32 bytes from the smallest input that
does, and every output byte, every output offset and fetches on both sides of 2^32 are compared with tests/bigout.py,
whose tables come from the CPU references and the CPU oracle and whose cases tests/test_bigout_ref.py pins (a run
crosses 2^32; the bytes behind 2^32 differ from the first ones, so a store whose offset wraps shows).  Caller-owned
outputs are guard-banded at exact capacity.  With it the gather at the six output sizes around 64 MiB where the write
grid goes from one window per wave to four.  Integer work: bit-exact.  No expectation comes from the device.

Seconds per test on an MI355X in one run: the gather 2.6, the replace 0.9 and 0.8, the per-document replace 0.9, the
text 6.0, each of the six gathers around 64 MiB under 0.005; test_gpu_replace.py::test_one_gib_experimentpattern_text in
the same run: 14.0.

With one store offset of pfac_ga_write_kernel truncated to 32 bits test_gather_past_4g fails with "fetch of 4096 bytes at
4294965248: byte 4294967296 differs (2041 do)"; with the group's text offset of pfac_text_format_kernel truncated
test_text_past_4g fails with "text bytes [134217728, 201326592) hold 1663931 newlines, want 1703021; line 3529534 ends at
139082328, want 139082357" (the wrapped lines land on the text's low part, which the walk meets first)."""
import numpy as np
import pytest
import torch

import bigout
from bigout import CHUNK, G4, BigGather, BigReplace, BigText, EdgeGather, assert_device_equals, window
from heapguard import GuardedBuffer
from orc import match_checksum
from phfpfac_amd import GpuMatcher, PfacError, PfacTable
from phfpfac_amd import _ffi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def upload(host, pad=4096):
    """`host` on the device, `pad` zero bytes behind it."""
    t = torch.zeros(host.size + pad, dtype=torch.uint8, device=DEV)
    t[:host.size] = torch.from_numpy(host)
    torch.cuda.synchronize()                # (a slot's stream is not torch's)
    return t


def device_u64(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(DEV)
    torch.cuda.synchronize()
    return t


def windows(out_bytes):
    """The three fetches of every big output: across 2^32, behind it, the last 4096 bytes."""
    return [(G4 - 2048, 4096), (G4 + 4096, 4096), (out_bytes - 4096, 4096)]


def assert_fetches(seg, source, fetch, out_bytes, what):
    for first, n in windows(out_bytes):
        got = fetch(first, n)
        want = window(seg, source, first, first + n)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: fetch of {n} bytes at {first}: byte {first + int(bad[0])} differs ({bad.size} do)"


def assert_offsets(got, want, what):
    got, want = np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64)
    assert got.size == want.size, f"{what}: {got.size} output offsets, want {want.size}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: out_off[{int(bad[0])}] is {int(got[bad[0]])}, want {int(want[bad[0]])} ({bad.size} differ)"


def assert_overflow_writes_nothing(call, out_bytes, guards, what):
    """`call` with a capacity one byte short: PFAC_E_OVERFLOW with the exact length, the guarded buffers as they were."""
    with pytest.raises(PfacError) as e:
        call()
    assert e.value.status == _ffi.PFAC_E_OVERFLOW and e.value.out_bytes == out_bytes, what
    torch.cuda.synchronize()
    for gb in guards:
        gb.check(what=f"{what} after the overflow")
        assert int((gb.payload() != gb.fill).sum()) == 0, f"{what}: the overflow wrote into the payload"


def free(*segs):
    for s in segs:
        s.release()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# the gather

def test_gather_past_4g():
    c = BigGather()
    seg, total = c.seg, c.seg.total
    d_in, d_ids, d_off = upload(c.data), device_u64(c.ids), device_u64(c.offsets)
    args = dict(d_input=d_in, d_doc_offsets=d_off, d_ids=d_ids)
    with GpuMatcher(0, 1) as g:
        n = g.gather_documents(c.n_docs, c.n_ids, c.n, **args)
        assert n == total
        assert_offsets(g.gathered_offsets_to_host(c.n_ids), seg.out_off, "slot-owned")
        assert_fetches(seg, c.data, lambda first, k: g.gathered_to_host(k, first=first), n, "slot-owned gather")
        assert_device_equals(seg, d_in, lambda first, k: g.gathered_to_host(k, first=first), n, what="slot-owned gather")
        gb, go = GuardedBuffer(total), GuardedBuffer((c.n_ids + 1) * 8, fill=0x3C)
        out = dict(d_out=gb.ptr, d_out_offsets=go.ptr)
        assert_overflow_writes_nothing(lambda: g.gather_documents(c.n_docs, c.n_ids, c.n, out_cap=total - 1, **args, **out),
                                       total, (gb, go), "gather into a caller's buffer")
        n = g.gather_documents(c.n_docs, c.n_ids, c.n, out_cap=total, **args, **out)
        g.sync()
        assert_offsets(go.host().view(np.uint64), seg.out_off, "caller's buffer")
        assert_device_equals(seg, d_in, gb.payload(), n, what="gather into a caller's buffer")
        gb.check(what="d_out at exactly out_bytes")
        go.check(what="d_out_offsets at exactly n_ids + 1 entries")
        del gb, go
    del d_in, d_ids, d_off
    free(seg)


# ---------------------------------------------------------------------------
# the write grid where it goes from one window per wave to four

@pytest.fixture(scope="module")
def edge():
    e = EdgeGather()
    e.d_in, e.d_ids = upload(e.data), device_u64(e.ids)
    with GpuMatcher(0, 1) as g:
        e.g = g
        yield e
    del e.d_in, e.d_ids
    torch.cuda.empty_cache()


@pytest.mark.parametrize("out_bytes", EdgeGather.SIZES, ids=lambda s: f"64MiB{s - (64 << 20):+d}")
def test_gather_at_the_four_window_edge(edge, out_bytes):
    e, g = edge, edge.g
    off = e.offsets(out_bytes)
    seg = bigout.gather_segments(off, e.ids)
    assert seg.total == out_bytes
    d_off = device_u64(off)
    gb, go = GuardedBuffer(out_bytes), GuardedBuffer((e.n_ids + 1) * 8, fill=0x3C)
    n = g.gather_documents(e.n_docs, e.n_ids, e.n, d_input=e.d_in, d_doc_offsets=d_off, d_ids=e.d_ids, d_out=gb.ptr,
                           out_cap=out_bytes, d_out_offsets=go.ptr)
    g.sync()
    assert_offsets(go.host().view(np.uint64), seg.out_off, "caller's buffer")
    assert_device_equals(seg, e.d_in, gb.payload(), n, what=f"gather of {out_bytes} bytes")
    gb.check(what="d_out at exactly out_bytes")
    go.check(what="d_out_offsets at exactly n_ids + 1 entries")
    seg.release()


# ---------------------------------------------------------------------------
# the replace

@pytest.fixture(scope="module")
def big_replace(tmp_path_factory):
    return BigReplace(tmp_path_factory.mktemp("bigreplace"))


def replace_matcher(r):
    table = PfacTable.from_file(r.path, 256)
    g = GpuMatcher(0, 1)
    g.load_table(table)
    g.set_final_lengths(table.final_lengths())
    g.set_replacements(r.reps)
    g.reserve(0, 0, r.n)
    return g


@pytest.mark.parametrize("config", ["whole", "halo"])
def test_replace_past_4g(big_replace, config):
    r = big_replace
    c = r.configs[config]
    seg, total = c["seg"], c["seg"].total
    buf, d_src = upload(r.data), torch.from_numpy(r.source).to(DEV)
    torch.cuda.synchronize()
    with replace_matcher(r) as g:
        assert g.scan_resident(c["n_owned"], r.n, d_input=buf) == int((r.pos < c["n_owned"]).sum())
        n_sel, ex = g.select_leftmost_longest(c["entry"])
        assert (n_sel, ex) == (c["picks"][0].size, c["exit"])
        n = g.replace_selection(d_input=buf)
        assert n == total
        assert_fetches(seg, r.source, lambda first, k: g.replacement_to_host(k, first=first), n, "slot-owned replace")
        assert_device_equals(seg, d_src, lambda first, k: g.replacement_to_host(k, first=first), n, what=f"slot-owned replace ({config})")
        gb = GuardedBuffer(total)
        g.select_leftmost_longest(c["entry"])
        assert_overflow_writes_nothing(lambda: g.replace_selection(d_input=buf, d_out=gb.ptr, out_cap=total - 1), total, (gb,),
                                       "replace into a caller's buffer")
        g.select_leftmost_longest(c["entry"])
        n = g.replace_selection(d_input=buf, d_out=gb.ptr, out_cap=total)
        g.sync()
        assert_device_equals(seg, d_src, gb.payload(), n, what=f"replace into a caller's buffer ({config})")
        gb.check(what="d_out at exactly out_bytes")
        del gb
    del buf, d_src
    free(seg)


def test_doc_replace_past_4g(big_replace):
    r = big_replace
    seg, doc_out = r.per_document()
    total, n_docs = seg.total, r.doc_off.size - 1
    assert int((doc_out > G4).sum()) >= 5
    buf, d_src = upload(r.data), torch.from_numpy(r.source).to(DEV)
    torch.cuda.synchronize()
    with replace_matcher(r) as g:
        g.scan_resident(r.n, r.n, d_input=buf)
        g.set_doc_offsets(r.doc_off)
        g.select_leftmost_longest_documents(n_docs)
        n = g.replace_selection_documents(d_input=buf)
        assert n == total
        assert_offsets(g.replacement_doc_offsets_to_host(n_docs), doc_out, "slot-owned")
        assert_fetches(seg, r.source, lambda first, k: g.replacement_to_host(k, first=first), n, "slot-owned per-document replace")
        assert_device_equals(seg, d_src, lambda first, k: g.replacement_to_host(k, first=first), n, what="slot-owned per-document replace")
        gb, go = GuardedBuffer(total), GuardedBuffer((n_docs + 1) * 8, fill=0x3C)
        g.select_leftmost_longest_documents(n_docs)
        n = g.replace_selection_documents(d_input=buf, d_out=gb.ptr, out_cap=total, d_out_offsets=go.ptr)
        g.sync()
        assert_offsets(go.host().view(np.uint64), doc_out, "caller's buffer")
        assert_device_equals(seg, d_src, gb.payload(), n, what="per-document replace into a caller's buffer")
        gb.check(what="d_out at exactly out_bytes")
        go.check(what="d_out_offsets at exactly n_docs + 1 entries")
        del gb, go
    del buf, d_src
    free(seg)


# ---------------------------------------------------------------------------
# the text

def assert_newlines(fetch, nbytes, ends, what):
    """Over the whole text, on the device: the indices of the newlines are `ends` - 1, for every line."""
    d_last = torch.from_numpy(ends - 1).to(DEV)
    k = 0
    for a in range(0, nbytes, CHUNK):
        b = min(a + CHUNK, nbytes)
        chunk = torch.from_numpy(np.frombuffer(fetch(a, b - a), dtype=np.uint8).copy()).to(DEV)
        nl = torch.nonzero(chunk == 10).flatten() + a
        kb = int(np.searchsorted(ends, b, side="right"))           # lines that end at or before b
        want = d_last[k:kb]
        if nl.numel() != want.numel() or not torch.equal(nl, want):
            m = min(nl.numel(), want.numel())
            bad = torch.nonzero(nl[:m] != want[:m]).flatten()
            at = int(bad[0]) if bad.numel() else m
            raise AssertionError(f"{what}: text bytes [{a}, {b}) hold {nl.numel()} newlines, want {want.numel()}; line {k + at} ends at "
                                 f"{int(nl[at]) if at < nl.numel() else None}, want {int(want[at]) if at < want.numel() else None}")
        k = kb
    assert k == ends.size, f"{what}: {k} lines, want {ends.size}"


def expected_text(t, pos, ids, ends, first, n):
    """Bytes [first, first + n) of the text, formatted on the host from the lines that overlap them."""
    k0 = int(np.searchsorted(ends, first, side="right"))           # the line that holds byte `first`
    k1 = int(np.searchsorted(ends, first + n, side="left")) + 1
    start = int(ends[k0 - 1]) if k0 else 0
    return t.format(pos[k0:k1], ids[k0:k1])[first - start:first - start + n]


def check_text(g, t, buf, hi, rec_bytes, what):
    """Scan of the positions [0, hi) and its text against the run lengths; -> the text's first MiB."""
    pos, ids, ends = t.all_line_ends(hi)
    nbytes = int(ends[-1])
    assert nbytes == t.text_bytes(hi)
    g.reserve(0, 0, pos.size + pos.size // 8 + 65536)
    n = g.scan_resident(hi, hi, d_input=buf)
    assert g.scan_format()[0] == rec_bytes, what
    assert n == pos.size, f"{what}: {n} records, want {pos.size}"
    assert g.checksum(n, base=t.base) == match_checksum(t.base + pos, ids), f"{what}: pfac_records_checksum"
    assert g.emit_text_device(t.base) == nbytes, what
    fetch = lambda first, k: g.text_to_host(k, first=first)      # noqa: E731
    assert_newlines(fetch, nbytes, ends, what)
    mib = 1 << 20
    spans = [(0, mib), (nbytes - mib, mib)] + ([(G4 - (mib >> 1), mib)] if nbytes > G4 + mib else [])
    for first, k in spans:
        got, want = fetch(first, k), expected_text(t, pos, ids, ends, first, k)
        assert len(got) == len(want) == k
        if got != want:
            at = next(i for i in range(k) if got[i] != want[i])
            raise AssertionError(f"{what}: text byte {first + at} differs: {got[max(at - 40, 0):at + 40]!r}, want {want[max(at - 40, 0):at + 40]!r}")
    return nbytes, fetch(0, mib)


def test_text_past_4g(tmp_path, monkeypatch):
    t = BigText(tmp_path)
    t.assert_oracle_agrees()
    table = PfacTable.from_file(t.path, 256)
    assert table.num_final == 16
    buf = upload(t.data)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        nbytes, head = check_text(g, t, buf, t.n, 2, "2-byte records")
    assert bigout.OUT_MIN <= nbytes <= bigout.OUT_MAX
    torch.cuda.empty_cache()
    # the 4-byte form of the same records on a prefix whose text stays under 2^32
    monkeypatch.setenv("PFAC_REC_BYTES", "4")
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        nq, head4 = check_text(g, t, buf, t.quarter(), 4, "4-byte records, a quarter of the input")
    assert nq < G4 and head4 == head
    del buf
    torch.cuda.empty_cache()
