"""Batches of documents (run with -m gpu on an MI355X): one scan over the concatenation, cut into documents on the GPU by
pfac_records_segment.  The reference answer is the CPU oracle run on every document's bytes on their own (positions
relative to the document) -- independent of the length table the device pass uses.  Integer work: bit-exact."""
import os

import numpy as np
import pytest

from docref import oracle_per_doc, random_offsets
from orc import Oracle, ac_whole_shard
from phfpfac_amd import GpuMatcher, PfacError, PfacTable
from phfpfac_amd import _ffi
from phfpfac_amd.matcher import splitmix64_bytes, tiled_bytes

pytestmark = pytest.mark.gpu

SEED = 0x5048465046414331
TILE = 4096


def para_bytes(resolve, n):
    return tiled_bytes(n, open(resolve("paragraph402"), "rb").read())


def assert_docs(table, got, want):
    first, rec = got
    wfirst, wpos, wids = want
    assert rec.size == wpos.size, (rec.size, wpos.size)
    np.testing.assert_array_equal(first, wfirst)
    np.testing.assert_array_equal(rec["pos"].astype(np.int64), wpos)
    np.testing.assert_array_equal(table.idmap[rec["state"]], wids)


def check(pattern_path, buf, off, n_streams=1, table=None):
    table = table or PfacTable.from_file(pattern_path, 256)
    with GpuMatcher(0, n_streams) as g:
        g.load_table(table)
        got = g.scan_documents((buf, off))
    o = Oracle(pattern_path, 1, 1)
    want = oracle_per_doc(o, buf, off)
    o.close()
    assert_docs(table, got, want)
    return got


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pat", ["xaa", "xaa+xab+xac+xad"])
@pytest.mark.parametrize("seed", [1, 2])
def test_random_splits_of_text(pat, seed, resolve):
    """1 MiB of paragraph text cut at seeded random places (4-byte records, tables in LDS)."""
    rng = np.random.default_rng(seed)
    buf = para_bytes(resolve, 1 << 20)
    off = random_offsets(rng, buf.size, int(rng.integers(50, 3000)), empties=20)
    first, rec = check(resolve(pat), buf, off)
    assert rec.size > 1000


def test_two_byte_records_experimentpattern(resolve):
    buf = para_bytes(resolve, 300_001)
    rng = np.random.default_rng(3)
    off = random_offsets(rng, buf.size, 700, empties=10)
    check(resolve("experimentpattern"), buf, off)


@pytest.mark.parametrize("env", [{"PFAC_WIDE": "1"}, {"PFAC_DENSE": "1"}, {"PFAC_FORCE_L2": "1"},
                                 {"PFAC_DENSE": "1", "PFAC_FORCE_L2": "1"}])
def test_record_forms_and_kernel_variants(env, resolve, monkeypatch):
    """8-byte records (PFAC_WIDE), dense staging (and its second form on L2 tables), the L2 table path."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    buf = para_bytes(resolve, 700_003)
    rng = np.random.default_rng(4)
    off = random_offsets(rng, buf.size, 900, empties=5)
    table = PfacTable.from_file(resolve("xaa+xab+xac+xad"), 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.scan_bytes(buf)                       # (dense mode: a first scan, so that the adapted mode is what runs)
        if "PFAC_WIDE" in env:
            assert g.scan_format()[0] == 8
        got = g.scan_documents((buf, off))
    o = Oracle(resolve("xaa+xab+xac+xad"), 1, 1)
    assert_docs(table, got, oracle_per_doc(o, buf, off))
    o.close()


@pytest.mark.parametrize("doc_bytes", [1500, None])
def test_snort_scale_set_on_random_bytes(doc_bytes, resolve):
    """75 840 patterns (tables through L2) on splitmix64 bytes, 1 500-byte and variable-size documents."""
    buf = splitmix64_bytes(3 << 20, SEED)
    if doc_bytes:
        off = np.append(np.arange(0, buf.size, doc_bytes, dtype=np.uint64), np.uint64(buf.size))
    else:
        rng = np.random.default_rng(5)
        sizes = rng.integers(0, 9000, 2000)
        off = np.minimum(np.concatenate([[0], np.cumsum(sizes)]), buf.size).astype(np.uint64)
        off[-1] = buf.size
    first, rec = check(resolve("bytefile/1000000byte"), buf, off)
    assert rec.size > 10000


# ---------------------------------------------------------------------------
def test_edge_documents(resolve):
    """Empty documents first, last and in runs; 5 000 documents (4 000 of one byte) inside one tile; boundaries at
    4096k - 1, 4096k, 4096k + 1."""
    buf = para_bytes(resolve, 64 * 1024 + 123)
    n = buf.size
    cuts = [0, 0, 0, 10, 10, 10, 10, 500]
    t1 = 4 * TILE                                              # one tile: 4 000 one-byte documents and 1 000 empty ones
    cuts += [t1 + i for i in range(4000)] + [t1 + 4000] * 1000
    for k in (6, 7, 9, 12):
        cuts += [k * TILE - 1, k * TILE, k * TILE + 1]
    cuts += [13 * TILE] * 3 + [n, n, n]
    off = np.array(sorted(cuts), dtype=np.uint64)
    assert off[0] == 0 and off[-1] == n
    first, rec = check(resolve("xaa"), buf, off)
    check(resolve("experimentpattern"), buf, off)
    assert first[0] == first[1] == first[2] == 0
    assert first[-1] == first[-2] == first[-3] == rec.size


def test_document_equal_to_a_pattern_and_one_byte_shorter(resolve, tmp_path):
    pf = tmp_path / "p.pat"
    pf.write_bytes(b"abcdefg\nxyz\nde\n")
    table = PfacTable.from_file(str(pf), 256)
    docs = [b"abcdefg", b"abcdef", b"xyz", b"xy", b"z"]
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        first, rec = g.scan_documents(docs)
    ids = table.idmap[rec["state"]]
    per = [list(zip(rec["pos"][first[d]:first[d + 1]].tolist(), ids[first[d]:first[d + 1]].tolist())) for d in range(5)]
    assert per == [[(0, 1), (3, 3)], [(3, 3)], [(0, 2)], [], []]
    off = np.array([0, 7, 13, 16, 18, 19], dtype=np.uint64)
    buf = np.frombuffer(b"".join(docs), dtype=np.uint8)
    check(str(pf), buf, off, table=table)


def test_one_pattern_spanning_three_documents(resolve, tmp_path):
    pf = tmp_path / "p.pat"
    pf.write_bytes(b"needle\nee\n")
    table = PfacTable.from_file(str(pf), 256)
    buf = np.frombuffer(b"..needle..needle", dtype=np.uint8)
    off = np.array([0, 3, 5, buf.size], dtype=np.uint64)       # "..n" "ee" "dle..needle"
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        whole = g.scan_bytes(buf)
        first, rec = g.scan_documents((buf, off))
    assert sorted(table.idmap[whole["state"]].tolist()) == [1, 1, 2, 2]
    assert first.tolist() == [0, 0, 1, 3]
    assert rec["pos"].tolist() == [0, 5, 6] and table.idmap[rec["state"]].tolist() == [2, 1, 2]


@pytest.mark.parametrize("pat", ["xaa", "experimentpattern"])
def test_whole_input_as_one_document(pat, resolve):
    buf = para_bytes(resolve, 500_000)
    table = PfacTable.from_file(resolve(pat), 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        whole = g.scan_bytes(buf)
        first, rec = g.scan_documents([buf.tobytes()])
    assert first.tolist() == [0, whole.size]
    np.testing.assert_array_equal(rec, whole)


def test_owned_range_shorter_than_the_input(resolve):
    """n_owned < n_avail: matches that run into the halo belong to no document and are dropped."""
    buf = para_bytes(resolve, 200_000)
    table = PfacTable.from_file(resolve("xaa"), 256)
    lens = table.final_lengths()
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(lens)
        whole = g.scan_bytes(buf)
        long_ = whole[(whole["pos"] > 150_000) & (lens[whole["state"]] >= 3)]
        n_owned = int(long_["pos"][0]) + 1                     # the walk of that match runs on into the halo
        off = np.array([0, 4095, 70_000, 70_000, n_owned], dtype=np.uint64)
        g.reserve(0, buf.size, 1 << 16)
        g.h2d(buf)
        total = g.scan_resident(n_owned, buf.size)
        g.set_doc_offsets(off)
        kept = g.segment_records(off.size - 1)
        got = g.segment_to_host(kept, off.size - 1)
    o = Oracle(resolve("xaa"), 1, 1)
    want = oracle_per_doc(o, buf, off)
    o.close()
    assert_docs(table, got, want)
    assert total > kept
    last = got[1][int(got[0][3]):]
    assert not ((last["pos"] == n_owned - 1 - int(off[3])) & (last["state"] == long_["state"][0])).any()


# ---------------------------------------------------------------------------
def status_of(fn):
    with pytest.raises(PfacError) as e:
        fn()
    return e.value


def test_bad_offsets_are_refused(resolve):
    buf = para_bytes(resolve, 20_000)
    table = PfacTable.from_file(resolve("xaa"), 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.scan_documents([buf[:10_000].tobytes(), buf[10_000:].tobytes()])
        for bad in ([0, 12_000, 11_000, 20_000], [1, 10_000, 20_000], [0, 10_000, 19_999], [0, 10_000, 20_001]):
            g.set_doc_offsets(np.array(bad, dtype=np.uint64))
            assert status_of(lambda: g.segment_records(len(bad) - 1)).status == _ffi.PFAC_E_ARG
        g.set_doc_offsets(np.array([0, 20_000], dtype=np.uint64))
        assert status_of(lambda: g.segment_records(2)).status == _ffi.PFAC_E_ARG     # n_docs differs from the slot's
        assert g.segment_records(1) > 0


def test_state_errors(resolve):
    buf = para_bytes(resolve, 20_000)
    off = np.array([0, 20_000], dtype=np.uint64)
    table = PfacTable.from_file(resolve("xaa"), 256)
    other = PfacTable.from_file(resolve("experimentpattern"), 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_doc_offsets(off)
        assert status_of(lambda: g.segment_records(1)).status == _ffi.PFAC_E_STATE          # before a scan
        assert status_of(lambda: g.segment_to_host(0, 1)).status == _ffi.PFAC_E_STATE
        g.scan_bytes(buf)
        assert g.segment_records(1) > 0
        g.load_table(table)                                                               # an upload clears the lengths
        g.scan_bytes(buf)
        assert status_of(lambda: g.segment_records(1)).status == _ffi.PFAC_E_STATE
        g.load_table(other)
        g.scan_bytes(buf)
        assert status_of(lambda: g.segment_records(1)).status == _ffi.PFAC_E_STATE          # never had lengths
        assert status_of(lambda: g.set_final_lengths(table.final_lengths())).status == _ffi.PFAC_E_ARG   # wrong table
        g.set_final_lengths(other.final_lengths())
        assert g.segment_records(1) > 0
        g.load_table(table)                                                               # the scan ran with `other`
        g.set_final_lengths(table.final_lengths())
        assert status_of(lambda: g.segment_records(1)).status == _ffi.PFAC_E_STATE
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_doc_offsets(off)
        g.scan_bytes(buf)
        assert status_of(lambda: g.segment_records(1)).status == _ffi.PFAC_E_STATE          # no lengths at all


def test_caller_buffers_overflow_and_sentinels(resolve):
    import torch
    buf = para_bytes(resolve, 100_000)
    rng = np.random.default_rng(9)
    off = random_offsets(rng, buf.size, 300)
    table = PfacTable.from_file(resolve("xaa"), 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        first, rec = g.scan_documents((buf, off))
        n = rec.size
        assert n > 100
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        sentinel = int(np.uint64(0xABABABABABABABAB).view(np.int64))
        out = torch.full((n + 1,), sentinel, dtype=torch.int64, device="cuda")
        dfirst = torch.full((off.size + 1,), sentinel, dtype=torch.int64, device="cuda")
        e = status_of(lambda: g.segment_records(off.size - 1, d_doc_offsets=d_off, d_out=out, out_cap=n - 1, d_doc_first=dfirst))
        assert e.status == _ffi.PFAC_E_OVERFLOW and e.n_kept == n
        g.sync()
        assert (out.cpu() == sentinel).all() and (dfirst.cpu() == sentinel).all()
        assert g.segment_records(off.size - 1, d_doc_offsets=d_off, d_out=out, out_cap=n, d_doc_first=dfirst) == n
        g.sync()
        got = out.cpu().numpy()
        assert got[n] == sentinel
        np.testing.assert_array_equal(got[:n].view(np.uint64), rec.view(np.uint64))
        f = dfirst.cpu().numpy()
        assert f[-1] == sentinel
        np.testing.assert_array_equal(f[:-1].view(np.uint64), first)
        assert status_of(lambda: g.segment_to_host(n, off.size - 1)).status == _ffi.PFAC_E_STATE   # nothing slot-owned


def test_two_slots_do_not_disturb_each_other(resolve):
    table = PfacTable.from_file(resolve("xaa+xab+xac+xad"), 256)
    a = para_bytes(resolve, 300_000)
    b = np.ascontiguousarray(para_bytes(resolve, 250_000 + 401)[401:])
    oa = random_offsets(np.random.default_rng(11), a.size, 400)
    ob = random_offsets(np.random.default_rng(12), b.size, 90)
    with GpuMatcher(0, 2) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        for s, buf, off in ((0, a, oa), (1, b, ob)):
            g.reserve(s, buf.size, 2 * buf.size)
            g.h2d(buf, s)
            g.scan_async(buf.size, slot=s)
        for s, buf, off in ((0, a, oa), (1, b, ob)):
            g.scan_finish(s)
            g.set_doc_offsets(off, s)
        ka = g.segment_records(oa.size - 1, slot=0)
        kb = g.segment_records(ob.size - 1, slot=1)
        gb = g.segment_to_host(kb, ob.size - 1, slot=1)
        ga = g.segment_to_host(ka, oa.size - 1, slot=0)
    o = Oracle(resolve("xaa+xab+xac+xad"), 1, 1)
    assert_docs(table, ga, oracle_per_doc(o, a, oa))
    assert_docs(table, gb, oracle_per_doc(o, b, ob))
    o.close()


# ---------------------------------------------------------------------------
def test_one_gib_random_bytes_snort_scale_1500_byte_documents(resolve):
    """1 GiB of splitmix64 bytes, 75 840 patterns, 1 500-byte documents.  The unsegmented scan is pinned first against
    one serial Aho-Corasick pass (count + checksum); the expectation of the cut is then built on the host from its
    records with the lengths of the pattern file's own lines."""
    import torch
    n = 1 << 30
    path = resolve("bytefile/1000000byte")
    table = PfacTable.from_file(path, 256)
    lines = open(path, "rb").read()[:-1].split(b"\n")
    line_len = np.array([len(x) for x in lines], dtype=np.int64)
    off = np.append(np.arange(0, n, 1500, dtype=np.uint64), np.uint64(n))
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_random(buf, n, SEED)
        g.reserve(0, 0, n // 8)
        total = g.scan_resident(n, n, d_input=buf)
        chk = g.checksum(total)
        host = buf[:n].cpu().numpy()
        del buf
        whole = g.records_to_host(total)
        g.set_doc_offsets(off)
        kept = g.segment_records(off.size - 1)
        first, rec = g.segment_to_host(kept, off.size - 1)
    torch.cuda.empty_cache()
    assert (total, chk) == ac_whole_shard(path, host)
    del host
    pos = whole["pos"].astype(np.int64)
    doc = np.searchsorted(off.astype(np.int64), pos, side="right") - 1
    end = off.astype(np.int64)[doc + 1]
    keep = pos + line_len[table.idmap[whole["state"]] - 1] <= end
    assert kept == int(keep.sum()) and 0 < kept < total
    np.testing.assert_array_equal(rec["pos"].astype(np.int64), (pos - off.astype(np.int64)[doc])[keep])
    np.testing.assert_array_equal(rec["state"], whole["state"][keep])
    np.testing.assert_array_equal(first, np.searchsorted(doc[keep], np.arange(off.size), side="left").astype(np.uint64))
