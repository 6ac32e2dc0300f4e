"""Per-document leftmost-longest selection and find-and-replace on the GPU (run with -m gpu on an MI355X):
pfac_records_leftmost_longest_documents and pfac_replace_documents against the CPU.  The expectation is the oracle run on
every document on its own, lengths from the pattern file's own lines, llref.greedy and replref.splice per document
(tests/docreplref.py), and Python `re` for small literal sets -- never the device.  Bit-exact."""
import numpy as np
import pytest

from docref import random_offsets
from docreplref import per_doc
from llref import check_greedy, line_lengths
from orc import Oracle, ac_whole_shard
from passfuzz import Case, KNOBS, knob_label
from phfpfac_amd import GpuMatcher, PfacError, PfacTable
from phfpfac_amd import _ffi
from phfpfac_amd.matcher import tiled_bytes
from replref import re_replace, rep_table, splice

pytestmark = pytest.mark.gpu

TILE = 4096
SEED = 0x5048465046414331


def write_patterns(tmp_path, pats, name="p.pat"):
    f = tmp_path / name
    f.write_bytes(b"".join(p + b"\n" for p in pats))
    return str(f)


def random_reps(n_ids, seed, max_len=16):
    rng = np.random.default_rng(seed)
    return {i: bytes(rng.integers(0, 256, int(rng.integers(0, max_len + 1))).astype(np.uint8))
            for i in range(1, n_ids + 1)}


def redaction_reps(ll, fill=b"#"):
    return {i: fill * int(ll[i]) for i in range(1, ll.size)}


def status_of(fn):
    with pytest.raises(PfacError) as e:
        fn()
    return e.value


def expect(path, buf, off, reps):
    o = Oracle(path, 1, 1)
    want = per_doc(o, buf, off, line_lengths(path), rep_table(reps))
    o.close()
    return want


def check(g, table, path, buf, off, reps, want=None):
    """select_documents and replace_documents of (buf, off) against the per-document CPU expectation."""
    want = want or expect(path, buf, off, reps)
    wfirst, wpos, wids, woff, wout = want
    first, rec = g.select_documents((buf, off))
    assert rec.size == wpos.size, (rec.size, wpos.size)
    np.testing.assert_array_equal(first, wfirst)
    np.testing.assert_array_equal(rec["pos"].astype(np.int64), wpos)
    np.testing.assert_array_equal(table.idmap[rec["state"]], wids)
    out_off, out = g.replace_documents((buf, off))
    np.testing.assert_array_equal(out_off, woff)
    assert out.size == wout.size and bytes(out) == bytes(wout)
    return want


def matcher_for(path, reps, width=256):
    table = PfacTable.from_file(path, width)
    g = GpuMatcher(0, 1)
    g.load_table(table)
    g.set_replacements(reps)
    return g, table


# ---------------------------------------------------------------------------
def test_worked_example(tmp_path):
    """Patterns abc and cd, documents xab and cdy, redaction with '*': xab + **y per document, x***dy as one text."""
    pats = [b"abc", b"cd"]
    path = write_patterns(tmp_path, pats)
    table = PfacTable.from_file(path, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_redaction(b"*")
        first, rec = g.select_documents([b"xab", b"cdy"])
        assert list(first) == [0, 0, 1] and rec["pos"].tolist() == [0] and table.idmap[rec["state"]].tolist() == [2]
        out_off, out = g.replace_documents([b"xab", b"cdy"])
        assert bytes(out) == b"xab**y" and out_off.tolist() == [0, 3, 6]
        whole, _ = g.replace(np.frombuffer(b"xabcdy", dtype=np.uint8))
        assert bytes(whole) == b"x***dy" != bytes(out)
    reps = {1: b"***", 2: b"**"}
    assert bytes(re_replace(pats, [reps[1], reps[2]], np.frombuffer(b"cdy", dtype=np.uint8), 0, 3)[0]) == b"**y"


@pytest.mark.parametrize("pat", ["experimentpattern", "xaa", "xaa+xab+xac+xad"])
def test_random_cuts_of_text_with_empty_documents(pat, resolve):
    path = resolve(pat)
    ll = line_lengths(path)
    buf = tiled_bytes(300_007, open(resolve("paragraph402"), "rb").read())
    rng = np.random.default_rng(17)
    off = random_offsets(rng, buf.size, 400, empties=30)
    for reps in (random_reps(ll.size - 1, 3), redaction_reps(ll)):
        g, table = matcher_for(path, reps)
        with g:
            want = check(g, table, path, buf, off, reps)
    assert want[1].size > 1000


def test_small_literal_set_against_re(tmp_path):
    pats = [b"the", b"th", b"he", b"e t", b"them", b"a"]
    reps = [b"", b"TH", b"<he>", b"_", b"THEM!", b"aaaa"]
    path = write_patterns(tmp_path, pats)
    text = b"the theme of them is that the heat; a hat, then them. " * 300
    buf = np.frombuffer(text, dtype=np.uint8)
    off = random_offsets(np.random.default_rng(2), buf.size, 200, empties=10)
    g, table = matcher_for(path, {i + 1: r for i, r in enumerate(reps)})
    with g:
        out_off, out = g.replace_documents((buf, off))
    for d in range(off.size - 1):
        a, b = int(off[d]), int(off[d + 1])
        want, _ = re_replace(pats, reps, buf[a:b], 0, b - a)
        assert bytes(out[int(out_off[d]):int(out_off[d + 1])]) == bytes(want)


@pytest.mark.parametrize("env", [{}, {"PFAC_WIDE": "1"}, {"PFAC_REC_BYTES": "4"}, {"PFAC_DENSE": "1"},
                                 {"PFAC_FORCE_L2": "1"}, {"PFAC_FORCE_L2": "1", "PFAC_DENSE": "1"}],
                         ids=knob_label)
@pytest.mark.parametrize("pat", ["experimentpattern", "xaa+xab+xac+xad"])
def test_record_forms_and_kernel_variants(pat, env, resolve, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    path = resolve(pat)
    buf = tiled_bytes((1 << 20) + 77, open(resolve("paragraph402"), "rb").read())
    off = random_offsets(np.random.default_rng(5), buf.size, 700, empties=20)
    reps = random_reps(line_lengths(path).size - 1, 5)
    g, table = matcher_for(path, reps)
    with g:
        check(g, table, path, buf, off, reps)
        if "PFAC_WIDE" in env:
            assert g.scan_format()[0] == 8
        elif "PFAC_REC_BYTES" in env:
            assert g.scan_format()[0] == 4


@pytest.mark.parametrize("pat", ["experimentpattern", "xaa+xab+xac+xad"])
def test_document_window_edges(pat, resolve):
    """Tiles with 58 to 66 document starts (both sides of the shuffle window), starts on a tile's first byte, a document
    over several tiles and one over several groups of 64 tiles."""
    buf = tiled_bytes(200 * TILE + 99, open(resolve("paragraph402"), "rb").read())
    rng = np.random.default_rng(63)
    cuts = [0, buf.size]
    for k, S in enumerate(range(58, 67)):
        t = 2 + 2 * k
        starts = rng.choice(np.arange(t * TILE + 1, (t + 1) * TILE), S, replace=False).tolist()
        if k % 2:
            starts[0] = t * TILE                                # one start on the tile's first byte
        cuts += starts
    cuts += [21 * TILE + 100, 25 * TILE - 5, 30 * TILE, 30 * TILE + 150 * TILE + 7]   # 3 tiles; > 2 groups of 64
    off = np.array(sorted(cuts), dtype=np.uint64)
    path = resolve(pat)
    reps = random_reps(line_lengths(path).size - 1, 8)
    g, table = matcher_for(path, reps)
    with g:
        want = check(g, table, path, buf, off, reps)
    assert want[1].size > 1000


def test_lengths(tmp_path):
    """Patterns up to 1 022 bytes (the longest the pattern reader takes); documents shorter than a pattern, equal to it
    and one byte longer; 1-byte documents; every document but one empty; nothing scanned."""
    rng = np.random.default_rng(9)
    long_pat = bytes(rng.integers(97, 100, 1022).astype(np.uint8))
    pats = [long_pat, long_pat[:700], long_pat[:5], b"a", b"ab", b"ba"]
    path = write_patterns(tmp_path, pats)
    reps = random_reps(len(pats), 4, 40)
    reps[1] = b"L" * 5000
    g, table = matcher_for(path, reps)
    filler = bytes(rng.integers(97, 100, 3000).astype(np.uint8))
    with g:
        for L in (1022, 700):
            docs = [long_pat[:L - 1], long_pat[:L], long_pat[:L] + b"c", filler[:L + 1], long_pat[:L] + long_pat[:L]]
            buf = np.frombuffer(b"".join(docs), dtype=np.uint8)
            off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
            check(g, table, path, buf, off, reps)
        buf = np.frombuffer(filler[:2000], dtype=np.uint8)
        check(g, table, path, buf, np.arange(buf.size + 1, dtype=np.uint64), reps)          # 1-byte documents
        for k in (0, 500, 999):                                 # every document but document k empty
            off = np.zeros(1001, dtype=np.uint64)
            off[k + 1:] = buf.size
            check(g, table, path, buf, off, reps)
        check(g, table, path, np.zeros(0, dtype=np.uint8), np.zeros(4, dtype=np.uint64), reps)   # nothing to scan


@pytest.mark.parametrize("pat", ["experimentpattern", "xaa+xab+xac+xad"])
def test_one_document_equals_the_whole_stream(pat, resolve):
    path = resolve(pat)
    buf = np.fromfile(resolve("1M"), dtype=np.uint8)
    reps = random_reps(line_lengths(path).size - 1, 6)
    g, table = matcher_for(path, reps)
    with g:
        first, rec = g.select_documents([buf])
        whole, ex = g.scan_leftmost_longest(buf)
        assert ex == 0 and list(first) == [0, whole.size]
        assert rec.tobytes() == whole.tobytes()
        out_off, out = g.replace_documents([buf])
        wout, _ = g.replace(buf)
        assert bytes(out) == bytes(wout) and out_off.tolist() == [0, wout.size]


def test_halo_record_is_never_picked(tmp_path):
    """A scan with n_owned < n_avail: a record that runs past n_owned (into the halo) is never picked."""
    path = write_patterns(tmp_path, [b"abcd", b"ab", b"x"])
    reps = {1: b"1111", 2: b"2", 3: b"333"}
    data = np.frombuffer(b"xxabxabcdzzz" * 1000 + b"abcd", dtype=np.uint8)
    n_owned = data.size - 2                                     # the last "abcd" starts in the owned range
    g, table = matcher_for(path, reps)
    with g:
        g.set_final_lengths(table.final_lengths())
        g.reserve(0, data.size, 1 << 16)
        g.h2d(data)
        g.scan_resident(n_owned, data.size)
        off = np.array([0, 5000, n_owned], dtype=np.uint64)
        g.set_doc_offsets(off)
        n = g.select_leftmost_longest_documents(2)
        first, rec = g.doc_selection_to_host(n, 2)
        ob = g.replace_selection_documents()
        out_off = g.replacement_doc_offsets_to_host(2)
        out = g.replacement_to_host(ob)
    ll = line_lengths(path)
    assert (rec["pos"].astype(np.int64) + ll[table.idmap[rec["state"]]] <= n_owned).all()
    wfirst, wpos, wids, woff, wout = expect(path, np.ascontiguousarray(data[:n_owned]), off, reps)
    np.testing.assert_array_equal(first, wfirst)
    doc = np.repeat([0, 1], np.diff(first.astype(np.int64)))
    np.testing.assert_array_equal(rec["pos"].astype(np.int64) - off[doc].astype(np.int64), wpos)
    np.testing.assert_array_equal(out_off, woff)
    assert bytes(out) == bytes(wout) and bytes(out[-2:]) == b"z2"  # the owned "ab" of the last "abcd" is picked


def test_state_handling(resolve, tmp_path):
    import torch
    path = resolve("experimentpattern")
    buf = np.fromfile(resolve("paragraph402"), dtype=np.uint8)
    buf = np.ascontiguousarray(np.tile(buf, 20))
    off = random_offsets(np.random.default_rng(3), buf.size, 40, empties=3)
    n_docs = off.size - 1
    reps = random_reps(line_lengths(path).size - 1, 12)
    wfirst, wpos, wids, woff, wout = expect(path, buf, off, reps)
    table = PfacTable.from_file(path, 256)
    with GpuMatcher(0, 2) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_doc_offsets(off)
        assert status_of(lambda: g.select_leftmost_longest_documents(n_docs)).status == _ffi.PFAC_E_STATE   # before a scan
        g.reserve(0, buf.size, 1 << 16)
        g.h2d(buf)
        g.scan_resident(buf.size)
        n = g.select_leftmost_longest_documents(n_docs)
        assert n == wpos.size
        assert status_of(lambda: g.replace_selection_documents()).status == _ffi.PFAC_E_STATE   # no replacements
        g.set_replacements(reps)
        # after a document selection the plain replace returns the concatenated output (entry 0, exit 0)
        ob = g.replace_selection()
        assert bytes(g.replacement_to_host(ob)) == bytes(wout)
        assert status_of(lambda: g.replacement_doc_offsets_to_host(n_docs)).status == _ffi.PFAC_E_STATE
        # after a plain selection the document replace refuses
        g.select_leftmost_longest(0)
        assert status_of(lambda: g.replace_selection_documents()).status == _ffi.PFAC_E_STATE
        g.select_leftmost_longest_documents(n_docs)
        assert g.replace_selection_documents() == wout.size
        np.testing.assert_array_equal(g.replacement_doc_offsets_to_host(n_docs), woff)
        g.scan_resident(buf.size)                               # a new scan: no selection since
        assert status_of(lambda: g.replace_selection_documents()).status == _ffi.PFAC_E_STATE
        g.select_leftmost_longest_documents(n_docs)
        g.set_doc_offsets(off)                                  # the slot's offsets replaced since the selection
        assert status_of(lambda: g.replace_selection_documents()).status == _ffi.PFAC_E_STATE
        # an earlier table, then no lengths
        g.load_table(table)
        assert status_of(lambda: g.select_leftmost_longest_documents(n_docs)).status == _ffi.PFAC_E_STATE
        g.scan_resident(buf.size)
        assert status_of(lambda: g.select_leftmost_longest_documents(n_docs)).status == _ffi.PFAC_E_STATE
        g.set_final_lengths(table.final_lengths())
        n = g.select_leftmost_longest_documents(n_docs)
        assert status_of(lambda: g.replace_selection_documents()).status == _ffi.PFAC_E_STATE   # replacements cleared
        g.set_replacements(reps)
        # bad offsets: PFAC_E_ARG, caller buffers with sentinels untouched
        d_out = torch.full((n + 16,), -1, dtype=torch.int64, device="cuda:0")
        d_first = torch.full((n_docs + 1,), -1, dtype=torch.int64, device="cuda:0")
        for bad in ([1] + off[1:].tolist(), off[:-1].tolist() + [buf.size - 1],
                    off[:5].tolist() + [int(off[6]) + 1, int(off[6])] + off[7:].tolist()):
            d_bad = torch.tensor(np.array(bad, dtype=np.int64), device="cuda:0")
            e = status_of(lambda: g.select_leftmost_longest_documents(len(bad) - 1, d_doc_offsets=d_bad, d_out=d_out,
                                                                      out_cap=n + 16, d_doc_first=d_first))
            assert e.status == _ffi.PFAC_E_ARG
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == -1).all() and (d_first.cpu().numpy() == -1).all()
        # overflow reports the exact count, writes nothing
        d_off = torch.tensor(off.astype(np.int64), device="cuda:0")
        e = status_of(lambda: g.select_leftmost_longest_documents(n_docs, d_doc_offsets=d_off, d_out=d_out, out_cap=n - 1,
                                                                  d_doc_first=d_first))
        assert e.status == _ffi.PFAC_E_OVERFLOW and e.n_selected == n
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == -1).all() and (d_first.cpu().numpy() == -1).all()
        # caller buffers end to end: the replace needs them back
        assert g.select_leftmost_longest_documents(n_docs, d_doc_offsets=d_off, d_out=d_out, out_cap=n + 16,
                                                   d_doc_first=d_first) == n
        assert status_of(lambda: g.replace_selection_documents()).status == _ffi.PFAC_E_STATE
        assert status_of(lambda: g.replace_selection_documents(d_sel=d_out)).status == _ffi.PFAC_E_STATE
        assert status_of(lambda: g.replace_selection_documents(d_sel=d_out, d_doc_offsets=d_off)).status == _ffi.PFAC_E_STATE
        d_rep = torch.full((wout.size + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
        d_ooff = torch.full((n_docs + 1,), -1, dtype=torch.int64, device="cuda:0")
        e = status_of(lambda: g.replace_selection_documents(d_out=d_rep, out_cap=wout.size - 1, d_out_offsets=d_ooff,
                                                            d_sel=d_out, d_doc_offsets=d_off, d_doc_first=d_first))
        assert e.status == _ffi.PFAC_E_OVERFLOW and e.out_bytes == wout.size
        torch.cuda.synchronize()
        assert (d_rep.cpu().numpy() == 0xA5).all() and (d_ooff.cpu().numpy() == -1).all()
        assert g.replace_selection_documents(d_out=d_rep, out_cap=wout.size + 64, d_out_offsets=d_ooff, d_sel=d_out,
                                             d_doc_offsets=d_off, d_doc_first=d_first) == wout.size
        g.sync()
        host = d_rep.cpu().numpy()
        assert bytes(host[:wout.size]) == bytes(wout) and (host[wout.size:] == 0xA5).all()
        np.testing.assert_array_equal(d_ooff.cpu().numpy().view(np.uint64), woff)
        np.testing.assert_array_equal(d_first.cpu().numpy().view(np.uint64), wfirst)
        sel = d_out[:n].cpu().numpy().view(np.uint32).reshape(-1, 2)
        doc = np.repeat(np.arange(n_docs), np.diff(wfirst.astype(np.int64)))
        np.testing.assert_array_equal(sel[:, 0].astype(np.int64) - off[doc].astype(np.int64), wpos)
        assert status_of(lambda: g.replacement_doc_offsets_to_host(n_docs)).status == _ffi.PFAC_E_STATE
        # two slots stay independent
        other = np.ascontiguousarray(buf[::-1])
        ooff = random_offsets(np.random.default_rng(4), other.size, 25)
        g.reserve(1, other.size, 1 << 16)
        g.h2d(other, 1)
        g.scan_resident(other.size, slot=1)
        g.set_doc_offsets(ooff, slot=1)
        g.set_doc_offsets(off, slot=0)
        g.scan_resident(buf.size, slot=0)
        n0 = g.select_leftmost_longest_documents(n_docs, slot=0)
        n1 = g.select_leftmost_longest_documents(ooff.size - 1, slot=1)
        b1 = g.replace_selection_documents(slot=1)
        b0 = g.replace_selection_documents(slot=0)
        f0, _ = g.doc_selection_to_host(n0, n_docs, slot=0)
        o0, o1 = g.replacement_doc_offsets_to_host(n_docs, 0), g.replacement_doc_offsets_to_host(ooff.size - 1, 1)
        out0, out1 = g.replacement_to_host(b0, 0), g.replacement_to_host(b1, 1)
    np.testing.assert_array_equal(f0, wfirst)
    np.testing.assert_array_equal(o0, woff)
    assert bytes(out0) == bytes(wout)
    w1 = expect(path, other, ooff, reps)
    assert n1 == w1[1].size
    np.testing.assert_array_equal(o1, w1[3])
    assert bytes(out1) == bytes(w1[4])


@pytest.mark.parametrize("seed", range(1, 3 * len(KNOBS), 8))
def test_passes_fuzz_documents(seed, tmp_path, monkeypatch):
    """Seeded random cases of tests/passfuzz.py: their offsets (over the owned range), replacements and knob sets."""
    case = Case(seed)
    for k, v in case.knobs.items():
        monkeypatch.setenv(k, v)
    path = case.write_patterns(str(tmp_path / "p.pat"))
    no = case.n_owned
    table = PfacTable.from_file(path, case.width)
    want = expect(path, np.ascontiguousarray(case.data[:no]), case.off, case.reps)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_replacements(case.reps)
        g.reserve(0, max(case.n, 1), max(case.n // 8, 4096))
        if case.n:
            g.h2d(case.data)
        g.scan_resident(no, case.n)
        n_docs = case.off.size - 1
        g.set_doc_offsets(case.off)
        n = g.select_leftmost_longest_documents(n_docs)
        first, rec = g.doc_selection_to_host(n, n_docs)
        ob = g.replace_selection_documents()
        out_off = g.replacement_doc_offsets_to_host(n_docs)
        out = g.replacement_to_host(ob)
    wfirst, wpos, wids, woff, wout = want
    assert n == wpos.size, case.describe()
    np.testing.assert_array_equal(first, wfirst)
    doc = np.repeat(np.arange(n_docs), np.diff(wfirst.astype(np.int64)))
    np.testing.assert_array_equal(rec["pos"].astype(np.int64) - case.off[doc].astype(np.int64), wpos)
    np.testing.assert_array_equal(table.idmap[rec["state"]], wids)
    np.testing.assert_array_equal(out_off, woff)
    assert bytes(out) == bytes(wout), case.describe()


def test_scale_snort_random_1500_byte_documents(resolve):
    """256 MiB of splitmix64 bytes, 75 840 patterns, 1 500-byte documents.  The scan is pinned against serial
    Aho-Corasick; the records that stay inside their document (lengths from the pattern file's lines) are the ones
    the per-document selection chooses from, and the greedy over them from 0 is that selection (check_greedy).  The
    output against splice of that selection, out_off against a cumulative sum on the host."""
    import torch
    n = 256 << 20
    path = resolve("bytefile/1000000byte")
    table = PfacTable.from_file(path, 256)
    ll = line_lengths(path)
    reps = random_reps(ll.size - 1, 31)
    off = np.append(np.arange(0, n, 1500, dtype=np.uint64), np.uint64(n))
    n_docs = off.size - 1
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_replacements(reps)
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_random(buf, n, SEED)
        g.reserve(0, 0, n // 8)
        total = g.scan_resident(n, n, d_input=buf)
        chk = g.checksum(total)
        whole = g.records_to_host(total)
        g.set_doc_offsets(off)
        n_sel = g.select_leftmost_longest_documents(n_docs)
        first, sel = g.doc_selection_to_host(n_sel, n_docs)
        ob = g.replace_selection_documents(d_input=buf)
        out_off = g.replacement_doc_offsets_to_host(n_docs)
        out = g.replacement_to_host(ob)
        host = buf[:n].cpu().numpy()
        del buf
    torch.cuda.empty_cache()
    assert (total, chk) == ac_whole_shard(path, host)
    pos = whole["pos"].astype(np.int64)
    lens = ll[table.idmap[whole["state"]]]
    del whole
    o64 = off.astype(np.int64)
    doc = np.searchsorted(o64, pos, side="right") - 1
    keep = pos + lens <= o64[doc + 1]
    sids = table.idmap[sel["state"]]
    spos = sel["pos"].astype(np.int64)
    assert check_greedy(pos[keep], lens[keep], (spos, ll[sids]), 0, n) == 0
    np.testing.assert_array_equal(first, np.searchsorted(spos, o64, side="left").astype(np.uint64))
    assert 0 < n_sel < int(keep.sum())
    off_t, rb = rep_table(reps)
    delta = np.concatenate([[0], np.cumsum((off_t[sids + 1] - off_t[sids]) - ll[sids])])
    np.testing.assert_array_equal(out_off.astype(np.int64), o64 + delta[first.astype(np.int64)])
    want = splice(host, 0, n, spos, ll[sids], sids, (off_t, rb))
    assert out.size == want.size == ob == int(out_off[-1])
    assert np.array_equal(out, want)
