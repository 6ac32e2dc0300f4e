"""The whole-word filter, pfac_records_filter_words (run with -m gpu on an MI355X): the records of a finished scan that
split a word are dropped in place, and every consumer of the scan -- fetches, text, checksum, the document cut, both
selections, both replaces -- then sees whole-word matches only.  The checker is always the CPU oracle's records passed
through tests/wordref.py (then tests/llref.py / tests/replref.py for the passes behind the filter), never the device's
own output.  Integer work: bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest

import wordfuzz
import wordref
from docref import random_offsets
from heapguard import GuardedBuffer, heap_runs
from llref import greedy, line_lengths
from orc import Oracle, match_checksum
from phfpfac_amd import GpuMatcher, PfacError, PfacTable, _ffi, emit_packed, word_set
from phfpfac_amd.matcher import splitmix64_bytes, tiled_bytes
from replref import greedy_replace, rep_table

pytestmark = pytest.mark.gpu

TILE = 4096
N = 65536 + 123
A, DOT = ord("a"), ord(".")


def para_bytes(resolve, n):
    return tiled_bytes(n, open(resolve("paragraph402"), "rb").read())


def oracle_records(path, buf, n_owned=None):
    """(pos, ids, lens) of the CPU oracle's scan of buf, start offsets below n_owned."""
    o = Oracle(path, 1, 1)
    pos, ids = o.scan_spec(np.ascontiguousarray(buf))
    o.close()
    if n_owned is not None:
        own = pos < n_owned
        pos, ids = pos[own], ids[own]
    return pos, ids, line_lengths(path)[ids]


def text_of(pos, ids, base=0):
    return "".join("At position %4d, match pattern %d\n" % (p + base, i) for p, i in zip(pos.tolist(), ids.tolist())).encode()


def assert_records(table, rec, pos, ids, what="records"):
    assert rec.size == pos.size, f"{what}: {rec.size} records, want {pos.size}"
    np.testing.assert_array_equal(rec["pos"].astype(np.int64), pos, err_msg=what)
    np.testing.assert_array_equal(table.idmap[rec["state"]], ids, err_msg=what)


def scan(g, buf, n_owned=None):
    n_owned = buf.size if n_owned is None else n_owned
    g.reserve(0, max(buf.size, 1), max(buf.size // 8, 4096))
    if buf.size:
        g.h2d(buf)
    return g.scan_resident(n_owned, buf.size)


def status_of(fn):
    with pytest.raises(PfacError) as e:
        fn()
    return e.value.status


def pattern_file(tmp_path, lines, name="p.pat"):
    pf = tmp_path / name
    pf.write_bytes(b"".join(p + b"\n" for p in lines))
    return str(pf)


# ---------------------------------------------------------------------------
# record widths and kernel variants: every reader of the scan after the filter

VARIANTS = [("experimentpattern", {}, 2), ("xaa", {}, 4), ("xaa+xab+xac+xad", {}, 4), ("xaa+xab+xac+xad", {"PFAC_WIDE": "1"}, 8),
            ("xaa+xab+xac+xad", {"PFAC_DENSE": "1"}, 4), ("xaa+xab+xac+xad", {"PFAC_FORCE_L2": "1"}, 4),
            ("xaa+xab+xac+xad", {"PFAC_DENSE": "1", "PFAC_FORCE_L2": "1"}, 4)]


@pytest.mark.parametrize("pat,env,width", VARIANTS, ids=[f"{p}-{'+'.join(e) or 'default'}" for p, e, _ in VARIANTS])
def test_every_reader_sees_the_filtered_scan(pat, env, width, resolve, monkeypatch, tmp_path):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    buf = para_bytes(resolve, N)
    path = resolve(pat)
    pos, ids, lens = oracle_records(path, buf)
    keep = wordref.filter_words(buf, pos, lens)
    assert 0 < keep.sum() < pos.size / 2
    if pat == "xaa+xab+xac+xad":
        assert np.bincount(pos // TILE).max() > 1700           # the compaction of one tile runs over many chunks
    kpos, kids = pos[keep], ids[keep]
    table = PfacTable.from_file(path, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.scan_bytes(buf)                                       # (a first scan, so that the adapted staging is what runs)
        assert scan(g, buf) == pos.size
        fmt = g.scan_format()
        assert fmt[0] == width
        n = g.filter_whole_words()
        assert n == kpos.size and g.last_count() == n
        assert g.scan_format() == fmt
        assert_records(table, g.records_to_host(n), kpos, kids)
        want_text = text_of(kpos, kids, 7)
        if width != 8:
            words, tix = g.packed_to_host()
            out = tmp_path / "packed.txt"
            emit_packed(str(out), words, tix, table.idmap, base=7)
            assert out.read_bytes() == want_text
        assert g.text_to_host(g.emit_text_device(7)) == want_text
        assert g.checksum(n, base=7) == match_checksum(kpos + 7, kids)


# ---------------------------------------------------------------------------
# edges

def test_words_around_tile_boundaries(resolve, tmp_path):
    """`aa` / `aaa` as words of their own starting at 4096k - 1, 4096k and 4096k + 1, and glued to a word there."""
    path = resolve("experimentpattern")
    table = PfacTable.from_file(path, 256)
    rng = np.random.default_rng(1)
    for glue in (False, True):
        buf = np.full(6 * TILE + 50, DOT, dtype=np.uint8)
        for k, d in ((1, -1), (2, 0), (3, 1), (4, -3), (5, -2)):
            at = k * TILE + d
            buf[at:at + 3] = A
            if glue:
                buf[at - 1 if k % 2 else at + 3] = ord("b")
        buf[rng.integers(0, buf.size, 40)] = A
        pos, ids, lens = oracle_records(path, buf)
        for edges, name in wordfuzz.EDGES.items():
            keep = wordref.filter_words(buf, pos, lens, edges=edges)
            with GpuMatcher(0, 1) as g:
                g.load_table(table)
                g.set_final_lengths(table.final_lengths())
                scan(g, buf)
                n = g.filter_whole_words(edges=name)
                assert_records(table, g.records_to_host(n), pos[keep], ids[keep], f"glue {glue} edges {name}")
        assert 0 < wordref.filter_words(buf, pos, lens).sum() < pos.size


@pytest.mark.parametrize("nb", [-1, A, DOT])
def test_first_and_last_byte_with_neighbours(nb, resolve, tmp_path):
    """A match at pos 0 and one that ends at n_avail, with no byte, a word byte and a non-word byte outside."""
    path = pattern_file(tmp_path, [b"cat", b"he", b"the cat", b"at"])
    table = PfacTable.from_file(path, 256)
    buf = np.frombuffer(b"cat on the mat, the cat", dtype=np.uint8)
    pos, ids, lens = oracle_records(path, buf)
    assert pos[0] == 0 and (pos + lens == buf.size).any()
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        for prev, nxt in ((nb, -1), (-1, nb), (nb, nb)):
            keep = wordref.filter_words(buf, pos, lens, prev=prev, next=nxt)
            scan(g, buf)
            n = g.filter_whole_words(prev_byte=prev, next_byte=nxt)
            assert_records(table, g.records_to_host(n), pos[keep], ids[keep], f"prev {prev} next {nxt}")
            assert keep[0] == (prev != A) and keep[pos + lens == buf.size].any() == (nxt != A)


def test_owned_range_with_a_halo(resolve):
    """n_owned < n_avail: the byte behind a match that ends in the halo is the buffer's, not next_byte."""
    path = resolve("xaa")
    table = PfacTable.from_file(path, 256)
    buf = para_bytes(resolve, 3 * TILE + 777)
    n_owned = 2 * TILE + 5
    pos, ids, lens = oracle_records(path, buf, n_owned)
    assert (pos + lens > n_owned).any()
    keep = wordref.filter_words(buf, pos, lens, next=A)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        assert scan(g, buf, n_owned) == pos.size
        n = g.filter_whole_words(next_byte=A)
        assert_records(table, g.records_to_host(n), pos[keep], ids[keep])
        assert g.scan_bytes(buf, n_owned, whole_words=True, next_byte=A).size == n


def test_runs_of_a_and_separated_a(resolve):
    """Only `a`: every tile drops to count 0 (and stays there); `a a a ...`: the single `a`s all stay."""
    path = resolve("experimentpattern")
    table = PfacTable.from_file(path, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        buf = np.full(3 * TILE + 11, A, dtype=np.uint8)
        total = scan(g, buf)
        assert total == 4 * buf.size - 6
        assert g.filter_whole_words(prev_byte=A) == 0
        _, tix = g.packed_to_host()
        assert (heap_runs(tix)[1] == 0).all()
        assert g.records_to_host(0).size == 0 and g.emit_text_device() == 0 and g.checksum(0) == 0
        assert g.filter_whole_words() == 0
        n_sel, ex = g.select_leftmost_longest(0)
        assert (n_sel, ex) == (0, 0)
        # the whole buffer is one word `aaa...a`: without neighbours only a match of all of it would stay
        scan(g, buf)
        assert g.filter_whole_words(edges="left") == 4 and g.filter_whole_words(edges="right") == 0
        buf = np.tile(np.frombuffer(b"a ", dtype=np.uint8), TILE + 3)
        assert scan(g, buf) == buf.size // 2
        assert g.filter_whole_words() == buf.size // 2
        rec = g.records_to_host(buf.size // 2)
        assert (rec["pos"] == np.arange(0, buf.size, 2)).all()


def test_scan_without_matches(resolve, tmp_path):
    path = pattern_file(tmp_path, [b"zebra"])
    table = PfacTable.from_file(path, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        for n in (0, 1, 2 * TILE + 1):
            assert scan(g, np.full(n, DOT, dtype=np.uint8)) == 0
            assert g.filter_whole_words() == 0
            assert g.scan_finish()[0] == 0


def test_custom_word_set_on_random_bytes(resolve, tmp_path):
    """UTF-8 style: bytes 0x80..0xFF are word bytes too; splitmix64 bytes, short binary patterns."""
    buf = splitmix64_bytes(5 * TILE + 99, 0x5048465046414331)
    lines = [bytes(buf[i:i + k]) for i, k in ((10, 1), (500, 2), (9000, 2), (12000, 3), (20000, 1), (20479, 2))]
    lines = [p for p in lines if b"\n" not in p] + [b"\xc3", b"a", b" "]
    path = pattern_file(tmp_path, sorted(set(lines)))
    table = PfacTable.from_file(path, 256)
    chars = wordref.DEFAULT_WORD + bytes(range(0x80, 0x100))
    pos, ids, lens = oracle_records(path, buf)
    keep = wordref.filter_words(buf, pos, lens, word_set(chars))
    assert 0 < keep.sum() < pos.size
    assert not np.array_equal(keep, wordref.filter_words(buf, pos, lens))
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        scan(g, buf)
        n = g.filter_whole_words(word_bytes=chars)
        assert_records(table, g.records_to_host(n), pos[keep], ids[keep])
        assert_records(table, g.scan_bytes(buf, whole_words=chars), pos[keep], ids[keep], "scan_bytes(whole_words=bytes)")
        scan(g, buf)
        assert g.filter_whole_words(word_bytes=word_set(chars)) == n


# ---------------------------------------------------------------------------
# chaining

def test_chained_ranges_equal_one_call(resolve):
    """300 001 bytes in three owned ranges with a max_pat_len halo, the neighbours' bytes and entry / exit passed on."""
    path = resolve("xaa+xab+xac+xad")
    table = PfacTable.from_file(path, 256)
    buf = para_bytes(resolve, 300_001)
    n = buf.size
    pos, ids, lens = oracle_records(path, buf)
    keep = wordref.filter_words(buf, pos, lens)
    kpos, kids, klens = pos[keep], ids[keep], lens[keep]
    pick, wex = greedy(kpos, klens, 0, n)
    cuts = [0, 100_003, 100_003 + 2 * TILE, n]
    assert wordref.cuts(buf)[cuts[1]]                          # the first cut falls inside a word
    M = table.max_pat_len
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_redaction(b"*")
        reps = {i: b"*" * int(l) for i, l in enumerate(line_lengths(path)) if i}
        whole, ex = g.scan_leftmost_longest(buf, whole_words=True)
        assert_records(table, whole, kpos[pick], kids[pick], "selection of the whole")
        assert ex == wex
        out, _ = g.replace(buf, whole_words=True)
        want, _ = greedy_replace(buf, 0, n, kpos, klens, kids, rep_table(reps))
        assert np.array_equal(out, want)
        unfiltered, _ = g.scan_leftmost_longest(buf)
        assert unfiltered.size > whole.size                    # in-word hits further left did shadow real words
        sel, outs, entry, entry2 = [], [], 0, 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            avail = min(b + M, n)
            part = np.ascontiguousarray(buf[a:avail])
            kw = dict(whole_words=True, prev_byte=int(buf[a - 1]) if a else -1, next_byte=int(buf[avail]) if avail < n else -1)
            r, entry = g.scan_leftmost_longest(part, b - a, entry, **kw)
            r["pos"] += a
            sel.append(r)
            o, entry2 = g.replace(part, b - a, entry2, **kw)
            outs.append(o)
        assert_records(table, np.concatenate(sel), kpos[pick], kids[pick], "chained selection")
        assert entry == wex and entry2 == wex
        assert np.array_equal(np.concatenate(outs), want)


# ---------------------------------------------------------------------------
# documents

def per_document(path, buf, off, table_ids=True):
    """Every document scanned, filtered and selected on its own by the references:
    (doc_first, pos, ids) of the kept records, (doc_first, pos, ids) of the picks, the redacted documents."""
    o = Oracle(path, 1, 1)
    ll = line_lengths(path)
    reps = rep_table({i: b"*" * int(l) for i, l in enumerate(ll) if i})
    kf, kp, ki, sf, sp_, si, outs = [0], [], [], [0], [], [], []
    for a, b in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64)):
        doc = np.ascontiguousarray(buf[a:b])
        if b > a:
            pos, ids = o.scan_spec(doc)
            lens = ll[ids]
            keep = wordref.filter_words(doc, pos, lens)
            pos, ids, lens = pos[keep], ids[keep], lens[keep]
            pick, _ = greedy(pos, lens, 0, b - a)
            out, _ = greedy_replace(doc, 0, b - a, pos, lens, ids, reps)
            kp.append(pos); ki.append(ids); sp_.append(pos[pick]); si.append(ids[pick]); outs.append(out)
        kf.append(kf[-1] + (kp[-1].size if b > a else 0))
        sf.append(sf[-1] + (sp_[-1].size if b > a else 0))
    o.close()
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.empty(0, dt)
    return ((np.array(kf, np.uint64), cat(kp, np.int64), cat(ki, np.int32)),
            (np.array(sf, np.uint64), cat(sp_, np.int64), cat(si, np.int32)), outs)


def check_documents(path, buf, off):
    table = PfacTable.from_file(path, 256)
    kept, picks, outs = per_document(path, buf, off)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_redaction(b"*")
        first, rec = g.scan_documents((buf, off), whole_words=True)
        np.testing.assert_array_equal(first, kept[0])
        assert_records(table, rec, kept[1], kept[2], "scan_documents")
        first, rec = g.select_documents((buf, off), whole_words=True)
        np.testing.assert_array_equal(first, picks[0])
        assert_records(table, rec, picks[1], picks[2], "select_documents")
        out_off, out = g.replace_documents((buf, off), whole_words=True)
        want = np.concatenate(outs) if outs else np.empty(0, np.uint8)
        assert np.array_equal(out, want)
        np.testing.assert_array_equal(out_off, np.concatenate([[0], np.cumsum(np.diff(off.astype(np.int64)))]).astype(np.uint64))
        plain_first, plain = g.scan_documents((buf, off))
    return kept[1].size, plain.size


def test_documents_cut_mid_word(resolve):
    """1 MiB of text cut at random places: document ends are word boundaries (the lane-window path of doc_lookup)."""
    buf = para_bytes(resolve, 1 << 20)
    off = random_offsets(np.random.default_rng(21), buf.size, 1200, empties=20)
    assert wordref.cuts(buf)[off[1:-1].astype(np.int64)].sum() > 300
    kept, plain = check_documents(resolve("xaa"), buf, off)
    assert 0 < kept < plain / 2


def test_edge_documents(resolve):
    """The layout of test_gpu_documents.test_edge_documents: empty documents first, last and in runs, 5 000 documents
    inside one tile (the binary-search path of doc_lookup), boundaries at 4096k - 1, 4096k, 4096k + 1."""
    buf = para_bytes(resolve, N)
    n = buf.size
    cuts = [0, 0, 0, 10, 10, 10, 10, 500]
    t1 = 4 * TILE
    cuts += [t1 + i for i in range(4000)] + [t1 + 4000] * 1000
    for k in (6, 7, 9, 12):
        cuts += [k * TILE - 1, k * TILE, k * TILE + 1]
    cuts += [13 * TILE] * 3 + [n, n, n]
    off = np.array(sorted(cuts), dtype=np.uint64)
    for pat in ("xaa", "experimentpattern"):
        kept, plain = check_documents(resolve(pat), buf, off)
        assert 0 < kept < plain


def test_bad_offsets_leave_the_scan_unfiltered(resolve):
    path = resolve("xaa")
    table = PfacTable.from_file(path, 256)
    buf = para_bytes(resolve, 20_000)
    pos, ids, lens = oracle_records(path, buf)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        total = scan(g, buf)
        for bad in ([0, 12_000, 11_000, 20_000], [1, 10_000, 20_000], [0, 10_000, 19_999], [0, 10_000, 20_001]):
            g.set_doc_offsets(np.array(bad, dtype=np.uint64))
            assert status_of(lambda: g.filter_whole_words(n_docs=len(bad) - 1)) == _ffi.PFAC_E_ARG
            assert g.scan_finish()[0] == total
            assert_records(table, g.records_to_host(total), pos, ids, "after refused offsets")
        g.set_doc_offsets(np.array([0, 20_000], dtype=np.uint64))
        assert status_of(lambda: g.filter_whole_words(n_docs=2)) == _ffi.PFAC_E_STATE     # not the slot's n_docs
        assert g.filter_whole_words(n_docs=1) == int(wordref.filter_words(buf, pos, lens).sum())
        # The offsets' check with no tiles behind it: a scan of zero bytes owns none, so every offset must be 0.  n_docs on
        # both sides of one workgroup of the check and above its grid of 4096 x 256 threads (the stride loop runs twice);
        # the broken rule first in thread 0's offsets, then in the last thread's (a decreasing pair needs two documents).
        assert scan(g, np.zeros(0, dtype=np.uint8)) == 0
        for n_docs in (1, 256, 257, 4096 * 256 + 300):
            for k in (0, n_docs - 1) if n_docs > 1 else (0,):
                off = np.zeros(n_docs + 1, dtype=np.uint64)
                off[k] = 1                                      # k = 0: off[0] != 0; else off[k] > off[k + 1]
                g.set_doc_offsets(off)
                assert status_of(lambda: g.filter_whole_words(n_docs=n_docs)) == _ffi.PFAC_E_ARG
                assert status_of(lambda: g.select_leftmost_longest_documents(n_docs)) == _ffi.PFAC_E_ARG
                assert g.scan_finish()[0] == 0
            g.set_doc_offsets(np.zeros(n_docs + 1, dtype=np.uint64))
            assert g.filter_whole_words(n_docs=n_docs) == 0
            assert g.select_leftmost_longest_documents(n_docs) == 0


# ---------------------------------------------------------------------------
# the contract

def test_state_overflow_and_argument_errors(resolve):
    path = resolve("xaa")
    table = PfacTable.from_file(path, 256)
    other = PfacTable.from_file(resolve("experimentpattern"), 256)
    buf = para_bytes(resolve, 20_000)
    E_STATE, E_ARG, E_OVERFLOW = _ffi.PFAC_E_STATE, _ffi.PFAC_E_ARG, _ffi.PFAC_E_OVERFLOW
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        assert status_of(g.filter_whole_words) == E_STATE                                  # no scan at all
        g.reserve(0, buf.size, 1 << 16)
        g.h2d(buf)
        g.scan_async(buf.size)
        assert status_of(g.filter_whole_words) == E_STATE                                  # before scan_finish
        total, _ = g.scan_finish()
        assert status_of(g.filter_whole_words) == E_STATE                                  # no final lengths
        g.set_final_lengths(table.final_lengths())
        for edges in (0, 4):
            n = C.c_uint64(0)
            rc = g._L.pfac_records_filter_words(g._ctx, 0, None, None, None, edges, -1, -1, None, 0, C.byref(n))
            assert rc == E_ARG
        assert status_of(lambda: g.filter_whole_words(prev_byte=256)) == E_ARG
        assert status_of(lambda: g.filter_whole_words(next_byte=-2)) == E_ARG
        assert status_of(lambda: g.filter_whole_words(d_records=g.records_ptr() + 16)) == E_ARG
        assert status_of(lambda: g.filter_whole_words(d_input=g.input_ptr() + 4)) == E_ARG
        assert g.scan_finish()[0] == total                                                 # nothing was filtered so far
        # a selection made before the filter is stale
        g.set_redaction(b"*")
        g.select_leftmost_longest(0)
        kept = g.filter_whole_words()
        assert 0 < kept < total
        assert status_of(g.replace_selection) == E_STATE
        g.select_leftmost_longest(0)
        assert g.replace_selection() == buf.size
        # the count: a repeated scan_finish, the bounds of the record fetch
        assert g.scan_finish()[0] == kept
        assert status_of(lambda: g.records_to_host(1, first=kept)) == E_ARG
        rec = g.records_to_host(kept)
        assert g.filter_whole_words() == kept                                              # a second, identical filter
        assert np.array_equal(g.records_to_host(kept), rec)
        # a table upload: the scan ran with an earlier table
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        assert status_of(g.filter_whole_words) == E_STATE
        g.load_table(other)
        g.scan_bytes(buf)
        assert status_of(g.filter_whole_words) == E_STATE                                  # lengths never set for it
        # a reserve that dropped the scan
        g.set_final_lengths(other.final_lengths())
        assert g.filter_whole_words() > 0
        g.reserve(0, 0, 1 << 22)
        assert status_of(g.filter_whole_words) == E_STATE
        # an overflowed scan
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        import torch
        heap = torch.zeros(64 * 4, dtype=torch.uint8, device="cuda:0")
        g.h2d(buf)
        g.scan_async(buf.size, d_records=heap, capacity=64)
        assert g.scan_finish(allow_overflow=True)[1]
        assert status_of(lambda: g.filter_whole_words(d_records=heap)) == E_OVERFLOW


def test_left_then_right_is_both(resolve):
    path = resolve("xaa")
    table = PfacTable.from_file(path, 256)
    buf = para_bytes(resolve, N)
    pos, ids, lens = oracle_records(path, buf)
    both = wordref.filter_words(buf, pos, lens)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        scan(g, buf)
        left = g.filter_whole_words(edges="left")
        assert left == int(wordref.filter_words(buf, pos, lens, edges=wordref.LEFT).sum()) > both.sum()
        n = g.filter_whole_words(edges="right")
        assert_records(table, g.records_to_host(n), pos[both], ids[both])


# ---------------------------------------------------------------------------
# writes stay home

@pytest.mark.parametrize("pat,env,width", [("experimentpattern", {}, 2), ("xaa+xab+xac+xad", {}, 4),
                                           ("xaa+xab+xac+xad", {"PFAC_WIDE": "1"}, 8)], ids=["2", "4", "8"])
def test_writes_stay_inside_the_tiles_runs(pat, env, width, resolve, monkeypatch):
    """The scan goes into a guarded heap of exactly the hinted capacity; the filter may change nothing but the words of
    the tiles' own runs [FIRST, FIRST + old COUNT)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    path = resolve(pat)
    table = PfacTable.from_file(path, 256)
    buf = para_bytes(resolve, N)
    pos, ids, lens = oracle_records(path, buf)
    keep = wordref.filter_words(buf, pos, lens)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        scan(g, buf)
        cap = g.capacity_hint()
        heap = GuardedBuffer(cap * width)
        g.scan_async(buf.size, d_records=heap.ptr, capacity=cap)
        total, over = g.scan_finish()
        rb, n_tiles, used = g.scan_format()
        assert (rb, total, over) == (width, pos.size, False)
        before = heap.host().copy()
        counts = np.bincount(pos // TILE, minlength=n_tiles)    # the old COUNT of every tile (the oracle's)
        n = g.filter_whole_words(d_records=heap.ptr)
        g.sync()
        heap.check(what="the record heap after the filter")
        after = heap.host()
        assert_records(table, g.records_to_host(n, d_records=heap.ptr), pos[keep], ids[keep])
        if width != 8:
            _, tix = g.packed_to_host(d_records=heap.ptr)
            first, cnt = heap_runs(tix)
            np.testing.assert_array_equal(cnt, np.bincount(pos[keep] // TILE, minlength=n_tiles))
        else:                                                   # no index to fetch: the runs lie where the records did
            r = before[:used * 8].view(np.dtype([("pos", "<u4"), ("state", "<u4")]))
            live = np.flatnonzero(~((r["pos"] == 0xA5A5A5A5) & (r["state"] == 0xA5A5A5A5)))
            assert live.size == pos.size
            first = np.zeros(n_tiles, dtype=np.int64)
            tile = r["pos"][live] // TILE
            start = np.flatnonzero(np.append(True, tile[1:] != tile[:-1]))
            first[tile[start]] = live[start]
        inside = np.zeros(before.size, dtype=bool)
        for f, c in zip(first.tolist(), counts.tolist()):
            inside[f * width:(f + c) * width] = True
        changed = before != after
        assert changed.any() and not (changed & ~inside).any()


# ---------------------------------------------------------------------------
# seeded cases

@pytest.mark.parametrize("seed", wordfuzz.SEEDS)
def test_seeded_cases(seed, tmp_path, monkeypatch):
    case = wordfuzz.WordCase(seed)
    for k in wordfuzz.KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.knobs.items():
        monkeypatch.setenv(k, v)
    wordfuzz.run_word_case(lambda: GpuMatcher(0, 1), case, str(tmp_path))
