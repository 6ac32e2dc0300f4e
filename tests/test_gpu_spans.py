"""The span filter, pfac_records_filter_spans / pfac_table_set_state_spans (run with -m gpu on an MI355X): the records of
a finished scan that their pattern's span does not admit -- ^pat, pat$, grep -x, offset / depth -- are dropped in place,
and every consumer of the scan then sees the admissible matches only.  The checker is always the CPU oracle's records
passed through tests/spanref.py (then the references of the passes behind the filter), never the device's own output;
tests/test_span_ref.py pins that reference and the counts relied on here without a GPU.  Integer work: bit-exact."""
import ctypes as C
import re

import numpy as np
import pytest

import spanref
import wordref
from countref import state_counts
from gatherref import gather_ref
from groupref import groups_for, masks_by_id, masks_cut
from heapguard import GuardedBuffer, heap_runs
from llref import greedy, line_lengths
from nocaseref import fold
from orc import Oracle, match_checksum
from phfpfac_amd import GpuMatcher, PfacError, PfacTable, _ffi, emit_packed, strip_anchors
from phfpfac_amd.matcher import tiled_bytes
from replref import greedy_replace, rep_table
from splitref import matching_ids
from test_gpu_whole_words import VARIANTS

pytestmark = pytest.mark.gpu

TILE = 4096
N = 65536 + 123
SP, W, NL = ord(" "), ord("w"), 10
E_STATE, E_ARG, E_OVERFLOW = _ffi.PFAC_E_STATE, _ffi.PFAC_E_ARG, _ffi.PFAC_E_OVERFLOW
DICT = "xaa+xab+xac+xad"


def para_bytes(resolve, n):
    return tiled_bytes(n, open(resolve("paragraph402"), "rb").read())


def oracle_records(path, buf, n_owned=None, escapes=False, lens_by_id=None):
    """(pos, ids, lens) of the CPU oracle's scan of buf, start offsets below n_owned."""
    o = Oracle(path, 1, 1, escapes=escapes)
    pos, ids = o.scan_spec(np.ascontiguousarray(buf))
    o.close()
    if n_owned is not None:
        own = pos < n_owned
        pos, ids = pos[own], ids[own]
    return pos, ids, (line_lengths(path) if lens_by_id is None else np.asarray(lens_by_id, dtype=np.int64))[ids]


def ref_keep(buf, pos, ids, lens, rules, delim=-1, off=None, n_avail=None):
    return spanref.filter_spans(buf, pos, lens, *spanref.record_spans(rules, ids), delim, off, n_avail)


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


def upload(arr):
    import torch
    raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
    t = torch.zeros(max(raw.size, 16), dtype=torch.uint8, device="cuda:0")
    if raw.size:
        t[:raw.size].copy_(torch.from_numpy(raw.copy()))
    torch.cuda.synchronize()
    return t


def matcher(table, rules=None):
    g = GpuMatcher(0, 1)
    g.load_table(table)
    g.set_final_lengths(table.final_lengths())
    if rules is not None:
        g.set_pattern_spans(rules)
    return g


def filtered(g, buf, delim, off=None, n_owned=None, line=False):
    """Scan buf, cut it (off None and delim >= 0: on the device at delim; off: the caller's, as the slot's), filter."""
    total = scan(g, buf, n_owned)
    if off is None and delim >= 0:
        n_docs, _ = g.split_documents(buf.size, delim)
    elif off is not None:
        g.set_doc_offsets(off)
        n_docs = off.size - 1
    else:
        n_docs = 0
    return total, g.filter_spans(delimiter=None if delim < 0 else delim, line_match=line, n_docs=n_docs)


# ---------------------------------------------------------------------------
# record widths and kernel variants: every reader of the scan after the filter

@pytest.mark.parametrize("pat,env,width", VARIANTS, ids=[f"{p}-{'+'.join(e) or 'default'}" for p, e, _ in VARIANTS])
def test_every_reader_sees_the_filtered_scan(pat, env, width, resolve, monkeypatch, tmp_path):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    buf = para_bytes(resolve, N)
    path = resolve(pat)
    pos, ids, lens = oracle_records(path, buf)
    rules = spanref.drawn_rules(line_lengths(path))
    off = spanref.split_offsets(buf, SP)
    keep = ref_keep(buf, pos, ids, lens, rules, SP, off)
    assert 0 < keep.sum() < pos.size
    if pat == DICT:
        assert np.bincount(pos // TILE).max() > 1700           # the compaction of one tile runs over many chunks
    kpos, kids = pos[keep], ids[keep]
    table = PfacTable.from_file(path, 256)
    assert (table.num_final <= 64) == (pat == "experimentpattern")         # spans in lane registers / gathered
    with matcher(table, rules) as g:
        g.scan_bytes(buf)                                       # (a first scan, so that the adapted staging is what runs)
        assert scan(g, buf) == pos.size
        fmt = g.scan_format()
        assert fmt[0] == width
        n_docs, _ = g.split_documents(buf.size, SP)
        assert n_docs == off.size - 1
        n = g.filter_spans(delimiter=b" ", n_docs=n_docs)
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
# both document lookups

@pytest.mark.parametrize("delim,lo,hi,want", [(SP, 63, 646, (11266, 10454, 5716, 0)), (W, 1, 53, (816, 164, 0, 1305))],
                         ids=["memory-search", "lane-window"])
def test_both_document_lookups(delim, lo, hi, want, resolve):
    """Delimiter ` `: up to 646 documents start in one tile (the binary search in memory); `w`: at most 53 (the lane
    window), and 1 305 records run across their document's end."""
    path = resolve(DICT)
    buf = para_bytes(resolve, N)
    pos, ids, lens = oracle_records(path, buf)
    off = spanref.split_offsets(buf, delim)
    starts = np.bincount(off[:-1] // TILE)
    assert lo <= starts.max() == hi and (delim == SP or starts.max() + 2 <= 64)
    d = np.searchsorted(off, pos, side="right") - 1
    assert int((pos + lens > off[d + 1]).sum()) == want[3]
    table = PfacTable.from_file(path, 256)
    n_ids = line_lengths(path).size
    drawn = spanref.drawn_rules(line_lengths(path))
    with matcher(table) as g:
        for rules, count in (([None] + ["^"] * (n_ids - 1), want[0]), ([None] + ["$"] * (n_ids - 1), want[1]),
                             ([None] + ["^$"] * (n_ids - 1), want[2]), (drawn, None)):
            keep = ref_keep(buf, pos, ids, lens, rules, delim, off)
            assert count is None or int(keep.sum()) == count
            g.set_pattern_spans(rules)
            total, n = filtered(g, buf, delim)
            assert total == pos.size
            assert_records(table, g.records_to_host(n), pos[keep], ids[keep], f"delimiter {delim} rules {rules[1]}")
        # a record that runs across its document's end: its start rule is judged as usual, every judged tail drops it
        cross = pos + lens > off[d + 1]
        keep = ref_keep(buf, pos, ids, lens, [None] + [(None, None, 1 << 20)] * (n_ids - 1), delim, off)
        assert np.array_equal(keep, ~cross)
        g.set_pattern_spans([None] + [(None, None, 1 << 20)] * (n_ids - 1))
        _, n = filtered(g, buf, delim)
        assert_records(table, g.records_to_host(n), pos[keep], ids[keep], "a huge max_tail")


# ---------------------------------------------------------------------------
# edges

def test_documents_around_tile_boundaries(tmp_path):
    """Caller-made offsets with documents that start at 4096k - 1, 4096k and 4096k + 1, `cat` at each document's start
    and `hat` at its end, both also elsewhere; no delimiter.  The caller's device offsets and the slot's own."""
    path = pattern_file(tmp_path, [b"cat", b"hat", b"at"])
    table = PfacTable.from_file(path, 256)
    rules = [None, "^", "$", (1, None, 0)]
    buf = np.full(14 * TILE + 50, ord("."), dtype=np.uint8)
    cuts = [0]
    for k, d in ((1, -1), (2, 0), (3, 1), (5, -1), (5, 0), (5, 1), (9, 0), (9, 0), (12, 1)):
        cuts.append(k * TILE + d)
    cuts.append(buf.size)
    off = np.array(sorted(cuts), dtype=np.uint64)
    rng = np.random.default_rng(4)
    for at in rng.integers(8, buf.size - 8, 300):
        buf[at:at + 3] = np.frombuffer(b"cat" if at % 2 else b"hat", dtype=np.uint8)
    for a, b in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64)):
        if b - a >= 6:
            buf[a:a + 3] = np.frombuffer(b"cat", dtype=np.uint8)
            buf[b - 3:b] = np.frombuffer(b"hat", dtype=np.uint8)
    pos, ids, lens = oracle_records(path, buf)
    keep = ref_keep(buf, pos, ids, lens, rules, -1, off)
    n_docs = off.size - 1
    assert keep.sum() >= 3 * int((np.diff(off.astype(np.int64)) >= 6).sum()) >= 21 and (~keep).sum() > 300
    d_off = upload(off)
    with matcher(table, rules) as g:
        scan(g, buf)
        n = g.filter_spans(n_docs=n_docs, d_doc_offsets=d_off)
        assert_records(table, g.records_to_host(n), pos[keep], ids[keep], "caller's offsets")
        total, n = filtered(g, buf, -1, off)
        assert_records(table, g.records_to_host(n), pos[keep], ids[keep], "the slot's offsets")
        assert (total, n) == (pos.size, int(keep.sum()))


def test_document_straddles_the_group_edge(resolve):
    """65 tiles + 17 bytes: two groups of 64 tiles (not a multiple of the four a workgroup takes), and a document that
    runs across the groups' edge at 256 KiB."""
    path = resolve("xaa")
    buf = para_bytes(resolve, 65 * TILE + 17)
    edge = 64 * TILE
    off = spanref.split_offsets(buf, SP)
    off = off[(off <= edge - 300) | (off >= edge + 300)]
    d = np.searchsorted(off, edge, side="right") - 1
    assert off[d] < edge - 250 and off[d + 1] > edge + 250
    pos, ids, lens = oracle_records(path, buf)
    rules = spanref.drawn_rules(line_lengths(path))
    keep = ref_keep(buf, pos, ids, lens, rules, SP, off)
    inside = (pos >= off[d]) & (pos < off[d + 1])
    assert (pos[inside] < edge).any() and (pos[inside] >= edge).any() and 0 < keep[inside].sum() < inside.sum()
    table = PfacTable.from_file(path, 256)
    with matcher(table, rules) as g:
        total, _ = filtered(g, buf, SP, off.astype(np.uint64))
        # (filtered() passes the delimiter with the caller's offsets: C = E - 1 where a document ends in a blank)
        n_tiles = g.scan_format()[1]
        assert n_tiles == 66 and (n_tiles + 63) // 64 == 2      # (the 17 bytes are a tile of their own)
        n = g.last_count()
        assert (total, n) == (pos.size, int(keep.sum()))
        assert_records(table, g.records_to_host(n), pos[keep], ids[keep])


def test_delimiter_runs_empty_documents_and_covered_delimiters(tmp_path):
    """Runs of delimiters (documents of their delimiter alone), empty documents in caller offsets, an unterminated
    against a terminated last line under `$`, and a pattern that ends in the delimiter (an escaped file): tail 0."""
    pf = tmp_path / "e.pat"
    pf.write_bytes(b"foo\nfoo\\n\n\\nfoo\nbar\n")
    lens_by_id = [0, 3, 4, 4, 3]
    table = PfacTable.from_file(str(pf), 256, escapes=True)
    rules = [None, "$", "$", "^$", "^"]
    rng = np.random.default_rng(8)
    pieces = [b"foo", b"bar", b"foo bar", b"bar foo", b"", b"", b"xfoo", b"foox", b"barfoo"]
    for terminated in (True, False):
        raw = b"\n".join(pieces[k] for k in rng.integers(0, len(pieces), 3000)) + b"\nfoo" + (b"\n" if terminated else b"")
        assert b"\n\n\n" in raw
        buf = np.frombuffer(raw, dtype=np.uint8)
        pos, ids, lens = oracle_records(str(pf), buf, escapes=True, lens_by_id=lens_by_id)
        assert set(ids.tolist()) == {1, 2, 3, 4}
        off = spanref.split_offsets(buf, NL)
        assert (np.diff(off) == 1).sum() > 100                   # documents of their delimiter alone
        keep = ref_keep(buf, pos, ids, lens, rules, NL, off)
        last = pos == buf.size - (4 if terminated else 3)
        assert keep[last & (ids == 1)].all() and (keep[last & (ids == 2)].size == int(terminated))
        assert keep[ids == 2].all() and (ids == 2).sum() > 500   # `foo\n` covers the delimiter: tail 0
        assert not keep[ids == 3].any()                         # `\nfoo` starts in the line before: it crosses
        assert 0 < keep[ids == 1].sum() < (ids == 1).sum() and 0 < keep[ids == 4].sum() < (ids == 4).sum()
        with matcher(table, rules) as g:
            total, n = filtered(g, buf, NL)
            assert_records(table, g.records_to_host(n), pos[keep], ids[keep], f"split, terminated {terminated}")
            # the same cut with empty documents put in by the caller
            more = np.sort(np.concatenate([off, off[rng.integers(0, off.size, 200)], [0, 0, buf.size, buf.size]])).astype(np.uint64)
            assert np.array_equal(ref_keep(buf, pos, ids, lens, rules, NL, more), keep)
            total, n = filtered(g, buf, NL, more)
            assert_records(table, g.records_to_host(n), pos[keep], ids[keep], f"empty documents, terminated {terminated}")
            # no delimiter: `$` is the document's very end
            keep = ref_keep(buf, pos, ids, lens, rules, -1, off)
            assert keep[ids == 2].all() and not keep[(ids == 1) & ~last].any()
            total, n = filtered(g, buf, -1, off.astype(np.uint64))
            assert_records(table, g.records_to_host(n), pos[keep], ids[keep], f"delimiter -1, terminated {terminated}")


def test_no_documents_with_a_halo(resolve, tmp_path):
    """n_docs == 0, n_owned < n_avail: one document [0, n_avail), with and without a delimiter at its end."""
    path = pattern_file(tmp_path, [b"the", b"he", b"cat", b"at"])
    table = PfacTable.from_file(path, 256)
    rules = [None, "^", (1, 1, None), "$", (None, None, 1)]
    for raw in (b"the cat on the mat, the cat", b"the cat on the mat, the cat\n", b"the cat on the mat, the cat."):
        buf = np.frombuffer(raw, dtype=np.uint8)
        n_owned = 26                                            # `cat` at 24 and `at` at 25 end in the halo
        pos, ids, lens = oracle_records(path, buf, n_owned)
        assert (pos + lens > n_owned).any()
        keep = ref_keep(buf, pos, ids, lens, rules, NL, None, buf.size)
        with matcher(table, rules) as g:
            assert scan(g, buf, n_owned) == pos.size
            n = g.filter_spans(delimiter=b"\n")
            assert_records(table, g.records_to_host(n), pos[keep], ids[keep], repr(raw))
        kept = set(zip(pos[keep].tolist(), ids[keep].tolist()))
        assert ((0, 1) in kept) and ((1, 2) in kept) and ((24, 3) in kept) == (raw[-1:] != b".") and ((25, 4) in kept)


# ---------------------------------------------------------------------------
# composition and the passes behind the filter

def test_composes_with_the_whole_word_filter(resolve):
    path = resolve("xaa")
    table = PfacTable.from_file(path, 256)
    buf = para_bytes(resolve, N)
    pos, ids, lens = oracle_records(path, buf)
    rules = spanref.drawn_rules(line_lengths(path))
    off = spanref.split_offsets(buf, W)
    spans = ref_keep(buf, pos, ids, lens, rules, W, off)
    words = wordref.filter_words(buf, pos, lens, off=off)
    both = spans & words
    assert 0 < both.sum() < min(spans.sum(), words.sum())
    with matcher(table, rules) as g:
        for order in ("spans first", "words first"):
            scan(g, buf)
            n_docs, _ = g.split_documents(buf.size, W)
            if order == "spans first":
                assert g.filter_spans(delimiter=W, n_docs=n_docs) == int(spans.sum())
                n = g.filter_whole_words(n_docs=n_docs)
            else:
                assert g.filter_whole_words(n_docs=n_docs) == int(words.sum())
                n = g.filter_spans(delimiter=W, n_docs=n_docs)
            assert_records(table, g.records_to_host(n), pos[both], ids[both], order)
            rec = g.records_to_host(n)
            words_before, tix_before = g.packed_to_host()
            assert g.filter_spans(delimiter=W, n_docs=n_docs) == n              # a second, identical call
            words_after, tix_after = g.packed_to_host()
            assert np.array_equal(g.records_to_host(n), rec)
            assert np.array_equal(words_before, words_after) and np.array_equal(tix_before, tix_after)


def test_selection_made_before_the_filter_is_stale(resolve):
    path = resolve("xaa")
    table = PfacTable.from_file(path, 256)
    buf = para_bytes(resolve, 20_000)
    with matcher(table, spanref.drawn_rules(line_lengths(path))) as g:
        g.set_redaction(b"*")
        total = scan(g, buf)
        n_docs, _ = g.split_documents(buf.size, SP)
        g.select_leftmost_longest(0)
        assert 0 < g.filter_spans(delimiter=SP, n_docs=n_docs) < total
        assert status_of(g.replace_selection) == E_STATE
        g.select_leftmost_longest(0)
        assert g.replace_selection() == buf.size
        scan(g, buf)
        g.select_leftmost_longest_documents(n_docs)
        assert g.filter_spans(delimiter=SP, line_match=True, n_docs=n_docs) > 0
        assert status_of(g.replace_selection_documents) == E_STATE
        g.select_leftmost_longest_documents(n_docs)
        assert g.replace_selection_documents() == buf.size


def test_passes_behind_the_filter(resolve):
    """Segment, per-document selection and replace, count_states, group masks, matching documents and gather: each
    equals its CPU reference on the kept records (some of which run across their document's end)."""
    path = resolve(DICT)
    table = PfacTable.from_file(path, 256)
    buf = para_bytes(resolve, N)
    ll = line_lengths(path)
    pos, ids, lens = oracle_records(path, buf)
    rules = spanref.drawn_rules(ll)
    off = spanref.split_offsets(buf, W)
    n_docs = off.size - 1
    keep = ref_keep(buf, pos, ids, lens, rules, W, off)
    kpos, kids, klens = pos[keep], ids[keep], lens[keep]
    doc = np.searchsorted(off, kpos, side="right") - 1
    fits = kpos + klens <= off[doc + 1]                          # the document cut of the passes
    assert 0 < keep.sum() < pos.size and 0 < fits.sum() < fits.size
    seg_first = np.concatenate([[0], np.cumsum(np.bincount(doc[fits], minlength=n_docs))]).astype(np.uint64)
    reps = rep_table({i: b"*" * int(l) for i, l in enumerate(ll) if i})
    sel_first, sel_pos, sel_ids, outs = [0], [], [], []
    for d_, (a, b) in enumerate(zip(off[:-1], off[1:])):
        mine = fits & (doc == d_)
        p, i, l = kpos[mine] - a, kids[mine], klens[mine]
        pick, _ = greedy(p, l, 0, b - a)
        out, _ = greedy_replace(buf[a:b], 0, b - a, p, l, i, reps)
        sel_pos.append(p[pick]); sel_ids.append(i[pick]); outs.append(out)
        sel_first.append(sel_first[-1] + pick.size)
    groups = groups_for(ll.size - 1)
    want_masks = masks_cut(kpos, kids, klens, off, masks_by_id(groups))
    want_ids = matching_ids(seg_first)
    want_lines, want_line_off = gather_ref(buf, off, want_ids)
    assert 0 < want_ids.size < n_docs and want_masks.any()
    with matcher(table, rules) as g:
        g.set_redaction(b"*")
        g.set_pattern_groups(groups)
        first, rec, offsets = g.scan_lines(buf, b"w", spans=True)
        np.testing.assert_array_equal(offsets.astype(np.int64), off)
        np.testing.assert_array_equal(first, seg_first)
        assert_records(table, rec, (kpos - off[doc])[fits], kids[fits], "scan_lines")
        g.count_states()
        np.testing.assert_array_equal(g.state_counts_to_host(), state_counts(table, kids))
        first, rec, _ = g.select_lines(buf, b"w", spans=True)
        np.testing.assert_array_equal(first, np.array(sel_first, dtype=np.uint64))
        assert_records(table, rec, np.concatenate(sel_pos), np.concatenate(sel_ids), "select_lines")
        out_off, out, _ = g.replace_lines(buf, b"w", spans=True)
        assert np.array_equal(out, np.concatenate(outs))
        np.testing.assert_array_equal(out_off.astype(np.int64), off)                # (a redaction keeps every length)
        _, masks = g.tag_lines(buf, b"w", spans=True)
        np.testing.assert_array_equal(masks, want_masks)
        got_ids, _ = g.matching_lines(buf, b"w", spans=True)
        np.testing.assert_array_equal(got_ids, want_ids)
        out, out_off, got_ids = g.grep_lines(buf, b"w", spans=True)
        np.testing.assert_array_equal(got_ids, want_ids)
        np.testing.assert_array_equal(out_off, want_line_off)
        assert np.array_equal(out, want_lines)
        # the document forms pass no delimiter: `$` is the document's very end, behind the blank that ends it
        off = spanref.split_offsets(buf, SP)
        dkeep = ref_keep(buf, pos, ids, lens, rules, -1, off)
        assert (dkeep != ref_keep(buf, pos, ids, lens, rules, SP, off)).sum() > 1000
        ddoc = np.searchsorted(off, pos[dkeep], side="right") - 1
        dfits = pos[dkeep] + lens[dkeep] <= off[ddoc + 1]
        first, rec = g.scan_documents((buf, off.astype(np.uint64)), spans=True)
        assert_records(table, rec, (pos[dkeep] - off[ddoc])[dfits], ids[dkeep][dfits], "scan_documents")
        np.testing.assert_array_equal(g.tag_documents((buf, off.astype(np.uint64)), spans=True),
                                      masks_cut(pos[dkeep], ids[dkeep], lens[dkeep], off, masks_by_id(groups)))


def grep_text(seed):
    rng = np.random.default_rng(seed)
    words = [b"the", b"cat", b"a", b"mat", b"he", b"at", b"on", b"that", b"The Cat", b"ON"]
    lines = [b" ".join(words[k] for k in rng.integers(0, len(words), rng.integers(0, 5))) for _ in range(3000)]
    return lines + [b"cat"]


@pytest.mark.parametrize("terminated", [True, False])
def test_grep_lines(tmp_path, terminated):
    """grep -x (line_match) against `line in patterns`; ^ / $ rules from strip_anchors against re.MULTILINE."""
    lines = grep_text(12)
    raw = b"\n".join(lines) + (b"\n" if terminated else b"")
    lines = raw.split(b"\n")[:-1] if terminated else raw.split(b"\n")
    data = np.frombuffer(raw, dtype=np.uint8)
    patterns = [b"the cat", b"cat", b"on a mat", b"he", b"a", b"that that"]
    table = PfacTable.from_file(pattern_file(tmp_path, patterns), 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        out, out_off, ids = g.grep_lines(data, line_match=True)
        want = [k for k, l in enumerate(lines) if l.rstrip(b"\n") in patterns]
        assert 20 < len(want) < len(lines) / 2
        np.testing.assert_array_equal(ids, np.array(want, dtype=np.uint64))
        got = [bytes(out[int(a):int(b)]) for a, b in zip(out_off[:-1], out_off[1:])]
        nl = lambda k: b"" if k == len(lines) - 1 and not terminated else b"\n"     # noqa: E731
        assert got == [lines[k] + nl(k) for k in want]
    anchored = [b"^the cat", b"mat$", b"^on a$", b"he he", b"^that$", b"at on$"]
    stripped, rules = strip_anchors(anchored)
    table = PfacTable.from_file(pattern_file(tmp_path, stripped, "a.pat"), 256)
    rx = re.compile(b"|".join((b"^" if a.startswith(b"^") else b"") + re.escape(s) + (b"$" if a.endswith(b"$") else b"")
                              for a, s in zip(anchored, stripped)), re.MULTILINE)
    starts = np.concatenate([[0], np.cumsum([len(l) + 1 for l in lines])])
    want = sorted({int(np.searchsorted(starts, m.start(), side="right")) - 1 for m in rx.finditer(raw)})
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_pattern_spans(rules)
        _, _, ids = g.grep_lines(data, spans=True)
        np.testing.assert_array_equal(ids, np.array(want, dtype=np.uint64))
        _, _, plain = g.grep_lines(data)
        assert 20 < len(want) < plain.size


def test_ignore_case_gathers_the_lines_as_written(tmp_path):
    lines = grep_text(13)
    raw = b"\n".join(lines) + b"\n"
    data = np.frombuffer(raw, dtype=np.uint8)
    anchored = [b"^the cat", b"on$", b"^a$"]
    stripped, rules = strip_anchors(anchored)
    table = PfacTable.from_bytes(b"".join(p + b"\n" for p in stripped), 256, ignore_case=True)
    rx = re.compile(b"^the cat|on$|^a$", re.MULTILINE | re.IGNORECASE)
    want = [l + b"\n" for l in lines if rx.search(l)]
    exact = [l + b"\n" for l in lines if re.search(b"^the cat|on$|^a$", l)]
    assert len(want) > len(exact) > 20 and bytes(fold(data)) != raw
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        assert g.case_fold
        g.set_pattern_spans(rules)
        out, out_off, ids = g.grep_lines(data, spans=True)
        assert [bytes(out[int(a):int(b)]) for a, b in zip(out_off[:-1], out_off[1:])] == want
        assert any(l != l.lower() for l in want)


# ---------------------------------------------------------------------------
# the contract

def heap_state(g):
    words, tix = g.packed_to_host()
    return words.copy(), tix.copy(), g.scan_finish()[0]


def raw_filter(g, delimiter=-1, flags=0, d_input=None, d_records=None, d_off=None, n_docs=0):
    n = C.c_uint64(0)
    return g._L.pfac_records_filter_spans(g._ctx, 0, d_input, d_records, delimiter, flags, d_off, n_docs, C.byref(n))


def test_errors_in_order_and_nothing_touched(resolve):
    path = resolve("xaa")
    table = PfacTable.from_file(path, 256)
    other = PfacTable.from_file(resolve("experimentpattern"), 256)
    buf = para_bytes(resolve, 20_000)
    rules = spanref.drawn_rules(line_lengths(path))
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        assert status_of(g.filter_spans) == E_STATE                                        # no scan at all
        g.reserve(0, buf.size, 1 << 16)
        g.h2d(buf)
        g.scan_async(buf.size)
        assert status_of(g.filter_spans) == E_STATE                                        # before scan_finish
        total, _ = g.scan_finish()
        assert status_of(lambda: g.filter_spans(line_match=True)) == E_STATE               # no final lengths
        g.set_final_lengths(table.final_lengths())
        assert status_of(g.filter_spans) == E_STATE                                        # no spans for the table
        assert raw_filter(g, delimiter=300) == E_STATE                                     # ... judged before the arguments
        g.set_pattern_spans(rules)
        g.set_doc_offsets(np.array([0, 20_000], dtype=np.uint64))
        assert status_of(lambda: g.filter_spans(n_docs=2)) == E_STATE                      # not the slot's n_docs
        assert raw_filter(g, delimiter=300, n_docs=2) == E_STATE
        before = heap_state(g)
        for kw in (dict(delimiter=-2), dict(delimiter=256), dict(flags=2), dict(flags=3),
                   dict(delimiter=SP, d_input=g.input_ptr() + 4), dict(d_records=g.records_ptr() + 16)):
            assert raw_filter(g, **kw) == E_ARG, kw
        for bad in ([0, 12_000, 11_000, 20_000], [1, 10_000, 20_000], [0, 10_000, 19_999], [0, 10_000, 20_001]):
            g.set_doc_offsets(np.array(bad, dtype=np.uint64))
            assert status_of(lambda: g.filter_spans(delimiter=SP, n_docs=len(bad) - 1)) == E_ARG
            d_bad = upload(np.array(bad, dtype=np.uint64))
            assert raw_filter(g, SP, 0, None, None, d_bad.data_ptr(), len(bad) - 1) == E_ARG
        after = heap_state(g)
        assert all(np.array_equal(a, b) for a, b in zip(before, after)) and after[2] == total
        # with delimiter -1 the input is ignored: a misaligned d_input is no error
        assert g.filter_spans(d_input=g.input_ptr() + 4) < total
        # a table upload: the scan ran with an earlier table, and the spans are gone
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        assert status_of(lambda: g.filter_spans(line_match=True)) == E_STATE
        scan(g, buf)
        assert status_of(g.filter_spans) == E_STATE                                        # cleared by the upload
        assert g.filter_spans(line_match=True) == 0                                        # PFAC_SPANS_LINE needs none
        g.load_table(other)
        g.scan_bytes(buf)
        assert status_of(lambda: g.filter_spans(line_match=True)) == E_STATE               # lengths never set for it
        # an overflowed scan: after the state, before the arguments
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        import torch
        heap = torch.zeros(64 * 4, dtype=torch.uint8, device="cuda:0")
        g.h2d(buf)
        g.scan_async(buf.size, d_records=heap, capacity=64)
        assert g.scan_finish(allow_overflow=True)[1]
        assert raw_filter(g, delimiter=300, d_records=heap.data_ptr()) == E_STATE          # no spans: state first
        g.set_pattern_spans(rules)
        assert raw_filter(g, delimiter=300, d_records=heap.data_ptr()) == E_OVERFLOW
        assert status_of(lambda: g.filter_spans(d_records=heap)) == E_OVERFLOW


def test_set_state_spans_contract(resolve):
    path = resolve("xaa")
    table = PfacTable.from_file(path, 256)
    buf = para_bytes(resolve, 20_000)
    pos, ids, lens = oracle_records(path, buf)
    rules = spanref.drawn_rules(line_lengths(path))
    off = spanref.split_offsets(buf, SP)
    keep = ref_keep(buf, pos, ids, lens, rules, SP, off)
    spans = table.state_spans(rules)
    with GpuMatcher(0, 1) as g:
        L, ctx = g._L, g._ctx
        assert L.pfac_table_set_state_spans(ctx, spans.ctypes.data, spans.size) == E_STATE       # before an upload
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_pattern_spans(rules)
        longer = np.concatenate([spans, spans[:1]])
        assert L.pfac_table_set_state_spans(ctx, longer.ctypes.data, spans.size + 1) == E_ARG
        assert L.pfac_table_set_state_spans(ctx, spans.ctypes.data, spans.size - 1) == E_ARG
        assert L.pfac_table_set_state_spans(ctx, None, spans.size) == E_ARG
        odd = table.state_spans([None] + ["^$"] * (len(rules) - 1))
        odd["reserved"][-1] = 1
        assert L.pfac_table_set_state_spans(ctx, odd.ctypes.data, odd.size) == E_ARG
        total, n = filtered(g, buf, SP)                           # the earlier spans still apply
        assert_records(table, g.records_to_host(n), pos[keep], ids[keep], "after refused spans")
        # a second call replaces them
        g.set_pattern_spans([None] + ["^"] * (len(rules) - 1))
        head = ref_keep(buf, pos, ids, lens, [None] + ["^"] * (len(rules) - 1), SP, off)
        total, n = filtered(g, buf, SP)
        assert_records(table, g.records_to_host(n), pos[head], ids[head], "replaced spans")
        # grep -x whatever spans are set
        whole = spanref.filter_spans(buf, pos, lens, *spanref.line_spans(pos.size), SP, off)
        total, n = filtered(g, buf, SP, line=True)
        assert_records(table, g.records_to_host(n), pos[whole], ids[whole], "line_match")
        assert 0 < whole.sum() < head.sum()


@pytest.mark.parametrize("pat,env,width", [("experimentpattern", {}, 2), (DICT, {}, 4), (DICT, {"PFAC_WIDE": "1"}, 8)],
                         ids=["2", "4", "8"])
def test_writes_stay_inside_the_tiles_runs(pat, env, width, resolve, monkeypatch):
    """The scan goes into a guarded heap of exactly the hinted capacity; the filter may change nothing but the words of
    the tiles' own runs [FIRST, FIRST + old COUNT), and the guards stay intact."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    path = resolve(pat)
    table = PfacTable.from_file(path, 256)
    buf = para_bytes(resolve, N)
    pos, ids, lens = oracle_records(path, buf)
    rules = spanref.drawn_rules(line_lengths(path))
    off = spanref.split_offsets(buf, SP)
    keep = ref_keep(buf, pos, ids, lens, rules, SP, off)
    with matcher(table, rules) as g:
        scan(g, buf)
        cap = g.capacity_hint()
        heap = GuardedBuffer(cap * width)
        g.scan_async(buf.size, d_records=heap.ptr, capacity=cap)
        total, over = g.scan_finish()
        rb, n_tiles, used = g.scan_format()
        assert (rb, total, over) == (width, pos.size, False)
        before = heap.host().copy()
        counts = np.bincount(pos // TILE, minlength=n_tiles)    # the old COUNT of every tile (the oracle's)
        n_docs, _ = g.split_documents(buf.size, SP)
        n = g.filter_spans(delimiter=SP, n_docs=n_docs, d_records=heap.ptr)
        g.sync()
        heap.check(what="the record heap after the span filter")
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
