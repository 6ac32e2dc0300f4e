"""The document passes at millions of documents and ids (run with -m gpu on an MI355X): the compaction behind the four
pfac_documents_matching* forms and the context form, pfac_documents_top_scores, the plain and the formatted gather, and
the split, at the sizes of tests/manydocs.py -- past 1024 group sums, where every thread of pfac_scan_groups_kernel owns
more than one; past one trip of the rank's histogram; past 1024 blocks of the ranked sort -- against the array-at-a-time
references that tests/test_manydocs_cases.py holds to the existing ones.  Those passes take their doc_first, masks,
scores, ids and offsets from caller buffers made on the host: no scan.  The heap-driven passes (the segment pass, the
group masks, the scores, the per-document selection, its scores and its replace) and the chain (grep_text, top_lines)
run over manydocs.heap_input, more than six million documents in under 9 MiB, against the CPU oracle's records cut by
the header's rule.  Integer work: bit-exact.  No expectation comes from the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import groupref
import manydocs as md
import scoreref
import spanref
import wordref
from heapguard import GuardedBuffer
from manydocs import BY_COUNT, DOCS, HIST_DOCS, IDS, LOWEST, RANKED
from passguard import TABLES, WIDTHS, _Env, cpu
from phfpfac_amd import GpuMatcher, PfacError, PfacTable
from phfpfac_amd import _ffi

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW = _ffi.PFAC_E_ARG, _ffi.PFAC_E_OVERFLOW
SORT_K = 3 * md.SORT_BLOCK + 1              # a k of top_lines past the one-workgroup sort
GUARDED = "runs"                            # the pattern that runs into a caller's buffer of exactly n x 8 bytes


@pytest.fixture(scope="module")
def g():
    with GpuMatcher(0, 1) as m:
        yield m


def upload(arr):
    """A device copy of an array's bytes (16 spare ones, so that an empty array still has an address)."""
    raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
    t = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda:0")
    if raw.size:
        t[:raw.size].copy_(torch.from_numpy(raw))
    torch.cuda.synchronize()                # (the slot's stream is not torch's)
    assert t.data_ptr() % 16 == 0
    return t


_KEPT = {}


def kept(key, make):
    """One device copy per key; a new first element of the key (a new size) drops the others."""
    if key not in _KEPT:
        for k in [k for k in _KEPT if k[0] != key[0]]:
            del _KEPT[k]
        _KEPT[key] = make()
    return _KEPT[key]


def overflow_of(fn, attr):
    with pytest.raises(PfacError) as e:
        fn()
    assert e.value.status == E_OVERFLOW
    return getattr(e.value, attr)


# ---------------------------------------------------------------------------
# the compaction: dm_run under every predicate

def compaction(g, call, want, what, guarded):
    """One form: into the slot's buffer, and with `guarded` into a caller's buffer of exactly n x 8 bytes -- one entry
    short is an overflow with the exact count and nothing written."""
    n = call()
    md.assert_ids(g.matching_documents_to_host(n), n, want, what)
    if not guarded:
        return
    gb = GuardedBuffer(want.size * 8)
    if want.size:
        assert overflow_of(lambda: call(d_out=gb.ptr, out_cap=want.size - 1), "n_matching") == want.size, what
        g.sync()
        gb.check(payload_untouched=True, what=f"{what}: d_ids_out after the overflow")
    n = call(d_out=gb.ptr, out_cap=want.size)
    g.sync()
    md.assert_ids(gb.host().view(np.uint64), n, want, what + " (caller's buffer)")
    gb.check(what=f"{what}: d_ids_out at exact capacity")


def context_call(g, n_docs, before, after, d_first, d_out=None, out_cap=0):
    """pfac_documents_matching_context itself (GpuMatcher.matching_documents takes the plain call for 0, 0)."""
    n = C.c_uint64(0)
    rc = g._L.pfac_documents_matching_context(g._ctx, 0, int(d_first.data_ptr()), n_docs, before, after, 0, d_out, out_cap, C.byref(n))
    if rc:
        err = PfacError(rc, "pfac_documents_matching_context")
        err.n_matching = n.value
        raise err
    return n.value


@pytest.mark.parametrize("n,name", [(n, name) for n in DOCS for name in md.FLAGS], ids=lambda v: str(v))
def test_matching_documents(g, n, name):
    """The plain call, inverted, and grep's context with windows (0, 0), (1, 0), (0, 64) and (n, n)."""
    f = md.flags(name, n)
    first = md.doc_first_of(f)
    d_first = upload(first)
    guarded = name == GUARDED
    for invert in (False, True):
        compaction(g, lambda **kw: g.matching_documents(n, invert=invert, d_doc_first=d_first, **kw), md.matching_ids(first, invert),
                   f"{name} n_docs={n} invert={invert}", guarded)
    for before, after in ((0, 0), (1, 0), (0, 64), (n, n)):
        compaction(g, lambda **kw: context_call(g, n, before, after, d_first, **kw), md.context_ids(first, before, after),
                   f"{name} n_docs={n} before={before} after={after}", guarded and before <= 1)


@pytest.mark.parametrize("n,name", [(n, name) for n in DOCS for name in md.FLAGS], ids=lambda v: str(v))
def test_matching_documents_where_and_scored(g, n, name):
    """The group predicate, and the score rule without and with a density, each also inverted."""
    f = md.flags(name, n)
    guarded = name == GUARDED
    masks = md.masks_of(f)
    d_masks = upload(masks)
    for invert in (False, True):
        compaction(g, lambda **kw: g.matching_documents_where(n, invert=invert, d_masks=d_masks, **md.WHERE, **kw),
                   md.group_ids(masks, invert=invert, **md.WHERE), f"{name} n_docs={n} where invert={invert}", guarded and not invert)
    del d_masks, masks
    off = md.offsets_of(md.doc_lengths(n))
    d_off = upload(off)
    for dense in (False, True):
        sc = md.scores_of(f, dense)
        d_sc = upload(sc)
        kw = dict(md.RULE, density=md.DENSITY) if dense else md.RULE
        for invert in (False, True):
            compaction(g, lambda **k: g.matching_documents_scored(n, invert=invert, d_scores=d_sc, d_doc_offsets=d_off, **kw, **k),
                       md.score_ids(sc, off, invert=invert, **kw), f"{name} n_docs={n} scored dense={dense} invert={invert}",
                       guarded and not invert)
        del d_sc


# ---------------------------------------------------------------------------
# the rank

def flag_kw(flags):
    return dict(by="count" if flags & BY_COUNT else "score", lowest=bool(flags & LOWEST), ranked=bool(flags & RANKED))


def rank_run(g, c, d_sc, d_off, k, flags, what):
    want, _ = md.top(c.rank(flags), k, flags)
    n = g.top_documents(c.n, k, d_scores=d_sc, d_doc_offsets=d_off, **flag_kw(flags), **c.kw)
    ids = g.matching_documents_to_host(n) if n == want.size else None
    pairs = g.top_scores_to_host(n) if n == want.size else None
    md.assert_top(ids, pairs, n, c.sc, want, what)
    return ids, pairs


@pytest.mark.parametrize("n,keys,rule,order", [(n, k, r, o) for n in HIST_DOCS for k, r in md.RANK_KEYS for o in (0, BY_COUNT, LOWEST, BY_COUNT | LOWEST)],
                         ids=lambda v: str(v))
def test_top_documents(g, n, keys, rule, order):
    """Every k of RankCase.ks, ranked and in document order; the ranked cut through the tie class twice, byte for byte."""
    c = md.rank_case(n, keys, rule)
    d_sc = kept((n, keys, "scores"), lambda: upload(c.sc))
    d_off = None if c.off is None else kept((n, "offsets"), lambda: upload(c.off))
    ks = c.ks(order)
    for flags in (order, order | RANKED):
        for k in ks:
            rank_run(g, c, d_sc, d_off, k, flags, f"{c} flags {flags} k {k}")
    b, e = md.tie_class(c.sc, c.rank(order), order)
    k = (b + e) // 2
    first = rank_run(g, c, d_sc, d_off, k, order | RANKED, f"{c} flags {order | RANKED} k {k}, first run")
    again = rank_run(g, c, d_sc, d_off, k, order | RANKED, f"{c} flags {order | RANKED} k {k}, second run")
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()


# ---------------------------------------------------------------------------
# the gather

def gather_inputs(g, n_ids):
    d = md.gather_data(n_ids)
    return d, kept((n_ids, "input"), lambda: upload(d.storage())), kept((n_ids, "offsets"), lambda: upload(d.offsets)), \
        kept((n_ids, "first"), lambda: upload(d.doc_first))


def gather_check(g, call, n_ids, want, want_off, what, guarded):
    n = call()
    md.assert_gather(n, g.gathered_offsets_to_host(n_ids), g.gathered_to_host(n) if n == want.size else [], want, want_off, what=what)
    if not guarded:
        return
    gb, go = GuardedBuffer(want.size), GuardedBuffer((n_ids + 1) * 8, fill=0x3C)
    assert overflow_of(lambda: call(d_out=gb.ptr, out_cap=want.size - 1, d_out_offsets=go.ptr), "out_bytes") == want.size
    g.sync()
    gb.check(payload_untouched=True, what=f"{what}: d_out after the overflow")
    go.check(payload_untouched=True, what=f"{what}: d_out_offsets after the overflow")
    n = call(d_out=gb.ptr, out_cap=want.size, d_out_offsets=go.ptr)
    g.sync()
    whole = gb.tensor[gb.front:].cpu().numpy()                     # the payload and the back guard behind it
    md.assert_gather(n, go.host().view(np.uint64), whole, want, want_off, fill=gb.fill, what=what + " (caller's buffers)")
    gb.check(what=f"{what}: d_out at exactly out_bytes")
    go.check(what=f"{what}: d_out_offsets at exactly n_ids + 1 entries")


@pytest.mark.parametrize("n_ids,name", [(n, name) for n in IDS for name in md.ID_LISTS], ids=lambda v: str(v))
def test_gather(g, n_ids, name):
    d, d_in, d_off, _ = gather_inputs(g, n_ids)
    d_ids = upload(d.ids(name))
    want, want_off = d.want(name)
    gather_check(g, lambda **kw: g.gather_documents(d.n_docs, n_ids, d.n, d_input=d_in, d_doc_offsets=d_off, d_ids=d_ids, **kw),
                 n_ids, want, want_off, f"{name} n_ids={n_ids}", name == "ascending")


@pytest.mark.parametrize("n_ids,fmt", [(n, fmt) for n in IDS for fmt in md.FORMATS], ids=lambda v: str(v))
def test_gather_formatted(g, n_ids, fmt):
    """grep -n, -b, both, and context separators with `--` between the groups over a synthetic doc_first."""
    d, d_in, d_off, d_first = gather_inputs(g, n_ids)
    name = md.FORMAT_IDS[fmt]
    d_ids = upload(d.ids(name))
    want, want_off = d.want(name, fmt)
    gather_check(g, lambda **kw: g.gather_documents_formatted(d.n_docs, n_ids, d.n, d_input=d_in, d_doc_offsets=d_off, d_ids=d_ids,
                                                              d_doc_first=d_first, **md.FORMATS[fmt], **kw),
                 n_ids, want, want_off, f"{fmt} ({name}) n_ids={n_ids}", fmt == "both")


@pytest.mark.parametrize("formatted", [False, True], ids=["plain", "formatted"])
def test_gather_offsets_rule_at_depth(g, formatted):
    """One decrease at document 5 000 000 and one end past n_bytes at the last document, both selected: PFAC_E_ARG from
    the device's own check in the count pass, nothing written.  The unbroken offsets gather."""
    n_bytes, off, ids = md.rule_case()
    data = np.random.default_rng(0x0FF).integers(0, 256, n_bytes).astype(np.uint8)
    d_in = upload(np.concatenate([data, np.zeros(4096, np.uint8)]))
    d_ids = upload(ids)
    fmt = md.FORMATS["both"] if formatted else {}
    call = g.gather_documents_formatted if formatted else g.gather_documents
    want, want_off = (md.format_ref(data, off, ids, md.Fmt(**fmt)) if formatted else md.gather_ref(data, off, ids))
    gb, go = GuardedBuffer(want.size), GuardedBuffer((ids.size + 1) * 8, fill=0x3C)
    for how in ("decrease", "past_end"):
        d_bad = upload(md.broken_offsets(off, how))
        with pytest.raises(PfacError) as e:
            call(md.RULE_DOCS, ids.size, n_bytes, d_input=d_in, d_doc_offsets=d_bad, d_ids=d_ids, d_out=gb.ptr, out_cap=want.size,
                 d_out_offsets=go.ptr, **fmt)
        assert e.value.status == E_ARG, how
        g.sync()
        gb.check(payload_untouched=True, what=f"d_out after {how}")
        go.check(payload_untouched=True, what=f"d_out_offsets after {how}")
        del d_bad
    d_off = upload(off)
    n = call(md.RULE_DOCS, ids.size, n_bytes, d_input=d_in, d_doc_offsets=d_off, d_ids=d_ids, d_out=gb.ptr, out_cap=want.size,
             d_out_offsets=go.ptr, **fmt)
    g.sync()
    md.assert_gather(n, go.host().view(np.uint64), gb.host(), want, want_off, what="the unbroken offsets")
    gb.check(what="d_out")
    go.check(what="d_out_offsets")


# ---------------------------------------------------------------------------
# the split

def test_split_where_every_byte_is_a_delimiter(g):
    """8 MiB + 17 delimiters, more delimiters behind them up to the next tile: offset k is k, in all 33 groups."""
    n = md.ALL_DELIMS
    d_in = upload(np.full((n + 16 + md.TILE - 1) // md.TILE * md.TILE, md.NL, dtype=np.uint8))
    n_docs, tail = g.split_documents(n, md.NL, d_input=d_in)
    p = md.Periodic(n, bytes([md.NL]), 0)
    fetch = lambda first, k: g.doc_offsets_to_host(n_docs, first=first, n=k)      # noqa: E731
    md.assert_split(n_docs, tail, fetch, n, n, md.split_windows(p) + [(0, n + 1)],
                    lambda first, k: np.arange(first, first + k, dtype=np.uint64), "every byte a delimiter")


def test_split_of_1025_groups_of_tiles(g):
    """1025 x 64 tiles filled on the device from a period of 65 bytes with three delimiters: more than twelve million
    documents, the offsets by arithmetic, windows at the start, across all 1024 group edges and at the end."""
    n = md.TILED_BYTES
    t = torch.empty(n + md.TILE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    g.fill_tiled(t, n + md.TILE, md.TILED_PERIOD, md.TILED_PHASE)     # (the period goes on behind n_bytes, delimiters and all)
    g.sync()
    n_docs, tail = g.split_documents(n, md.NL, d_input=t)
    p = md.Periodic(n, md.TILED_PERIOD, md.TILED_PHASE)
    fetch = lambda first, k: g.doc_offsets_to_host(n_docs, first=first, n=k)      # noqa: E731
    md.assert_split(n_docs, tail, fetch, p.n_docs, p.tail_start, md.split_windows(p), p.offsets, "1025 groups of tiles")
    # the same period on the host, for the bytes the device filled: the first group and the last
    for at in (0, n - md.SPLIT_GROUP):
        got = t[at:at + md.SPLIT_GROUP].cpu().numpy()
        idx = (np.arange(at, at + md.SPLIT_GROUP, dtype=np.int64) + md.TILED_PHASE) % len(md.TILED_PERIOD)
        assert np.array_equal(got, np.frombuffer(md.TILED_PERIOD, dtype=np.uint8)[idx]), f"the filled bytes from {at} on"


# ---------------------------------------------------------------------------
# the heap-driven passes over manydocs.heap_input: one scan per record width, records from the CPU oracle

_SCAN = {}


def scanned(g, W):
    """The context with the table of record width W (W = 1: the table of single bytes), its lengths, groups, weights
    and replacements, and the slot's last finished scan that of the heap input from a caller's buffer.  -> what the CPU
    says: dict(pos, ids, lens, ll, idmap, n_ids, d_in, d_off)."""
    h = md.heap_input()
    if _SCAN.get("W") != W:
        _SCAN.clear()
        if W == 1:
            table = PfacTable.from_bytes(b"".join(p + b"\n" for p in md.BYTE_PATTERNS), 256)
            pos, ids, lens = md.byte_records(h.data)
            n_ids, knobs, ll = len(md.BYTE_PATTERNS), {}, np.array([0] + [1] * len(md.BYTE_PATTERNS))
        else:
            x = cpu()
            table, info = x.table(W), x.tinfo(W)
            pos, ids, lens = h.records(info["matcher"], info["ll"])
            n_ids, knobs, ll = info["ll"].size - 1, TABLES[W]["knobs"], info["ll"]
        with _Env(knobs):
            g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_pattern_groups(groupref.groups_for(n_ids))
        g.set_pattern_weights(md.heap_weights(n_ids))
        if W == 1:
            g.set_replacements(md.BYTE_REPS)
        _SCAN.update(W=W, pos=pos, ids=ids, lens=lens, n_ids=n_ids, ll=ll, idmap=np.asarray(table.idmap, dtype=np.int64), fresh=False)
    c = _SCAN
    c["d_in"] = kept(("heap", "input"), lambda: upload(h.storage()))
    c["d_off"] = kept(("heap", "offsets"), lambda: upload(h.offsets))
    if not c["fresh"]:
        g.reserve(0, 0, max(c["pos"].size + c["pos"].size // 4, 1 << 20))
        n = g.scan_resident(h.n, h.n, d_input=c["d_in"])
        assert n == c["pos"].size, f"the scan counts {n} records, the oracle {c['pos'].size}"
        assert W == 1 or g.scan_format()[0] == W, f"record width {g.scan_format()[0]}, want {W}"
        c["fresh"] = True
    return h, c


def status_of(fn):
    with pytest.raises(PfacError) as e:
        fn()
    return e.value.status


@pytest.mark.parametrize("W", WIDTHS)
def test_segment_records(g, W):
    h, c = scanned(g, W)
    first, rel, kids, keep, _ = md.cut_records(c["pos"], c["ids"], c["lens"], h.offsets)
    n = g.segment_records(h.n_docs, d_doc_offsets=c["d_off"])
    got_first, rec = g.segment_to_host(n, h.n_docs) if n == rel.size else (None, None)
    assert n == rel.size, f"width {W}: {n} records kept, want {rel.size}"
    md.assert_segment(got_first, rec, n, first, rel, kids, c["idmap"], f"pfac_records_segment width {W}")


@pytest.mark.parametrize("W", WIDTHS)
def test_document_group_masks(g, W):
    h, c = scanned(g, W)
    by_id = groupref.masks_by_id(groupref.groups_for(c["n_ids"]))
    want = groupref.masks_cut(c["pos"], c["ids"], c["lens"], h.offsets, by_id)
    assert np.count_nonzero(want) > 100_000
    any_mask = g.document_group_masks(h.n_docs, d_doc_offsets=c["d_off"])
    md.assert_masks(g.group_masks_to_host(h.n_docs), any_mask, want, f"pfac_documents_group_masks width {W}")


@pytest.mark.parametrize("W", WIDTHS)
def test_document_scores(g, W):
    h, c = scanned(g, W)
    want = scoreref.scores_cut(c["pos"], c["ids"], c["lens"], h.offsets, scoreref.w_by_id(md.heap_weights(c["n_ids"])))
    assert np.count_nonzero(want["score"]) > 100_000 and ((want["count"] > 0) & (want["score"] == 0)).any()
    totals = g.document_scores(h.n_docs, d_doc_offsets=c["d_off"])
    md.assert_scores(g.document_scores_to_host(h.n_docs), totals, want, f"pfac_documents_scores width {W}")


def test_selection_scores_and_replace_per_document(g):
    """The table of single bytes: the per-document selection is the kept records, its scores are the documents', and
    the replace is a byte map with replacements of 0, 1, 2 and 6 bytes."""
    h, c = scanned(g, 1)
    first, _, kids, keep, _ = md.cut_records(c["pos"], c["ids"], c["lens"], h.offsets)
    assert keep.all()
    n = g.select_leftmost_longest_documents(h.n_docs, d_doc_offsets=c["d_off"])
    assert n == c["pos"].size, f"{n} picks, want {c['pos'].size}"
    got_first, rec = g.doc_selection_to_host(n, h.n_docs)
    md.assert_segment(got_first, rec, n, first, c["pos"], kids, c["idmap"], "pfac_records_leftmost_longest_documents")
    want = scoreref.scores_cut(c["pos"], c["ids"], c["lens"], h.offsets, scoreref.w_by_id(md.heap_weights(c["n_ids"])))
    totals = g.selection_document_scores(h.n_docs)
    md.assert_scores(g.document_scores_to_host(h.n_docs), totals, want, "pfac_selection_document_scores")
    out, out_off = md.byte_replace(h.data, h.offsets)
    gb, go = GuardedBuffer(out.size), GuardedBuffer((h.n_docs + 1) * 8, fill=0x3C)
    call = lambda cap: g.replace_selection_documents(d_input=c["d_in"], d_out=gb.ptr, out_cap=cap, d_out_offsets=go.ptr,       # noqa: E731
                                                     d_doc_offsets=c["d_off"])
    assert overflow_of(lambda: call(out.size - 1), "out_bytes") == out.size
    g.sync()
    gb.check(payload_untouched=True, what="d_out after the overflow")
    go.check(payload_untouched=True, what="d_out_offsets after the overflow")
    n = call(out.size)
    g.sync()
    md.assert_gather(n, go.host().view(np.uint64), gb.tensor[gb.front:].cpu().numpy(), out, out_off, fill=gb.fill, what="pfac_replace_documents")
    gb.check(what="d_out at exactly out_bytes")
    go.check(what="d_out_offsets at exactly n_docs + 1 entries")


@pytest.mark.parametrize("how", ["decrease", "past_end"])
def test_heap_passes_offsets_rule_at_depth(g, how):
    """One decrease at offset 5 000 000 and one end past n_owned: every heap-driven pass answers PFAC_E_ARG from the
    device's own check and leaves the caller's buffers as they were."""
    h, c = scanned(g, 4)
    d_bad = upload(h.broken(how))
    first, rel, _, _, _ = md.cut_records(c["pos"], c["ids"], c["lens"], h.offsets)
    recs, firsts = GuardedBuffer(rel.size * 8), GuardedBuffer((h.n_docs + 1) * 8, fill=0x3C)
    masks, scores = GuardedBuffer(h.n_docs * 8), GuardedBuffer(h.n_docs * 16)
    calls = {
        "pfac_records_segment": (lambda: g.segment_records(h.n_docs, d_doc_offsets=d_bad, d_out=recs.ptr, out_cap=rel.size,
                                                           d_doc_first=firsts.ptr), (recs, firsts)),
        "pfac_documents_group_masks": (lambda: g.document_group_masks(h.n_docs, d_doc_offsets=d_bad, d_out=masks.ptr), (masks,)),
        "pfac_documents_scores": (lambda: g.document_scores(h.n_docs, d_doc_offsets=d_bad, d_out=scores.ptr), (scores,)),
        "pfac_records_leftmost_longest_documents": (lambda: g.select_leftmost_longest_documents(
            h.n_docs, d_doc_offsets=d_bad, d_out=recs.ptr, out_cap=rel.size, d_doc_first=firsts.ptr), (recs, firsts)),
    }
    for name, (call, bufs) in calls.items():
        assert status_of(call) == E_ARG, f"{name}: {how}"
        g.sync()
        for b in bufs:
            b.check(payload_untouched=True, what=f"a caller's buffer of {name} after {how}")
    # the unbroken offsets, into the same buffers
    n = g.segment_records(h.n_docs, d_doc_offsets=c["d_off"], d_out=recs.ptr, out_cap=rel.size, d_doc_first=firsts.ptr)
    g.sync()
    assert n == rel.size
    md._same(firsts.host().view(np.uint64), first, "the unbroken offsets", "doc_first")
    recs.check(what="d_out")
    firsts.check(what="d_doc_first")
    # the in-place filters refuse the same offsets and drop nothing
    c["fresh"] = False
    g.set_pattern_spans(spanref.drawn_rules(c["ll"]))
    assert status_of(lambda: g.filter_spans(delimiter=b" ", n_docs=h.n_docs, d_doc_offsets=d_bad, d_input=c["d_in"])) == E_ARG, how
    assert status_of(lambda: g.filter_whole_words(n_docs=h.n_docs, d_doc_offsets=d_bad, d_input=c["d_in"])) == E_ARG, how
    md._same_records(g.records_to_host(c["pos"].size), c["pos"], c["ids"], c["idmap"], f"the scan's records after {how}")


# ---------------------------------------------------------------------------
# the chain, end to end over the same bytes, cut on the device at every space

def test_grep_text_end_to_end(g):
    h, c = scanned(g, 2)
    off = h.split[0]
    first = md.cut_records(c["pos"], c["ids"], c["lens"], off)[0]
    ids = md.matching_ids(first)
    assert ids.size > 100_000 and int(ids[-1]) > DOCS[1]
    want, want_off = md.format_ref(h.data, off, ids, md.Fmt(number=True, byte_offset=True, terminate=md.SPACE))
    c["fresh"] = False                                            # (the call scans from the slot's own input)
    text, out_off, got = g.grep_text(h.data, delimiter=b" ", number=True, byte_offset=True)
    md.assert_ids(got, got.size, ids, "grep_text: the lines")
    md.assert_gather(text.size, out_off, text, want, want_off, what="grep_text")


def test_top_lines_end_to_end(g):
    h, c = scanned(g, 4)
    off = h.split[0]
    sc = scoreref.scores_cut(c["pos"], c["ids"], c["lens"], off, scoreref.w_by_id(md.heap_weights(c["n_ids"])))
    c["fresh"] = False
    for k, kw, flags in ((5000, dict(), RANKED), (SORT_K, dict(by="count", lowest=True, ranked=False, min_count=1), BY_COUNT | LOWEST)):
        cand = md.score_ids(sc, **{a: b for a, b in kw.items() if a == "min_count"})
        ids, n = md.top(md.ranking(sc, cand, flags), k, flags)
        assert n == k
        want, want_off = md.gather_ref(h.data, off, ids)
        out, out_off, got, pairs = g.top_lines(h.data, k, delimiter=b" ", **kw)
        md.assert_top(got, pairs, got.size, sc, ids, f"top_lines k={k} {kw}")
        md.assert_gather(out.size, out_off, out, want, want_off, what=f"top_lines k={k} {kw}")


# ---------------------------------------------------------------------------
# the in-place filters with documents: every record looks its document up among six million

def kept_records(g, c, keep, n, what):
    want_pos, want_ids = c["pos"][keep], c["ids"][keep]
    assert n == want_pos.size, f"{what}: {n} records kept, want {want_pos.size} of {keep.size}"
    md._same_records(g.records_to_host(n), want_pos, want_ids, c["idmap"], what)


@pytest.mark.parametrize("W", WIDTHS)
def test_filter_spans_with_documents(g, W):
    """spanref's drawn rules (none, ^, $, ^$, offset 5 depth 20) per pattern; `$` sits in front of a document's space."""
    h, c = scanned(g, W)
    rules = spanref.drawn_rules(c["ll"])
    keep = spanref.filter_spans(h.data, c["pos"], c["lens"], *spanref.record_spans(rules, c["ids"]), delimiter=md.SPACE, off=h.offsets)
    assert 10_000 < int(keep.sum()) < keep.size - 10_000
    g.set_pattern_spans(rules)
    c["fresh"] = False                                            # (the filter works in place: the next test scans again)
    n = g.filter_spans(delimiter=b" ", n_docs=h.n_docs, d_doc_offsets=c["d_off"], d_input=c["d_in"])
    kept_records(g, c, keep, n, f"pfac_records_filter_spans width {W}")


@pytest.mark.parametrize("W", WIDTHS)
def test_filter_whole_words_with_documents(g, W):
    """The default word set; the document offsets are boundaries too, the cuts inside the text's words among them."""
    h, c = scanned(g, W)
    keep = wordref.filter_words(h.data, c["pos"], c["lens"], off=h.offsets)
    alone = wordref.filter_words(h.data, c["pos"], c["lens"])
    assert 10_000 < int(keep.sum()) < keep.size - 10_000 and int(keep.sum()) > int(alone.sum())     # the offsets admit some
    c["fresh"] = False
    n = g.filter_whole_words(n_docs=h.n_docs, d_doc_offsets=c["d_off"], d_input=c["d_in"])
    kept_records(g, c, keep, n, f"pfac_records_filter_words width {W}")
