"""The four passes behind the scan that the older fuzzers do not reach -- the span filter (pfac_records_filter_spans),
the group masks (pfac_documents_group_masks), replacement templates (pfac_table_set_replacement_templates) and match
extraction (pfac_extract_leftmost_longest) -- and their composition, on the seeded random cases of tests/latefuzz.py
under the knob sets that change the record form or the heap layout; then two directed tests at the code the passes
share: the window writer (every piece boundary on every byte of a chunk, on window and workgroup edges) and the offsets
rule (every call that carries it, one bad pair at a time).  Run with -m gpu on an MI355X.  Expectations come from the CPU
oracle and the host references alone (tests/test_latefuzz_cases.py pins them without a GPU).  Bit-exact."""
import numpy as np
import pytest

import tplref
from latefuzz import (KNOB_NAMES, LADDER_PATTERNS, RULE_BAD, RULE_BYTES, RULE_DOCS, RULE_GROUPS, RULE_PATTERNS, RULE_SPANS,
                      SEEDS, LateCase, case_id, ladder_cases, rule_expect, rule_offsets, run_late_case)
from phfpfac_amd import GpuMatcher, PfacError, PfacTable, _ffi

pytestmark = pytest.mark.gpu


def set_knobs(monkeypatch, knobs):
    for k in KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def write_patterns(tmp_path, pats, name="p.pat"):
    f = tmp_path / name
    f.write_bytes(b"".join(p + b"\n" for p in pats))
    return str(f)


def same(got, want, what):
    got, want = bytes(got), bytes(want)
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{what}: {len(got)} bytes, want {len(want)}; first difference at {k}: "
                             f"{got[max(k - 8, 0):k + 24]!r} / {want[max(k - 8, 0):k + 24]!r}")


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS, ids=[case_id(s) for s in SEEDS])
def test_late_fuzz(seed, monkeypatch, tmp_path):
    """One random case (tests/latefuzz.py): scan, offsets, span filter, group masks, per-document selection, templated
    replace and extraction per document and over the whole stream, the plain replace, the templates again."""
    case = LateCase(seed)
    set_knobs(monkeypatch, case.knobs)
    n_rec, n_bytes = run_late_case(lambda: GpuMatcher(0, 1), case, str(tmp_path))
    print(f"case {case.describe()}: {n_rec} records and {n_bytes} bytes compared")


# ---------------------------------------------------------------------------
def test_template_piece_ladder(tmp_path):
    """The shared window writer under its four instantiations -- plain replace, templated replace, extraction and the
    per-document templated replace -- on `gap ab gap ab ...` with the gap, the prefix and the suffix stepped through
    0..17, a lead that puts each piece boundary on 1023, 1024, 1025, 4095, 4096 and 4097, and outputs that end at
    4095, 4096 and 4097 bytes (tests/test_latefuzz_cases.py asserts that the inputs do meet these)."""
    table = PfacTable.from_file(write_patterns(tmp_path, LADDER_PATTERNS), 256)
    compared = 0
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        for lc in ladder_cases():
            n = lc.data.size
            g.reserve(0, n, 4096)
            g.h2d(lc.data)
            assert g.scan_resident(n, n) == lc.pos.size, lc.name
            g.set_replacements(lc.templates("plain"))
            n_sel, ex = g.select_leftmost_longest(0)
            assert (n_sel, ex) == (lc.pos.size, 0), lc.name
            out, _, _ = lc.want("plain")
            same(g.replacement_to_host(g.replace_selection()), out, f"{lc.name}: plain replace")
            g.set_replacement_templates(lc.templates("templated"))
            out, _, _ = lc.want("templated")
            same(g.replacement_to_host(g.replace_selection()), out, f"{lc.name}: templated replace")
            ext, pick_off, _ = lc.want("extract")
            same(g.extracted_to_host(g.extract_selection()), ext, f"{lc.name}: extraction")
            assert np.array_equal(g.extract_offsets_to_host(n_sel), pick_off), f"{lc.name}: pick offsets"
            # every document on its own: the same bytes (no cut lies inside a pick), and where each document's begin
            off = lc.off.astype(np.int64)
            g.set_doc_offsets(lc.off)
            assert g.select_leftmost_longest_documents(off.size - 1) == n_sel, lc.name
            same(g.replacement_to_host(g.replace_selection_documents()), out, f"{lc.name}: templated replace per document")
            lens = []
            for a, b in zip(off[:-1], off[1:]):
                mine = (lc.pos >= a) & (lc.pos < b)
                lens.append(len(tplref.assemble(lc.data[a:b], 0, b - a, lc.pos[mine] - a, np.full(int(mine.sum()), 2),
                                                np.ones(int(mine.sum()), dtype=np.int64), lc.templates("templated")).replaced))
            assert np.array_equal(g.replacement_doc_offsets_to_host(off.size - 1),
                                  np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)), f"{lc.name}: output offsets"
            compared += 3 * len(out) + len(ext)
    print(f"{len(ladder_cases())} ladder inputs, {compared} bytes compared")


# ---------------------------------------------------------------------------
def heap_state(g, n):
    words, tix = g.packed_to_host()
    return g.scan_format(), g.last_count(), g.records_to_host(n).copy(), words.copy(), tix.copy()


def same_state(a, b):
    return a[0] == b[0] and a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:]))


@pytest.mark.parametrize("bad", RULE_BAD)
def test_offsets_rule_everywhere(bad, tmp_path):
    """70 000 documents over a scan of 70 001 bytes, one bad pair in the offsets: every call that carries or launches
    the offsets rule refuses them with PFAC_E_ARG and leaves the record heap, its count and format, and the masks of an
    earlier call as they were."""
    import torch
    path = write_patterns(tmp_path, RULE_PATTERNS)
    table = PfacTable.from_file(path, 256)
    want = rule_expect(path)
    data, pos, ids, want_masks, good = want.data, want.pos, want.ids, want.masks, rule_offsets()
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_pattern_spans(RULE_SPANS)
        g.set_pattern_groups(RULE_GROUPS)
        g.reserve(0, RULE_BYTES, 1 << 16)
        g.h2d(data)
        assert g.scan_resident(RULE_BYTES, RULE_BYTES) == pos.size
        g.set_doc_offsets(good)
        g.document_group_masks(RULE_DOCS)
        assert np.array_equal(g.group_masks_to_host(RULE_DOCS), want_masks)
        before = heap_state(g, pos.size)
        g.set_doc_offsets(rule_offsets(bad))
        sentinel = 0x5A5A5A5A5A5A5A5A
        d_masks = torch.full((RULE_DOCS,), sentinel, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        calls = [("segment_records", lambda: g.segment_records(RULE_DOCS)),
                 ("select_leftmost_longest_documents", lambda: g.select_leftmost_longest_documents(RULE_DOCS)),
                 ("filter_spans", lambda: g.filter_spans(delimiter=ord("c"), n_docs=RULE_DOCS)),
                 ("filter_whole_words", lambda: g.filter_whole_words(n_docs=RULE_DOCS)),
                 ("document_group_masks", lambda: g.document_group_masks(RULE_DOCS, d_out=d_masks))]
        for name, call in calls:
            with pytest.raises(PfacError) as e:
                call()
            assert e.value.status == _ffi.PFAC_E_ARG, f"{name}: status {e.value.status}"
            g.sync()
            assert same_state(before, heap_state(g, pos.size)), f"{name}: the record heap changed"
            if name != "document_group_masks":                  # (that call discards the slot-owned masks even when refused)
                assert np.array_equal(g.group_masks_to_host(RULE_DOCS), want_masks), f"{name}: the earlier masks changed"
        assert int((d_masks != sentinel).sum()) == 0, "a refused document_group_masks wrote into the caller's buffer"
        # the good offsets again: every call runs, on a heap that is still the scan's
        g.set_doc_offsets(good)
        assert g.segment_records(RULE_DOCS) == int(want.fits.sum())
        g.document_group_masks(RULE_DOCS)
        assert np.array_equal(g.group_masks_to_host(RULE_DOCS), want_masks)
        assert g.filter_whole_words(n_docs=RULE_DOCS) == int(want.words.sum())
        n = g.filter_spans(delimiter=ord("c"), n_docs=RULE_DOCS)
        assert n == int(want.spans.sum())
        rec = g.records_to_host(n)
        assert np.array_equal(rec["pos"].astype(np.int64), pos[want.spans])
        assert np.array_equal(table.idmap[rec["state"]], ids[want.spans])
