"""CPU side of the rank fuzzer (tests/rankfuzz.py): the generator is pinned per seed, every expectation of every suite
seed is computed on the host, and the conditions below say that the seeds reach what the GPU file is there to test -- so
that a GPU run cannot pass by checking nothing.  They are conditions on the inputs, asserted over the references alone.
The vectorised references are held against their second forms (scoreref.scores_by_find, topref.ranking_py / top_heap,
fmtref.format_ref_loop, gatherref.context_ids_loop, llref.greedy per document) on the seeds that are small enough:
SECOND_FORM_DOCS documents at most (the loops are quadratic in places), and for scores_by_find also an exact table
without duplicate lines and no filter (`find` knows neither)."""
import numpy as np
import pytest

import scoreref
import topref
from fmtref import _digits, format_ref_loop
from gatherref import context_ids_loop
from llref import greedy
from rankfuzz import (DOC_LADDER, FILTERS, GROUP, KNOBS, SEEDS, TILE, RankCase, expectation, knob_label, record_width,
                      with_context_sep)

SECOND_FORM_DOCS = 1100                  # the second forms run on the seeds with at most this many documents

FINGERPRINTS = {                         # RankCase(seed).fingerprint(): the patterns, the data, the offsets and every draw
    0: "6d49ab36707416d7", 1: "79193e28fb4e6aa7", 2: "52452ab3fa6c339c", 3: "89c83fde4abdffb0", 4: "833609643f413e8f",
    5: "5d8dbd032f7f5691", 6: "9039d6de68b0dc63", 7: "0b5c986f5400271f", 8: "ab4edd6149cab816", 9: "5e26e2d5b58dc7bc",
    10: "19dd0e93bc5e15e7", 11: "c8a2a015027d845e", 12: "9fe935803aa7356f", 13: "828e974d81c246dc", 14: "3690b7305ce0f21e",
    15: "91765657cd22dfb2", 16: "9539de7c7a97f4c6", 17: "ab95e73a73d480a3", 18: "173015484a370020", 19: "3fd93520b8c6e3e6",
    20: "fb9a68fc9dedfadc", 21: "d5836dd8aa572a31", 22: "30ebedf8681b2b40", 23: "5de91763e0b52c6d", 24: "bc98773912453e66",
    25: "8c00b6ae687adf7b", 26: "3a3e83f6e2c8334a", 27: "3b7ff1632a8320ce", 28: "9c000a7ab25711bf", 29: "dd18f0edf6c729a9",
    30: "d19e0e884aa38fd4", 31: "94a6542c319ef496", 32: "788ec146c7bc0c3a", 33: "d83c8c6aeb99357e", 34: "3c4aa94caf0a49a8",
    35: "61967440942fffc2", 36: "950892c00eb13c80", 37: "13a95d53defc9b49", 38: "a9f5c3b897727587", 39: "2d06338e2dbc6dc7",
    40: "5f03d74a796eda84", 41: "f4122531fce205c7", 42: "59acb6f98a27ac0b", 43: "b90b079f6f66c8ac", 44: "88e23022064dbe2d",
    45: "7be9181fa10bc36c", 46: "9f41d4e7eb217274", 47: "a0322f1b9933f7c3",
}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("rank"))
    out = []
    for s in SEEDS:
        c, w = expectation(s, tmp)
        out.append((c, w, c.table(f"{tmp}/rank_{s}.pat")))
    return out


def test_the_generator_is_pinned():
    got = {s: RankCase(s).fingerprint() for s in SEEDS}
    assert got == FINGERPRINTS, "the generator's draws changed:\n" + "\n".join(
        f"    {s}: \"{got[s]}\"," for s in SEEDS if FINGERPRINTS.get(s) != got[s])
    assert RankCase(7, KNOBS[1]).knobs == KNOBS[1] and RankCase(7).knobs == KNOBS[7 % len(KNOBS)]


def test_seeds_cover_knobs_widths_tables_filters_and_document_counts(cases):
    runs, widths, filters = {}, {2: 0, 4: 0, 8: 0}, {f: 0 for f in FILTERS}
    folded = few = group = workgroup = third = 0
    for c, w, table in cases:
        runs[knob_label(c.knobs)] = runs.get(knob_label(c.knobs), 0) + 1
        assert table.max_pat_len == c.M
        widths[record_width(table.num_final, c.knobs)] += 1
        filters[c.filter] += 1
        folded += c.folded
        off, nd = w.off, w.n_docs
        assert off[0] == 0 and off[-1] == c.n_owned and (np.diff(off) >= 0).all() and 1 <= c.n_owned <= c.n == c.data.size
        assert c.n <= 300007 + 5000 and not any(bytes([c.delim]) in p or b"\n" in p for p in c.lines)
        assert len(c.rules) == len(c.weights) == len(c.lines) + 1 and len(c.tops) == 3 and len(c.fmts) == 2
        if c.lines_half:
            assert np.array_equal(w.split, off) and (c.data[c.n_owned - 1] == c.delim) == c.terminated
        few += nd < 64
        group += 4097 <= nd <= 16384
        workgroup += nd > 16384
        third += nd >= 32769
    print(f"knob sets {runs}; widths {widths}; filters {filters}; folded {folded}; documents: < 64 in {few} seeds, 4 097 .. 16 384 "
          f"in {group}, > 16 384 in {workgroup}, >= 32 769 in {third}")
    assert sorted(runs) == sorted(knob_label(k) for k in KNOBS) and set(runs.values()) == {8}
    assert min(widths.values()) >= 6
    assert folded >= 12 and min(filters.values()) >= 10
    assert 16 <= sum(c.lines_half for c, _, _ in cases) <= 32, "the device split and the explicit offsets are not about half each"
    assert few >= 4 and group >= 6 and workgroup >= 6 and third >= 2
    assert {w.n_docs for _, w, _ in cases} >= set(DOC_LADDER) - {1000, 40000}


def test_the_score_passes_have_work(cases):
    dense = straddle = zero = hole = ranges = 0
    for c, w, _ in cases:
        off, nd, sc = w.off, w.n_docs, w.sc
        kp, kd = w.kpos[w.fits], w.kdoc[w.fits]                 # the records the score pass counts
        # more than 64 of one document from one tile: the open run is carried across a chunk of 64 lanes
        per = np.unique(kd * (c.n // TILE + 2) + kp // TILE, return_counts=True)[1]
        dense += bool(per.size and per.max() > 64)
        for edge in range(GROUP, c.n_owned, GROUP):
            d = int(np.searchsorted(off, edge, side="right")) - 1
            if off[d] < edge < off[d + 1] and (kp[kd == d] < edge).any() and (kp[kd == d] >= edge).any():
                straddle += 1
                break
        zero += bool(((sc["count"] >= 1) & (sc["score"] == 0)).any())
        has, full = sc["count"] > 0, np.diff(off) > 0
        hole += bool(nd >= 3 and (has[:-2] & ~has[1:-1] & full[1:-1] & has[2:]).any())
        f = w.sel_first.astype(np.int64)
        some = f[1:] > f[:-1]
        ranges += bool(f[-1] > 256 and (f[:-1][some] // 256 != (f[1:][some] - 1) // 256).any())
    print(f"seeds with: more than 64 kept records of a document from one tile {dense}; kept records on both sides of a 64-tile "
          f"edge {straddle}; a matched document of score 0 {zero}; an unmatched document between two matched ones {hole}; a "
          f"document's picks across two 256-pick ranges {ranges}")
    assert dense >= 10 and straddle >= 6 and zero >= 8 and hole >= 8 and ranges >= 6


def test_the_top_draws_have_work(cases):
    flags = {f: 0 for f in range(8)}
    cut = cut_groups = small = block = more = beyond = none = dens = inv = seven = signs = edge = 0
    for c, w, _ in cases:
        for (k, by, lowest, ranked, rule), t in zip(c.tops, w.tops):
            flags[t.flags] += 1
            key = topref.key_word(w.sc, t.flags)
            kr = key[t.rank.astype(np.int64)]
            if 0 < t.n_top < t.cand.size and kr[t.n_top - 1] == kr[t.n_top]:
                cut += 1
                members = t.rank[kr == kr[t.n_top]].astype(np.int64)
                cut_groups += np.unique(members // topref.GROUP).size > 1
            small += 64 < t.n_top <= 1024
            block += 1024 < t.n_top <= 2048
            more += t.n_top > 2048
            beyond += k > t.cand.size
            none += t.cand.size == 0
            dens += bool(rule and "density" in rule)
            inv += bool(rule and rule.get("invert"))
            seven += bool(kr.size >= 2 and np.unique(kr >> np.uint64(8)).size == 1)
            s = w.sc["score"][t.cand.astype(np.int64)]
            signs += bool(by == "score" and (s < 0).any() and (s > 0).any())
            # a document whose score or count IS one of the rule's bounds: `>=` and `>` differ there
            edge += any(rule is not None and b in rule and (w.sc[f] == rule[b]).any()
                        for b, f in (("min_score", "score"), ("max_score", "score"), ("min_count", "count"), ("max_count", "count")))
    print(f"top draws: flags {flags}; k cuts a tie class {cut}, of which across 4 096-document groups {cut_groups}; n_top in "
          f"(64, 1 024] {small}, (1 024, 2 048] {block}, above {more}; k beyond the candidates {beyond}; no candidate {none}; "
          f"density {dens}; invert {inv}; keys equal in seven bytes {seven}; both signs by score {signs}; a document on a bound of the "
          f"rule's windows {edge}")
    assert sum(flags.values()) == 144 and min(flags.values()) >= 8
    assert cut >= 16 and cut_groups >= 4
    assert small >= 12 and block >= 4 and more >= 4
    assert beyond >= 6 and none >= 2 and dens >= 8 and inv >= 8 and seven >= 12 and signs >= 12
    assert edge >= 8


def _label_digits(c, w, fmt, ids):
    """The digit counts of the labels `fmt` prints for `ids` (empty without a label)."""
    ids = ids.astype(np.int64)
    out = []
    if fmt.number:
        out.append(_digits(ids + fmt.number_base)[1])
    if fmt.byte_offset:
        out.append(_digits(w.off[ids] + fmt.offset_base)[1])
    return out


def test_the_formatter_and_the_context_have_work(cases):
    descend = long_out = empty = last = overlap = both = 0
    for c, w, _ in cases:
        off, nd = w.off, w.n_docs
        r = w.tops[w.ranked].ids.astype(np.int64)
        descend += bool((np.diff(r) < 0).any() and any(np.unique(d).size > 1 for d in _label_digits(c, w, c.fmts[0], r)))
        long_out += max(w.fmt_ranked[0].size, w.fmt_ctx[0].size) > 4096
        lists = [w.rule_ids, w.tops[w.ranked].ids, w.ctx_ids]
        gathered = np.unique(np.concatenate(lists)).astype(np.int64)
        empty += bool((off[gathered + 1] == off[gathered]).any())
        last += bool(not c.terminated and off[nd] > off[nd - 1] and nd - 1 in gathered)
        before, after = c.context
        m = np.flatnonzero(w.sc["count"] > 0)
        clamped = m.size and (m[0] - before < 0 or m[-1] + after > nd - 1)
        overlap += bool(clamped and m.size >= 2 and (m[:-1] + after >= m[1:] - before).any()
                        and np.unique(w.ctx_ids).size == w.ctx_ids.size)
        x = w.ctx_ids.astype(np.int64)
        matched = w.doc_first[x + 1] > w.doc_first[x]
        f = c.fmts[1]
        both += bool((f.number or f.byte_offset) and matched.any() and not matched.all())
    print(f"seeds with: descending ranked ids under labels of two digit counts {descend}; more than 4 096 formatted bytes "
          f"{long_out}; a gathered empty document {empty}; the unterminated last document gathered {last}; overlapping context "
          f"windows, one clamped {overlap}; both label separators in one output {both}")
    assert descend >= 10 and long_out >= 10 and empty >= 8 and last >= 6 and overlap >= 10 and both >= 12


def test_the_references_equal_their_second_forms(cases):
    ran = found = 0
    for c, w, _ in cases:
        if w.n_docs > SECOND_FORM_DOCS:
            continue
        ran += 1
        off = w.off
        if not c.folded and c.filter == "none" and len(set(c.lines)) == len(c.lines) and w.n_docs * len(c.lines) <= 100_000:
            found += 1
            by_find = scoreref.scores_by_find(c.data[:c.n_owned], off, c.lines, w.by_id)
            assert np.array_equal(by_find, w.sc), c.describe()
        assert np.array_equal(scoreref.predicate_loop(w.sc, off, **c.score_rule), w.rule_ids), c.describe()
        for (k, by, lowest, ranked, rule), t in zip(c.tops, w.tops):
            assert np.array_equal(topref.ranking_py(w.sc, t.cand, t.flags), t.rank), c.describe()
            heap = topref.top_heap(w.sc, t.cand, t.flags, k)
            assert np.array_equal(heap if ranked else np.sort(heap), t.ids), c.describe()
        assert np.array_equal(context_ids_loop(w.doc_first, *c.context), w.ctx_ids), c.describe()
        for want, ids, fmt, first in ((w.fmt_ranked, w.tops[w.ranked].ids, c.fmts[0], None),
                                      (w.fmt_ctx, w.ctx_ids, with_context_sep(c.fmts[1]), w.doc_first)):
            out, out_off = format_ref_loop(c.data, off, ids, fmt, first)
            assert np.array_equal(out, want[0]) and np.array_equal(out_off, want[1]), c.describe()
        # the one greedy walk over all documents is llref.greedy per document, back to back
        kp, kl, kd = w.kpos[w.fits], w.klens[w.fits], w.kdoc[w.fits]
        cutp = np.searchsorted(kd, np.arange(w.n_docs + 1), side="left")
        per = []
        for d in np.flatnonzero(np.diff(cutp)):
            a, b = int(cutp[d]), int(cutp[d + 1])
            pick, ex = greedy(kp[a:b] - off[d], kl[a:b], 0, off[d + 1] - off[d])
            assert ex == 0
            per.append(kp[a:b][pick])
        assert np.array_equal(np.concatenate(per) if per else np.empty(0, np.int64), w.sel_pos), c.describe()
    print(f"second forms on {ran} seeds of at most {SECOND_FORM_DOCS} documents, scores_by_find on {found}")
    assert ran >= 20 and found >= 3
