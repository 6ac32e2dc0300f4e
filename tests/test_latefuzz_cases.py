"""CPU side of the late-pass fuzzer (tests/latefuzz.py): every expectation of every suite seed is computed on the host,
and the conditions below say that the seeds reach what the GPU file is there to test -- so that a GPU run cannot pass
by checking nothing.  The two vectorised checkers are pinned to their loop forms, the template reference to Python's
`re`, and the directed inputs of the piece ladder and the offsets rule to the edges they are named for."""
import numpy as np
import pytest

import groupref
import spanref
import tplref
from latefuzz import (GROUP, KNOBS, LADDER_EDGES, LADDER_MODES, LADDER_PATTERNS, LADDER_TOTALS, RULE_BAD, RULE_BYTES,
                      RULE_DOCS, RULE_PATTERNS, SEEDS, TILE, WIN, LateCase, expectation, knob_label, ladder_cases, pick_layout,
                      piece_boundaries, record_width, rule_expect, rule_offsets)
from llref import greedy
from orc import Oracle

LOOP_MAX = 50_000                        # records up to which the loop forms of the checkers run


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("late"))
    out = []
    for s in SEEDS:
        c, w = expectation(s, tmp)
        out.append((c, w, c.table(f"{tmp}/late_{s}.pat")))
    return out


def test_seed_alone_fixes_the_case():
    a, b = LateCase(7), LateCase(7)
    assert a.describe() == b.describe() and np.array_equal(a.data, b.data) and np.array_equal(a.off, b.off)
    assert a.lines == b.lines and a.templates == b.templates and a.rules == b.rules
    assert LateCase(7, KNOBS[1]).knobs == KNOBS[1] and a.knobs == KNOBS[7 % len(KNOBS)]


def test_seeds_cover_knobs_widths_tables_and_are_well_formed(cases):
    runs, widths, small, big, folded, ready63 = {}, set(), 0, 0, 0, 0
    for c, w, table in cases:
        runs[knob_label(c.knobs)] = runs.get(knob_label(c.knobs), 0) + 1
        assert table.max_pat_len == c.M
        widths.add(record_width(table.num_final, c.knobs))
        small += table.num_final <= 64
        big += table.num_final > 64
        folded += c.folded
        off = c.off.astype(np.int64)
        assert off[0] == 0 and off[-1] == c.n_owned and (np.diff(off) >= 0).all()
        assert 0 <= c.entry <= c.M and 1 <= c.n_owned <= c.n == c.data.size
        assert not any(bytes([c.delim]) in p or b"\n" in p for p in c.lines)
        assert len(c.rules) == len(c.lines) + 1 == len(c.templates) + 1 == len(c.reps) + 1 == c.group_masks.size
        if c.lines_half:
            assert np.array_equal(w.split, off)
            assert (c.data[c.n_owned - 1] == c.delim) == c.terminated
        if c.ready_masks and (w.masks >> np.uint64(63)).any():
            ready63 += 1
    print(f"knob sets {runs}; widths {sorted(widths)}; <= 64 final states {small}, > 64 {big}; folded {folded}; "
          f"ready masks with bit 63 in a document's mask {ready63}")
    assert sorted(runs) == sorted(knob_label(k) for k in KNOBS) and min(runs.values()) >= 4
    assert widths == {2, 4, 8}
    assert small >= 10 and big >= 10 and folded >= 10 and ready63 >= 1


def test_the_filter_the_selection_and_the_masks_have_work(cases):
    sized = both = empty_sel = no_mask = searched = straddle = two_waves = 0
    for c, w, _ in cases:
        off = w.off
        kept_and_dropped = 0 < w.kpos.size < w.pos.size
        # a kept record whose tail was judged, in a document that ends in the delimiter
        end = off[w.kdoc + 1]
        judged = w.spans[2][w.keep] != spanref.ANY
        term = np.zeros(w.kpos.size, dtype=bool)
        if c.delim_arg is not None:
            some = end > off[w.kdoc]
            term[some] = c.data[end[some] - 1] == c.delim_arg
        if c.n >= 4095:
            sized += 1
            both += bool(kept_and_dropped and (judged & term).any())
        empty_sel += w.sel[0].size == 0
        no_mask += not (w.masks != 0).any()
        starts = np.bincount(off[:-1] // TILE, minlength=c.n // TILE + 2)
        kept_tiles = np.bincount(w.kpos // TILE, minlength=starts.size)
        searched += bool(((starts > 63) & (kept_tiles > 0)).any())
        # a document across a multiple of 64 tiles with a kept record that carries a group and ends inside it, each side
        fits = (w.kpos + w.klens <= end) & (c.group_masks[w.kids] != 0)
        for edge in range(GROUP, c.n_owned, GROUP):
            d = int(np.searchsorted(off, edge, side="right")) - 1
            if off[d] < edge < off[d + 1]:
                mine = fits & (w.kdoc == d)
                near, far = mine & (w.kpos < edge), mine & (w.kpos >= edge)
                if near.any() and far.any():
                    straddle += 1
                    # ... and the far side carries a group that the near side does not: the mask needs both waves
                    m = c.group_masks[w.kids]
                    two_waves += bool(int(np.bitwise_or.reduce(m[far])) & ~int(np.bitwise_or.reduce(m[near])))
                    break
    print(f"of {sized} seeds with n >= 4095, {both} keep and drop records and keep one with a judged tail in a terminated "
          f"document; {empty_sel} empty selections; {no_mask} without a mask; {searched} with kept records in a tile of "
          f"more than 63 document starts; {straddle} with a grouped document across a 64-tile edge, {two_waves} of them "
          f"with a group on the far side alone")
    assert 4 * both >= 3 * sized
    assert empty_sel <= 6 and no_mask <= 6
    assert searched >= 8 and straddle >= 5 and two_waves >= 2


def test_piece_boundaries_meet_every_byte_of_a_chunk(cases):
    rep = [set() for _ in range(4)]
    ext = [set() for _ in range(4)]
    long_out = identity = deletion = 0
    for c, w, _ in cases:
        pos, lens, ids = w.sel
        for k, b in enumerate(piece_boundaries(pos, lens, ids, c.templates, c.entry, c.n_owned)):
            rep[k] |= set((b % 16).tolist())
        for k, b in enumerate(piece_boundaries(pos, lens, ids, c.templates, c.entry, c.n_owned, extract=True)):
            ext[k] |= set((b % 16).tolist())
        # the layout the boundaries come from is the reference output's own: every 97th rewritten pick, where it says
        o, E, *_ = pick_layout(pos, lens, ids, c.templates, c.entry, c.n_owned)
        xo, xE, *_ = pick_layout(pos, lens, ids, c.templates, c.entry, c.n_owned, extract=True)
        assert np.array_equal(xo.astype(np.uint64), w.whole.pick_off[:-1])
        raw = bytes(c.data)
        for k in range(0, pos.size, 97):
            e = tplref.rewrite(tplref.by_id(c.templates)[int(ids[k])], raw[int(pos[k]):int(pos[k] + lens[k])])
            assert w.whole.replaced[int(o[k]):int(o[k] + E[k])] == e == w.whole.extracted[int(xo[k]):int(xo[k] + xE[k])]
        long_out += bool(len(w.whole.replaced) > 4096 and (((o + 16) % WIN) < 32).any())
        picked = {c.templates[int(i)] for i in set(ids.tolist())}
        identity += (b"", b"") in picked
        deletion += b"" in picked
    print(f"residues met: replace {[len(s) for s in rep]}, extraction {[len(s) for s in ext[1:]]}; {long_out} seeds with more "
          f"than 4096 bytes out and a segment within 16 bytes of a window's edge; identity picked in {identity} seeds, "
          f"deletion in {deletion}")
    assert all(len(s) == 16 for s in rep) and all(len(s) == 16 for s in ext[1:])
    assert long_out >= 10 and identity >= 1 and deletion >= 1
    assert any(len(t[0]) >= 1000 for c, w, _ in cases for i in set(w.sel[2].tolist()) for t in [c.templates[int(i)]]
               if isinstance(t, tuple)), "no pick with a prefix longer than an output window"


def test_the_vectorised_checkers_equal_their_loops(cases):
    ran = 0
    for c, w, _ in cases:
        if w.pos.size > LOOP_MAX:
            continue
        ran += 1
        dl = -1 if c.delim_arg is None else c.delim_arg
        assert np.array_equal(w.keep, spanref.filter_spans_loop(c.data, w.pos, w.lens, *w.spans, dl, w.off, c.n)), c.describe()
        if w.keep_nodocs is not None:
            assert np.array_equal(w.keep_nodocs, spanref.filter_spans_loop(c.data, w.pos, w.lens, *w.spans, dl, None, c.n))
        assert np.array_equal(w.match_ids, groupref.predicate_loop(w.masks, **c.predicate)), c.describe()
    assert ran >= 20


def test_the_template_reference_equals_re(cases):
    ran = 0
    for c, w, _ in cases:
        if c.folded or len(c.lines) > 20:
            continue
        ran += 1
        sel, ex = greedy(w.pos, w.lens, c.entry, c.n_owned)     # (no span filter: `re` knows no spans)
        a = tplref.assemble(c.data, c.entry, c.n_owned, w.pos[sel], w.lens[sel], w.ids[sel], c.templates)
        b = tplref.re_templates(c.lines, c.templates, c.data, c.entry, c.n_owned)
        assert (a.replaced, a.extracted, a.exit, a.n_picks) == (b.replaced, b.extracted, b.exit, b.n_picks), c.describe()
        assert np.array_equal(a.pick_off, b.pick_off) and a.exit == ex
    assert ran >= 8


# ---------------------------------------------------------------------------
def test_the_piece_ladder_meets_its_edges(tmp_path):
    pf = tmp_path / "ab.pat"
    pf.write_bytes(b"".join(p + b"\n" for p in LADDER_PATTERNS))
    o = Oracle(str(pf), 1, 1)
    res = {m: [set() for _ in range(4)] for m in LADDER_MODES}
    at = {m: [set() for _ in range(4)] for m in LADDER_MODES}
    totals = {m: set() for m in LADDER_MODES}
    for lc in ladder_cases():
        pos, ids = o.scan_spec(lc.data, None)
        assert np.array_equal(pos, lc.pos) and pos.size == len(lc.gaps) and lc.data.size < 65536
        off = lc.off.astype(np.int64)
        assert off[0] == 0 and off[-1] == lc.data.size and not np.isin(off, lc.pos + 1).any()   # no cut inside a pick
        for m in LADDER_MODES:
            out, pick_off, bs = lc.want("templated" if m == "documents" else m)
            assert len(out) < 65536
            if m == "documents":                                # every document on its own, concatenated: the same bytes
                per = b""
                for a, b in zip(off[:-1], off[1:]):
                    mine = (pos >= a) & (pos < b)
                    per += tplref.assemble(lc.data[a:b], 0, b - a, pos[mine] - a, np.full(int(mine.sum()), 2), ids[mine],
                                           lc.templates(m)).replaced
                assert per == out
            totals[m].add(len(out))
            for k, b in enumerate(bs):
                at[m][k] |= set(b.tolist())
                if lc.name.startswith("steps"):
                    res[m][k] |= set((b % 16).tolist())
    o.close()
    kinds = {"plain": (0, 3), "templated": (0, 1, 2, 3), "extract": (1, 2, 3), "documents": (0, 1, 2, 3)}
    for m in LADDER_MODES:
        for k in kinds[m]:
            assert len(res[m][k]) == 16, (m, k, sorted(res[m][k]))
            assert set(LADDER_EDGES) <= at[m][k], (m, k, sorted(set(LADDER_EDGES) - at[m][k]))
        assert set(LADDER_TOTALS) <= totals[m], (m, sorted(totals[m]))
    steps = [lc for lc in ladder_cases() if lc.name.startswith("steps")]
    assert {lc.pre for lc in steps} == {lc.suf for lc in steps} == set(range(18)) == {g for lc in steps for g in lc.gaps}


def test_the_offsets_rule_input_gives_every_call_work(tmp_path):
    pf = tmp_path / "r.pat"
    pf.write_bytes(b"".join(p + b"\n" for p in RULE_PATTERNS))
    w = rule_expect(str(pf))
    assert w.data.size == RULE_BYTES and set(w.ids.tolist()) == {1, 2, 3, 4}
    assert (w.masks != 0).sum() > 10_000 and 0 < w.fits.sum() < w.pos.size
    assert 0 < w.spans.sum() < w.words.sum() < w.pos.size


def test_the_broken_offsets_break_one_rule_each():
    good = rule_offsets().astype(np.int64)
    assert good.size == RULE_DOCS + 1 and good[0] == 0 and good[-1] == RULE_BYTES and (np.diff(good) >= 0).all()
    assert RULE_DOCS > 256 * 256                                # more than one pass of the widest check grid's first stride
    where = {"decrease-0": 0, "decrease-255": 255, "decrease-65535": 65535, "decrease-last": RULE_DOCS - 1}
    for name in RULE_BAD:
        off = rule_offsets(name).astype(np.int64)
        down = np.flatnonzero(np.diff(off) < 0)
        if name in where:
            assert down.tolist() == [where[name]] and off[-1] == RULE_BYTES
            assert (off[0] == 0) == (name != "decrease-0")
        else:
            assert down.size == 0 and (off[0] != 0) == (name == "first-not-0") and (off[-1] != RULE_BYTES) == (name == "last-not-n_owned")
