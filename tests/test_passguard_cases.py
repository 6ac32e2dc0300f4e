"""The cases of tests/passguard.py and its exact-capacity protocol, checked without a GPU: every case's expectation is
built by the CPU references, its preconditions are asserted (no case is left out at run time, every case meant to have
output has some, every listed shape occurs), every reference is held against a second, independent one, and
`exact_call` itself is run against fake passes written in numpy that break the contract one way each."""
import numpy as np
import pytest

import wordref
from docref import oracle_per_doc
from docreplref import per_doc
from heapguard import E_ARG, E_OVERFLOW, FILLS, GUARD, TILE, GuardedBuffer, GuardError
from llref import check_greedy, greedy
from passfuzz import record_width
from passguard import (DOC_SHAPES, EMPTY_AT, EMPTY_RUN, FILTERED, GROUP, LADDER, LADDER_ENTRY, LADDER_STRETCH, OK, SEL_COUNTS, SIZE_CASES,
                       TABLES, WIDTHS, WINDOW_N, DocCut, Judge, Want, bad_offsets, cpu, cut_by_hand, exact_call)
from replref import greedy_replace, re_replace

PATS = (2, 4)                           # the two pattern sets (width 8 is the 16 lines again, under PFAC_WIDE)
SCANS = SIZE_CASES + (FILTERED,)


def test_three_tables_three_record_widths():
    x = cpu()
    for W in WIDTHS:
        assert record_width(int(x.table(W).num_final), TABLES[W]["knobs"]) == W
    assert int(x.table(2).num_final) <= 16 and x.table(8) is x.table(2)
    assert all(len(p) >= 2 for p in x.tinfo(2)["lines"])
    assert sum(len(p) == 1 for p in x.tinfo(4)["lines"]) == 1 and b"i" in x.tinfo(4)["lines"]     # what the "noi" input avoids


# ---------------------------------------------------------------------------
# scans, selections, replaces

@pytest.mark.parametrize("name", SCANS)
@pytest.mark.parametrize("W", PATS)
def test_scan_cases(W, name):
    x = cpu()
    key = x.size_key(name)
    inp, no, na, filt = key
    pos, ids, lens = x.scan(W, key)
    data = x.input(inp)
    assert na <= data.size and no <= na
    if name == "none":
        assert pos.size == 0
    else:
        assert pos.size > 0 and (np.diff(pos) >= 0).all() and int(pos.max()) < no and int((pos + lens).max()) <= na
        assert x.tile_counts(W, key).min() > 0, "a tile without a record: the input is not text-like everywhere"
    want_tiles = {"t3": 4, "t63": 63, "t64": 64, "t65": 65, "t130": 131, FILTERED: 65}
    if name in want_tiles:
        assert x.tile_counts(W, key).size == want_tiles[name]
    if name == "halo":
        assert no < na and ((pos + lens) > no).any(), "no record runs into the halo"
    # the selection: the loop against the vectorised characterisation
    spos, sids, ex = x.sel(W, key)
    ll = x.tinfo(W)["ll"]
    assert check_greedy(pos, lens, (spos, ll[sids]), 0, no) == ex
    assert (spos.size > 0) == (name != "none")
    # the replace: greedy + splice against Python's re for the 16 literal lines
    out = x.replace(W, key)
    again, ex2 = greedy_replace(data, 0, no, pos, lens, ids, x.rep_table(W))
    assert np.array_equal(out, again) and ex2 == ex
    if W == 2 and not filt:
        ref, ex3 = re_replace(x.tinfo(W)["lines"], x.reps(W), data[:na], 0, no)
        assert np.array_equal(out, ref) and ex3 == ex
    assert out.size > 0


@pytest.mark.parametrize("W", PATS)
def test_filtered_scan_has_holes_inside_runs(W):
    x = cpu()
    key = x.size_key(FILTERED)
    inp, no, na, _ = key
    pos, ids, lens = x.scan(W, key[:3] + (False,))
    keep = wordref.filter_words(x.input(inp)[:na], pos, lens)
    assert np.array_equal(keep, wordref.filter_words_loop(x.input(inp)[:na], pos, lens))
    kpos = x.scan(W, key)[0]
    assert np.array_equal(kpos, pos[keep]) and 0 < kpos.size < pos.size
    tile = pos // TILE
    inner = ~keep[1:-1] & keep[:-2] & keep[2:] & (tile[:-2] == tile[2:])       # a dropped record between two kept ones of its tile
    assert inner.any(), "no hole inside a tile's run"
    assert (x.tile_counts(W, key) != x.tile_counts(W, key[:3] + (False,))).all(), "a tile the filter left alone"


@pytest.mark.parametrize("W", PATS)
def test_selection_sizes(W):
    x = cpu()
    for count in SEL_COUNTS:
        key = x.sel_key(W, count)
        assert x.sel(W, key)[0].size == count and key[1] < key[2]
        pos, ids, lens = x.scan(W, key)
        spos, sids, ex = x.sel(W, key)
        assert check_greedy(pos, lens, (spos, x.tinfo(W)["ll"][sids]), 0, key[1]) == ex
        assert x.replace(W, key).size > 0
    assert {63, 65} <= set(SEL_COUNTS) and {1023, 1025} <= set(SEL_COUNTS)


@pytest.mark.parametrize("W", WIDTHS)
def test_expand_windows(W):
    x = cpu()
    for key in (x.size_key("t130"), x.size_key("t130")[:3] + (True,)):
        windows, (c0, G, T) = x.windows(W, key)
        assert T == x.scan(W, key)[0].size and len(windows) == len(set(windows))
        firsts = {f for f, _ in windows}
        assert firsts == {0, 1, c0 - 1, c0, c0 + 1, G - 1, G, G + 1, T - 1, T}
        for f in firsts:
            ns = {n for ff, n in windows if ff == f}
            assert T - f in ns and ns == {n for n in WINDOW_N + (T - f,) if f + n <= T}
        assert all(f + n <= T for f, n in windows)


# ---------------------------------------------------------------------------
# the replace ladder

def test_replace_ladder():
    x = cpu()
    W = 2
    sizes = x._ladder_sizes(W)
    outs = {}
    for name in LADDER:
        key, entry = x.ladder_key(W, name)
        inp, no, na, _ = key
        out = x.replace(W, key, entry)
        pos, ids, lens = x.scan(W, key)
        ref, ex = re_replace(x.tinfo(W)["lines"], x.reps(W), x.input(inp)[:na], entry, no)
        assert np.array_equal(out, ref) and ex == x.sel(W, key, entry)[2]
        if entry == 0:
            assert out.size == sizes[no], "the ladder's arithmetic and the reference disagree"
        outs[name] = (out.size, key, entry, ex)
    assert {outs[f"res{r}"][0] % 16 for r in range(16)} == set(range(16)), "the ladder misses a residue of out_bytes mod 16"
    assert all(outs[f"res{r}"][0] % 16 == r and outs[f"res{r}"][0] > 4112 for r in range(16))
    assert 0 < outs["lt16"][0] < 16
    assert outs["zero"][0] == 0 and outs["zero"][1][1] > 0 and x.sel(W, outs["zero"][1])[0].size == 10
    assert 1008 <= outs["k1"][0] <= 1040 and 4080 <= outs["k4"][0] <= 4112
    assert outs["entry"][2] == LADDER_ENTRY > 0 and outs["entry"][3] > 0
    # the stretch: more than 64 consecutive picks with empty replacements and no gap between them
    spos, sids, _ = x.sel(W, outs["gallop"][1])
    ll, (roff, _) = x.tinfo(W)["ll"], x.rep_table(W)
    head = slice(0, LADDER_STRETCH)
    assert LADDER_STRETCH > 3 * 64 and np.array_equal(spos[head], 3 * np.arange(LADDER_STRETCH))
    assert (ll[sids[head]] == 3).all() and (roff[sids[head] + 1] == roff[sids[head]]).all()
    assert spos.size > LADDER_STRETCH and outs["gallop"][0] > 0
    reps = x.reps(W)
    assert any(len(r) == 0 for r in reps.values()) and any(len(r) > len(x.tinfo(W)["lines"][i - 1]) for i, r in reps.items())
    assert any(0 < len(r) < len(x.tinfo(W)["lines"][i - 1]) for i, r in reps.items())


# ---------------------------------------------------------------------------
# documents

def _rules_hold(off, no):
    o = off.astype(np.int64)
    return bool(o[0] == 0 and o[-1] == no and (np.diff(o) >= 0).all())


def _doc_params():
    return [(W, "docs", s) for W in PATS for s in DOC_SHAPES] + [(W, n, "rand") for W in PATS for n in SCANS]


@pytest.mark.parametrize("case", _doc_params(), ids=lambda c: f"w{c[0]}-{c[1]}-{c[2]}")
def test_document_cases(case):
    x = cpu()
    W, name, shape = case
    key = x.doc_key(shape) if name == "docs" else x.size_key(name)
    inp, no, na, filt = key
    off = x.offsets(W, key, shape)
    assert _rules_hold(off, no) and off.dtype == np.uint64
    for bad in bad_offsets(off, no):
        assert bad.size == off.size and not _rules_hold(bad, no)
    pos, ids, lens = x.scan(W, key)
    first, dpos, dids = x.seg(W, key, shape)
    sfirst, spos, sids, out_off, out = x.docsel(W, key, shape)
    nd = off.size - 1
    assert first.size == sfirst.size == out_off.size == nd + 1 and int(first[-1]) == dpos.size and int(sfirst[-1]) == spos.size
    # the cut by hand against every document scanned on its own (a filtered scan: its kept records, document by document)
    data = np.ascontiguousarray(x.input(inp)[:no])
    matcher = (lambda: DocCut((pos, ids, lens), off)) if filt else (lambda: x.tinfo(W)["matcher"])
    wfirst, wpos, wids = oracle_per_doc(matcher(), data, off)
    assert np.array_equal(first, wfirst) and np.array_equal(dpos, wpos) and np.array_equal(dids, wids)
    # one greedy and one splice over the whole buffer against greedy and splice per document
    pfirst, ppos, pids, pout_off, pout = per_doc(matcher(), data, off, x.tinfo(W)["ll"], x.rep_table(W))
    doc = np.repeat(np.arange(nd, dtype=np.int64), np.diff(pfirst.astype(np.int64)))
    assert np.array_equal(sfirst, pfirst) and np.array_equal(spos, ppos + off.astype(np.int64)[doc]) and np.array_equal(sids, pids)
    assert np.array_equal(out_off, pout_off) and np.array_equal(out, pout) and int(out_off[-1]) == out.size
    # the conditions on the case
    if shape == "nothing":
        assert pos.size > 0 and dpos.size == 0 and spos.size == 0, "the batch that keeps nothing must still scan something"
    elif name == "none":
        assert pos.size == 0
    elif name == "docs":
        assert 0 < dpos.size < pos.size and 0 < spos.size, "a document case keeps fewer records than it scanned, and some"
    else:
        assert 0 < dpos.size <= pos.size and 0 < spos.size
    assert out.size > 0


@pytest.mark.parametrize("W", PATS)
def test_offset_shapes(W):
    """Every listed shape is what its name says."""
    x = cpu()
    shapes = {s: x.offsets(W, x.doc_key(s), s).astype(np.int64) for s in DOC_SHAPES}
    no = x.doc_key("one")[1]
    assert no > 65 * TILE and shapes["one"].tolist() == [0, no]
    assert np.diff(shapes["big"]).min() >= 64                                       # the lane-shuffle window
    starts = np.bincount(shapes["tiny"][:-1] // TILE, minlength=66)
    assert starts[1] >= 63 and starts[2] >= 63 and starts[63] >= 63 and starts[64] >= 63  # the binary-search path, at a group edge too
    for s, at in EMPTY_AT.items():
        at = no if at is None else at
        o = shapes[s]
        assert EMPTY_RUN >= 200 and int((o == at).sum()) >= EMPTY_RUN + (at in (0, no)), f"{s}: no run of empty documents at {at}"
    assert EMPTY_AT["empty0"] == 0 and EMPTY_AT["emptymid"] % TILE and EMPTY_AT["emptytile"] % TILE == 0 and EMPTY_AT["emptytile"] % GROUP
    assert EMPTY_AT["emptygroup"] == GROUP < no and shapes["emptyend"][-EMPTY_RUN - 1:].tolist() == [no] * (EMPTY_RUN + 1)
    key = x.doc_key("cut")
    pos, _, lens = x.scan(W, key)
    inside = np.isin(shapes["cut"], np.concatenate([pos[lens >= 2] + 1]))
    assert inside[1:-1].all() and x.seg(W, key, "cut")[1].size < 0.8 * pos.size, "the cuts go through matches"
    nkey = x.doc_key("nothing")
    assert shapes["nothing"].tolist() == list(range(nkey[1] + 1))
    assert set(DOC_SHAPES) == set(shapes) and len(DOC_SHAPES) == 10


# ---------------------------------------------------------------------------
# the protocol against fake passes

class _Sync:
    def sync(self, slot):
        pass


def _fake(bufs, records, first, stray=None, stray_value=0x5A, dirty_refusal=False, report=0, late_refusal=False):
    """A pass in numpy over host GuardedBuffers: writes `records` and `first` at the exact capacity, refuses one below."""
    def put(name, raw, at=0):
        a = bufs[name].tensor.numpy()
        a[bufs[name].front + at:bufs[name].front + at + raw.size] = raw

    def call(cap, bad=None):
        if bad is not None:
            if late_refusal:
                put("d_doc_first", first.view(np.uint8)[:8])
            return E_ARG, None
        if cap < records.size:
            if dirty_refusal:
                put("d_doc_first", np.zeros(8, np.uint8), at=first.nbytes - 8)
            return E_OVERFLOW, records.size + report
        put("d_out", records.view(np.uint8))
        put("d_doc_first", first.view(np.uint8))
        if stray is not None:
            put(stray, np.array([stray_value], np.uint8), at=bufs[stray].n_bytes)
        return OK, records.size + report
    return call


def _run_fake(fill, n=5, front=GUARD, **kw):
    records = np.arange(n, dtype=np.uint64) * np.uint64(0x0101010101010101)
    first = np.array([0, 2, n], dtype=np.uint64)
    bufs = {"d_out": GuardedBuffer(n * 8, front=front, fill=fill, device="cpu"), "d_doc_first": GuardedBuffer(24, fill=fill, device="cpu")}
    want = Want(n, {"d_out": Judge(n * 8, lambda raw: np.testing.assert_array_equal(raw.view(np.uint64), records)), "d_doc_first": first}, bad=2)
    exact_call(_Sync(), _fake(bufs, records, first, **kw), want, bufs, fill, "fake pass")


@pytest.mark.parametrize("fill", FILLS)
def test_protocol_passes_a_correct_pass(fill):
    _run_fake(fill)
    _run_fake(fill, n=0)                                        # the zero result: a payload of no byte, out_cap 0
    _run_fake(fill, front=GUARD + 16)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name", ["d_out", "d_doc_first"])
def test_protocol_catches_one_byte_past_the_payload(fill, name):
    with pytest.raises(GuardError, match=rf"back guard of {name} damaged: 1 bytes, first at \+0, last at \+0"):
        _run_fake(fill, stray=name)
    with pytest.raises(GuardError, match="back guard of d_out damaged"):
        _run_fake(fill, n=0, stray="d_out")


def test_protocol_needs_both_fills():
    """A stray byte that equals one fill goes unseen under it and shows under the other."""
    _run_fake(FILLS[0], stray="d_out", stray_value=FILLS[0])
    with pytest.raises(GuardError):
        _run_fake(FILLS[1], stray="d_out", stray_value=FILLS[0])


@pytest.mark.parametrize("fill", FILLS)
def test_protocol_catches_a_write_before_a_refusal(fill):
    """... in a buffer that was not the one too small, and behind rule-breaking arguments."""
    with pytest.raises(GuardError, match=r"payload of d_doc_first after the refused call \(out_cap 4\) damaged"):
        _run_fake(fill, dirty_refusal=True)
    with pytest.raises(GuardError, match=r"payload of d_doc_first after the refused call \(rule-breaking variant 0\) damaged"):
        _run_fake(fill, late_refusal=True)


@pytest.mark.parametrize("fill", FILLS)
def test_protocol_catches_a_wrong_count(fill):
    with pytest.raises(AssertionError, match="the overflow reports 4, want 5"):
        _run_fake(fill, report=-1)


def test_protocol_wants_exact_buffers():
    bufs = {"d_out": GuardedBuffer(48, device="cpu")}
    with pytest.raises(AssertionError, match="a buffer of 48 bytes"):
        exact_call(_Sync(), lambda cap, bad=None: (OK, 5), Want(5, {"d_out": np.zeros(5, np.uint64)}), bufs, FILLS[0])
