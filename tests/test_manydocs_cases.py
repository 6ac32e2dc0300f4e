"""The cases of tests/manydocs.py checked without a GPU: every twin reference equals the existing reference on that
module's own cases, every case meets the preconditions that make it the case it is named for, and the check functions
refuse host-side stand-ins that are wrong in the ways tests/test_gpu_many_docs.py exists to find."""
import numpy as np
import pytest

import manydocs as md
import scoreref
import splitref
import topref
from fmtref import format_ref_loop
from gatherref import context_ids_loop, gather_ref_loop
from manydocs import (DOCS, EDGE, GROUP_DOCS, HIST_DOCS, HIST_TRIP, ID_GROUP, IDS, SORT_BLOCK, SPLIT_GROUP, groups_of, per_of,
                      total_owner)
from phfpfac_amd.matcher import tiled_bytes

SMALL = 301                             # where the one-at-a-time forms are run as well


# ---------------------------------------------------------------------------
# the twins

@pytest.mark.parametrize("n,keys,rule", topref.CASE_IDS, ids=[f"{n}-{k}-{r}" for n, k, r in topref.CASE_IDS])
def test_ranking_equals_toprefs(n, keys, rule):
    c = topref.case(n, keys, rule)
    for order in (0, topref.BY_COUNT, topref.LOWEST, topref.BY_COUNT | topref.LOWEST):
        assert np.array_equal(md.ranking(c.sc, c.cand, order), topref.ranking(c.sc, c.cand, order)), (c, order)


RULES = [dict(), dict(min_count=1), dict(min_score=-3, max_score=40, max_count=3), dict(density=(3, 1000)), dict(density=(-2, 7), invert=True),
         dict(density=md.DENSITY, **md.RULE), dict(density=md.RANK_DENSITY), dict(min_count=1, invert=True)]


@pytest.mark.parametrize("keys", ["perm", "sparse", "equal"])
@pytest.mark.parametrize("n", topref.SIZES)
def test_score_ids_equals_scorerefs_predicate(n, keys):
    sc = topref.keyset(keys, n)
    off = md.offsets_of(np.random.default_rng(n).integers(0, 5000, n))
    for kw in RULES:
        want = scoreref.predicate(sc, off, **kw)
        assert np.array_equal(md.score_ids(sc, off, **kw), want), (n, keys, kw)
        assert np.array_equal(want, scoreref.predicate_loop(sc, off, **kw))


def test_score_ids_refuses_products_it_cannot_hold():
    sc = topref.keyset("extremes", 65)
    with pytest.raises(AssertionError):
        md.score_ids(sc, md.offsets_of(np.ones(65, np.int64)), density=(1, 3))


@pytest.mark.parametrize("phase", [0, md.TILED_PHASE, 19, 31, 60])
def test_periodic_split_equals_splitrefs(phase):
    """The arithmetic split against split_offsets on the bytes themselves: lengths that end on a delimiter, behind one,
    in front of one, inside the empty document, and across a few periods and tiles."""
    P = len(md.TILED_PERIOD)
    for n in (0, 1, 2, P - 1, P, P + 1, 5 * P + 20, 5 * P + 31, 5 * P + 32, 3 * 4096 + 7, SPLIT_GROUP + 9):
        p = md.Periodic(n, md.TILED_PERIOD, phase)
        want, n_docs, tail = splitref.split_offsets(tiled_bytes(n, md.TILED_PERIOD, phase), md.NL)
        assert (p.n_docs, p.tail_start) == (n_docs, tail), (n, phase)
        assert np.array_equal(p.offsets(0, n_docs + 1), want), (n, phase)
        for byte in (0, 1, n // 2, max(n - 1, 0), n):
            assert p.index_at(byte) == int(np.searchsorted(want, byte, side="left")), (n, phase, byte)
        for first, count in md.split_windows(p):
            assert np.array_equal(p.offsets(first, count), want[first:first + count])


# ---------------------------------------------------------------------------
# the sizes

def test_sizes_cross_the_thresholds_they_are_named_for():
    assert [groups_of(n, GROUP_DOCS) for n in DOCS] == [1024, 1025, 2049]
    assert [per_of(groups_of(n, GROUP_DOCS)) for n in DOCS] == [1, 2, 3]
    assert [total_owner(groups_of(n, GROUP_DOCS)) for n in DOCS] == [1023, 512, 682]        # the last thread; half idle; a third
    assert [groups_of(n, ID_GROUP) for n in IDS] == [1024, 1025, 2049]
    assert [per_of(groups_of(n, ID_GROUP)) for n in IDS] == [1, 2, 3]
    assert [groups_of(n, HIST_TRIP) for n in HIST_DOCS] == [1, 2, 3, 8, 9, 17]              # trips of the histogram's loop
    assert (2 * HIST_TRIP + 65) % 256 == 65                                                 # the third trip: one wave and a lane
    # the sort's block histograms at k = 1024 groups of documents + 1: 256 counts per block, hundreds per thread of the scan
    blocks = groups_of(GROUP_DOCS * 1024 + 1, SORT_BLOCK)
    assert blocks == 4097 and per_of(256 * blocks) == 1025
    assert groups_of(md.ALL_DELIMS, SPLIT_GROUP) == 33 and md.ALL_DELIMS % 16 == 1
    assert groups_of(md.TILED_BYTES, SPLIT_GROUP) == 1025 and per_of(1025) == 2
    assert len(md.TILED_PERIOD) == 65
    p = md.Periodic(md.TILED_BYTES, md.TILED_PERIOD, md.TILED_PHASE)
    assert p.n_docs > DOCS[1] and p.c == 3 and p.open_tail
    assert len(md.split_windows(p)) == 1024 + 2


@pytest.mark.parametrize("n", DOCS)
def test_flag_patterns_put_the_truth_on_both_sides_of_group_1024(n):
    seen = {}
    for name in md.FLAGS:
        f = md.flags(name, n)
        assert f.size == n and np.array_equal(f, md.flags(name, n))             # a function of its name
        g = np.add.reduceat(f.astype(np.int64), np.arange(0, n, GROUP_DOCS))
        seen[name] = (int(g[:EDGE].sum()), int(g[EDGE:].sum()), int(g[EDGE - 1]))
    assert seen["all"] == (EDGE * GROUP_DOCS, n - EDGE * GROUP_DOCS, GROUP_DOCS)
    assert seen["none"] == (0, 0, 0)
    assert seen["late"] == (0, n - EDGE * GROUP_DOCS, 0)
    assert seen["last"][0] + seen["last"][1] == 1 and (n == DOCS[0] or seen["last"][0] == 0)
    assert seen["group_firsts"] == (EDGE, groups_of(n, GROUP_DOCS) - EDGE, 1)
    for name in ("all", "alternating", "runs", "group_firsts"):
        left, right, edge = seen[name]
        assert left > 0 and edge > 0 and (n == DOCS[0] or right > 0), name      # a prefix short by group 1023's sum shows


@pytest.mark.parametrize("n", [SMALL, DOCS[1]], ids=["small", "large"])
def test_the_truth_of_every_pattern_is_its_flags(n):
    """doc_first, masks and scores made from flags select exactly those documents (and, inverted, the others) under the
    existing references; the small size also under their one-at-a-time forms."""
    d = np.arange(n, dtype=np.uint64)
    off = md.offsets_of(md.doc_lengths(n))
    for name in md.FLAGS:
        f = md.flags(name, n)
        want = d[f]
        first, masks = md.doc_first_of(f), md.masks_of(f)
        assert np.array_equal(md.matching_ids(first), want) and np.array_equal(md.matching_ids(first, True), d[~f])
        assert np.array_equal(md.group_ids(masks, **md.WHERE), want)
        assert np.array_equal(md.group_ids(masks, invert=True, **md.WHERE), d[~f])
        assert np.array_equal(md.score_ids(md.scores_of(f), **md.RULE), want)
        assert np.array_equal(md.score_ids(md.scores_of(f, True), off, density=md.DENSITY, **md.RULE), want)
        if n == SMALL:
            assert np.array_equal(splitref.matching_ids_loop(first), want)
            assert np.array_equal(scoreref.predicate_loop(md.scores_of(f, True), off, density=md.DENSITY, **md.RULE), want)
            # without the density the dense scores select more: the density decides
            assert md.score_ids(md.scores_of(f, True), **md.RULE).size > want.size or name == "all"
            for b, a in ((1, 0), (0, 64), (n, n)):
                assert np.array_equal(md.context_ids(first, b, a), context_ids_loop(first, b, a))


# ---------------------------------------------------------------------------
# the rank

@pytest.mark.parametrize("n", [HIST_DOCS[1], HIST_DOCS[2]])
def test_rank_cases(n):
    for keys, rule in md.RANK_KEYS:
        c = md.rank_case(n, keys, rule)
        assert 0 < c.cand.size and (rule == "all") == (c.cand.size == n)
        for order in (0, topref.BY_COUNT | topref.LOWEST):
            rank = c.rank(order)
            ks = c.ks(order)
            assert rank.size == c.cand.size and {1, SORT_BLOCK, SORT_BLOCK + 1, c.cand.size, c.cand.size + 1} <= set(ks)
            b, e = md.tie_class(c.sc, rank, order)
            # the winners do not all lie in the histogram's first trip: from the tie class's middle on at the latest,
            # among the first ranks where the keys are distinct (one document past the trip: it is a candidate)
            k = (b + e) // 2 if keys == "ties" else SORT_BLOCK
            assert (rank[:k if n > HIST_TRIP + 1 else rank.size] >= HIST_TRIP).any(), (c, order)
            if keys == "ties":                                  # the class spans sort blocks, and its middle cuts it
                assert e - b > SORT_BLOCK and b // SORT_BLOCK < (e - 1) // SORT_BLOCK and b < (b + e) // 2 < e - 1
            else:
                assert e - b == 1


# ---------------------------------------------------------------------------
# the gather

def test_gather_cases():
    n_ids = IDS[1]
    g = md.gather_data(n_ids)
    lens = np.diff(g.offsets.astype(np.int64))
    assert lens.min() == 0 and lens.max() == 40
    for at in md.EMPTY_AT:
        assert lens[at:at + md.EMPTY_RUN].max() == 0 and md.EMPTY_RUN > 64 * ID_GROUP
    assert md.EMPTY_AT[0] % ID_GROUP == 0 and md.EMPTY_AT[1] % ID_GROUP != 0
    for name in md.ID_LISTS:
        ids = g.ids(name).astype(np.int64)
        assert ids.size == n_ids and 0 <= ids.min() and ids.max() < g.n_docs
        seg = np.add.reduceat(lens[ids], np.arange(0, n_ids, ID_GROUP))
        assert seg[:EDGE].sum() > 0 and seg[EDGE:].sum() > 0, name             # bytes on both sides of group 1024
        if name == "ascending":
            zero = np.flatnonzero(seg == 0)
            assert zero.size >= 2 * 63 and (np.diff(zero) == 1).sum() >= 2 * 62    # whole groups that sum to zero, in runs
            assert {999_999, 1_000_000} <= set((ids[999_990:1_000_010] + 1).tolist())
            o = g.offsets[ids].astype(np.int64)
            assert o.min() < 999_999 < 1_000_000 <= o.max()
    assert np.diff(g.ids("repeats").astype(np.int64)).min() == 0 and np.diff(g.ids("reversed").astype(np.int64)).max() == -1
    assert lens[md.SAME_ID] == 40
    # the reference, held against the loop form on a window of the ids
    for name, fmt in (("repeats", None), ("ascending", "both"), ("repeats", "context")):
        out, out_off = g.want(name, fmt)
        k = slice(1_000_000 - 40, 1_000_000 + 40)
        ids = g.ids(name)[k]
        if fmt is None:
            piece, _ = gather_ref_loop(g.data, g.offsets, ids)
        else:
            piece, _ = format_ref_loop(g.data, g.offsets, ids, md.Fmt(**md.FORMATS[fmt]), g.doc_first)
        lo = int(out_off[k.start])
        if fmt == "context":                                    # (the window's first id may or may not follow the one before it)
            sep = int(ids[0]) != int(g.ids(name)[k.start - 1]) + 1
            lo += 3 if sep else 0                               # format_ref_loop sets none in front of a first id
        assert bytes(out[lo:lo + piece.size]) == bytes(piece), (name, fmt)


def test_offsets_rule_cases():
    n_bytes, off, ids = md.rule_case()
    assert off.size - 1 == md.RULE_DOCS > md.RULE_BREAK and (np.diff(off.astype(np.int64)) >= 0).all() and int(off[-1]) == n_bytes
    assert int(ids[md.RULE_BREAK // 4]) == md.RULE_BREAK and int(ids[-1]) == md.RULE_DOCS - 1
    dec = md.broken_offsets(off, "decrease")
    bad = np.flatnonzero(np.diff(dec.astype(np.int64)) < 0)
    assert bad.tolist() == [md.RULE_BREAK] and int(dec[-1]) == n_bytes          # one decrease, at a selected document
    past = md.broken_offsets(off, "past_end")
    assert np.array_equal(past[:-1], off[:-1]) and int(past[-1]) == n_bytes + 1


# ---------------------------------------------------------------------------
# the checks refuse what these tests exist to find

def refused(fn, *words):
    with pytest.raises(AssertionError) as e:
        fn()
    assert all(w in str(e.value) for w in words), str(e.value)


@pytest.mark.parametrize("name", ["all", "alternating", "runs", "group_firsts"])
def test_a_prefix_short_by_one_groups_sum_is_refused(name):
    """A compaction whose groups >= 1024 start at a prefix that misses group 1023's sum: the right count, the ids of the
    late groups written over the end of the early ones."""
    n = DOCS[1] if name != "runs" else DOCS[2]
    want = md.matching_ids(md.doc_first_of(md.flags(name, n)))
    md.assert_ids(want, want.size, want, name)
    g = want.astype(np.int64) // GROUP_DOCS
    short = int((g == EDGE - 1).sum())
    at = np.arange(want.size) - np.where(g >= EDGE, short, 0)
    got = np.zeros(want.size, dtype=np.uint64)
    got[at] = want
    first = int(np.flatnonzero(g >= EDGE)[0]) - short
    refused(lambda: md.assert_ids(got, want.size, want, name), f"id {first} is")


def test_a_dropped_total_is_refused():
    want = md.matching_ids(md.doc_first_of(md.flags("alternating", DOCS[1])))
    refused(lambda: md.assert_ids(want, 0, want), "n_matching 0")
    refused(lambda: md.assert_ids(want[:0], 0, want), "n_matching 0")
    # the count of every group but those of the last owning thread
    refused(lambda: md.assert_ids(want[:-1], want.size - 1, want), "n_matching")
    c = md.rank_case(HIST_DOCS[1], "ties", "all")
    ids, n = md.top(c.rank(0), SORT_BLOCK, md.RANKED)
    refused(lambda: md.assert_top(ids, None, 0, c.sc, ids), "n_top 0")
    off = md.offsets_of(np.full(IDS[0], 3))
    out = np.zeros(int(off[-1]), dtype=np.uint8)
    md.assert_gather(out.size, off, out, out, off)
    lost = off.copy()
    lost[-1] = 0
    refused(lambda: md.assert_gather(out.size, lost, out, out, off), f"output offset {IDS[0]} is 0")
    refused(lambda: md.assert_gather(0, off, out, out, off), "out_bytes 0")


@pytest.mark.parametrize("keys,rule", md.RANK_KEYS)
def test_a_rank_of_the_first_trip_alone_is_refused(keys, rule):
    """A rank whose histogram never took its second trip: the best of the first 524 288 documents."""
    c = md.rank_case(HIST_DOCS[2], keys, rule)
    for flags in (md.RANKED, 0, md.RANKED | md.BY_COUNT | md.LOWEST):
        rank = c.rank(flags)
        fake = md.ranking(c.sc, c.cand[c.cand < HIST_TRIP], flags)
        b, e = md.tie_class(c.sc, rank, flags)
        for k in ((b + e) // 2 if keys == "ties" else SORT_BLOCK, c.cand.size):
            want, n = md.top(rank, k, flags)
            md.assert_top(want, c.sc[want.astype(np.int64)], n, c.sc, want)
            got, m = md.top(fake, k, flags)
            refused(lambda: md.assert_top(got, c.sc[got.astype(np.int64)], m, c.sc, want))
    # ... and one that counted the second trip and compacted the first alone: the right count, ids that differ
    k = min(int((c.cand < HIST_TRIP).sum()), c.cand.size // 2)
    want, n = md.top(c.rank(0), k, md.RANKED)
    got, _ = md.top(md.ranking(c.sc, c.cand[c.cand < HIST_TRIP], 0), k, md.RANKED)
    assert got.size == n
    refused(lambda: md.assert_top(got, None, n, c.sc, want), "differ")


def test_gather_offsets_right_for_1024_groups_only_are_refused():
    """Output offsets whose groups >= 1024 start from the prefix of group 1024 - 1 (one group's bytes short), and ones
    that restart at zero there; the bytes are right in both."""
    n_ids = IDS[2]
    lens = md.gather_lengths(n_ids)
    off = md.offsets_of(lens)
    out = (np.arange(int(off[-1])) % 251).astype(np.uint8)
    md.assert_gather(out.size, off, out, out, off)
    k = EDGE * ID_GROUP
    short = off.copy()
    short[k:] -= off[k] - off[k - ID_GROUP]
    refused(lambda: md.assert_gather(out.size, short, out, out, off), f"output offset {k} is")
    restart = off.copy()
    restart[k:] -= off[k]
    refused(lambda: md.assert_gather(out.size, restart, out, out, off), f"output offset {k} is")
    # the bytes of the late groups written where those short offsets point
    moved = out.copy()
    d = int(off[k] - off[k - ID_GROUP])
    moved[int(off[k]) - d:out.size - d] = out[int(off[k]):]
    refused(lambda: md.assert_gather(out.size, off, moved, out, off), "output byte")
    refused(lambda: md.assert_gather(out.size, off, np.append(out, [7, 0xA5]), out, off, fill=0xA5), "past the output's end")


def test_a_split_wrong_past_a_group_edge_is_refused():
    p = md.Periodic(8 * SPLIT_GROUP + 77, md.TILED_PERIOD, md.TILED_PHASE)
    want = p.offsets(0, p.n_docs + 1)
    wins = md.split_windows(p)
    fetch = lambda a, first, n: a[first:first + n]                 # noqa: E731
    md.assert_split(p.n_docs, p.tail_start, lambda f, n: fetch(want, f, n), p.n_docs, p.tail_start, wins, p.offsets)
    at = p.index_at(5 * SPLIT_GROUP)
    got = want.copy()
    got[at:] -= np.uint64(1)                                      # group 5 starts from a prefix that is one short
    refused(lambda: md.assert_split(p.n_docs, p.tail_start, lambda f, n: fetch(got, f, n), p.n_docs, p.tail_start, wins, p.offsets),
            f"offset {at} is")
    refused(lambda: md.assert_split(p.n_docs - 1, p.tail_start, lambda f, n: fetch(want, f, n), p.n_docs, p.tail_start, wins, p.offsets),
            "n_docs")
    refused(lambda: md.assert_split(p.n_docs, p.n, lambda f, n: fetch(want, f, n), p.n_docs, p.tail_start, wins, p.offsets), "tail_start")


# ---------------------------------------------------------------------------
# the heap-driven input

def test_heap_input(tmp_path):
    from orc import Oracle
    from passguard import cpu
    h = md.heap_input()
    off = h.offsets.astype(np.int64)
    lens = np.diff(off)
    assert h.n_docs > md.HEAP_BREAK + 1 > DOCS[1] and h.split[1] > DOCS[1]     # with the empty runs, and without (the chain)
    assert off[0] == 0 and off[-1] == h.n and lens.min() == 0 and h.n < 16 << 20
    assert int(h.data[-1]) != md.SPACE and h.split[2] < h.n                    # an unterminated last document
    full = lens[lens > 0]
    assert (full <= 2).sum() > 0.85 * full.size and (full == 1).sum() > 1_000_000 and (full == 2).sum() > 2_000_000
    for at in md.HEAP_EMPTY_AT:                                                # the runs: where they start, how long they are
        k = int(np.searchsorted(off, at, side="left"))
        assert (off[k:k + md.HEAP_EMPTY_RUN] == at).all() and md.HEAP_EMPTY_RUN - 1 > 4096 * 64
    assert md.HEAP_EMPTY_AT[0] % SPLIT_GROUP == 0 and md.HEAP_EMPTY_AT[1] % SPLIT_GROUP != 0
    assert groups_of(h.n, SPLIT_GROUP) >= 34 and int(np.bincount(off[:-1] // SPLIT_GROUP).max()) > md.HEAP_EMPTY_RUN
    x = cpu()
    tiles = groups_of(h.n, md.TILE)
    for W in (2, 4):
        pos, ids, lens_r = h.records(x.tinfo(W)["matcher"], x.tinfo(W)["ll"])
        first, rel, kids, keep, kd = md.cut_records(pos, ids, lens_r, h.offsets)
        assert 0 < int((~keep).sum()) and int(keep.sum()) > 500_000, W         # records cross document ends, most do not
        per_tile = np.bincount(pos // md.TILE, minlength=tiles)
        a, b = h.blank
        assert a % md.TILE == 0 and (b - a) // md.TILE > 64 and per_tile[a // md.TILE:b // md.TILE].max() == 0     # tiles with no record
        assert per_tile[b // md.TILE:].min() > 0 and per_tile[:md.HEAP_TEXT // md.TILE].min() > 0                  # records on both sides of them
        kept_docs = np.unique(kd)
        assert kept_docs[0] < 1000 and kept_docs[-1] > md.HEAP_BREAK           # documents with records at either end of the offsets
        # a document of one byte or two that keeps a record, and many one after the other (a tile of them holds thousands)
        assert (np.diff(off)[kept_docs] <= 3).sum() > 10_000, W
    # the single-byte table: comparison against the oracle, the byte map against bytes.replace per document
    path = tmp_path / "bytes.pat"
    path.write_bytes(b"".join(p + b"\n" for p in md.BYTE_PATTERNS))
    o = Oracle(str(path), 1, 1)
    pos, ids = o.scan_spec(h.data, None)
    bp, bi, bl = md.byte_records(h.data)
    assert np.array_equal(bp, pos) and np.array_equal(bi, ids) and bp.size > 1_000_000
    lo, hi = int(np.searchsorted(off, md.HEAP_TEXT - 3000)), int(np.searchsorted(off, md.HEAP_TEXT + 3000))
    out, out_off = md.byte_replace(h.data, h.offsets)
    data = bytes(h.data)
    for d in list(range(0, 300)) + list(range(lo, hi)) + list(range(h.n_docs - 300, h.n_docs)):
        doc = data[off[d]:off[d + 1]]
        for p, i in zip(md.BYTE_PATTERNS, sorted(md.BYTE_REPS)):
            doc = doc.replace(p, b"\x00" + bytes([i]))
        for i in sorted(md.BYTE_REPS):
            doc = doc.replace(b"\x00" + bytes([i]), md.BYTE_REPS[i])
        assert bytes(out[int(out_off[d]):int(out_off[d + 1])]) == doc, d
    assert int(out_off[-1]) == out.size and 0 not in h.data
    # the broken offsets break one rule each
    dec = h.broken("decrease").astype(np.int64)
    assert np.flatnonzero(np.diff(dec) < 0).tolist() == [md.HEAP_BREAK] and dec[-1] == h.n
    assert int(h.broken("past_end")[-1]) == h.n + 1
