"""Document scores on the GPU (run with -m gpu on an MI355X): pfac_table_set_state_weights, pfac_documents_scores,
pfac_selection_document_scores, pfac_document_scores_d2h and pfac_documents_matching_scores against tests/scoreref.py --
the scans and offsets of tests/groupref.py, whose preconditions tests/test_score_ref.py asserts without a GPU -- with
guard bands around the caller's buffers (heapguard, the protocol of passguard.exact_call).  Integer work: bit-exact.
No expectation comes from the device."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import scoreref
import wordref
from fmtref import Fmt, format_ref
from gatherref import gather_ref
from heapguard import FILLS, TILE, GuardedBuffer
from llref import greedy
from nocaseref import expected as folded_scan
from orc import Oracle
from passguard import OK, Device, Want, bad_offsets, cut_by_hand, exact_call
from phfpfac_amd import SCORE_DTYPE, GpuMatcher, PfacError, PfacTable
from phfpfac_amd import _ffi
from phfpfac_amd.matcher import tiled_bytes
from scoreref import I64_MAX, I64_MIN, SHAPES, TILES, U64_MAX, cases, predicate, scores_cut, scores_of_selection, totals, weights_for
from spanref import filter_spans as ref_filter_spans
from spanref import record_spans
from splitref import split_offsets

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("charclass_oracle", os.path.join(REPO, "oracle", "charclass_oracle.py"))
cco = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cco)
DATA = os.path.join(REPO, "tests", "golden", "data")
E_ARG, E_STATE, E_OVERFLOW = _ffi.PFAC_E_ARG, _ffi.PFAC_E_STATE, _ffi.PFAC_E_OVERFLOW


def status_of(fn):
    with pytest.raises(PfacError) as e:
        fn()
    return e.value.status


def n_ids_of(table):
    ids = np.asarray(getattr(table, "out_ids", table.idmap), dtype=np.int64)
    return max(int(table.n_patterns), int(ids.max()) if ids.size else 0)


def upload(arr, slack=0):
    raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
    t = torch.zeros(max(raw.size + slack, 16), dtype=torch.uint8, device="cuda:0")
    if raw.size:
        t[:raw.size].copy_(torch.from_numpy(raw.copy()))
    torch.cuda.synchronize()
    return t


def same(got, want, what=""):
    assert got.dtype == SCORE_DTYPE and got.size == want.size, what
    for f in ("count", "score"):
        ne = np.flatnonzero(got[f] != want[f])
        assert ne.size == 0, (f"{what}: {ne.size} of {want.size} {f}s differ, first at document {int(ne[0])}: "
                              f"{int(got[f][ne[0]])}, want {int(want[f][ne[0]])}")


class Dev:
    """passguard's Device of record width W with the test weights set, and the planted text resident."""

    def __init__(self, W):
        self.W, self.c = W, cases()
        self.d = Device(W, self.c.x)
        self.g = self.d.g
        self.weights = weights_for(n_ids_of(self.d.table))
        self.g.set_pattern_weights(self.weights)
        self.by_id = scoreref.w_by_id(self.weights)
        self.text = upload(self.c.text, slack=TILE)
        self.tiles = None

    def scan(self, tiles):
        if self.tiles == tiles:
            return
        self.tiles = self.d.cur = None
        no = self.c.n_owned(tiles)
        self.g.reserve(0, 0, max(no, TILE))
        n = self.g.scan_resident(no, no, d_input=self.text)
        assert n == self.c.scan(self.W, tiles)[0].size
        assert self.g.scan_format()[0] == self.W
        self.tiles = tiles


@pytest.fixture(scope="module")
def devs():
    made = {}

    def get(W):
        if W not in made:
            made[W] = Dev(W)
        return made[W]
    yield get
    for d in made.values():
        d.d.close()


# ---------------------------------------------------------------------------
# the scores: record widths, weight forms, sizes, offset shapes

@pytest.mark.parametrize("tiles", TILES)
@pytest.mark.parametrize("W", [2, 4, 8])
def test_scores_equal_reference(devs, W, tiles):
    """Widths 2 and 8 hold 16 final states (lengths and weights in lane registers), width 4 the dictionary's (gathers).
    Every offset shape of groupref.SHAPES, twice: the scores, the counts and the totals, and the same again -- the
    memset and the atomics start clean."""
    d = devs(W)
    d.scan(tiles)
    g = d.g
    assert (d.d.table.num_final <= 64) == (W != 4)
    for shape in SHAPES:
        off = d.c.offsets(W, tiles, shape)
        want = scoreref.want(W, tiles, shape)
        nd = off.size - 1
        d_off = upload(off)
        for rep in range(2):
            total = g.document_scores(nd, d_doc_offsets=d_off)
            same(g.document_scores_to_host(nd), want, f"{shape} run {rep}")
            assert total == totals(want), shape
    # the slot's own offsets (NULL)
    off = d.c.offsets(W, tiles, "mid")
    g.set_doc_offsets(off)
    assert g.document_scores(off.size - 1) == totals(scoreref.want(W, tiles, "mid"))
    same(g.document_scores_to_host(off.size - 1), scoreref.want(W, tiles, "mid"), "the slot's offsets")


def test_zero_and_cancelling_weights_still_count(devs):
    d = devs(2)
    d.scan(65)
    g, c = d.g, d.c
    pos, ids, lens = c.scan(2, 65)
    n_ids = n_ids_of(d.d.table)
    cancels = False
    try:
        for shape in ("tiny", "huge", "cut"):
            off = c.offsets(2, 65, shape)
            nd = off.size - 1
            g.set_doc_offsets(off)
            first = cut_by_hand(pos, ids, lens, off)[0]
            g.set_pattern_weights([0] * (n_ids + 1))
            assert g.segment_records(nd) == int(first[-1])
            dev_first = g.segment_to_host(int(first[-1]), nd)[0]
            np.testing.assert_array_equal(dev_first, first)
            assert g.document_scores(nd) == (0, int(first[-1]))
            got = g.document_scores_to_host(nd)
            assert (got["score"] == 0).all(), shape
            np.testing.assert_array_equal(got["count"], np.diff(first), err_msg=shape)
            assert (got["count"] > 0).any()
            alt = [0] + [1 if i % 2 else -1 for i in range(1, n_ids + 1)]
            g.set_pattern_weights(alt)
            want = scores_cut(pos, ids, lens, off, scoreref.w_by_id(alt))
            cancels |= bool(((want["count"] > 0) & (want["score"] == 0)).any())
            assert g.document_scores(nd) == totals(want)
            same(g.document_scores_to_host(nd), want, f"{shape} +1/-1")
    finally:
        g.set_pattern_weights(d.weights)
    assert cancels, "no document whose +1 / -1 cancel"


def dense_case():
    pat = os.path.join(DATA, "experimentpattern")
    unit = open(os.path.join(DATA, "experimentinput"), "rb").read()
    data = tiled_bytes(66 * TILE + 123, unit)
    o = Oracle(pat, 1, 1)
    pos, ids = o.scan_spec(data)
    o.close()
    pos, ids = pos.astype(np.int64), ids.astype(np.int64)
    lens = np.array([0] + [len(x) for x in open(pat, "rb").read().split(b"\n")[:-1]], dtype=np.int64)[ids]
    rng = np.random.default_rng(5)
    shapes = {"one": np.array([0, data.size]), "tiles": np.arange(0, data.size + TILE, 3 * TILE + 100).clip(0, data.size),
              "small": np.concatenate([[0], np.sort(rng.integers(1, data.size, 3000)), [data.size]])}
    return pat, data, pos, ids, lens, {k: np.unique(v).astype(np.uint64) for k, v in shapes.items()}


def test_dense_input_carries_runs_across_chunks_and_tiles():
    """The headline pattern set on its own input, tiled: more than 64 records in a tile, documents longer than a chunk of
    64 records and longer than a tile, so the open run is carried across both -- what an add-twice or a dropped carry
    fails.  The segment pass's output of the same scan, given as the caller's arrays, is the selection kernel's dense
    case: many waves, documents that straddle their ranges."""
    pat, data, pos, ids, lens, shapes = dense_case()
    assert np.bincount(pos // TILE).max() > 64
    t = PfacTable.from_file(pat, 256)
    weights = [0] + [i % 7 - 3 for i in range(1, n_ids_of(t) + 1)]
    by_id = scoreref.w_by_id(weights)
    with GpuMatcher(0, 1) as g:
        g.load_table(t)
        g.set_pattern_weights(weights)
        for name, off in shapes.items():
            want = scores_cut(pos, ids, lens, off, by_id)
            if name == "tiles":                                 # every document's records fill more than one chunk
                assert np.bincount(np.searchsorted(off.astype(np.int64), pos, side="right") - 1).min() > 64
            same(g.score_documents((data, off)), want, name)
            assert want["score"].any() and int(want["count"].sum()) > 64 * 66
            nd = off.size - 1
            kept = g.segment_records(nd)
            assert kept == int(want["count"].sum()) and kept > 4 * 256
            d_rec = torch.zeros(kept * 8, dtype=torch.uint8, device="cuda:0")
            d_first = torch.zeros((nd + 1) * 8, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            assert g.segment_records(nd, d_out=d_rec, out_cap=kept, d_doc_first=d_first) == kept
            assert g.selection_document_scores(nd, d_sel=d_rec, d_doc_first=d_first) == totals(want)
            same(g.document_scores_to_host(nd), want, name + " through the segment pass")


def test_class_table_with_a_multi_id_state():
    pats = b"[a-c]x\nax\n[^a-z0-9 ]\nq[0-9][0-9]\n[a-c]\nax[xy]\n[a-c]x\n"
    weights = weights_for(7)
    rng = np.random.default_rng(78)
    alphabet = np.frombuffer(b"abcxyzq0123456789 AB-!", dtype=np.uint8)
    data = alphabet[rng.integers(0, alphabet.size, 2 * TILE + 55)]
    off = np.unique(np.concatenate([[0, data.size, TILE], rng.integers(0, data.size, 400)])).astype(np.uint64)
    parsed = cco.parse(pats)
    plen = np.array([0] + [len(p) for p in parsed], dtype=np.int64)
    pos, ids = cco.match(pats, data, parsed)
    ids = ids.astype(np.int64)
    # a state that ends several patterns is ONE record whose weight is their sum: the score is the sum over the
    # oracle's (pos, id) rows, the count the number of distinct (pos, state) among them
    t = PfacTable.from_charclass(pats, 256)
    assert any(t.out_first[s + 1] - t.out_first[s] > 1 for s in range(t.num_final))
    state_of = {}
    for s in range(t.num_final):
        for i in t.out_ids[t.out_first[s]:t.out_first[s + 1]]:
            state_of.setdefault(int(i), []).append(s)
    rows = scores_cut(pos, ids, plen[ids], off, scoreref.w_by_id(weights))
    with GpuMatcher(0, 1) as g:
        g.load_table(t)
        g.set_pattern_weights(weights)
        got = g.score_documents((data, off))
        first, rec = g.scan_documents((data, off))
    np.testing.assert_array_equal(got["score"], rows["score"])
    np.testing.assert_array_equal(got["count"], np.diff(first))
    assert (got["count"] <= rows["count"]).all() and (got["count"] < rows["count"]).any() and int(got["count"].sum()) == rec.size
    assert (rows["count"] == 0).any() and (rows["score"] != 0).any()


def test_after_the_filters(devs):
    d = devs(2)
    d.scan(65)
    g, c = d.g, d.c
    no = c.n_owned(65)
    pos, ids, lens = c.scan(2, 65)
    off = c.offsets(2, 65, "mid")
    nd = off.size - 1
    d_off = upload(off)
    keep = wordref.filter_words(c.text[:no], pos, lens, off=off.astype(np.int64))
    assert 0 < keep.sum() < keep.size
    want = scores_cut(pos[keep], ids[keep], lens[keep], off, d.by_id)
    assert (want["count"] != scoreref.want(2, 65, "mid")["count"]).any()
    rules = [None] + ["^" if i % 3 == 0 else None for i in range(1, n_ids_of(d.d.table) + 1)]
    try:
        assert g.filter_whole_words(0, n_docs=nd, d_doc_offsets=d_off, d_input=d.text) == int(keep.sum())
        assert g.document_scores(nd, d_doc_offsets=d_off) == totals(want)
        same(g.document_scores_to_host(nd), want, "after the whole-word filter")
        # the span filter over a fresh scan: "^" rules, the documents' starts being the lines' starts
        d.tiles = None
        d.scan(65)
        g.set_pattern_spans(rules)
        smin, smax, stail = record_spans(rules, ids)
        keep2 = ref_filter_spans(c.text[:no], pos, lens, smin, smax, stail, off=off.astype(np.int64), n_avail=no)
        assert 0 < keep2.sum() < keep2.size
        want2 = scores_cut(pos[keep2], ids[keep2], lens[keep2], off, d.by_id)
        assert g.filter_spans(0, None, False, n_docs=nd, d_doc_offsets=d_off, d_input=d.text) == int(keep2.sum())
        assert g.document_scores(nd, d_doc_offsets=d_off) == totals(want2)
        same(g.document_scores_to_host(nd), want2, "after the span filter")
    finally:
        d.tiles = None                                          # (the filters changed the slot's records)
        g.set_pattern_spans([None] * len(rules))


def test_folded_scan_under_a_nocase_table():
    pats = b"The\nhe\nAND\nwith\nThat\n"
    weights = [0, 3, 0, -3, 1, -(2 ** 31)]
    para = open(os.path.join(DATA, "paragraph402"), "rb").read()
    data = tiled_bytes(5 * TILE + 9, para).copy()
    data[::7] = np.frombuffer(bytes(data[::7]).upper(), dtype=np.uint8)
    pos, ids = folded_scan(pats, data)
    pos, ids = pos.astype(np.int64), ids.astype(np.int64)
    lens = np.array([0, 3, 2, 3, 4, 4], dtype=np.int64)[ids]
    off = np.unique(np.concatenate([[0, data.size], np.arange(97, data.size, 211)])).astype(np.uint64)
    want = scores_cut(pos, ids, lens, off, scoreref.w_by_id(weights))
    t = PfacTable.from_bytes(pats, 256, ignore_case=True)
    with GpuMatcher(0, 1) as g:
        g.load_table(t)
        assert g.case_fold
        g.set_pattern_weights(weights)
        got = g.score_documents((data, off))
    same(got, want, "folded")
    assert (want["score"] != 0).any() and ((want["count"] > 0) & (want["score"] == 0)).any() and 0 < int(want["count"].sum()) < pos.size


# ---------------------------------------------------------------------------
# the selection

def picks_of(pos, ids, lens, off, no):
    """The per-document leftmost-longest picks: the kept records never cross a document's end, so the greedy walk over
    them restarts at every document by itself.  -> (doc_first, pattern ids of the picks)."""
    first, _, kid, keep, kd = cut_by_hand(pos, ids, lens, off)
    sel = greedy(pos[keep], lens[keep], 0, no)[0]
    pfirst = np.searchsorted(kd[sel], np.arange(off.size), side="left").astype(np.uint64)
    return pfirst, kid[sel]


@pytest.mark.parametrize("W,tiles", [(4, 65), (2, 130)])
def test_selection_scores(devs, W, tiles):
    d = devs(W)
    d.scan(tiles)
    g, c = d.g, d.c
    no = c.n_owned(tiles)
    pos, ids, lens = c.scan(W, tiles)
    for shape in ("tiny", "huge", "empties"):
        off = c.offsets(W, tiles, shape)
        nd = off.size - 1
        g.set_doc_offsets(off)
        pfirst, pids = picks_of(pos, ids, lens, off, no)
        want = scores_of_selection(pfirst, pids, d.by_id)      # (indexed by the picks' pattern ids)
        assert (want["count"] < scoreref.want(W, tiles, shape)["count"]).any(), "no overlapping match was dropped"
        assert g.select_leftmost_longest_documents(nd) == pids.size
        for _ in range(2):
            assert g.selection_document_scores(nd) == totals(want), shape
            same(g.document_scores_to_host(nd), want, f"picks, {shape}")
        # the segment pass's output as the caller's arrays: exactly pfac_documents_scores of the same scan
        full = scoreref.want(W, tiles, shape)
        kept = int(full["count"].sum())
        d_rec = torch.zeros(max(kept, 1) * 8, dtype=torch.uint8, device="cuda:0")
        d_first = torch.zeros((nd + 1) * 8, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert g.segment_records(nd, d_out=d_rec, out_cap=kept, d_doc_first=d_first) == kept
        assert g.selection_document_scores(nd, d_sel=d_rec, d_doc_first=d_first) == totals(full)
        same(g.document_scores_to_host(nd), full, f"segment arrays, {shape}")
        g.document_scores(nd)
        same(g.document_scores_to_host(nd), full, f"heap, {shape}")
    # rule-breaking arrays: PFAC_E_ARG, the caller's buffer untouched, the slot's result discarded
    off = c.offsets(W, tiles, "tiny")
    nd = off.size - 1
    g.set_doc_offsets(off)
    full = scoreref.want(W, tiles, "tiny")
    kept = int(full["count"].sum())
    first, _, kid, keep, _ = cut_by_hand(pos, ids, lens, off)
    state_of_id = {int(i): s for s, i in enumerate(np.asarray(d.d.table.idmap)[: d.d.table.num_final])}
    rec = np.zeros(kept, dtype=np.dtype([("pos", "<u4"), ("state", "<u4")]))
    rec["state"] = [state_of_id[int(i)] for i in kid]
    out = GuardedBuffer(nd * 16, fill=FILLS[0])
    assert g.selection_document_scores(nd, d_sel=upload(rec), d_doc_first=upload(first), d_out=out.ptr) == totals(full)
    g.sync(0)
    out.check(what="d_scores_out")
    same(out.host().view(SCORE_DTYPE), full, "host-made arrays")
    assert status_of(lambda: g.document_scores_to_host(nd)) == E_STATE          # they went to the caller's buffer
    out = GuardedBuffer(nd * 16, fill=FILLS[1])
    descending = first.copy()
    descending[nd // 2] = first[nd // 2 + 1] + np.uint64(1)
    assert descending[0] == 0 and descending[-1] == first[-1]
    assert status_of(lambda: g.selection_document_scores(nd, d_sel=upload(rec), d_doc_first=upload(descending), d_out=out.ptr)) == E_ARG
    nonzero = first.copy()
    nonzero[0] = 1
    assert status_of(lambda: g.selection_document_scores(nd, d_sel=upload(rec), d_doc_first=upload(nonzero), d_out=out.ptr)) == E_ARG
    wrong = rec.copy()
    wrong["state"][kept // 2] = d.d.table.num_final
    assert status_of(lambda: g.selection_document_scores(nd, d_sel=upload(wrong), d_doc_first=upload(first), d_out=out.ptr)) == E_ARG
    g.sync(0)
    out.check(payload_untouched=True, what="d_scores_out of the refused calls")
    g.selection_document_scores(nd, d_sel=upload(rec), d_doc_first=upload(first))
    assert status_of(lambda: g.selection_document_scores(nd, d_sel=upload(wrong), d_doc_first=upload(first))) == E_ARG
    assert status_of(lambda: g.document_scores_to_host(nd)) == E_STATE          # a failed call discards the slot's result
    assert status_of(lambda: g.selection_document_scores(nd, d_sel=upload(rec))) == E_ARG       # one NULL, one not
    d_first = upload(first)
    assert status_of(lambda: g.selection_document_scores(nd, d_sel=upload(rec), d_doc_first=int(d_first.data_ptr()) + 4)) == E_ARG
    # the slot's own selection goes stale with the next scan
    g.select_leftmost_longest_documents(nd)
    g.selection_document_scores(nd)
    assert status_of(lambda: g.selection_document_scores(nd + 1)) == E_ARG      # not that selection's n_docs
    d.tiles = None
    d.scan(tiles)
    assert status_of(lambda: g.selection_document_scores(nd)) == E_STATE


# ---------------------------------------------------------------------------
# guard bands

@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("W,tiles,shape", [(2, 65, "cut"), (4, 65, "tiny"), (8, 3, "empties"), (2, 130, "huge")])
def test_caller_buffers_at_exact_capacity(devs, W, tiles, shape, fill):
    """d_scores_out of exactly n_docs x 16 bytes: rule-breaking offsets are refused with every byte untouched, the call
    proper writes the scores and no byte more.  Then d_ids_out of exactly n_matching x 8: one entry too few gives
    PFAC_E_OVERFLOW with the exact count and an untouched buffer."""
    d = devs(W)
    d.scan(tiles)
    g = d.g
    off, want = d.c.offsets(W, tiles, shape), scoreref.want(W, tiles, shape)
    nd = off.size - 1
    d_off = upload(off)
    d_bad = [upload(b) for b in bad_offsets(off, d.c.n_owned(tiles))]
    buf = {"d_scores_out": GuardedBuffer(nd * 16, fill=fill)}

    def call(cap, bad=None):
        st, got = d.d._status(lambda: g.document_scores(nd, d_doc_offsets=d_off if bad is None else d_bad[bad], d_out=buf["d_scores_out"].ptr))
        assert st != OK or got == totals(want)
        return st, None
    exact_call(g, call, Want(nd, {"d_scores_out": want}, bad=len(d_bad), capped=False), buf, fill, f"pfac_documents_scores width {W} {tiles} tiles {shape}")
    assert status_of(lambda: g.document_scores_to_host(nd)) == E_STATE          # they went to the caller's buffer
    assert status_of(lambda: g.matching_documents_scored(nd, min_count=1)) == E_STATE
    for kw in (dict(min_count=1), dict(min_score=1, max_count=5), dict(max_score=-1, invert=True), dict(density=(1, 1000), min_count=2)):
        ids = predicate(want, off, **kw)
        ibuf = {"d_ids_out": GuardedBuffer(ids.size * 8, fill=fill)}

        def icall(cap, bad=None):
            return d.d._status(lambda: g.matching_documents_scored(nd, d_scores=buf["d_scores_out"].ptr, d_doc_offsets=d_off,
                                                                   d_out=ibuf["d_ids_out"].ptr, out_cap=cap, **kw), "n_matching")
        exact_call(g, icall, Want(ids.size, {"d_ids_out": ids}), ibuf, fill, f"pfac_documents_matching_scores {kw}")
    buf["d_scores_out"].check(what="the d_scores of a predicate")


# ---------------------------------------------------------------------------
# the contract

def test_state_errors_come_first_and_in_order():
    c = cases()
    table = c.x.table(2)
    weights = weights_for(n_ids_of(table))
    by_id = scoreref.w_by_id(weights)
    w = table.state_weights(weights)
    text = c.text[:3 * TILE]
    off = np.array([0, 100, 100, 3 * TILE], dtype=np.uint64)
    d_off = upload(off)
    odd = int(d_off.data_ptr()) + 4                              # a misaligned pointer: an argument error
    with GpuMatcher(0, 1) as g:
        L, ctx = g._L, g._ctx
        assert L.pfac_table_set_state_weights(ctx, w.ctypes.data, w.size) == E_STATE              # before an upload
        g.load_table(table)
        assert L.pfac_table_set_state_weights(ctx, w.ctypes.data, w.size + 1) == E_ARG
        assert L.pfac_table_set_state_weights(ctx, None, w.size) == E_ARG
        # state before arguments: no finished scan, with a misaligned pointer and n_docs = 2^32
        assert status_of(lambda: g.document_scores(1 << 32, d_doc_offsets=odd)) == E_STATE
        g.reserve(0, text.size, TILE)
        g.h2d(text)
        g.scan_resident(text.size, text.size)
        assert status_of(lambda: g.document_scores(3, d_doc_offsets=odd)) == E_STATE              # no final lengths
        g.set_final_lengths(table.final_lengths())
        assert status_of(lambda: g.document_scores(3, d_doc_offsets=odd)) == E_STATE              # no state weights
        assert status_of(lambda: g.selection_document_scores(3, d_sel=odd, d_doc_first=odd)) == E_STATE
        g.set_pattern_weights(weights)
        assert status_of(lambda: g.document_scores(3)) == E_STATE                                 # no offsets for the slot
        assert status_of(lambda: g.document_scores_to_host(3)) == E_STATE                         # no scores yet
        assert status_of(lambda: g.matching_documents_scored(3, min_count=1)) == E_STATE
        assert status_of(lambda: g.selection_document_scores(3)) == E_STATE                       # no selection
        # a wrong n_states leaves the earlier weights
        assert L.pfac_table_set_state_weights(ctx, w.ctypes.data, w.size - 1) == E_ARG
        # arguments
        assert status_of(lambda: g.document_scores(3, d_doc_offsets=odd)) == E_ARG
        assert status_of(lambda: g.document_scores(3, d_doc_offsets=d_off, d_out=int(d_off.data_ptr()) + 8)) == E_ARG    # 16-B
        assert status_of(lambda: g.document_scores(1 << 32, d_doc_offsets=d_off)) == E_ARG
        assert status_of(lambda: g.document_scores(3, d_doc_offsets=d_off, d_records=int(d_off.data_ptr()))) == E_ARG
        assert status_of(lambda: g.document_scores(0, d_doc_offsets=d_off)) == E_ARG              # no documents, but bytes
        g.set_doc_offsets(off)
        assert status_of(lambda: g.document_scores(2)) == E_STATE                                 # not the slot's n_docs
        total = g.document_scores(3)
        pos, ids = c.x.tinfo(2)["matcher"].scan_spec(np.ascontiguousarray(text), None)
        pos, ids = pos.astype(np.int64), ids.astype(np.int64)
        lens = c.x.tinfo(2)["ll"][ids]
        want = scores_cut(pos, ids, lens, off, by_id)
        assert total == totals(want) and want["count"][1] == 0 and want["count"][0] > 0
        # the window fetches
        same(g.document_scores_to_host(3), want)
        same(g.document_scores_to_host(3, first=1, n=2), want[1:])
        assert g.document_scores_to_host(3, first=3, n=0).size == 0
        assert status_of(lambda: g.document_scores_to_host(3, first=2, n=2)) == E_ARG
        assert status_of(lambda: g.document_scores_to_host(3, first=4, n=0)) == E_ARG
        # the predicate's arguments
        assert status_of(lambda: g.matching_documents_scored(2, min_count=1)) == E_ARG            # NULL scores, another n_docs
        n = C.c_uint64(0)
        rule = _ffi.CScoreRule(I64_MIN, I64_MAX, 1, U64_MAX, 0, 0)
        d_sc = upload(want)
        assert L.pfac_documents_matching_scores(ctx, 0, None, None, 3, C.byref(rule), 2, None, 0, C.byref(n)) == E_ARG     # flags
        assert L.pfac_documents_matching_scores(ctx, 0, None, None, 3, None, 0, None, 0, C.byref(n)) == E_ARG              # no rule
        assert L.pfac_documents_matching_scores(ctx, 0, int(d_sc.data_ptr()) + 8, None, 3, C.byref(rule), 0, None, 0, C.byref(n)) == E_ARG
        assert L.pfac_documents_matching_scores(ctx, 0, int(d_sc.data_ptr()), None, 1 << 32, C.byref(rule), 0, None, 0, C.byref(n)) == E_ARG
        # a failed pass discards the slot's scores
        assert g.matching_documents_scored(3, min_count=1) == predicate(want, min_count=1).size
        assert status_of(lambda: g.document_scores(3, d_doc_offsets=odd)) == E_ARG
        assert status_of(lambda: g.document_scores_to_host(3)) == E_STATE
        # a second call replaces the weights; the scores survive a later scan; an upload clears the weights
        g.set_pattern_weights([0] + [9] * (len(weights) - 1))
        assert g.document_scores(3) == (9 * int(want["count"].sum()), int(want["count"].sum()))
        np.testing.assert_array_equal(g.document_scores_to_host(3)["score"], 9 * want["count"].astype(np.int64))
        g.set_pattern_weights(weights)
        g.document_scores(3)
        g.scan_resident(TILE, TILE)
        same(g.document_scores_to_host(3), want)                                                  # through a later scan ...
        g.load_table(table)
        same(g.document_scores_to_host(3), want)                                                  # ... and an upload
        g.set_final_lengths(table.final_lengths())
        assert status_of(lambda: g.document_scores(3)) == E_STATE                                 # a scan of the earlier table
        g.scan_resident(text.size, text.size)
        assert status_of(lambda: g.document_scores(3)) == E_STATE                                 # the upload cleared the weights
        g.set_pattern_weights(weights)
        assert g.document_scores(3) == total
        # overflow is judged behind the state, in front of the arguments
        heap = torch.zeros(64 * 8, dtype=torch.uint8, device="cuda:0")
        g.scan_async(text.size, d_records=heap, capacity=64)
        assert g.scan_finish(allow_overflow=True)[1]
        assert status_of(lambda: g.document_scores(3, d_doc_offsets=odd, d_records=heap)) == E_OVERFLOW
        # no documents and no bytes
        g.scan_resident(0, 0)
        g.set_doc_offsets(np.zeros(1, dtype=np.uint64))
        assert g.document_scores(0) == (0, 0)
        assert g.document_scores_to_host(0).size == 0
        assert g.matching_documents_scored(0, min_count=1) == 0


def test_predicate_matches_reference(devs):
    """Caller's scores made on the host and uploaded (the predicate takes any device array): windows, both infinities,
    invert, densities whose products pass 2^63.  Then the slot's own scores, whose ids feed both gathers."""
    d = devs(2)
    d.scan(65)
    g, c = d.g, d.c
    no = c.n_owned(65)
    rng = np.random.default_rng(0x5C1)
    special = [I64_MIN, I64_MIN + 1, -(2 ** 62), -3, -1, 0, 1, 3, 2 ** 62, I64_MAX - 1, I64_MAX]
    n = 64 * 64 + 70                                            # two groups of the compaction, the second one short
    score = np.array((special * (n // len(special) + 1))[:n], dtype=np.int64)
    score[100:4000] = rng.integers(-50, 50, 3900)
    count = np.array(([0, 1, 2, U64_MAX, U64_MAX - 1, 2 ** 63, 7] * (n // 7 + 1))[:n], dtype=np.uint64)
    sc = scoreref.make(score, count)
    lens = rng.integers(0, 2 ** 40, n).tolist()
    lens[5], lens[6], lens[7] = 2 ** 62, 2 ** 63, 0
    hoff = np.array(np.cumsum([0] + lens, dtype=object), dtype=np.uint64)
    d_sc, d_hoff = upload(sc), upload(hoff)
    windows = [dict(), dict(min_score=0), dict(max_score=0), dict(min_score=-3, max_score=3), dict(min_score=I64_MIN, max_score=I64_MAX),
               dict(min_score=I64_MAX), dict(max_score=I64_MIN), dict(min_count=1), dict(max_count=2), dict(min_count=2, max_count=U64_MAX - 1),
               dict(min_count=U64_MAX), dict(min_count=0, max_count=0), dict(min_score=1, min_count=1, max_count=7)]
    densities = [None, (1, 1000), (-1, 3), (I64_MAX, U64_MAX), (I64_MIN, U64_MAX), (-(2 ** 40), 2 ** 63 + 5), (3, 1)]
    seen = set()
    for kw in windows:
        for dens in densities:
            for inv in (False, True):
                ids = predicate(sc, hoff, density=dens, invert=inv, **kw)
                got_n = g.matching_documents_scored(n, density=dens, invert=inv, d_scores=d_sc, d_doc_offsets=d_hoff, **kw)
                assert got_n == ids.size, (kw, dens, inv)
                np.testing.assert_array_equal(g.matching_documents_to_host(got_n), ids, err_msg=str((kw, dens, inv)))
                seen.add(ids.size)
    assert 0 in seen and n in seen and len(seen) > 20
    # the 64-bit products of these two are equal, the 128-bit ones are not
    two = scoreref.make(np.array([2 ** 62, 2 ** 62], dtype=np.int64), np.array([1, 1], dtype=np.uint64))
    off2 = np.array([0, 2 ** 62, 2 ** 63], dtype=np.uint64)
    for dens, ids in (((4, 8), [0, 1]), ((8, 4), []), ((8, 8), [0, 1]), ((9, 8), [])):
        assert predicate(two, off2, density=dens).tolist() == ids
        assert g.matching_documents_scored(2, density=dens, d_scores=upload(two), d_doc_offsets=upload(off2)) == len(ids)
        assert g.matching_documents_to_host(len(ids)).tolist() == ids
    # density with NULL offsets: the slot's, and none at all
    off, want = c.offsets(2, 65, "tiny"), scoreref.want(2, 65, "tiny")
    nd = off.size - 1
    with GpuMatcher(0, 1) as g2:
        g2.load_table(d.d.table)
        assert status_of(lambda: g2.matching_documents_scored(nd, density=(1, 1000), d_scores=upload(want))) == E_STATE
        assert g2.matching_documents_scored(nd, min_count=1, d_scores=upload(want)) == predicate(want, min_count=1).size
    g.set_doc_offsets(off)
    assert g.document_scores(nd) == totals(want)
    sizes = []
    for kw in (dict(min_count=1), dict(min_count=3), dict(min_score=1, density=(1, 10)), dict(density=(-1, 3), max_count=0),
               dict(max_score=-1), dict(min_count=1, invert=True), dict(min_score=I64_MAX, min_count=U64_MAX)):
        ids = predicate(want, off, **kw)
        sizes.append(ids.size)
        assert g.matching_documents_scored(nd, **kw) == ids.size, kw
        np.testing.assert_array_equal(g.matching_documents_to_host(ids.size), ids)
        out_bytes = g.gather_documents(nd, ids.size, no, d_input=d.text)
        ref_out, ref_off = gather_ref(c.text[:no], off, ids)
        assert out_bytes == ref_out.size
        np.testing.assert_array_equal(g.gathered_to_host(out_bytes), ref_out)
        np.testing.assert_array_equal(g.gathered_offsets_to_host(ids.size), ref_off)
        fmt = Fmt(number=True, byte_offset=True, terminate=0x0A, group_sep=b"--\n")
        out_bytes = g.gather_documents_formatted(nd, ids.size, no, d_input=d.text, **fmt.kwargs())
        ref_out, ref_off = format_ref(c.text[:no], off, ids, fmt)
        assert out_bytes == ref_out.size
        np.testing.assert_array_equal(g.gathered_to_host(out_bytes), ref_out)
        np.testing.assert_array_equal(g.gathered_offsets_to_host(ids.size), ref_off)
    assert sizes[-1] == 0 and 0 < sizes[1] < sizes[0] < nd and sizes[0] + sizes[5] == nd


# ---------------------------------------------------------------------------
# end to end

def test_scoring_a_small_log():
    lines = [b"GET /index.html 200 alice",          # 0: GET, alice
             b"POST /login 403 bob",                # 1: 403, bob
             b"",                                   # 2
             b"GET /admin 500 root error",          # 3: GET, root, error
             b"error: disk full",                   # 4: error
             b"alice and bob",                      # 5: alice, bob
             b"nothing here",                       # 6
             b"error error alice root",             # 7: error x 2, alice, root
             b"assassin bob",                       # 8: ass x 2, assassin, bob
             b"root root root",                     # 9: root x 3
             b"GET 403 GET",                        # 10: GET x 2, 403
             b"errors and assassins"]               # 11: error, ass x 2, assassin
    #        id:   1      2    3      4     5    6    7    8
    pats = b"alice\nbob\nerror\nroot\nGET\n403\nass\nassassin\n"
    weights = [0, 1, 1, -2, 5, 0, -5, 2, 10]
    data = np.frombuffer(b"\n".join(lines) + b"\n" + b"bob error", dtype=np.uint8)       # 12: bob, error (no newline)
    off = split_offsets(data, 0x0A)[0]
    score = [1, -4, 0, 3, -2, 2, 0, 2, 15, 15, -5, 12, -1]
    count = [2, 2, 0, 3, 1, 2, 0, 4, 4, 3, 3, 4, 2]
    # non-overlapping: "assassin" is one pick, the "ass" inside it none
    score_no = [1, -4, 0, 3, -2, 2, 0, 2, 11, 15, -5, 8, -1]
    count_no = [2, 2, 0, 3, 1, 2, 0, 4, 2, 3, 3, 2, 2]
    want, want_no = scoreref.make(score, count), scoreref.make(score_no, count_no)
    by_find = scoreref.scores_by_find(data, off, pats.split(b"\n")[:-1], scoreref.w_by_id(weights))
    np.testing.assert_array_equal(by_find, want)                # the values written out above are what bytes.find counts
    t = PfacTable.from_bytes(pats, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(t)
        g.set_pattern_weights(weights)
        docs = [bytes(data[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])]
        same(g.score_documents(docs), want, "score_documents")
        same(g.score_documents(docs, non_overlapping=True), want_no, "score_documents, non-overlapping")
        got_off, got = g.score_lines(data)
        np.testing.assert_array_equal(got_off, off)
        same(got, want, "score_lines")
        same(g.score_lines(data, non_overlapping=True)[1], want_no, "score_lines, non-overlapping")
        # whole words: "errors", "assassins" and the "ass" inside them go
        ww = g.score_lines(data, whole_words=True)[1]
        assert ww["count"].tolist() == [2, 2, 0, 3, 1, 2, 0, 4, 2, 3, 3, 0, 2]
        assert ww["score"].tolist() == [1, -4, 0, 3, -2, 2, 0, 2, 11, 15, -5, 0, -1]
        for kw, no in ((dict(min_count=3), False), (dict(min_score=3), False), (dict(min_score=12), True), (dict(max_score=-1), False),
                       (dict(min_count=1, invert=True), False), (dict(density=(1, 2), min_count=1), False), (dict(min_count=3, max_count=3), True)):
            ref = want_no if no else want
            ids = predicate(ref, off, **kw)
            out, out_off, got_ids = g.grep_lines_scored(data, non_overlapping=no, **kw)
            ref_out, ref_off = gather_ref(data, off, ids)
            np.testing.assert_array_equal(got_ids, ids, err_msg=str(kw))
            np.testing.assert_array_equal(out, ref_out)
            np.testing.assert_array_equal(out_off, ref_off)
        assert g.grep_lines_scored(data, min_count=3)[2].tolist() == [3, 7, 8, 9, 10, 11]
        assert g.grep_lines_scored(data, min_score=12, non_overlapping=True)[2].tolist() == [9]
        assert g.grep_lines_scored(data, density=(1, 2), min_count=1)[2].tolist() == [8, 9, 11]
        # weight 1 everywhere, a count of one or more: grep_lines
        g.set_pattern_weights([0] + [1] * 8)
        a = g.grep_lines_scored(data, min_score=1)
        b = g.grep_lines(data)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        assert a[2].size == 11
