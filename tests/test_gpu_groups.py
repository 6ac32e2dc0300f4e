"""Pattern groups on the GPU (run with -m gpu on an MI355X): pfac_table_set_state_groups, pfac_documents_group_masks,
pfac_group_masks_d2h and pfac_documents_matching_groups against tests/groupref.py -- the case list whose preconditions
tests/test_groups_ref.py asserts without a GPU, with guard bands around the caller's buffers (heapguard, the protocol
of passguard.exact_call).  Integer work: bit-exact.  No expectation comes from the device."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import wordref
from gatherref import gather_ref
from groupref import ALL, SHAPES, TILES, cases, groups_for, masks_by_id, masks_cut, predicate
from heapguard import FILLS, TILE, GuardedBuffer
from nocaseref import expected as folded_scan
from orc import Oracle
from passguard import OK, Device, Want, bad_offsets, cut_by_hand, exact_call
from phfpfac_amd import GpuMatcher, PfacError, PfacTable
from phfpfac_amd import _ffi
from phfpfac_amd.matcher import _ptr, tiled_bytes
from splitref import matching_ids, split_offsets

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


class Dev:
    """passguard's Device of record width W with the test grouping set, and the planted text resident."""

    def __init__(self, W):
        self.W, self.c = W, cases()
        self.d = Device(W, self.c.x)
        self.g = self.d.g
        self.g.set_pattern_groups(groups_for(n_ids_of(self.d.table)))
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
# the masks: record widths, mask forms, sizes, offset shapes

@pytest.mark.parametrize("tiles", TILES)
@pytest.mark.parametrize("W", [2, 4, 8])
def test_masks_equal_reference(devs, W, tiles):
    """Widths 2 and 8 hold 16 final states (lengths and masks in lane registers), width 4 the dictionary's (gathers).
    Every offset shape of groupref.SHAPES, twice: the masks, the OR of them, and the same again."""
    d = devs(W)
    d.scan(tiles)
    g = d.g
    assert (d.d.table.num_final <= 64) == (W != 4)
    for shape in SHAPES:
        off = d.c.offsets(W, tiles, shape)
        want = d.c.want(W, tiles, shape)
        nd = off.size - 1
        d_off = upload(off)
        for _ in range(2):
            any_mask = g.document_group_masks(nd, d_doc_offsets=d_off)
            got = g.group_masks_to_host(nd)
            ne = np.flatnonzero(got != want)
            assert ne.size == 0, f"{shape}: {ne.size} of {nd} masks differ, first at document {int(ne[0])}: {int(got[ne[0]]):#x}, want {int(want[ne[0]]):#x}"
            assert any_mask == int(np.bitwise_or.reduce(want)), shape
    # the slot's own offsets (NULL)
    off = d.c.offsets(W, tiles, "mid")
    g.set_doc_offsets(off)
    g.document_group_masks(off.size - 1)
    np.testing.assert_array_equal(g.group_masks_to_host(off.size - 1), d.c.want(W, tiles, "mid"))


def test_class_table_with_a_multi_id_state():
    pats = b"[a-c]x\nax\n[^a-z0-9 ]\nq[0-9][0-9]\n[a-c]\nax[xy]\n[a-c]x\n"
    groups = [None, 0, 63, 7, None, (1, 2), 9, 20]
    rng = np.random.default_rng(78)
    alphabet = np.frombuffer(b"abcxyzq0123456789 AB-!", dtype=np.uint8)
    data = alphabet[rng.integers(0, alphabet.size, 2 * TILE + 55)]
    off = np.unique(np.concatenate([[0, data.size, TILE], rng.integers(0, data.size, 400)])).astype(np.uint64)
    parsed = cco.parse(pats)
    plen = np.array([0] + [len(p) for p in parsed], dtype=np.int64)
    pos, ids = cco.match(pats, data, parsed)
    want = masks_cut(pos, ids.astype(np.int64), plen[ids], off, masks_by_id(groups))
    t = PfacTable.from_charclass(pats, 256)
    assert any(t.out_first[s + 1] - t.out_first[s] > 1 for s in range(t.num_final))
    with GpuMatcher(0, 1) as g:
        g.load_table(t)
        g.set_pattern_groups(groups)
        got = g.tag_documents((data, off))
    np.testing.assert_array_equal(got, want)
    assert (want == 0).any() and int(np.bitwise_or.reduce(want)) == 1 | 1 << 63 | 1 << 7 | 6 | 1 << 9 | 1 << 20


def test_dense_input_carries_runs_across_chunks_and_tiles():
    """The headline pattern set on its own input, tiled: more than 64 records in a tile, documents longer than a chunk of
    64 records and longer than a tile, so the open run is carried across both."""
    pat = os.path.join(DATA, "experimentpattern")
    unit = open(os.path.join(DATA, "experimentinput"), "rb").read()
    data = tiled_bytes(66 * TILE + 123, unit)
    o = Oracle(pat, 1, 1)
    pos, ids = o.scan_spec(data)
    o.close()
    pos, ids = pos.astype(np.int64), ids.astype(np.int64)
    lens = np.array([0] + [len(x) for x in open(pat, "rb").read().split(b"\n")[:-1]], dtype=np.int64)[ids]
    assert np.bincount(pos // TILE).max() > 64
    t = PfacTable.from_file(pat, 256)
    groups = [None] + [(i - 1) % 3 + 60 if i % 4 else None for i in range(1, n_ids_of(t) + 1)]
    by_id = masks_by_id(groups)
    rng = np.random.default_rng(5)
    shapes = {"one": np.array([0, data.size]), "tiles": np.arange(0, data.size + TILE, 3 * TILE + 100).clip(0, data.size),
              "small": np.concatenate([[0], np.sort(rng.integers(1, data.size, 3000)), [data.size]])}
    with GpuMatcher(0, 1) as g:
        g.load_table(t)
        g.set_pattern_groups(groups)
        for name, off in shapes.items():
            off = np.unique(off).astype(np.uint64)
            want = masks_cut(pos, ids, lens, off, by_id)
            if name == "tiles":                                 # every document's records fill more than one chunk
                assert np.bincount(np.searchsorted(off.astype(np.int64), pos, side="right") - 1).min() > 64
            np.testing.assert_array_equal(g.tag_documents((data, off)), want, err_msg=name)
            assert want.any()


def test_after_the_whole_word_filter(devs):
    d = devs(2)
    d.scan(65)
    g, c = d.g, d.c
    no = c.n_owned(65)
    pos, ids, lens = c.scan(2, 65)
    off = c.offsets(2, 65, "mid")
    d_off = upload(off)
    keep = wordref.filter_words(c.text[:no], pos, lens, off=off.astype(np.int64))
    assert 0 < keep.sum() < keep.size
    want = masks_cut(pos[keep], ids[keep], lens[keep], off, c.by_id(2))
    assert (want != c.want(2, 65, "mid")).any()
    try:
        assert g.filter_whole_words(0, n_docs=off.size - 1, d_doc_offsets=d_off, d_input=d.text) == int(keep.sum())
        g.document_group_masks(off.size - 1, d_doc_offsets=d_off)
        np.testing.assert_array_equal(g.group_masks_to_host(off.size - 1), want)
    finally:
        d.tiles = None                                          # (the filter changed the slot's records)


def test_folded_scan_under_a_nocase_table():
    pats = b"The\nhe\nAND\nwith\nThat\n"
    groups = [None, 0, 63, 5, (1, 2), None]
    para = open(os.path.join(DATA, "paragraph402"), "rb").read()
    data = tiled_bytes(5 * TILE + 9, para).copy()
    data[::7] = np.frombuffer(bytes(data[::7]).upper(), dtype=np.uint8)
    pos, ids = folded_scan(pats, data)
    pos, ids = pos.astype(np.int64), ids.astype(np.int64)
    lens = np.array([0, 3, 2, 3, 4, 4], dtype=np.int64)[ids]
    off = np.unique(np.concatenate([[0, data.size], np.arange(97, data.size, 211)])).astype(np.uint64)
    want = masks_cut(pos, ids, lens, off, masks_by_id(groups))
    t = PfacTable.from_bytes(pats, 256, ignore_case=True)
    with GpuMatcher(0, 1) as g:
        g.load_table(t)
        assert g.case_fold
        g.set_pattern_groups(groups)
        got = g.tag_documents((data, off))
    np.testing.assert_array_equal(got, want)
    assert int(np.bitwise_or.reduce(want)) == 1 | 1 << 63 | 1 << 5 | 6


# ---------------------------------------------------------------------------
# guard bands

@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("W,tiles,shape", [(2, 65, "cut"), (4, 65, "tiny"), (8, 3, "empties"), (2, 130, "huge")])
def test_caller_buffers_at_exact_capacity(devs, W, tiles, shape, fill):
    """d_masks_out of exactly n_docs x 8 bytes: rule-breaking offsets are refused with every byte untouched, the call
    proper writes the masks and no byte more.  Then d_ids_out of exactly n_matching x 8: one entry too few gives
    PFAC_E_OVERFLOW with the exact count and an untouched buffer."""
    d = devs(W)
    d.scan(tiles)
    g = d.g
    off, want = d.c.offsets(W, tiles, shape), d.c.want(W, tiles, shape)
    nd = off.size - 1
    d_off = upload(off)
    d_bad = [upload(b) for b in bad_offsets(off, d.c.n_owned(tiles))]
    buf = {"d_masks_out": GuardedBuffer(nd * 8, fill=fill)}

    def call(cap, bad=None):
        st, got = d.d._status(lambda: g.document_group_masks(nd, d_doc_offsets=d_off if bad is None else d_bad[bad], d_out=buf["d_masks_out"].ptr))
        assert st != OK or got == int(np.bitwise_or.reduce(want))
        return st, None
    exact_call(g, call, Want(nd, {"d_masks_out": want}, bad=len(d_bad), capped=False), buf, fill, f"pfac_documents_group_masks width {W} {tiles} tiles {shape}")
    assert status_of(lambda: g.group_masks_to_host(nd)) == E_STATE          # they went to the caller's buffer
    assert status_of(lambda: g.matching_documents_where(nd, any_of=ALL)) == E_STATE
    for kw in (dict(any_of=ALL), dict(all_of=1, none_of=1 << 63), dict(any_of=6, invert=True)):
        ids = predicate(want, **kw)
        ibuf = {"d_ids_out": GuardedBuffer(ids.size * 8, fill=fill)}

        def icall(cap, bad=None):
            return d.d._status(lambda: g.matching_documents_where(nd, d_masks=buf["d_masks_out"].ptr, d_out=ibuf["d_ids_out"].ptr, out_cap=cap, **kw),
                               "n_matching")
        exact_call(g, icall, Want(ids.size, {"d_ids_out": ids}), ibuf, fill, f"pfac_documents_matching_groups {kw}")
    buf["d_masks_out"].check(what="the d_masks of a predicate")


# ---------------------------------------------------------------------------
# the contract

def test_state_errors_come_first_and_in_order():
    c = cases()
    table = c.x.table(2)
    groups = groups_for(n_ids_of(table))
    masks = table.state_group_masks(groups)
    text = c.text[:3 * TILE]
    off = np.array([0, 100, 100, 3 * TILE], dtype=np.uint64)
    d_off = upload(off)
    odd = int(d_off.data_ptr()) + 4                              # a misaligned pointer: an argument error
    with GpuMatcher(0, 1) as g:
        L, ctx = g._L, g._ctx
        assert L.pfac_table_set_state_groups(ctx, masks.ctypes.data, masks.size) == E_STATE       # before an upload
        g.load_table(table)
        assert L.pfac_table_set_state_groups(ctx, masks.ctypes.data, masks.size + 1) == E_ARG
        assert L.pfac_table_set_state_groups(ctx, None, masks.size) == E_ARG
        # state before arguments: no finished scan, with a misaligned pointer and n_docs = 2^32
        assert status_of(lambda: g.document_group_masks(1 << 32, d_doc_offsets=odd)) == E_STATE
        g.reserve(0, text.size, TILE)
        g.h2d(text)
        g.scan_resident(text.size, text.size)
        assert status_of(lambda: g.document_group_masks(3, d_doc_offsets=odd)) == E_STATE         # no final lengths
        g.set_final_lengths(table.final_lengths())
        assert status_of(lambda: g.document_group_masks(3, d_doc_offsets=odd)) == E_STATE         # no state groups
        g.set_pattern_groups(groups)
        assert status_of(lambda: g.document_group_masks(3)) == E_STATE                            # no offsets for the slot
        assert status_of(lambda: g.group_masks_to_host(3)) == E_STATE                             # no masks yet
        assert status_of(lambda: g.matching_documents_where(3, any_of=ALL)) == E_STATE
        # arguments
        assert status_of(lambda: g.document_group_masks(3, d_doc_offsets=odd)) == E_ARG
        assert status_of(lambda: g.document_group_masks(3, d_doc_offsets=d_off, d_out=odd)) == E_ARG
        assert status_of(lambda: g.document_group_masks(1 << 32, d_doc_offsets=d_off)) == E_ARG
        assert status_of(lambda: g.document_group_masks(3, d_doc_offsets=d_off, d_records=int(d_off.data_ptr()))) == E_ARG
        assert status_of(lambda: g.document_group_masks(0, d_doc_offsets=d_off)) == E_ARG         # no documents, but bytes
        g.set_doc_offsets(off)
        assert status_of(lambda: g.document_group_masks(2)) == E_STATE                            # not the slot's n_docs
        any_mask = g.document_group_masks(3)
        pos, ids = c.x.tinfo(2)["matcher"].scan_spec(np.ascontiguousarray(text), None)
        pos, ids = pos.astype(np.int64), ids.astype(np.int64)
        lens = c.x.tinfo(2)["ll"][ids]
        want = masks_cut(pos, ids, lens, off, masks_by_id(groups))
        assert any_mask == int(np.bitwise_or.reduce(want)) and want[1] == 0
        # the window fetches
        np.testing.assert_array_equal(g.group_masks_to_host(3), want)
        np.testing.assert_array_equal(g.group_masks_to_host(3, first=1, n=2), want[1:])
        assert g.group_masks_to_host(3, first=3, n=0).size == 0
        assert status_of(lambda: g.group_masks_to_host(3, first=2, n=2)) == E_ARG
        assert status_of(lambda: g.group_masks_to_host(3, first=4, n=0)) == E_ARG
        # the predicate's arguments
        assert status_of(lambda: g.matching_documents_where(2, any_of=ALL)) == E_ARG              # NULL masks, another n_docs
        n = C.c_uint64(0)
        assert L.pfac_documents_matching_groups(ctx, 0, None, 3, 0, ALL, 0, 2, None, 0, C.byref(n)) == E_ARG     # flags
        assert L.pfac_documents_matching_groups(ctx, 0, odd, 3, 0, ALL, 0, 0, None, 0, C.byref(n)) == E_ARG
        assert L.pfac_documents_matching_groups(ctx, 0, int(d_off.data_ptr()), 1 << 32, 0, ALL, 0, 0, None, 0, C.byref(n)) == E_ARG
        # a failed pass discards the slot's masks
        assert g.matching_documents_where(3, any_of=ALL) == predicate(want, any_of=ALL).size
        assert status_of(lambda: g.document_group_masks(3, d_doc_offsets=odd)) == E_ARG
        assert status_of(lambda: g.group_masks_to_host(3)) == E_STATE
        # a second call replaces the groups; the masks survive a later scan; an upload clears the groups
        g.set_pattern_groups([None] + [9] * (len(groups) - 1))
        assert g.document_group_masks(3) == 1 << 9
        first = cut_by_hand(pos, ids, lens, off)[0]
        np.testing.assert_array_equal(g.group_masks_to_host(3), np.where(first[1:] > first[:-1], np.uint64(1 << 9), np.uint64(0)))
        g.set_pattern_groups(groups)
        g.document_group_masks(3)
        g.scan_resident(TILE, TILE)
        np.testing.assert_array_equal(g.group_masks_to_host(3), want)                             # through a later scan ...
        g.load_table(table)
        np.testing.assert_array_equal(g.group_masks_to_host(3), want)                             # ... and an upload
        g.set_final_lengths(table.final_lengths())
        assert status_of(lambda: g.document_group_masks(3)) == E_STATE                            # a scan of the earlier table
        g.scan_resident(text.size, text.size)
        assert status_of(lambda: g.document_group_masks(3)) == E_STATE                            # the upload cleared the groups
        g.set_pattern_groups(groups)
        assert g.document_group_masks(3) == any_mask
        # overflow is judged behind the state, in front of the arguments
        heap = torch.zeros(64 * 8, dtype=torch.uint8, device="cuda:0")
        g.scan_async(text.size, d_records=heap, capacity=64)
        assert g.scan_finish(allow_overflow=True)[1]
        assert status_of(lambda: g.document_group_masks(3, d_doc_offsets=odd, d_records=heap)) == E_OVERFLOW
        # no documents and no bytes
        g.scan_resident(0, 0)
        g.set_doc_offsets(np.zeros(1, dtype=np.uint64))
        assert g.document_group_masks(0) == 0
        assert g.group_masks_to_host(0).size == 0
        assert g.matching_documents_where(0, any_of=ALL) == 0


def test_predicate_feeds_the_gather(devs):
    """The ids of the predicate are the slot's matching ids: pfac_documents_matching_d2h fetches them and
    pfac_documents_gather(d_ids = NULL) consumes them; the bytes equal gatherref's."""
    d = devs(2)
    d.scan(65)
    g, c = d.g, d.c
    no = c.n_owned(65)
    off, want = c.offsets(2, 65, "tiny"), c.want(2, 65, "tiny")
    nd = off.size - 1
    g.set_doc_offsets(off)
    g.document_group_masks(nd)
    pos, ids_, lens = c.scan(2, 65)
    first = cut_by_hand(pos, ids_, lens, off)[0]
    for kw in (dict(any_of=ALL), dict(all_of=1 | 1 << 63), dict(all_of=1, none_of=6), dict(none_of=ALL),
               dict(all_of=1, any_of=6, none_of=1 << 7, invert=True), dict(any_of=1 << 40)):
        ids = predicate(want, **kw)
        assert g.matching_documents_where(nd, **kw) == ids.size, kw
        np.testing.assert_array_equal(g.matching_documents_to_host(ids.size), ids)
        out_bytes = g.gather_documents(nd, ids.size, no, d_input=d.text)
        ref_out, ref_off = gather_ref(c.text[:no], off, ids)
        assert out_bytes == ref_out.size
        np.testing.assert_array_equal(g.gathered_to_host(out_bytes), ref_out)
        np.testing.assert_array_equal(g.gathered_offsets_to_host(ids.size), ref_off)
    assert 0 < predicate(want, all_of=1 | 1 << 63).size < predicate(want, any_of=ALL).size < nd
    # every pattern in one group: the answer of pfac_documents_matching over the segment pass
    g.set_pattern_groups([None] + [33] * n_ids_of(d.d.table))
    try:
        assert g.document_group_masks(nd) == 1 << 33
        for inv in (False, True):
            want_ids = matching_ids(first, inv)
            assert g.matching_documents_where(nd, any_of=ALL, invert=inv) == want_ids.size
            np.testing.assert_array_equal(g.matching_documents_to_host(want_ids.size), want_ids)
    finally:
        g.set_pattern_groups(groups_for(n_ids_of(d.d.table)))


# ---------------------------------------------------------------------------
# end to end

def test_tagging_and_grepping_a_small_log():
    lines = [b"GET /index.html 200 alice", b"POST /login 403 bob", b"", b"GET /admin 500 root error", b"error: disk full",
             b"alice and bob", b"nothing here", b"error error alice root"]
    pats = b"alice\nbob\nerror\nroot\nGET\n403\n"
    groups = [None, 0, 0, 63, 5, None, (5, 6)]                  # users, errors, privileged, (ungrouped), two groups
    by_id = masks_by_id(groups)
    data = np.frombuffer(b"\n".join(lines) + b"\n" + b"bob error", dtype=np.uint8)
    off = split_offsets(data, 0x0A)[0]
    want = np.zeros(off.size - 1, dtype=np.uint64)
    for k in range(off.size - 1):
        doc = bytes(data[int(off[k]):int(off[k + 1])])
        for i, p in enumerate(pats.split(b"\n")[:-1], 1):
            if p in doc:
                want[k] |= by_id[i]
    t = PfacTable.from_bytes(pats, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(t)
        g.set_pattern_groups(groups)
        np.testing.assert_array_equal(g.tag_documents([bytes(data[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])]), want)
        got_off, got = g.tag_lines(data)
        np.testing.assert_array_equal(got_off, off)
        np.testing.assert_array_equal(got, want)
        for kw in (dict(all_of=1 | 1 << 63), dict(any_of=1 << 5, none_of=1), dict(any_of=ALL, invert=True), dict(all_of=1 << 6)):
            ids = predicate(want, **kw)
            out, out_off, got_ids = g.grep_lines_where(data, **kw)
            ref_out, ref_off = gather_ref(data, off, ids)
            np.testing.assert_array_equal(got_ids, ids)
            np.testing.assert_array_equal(out, ref_out)
            np.testing.assert_array_equal(out_off, ref_off)
        # every pattern grouped: any_of = all groups is grep_lines
        g.set_pattern_groups([None, 0, 1, 2, 3, 4, 63])
        a = g.grep_lines_where(data, any_of=ALL)
        b = g.grep_lines(data)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        assert a[2].size == 7
