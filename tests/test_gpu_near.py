"""Proximity rules on the GPU (run with -m gpu on an MI355X): pfac_documents_near, pfac_near_masks_d2h and
pfac_slot_near_masks against tests/nearref.py, whose cases tests/test_near_ref.py holds against a second reference and
checks for their preconditions without a GPU.  Most cases are host-made cut arrays fed through d_sel and d_doc_first: no
scan, small shapes.  Every such case runs through passguard.exact_call with a guard band of exactly n_docs x 8 bytes.
Integer work: bit-exact.  No expectation comes from the device."""
import ctypes as C

import numpy as np
import pytest

import gatherref
import groupref
import nearref
import passguard
from heapguard import FILLS, GuardedBuffer
from nearref import ALL, ANY_DIST, BLOCK, GA, GB, GMASK, case, check, near_masks, rule, rules_array
from passguard import E_ARG, E_STATE, OK, Want, exact_call
from phfpfac_amd import GpuMatcher, PfacError, PfacTable, near_rule
from phfpfac_amd.matcher import _ptr

pytestmark = pytest.mark.gpu

_DEV = []
SCAN_RULES = rules_array([rule(GA, GB, 5), rule(GA, GB, 5, True), rule(GB, GA, 2, True), rule(1 << 2, 1 << 3, 12), rule(1 << 63, 1 << 63, 40),
                          rule(GA | GB, 1 << 5, ANY_DIST, True), rule(1 << 7, 1 << 7, 0)])


def set_groups(g):
    assert g._L.pfac_table_set_state_groups(g._ctx, GMASK.ctypes.data, GMASK.size) == OK


def fresh_device():
    dev = passguard.Device(2)
    assert dev.table.num_final == nearref.NUM_FINAL
    set_groups(dev.g)
    return dev


def device():
    if not _DEV:
        _DEV.append(fresh_device())
    return _DEV[0]


@pytest.fixture(scope="module", autouse=True)
def _close_devices():
    yield
    for d in _DEV:
        d.close()
    _DEV.clear()


def raw_call(g, d_sel, d_first, n_docs, rules, flags=0, out=None, n_rules=None, slot=0):
    """The C-ABI as it is: (status, *any_mask).  `rules`: a nearref.RULE array, or None for a NULL pointer."""
    any_ = C.c_uint64(12345)
    n = (0 if rules is None else rules.size) if n_rules is None else n_rules
    p = rules.ctypes.data if rules is not None and rules.size else None
    rc = g._L.pfac_documents_near(g._ctx, slot, _ptr(d_sel), _ptr(d_first), int(n_docs), int(flags), p, int(n), _ptr(out), C.byref(any_))
    return rc, any_.value


def any_of(want):
    return int(np.bitwise_or.reduce(want)) if want.size else 0


def exact(dev, c, fill, broken=()):
    """One case into a caller's buffer of exactly n_docs x 8 bytes; `broken`: (d_sel, d_first) pairs that break a rule of
    the input, each refused with PFAC_E_ARG and the buffer untouched before the call that breaks none."""
    g = dev.g
    d_sel, d_first = dev.upload(c.sel()), dev.upload(c.first)
    buf = {"d_masks_out": GuardedBuffer(c.n_docs * 8, fill=fill)}

    def call(cap, bad=None):
        s, f = (d_sel, d_first) if bad is None else broken[bad]
        rc, any_ = raw_call(g, s, f, c.n_docs, c.rules, out=buf["d_masks_out"].ptr)
        assert any_ == (any_of(c.want()) if rc == OK else 0), f"*any_mask 0x{any_:x}"
        return rc, None
    exact_call(g, call, Want(c.n_docs, {"d_masks_out": c.want()}, bad=len(broken), capped=False), buf, fill,
               f"pfac_documents_near case {c.name} ({c.n} records, {c.n_docs} documents, {c.rules.size} rules)")
    return d_sel, d_first


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name", ALL)
def test_case_at_exact_capacity(name, fill):
    exact(device(), case(name), fill)


def test_rule_breaking_inputs_are_refused_untouched():
    dev = device()
    # one document across a block edge: a position that decreases inside a chunk, at a chunk's first lane, at a block's
    # first record; a state at and past num_final at the first, a middle and the last record
    c = case("records4095-4096")
    bad = []
    for at in (10, nearref.CHUNK, BLOCK, c.n - 1):
        sel = c.sel()
        assert at > 0 and c.doc_of(at) == c.doc_of(at - 1) and sel["pos"][at - 1] > 0
        sel["pos"][at] = sel["pos"][at - 1] - 1
        bad.append((dev.upload(sel), dev.upload(c.first)))
    for at, st in ((0, nearref.NUM_FINAL), (c.n // 2, nearref.NUM_FINAL), (c.n - 1, 2 ** 32 - 1)):
        sel = c.sel()
        sel["state"][at] = st
        bad.append((dev.upload(sel), dev.upload(c.first)))
    exact(dev, c, FILLS[0], bad)
    # many documents: doc_first that does not start at 0, that decreases in the middle, in front and at the end
    c = case("positions-stream")
    f = c.first
    k = int(np.flatnonzero(np.diff(f.astype(np.int64)) > 1)[3])
    firsts = []
    for i, v in ((0, 1), (k, f[k + 1] + np.uint64(1)), (0, f[1] + np.uint64(1)), (-1, f[-2] - np.uint64(1))):
        b = f.copy()
        b[i] = v
        firsts.append(b)
    assert c.first[-2] > 0
    d_sel = dev.upload(c.sel(), slack=64)
    exact(dev, c, FILLS[1], [(d_sel, dev.upload(b)) for b in firsts])
    # positions that fall at a document's first record are no decrease
    assert (np.diff(case("positions-document").pos) < 0).any()


def test_error_ladder():
    dev, c = device(), case("positions-stream")
    g = dev.g
    d_sel, d_first = dev.upload(c.sel(), slack=16), dev.upload(c.first, slack=16)
    buf = GuardedBuffer(c.n_docs * 8, fill=FILLS[1])

    def refused(status, gm, *a, **kw):
        rc, any_ = raw_call(gm, *a, **{"out": buf.ptr, **kw})
        assert rc == status, f"{passguard.STATUS.get(rc, rc)}, want {passguard.STATUS[status]}: {kw}"
        assert any_ == 0
        gm.sync(0)
        buf.check(payload_untouched=True, what="d_masks_out")

    bad_flags, bad_reserved = c.rules.copy(), c.rules.copy()
    bad_flags["flags"][-1] = 2
    bad_reserved["reserved"][0] = 1
    with GpuMatcher(0, 1) as bare:                               # no table
        refused(E_STATE, bare, d_sel, d_first, c.n_docs, c.rules)
        refused(E_STATE, bare, d_sel, d_first, c.n_docs, c.rules, flags=2)    # ... comes before the flags
        bare.load_table(dev.table)                               # no state groups for it
        refused(E_STATE, bare, d_sel, d_first, c.n_docs, c.rules)
        refused(E_STATE, bare, d_sel, d_first.data_ptr() + 4, c.n_docs, bad_flags)       # ... comes before every PFAC_E_ARG
        set_groups(bare)                                         # nothing held
        refused(E_STATE, bare, None, None, c.n_docs, c.rules)
        refused(E_STATE, bare, None, None, c.n_docs, c.rules, flags=1)
        refused(E_STATE, bare, None, None, c.n_docs, c.rules, n_rules=65)
        bare.load_table(dev.table)                               # an upload drops the groups
        refused(E_STATE, bare, d_sel, d_first, c.n_docs, c.rules)
    refused(E_ARG, g, d_sel.data_ptr() + 4, d_first, c.n_docs, c.rules)      # misalignment
    refused(E_ARG, g, d_sel, d_first.data_ptr() + 4, c.n_docs, c.rules)
    refused(E_ARG, g, d_sel, d_first, c.n_docs, c.rules, out=buf.ptr + 4)
    refused(E_ARG, g, d_sel, None, c.n_docs, c.rules)            # one NULL
    refused(E_ARG, g, None, d_first, c.n_docs, c.rules)
    refused(E_ARG, g, d_sel, d_first, 2 ** 32, c.rules)
    refused(E_ARG, g, d_sel, d_first, c.n_docs, c.rules, flags=2)
    refused(E_ARG, g, d_sel, d_first, c.n_docs, c.rules, n_rules=65)
    refused(E_ARG, g, d_sel, d_first, c.n_docs, None, n_rules=1)
    refused(E_ARG, g, d_sel, d_first, c.n_docs, bad_flags)
    refused(E_ARG, g, d_sel, d_first, c.n_docs, bad_reserved)
    big = c.first.copy()
    big[1:] = 2 ** 32
    refused(E_ARG, g, d_sel, dev.upload(big), c.n_docs, c.rules)             # 2^32 records
    refused(E_ARG, g, d_sel, dev.upload(np.array([3], dtype=np.uint64)), 0, c.rules)    # records without a document
    # and the call that breaks no rule; n_rules = 0 takes a NULL
    rc, any_ = raw_call(g, d_sel, d_first, c.n_docs, c.rules, out=buf.ptr)
    g.sync(0)
    assert (rc, any_) == (OK, any_of(c.want()))
    buf.check(what="d_masks_out")
    check(c.want(), buf.host().view(np.uint64))
    rc, any_ = raw_call(g, d_sel, d_first, c.n_docs, None, out=buf.ptr)
    g.sync(0)
    assert (rc, any_) == (OK, 0) and not buf.host().any()


# ---------------------------------------------------------------------------
# real inputs: the slot's segment result and its per-document selection of a scan over the committed patterns

def scanned(dev, shape="tiny"):
    x = dev.x
    key = x.doc_key(shape)
    dev.scan(key)
    off = x.offsets(2, key, shape)
    return key, off, int(off.size - 1), dev.upload(off)


@pytest.mark.parametrize("shape", ["tiny", "emptygroup"])
def test_slot_owned_segment_and_selection(shape):
    dev = device()
    g = dev.g
    key, off, nd, d_off = scanned(dev, shape)
    kept = g.segment_records(nd, d_doc_offsets=d_off)
    first, rec = g.segment_to_host(kept, nd)
    assert kept > 1000 and kept > BLOCK
    want = near_masks(rec["state"], rec["pos"], first, SCAN_RULES)
    assert 0 < np.count_nonzero(want) < nd
    any_ = g.document_near_masks(nd, SCAN_RULES)
    assert any_ == any_of(want)
    got = g.near_masks_to_host(nd)
    check(want, got, what=f"segment, {shape}")
    assert g.near_masks_to_host(nd).tobytes() == got.tobytes()              # fetched twice: the same bytes
    check(want[3:10], g.near_masks_to_host(nd, first=3, n=7))
    assert raw_call(g, None, None, nd + 1, SCAN_RULES)[0] == E_ARG           # an n_docs that is not the segment's
    with pytest.raises(PfacError) as e:                                      # ... and the failed call discarded the result
        g.near_masks_to_host(nd)
    assert e.value.status == E_STATE
    assert g.document_near_masks(nd, SCAN_RULES) == any_
    # the leftmost-longest picks of every document: positions relative to the scan
    n_sel = g.select_leftmost_longest_documents(nd, d_doc_offsets=d_off)
    sfirst, srec = g.doc_selection_to_host(n_sel, nd)
    assert 500 < n_sel < kept
    swant = near_masks(srec["state"], srec["pos"], sfirst, SCAN_RULES)
    assert g.document_near_masks(nd, SCAN_RULES, selection=True) == any_of(swant)
    check(swant, g.near_masks_to_host(nd), what=f"selection, {shape}")
    assert not np.array_equal(swant, want)
    # the caller's copies of both give the same, and the segment result is still the slot's
    buf = GuardedBuffer(nd * 8, fill=FILLS[0])
    assert g.document_near_masks(nd, SCAN_RULES, d_sel=dev.upload(srec), d_doc_first=dev.upload(sfirst), d_out=buf.ptr) == any_of(swant)
    g.sync(0)
    buf.check(what="d_masks_out")
    check(swant, buf.host().view(np.uint64))
    assert g.near_masks_ptr() == 0                               # the masks went to the caller's buffer
    assert g.document_near_masks(nd, SCAN_RULES) == any_ and g.near_masks_ptr() != 0


def test_a_stale_selection_is_refused():
    dev = fresh_device()
    try:
        g, x = dev.g, dev.x
        key, off, nd, d_off = scanned(dev)
        g.select_leftmost_longest_documents(nd, d_doc_offsets=d_off)
        g.document_near_masks(nd, SCAN_RULES, selection=True)
        g.scan_resident(key[1], key[2], d_input=dev.d_input(key[0]))         # a later scan: the picks are stale
        assert raw_call(g, None, None, nd, SCAN_RULES, flags=1) == (E_STATE, 0)
        g.select_leftmost_longest_documents(nd, d_doc_offsets=d_off)
        g.load_table(dev.table)                                  # ... and a later table: its states mean something else
        set_groups(g)
        assert raw_call(g, None, None, nd, SCAN_RULES, flags=1) == (E_STATE, 0)
        assert raw_call(g, None, None, nd, SCAN_RULES, flags=0) == (E_STATE, 0)          # no segment result at all
    finally:
        dev.close()


def test_lifetime():
    dev = fresh_device()
    try:
        g, x = dev.g, dev.x
        a, b = case("positions-stream"), case("rules-64")
        ups = {c.name: (dev.upload(c.sel()), dev.upload(c.first)) for c in (a, b)}

        def run(c):
            assert g.document_near_masks(c.n_docs, c.rules, d_sel=ups[c.name][0], d_doc_first=ups[c.name][1]) == any_of(c.want())

        def fetch_status(c):
            m = np.empty(max(c.n_docs, 1), dtype=np.uint64)
            rc = g._L.pfac_near_masks_d2h(g._ctx, 0, m.ctypes.data, 0, c.n_docs)
            g.sync(0)
            return rc
        with pytest.raises(PfacError) as e:                      # nothing to fetch yet
            g.near_masks_to_host(1)
        assert e.value.status == E_STATE and g.near_masks_ptr() == 0
        run(a)
        # a scan, a table upload, a group-mask pass and a term-count pass in between do not discard it
        key, off, nd, d_off = scanned(dev)
        g.load_table(dev.table)
        g.set_final_lengths(dev.table.final_lengths())
        dev.cur = None
        dev.scan(key)
        set_groups(g)
        g.document_group_masks(nd, d_doc_offsets=d_off)
        g.segment_records(nd, d_doc_offsets=d_off)
        g.document_term_counts(nd)
        check(a.want(), g.near_masks_to_host(a.n_docs), what="behind a scan, an upload, a group-mask and a term-count pass")
        with pytest.raises(PfacError) as e:
            g.near_masks_to_host(a.n_docs, first=1, n=a.n_docs)  # a window past the result
        assert e.value.status == E_ARG
        # ... nor does this pass discard theirs
        masks = g.group_masks_to_host(nd)
        run(b)
        assert g.group_masks_to_host(nd).tobytes() == masks.tobytes()
        check(b.want(), g.near_masks_to_host(b.n_docs), what="the second call")
        # a failed call discards it
        assert raw_call(g, *ups[b.name], b.n_docs, b.rules, flags=2)[0] == E_ARG
        assert fetch_status(b) == E_STATE and g.near_masks_ptr() == 0
        run(b)
        assert fetch_status(b) == OK
    finally:
        dev.close()


def test_near_masks_feed_the_predicate_and_the_gather():
    dev = device()
    g = dev.g
    key, off, nd, d_off = scanned(dev)
    kept = g.segment_records(nd, d_doc_offsets=d_off)
    first, rec = g.segment_to_host(kept, nd)
    want = near_masks(rec["state"], rec["pos"], first, SCAN_RULES)
    g.document_near_masks(nd, SCAN_RULES)
    ptr = g.near_masks_ptr()
    assert ptr and ptr % 8 == 0
    buf = dev.x.input(key[0])[:key[1]]
    for kw in (dict(any_of=2 ** 64 - 1), dict(all_of=0b11), dict(any_of=0b100000, none_of=0b10), dict(all_of=1, invert=True)):
        ids = groupref.predicate(want, **kw)
        assert 0 < ids.size < nd, kw
        n = g.matching_documents_where(nd, d_masks=ptr, **kw)
        assert n == ids.size
        np.testing.assert_array_equal(g.matching_documents_to_host(n), ids)
        out_bytes = g.gather_documents(nd, n, key[1], d_input=dev.d_input(key[0]), d_doc_offsets=d_off)
        w_out, w_off = gatherref.gather_ref(buf, off, ids)
        assert out_bytes == w_out.size
        np.testing.assert_array_equal(g.gathered_to_host(out_bytes), w_out)
        np.testing.assert_array_equal(g.gathered_offsets_to_host(n), w_off.astype(np.uint64))


# ---------------------------------------------------------------------------
# the conveniences, on a log whose expected lines are written out by hand

PATTERNS = b"card\nexpires\nBEGIN\nEND\n"                        # ids 1, 2, 3, 4 = groups 0, 1, 2, 3
LOG = (b"card 4111 expires 09/27\n"                              # 0: "card" at 0, "expires" at 10
       b"expires soon, your card is 4111\n"                      # 1: "expires" at 0, "card" at 19
       b"card one ............................................................ expires\n"    # 2: 70 bytes apart
       b"BEGIN x END\n"                                          # 3
       b"END then BEGIN\n"                                       # 4
       b"card\n"                                                 # 5
       b"\n"                                                     # 6
       b"card card\n")                                           # 7: "card" twice, 5 bytes apart
LINES = LOG.split(b"\n")[:-1]


def lines_of(out, out_off):
    o = out_off.astype(np.int64)
    return [bytes(out[a:b]).rstrip(b"\n") for a, b in zip(o[:-1], o[1:])]


def test_conveniences_on_a_small_log():
    table = PfacTable.from_bytes(PATTERNS, 256)
    rules = [near_rule(0, 1, 60), near_rule(0, 1, 60, ordered=True), near_rule(2, 3, None, ordered=True), near_rule(0, 0, 5)]
    masks = [0b0011, 0b0001, 0, 0b0100, 0, 0, 0, 0b1000]
    assert LOG[LOG.index(b"card one"):].index(b"expires") == 70
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_pattern_groups([None, 0, 1, 2, 3])
        offsets, got = g.near_lines(LOG, rules)
        assert got.dtype == np.uint64 and got.tolist() == masks
        assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(x) + 1 for x in LINES])]).tolist()
        assert g.near_lines(LOG.replace(b"\n", b";"), rules, delimiter=b";")[1].tolist() == masks
        assert g.near_lines(LOG, rules, non_overlapping=True)[1].tolist() == masks
        docs = [LINES[3], b"", LINES[0], LINES[7], LINES[4]]
        assert g.near_documents(docs, rules).tolist() == [0b0100, 0, 0b0011, 0b1000, 0]
        assert g.near_documents(docs, np.stack(rules)).tolist() == [0b0100, 0, 0b0011, 0b1000, 0]
        assert g.near_documents(docs, rules, non_overlapping=True).tolist() == [0b0100, 0, 0b0011, 0b1000, 0]
        assert g.near_documents(docs, []).tolist() == [0] * 5
        # the lines on which some rule fired; an ordered pair alone; one rule and not another
        out, out_off, ids = g.grep_lines_near(LOG, rules)
        assert ids.tolist() == [0, 1, 3, 7] and lines_of(out, out_off) == [LINES[i] for i in (0, 1, 3, 7)]
        out, out_off, ids = g.grep_lines_near(LOG, rules, all_of=0b10)
        assert ids.tolist() == [0] and lines_of(out, out_off) == [LINES[0]]
        out, out_off, ids = g.grep_lines_near(LOG, rules, any_of=0b1, none_of=0b10)
        assert ids.tolist() == [1] and lines_of(out, out_off) == [LINES[1]]
        out, out_off, ids = g.grep_lines_near(LOG, rules, invert=True)
        assert ids.tolist() == [2, 4, 5, 6]
        out, out_off, ids = g.grep_lines_near(LOG, rules, non_overlapping=True, whole_words=True)
        assert ids.tolist() == [0, 1, 3, 7]
    # "he" inside "she": every match against the leftmost-longest picks
    table = PfacTable.from_bytes(b"he\nshe\n", 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_pattern_groups([None, 0, 1])
        r = [near_rule(1, 0, 1, ordered=True)]                   # a "she", then a "he" one byte behind its start
        assert g.near_documents([b"she", b"he she", b"she he"], r).tolist() == [1, 1, 1]
        assert g.near_documents([b"she", b"he she", b"she he"], r, non_overlapping=True).tolist() == [0, 0, 0]
        assert g.near_documents([b"she", b"he she", b"she he"], [near_rule(1, 0, 4, ordered=True)], non_overlapping=True).tolist() == [0, 0, 1]
