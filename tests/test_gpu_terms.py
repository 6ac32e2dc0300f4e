"""Term counts per document on the GPU (run with -m gpu on an MI355X): pfac_documents_term_counts and
pfac_documents_term_counts_d2h against tests/termref.py, whose cases tests/test_terms_ref.py holds against a second
reference and checks for their preconditions without a GPU.  Most cases are host-made cut arrays fed through d_sel and
d_doc_first: no scan, small shapes.  Every such case runs through passguard.exact_call with guard bands of exactly
(n_docs + 1) x 8, n_terms x 4 and n_terms x 4 bytes.  Integer work: bit-exact.  No expectation comes from the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import passguard
import termref
from heapguard import FILLS, GuardedBuffer
from passguard import E_ARG, E_OVERFLOW, E_STATE, OK, Want, exact_call
from phfpfac_amd import GpuMatcher, PfacError, PfacTable
from phfpfac_amd.matcher import _ptr
from termref import cases, check, names, term_counts

pytestmark = pytest.mark.gpu

ALL = [(W, name) for W in (2, 4) for name in names(W)]
_DEV = {}


def device(W):
    if W not in _DEV:
        _DEV[W] = passguard.Device(W)
    return _DEV[W]


@pytest.fixture(scope="module", autouse=True)
def _close_devices():
    yield
    for d in _DEV.values():
        d.close()
    _DEV.clear()


def raw_call(g, d_sel, d_first, n_docs, flags=0, row=None, st=None, cnt=None, cap=0, slot=0):
    """The C-ABI as it is: (status, *n_terms)."""
    n = C.c_uint64(12345)
    rc = g._L.pfac_documents_term_counts(g._ctx, slot, _ptr(d_sel), _ptr(d_first), int(n_docs), int(flags), _ptr(row), _ptr(st),
                                         _ptr(cnt), int(cap), C.byref(n))
    return rc, n.value


def guarded(n_docs, n_terms, fill):
    return {"d_row_ptr_out": GuardedBuffer((n_docs + 1) * 8, fill=fill), "d_states_out": GuardedBuffer(n_terms * 4, fill=fill),
            "d_counts_out": GuardedBuffer(n_terms * 4, fill=fill)}


def exact(dev, c, fill):
    """One case into caller's buffers of exactly the result's bytes: one entry too few, then the exact capacity."""
    g = dev.g
    want = c.want()
    d_sel, d_first = dev.upload(c.sel()), dev.upload(c.first)
    buf = guarded(c.n_docs, want[1].size, fill)

    def call(cap, bad=None):
        return dev._status(lambda: g.document_term_counts(c.n_docs, d_sel=d_sel, d_doc_first=d_first, d_row_ptr=buf["d_row_ptr_out"].ptr,
                                                          d_states=buf["d_states_out"].ptr, d_counts=buf["d_counts_out"].ptr,
                                                          out_cap=cap), "n_terms")
    w = Want(want[1].size, {"d_row_ptr_out": want[0], "d_states_out": want[1], "d_counts_out": want[2]})
    exact_call(g, call, w, buf, fill, f"pfac_documents_term_counts case {c.name} ({c.n} records, {c.n_docs} documents, {c.passes} passes)")
    return d_sel, d_first


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("W,name", ALL, ids=[f"{W}-{n}" for W, n in ALL])
def test_case_at_exact_capacity(W, name, fill):
    dev = device(W)
    assert dev.table.num_final == termref.num_final(W)
    exact(dev, cases(W)[name], fill)


def test_several_chunks_per_workgroup(monkeypatch):
    """The sort's workgroups limited to three (the PFAC_TERMS_ROWS knob, read when the table is installed): every workgroup
    of the histogram and scatter kernels loops over several chunks of 1024 keys, the last one over fewer."""
    monkeypatch.setenv("PFAC_TERMS_ROWS", str(termref.CHUNKED_ROWS))
    dev = passguard.Device(2)
    try:
        for name in termref.CHUNKED:
            exact(dev, cases(2)[name], FILLS[0])
    finally:
        dev.close()


@pytest.mark.parametrize("W,name", [(2, "n16454"), (2, "run3000"), (4, "passes-d524289"), (2, "passes-one-d17")])
def test_slot_owned_result_twice_gives_the_same_bytes(W, name):
    dev, c = device(W), cases(W)[name]
    g = dev.g
    d_sel, d_first = dev.upload(c.sel()), dev.upload(c.first)
    got = []
    for _ in range(2):
        n = g.document_term_counts(c.n_docs, d_sel=d_sel, d_doc_first=d_first)
        assert n == c.want()[1].size
        got.append(g.term_counts_to_host(c.n_docs, n))
        check(c.want(), *got[-1], what=c.name)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*got))
    # each output alone may be the caller's: the other two stay the slot's
    buf = guarded(c.n_docs, c.want()[1].size, FILLS[0])
    n = g.document_term_counts(c.n_docs, d_sel=d_sel, d_doc_first=d_first, d_states=buf["d_states_out"].ptr, out_cap=c.want()[1].size)
    row = np.empty(c.n_docs + 1, dtype=np.uint64)
    cnt = np.empty(n, dtype=np.uint32)
    assert g._L.pfac_documents_term_counts_d2h(g._ctx, 0, row.ctypes.data, None, cnt.ctypes.data) == OK
    g.sync(0)
    buf["d_states_out"].check(what="d_states_out")
    check(c.want(), row, buf["d_states_out"].host().view(np.uint32), cnt, what=c.name)
    st = np.empty(max(n, 1), dtype=np.uint32)
    assert g._L.pfac_documents_term_counts_d2h(g._ctx, 0, None, st.ctypes.data, None) == E_STATE     # it went to the caller's buffer
    buf["d_row_ptr_out"].check(payload_untouched=True, what="a d_row_ptr_out the call did not get")
    buf["d_counts_out"].check(payload_untouched=True, what="a d_counts_out the call did not get")


# ---------------------------------------------------------------------------
# real inputs: the slot's segment result and its per-document selection, against the CPU oracle's records

def by_ids(dev, row, st, cnt):
    """The device's triple with pattern ids for states, every row ordered by id (the states strictly ascend as they come)."""
    r = row.astype(np.int64)
    rows = np.repeat(np.arange(r.size - 1), np.diff(r))
    if st.size:
        inner = rows[1:] == rows[:-1]
        assert (np.diff(st.astype(np.int64))[inner] > 0).all(), "the states do not strictly ascend inside a document"
        assert int(st.max()) < dev.idmap.size
    ids = dev.idmap[st.astype(np.int64)]
    order = np.lexsort((ids, rows))
    return row, ids[order].astype(np.uint32), cnt[order]


@pytest.mark.parametrize("W", passguard.WIDTHS)
@pytest.mark.parametrize("shape", ["tiny", "emptygroup"])
def test_slot_owned_segment_and_selection(W, shape):
    dev = device(W)
    g, x = dev.g, dev.x
    key = x.doc_key(shape)
    dev.scan(key)
    off = x.offsets(W, key, shape)
    nd, d_off = int(off.size - 1), dev.upload(off)
    n_ids = int(x.tinfo(W)["ll"].size)
    # every match
    first, pos, ids = x.seg(W, key, shape)
    assert g.segment_records(nd, d_doc_offsets=d_off) == pos.size > 1000
    want = term_counts(ids, first, n_ids)
    n = g.document_term_counts(nd)
    assert n == want[1].size
    check(want, *by_ids(dev, *g.term_counts_to_host(nd, n)), what=f"segment, width {W}, {shape}")
    assert raw_call(g, None, None, nd + 1)[0] == E_ARG           # an n_docs that is not the segment's
    # the leftmost-longest picks of every document
    sfirst, spos, sids, _, _ = x.docsel(W, key, shape)
    assert g.select_leftmost_longest_documents(nd, d_doc_offsets=d_off) == spos.size > 500
    swant = term_counts(sids, sfirst, n_ids)
    n = g.document_term_counts(nd, selection=True)
    assert n == swant[1].size < want[1].size
    check(swant, *by_ids(dev, *g.term_counts_to_host(nd, n)), what=f"selection, width {W}, {shape}")
    # the segment result is still the slot's
    assert g.document_term_counts(nd) == want[1].size


# ---------------------------------------------------------------------------
# errors

def test_error_ladder():
    dev, c = device(2), cases(2)["n1025"]
    g = dev.g
    d_sel, d_first = dev.upload(c.sel(), slack=16), dev.upload(c.first, slack=16)
    nt = c.want()[1].size
    buf = guarded(c.n_docs, nt, FILLS[1])
    out = dict(row=buf["d_row_ptr_out"].ptr, st=buf["d_states_out"].ptr, cnt=buf["d_counts_out"].ptr, cap=nt)

    def refused(status, *a, **kw):
        rc, n = raw_call(*a, **{**out, **kw})
        assert rc == status, f"{passguard.STATUS.get(rc, rc)}, want {passguard.STATUS[status]}: {kw}"
        assert n == 0
        a[0].sync(0)
        for name, b in buf.items():
            b.check(payload_untouched=True, what=name)

    with GpuMatcher(0, 1) as bare:                               # no table
        refused(E_STATE, bare, d_sel, d_first, c.n_docs)
        refused(E_STATE, bare, d_sel, d_first, c.n_docs, flags=2)            # ... comes before the flags
        bare.load_table(dev.table)                               # nothing held
        refused(E_STATE, bare, None, None, c.n_docs)
        refused(E_STATE, bare, None, None, c.n_docs, flags=1)
    refused(E_ARG, g, d_sel, None, c.n_docs)                     # one NULL
    refused(E_ARG, g, None, d_first, c.n_docs)
    refused(E_ARG, g, d_sel.data_ptr() + 4, d_first, c.n_docs)   # misalignment
    refused(E_ARG, g, d_sel, d_first.data_ptr() + 4, c.n_docs)
    refused(E_ARG, g, d_sel, d_first, c.n_docs, row=out["row"] + 4)
    refused(E_ARG, g, d_sel, d_first, c.n_docs, st=out["st"] + 2)
    refused(E_ARG, g, d_sel, d_first, c.n_docs, cnt=out["cnt"] + 1)
    refused(E_ARG, g, d_sel, d_first, c.n_docs, flags=2)
    refused(E_ARG, g, d_sel, d_first, 2 ** 32)

    def with_first(change):
        f = c.first.copy()
        change(f)
        return dev.upload(f)

    def set_(i, v):
        return lambda f: f.__setitem__(i, v)
    refused(E_ARG, g, d_sel, with_first(set_(0, 1)), c.n_docs)               # doc_first[0] != 0
    assert c.first[-2] > 0
    refused(E_ARG, g, d_sel, with_first(set_(1, c.first[2] + np.uint64(1))), c.n_docs)      # a decrease at the first entry that can hold one
    refused(E_ARG, g, d_sel, with_first(set_(0, c.first[1] + np.uint64(1))), c.n_docs)      # ... and in front of it
    refused(E_ARG, g, d_sel, with_first(set_(-1, c.first[-2] - np.uint64(1))), c.n_docs)    # a decrease at the last entry
    refused(E_ARG, g, d_sel, with_first(lambda f: f.__setitem__(slice(1, None), 2 ** 32)), c.n_docs)   # 2^32 records
    for at in (0, c.n // 2, c.n - 1):                            # a state equal to num_final
        sel = c.sel()
        sel["state"][at] = c.num_final
        refused(E_ARG, g, dev.upload(sel), d_first, c.n_docs)
    rc, n = raw_call(g, d_sel, d_first, c.n_docs, **{**out, "cap": nt - 1})
    assert (rc, n) == (E_OVERFLOW, nt)
    # and the call that breaks no rule
    rc, n = raw_call(g, d_sel, d_first, c.n_docs, **out)
    g.sync(0)
    assert (rc, n) == (OK, nt)
    check(c.want(), *(buf[k].host().view(dt) for k, dt in (("d_row_ptr_out", np.uint64), ("d_states_out", np.uint32), ("d_counts_out", np.uint32))))


def test_a_stale_selection_is_refused():
    dev = passguard.Device(2)
    try:
        g, x = dev.g, dev.x
        key = x.doc_key("tiny")
        dev.scan(key)
        off = x.offsets(2, key, "tiny")
        nd, d_off = int(off.size - 1), dev.upload(off)
        g.select_leftmost_longest_documents(nd, d_doc_offsets=d_off)
        assert g.document_term_counts(nd, selection=True) > 0
        g.scan_resident(key[1], key[2], d_input=dev.d_input(key[0]))         # a later scan: the picks are stale
        assert raw_call(g, None, None, nd, flags=1) == (E_STATE, 0)
        g.select_leftmost_longest_documents(nd, d_doc_offsets=d_off)
        g.load_table(dev.table)                                  # ... and a later table: its states mean something else
        assert raw_call(g, None, None, nd, flags=1) == (E_STATE, 0)
    finally:
        dev.close()


# ---------------------------------------------------------------------------
# the lifetime of the slot-owned result

def test_lifetime():
    dev = passguard.Device(2)
    try:
        g, x = dev.g, dev.x
        a, b = cases(2)["n2049"], cases(2)["n65"]
        ups = {c.name: (dev.upload(c.sel()), dev.upload(c.first)) for c in (a, b)}

        def run(c):
            n = g.document_term_counts(c.n_docs, d_sel=ups[c.name][0], d_doc_first=ups[c.name][1])
            assert n == c.want()[1].size
            return n

        def fetch_status(c):
            row = np.empty(c.n_docs + 1, dtype=np.uint64)
            rc = g._L.pfac_documents_term_counts_d2h(g._ctx, 0, row.ctypes.data, None, None)
            g.sync(0)
            return rc
        with pytest.raises(PfacError) as e:                      # nothing to fetch yet
            g.term_counts_to_host(1, 0)
        assert e.value.status == E_STATE
        n = run(a)
        # a scan, a table upload and a score pass in between do not discard it
        key = x.doc_key("tiny")
        dev.scan(key)
        off = x.offsets(2, key, "tiny")
        g.load_table(dev.table)
        g.set_final_lengths(dev.table.final_lengths())
        dev.cur = None
        dev.scan(key)
        g.set_pattern_weights([0] + [1] * len(passguard.LINES16))
        g.document_scores(int(off.size - 1), d_doc_offsets=dev.upload(off))
        check(a.want(), *g.term_counts_to_host(a.n_docs, n), what="behind a scan, an upload and a score pass")
        # a second call discards the first result
        n = run(b)
        check(b.want(), *g.term_counts_to_host(b.n_docs, n), what="the second call")
        # a failed call discards it
        assert raw_call(g, ups[b.name][0], ups[b.name][1], b.n_docs, flags=2)[0] == E_ARG
        assert fetch_status(b) == E_STATE
        run(b)
        assert fetch_status(b) == OK
    finally:
        dev.close()


# ---------------------------------------------------------------------------
# the conveniences

PATTERNS = b"he\nshe\nhers\nhis\n"                              # ids 1, 2, 3, 4
LOG = b"she sells\nhis hers\n\nhe he he\nushers\n"
ROWS = [{1: 1, 2: 1}, {1: 1, 3: 1, 4: 1}, {}, {1: 3}, {1: 1, 2: 1, 3: 1}]
ROWS_WORDS = [{2: 1}, {3: 1, 4: 1}, {}, {1: 3}, {}]              # "he" inside "she" and "hers", "ushers": no whole word
ROWS_PICKS = [{2: 1}, {3: 1, 4: 1}, {}, {1: 3}, {2: 1}]          # leftmost-longest: "she" wins over "he", "hers" over "he"


def as_rows(table, triple):
    row, st, cnt = triple
    assert row.dtype == np.uint64 and st.dtype == np.uint32 and cnt.dtype == np.uint32
    ids = table.states_to_patterns(st)
    r = row.astype(np.int64)
    return [dict(zip(ids[a:b].tolist(), cnt[a:b].tolist())) for a, b in zip(r[:-1], r[1:])]


def test_conveniences_on_a_small_log():
    table = PfacTable.from_bytes(PATTERNS, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        assert as_rows(table, g.term_counts_lines(LOG)) == ROWS
        assert as_rows(table, g.term_counts_lines(LOG, whole_words=True)) == ROWS_WORDS
        assert as_rows(table, g.term_counts_lines(LOG, non_overlapping=True)) == ROWS_PICKS
        assert as_rows(table, g.term_counts_lines(LOG.replace(b"\n", b";"), delimiter=b";")) == ROWS
        docs = [b"she sells", b"", b"ushers", b"his hers"]
        assert as_rows(table, g.term_counts_documents(docs)) == [ROWS[0], {}, ROWS[4], ROWS[1]]
        assert as_rows(table, g.term_counts_documents(docs, whole_words=True)) == [ROWS_WORDS[0], {}, {}, ROWS_WORDS[1]]
        assert as_rows(table, g.term_counts_documents(docs, non_overlapping=True)) == [ROWS_PICKS[0], {}, ROWS_PICKS[4], ROWS_PICKS[1]]
    folded = PfacTable.from_bytes(PATTERNS, 256, ignore_case=True)
    with GpuMatcher(0, 1) as g:
        g.load_table(folded)
        assert as_rows(folded, g.term_counts_lines(LOG.upper())) == ROWS
        assert as_rows(folded, g.term_counts_lines(b"She sells\nHIS hers\n\nhe HE He\nuSHErs\n", whole_words=True)) == ROWS_WORDS


def test_term_matrix_is_the_dense_reference():
    dev, c = device(2), cases(2)["n65"]
    g = dev.g
    want = c.want()
    nt = want[1].size
    d_row = torch.zeros(c.n_docs + 1, dtype=torch.int64, device="cuda:0")
    d_st = torch.zeros(nt, dtype=torch.int32, device="cuda:0")
    d_cnt = torch.zeros(nt, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    n = g.document_term_counts(c.n_docs, d_sel=dev.upload(c.sel()), d_doc_first=dev.upload(c.first), d_row_ptr=d_row, d_states=d_st,
                               d_counts=d_cnt, out_cap=nt)
    g.sync(0)
    m = g.term_matrix(c.n_docs, n, d_row, d_st, d_cnt)
    assert m.layout == torch.sparse_csr and m.is_cuda and tuple(m.shape) == (c.n_docs, c.num_final)
    np.testing.assert_array_equal(m.to_dense().cpu().numpy().astype(np.int64), termref.dense(*want, c.num_final))
