"""Rule sets per document on the GPU (run with -m gpu on an MI355X): pfac_table_set_rules, pfac_documents_rules and
pfac_documents_rules_d2h against tests/ruleref.py, whose cases tests/test_rules_ref.py holds against two more references
and checks for their preconditions without a GPU.  Most cases are host-made matrices fed through d_row_ptr and d_states:
no scan, small shapes.  Every such case runs through passguard.exact_call with guard bands of exactly (n_docs + 1) x 8
and n_fired x 4 bytes.  Integer work: bit-exact.  No expectation comes from the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import countref
import passguard
import ruleref
import termref
from heapguard import FILLS, GuardedBuffer
from passguard import E_ARG, E_OVERFLOW, E_STATE, OK, Want, exact_call
from phfpfac_amd import PFAC_RULE_NOT, GpuMatcher, PfacError, PfacTable
from phfpfac_amd.matcher import _ptr
from ruleref import Rules, cases, check, fired, names

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


def set_rules(g, rules):
    return g.set_rules((rules.rule_ptr, rules.terms, rules.need))


def raw_set(g, ptr, terms, need, n_rules=None):
    """pfac_table_set_rules as it is."""
    ptr, terms, need = (np.ascontiguousarray(a, dtype=dt) for a, dt in ((ptr, np.uint64), (terms, np.uint32), (need, np.uint32)))
    return g._L.pfac_table_set_rules(g._ctx, ptr.ctypes.data, terms.ctypes.data if terms.size else None, need.ctypes.data if need.size else None,
                                     int(need.size if n_rules is None else n_rules))


def raw_call(g, d_row, d_st, n_docs, flags=0, row=None, out=None, cap=0, slot=0):
    """The C-ABI as it is: (status, *n_fired)."""
    n = C.c_uint64(12345)
    rc = g._L.pfac_documents_rules(g._ctx, slot, _ptr(d_row), _ptr(d_st), int(n_docs), int(flags), _ptr(row), _ptr(out), int(cap), C.byref(n))
    return rc, n.value


def guarded(n_docs, n_fired, fill):
    return {"d_row_ptr_out": GuardedBuffer((n_docs + 1) * 8, fill=fill), "d_rules_out": GuardedBuffer(n_fired * 4, fill=fill)}


def exact(dev, c, fill):
    """One case into caller's buffers of exactly the result's bytes: one entry too few, then the exact capacity."""
    g = dev.g
    want = c.want()
    set_rules(g, c.rules)
    d_row, d_st = dev.upload(c.row), dev.upload(c.states)
    buf = guarded(c.n_docs, want[1].size, fill)

    def call(cap, bad=None):
        return dev._status(lambda: g.document_rules(c.n_docs, d_row_ptr=d_row, d_states=d_st, d_row_ptr_out=buf["d_row_ptr_out"].ptr,
                                                    d_rules=buf["d_rules_out"].ptr, out_cap=cap), "n_fired")
    w = Want(want[1].size, {"d_row_ptr_out": want[0], "d_rules_out": want[1]})
    exact_call(g, call, w, buf, fill, f"pfac_documents_rules case {c.name} ({c.n} pairs, {c.n_docs} documents, {c.rules.n_rules} rules, "
                                      f"{c.E} keys, {c.passes} passes)")
    return d_row, d_st


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("W,name", ALL, ids=[f"{W}-{n}" for W, n in ALL])
def test_case_at_exact_capacity(W, name, fill):
    dev = device(W)
    assert dev.table.num_final == termref.num_final(W)
    exact(dev, cases(W)[name], fill)


def test_several_chunks_per_workgroup(monkeypatch):
    """The sort's workgroups limited to three (the PFAC_TERMS_ROWS knob, read when the table is installed): every workgroup
    of the histogram and scatter kernels loops over several chunks of 1024 keys, the last one over fewer."""
    monkeypatch.setenv("PFAC_TERMS_ROWS", str(ruleref.CHUNKED_ROWS))
    dev = passguard.Device(2)
    try:
        assert len(ruleref.CHUNKED) == 4
        for name in ruleref.CHUNKED:
            assert cases(2)[name].E > ruleref.CHUNKED_ROWS * ruleref.SORT_BLOCK
            exact(dev, cases(2)[name], FILLS[0])
    finally:
        dev.close()


@pytest.mark.parametrize("W,name", [(2, "E12293"), (2, "fan3000"), (4, "E4097"), (2, "passes-r65-d524289")])
def test_slot_owned_result_twice_gives_the_same_bytes(W, name):
    dev, c = device(W), cases(W)[name]
    g = dev.g
    set_rules(g, c.rules)
    d_row, d_st = dev.upload(c.row), dev.upload(c.states)
    got = []
    for _ in range(2):
        n = g.document_rules(c.n_docs, d_row_ptr=d_row, d_states=d_st)
        assert n == c.want()[1].size
        got.append(g.rules_to_host(c.n_docs, n))
        check(c.want(), *got[-1], what=c.name)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*got))
    # each output alone may be the caller's: the other stays the slot's
    buf = guarded(c.n_docs, c.want()[1].size, FILLS[0])
    n = g.document_rules(c.n_docs, d_row_ptr=d_row, d_states=d_st, d_rules=buf["d_rules_out"].ptr, out_cap=c.want()[1].size)
    row = np.empty(c.n_docs + 1, dtype=np.uint64)
    assert g._L.pfac_documents_rules_d2h(g._ctx, 0, row.ctypes.data, None) == OK
    g.sync(0)
    buf["d_rules_out"].check(what="d_rules_out")
    check(c.want(), row, buf["d_rules_out"].host().view(np.uint32), what=c.name)
    out = np.empty(max(n, 1), dtype=np.uint32)
    assert g._L.pfac_documents_rules_d2h(g._ctx, 0, None, out.ctypes.data) == E_STATE      # it went to the caller's buffer
    buf["d_row_ptr_out"].check(payload_untouched=True, what="a d_row_ptr_out the call did not get")


# ---------------------------------------------------------------------------
# real inputs: scan, segment pass / per-document selection, term counts, rules -- against the CPU oracle's records

def rules_over(states, nf, seed, n_rules=300):
    """Rules of 2 to 4 terms over the states that occur (so that they fire), some negated, need 1..|P|."""
    rng = np.random.default_rng([0x52554C45, seed])
    pool = np.unique(np.asarray(states, dtype=np.int64))
    out = []
    for _ in range(n_rules):
        t = rng.permutation(pool)[: int(rng.integers(2, 5))].tolist()
        n_neg = int(rng.integers(0, len(t))) if rng.random() < 0.3 else 0
        pos = t[: len(t) - n_neg]
        out.append((pos, t[len(pos):], int(rng.integers(1, len(pos) + 1))))
    return Rules(out, nf)


@pytest.mark.parametrize("W", passguard.WIDTHS)
@pytest.mark.parametrize("shape", ["tiny", "emptygroup"])
def test_slot_owned_segment_and_selection(W, shape):
    dev = device(W) if W != 8 else passguard.Device(8)
    try:
        g, x = dev.g, dev.x
        nf = int(dev.table.num_final)
        key = x.doc_key(shape)
        dev.scan(key)
        off = x.offsets(W, key, shape)
        nd, d_off = int(off.size - 1), dev.upload(off)
        for picks in (False, True):
            if picks:
                first, _, ids, _, _ = x.docsel(W, key, shape)
                assert g.select_leftmost_longest_documents(nd, d_doc_offsets=d_off) == ids.size > 500
            else:
                first, _, ids = x.seg(W, key, shape)
                assert g.segment_records(nd, d_doc_offsets=d_off) == ids.size > 1000
            row, st, _ = termref.term_counts(countref.states_of(dev.table, ids), first, nf)
            rules = rules_over(st, nf, W)
            want = fired(row, st, rules)
            assert 0 < want[1].size < nd * rules.n_rules
            set_rules(g, rules)
            assert g.document_term_counts(nd, selection=picks) == st.size
            n = g.document_rules(nd)
            assert n == want[1].size
            check(want, *g.rules_to_host(nd, n), what=f"{'selection' if picks else 'segment'}, width {W}, {shape}")
            assert raw_call(g, None, None, nd + 1)[0] == E_ARG       # an n_docs that is not the term counts'
    finally:
        if W == 8:
            dev.close()


# ---------------------------------------------------------------------------
# errors

def test_set_rules_validation():
    dev = passguard.Device(2)
    try:
        g = dev.g
        nf = int(dev.table.num_final)
        c = cases(2)["neighbours"]
        d_row, d_st = dev.upload(c.row), dev.upload(c.states)
        with GpuMatcher(0, 1) as bare:
            assert raw_set(bare, [0, 1], [0], [1]) == E_STATE                # before a table upload
            assert raw_set(bare, [0], [], []) == E_STATE
        set_rules(g, c.rules)
        N = PFAC_RULE_NOT
        for ptr, terms, need in (([1, 2], [1, 2], [1]),                      # rule_ptr[0] != 0
                                 ([0, 2, 1], [1, 2], [1, 1]),                # a decrease
                                 ([0, 2], [1, nf], [1]),                     # a state at num_final
                                 ([0, 2], [1, nf | N], [1]),                 # ... negated
                                 ([0, 2, 4], [1, 2, 3, 3], [1, 1]),          # a state twice in one rule
                                 ([0, 2, 4], [1, 2, 3, 3 | N], [1, 1]),      # ... under either sign
                                 ([0, 2], [1, 2], [0]),                      # need == 0
                                 ([0, 2], [1, 2], [3]),                      # need above the positive terms
                                 ([0, 3], [1, 2, 3 | N], [3]),
                                 ([0, 1], [1 | N], [1])):                    # no positive term
            assert raw_set(g, ptr, terms, need) == E_ARG, (ptr, terms, need)
            n = g.document_rules(c.n_docs, d_row_ptr=d_row, d_states=d_st)   # the earlier rules are kept
            check(c.want(), *g.rules_to_host(c.n_docs, n), what="behind a refused pfac_table_set_rules")
        assert g._L.pfac_table_set_rules(g._ctx, None, None, None, 1) == E_ARG
        assert g._L.pfac_table_set_rules(g._ctx, None, None, None, 2 ** 31) == E_ARG
        assert raw_set(g, [0, 2, 4], [1, 2, 2, 3], [1, 1]) == OK            # the same state in two rules is no repeat
        assert raw_set(g, [0, 2, 2], [1, 2], [1, 1]) == E_ARG                # an empty rule: need above its 0 positive terms
        # a second call replaces the rules; n_rules == 0 clears them and nothing else
        other = Rules([([1], [], 1), ([2], [3], 1)], nf)
        set_rules(g, other)
        n = g.document_rules(c.n_docs, d_row_ptr=d_row, d_states=d_st)
        check(fired(c.row, c.states, other), *g.rules_to_host(c.n_docs, n), what="the second rule table")
        assert g._L.pfac_table_set_rules(g._ctx, None, None, None, 0) == OK
        assert raw_call(g, d_row, d_st, c.n_docs) == (E_STATE, 0)
        g.set_pattern_weights([0] + [1] * len(passguard.LINES16))            # (what else is attached still works)
    finally:
        dev.close()


def test_error_ladder():
    dev, c = device(2), cases(2)["E1025"]
    g = dev.g
    set_rules(g, c.rules)
    d_row, d_st = dev.upload(c.row, slack=16), dev.upload(c.states, slack=16)
    nfired = c.want()[1].size
    buf = guarded(c.n_docs, nfired, FILLS[1])
    out = dict(row=buf["d_row_ptr_out"].ptr, out=buf["d_rules_out"].ptr, cap=nfired)

    def refused(status, *a, **kw):
        rc, n = raw_call(*a, **{**out, **kw})
        assert rc == status, f"{passguard.STATUS.get(rc, rc)}, want {passguard.STATUS[status]}: {kw}"
        assert n == 0
        a[0].sync(0)
        for name, b in buf.items():
            b.check(payload_untouched=True, what=name)

    with GpuMatcher(0, 1) as bare:                               # no table
        refused(E_STATE, bare, d_row, d_st, c.n_docs)
        refused(E_STATE, bare, d_row, d_st, c.n_docs, flags=1)               # ... comes before the flags
        bare.load_table(dev.table)                               # no rules
        refused(E_STATE, bare, d_row, d_st, c.n_docs)
        refused(E_STATE, bare, d_row.data_ptr() + 4, d_st, c.n_docs)        # ... comes before the alignment
        set_rules(bare, c.rules)                                 # no term counts held
        refused(E_STATE, bare, None, None, c.n_docs)
        refused(E_STATE, bare, None, None, c.n_docs, flags=1)
        # term counts whose states went to the caller: not the slot's
        tc = termref.cases(2)["n65"]
        st_out = torch.zeros(tc.want()[1].size + 4, dtype=torch.int32, device="cuda:0")
        bare.document_term_counts(tc.n_docs, d_sel=dev.upload(tc.sel()), d_doc_first=dev.upload(tc.first), d_states=st_out,
                                  out_cap=tc.want()[1].size)
        refused(E_STATE, bare, None, None, tc.n_docs)
        bare.document_term_counts(tc.n_docs, d_sel=dev.upload(tc.sel()), d_doc_first=dev.upload(tc.first))
        assert raw_call(bare, None, None, tc.n_docs)[0] == OK
        bare.load_table(dev.table)                               # made with an earlier table (and the rules are gone)
        refused(E_STATE, bare, None, None, tc.n_docs)
        set_rules(bare, c.rules)
        refused(E_STATE, bare, None, None, tc.n_docs)
    refused(E_ARG, g, d_row, None, c.n_docs)                     # one NULL
    refused(E_ARG, g, None, d_st, c.n_docs)
    refused(E_ARG, g, d_row.data_ptr() + 4, d_st, c.n_docs)      # misalignment
    refused(E_ARG, g, d_row, d_st.data_ptr() + 2, c.n_docs)
    refused(E_ARG, g, d_row, d_st, c.n_docs, row=out["row"] + 4)
    refused(E_ARG, g, d_row, d_st, c.n_docs, out=out["out"] + 2)
    refused(E_ARG, g, d_row, d_st, c.n_docs, flags=1)
    refused(E_ARG, g, d_row, d_st, 2 ** 32)

    def with_row(change):
        f = c.row.copy()
        change(f)
        return dev.upload(f)

    def set_(i, v):
        return lambda f: f.__setitem__(i, v)
    refused(E_ARG, g, with_row(set_(0, 1)), d_st, c.n_docs)                  # row_ptr[0] != 0
    assert c.row[2] > c.row[1] > 0
    refused(E_ARG, g, with_row(set_(1, c.row[2] + np.uint64(1))), d_st, c.n_docs)        # a decrease
    refused(E_ARG, g, with_row(set_(-1, c.row[-2] - np.uint64(1))), d_st, c.n_docs)      # ... at the last entry
    refused(E_ARG, g, with_row(lambda f: f.__setitem__(slice(1, None), 2 ** 32)), d_st, c.n_docs)     # 2^32 pairs
    for at in (0, c.n // 2, c.n - 1):                            # a state equal to num_final
        st = c.states.copy()
        st[at] = c.num_final
        refused(E_ARG, g, d_row, dev.upload(st), c.n_docs)
    inner = np.flatnonzero(np.diff(c.row.astype(np.int64)) >= 2)
    for d in (int(inner[0]), int(inner[-1])):                    # states not ascending in a row: equal, and swapped
        a = int(c.row[d])
        st = c.states.copy()
        st[a + 1] = st[a]
        refused(E_ARG, g, d_row, dev.upload(st), c.n_docs)
        st = c.states.copy()
        st[[a, a + 1]] = st[[a + 1, a]]
        refused(E_ARG, g, d_row, dev.upload(st), c.n_docs)
    rc, n = raw_call(g, d_row, d_st, c.n_docs, **{**out, "cap": nfired - 1})
    assert (rc, n) == (E_OVERFLOW, nfired)
    g.sync(0)
    for name, b in buf.items():
        b.check(payload_untouched=True, what=name)
    # and the call that breaks no rule
    rc, n = raw_call(g, d_row, d_st, c.n_docs, **out)
    g.sync(0)
    assert (rc, n) == (OK, nfired)
    check(c.want(), buf["d_row_ptr_out"].host().view(np.uint64), buf["d_rules_out"].host().view(np.uint32))


def test_an_expansion_of_2_32_keys_is_refused():
    """2^20 rules that name one state, 4096 documents that hold it: E = 2^32 exactly.  The count kernel's 64-bit group
    sums tell the host, which refuses before anything is expanded; one document fewer is not run here (its sort alone
    would hold 64 GiB)."""
    dev = device(2)
    g = dev.g
    n_rules, n_docs = 1 << 20, 4096
    rules = Rules.from_arrays(np.arange(n_rules + 1), np.full(n_rules, 5), np.ones(n_rules), 16)
    set_rules(g, rules)
    row, st = np.arange(n_docs + 1, dtype=np.uint64), np.full(n_docs, 5, dtype=np.uint32)
    assert int(rules.degree()[5]) * n_docs == 1 << 32
    buf = guarded(n_docs, 16, FILLS[0])
    rc, n = raw_call(g, dev.upload(row), dev.upload(st), n_docs, row=buf["d_row_ptr_out"].ptr, out=buf["d_rules_out"].ptr, cap=16)
    g.sync(0)
    assert (rc, n) == (E_ARG, 0)
    for name, b in buf.items():
        b.check(payload_untouched=True, what=name)
    # the same rules over one document: every rule fires
    n = g.document_rules(1, d_row_ptr=dev.upload(row[:2]), d_states=dev.upload(st[:1]))
    got = g.rules_to_host(1, n)
    assert n == n_rules and got[0].tolist() == [0, n_rules] and np.array_equal(got[1], np.arange(n_rules, dtype=np.uint32))


# ---------------------------------------------------------------------------
# the lifetime of the rules and of the slot-owned result

def test_lifetime():
    dev = passguard.Device(2)
    try:
        g, x = dev.g, dev.x
        a, b = cases(2)["E4097"], cases(2)["negated"]
        ups = {c.name: (dev.upload(c.row), dev.upload(c.states)) for c in (a, b)}

        def run(c):
            set_rules(g, c.rules)
            n = g.document_rules(c.n_docs, d_row_ptr=ups[c.name][0], d_states=ups[c.name][1])
            assert n == c.want()[1].size
            return n

        def fetch_status(c):
            row = np.empty(c.n_docs + 1, dtype=np.uint64)
            rc = g._L.pfac_documents_rules_d2h(g._ctx, 0, row.ctypes.data, None)
            g.sync(0)
            return rc
        with pytest.raises(PfacError) as e:                      # nothing to fetch yet
            g.rules_to_host(1, 0)
        assert e.value.status == E_STATE
        n = run(a)
        # a scan, a table upload, a group pass and a term-count pass in between do not discard it
        key = x.doc_key("tiny")
        dev.scan(key)
        off = x.offsets(2, key, "tiny")
        nd, d_off = int(off.size - 1), dev.upload(off)
        g.load_table(dev.table)
        g.set_final_lengths(dev.table.final_lengths())
        dev.cur = None
        dev.scan(key)
        g.set_pattern_groups([None] + [k % 3 for k in range(len(passguard.LINES16))])
        g.document_group_masks(nd, d_doc_offsets=d_off)
        g.segment_records(nd, d_doc_offsets=d_off)
        g.document_term_counts(nd)
        check(a.want(), *g.rules_to_host(a.n_docs, n), what="behind a scan, an upload, a group pass and a term-count pass")
        # ... but the upload dropped the rules, and the refused call discards the result
        assert raw_call(g, *ups[a.name], a.n_docs) == (E_STATE, 0)
        assert fetch_status(a) == E_STATE
        n = run(a)
        check(a.want(), *g.rules_to_host(a.n_docs, n), what="with the rules set again")
        # a second call discards the first result
        n = run(b)
        check(b.want(), *g.rules_to_host(b.n_docs, n), what="the second call")
        # a failed call discards it
        assert raw_call(g, *ups[b.name], b.n_docs, flags=2)[0] == E_ARG
        assert fetch_status(b) == E_STATE
        run(b)
        assert fetch_status(b) == OK
    finally:
        dev.close()


# ---------------------------------------------------------------------------
# the conveniences

PATTERNS = b"he\nshe\nhers\nhis\n"                              # ids 1, 2, 3, 4
LOG = b"she sells\nhis hers\n\nhe he he\nushers\n"
# every match:      {he, she}   {he, hers, his}   {}   {he}   {he, she, hers}
# whole words:      {she}       {hers, his}       {}   {he}   {}
# leftmost-longest: {she}       {hers, his}       {}   {he}   {she}
RULES = [[1, 2],                                                # 0: he and she
         {"any_of": [3, 4]},                                    # 1: hers or his
         {"all_of": [1], "none_of": [2]},                       # 2: he and not she
         {"all_of": [1, 2, 3, 4], "need": 3},                   # 3: three of the four
         {"any_of": [2, 3], "none_of": [4]}]                    # 4: (she or hers) and not his
FIRED = [[0, 4], [1, 2, 3], [], [2], [0, 1, 3, 4]]
FIRED_WORDS = [[4], [1], [], [2], []]
FIRED_PICKS = [[4], [1], [], [2], [4]]


def as_rows(pair):
    row, rules = pair
    assert row.dtype == np.uint64 and rules.dtype == np.uint32
    r = row.astype(np.int64)
    return [rules[a:b].tolist() for a, b in zip(r[:-1], r[1:])]


def test_conveniences_on_a_small_log():
    table = PfacTable.from_bytes(PATTERNS, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        assert g.set_rules(RULES) == 5
        assert as_rows(g.rules_lines(LOG)) == FIRED
        assert as_rows(g.rules_lines(LOG, whole_words=True)) == FIRED_WORDS
        assert as_rows(g.rules_lines(LOG, non_overlapping=True)) == FIRED_PICKS
        assert as_rows(g.rules_lines(LOG.replace(b"\n", b";"), delimiter=b";")) == FIRED
        docs = [b"she sells", b"", b"ushers", b"his hers"]
        assert as_rows(g.rules_documents(docs)) == [FIRED[0], [], FIRED[4], FIRED[1]]
        assert as_rows(g.rules_documents(docs, non_overlapping=True)) == [FIRED_PICKS[0], [], FIRED_PICKS[4], FIRED_PICKS[1]]
        g.load_table(table)                                      # an upload drops the rules
        with pytest.raises(PfacError) as e:
            g.rules_lines(LOG)
        assert e.value.status == E_STATE
    folded = PfacTable.from_bytes(PATTERNS, 256, ignore_case=True)
    with GpuMatcher(0, 1) as g:
        g.load_table(folded)
        g.set_rules(RULES)
        assert as_rows(g.rules_lines(LOG.upper())) == FIRED
        assert as_rows(g.rules_lines(b"She sells\nHIS hers\n\nhe HE He\nuSHErs\n", whole_words=True)) == FIRED_WORDS


def test_rule_matrix_is_the_dense_reference():
    dev, c = device(2), cases(2)["E1025"]
    g = dev.g
    set_rules(g, c.rules)
    want = c.want()
    nf = want[1].size
    d_row = torch.zeros(c.n_docs + 1, dtype=torch.int64, device="cuda:0")
    d_out = torch.zeros(nf, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    n = g.document_rules(c.n_docs, d_row_ptr=dev.upload(c.row), d_states=dev.upload(c.states), d_row_ptr_out=d_row, d_rules=d_out, out_cap=nf)
    g.sync(0)
    m = g.rule_matrix(c.n_docs, n, d_row, d_out)
    assert m.layout == torch.sparse_csr and m.is_cuda and tuple(m.shape) == (c.n_docs, c.rules.n_rules)
    np.testing.assert_array_equal(m.to_dense().cpu().numpy().astype(np.int64), ruleref.fired_dense(c.row, c.states, c.rules))
