"""WordPiece on the GPU (run with -m gpu on an MI355X): pfac_table_set_wordpiece, pfac_records_filter_roles,
pfac_wordpiece_leftmost_longest and pfac_wordpiece_documents against tests/wpref.py, whose cases
tests/test_wordpiece_ref.py holds against a second form of the rule (and a library) and checks for their preconditions
without a GPU.  Every named case runs through passguard.exact_call with guard bands of exactly n_tokens x 4 (ids),
n_tokens x 4 (positions) and (n_docs + 1) x 8 bytes, one below the capacity first, under both fills.  Integer work:
bit-exact.  No expectation comes from the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import passguard
import wpref
from heapguard import FILLS, GuardedBuffer
from passguard import E_ARG, E_OVERFLOW, E_STATE, OK, TILE, Want, exact_call
from phfpfac_amd import PFAC_TOKENS_POSITIONS, GpuMatcher, PfacError, wordpiece_table
from phfpfac_amd.matcher import _ptr
from wpref import DROP, case, check, names, want_of

pytestmark = pytest.mark.gpu

KNOBS = {2: {}, 4: {"PFAC_REC_BYTES": "4"}, 8: {"PFAC_WIDE": "1"}}
_DEV = {}


class WpDevice:
    """One GpuMatcher with the cases' vocabulary as wordpiece_table builds it, at record width W; `prepare(name)` leaves
    the case's scan, role filter and selection as the slot's last."""

    def __init__(self, W, fold):
        self.W, self.fold = W, fold
        self.table, self.first, self.cont, _, _ = wordpiece_table(wpref.ENTRIES, word_bytes=wpref.CASE_WORD, ignore_case=fold)
        self.g = GpuMatcher(0, 1)
        with passguard._Env(KNOBS[W]):
            self.g.load_table(self.table)
        self.flen = self.table.final_lengths()
        self.g.set_final_lengths(self.flen)
        self.inputs, self.attached = {}, None

    def close(self):
        self.g.close()

    def d_input(self, name):
        if name not in self.inputs:
            raw = np.ascontiguousarray(case(name)[0])
            t = torch.zeros(raw.size + TILE, dtype=torch.uint8, device="cuda:0")
            if raw.size:
                t[:raw.size].copy_(torch.from_numpy(raw.copy()))
            torch.cuda.synchronize()
            self.inputs[name] = t
        return self.inputs[name]

    def attach(self, v, byte_ids="given"):
        key = (v.max_word, tuple(v.byte_ids.tolist()), byte_ids)
        if self.attached != key:
            self.g.set_wordpiece(self.first, self.cont, None if byte_ids is None else v.byte_ids, v.unk, v.word_set(), v.max_word)
            self.attached = key

    def scan(self, name):
        data, no, _, _ = case(name)
        self.g.reserve(0, 0, max(data.size, TILE))
        n = self.g.scan_resident(no, data.size, d_input=self.d_input(name))
        assert self.g.scan_format()[0] == self.W, f"record width {self.g.scan_format()[0]}, want {self.W}"
        return n

    def prepare(self, name, byte_ids="given"):
        """-> n_docs or None"""
        data, no, v, off = case(name)
        assert v.fold == self.fold
        self.attach(v, byte_ids)
        self.scan(name)
        self.g.filter_roles(0, d_input=self.d_input(name))
        if off is None:
            self.g.select_leftmost_longest(0)
            return None
        self.g.set_doc_offsets(off)
        self.g.select_leftmost_longest_documents(int(off.size) - 1)
        return int(off.size) - 1

    def status(self, fn, attr=None):
        try:
            return OK, fn()
        except PfacError as e:
            return e.status, getattr(e, attr, None) if attr else None


def device(W=2, fold=False):
    if (W, fold) not in _DEV:
        _DEV[W, fold] = WpDevice(W, fold)
    return _DEV[W, fold]


@pytest.fixture(scope="module", autouse=True)
def _close_devices():
    yield
    for d in _DEV.values():
        d.close()
    _DEV.clear()


def exact(name, fill, W=2, byte_ids="given"):
    dev = device(W, case(name)[2].fold)
    nd = dev.prepare(name, byte_ids)
    g, want = dev.g, want_of(name)
    n = int(want[0].size)
    buf = {"d_ids": GuardedBuffer(n * 4, fill=fill), "d_pos": GuardedBuffer(n * 4, fill=fill)}
    payloads = {"d_ids": want[0], "d_pos": want[1]}
    d_in = dev.d_input(name)
    if nd is None:
        def call(cap, bad=None):
            return dev.status(lambda: g.wordpiece_selection(d_input=d_in, d_ids=buf["d_ids"].ptr, out_cap=cap, d_pos=buf["d_pos"].ptr), "n_tokens")
    else:
        buf["d_tok_offsets"] = GuardedBuffer((nd + 1) * 8, fill=fill)
        payloads["d_tok_offsets"] = want[2]

        def call(cap, bad=None):
            return dev.status(lambda: g.wordpiece_selection_documents(d_input=d_in, d_ids=buf["d_ids"].ptr, out_cap=cap, d_pos=buf["d_pos"].ptr,
                                                                      d_tok_offsets=buf["d_tok_offsets"].ptr), "n_tokens")
    exact_call(g, call, Want(n, payloads), buf, fill, f"wordpiece case {name} ({n} tokens" + (f", {nd} documents)" if nd is not None else ")"))


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name", names())
def test_case_at_exact_capacity(name, fill):
    exact(name, fill)


@pytest.mark.parametrize("W", [4, 8])
@pytest.mark.parametrize("name", ["n17", "t3", "t65", "edge-hole-left", "group-len-over", "docs-cut", "docs-tiny"])
def test_wider_records(name, W):
    exact(name, FILLS[0], W)


def test_null_byte_ids_drop_every_byte():
    """NULL byte_ids are all-DROP byte_ids: the case whose vocabulary has none, attached with a NULL pointer."""
    assert (case("alldrop-bytes")[2].byte_ids == DROP).all()
    exact("alldrop-bytes", FILLS[0], byte_ids=None)


@pytest.mark.parametrize("name", ["n0", "n17", "t65", "docs-emptygroup", "folded"])
def test_slot_owned_result(name):
    dev = device(2, case(name)[2].fold)
    nd = dev.prepare(name)
    g, want = dev.g, want_of(name)
    n = int(want[0].size)
    d_in = dev.d_input(name)
    if nd is None:
        assert g.wordpiece_selection(d_input=d_in, positions=True) == n
        check(want, *g.tokens_to_host(n, True), what=name)
    else:
        assert g.wordpiece_selection_documents(d_input=d_in, positions=True) == n
        check(want, *g.tokens_to_host(n, True), tok_off=g.token_offsets_to_host(nd), what=name)
    if n > 5:
        a, b = g.tokens_to_host(n - 5, True, first=3)
        assert np.array_equal(a, want[0][3:n - 2]) and np.array_equal(b, want[1][3:n - 2])
    # without the flag: ids only
    assert (g.wordpiece_selection(d_input=d_in) if nd is None else g.wordpiece_selection_documents(d_input=d_in)) == n
    check(want, g.tokens_to_host(n), what=name)
    if n:
        assert dev.status(lambda: g.tokens_to_host(n, True))[0] == E_STATE, "the last call wrote no positions"


# ---------------------------------------------------------------------------
# the role filter

def kept_reference(name, whole_words=False):
    """(pos, lens, first id, continuation id) of the records the filter keeps, in heap order."""
    data, no, v, _ = case(name)
    pos, lens, idx = wpref.records(data, no, v)
    keep = wpref.role_filter(data, pos, lens, idx, v)
    if whole_words:
        W = np.concatenate([[False], v.word[data], [False]])
        cut = W[:-1] & W[1:]                                    # cut[i]: a word byte on both sides of position i
        keep &= ~cut[pos] & ~cut[pos + lens]
    pairs = np.array([v.pair(p) for p in v.pieces], dtype=np.int64)
    return pos[keep], lens[keep], pairs[idx[keep], 0], pairs[idx[keep], 1]


def held(dev, n, ref, no, what):
    g = dev.g
    assert n == ref[0].size, f"{what}: {n} records kept, want {ref[0].size}"
    assert g.last_count() == n
    rec = g.records_to_host(n)
    st = rec["state"].astype(np.int64)
    got = (rec["pos"].astype(np.int64), dev.flen[st].astype(np.int64), dev.first[st].astype(np.int64), dev.cont[st].astype(np.int64))
    for a, b, part in zip(got, ref, ("positions", "lengths", "first ids", "continuation ids")):
        assert np.array_equal(a, b), f"{what}: the {part} of the kept records differ"
    if dev.W == 8:                                              # (no packed form: the fetch above walked the tile index)
        return
    _, tix = g.packed_to_host()
    counts = np.bincount(ref[0] // TILE, minlength=tix.size)
    assert np.array_equal((tix >> np.uint64(40)).astype(np.int64), counts), f"{what}: the tile index's counts"


@pytest.mark.parametrize("W", passguard.WIDTHS)
@pytest.mark.parametrize("name", ["n4097", "t3", "t65", "end-pick-in-halo"])
def test_role_filter(name, W):
    dev = device(W)
    data, no, v, _ = case(name)
    dev.attach(v)
    d_in = dev.d_input(name)
    n_all = dev.scan(name)
    ref = kept_reference(name)
    assert 0 < ref[0].size < n_all, "the case drops some records and keeps some"
    n = dev.g.filter_roles(0, d_input=d_in)
    held(dev, n, ref, no, "the filter")
    held(dev, dev.g.filter_roles(0, d_input=d_in), ref, no, "the filter applied twice")
    # it composes with the whole-word filter, in either order
    refw = kept_reference(name, whole_words=True)
    assert 0 < refw[0].size < ref[0].size
    held(dev, dev.g.filter_whole_words(0, wpref.CASE_WORD, d_input=d_in), refw, no, "whole words behind the roles")
    dev.scan(name)
    dev.g.filter_whole_words(0, wpref.CASE_WORD, d_input=d_in)
    held(dev, dev.g.filter_roles(0, d_input=d_in), refw, no, "the roles behind whole words")
    # and the token pass takes the scan that went through both
    dev.g.select_leftmost_longest(0)
    assert dev.status(lambda: dev.g.wordpiece_selection(d_input=d_in))[0] == OK


# ---------------------------------------------------------------------------
# the ladder of errors, through the C ABI as it is

def raw(g, d_input=None, d_sel=None, flags=0, d_ids=None, cap=0, d_pos=None, docs=None):
    n = C.c_uint64(12345)
    if docs is None:
        rc = g._L.pfac_wordpiece_leftmost_longest(g._ctx, 0, _ptr(d_input), _ptr(d_sel), int(flags), _ptr(d_ids), int(cap), _ptr(d_pos), C.byref(n))
    else:
        rc = g._L.pfac_wordpiece_documents(g._ctx, 0, _ptr(d_input), _ptr(d_sel), _ptr(docs.get("off")), _ptr(docs.get("first")), int(flags),
                                           _ptr(d_ids), int(cap), _ptr(d_pos), _ptr(docs.get("tok_off")), C.byref(n))
    return rc, n.value


class Guards:
    def __init__(self, n=64, nd=8):
        self.ids, self.pos, self.off = GuardedBuffer(n * 4), GuardedBuffer(n * 4), GuardedBuffer((nd + 1) * 8)
        self.n = n

    def untouched(self, what):
        for name in ("ids", "pos", "off"):
            getattr(self, name).check(payload_untouched=True, what=f"{name} after {what}")


def log_table():
    table, first, cont, byte_ids, _ = wordpiece_table(wpref.LOG_VOCAB)
    return table, first, cont, byte_ids


def attach_log(g, first, cont, byte_ids, **kw):
    g.set_wordpiece(first, cont, byte_ids, unk_id=0, **kw)


def wp_scan(g, data):
    g.scan_bytes(data)
    g.filter_roles(0)
    g.select_leftmost_longest(0)


def test_ladder_of_state_errors():
    table, first, cont, byte_ids = log_table()
    data = np.frombuffer(wpref.LOG, dtype=np.uint8)
    gd = Guards()
    with GpuMatcher(0, 1) as g:
        def refused(what, status=E_STATE, **kw):
            rc, n = raw(g, flags=PFAC_TOKENS_POSITIONS, d_ids=gd.ids.ptr, cap=gd.n, d_pos=gd.pos.ptr, **kw)
            g.sync(0)
            assert rc == status, f"{what}: {passguard.STATUS.get(rc, rc)}"
            gd.untouched(what)

        def filter_rc():
            n = C.c_uint64(0)
            return g._L.pfac_records_filter_roles(g._ctx, 0, None, None, C.byref(n))
        refused("no table")
        ws = wpref.Vocab(wpref.LOG_VOCAB, b"[UNK]").word_set()
        rc = g._L.pfac_table_set_wordpiece(g._ctx, None, None, 0, None, 0, ws.ctypes.data, 100)
        assert rc == E_STATE, "the attachment before a table"
        g.load_table(table)
        assert filter_rc() == E_STATE, "the filter without a scan"
        g.set_final_lengths(table.final_lengths())
        g.scan_bytes(data)
        assert filter_rc() == E_STATE, "the filter without an attachment"
        assert "pfac_table_set_wordpiece" in g._L.pfac_last_error(g._ctx).decode()
        g.select_leftmost_longest(0)
        refused("no attachment")
        g.set_token_ids({1: 1})                                 # the plain token ids are another attachment
        refused("no attachment (plain token ids do not serve)")
        attach_log(g, first, cont, byte_ids)
        refused("no role filter")
        assert "pfac_records_filter_roles" in g._L.pfac_last_error(g._ctx).decode()
        g.filter_roles(0)
        refused("a selection made before the filter")
        g.select_leftmost_longest(0)
        assert raw(g)[0] == OK
        attach_log(g, first, cont, byte_ids)                    # the same ids again are a new attachment
        refused("a filter under an earlier attachment")
        g.filter_roles(0)
        g.select_leftmost_longest(0)
        assert raw(g) == (OK, len(wpref.LOG_IDS))
        g.scan_bytes(data)
        refused("a scan that has not been filtered (and no selection)")
        g.select_leftmost_longest(0)
        refused("a scan that has not been filtered")
        wp_scan(g, data)
        g.select_leftmost_longest(1)
        refused("a selection from entry 1")
        g.select_leftmost_longest(0)
        refused("pfac_wordpiece_documents over a whole-stream selection", docs={"tok_off": gd.off.ptr})
        assert raw(g)[0] == OK
        g.load_table(table)
        refused("an upload drops the attachment")
        g.set_final_lengths(table.final_lengths())
        attach_log(g, first, cont, byte_ids)
        refused("a selection of an earlier table")
        wp_scan(g, data)
        assert raw(g) == (OK, len(wpref.LOG_IDS))
        g.reserve(0, 1 << 20, 1 << 16)
        refused("a reserve that replaced a buffer")


def test_ladder_of_argument_errors():
    table, first, cont, byte_ids = log_table()
    data = np.frombuffer(wpref.LOG, dtype=np.uint8)
    nf = int(table.num_final)
    gd = Guards(nd=4)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        L = g._L
        ws = wpref.Vocab(wpref.LOG_VOCAB, b"[UNK]").word_set()
        f, c = first.copy(), cont.copy()

        def attach(first=f, cont=c, n=nf, bytes_=byte_ids, unk=0, cap=100):
            return L.pfac_table_set_wordpiece(g._ctx, first.ctypes.data, cont.ctypes.data, n, None if bytes_ is None else bytes_.ctypes.data,
                                              unk, ws.ctypes.data, cap)
        assert attach() == OK
        wp_scan(g, data)
        assert raw(g) == (OK, len(wpref.LOG_IDS))
        assert attach(n=nf - 1) == E_ARG and attach(n=nf + 1) == E_ARG, "n_states != num_final"
        bad = f.copy()
        bad[nf - 1] = -2
        assert attach(first=bad) == E_ARG and attach(cont=bad) == E_ARG, "an id of -2"
        bb = byte_ids.copy()
        bb[255] = -2
        assert attach(bytes_=bb) == E_ARG, "a byte id of -2"
        assert attach(unk=-1) == E_ARG, "unk_id of -1"
        assert attach(cap=0) == E_ARG and attach(cap=4096) == E_ARG, "max_word_bytes outside 1..4095"
        assert raw(g) == (OK, len(wpref.LOG_IDS)), "a refused attachment leaves the earlier one in force"
        assert attach(cap=4095) == OK and attach(cap=1) == OK and attach(bytes_=None) == OK
        assert attach() == OK
        d_in = torch.zeros(data.size + 64, dtype=torch.uint8, device="cuda:0")
        d_in[:data.size].copy_(torch.from_numpy(data.copy()))
        torch.cuda.synchronize()
        g.reserve(0, 0, 4096)
        g.scan_resident(data.size, data.size, d_input=d_in)
        n = C.c_uint64(7)
        assert L.pfac_records_filter_roles(g._ctx, 0, int(d_in.data_ptr()) + 8, None, C.byref(n)) == E_ARG, "misaligned d_input"
        assert L.pfac_records_filter_roles(g._ctx, 0, int(d_in.data_ptr()), int(g.records_ptr()) + 64, C.byref(n)) == E_ARG, "another heap"
        assert L.pfac_records_filter_roles(g._ctx, 0, int(d_in.data_ptr()), None, None) == E_ARG
        before = g.last_count()
        assert g.records_to_host(before).size == before, "a refused filter leaves the scan as it was"
        g.filter_roles(0, d_input=d_in)
        nd = len(wpref.LOG_TOK_OFF) - 1
        off = np.concatenate([[0], np.flatnonzero(data == 10) + 1]).astype(np.uint64)
        g.set_doc_offsets(off)
        n_sel = g.select_leftmost_longest_documents(nd)
        sel = g.doc_selection_to_host(n_sel, nd)[1]
        d_sel = torch.from_numpy(sel.view(np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        P = PFAC_TOKENS_POSITIONS
        full = dict(d_input=d_in, flags=P, d_ids=gd.ids.ptr, cap=gd.n, d_pos=gd.pos.ptr)
        docs = {"tok_off": gd.off.ptr}

        def refused(what, **kw):
            rc, _ = raw(g, **{**full, **kw})
            g.sync(0)
            assert rc == E_ARG, f"{what}: {passguard.STATUS.get(rc, rc)}"
            gd.untouched(what)
        refused("misaligned d_input", d_input=int(d_in.data_ptr()) + 8, docs=docs)
        refused("misaligned d_ids", d_ids=gd.ids.ptr + 4, docs=docs)
        refused("misaligned d_pos", d_pos=gd.pos.ptr + 8, docs=docs)
        refused("misaligned d_sel", d_sel=int(d_sel.data_ptr()) + 4, docs=docs)
        refused("misaligned d_tok_offsets", docs={"tok_off": gd.off.ptr + 4})
        refused("an unknown flag", flags=P | 2, docs=docs)
        refused("d_pos without the flag", flags=0)
        v = sel.copy()
        v[[1, 2]] = v[[2, 1]]
        d_bad = torch.from_numpy(v.view(np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        refused("two picks swapped", d_sel=d_bad, docs=docs)
        v = sel.copy()
        v["state"][1] = nf
        d_bad = torch.from_numpy(v.view(np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        refused("a state equal to num_final", d_sel=d_bad)
        rc, n = raw(g, **full, d_sel=d_sel, docs=docs)
        g.sync(0)
        assert (rc, n) == (OK, len(wpref.LOG_IDS))
        assert gd.ids.host().view(np.int32)[:n].tolist() == wpref.LOG_IDS
        assert gd.off.host().view(np.uint64).tolist() == wpref.LOG_TOK_OFF
        gd.ids.check(what="ids")
        gd.off.check(what="tok_off")


def test_a_document_offset_inside_a_word():
    table, first, cont, byte_ids = log_table()
    data = np.frombuffer(wpref.LOG, dtype=np.uint8)
    at = wpref.LOG.index(b"player") + 4                         # between "play" and "er": a piece boundary, not a word boundary
    gd = Guards(nd=3)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        attach_log(g, first, cont, byte_ids)
        for cut, status in ((at, E_ARG), (at + 2, OK), (at + 3, OK)):       # ... behind the word, behind its space
            g.scan_bytes(data)
            g.filter_roles(0)
            g.set_doc_offsets(np.array([0, cut, data.size - 1, data.size], dtype=np.uint64))
            g.select_leftmost_longest_documents(3)
            rc, n = raw(g, flags=PFAC_TOKENS_POSITIONS, d_ids=gd.ids.ptr, cap=gd.n, d_pos=gd.pos.ptr, docs={"tok_off": gd.off.ptr})
            g.sync(0)
            assert rc == status, f"an offset at {cut}: {passguard.STATUS.get(rc, rc)}"
            if status != OK:
                assert "inside a word" in g._L.pfac_last_error(g._ctx).decode()
                gd.untouched("the refused call")
                assert raw(g)[0] == OK, "the whole-stream call has no offsets to refuse"


def test_overflow_carries_the_exact_count():
    name = "docs-big"
    dev = device()
    nd = dev.prepare(name)
    n = int(want_of(name)[0].size)
    gd = Guards(n=n - 1, nd=nd)
    with pytest.raises(PfacError) as e:
        dev.g.wordpiece_selection_documents(d_ids=gd.ids.ptr, out_cap=n - 1, d_pos=gd.pos.ptr, d_tok_offsets=gd.off.ptr, d_input=dev.d_input(name))
    assert e.value.status == E_OVERFLOW and e.value.n_tokens == n
    dev.g.sync(0)
    gd.untouched("the overflow")
    with pytest.raises(PfacError) as e:                         # the positions alone are the caller's
        dev.g.wordpiece_selection(d_pos=gd.pos.ptr, out_cap=n - 1, d_input=dev.d_input(name))
    assert e.value.status == E_OVERFLOW and e.value.n_tokens == n
    gd.untouched("the overflow")


def test_lifetime_across_other_passes():
    """The attachment and the slot-owned result across a plain tokenize, a replace and a score pass; the result is ONE
    with the tokenizer's: the next tokenize pass replaces it."""
    table, first, cont, byte_ids = log_table()
    data = np.frombuffer(wpref.LOG, dtype=np.uint8)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        attach_log(g, first, cont, byte_ids)
        g.set_token_ids({k: 100 + k for k in range(1, 8)}, byte_base=1000)
        g.set_replacements([b"<>"] * 7)
        wp_scan(g, data)
        n = g.wordpiece_selection(positions=True)
        ids, pos = g.tokens_to_host(n, True)
        assert ids.tolist() == wpref.LOG_IDS
        g.replace_selection()
        g.set_pattern_weights(np.arange(8))
        g.set_doc_offsets(np.array([0, 10, data.size], dtype=np.uint64))
        g.document_scores(2)
        assert g.tokens_to_host(n).tolist() == wpref.LOG_IDS, "after a replace and a score pass"
        m = g.tokenize_selection()                              # the plain tokenizer over the same selection: its own ids
        plain = g.tokens_to_host(m)
        assert m != n or plain.tolist() != wpref.LOG_IDS
        assert g.wordpiece_selection() == n and g.tokens_to_host(n).tolist() == wpref.LOG_IDS, "the attachment outlives a plain tokenize"
        g.set_token_ids({1: 5})                                 # ... and new plain ids
        assert g.wordpiece_selection() == n
        rc, _ = raw(g, flags=2)
        assert rc == E_ARG
        with pytest.raises(PfacError) as e:
            g.tokens_to_host(n)
        assert e.value.status == E_STATE, "a refused call discards the earlier result"


# ---------------------------------------------------------------------------
# the surface

def test_surface_on_a_small_log():
    table, first, cont, byte_ids = log_table()
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        attach_log(g, first, cont, byte_ids)
        ids, tok_off = g.wordpiece_lines(wpref.LOG)
        assert ids.dtype == np.int32 and ids.tolist() == wpref.LOG_IDS and tok_off.tolist() == wpref.LOG_TOK_OFF
        ids, pos, tok_off = g.wordpiece_lines(wpref.LOG, positions=True)
        assert ids.tolist() == wpref.LOG_IDS and pos.tolist() == wpref.LOG_POS and tok_off.tolist() == wpref.LOG_TOK_OFF
        docs = [line + b"\n" for line in wpref.LOG.split(b"\n")[:-1]]
        ids, pos, tok_off = g.wordpiece_documents(docs, positions=True)
        assert ids.tolist() == wpref.LOG_IDS and pos.tolist() == wpref.LOG_POS and tok_off.tolist() == wpref.LOG_TOK_OFF
        ids, ex = g.wordpiece(wpref.LOG)
        assert ids.tolist() == wpref.LOG_IDS and ex == 0
        ids, pos, ex = g.wordpiece(wpref.LOG, positions=True)
        off = np.concatenate([[0], np.flatnonzero(np.frombuffer(wpref.LOG, dtype=np.uint8) == 10) + 1])
        assert pos.tolist() == (np.array(wpref.LOG_POS) + np.repeat(off[:-1], np.diff(wpref.LOG_TOK_OFF))).tolist()
        with pytest.raises(ValueError):
            g.wordpiece_lines(wpref.LOG, delimiter=b"e")
        with pytest.raises(PfacError) as e:                     # two documents that meet inside a word
            g.wordpiece_documents([b"pla", b"ying"])
        assert e.value.status == E_ARG
        # a cap of four bytes: "player", "plays", "unplaying" and "playx" are [UNK] by their length, "thes" is not
        attach_log(g, first, cont, byte_ids, max_word_bytes=4)
        assert g.wordpiece(wpref.LOG)[0].tolist() == [5, 0, 0, 9, 0, 10, 0, 5, 9, 5, 8]
        with pytest.raises(PfacError) as e:
            g.wordpiece_selection(d_ids=GuardedBuffer(0).ptr, out_cap=0)
        assert e.value.status == E_OVERFLOW and e.value.n_tokens == 11


def test_surface_folded_table():
    """Ids of the folded pieces, positions into the unfolded text."""
    table, first, cont, byte_ids, _ = wordpiece_table(wpref.LOG_VOCAB, ignore_case=True)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        attach_log(g, first, cont, byte_ids)
        ids, pos, _ = g.wordpiece(b"The PLAYer.\n", positions=True)
        assert ids.tolist() == [5, 2, 4, 9] and pos.tolist() == [0, 4, 8, 10]


def test_embedding_bag_takes_the_device_arrays():
    name = "docs-tiny"
    dev = device()
    nd = dev.prepare(name)
    want = want_of(name)
    n = int(want[0].size)
    d_ids = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_off = torch.zeros(nd + 1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert dev.g.wordpiece_selection_documents(d_input=dev.d_input(name), d_ids=d_ids, out_cap=n, d_tok_offsets=d_off) == n
    dev.g.sync(0)
    gen = torch.Generator().manual_seed(7)
    weight = torch.randn(int(want[0].max()) + 1, 8, generator=gen).to("cuda:0")
    got = torch.nn.functional.embedding_bag(d_ids, weight, d_off[:-1], mode="sum")
    ref_ids = torch.from_numpy(want[0].astype(np.int32)).to("cuda:0")
    ref_off = torch.from_numpy(want[2].astype(np.int64)).to("cuda:0")
    exp = torch.nn.functional.embedding_bag(ref_ids, weight, ref_off[:-1], mode="sum")
    assert tuple(got.shape) == (nd, 8) and torch.equal(got, exp)
    assert torch.equal(d_ids, ref_ids) and torch.equal(d_off, ref_off)
