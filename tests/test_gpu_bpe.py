"""Byte-level BPE on the GPU (run with -m gpu on an MI355X): pfac_table_set_bpe, pfac_bpe_records and pfac_bpe_documents
against tests/bperef.py, whose cases tests/test_bpe_ref.py holds against a second form of the rule (and a library) and
checks for their preconditions without a GPU.  Every named case runs through passguard.exact_call with guard bands of
exactly n_tokens x 4 (ids), n_tokens x 4 (positions) and (n_docs + 1) x 8 bytes, one below the capacity first, under
both fills.  Integer work: bit-exact.  No expectation comes from the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import bperef
import passguard
from bperef import DROP, case, check, names, want_of
from heapguard import FILLS, GuardedBuffer
from passguard import E_ARG, E_OVERFLOW, E_STATE, OK, TILE, Want, exact_call
from phfpfac_amd import BPE_PIECE_DTYPE, PFAC_TOKENS_POSITIONS, GpuMatcher, PfacError, bpe_table
from phfpfac_amd.matcher import _ptr

pytestmark = pytest.mark.gpu

KNOBS = {None: {}, 4: {"PFAC_REC_BYTES": "4"}, 8: {"PFAC_WIDE": "1"}}
_DEV = {}


def case_table(v):
    """The table of a case vocabulary as bpe_table builds it, and the pieces of the reference's own strings (state ->
    pattern line through the table's id map): the ids the case drops are DROP, any_split is the attachment's."""
    table, pieces, _, _ = bpe_table(v.vocab, v.merges, byte_level=False, lead=None if v.lead < 0 else v.lead,
                                    word_bytes=bytes(np.flatnonzero(v.word).astype(np.uint8)), ignore_case=v.fold)
    lines = list(v.strings)
    nf = int(table.num_final)
    lens = table.final_lengths()
    line_of = [int(i) - 1 for i in np.asarray(table.idmap)[:nf]]
    assert sorted(lines[ln] for s, ln in enumerate(line_of) if lens[s] >= 1) == sorted(lines)
    return table, line_of, lines, pieces


class BpeDevice:
    """One GpuMatcher with a case vocabulary's table, at record width W (None: the width the scan picks by itself, 2
    bytes for the small vocabulary and 4 for the others); `prepare(name)` leaves the case's scan as the slot's last,
    under the case's attachment."""

    def __init__(self, W, v):
        self.fold = v.fold
        self.table, self.line_of, self.lines, self.built = case_table(v)
        self.W = W or (2 if len(v.pieces) == bperef.N_SMALL else 4)
        self.g = GpuMatcher(0, 1)
        with passguard._Env(KNOBS[W]):
            self.g.load_table(self.table)
        self.lens = self.table.final_lengths()
        self.g.set_final_lengths(self.lens)
        self.inputs, self.attached = {}, None

    def close(self):
        self.g.close()

    def pieces_of(self, v):
        pc = np.zeros(int(self.table.num_final), dtype=BPE_PIECE_DTYPE)
        pc["id"] = DROP
        for s, ln in enumerate(self.line_of):
            if self.lens[s] >= 1:
                pc["id"][s], pc["rank"][s], pc["split"][s], _ = v.quad(self.lines[ln])
        return pc

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
        key = (id(v), byte_ids)
        if self.attached != key:
            self.g.set_bpe(self.pieces_of(v), None if byte_ids is None else v.byte_ids, v.lead, v.word_set(), v.max_word)
            self.attached = key

    def scan(self, name):
        data, no, _, _ = case(name)
        self.g.reserve(0, 0, 4 * data.size + 2 * TILE)          # (a lattice: more records than bytes)
        n = self.g.scan_resident(no, data.size, d_input=self.d_input(name))
        assert self.g.scan_format()[0] == self.W, f"record width {self.g.scan_format()[0]}, want {self.W}"
        return n

    def prepare(self, name, byte_ids="given"):
        """-> n_docs or None"""
        data, no, v, off = case(name)
        assert v.fold == self.fold
        self.attach(v, byte_ids)
        self.scan(name)
        if off is None:
            return None
        self.g.set_doc_offsets(off)
        return int(off.size) - 1

    def status(self, fn, attr=None):
        try:
            return OK, fn()
        except PfacError as e:
            return e.status, getattr(e, attr, None) if attr else None


def device(name, W=None):
    v = case(name)[2]
    key = (W, v.fold, tuple(v.pieces))
    if key not in _DEV:
        _DEV[key] = BpeDevice(W, v)
    return _DEV[key]


@pytest.fixture(scope="module", autouse=True)
def _close_devices():
    yield
    for d in _DEV.values():
        d.close()
    _DEV.clear()


def exact(name, fill, W=None, byte_ids="given", want=None, prepare=True):
    dev = device(name, W)
    nd = dev.prepare(name, byte_ids) if prepare else None      # (not prepared here: a whole-stream case, the scan as it stands)
    g, want = dev.g, want_of(name) if want is None else want
    n = int(want[0].size)
    buf = {"d_ids": GuardedBuffer(n * 4, fill=fill), "d_pos": GuardedBuffer(n * 4, fill=fill)}
    payloads = {"d_ids": want[0], "d_pos": want[1]}
    d_in = dev.d_input(name)
    if nd is None:
        def call(cap, bad=None):
            return dev.status(lambda: g.bpe_records(d_input=d_in, d_ids=buf["d_ids"].ptr, out_cap=cap, d_pos=buf["d_pos"].ptr), "n_tokens")
    else:
        buf["d_tok_offsets"] = GuardedBuffer((nd + 1) * 8, fill=fill)
        payloads["d_tok_offsets"] = want[2]

        def call(cap, bad=None):
            return dev.status(lambda: g.bpe_records_documents(nd, d_input=d_in, d_ids=buf["d_ids"].ptr, out_cap=cap, d_pos=buf["d_pos"].ptr,
                                                              d_tok_offsets=buf["d_tok_offsets"].ptr), "n_tokens")
    exact_call(g, call, Want(n, payloads), buf, fill, f"bpe case {name} ({n} tokens" + (f", {nd} documents)" if nd is not None else ")"))


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name", names())
def test_case_at_exact_capacity(name, fill):
    exact(name, fill)


WIDER = ["n1", "n4097", "t3", "t65", "split-any", "chain", "edge-lookback-un", "group-chain", "group-dense", "lead-tile-last",
         "lead-two", "cap255", "cap64-lead-over-edge", "docs-cut", "docs-tiny"]


@pytest.mark.parametrize("name,W", [(n, 8) for n in WIDER] + [(n, W) for n in names() if n.startswith("w2-") for W in (4, 8)])
def test_wider_records(name, W):
    """The 16-bit record form is the small vocabulary's own and the 32-bit form the others' (every named case runs at
    its own width above); here the small one at 4 and 8 bytes and the others at 8."""
    exact(name, FILLS[0], W)


def test_null_byte_ids_drop_every_byte():
    """NULL byte_ids are all-DROP byte_ids: the case whose vocabulary has none, attached with a NULL pointer."""
    assert (case("alldrop-bytes")[2].byte_ids == DROP).all()
    exact("alldrop-bytes", FILLS[0], byte_ids=None)


def test_a_scan_through_the_whole_word_filter_first():
    """The rule is taken over the records as they stand: here without those that start or end inside a run of word
    bytes, which leaves whole runs only -- no merge of two letters inside a longer word has a record then."""
    name = "t3"
    dev = device(name)
    data, no, v, _ = case(name)
    dev.prepare(name)
    pos, lens, idx = bperef.records(data, no, v)
    W = np.concatenate([[False], v.word[data], [False]])
    cut = W[:-1] & W[1:]                                        # cut[i]: a word byte on both sides of position i
    keep = ~cut[pos] & ~cut[pos + lens]
    assert 0 < keep.sum() < keep.size
    assert dev.g.filter_whole_words(0, bperef.CASE_WORD, d_input=dev.d_input(name)) == int(keep.sum())
    want = bperef.by_records(data, no, pos[keep], lens[keep], idx[keep], v)
    assert not np.array_equal(want[0], want_of(name)[0])
    exact(name, FILLS[0], want=want, prepare=False)


@pytest.mark.parametrize("name", ["n0", "n1", "t65", "w2-t65", "docs-emptygroup", "folded"])
def test_slot_owned_result_windows_and_the_same_call_twice(name):
    dev = device(name)
    nd = dev.prepare(name)
    g, want = dev.g, want_of(name)
    n = int(want[0].size)
    d_in = dev.d_input(name)

    def run(positions):
        return g.bpe_records(d_input=d_in, positions=positions) if nd is None else g.bpe_records_documents(nd, d_input=d_in, positions=positions)
    assert run(True) == n
    first = g.tokens_to_host(n, True)
    check(want, *first, tok_off=None if nd is None else g.token_offsets_to_host(nd), what=name)
    if n > 5:
        a, b = g.tokens_to_host(n - 5, True, first=3)
        assert np.array_equal(a, want[0][3:n - 2]) and np.array_equal(b, want[1][3:n - 2])
    assert run(True) == n                                       # the same call twice, byte for byte
    again = g.tokens_to_host(n, True)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    assert run(False) == n                                      # without the flag: ids only
    check(want, g.tokens_to_host(n), what=name)
    if n:
        assert dev.status(lambda: g.tokens_to_host(n, True))[0] == E_STATE, "the last call wrote no positions"


# ---------------------------------------------------------------------------
# the ladder of errors, through the C ABI as it is

def raw(g, d_input=None, d_records=None, flags=0, d_ids=None, cap=0, d_pos=None, docs=None):
    n = C.c_uint64(12345)
    if docs is None:
        rc = g._L.pfac_bpe_records(g._ctx, 0, _ptr(d_input), _ptr(d_records), int(flags), _ptr(d_ids), int(cap), _ptr(d_pos), C.byref(n))
    else:
        rc = g._L.pfac_bpe_documents(g._ctx, 0, _ptr(d_input), _ptr(d_records), _ptr(docs.get("off")), int(docs["n"]), int(flags),
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
    table, pieces, byte_ids, skipped = bpe_table({t: i for i, t in enumerate(bperef.LOG_TOKENS)}, bperef.LOG_MERGES)
    assert skipped == []
    return table, pieces, byte_ids


def attach_log(g, pieces, byte_ids, **kw):
    g.set_bpe(pieces, byte_ids, **kw)


LOG_DATA = np.frombuffer(bperef.LOG, dtype=np.uint8)
LOG_OFF = np.concatenate([[0], np.flatnonzero(LOG_DATA == 10) + 1]).astype(np.uint64)


def test_ladder_of_state_errors():
    table, pieces, bids = log_table()
    data = LOG_DATA
    nd = len(bperef.LOG_TOK_OFF) - 1
    gd = Guards(nd=nd)
    with GpuMatcher(0, 1) as g:
        def refused(what, status=E_STATE, **kw):
            rc, n = raw(g, flags=PFAC_TOKENS_POSITIONS, d_ids=gd.ids.ptr, cap=gd.n, d_pos=gd.pos.ptr, **kw)
            g.sync(0)
            assert rc == status, f"{what}: {passguard.STATUS.get(rc, rc)}"
            gd.untouched(what)
        refused("no table")
        refused("no table (documents)", docs={"n": nd, "tok_off": gd.off.ptr})
        rc = g._L.pfac_table_set_bpe(g._ctx, None, 0, None, None, 32, 64)
        assert rc == E_STATE, "the attachment before a table"
        g.load_table(table)
        refused("no scan")
        attach_log(g, pieces, bids)
        g.scan_bytes(data)
        g.load_table(table)
        attach_log(g, pieces, bids)
        refused("no final lengths")
        g.set_final_lengths(table.final_lengths())
        refused("a scan of an earlier table")
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.scan_bytes(data)
        refused("no attachment (an upload dropped it)")
        assert "pfac_table_set_bpe" in g._L.pfac_last_error(g._ctx).decode()
        g.set_token_ids({1: 1})
        refused("no attachment (plain token ids do not serve)")
        g.set_unigram(np.zeros((int(table.num_final), 4), dtype=np.int32), None, -10)
        refused("no attachment (a Unigram one does not serve)")
        attach_log(g, pieces, bids)
        assert raw(g) == (OK, len(bperef.LOG_IDS))
        g.set_doc_offsets(LOG_OFF)
        rc, n = raw(g, flags=PFAC_TOKENS_POSITIONS, d_ids=gd.ids.ptr, cap=gd.n, d_pos=gd.pos.ptr, docs={"n": nd, "tok_off": gd.off.ptr})
        g.sync(0)
        assert (rc, n) == (OK, len(bperef.LOG_IDS))
        assert gd.ids.host().view(np.int32)[:n].tolist() == bperef.LOG_IDS
        assert gd.off.host().view(np.uint64).tolist() == bperef.LOG_TOK_OFF
        gd.ids.check(what="ids")
        gd.off.check(what="tok_off")
        gd = Guards(nd=nd)                                      # (fresh ones: those hold a result now)
        # an overflowed heap
        heap = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        g.h2d(data)
        g.scan_async(data.size, d_records=heap, capacity=8)
        assert g.scan_finish(allow_overflow=True)[1], "the scan overflows a heap of eight records"
        refused("an overflowed heap", d_records=heap)
        g.scan_bytes(data)
        assert raw(g)[0] == OK
        g.reserve(0, 1 << 20, 1 << 16)
        refused("a reserve that replaced a buffer")


def test_ladder_of_argument_errors():
    table, pieces, bids = log_table()
    data = LOG_DATA
    nf = int(table.num_final)
    nd = len(bperef.LOG_TOK_OFF) - 1
    gd = Guards(nd=nd)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        L = g._L
        ws = bperef.Vocab({}, [], word=bperef.DEFAULT_WORD).word_set()
        pc = pieces.copy()
        bb = bids.copy()

        def attach(p=pc, n=nf, bytes_=bb, words=ws, lead=32, cap=64):
            return L.pfac_table_set_bpe(g._ctx, p.ctypes.data, n, None if bytes_ is None else bytes_.ctypes.data,
                                        None if words is None else words.ctypes.data, lead, cap)
        assert attach() == OK
        g.scan_bytes(data)
        assert raw(g) == (OK, len(bperef.LOG_IDS))
        assert attach(n=nf - 1) == E_ARG and attach(n=nf + 1) == E_ARG, "n_states != num_final"
        for field, value in (("id", -2), ("rank", -1), ("reserved", 1)):
            bad = pc.copy()
            bad[field][nf - 1] = value
            assert attach(p=bad) == E_ARG, f"{field} of {value}"
        big = pc.copy()
        big["split"][:] = 0xFFFFFFFF                            # a split >= L_s can never apply and is not an error
        assert attach(p=big) == OK
        assert raw(g) == (OK, LOG_DATA.size), "no merge applies: one token per byte"
        bad = bb.copy()
        bad[255] = -2
        assert attach(bytes_=bad) == E_ARG, "a byte id of -2"
        assert attach(cap=0) == E_ARG and attach(cap=256) == E_ARG, "max_word_bytes outside 1..255"
        assert attach(lead=-2) == E_ARG and attach(lead=256) == E_ARG, "lead outside -1..255"
        assert attach(lead=ord("a")) == E_ARG, "a lead that is a word byte"
        assert raw(g) == (OK, LOG_DATA.size), "a refused attachment leaves the earlier one in force"
        assert attach() == OK
        assert raw(g) == (OK, len(bperef.LOG_IDS))
        assert attach(lead=-1) == OK and attach(cap=1) == OK and attach(cap=255) == OK and attach(words=None) == OK and attach() == OK
        d_in = torch.zeros(data.size + 64, dtype=torch.uint8, device="cuda:0")
        d_in[:data.size].copy_(torch.from_numpy(data.copy()))
        d_off = torch.from_numpy(LOG_OFF.view(np.int64).copy()).to("cuda:0")
        torch.cuda.synchronize()
        g.reserve(0, 0, 4096)
        g.scan_resident(data.size, data.size, d_input=d_in)
        P = PFAC_TOKENS_POSITIONS
        full = dict(d_input=d_in, flags=P, d_ids=gd.ids.ptr, cap=gd.n, d_pos=gd.pos.ptr)
        docs = {"n": nd, "off": d_off, "tok_off": gd.off.ptr}

        def refused(what, **kw):
            rc, _ = raw(g, **{**full, **kw})
            g.sync(0)
            assert rc == E_ARG, f"{what}: {passguard.STATUS.get(rc, rc)}"
            gd.untouched(what)
        refused("misaligned d_input", d_input=int(d_in.data_ptr()) + 8, docs=docs)
        refused("misaligned d_ids", d_ids=gd.ids.ptr + 4, docs=docs)
        refused("misaligned d_pos", d_pos=gd.pos.ptr + 8, docs=docs)
        refused("misaligned d_tok_offsets", docs={**docs, "tok_off": gd.off.ptr + 4})
        refused("misaligned d_doc_offsets", docs={**docs, "off": int(d_off.data_ptr()) + 4})
        refused("another heap", d_records=int(g.records_ptr()) + 64)
        refused("an unknown flag", flags=P | 2, docs=docs)
        refused("d_pos without the flag", flags=0)
        # "the player": inside the run, between the lead and its run, in front of the lead, behind the run
        at = bperef.LOG.index(b" player")
        for cut, status in ((at + 3, E_ARG), (at + 1, E_ARG), (at, OK), (at + 7, OK)):
            o = torch.tensor([0, cut, data.size - 1, data.size], dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            if status != OK:
                refused(f"an offset inside a word ({cut})", docs={"n": 3, "off": o, "tok_off": gd.off.ptr})
                assert "inside a word" in L.pfac_last_error(g._ctx).decode()
            else:
                rc, _ = raw(g, **full, docs={"n": 3, "off": o, "tok_off": gd.off.ptr})
                g.sync(0)
                assert rc == OK, f"an offset at {cut}"
        assert attach(lead=-1) == OK                            # without a lead the same offset is a boundary
        o = torch.tensor([0, at + 1, data.size - 1, data.size], dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        rc, _ = raw(g, **full, docs={"n": 3, "off": o, "tok_off": gd.off.ptr})
        g.sync(0)
        assert rc == OK and attach() == OK
        o = torch.tensor([0, 30, 18, data.size], dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        gd = Guards(nd=nd)
        refused("offsets that decrease", docs={"n": 3, "off": o, "tok_off": gd.off.ptr})
        rc, n = raw(g, **{**full, "d_ids": gd.ids.ptr, "d_pos": gd.pos.ptr}, docs={**docs, "tok_off": gd.off.ptr})
        g.sync(0)
        assert (rc, n) == (OK, len(bperef.LOG_IDS))
        assert gd.ids.host().view(np.int32)[:n].tolist() == bperef.LOG_IDS
        assert gd.off.host().view(np.uint64).tolist() == bperef.LOG_TOK_OFF
        gd.ids.check(what="ids")
        gd.off.check(what="tok_off")


def test_offsets_rule_with_nothing_owned():
    """n_owned == 0: no tile runs, the offsets rule still holds (every offset is 0)."""
    dev = device("n0")
    dev.prepare("n0")
    g = dev.g
    gd = Guards(n=4, nd=2)
    for offs, status in (([0, 0, 5], E_ARG), ([0, 1, 0], E_ARG), ([1, 0, 0], E_ARG), ([0, 0, 0], OK)):
        o = torch.tensor(offs, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        rc, n = raw(g, d_input=dev.d_input("n0"), d_ids=gd.ids.ptr, cap=gd.n, docs={"n": 2, "off": o, "tok_off": gd.off.ptr})
        g.sync(0)
        assert rc == status, f"offsets {offs}: {passguard.STATUS.get(rc, rc)}"
        if status != OK:
            gd.untouched(f"offsets {offs}")
    assert n == 0 and gd.off.host().view(np.uint64).tolist() == [0, 0, 0]
    gd.off.check(what="tok_off")
    gd.ids.check(payload_untouched=True, what="ids")


def test_overflow_carries_the_exact_count():
    name = "docs-big"
    dev = device(name)
    nd = dev.prepare(name)
    n = int(want_of(name)[0].size)
    gd = Guards(n=n - 1, nd=nd)
    with pytest.raises(PfacError) as e:
        dev.g.bpe_records_documents(nd, d_ids=gd.ids.ptr, out_cap=n - 1, d_pos=gd.pos.ptr, d_tok_offsets=gd.off.ptr, d_input=dev.d_input(name))
    assert e.value.status == E_OVERFLOW and e.value.n_tokens == n
    dev.g.sync(0)
    gd.untouched("the overflow")
    with pytest.raises(PfacError) as e:                         # the positions alone are the caller's
        dev.g.bpe_records(d_pos=gd.pos.ptr, out_cap=n - 1, d_input=dev.d_input(name))
    assert e.value.status == E_OVERFLOW and e.value.n_tokens == n
    gd.untouched("the overflow")


def test_lifetime_across_other_passes():
    """The attachment across a plain tokenize, a WordPiece pass, a Unigram pass and a replace; the slot-owned result is
    ONE with the tokenizer's: the next token pass replaces it, and a new attachment makes it stale."""
    table, pieces, bids = log_table()
    data = LOG_DATA
    nf = int(table.num_final)
    ug = np.zeros((nf, 4), dtype=np.int32)
    ug[:, 0], ug[:, 1], ug[:, 2], ug[:, 3] = 50 + np.arange(nf), 70 + np.arange(nf), -1, -1
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        attach_log(g, pieces, bids)
        g.set_token_ids({k: 100 + k for k in range(1, 8)}, byte_base=1000)
        g.set_replacements([b"<>"] * len(bperef.LOG_MERGES))    # (one per pattern)
        g.set_wordpiece(ug[:, 0], ug[:, 1], None, unk_id=0, word_bytes=bperef.DEFAULT_WORD)
        g.set_unigram(ug, None, -10, unk_id=0)
        g.scan_bytes(data)
        n = g.bpe_records(positions=True)
        ids, pos = g.tokens_to_host(n, True)
        assert ids.tolist() == bperef.LOG_IDS
        g.select_leftmost_longest(0)
        g.replace_selection()
        assert g.tokens_to_host(n).tolist() == bperef.LOG_IDS, "after a selection and a replace"
        m = g.tokenize_selection()                              # the plain tokenizer: its own ids, the ONE result
        assert m != n or g.tokens_to_host(m).tolist() != bperef.LOG_IDS
        assert g.bpe_records() == n and g.tokens_to_host(n).tolist() == bperef.LOG_IDS, "the attachment outlives a plain tokenize"
        m = g.unigram_records()                                 # a Unigram pass: its own ids, the ONE result
        assert m != n or g.tokens_to_host(m).tolist() != bperef.LOG_IDS
        g.set_unigram(ug, None, -10, unk_id=0)                  # a new Unigram attachment makes ITS result stale ...
        with pytest.raises(PfacError) as e:
            g.tokens_to_host(m)
        assert e.value.status == E_STATE
        assert g.bpe_records() == n and g.tokens_to_host(n).tolist() == bperef.LOG_IDS, "... and leaves the BPE attachment alone"
        g.set_unigram(ug, None, -10, unk_id=0)                  # ... and a BPE result is not the Unigram attachment's
        assert g.tokens_to_host(n).tolist() == bperef.LOG_IDS
        g.scan_bytes(data)
        g.filter_roles(0)
        g.select_leftmost_longest(0)
        g.wordpiece_selection()                                 # a WordPiece pass (over the filtered records)
        g.scan_bytes(data)
        assert g.bpe_records() == n and g.tokens_to_host(n).tolist() == bperef.LOG_IDS, "... and a WordPiece pass"
        attach_log(g, pieces, bids)                             # the same pieces again are a new attachment
        with pytest.raises(PfacError) as e:
            g.tokens_to_host(n)
        assert e.value.status == E_STATE, "a result made under the earlier attachment is stale"
        assert g.bpe_records() == n and g.tokens_to_host(n).tolist() == bperef.LOG_IDS
        m = g.unigram_records()
        attach_log(g, pieces, bids)                             # a new BPE attachment leaves a Unigram result alone
        assert g.tokens_to_host(m).size == m
        assert g.bpe_records() == n
        rc, _ = raw(g, flags=2)
        assert rc == E_ARG
        with pytest.raises(PfacError) as e:
            g.tokens_to_host(n)
        assert e.value.status == E_STATE, "a refused call discards the earlier result"


# ---------------------------------------------------------------------------
# the surface

def log_vocab(max_word=64, lead=0x20):
    from phfpfac_amd import bpe_byte_alphabet
    back = {c: b for b, c in bpe_byte_alphabet().items()}
    enc = lambda t: bytes(back[c] for c in t)                   # noqa: E731
    return bperef.Vocab({enc(t): i for i, t in enumerate(bperef.LOG_TOKENS)}, [(enc(l), enc(r)) for l, r in bperef.LOG_MERGES],
                        lead=lead, max_word=max_word, word=bperef.DEFAULT_WORD)


def test_surface_on_a_small_log():
    table, pieces, bids = log_table()
    LOG = bperef.LOG
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        attach_log(g, pieces, bids)
        ids, tok_off = g.bpe_lines(LOG)
        assert ids.dtype == np.int32 and ids.tolist() == bperef.LOG_IDS and tok_off.tolist() == bperef.LOG_TOK_OFF
        ids, pos, tok_off = g.bpe_lines(LOG, positions=True)
        assert ids.tolist() == bperef.LOG_IDS and pos.tolist() == bperef.LOG_POS and tok_off.tolist() == bperef.LOG_TOK_OFF
        docs = [line + b"\n" for line in LOG.split(b"\n")[:-1]]
        ids, pos, tok_off = g.bpe_documents(docs, positions=True)
        assert ids.tolist() == bperef.LOG_IDS and pos.tolist() == bperef.LOG_POS and tok_off.tolist() == bperef.LOG_TOK_OFF
        assert g.bpe(LOG).tolist() == bperef.LOG_IDS
        ids, pos = g.bpe(LOG, positions=True)
        assert pos.tolist() == (np.array(bperef.LOG_POS) + np.repeat(LOG_OFF[:-1].astype(np.int64), np.diff(bperef.LOG_TOK_OFF))).tolist()
        for delimiter in (b"e", b" "):                          # a word byte; the lead
            with pytest.raises(ValueError):
                g.bpe_lines(LOG, delimiter=delimiter)
        for pair in ([b"pla", b"ying"], [b"the ", b"play"]):    # two documents that meet inside a word; between a lead and its run
            with pytest.raises(PfacError) as e:
                g.bpe_documents(pair)
            assert e.value.status == E_ARG
        assert g.bpe_documents([b"the", b" play"])[0].tolist() == [14, 19]
        # a cap of four bytes: " player" and " plays." stay single bytes; no lead: the spaces stand alone
        for kw in ({"max_word_bytes": 4}, {"lead": None}, {"lead": -1, "max_word_bytes": 3}):
            attach_log(g, pieces, bids, **kw)
            v = log_vocab(kw.get("max_word_bytes", 64), -1 if "lead" in kw else 0x20)
            want = bperef.by_strings(LOG_DATA, LOG_DATA.size, v)
            got = g.bpe(LOG, positions=True)
            assert not np.array_equal(want[0], np.array(bperef.LOG_IDS))
            check(want, *got, what=f"the log under {kw}")
        with pytest.raises(PfacError) as e:
            g.bpe_records(d_ids=GuardedBuffer(0).ptr, out_cap=0)
        assert e.value.status == E_OVERFLOW and e.value.n_tokens == int(want[0].size)


def test_surface_folded_table():
    """Ids of the folded strings, positions into the unfolded text, byte ids of the bytes as written."""
    voc = {t: i for i, t in enumerate(bperef.LOG_TOKENS)}
    voc.update({"T": 40, "X": 41, "P": 42})
    table, pieces, bids, _ = bpe_table(voc, bperef.LOG_MERGES, ignore_case=True)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_bpe(pieces, bids)
        ids, pos = g.bpe(b"The PLAYer aX.\n", positions=True)
        assert ids.tolist() == [14, 19, 20, 21, 41, 10, 12] and pos.tolist() == [0, 3, 8, 10, 12, 13, 14]
        ids = g.bpe(b"T Pl")                                    # a single byte keeps the id of the byte as written
        assert ids.tolist() == [40, 11, 17]


def test_embedding_bag_takes_the_device_arrays():
    name = "docs-tiny"
    dev = device(name)
    nd = dev.prepare(name)
    want = want_of(name)
    n = int(want[0].size)
    d_ids = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_off = torch.zeros(nd + 1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert dev.g.bpe_records_documents(nd, d_input=dev.d_input(name), d_ids=d_ids, out_cap=n, d_tok_offsets=d_off) == n
    dev.g.sync(0)
    gen = torch.Generator().manual_seed(7)
    weight = torch.randn(int(want[0].max()) + 1, 8, generator=gen).to("cuda:0")
    got = torch.nn.functional.embedding_bag(d_ids, weight, d_off[:-1], mode="sum")
    ref_ids = torch.from_numpy(want[0].astype(np.int32)).to("cuda:0")
    ref_off = torch.from_numpy(want[2].astype(np.int64)).to("cuda:0")
    exp = torch.nn.functional.embedding_bag(ref_ids, weight, ref_off[:-1], mode="sum")
    assert tuple(got.shape) == (nd, 8) and torch.equal(got, exp)
    assert torch.equal(d_ids, ref_ids) and torch.equal(d_off, ref_off)
