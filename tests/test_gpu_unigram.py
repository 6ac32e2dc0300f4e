"""Unigram on the GPU (run with -m gpu on an MI355X): pfac_table_set_unigram, pfac_unigram_records and
pfac_unigram_documents against tests/uniref.py, whose cases tests/test_unigram_ref.py holds against a second form of
the rule (and a library) and checks for their preconditions without a GPU.  Every named case runs through
passguard.exact_call with guard bands of exactly n_tokens x 4 (ids), n_tokens x 4 (positions) and (n_docs + 1) x 8
bytes, one below the capacity first, under both fills.  Integer work: bit-exact.  No expectation comes from the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import passguard
import uniref
from heapguard import FILLS, GuardedBuffer
from passguard import E_ARG, E_OVERFLOW, E_STATE, OK, TILE, Want, exact_call
from phfpfac_amd import PFAC_TOKENS_POSITIONS, GpuMatcher, PfacError, unigram_table
from phfpfac_amd.matcher import _ptr
from uniref import DROP, case, check, names, want_of

pytestmark = pytest.mark.gpu

KNOBS = {None: {}, 4: {"PFAC_REC_BYTES": "4"}, 8: {"PFAC_WIDE": "1"}}
_DEV = {}


def case_table(entries=None, fold=False):
    entries = uniref.ENTRIES if entries is None else entries
    return unigram_table([(e, float(s)) for e, s in entries], word_bytes=uniref.CASE_WORD, scale=1.0, ignore_case=fold)


class UgDevice:
    """One GpuMatcher with a case vocabulary as unigram_table builds it, at record width W (None: the width the scan
    picks by itself, 2 bytes for the small vocabulary and 4 for the other); `prepare(name)` leaves the case's scan as
    the slot's last, under the case's attachment."""

    def __init__(self, W, fold, entries):
        self.fold = fold
        self.table, self.pieces, _, _ = case_table(entries, fold)
        self.W = W or (2 if len(entries) == len(uniref.SMALL_ENTRIES) else 4)
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
        key = (v.max_word, v.unk, v.byte_score, tuple(v.byte_ids.tolist()), byte_ids)
        if self.attached != key:
            self.g.set_unigram(self.pieces, None if byte_ids is None else v.byte_ids, v.byte_score, v.unk, v.word_set(), v.max_word)
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
    key = (W, v.fold, len(v.entries))
    if key not in _DEV:
        _DEV[key] = UgDevice(W, v.fold, v.entries)
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
            return dev.status(lambda: g.unigram_records(d_input=d_in, d_ids=buf["d_ids"].ptr, out_cap=cap, d_pos=buf["d_pos"].ptr), "n_tokens")
    else:
        buf["d_tok_offsets"] = GuardedBuffer((nd + 1) * 8, fill=fill)
        payloads["d_tok_offsets"] = want[2]

        def call(cap, bad=None):
            return dev.status(lambda: g.unigram_records_documents(nd, d_input=d_in, d_ids=buf["d_ids"].ptr, out_cap=cap, d_pos=buf["d_pos"].ptr,
                                                                  d_tok_offsets=buf["d_tok_offsets"].ptr), "n_tokens")
    exact_call(g, call, Want(n, payloads), buf, fill, f"unigram case {name} ({n} tokens" + (f", {nd} documents)" if nd is not None else ")"))


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name", names())
def test_case_at_exact_capacity(name, fill):
    exact(name, fill)


WIDER = ["n17", "n4097", "t3", "t65", "edge-lookback-un", "group-piece-across", "group-dense", "cap4095", "three-tiles-fallback",
         "docs-cut", "docs-tiny"]


@pytest.mark.parametrize("name,W", [(n, 8) for n in WIDER] + [(n, W) for n in names() if n.startswith("w2-") for W in (4, 8)])
def test_wider_records(name, W):
    """The 16-bit record form is the small vocabulary's own and the 32-bit form the other's (every named case runs at
    its own width above); here the small one at 4 and 8 bytes and the other at 8."""
    exact(name, FILLS[0], W)


def test_null_byte_ids_drop_every_byte():
    """NULL byte_ids are all-DROP byte_ids: the case whose vocabulary has none, attached with a NULL pointer."""
    assert (case("alldrop-bytes")[2].byte_ids == DROP).all()
    exact("alldrop-bytes", FILLS[0], byte_ids=None)


def test_a_scan_through_the_whole_word_filter_first():
    """The rule is taken over the records as they stand: here without those that start or end inside a word, which
    leaves whole words only -- "playing" has no edge but the byte edges then."""
    name = "t3"
    dev = device(name)
    data, no, v, _ = case(name)
    dev.prepare(name)
    pos, lens, idx = uniref.records(data, no, v)
    W = np.concatenate([[False], v.word[data], [False]])
    cut = W[:-1] & W[1:]                                        # cut[i]: a word byte on both sides of position i
    keep = ~cut[pos] & ~cut[pos + lens]
    assert 0 < keep.sum() < keep.size
    assert dev.g.filter_whole_words(0, uniref.CASE_WORD, d_input=dev.d_input(name)) == int(keep.sum())
    want = uniref.by_records(data, no, pos[keep], lens[keep], idx[keep], v)
    assert not np.array_equal(want[0], want_of(name)[0])
    exact(name, FILLS[0], want=want, prepare=False)


@pytest.mark.parametrize("name", ["n0", "n17", "t65", "w2-t65", "docs-emptygroup", "folded"])
def test_slot_owned_result_windows_and_the_same_call_twice(name):
    dev = device(name)
    nd = dev.prepare(name)
    g, want = dev.g, want_of(name)
    n = int(want[0].size)
    d_in = dev.d_input(name)

    def run(positions):
        return g.unigram_records(d_input=d_in, positions=positions) if nd is None else g.unigram_records_documents(nd, d_input=d_in, positions=positions)
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
        rc = g._L.pfac_unigram_records(g._ctx, 0, _ptr(d_input), _ptr(d_records), int(flags), _ptr(d_ids), int(cap), _ptr(d_pos), C.byref(n))
    else:
        rc = g._L.pfac_unigram_documents(g._ctx, 0, _ptr(d_input), _ptr(d_records), _ptr(docs.get("off")), int(docs["n"]), int(flags),
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
    table, pieces, scale, _ = unigram_table(uniref.LOG_VOCAB)
    return table, pieces, int(-10 * scale)


def attach_log(g, pieces, bscore, **kw):
    g.set_unigram(pieces, None, bscore, unk_id=0, **kw)


LOG_DATA = np.frombuffer(uniref.LOG, dtype=np.uint8)
LOG_OFF = np.concatenate([[0], np.flatnonzero(LOG_DATA == 10) + 1]).astype(np.uint64)


def test_ladder_of_state_errors():
    table, pieces, bscore = log_table()
    data = LOG_DATA
    nd = len(uniref.LOG_TOK_OFF) - 1
    gd = Guards(nd=nd)
    with GpuMatcher(0, 1) as g:
        def refused(what, status=E_STATE, **kw):
            rc, n = raw(g, flags=PFAC_TOKENS_POSITIONS, d_ids=gd.ids.ptr, cap=gd.n, d_pos=gd.pos.ptr, **kw)
            g.sync(0)
            assert rc == status, f"{what}: {passguard.STATUS.get(rc, rc)}"
            gd.untouched(what)
        refused("no table")
        refused("no table (documents)", docs={"n": nd, "tok_off": gd.off.ptr})
        rc = g._L.pfac_table_set_unigram(g._ctx, None, 0, None, 0, 0, None, 100)
        assert rc == E_STATE, "the attachment before a table"
        g.load_table(table)
        refused("no scan")
        attach_log(g, pieces, bscore)
        g.scan_bytes(data)
        g.load_table(table)
        attach_log(g, pieces, bscore)
        refused("no final lengths")
        g.set_final_lengths(table.final_lengths())
        refused("a scan of an earlier table")
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.scan_bytes(data)
        refused("no attachment (an upload dropped it)")
        assert "pfac_table_set_unigram" in g._L.pfac_last_error(g._ctx).decode()
        g.set_token_ids({1: 1})
        refused("no attachment (plain token ids do not serve)")
        attach_log(g, pieces, bscore)
        assert raw(g) == (OK, len(uniref.LOG_IDS))
        g.set_doc_offsets(LOG_OFF)
        rc, n = raw(g, flags=PFAC_TOKENS_POSITIONS, d_ids=gd.ids.ptr, cap=gd.n, d_pos=gd.pos.ptr, docs={"n": nd, "tok_off": gd.off.ptr})
        g.sync(0)
        assert (rc, n) == (OK, len(uniref.LOG_IDS))
        assert gd.ids.host().view(np.int32)[:n].tolist() == uniref.LOG_IDS
        assert gd.off.host().view(np.uint64).tolist() == uniref.LOG_TOK_OFF
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
    table, pieces, bscore = log_table()
    data = LOG_DATA
    nf = int(table.num_final)
    nd = len(uniref.LOG_TOK_OFF) - 1
    gd = Guards(nd=nd)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        L = g._L
        ws = uniref.Vocab([(b"a", -1)]).word_set()
        pc = pieces.copy()

        def attach(p=pc, n=nf, bytes_=None, bs=bscore, unk=0, cap=100):
            return L.pfac_table_set_unigram(g._ctx, p.ctypes.data, n, None if bytes_ is None else bytes_.ctypes.data, bs, unk, ws.ctypes.data, cap)
        assert attach() == OK
        g.scan_bytes(data)
        assert raw(g) == (OK, len(uniref.LOG_IDS))
        assert attach(n=nf - 1) == E_ARG and attach(n=nf + 1) == E_ARG, "n_states != num_final"
        for field in ("first_id", "cont_id"):
            bad = pc.copy()
            bad[field][nf - 1] = -2
            assert attach(p=bad) == E_ARG, "an id of -2"
        bb = np.full(256, DROP, dtype=np.int32)
        bb[255] = -2
        assert attach(bytes_=bb) == E_ARG, "a byte id of -2"
        assert attach(unk=-2) == E_ARG, "unk_id of -2"
        assert attach(cap=0) == E_ARG and attach(cap=4096) == E_ARG, "max_word_bytes outside 1..4095"
        # |score| * (max_word_bytes + 1) < 2^31: 2^31 / 101 = 21262214.7
        for field in ("first_score", "cont_score"):
            bad = pc.copy()
            bad[field][0] = -21262215
            assert attach(p=bad) == E_ARG, "a score over the bound"
            bad[field][0] = 21262214
            assert attach(p=bad) == OK, "a score at the bound"
        assert attach() == OK
        assert attach(bs=-21262215) == E_ARG and attach(bs=-21262214) == OK, "byte_score at the bound"
        assert attach(cap=4095, bs=-(2**19)) == E_ARG and attach(cap=4095, bs=-(2**19) + 1) == OK
        assert attach() == OK
        assert raw(g) == (OK, len(uniref.LOG_IDS)), "a refused attachment leaves the earlier one in force"
        assert attach(unk=DROP) == OK and attach(cap=1) == OK and attach() == OK
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
        at = uniref.LOG.index(b"player") + 4                    # between "play" and "er": a piece boundary, not a word boundary
        for cut, status in ((at, E_ARG), (at + 2, OK), (at + 3, OK)):
            o = torch.tensor([0, cut, data.size - 1, data.size], dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            rc, _ = raw(g, **full, docs={"n": 3, "off": o, "tok_off": gd.off.ptr}) if status == OK else (None, None)
            if status != OK:
                refused(f"an offset inside a word ({cut})", docs={"n": 3, "off": o, "tok_off": gd.off.ptr})
                assert "inside a word" in L.pfac_last_error(g._ctx).decode()
            else:
                g.sync(0)
                assert rc == OK, f"an offset at {cut}"
        o = torch.tensor([0, 30, 18, data.size], dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        gd = Guards(nd=nd)
        refused("offsets that decrease", docs={"n": 3, "off": o, "tok_off": gd.off.ptr})
        rc, n = raw(g, **{**full, "d_ids": gd.ids.ptr, "d_pos": gd.pos.ptr}, docs={**docs, "tok_off": gd.off.ptr})
        g.sync(0)
        assert (rc, n) == (OK, len(uniref.LOG_IDS))
        assert gd.ids.host().view(np.int32)[:n].tolist() == uniref.LOG_IDS
        assert gd.off.host().view(np.uint64).tolist() == uniref.LOG_TOK_OFF
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
        dev.g.unigram_records_documents(nd, d_ids=gd.ids.ptr, out_cap=n - 1, d_pos=gd.pos.ptr, d_tok_offsets=gd.off.ptr, d_input=dev.d_input(name))
    assert e.value.status == E_OVERFLOW and e.value.n_tokens == n
    dev.g.sync(0)
    gd.untouched("the overflow")
    with pytest.raises(PfacError) as e:                         # the positions alone are the caller's
        dev.g.unigram_records(d_pos=gd.pos.ptr, out_cap=n - 1, d_input=dev.d_input(name))
    assert e.value.status == E_OVERFLOW and e.value.n_tokens == n
    gd.untouched("the overflow")


def test_lifetime_across_other_passes():
    """The attachment across a plain tokenize, a WordPiece pass and a replace; the slot-owned result is ONE with the
    tokenizer's: the next token pass replaces it, and a new attachment makes it stale."""
    from phfpfac_amd import wordpiece_table
    table, pieces, bscore = log_table()
    data = LOG_DATA
    nf = int(table.num_final)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        attach_log(g, pieces, bscore)
        g.set_token_ids({k: 100 + k for k in range(1, 8)}, byte_base=1000)
        g.set_replacements([b"<>"] * 11)                        # (one per distinct stripped piece)
        g.set_wordpiece(pieces["first_id"], pieces["cont_id"], None, unk_id=0, word_bytes=uniref.DEFAULT_WORD)
        g.scan_bytes(data)
        n = g.unigram_records(positions=True)
        ids, pos = g.tokens_to_host(n, True)
        assert ids.tolist() == uniref.LOG_IDS
        g.select_leftmost_longest(0)
        g.replace_selection()
        assert g.tokens_to_host(n).tolist() == uniref.LOG_IDS, "after a selection and a replace"
        m = g.tokenize_selection()                              # the plain tokenizer: its own ids, the ONE result
        assert m != n or g.tokens_to_host(m).tolist() != uniref.LOG_IDS
        assert g.unigram_records() == n and g.tokens_to_host(n).tolist() == uniref.LOG_IDS, "the attachment outlives a plain tokenize"
        g.scan_bytes(data)
        g.filter_roles(0)
        g.select_leftmost_longest(0)
        g.wordpiece_selection()                                 # a WordPiece pass (over the filtered records)
        g.scan_bytes(data)
        assert g.unigram_records() == n and g.tokens_to_host(n).tolist() == uniref.LOG_IDS, "... and a WordPiece pass"
        attach_log(g, pieces, bscore)                           # the same pieces again are a new attachment
        with pytest.raises(PfacError) as e:
            g.tokens_to_host(n)
        assert e.value.status == E_STATE, "a result made under the earlier attachment is stale"
        assert g.unigram_records() == n and g.tokens_to_host(n).tolist() == uniref.LOG_IDS
        rc, _ = raw(g, flags=2)
        assert rc == E_ARG
        with pytest.raises(PfacError) as e:
            g.tokens_to_host(n)
        assert e.value.status == E_STATE, "a refused call discards the earlier result"


# ---------------------------------------------------------------------------
# the surface

def test_surface_on_a_small_log():
    table, pieces, bscore = log_table()
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        attach_log(g, pieces, bscore)
        ids, tok_off = g.unigram_lines(uniref.LOG)
        assert ids.dtype == np.int32 and ids.tolist() == uniref.LOG_IDS and tok_off.tolist() == uniref.LOG_TOK_OFF
        ids, pos, tok_off = g.unigram_lines(uniref.LOG, positions=True)
        assert ids.tolist() == uniref.LOG_IDS and pos.tolist() == uniref.LOG_POS and tok_off.tolist() == uniref.LOG_TOK_OFF
        docs = [line + b"\n" for line in uniref.LOG.split(b"\n")[:-1]]
        ids, pos, tok_off = g.unigram_documents(docs, positions=True)
        assert ids.tolist() == uniref.LOG_IDS and pos.tolist() == uniref.LOG_POS and tok_off.tolist() == uniref.LOG_TOK_OFF
        assert g.unigram(uniref.LOG).tolist() == uniref.LOG_IDS
        ids, pos = g.unigram(uniref.LOG, positions=True)
        assert pos.tolist() == (np.array(uniref.LOG_POS) + np.repeat(LOG_OFF[:-1].astype(np.int64), np.diff(uniref.LOG_TOK_OFF))).tolist()
        # the greedy cut of the same vocabulary differs: "abc" is "▁ab c" there
        assert 10 not in uniref.LOG_IDS and 12 in uniref.LOG_IDS
        with pytest.raises(ValueError):
            g.unigram_lines(uniref.LOG, delimiter=b"e")
        with pytest.raises(PfacError) as e:                     # two documents that meet inside a word
            g.unigram_documents([b"pla", b"ying"])
        assert e.value.status == E_ARG
        # a cap of four bytes: "player", "plays.", "unplaying" and "playx" have no piece edges: one unk each
        attach_log(g, pieces, bscore, max_word_bytes=4)
        assert g.unigram(uniref.LOG).tolist() == [1, 0, 0, 0, 8, 12, 0, 1, 9, 0]
        with pytest.raises(PfacError) as e:
            g.unigram_records(d_ids=GuardedBuffer(0).ptr, out_cap=0)
        assert e.value.status == E_OVERFLOW and e.value.n_tokens == 10
        # byte fallback: the x of "playx" and the lone x by their byte ids
        bytes_ = 500 + np.arange(256)
        g.set_unigram(pieces, bytes_, bscore, unk_id=DROP)
        ids = g.unigram(uniref.LOG).tolist()
        assert ids == [1, 532, 2, 3, 532, 2, 5, 9, 510, 6, 7, 4, 532, 8, 12, 532, 2, 620, 510, 510, 1, 9, 532, 620, 510]


def test_surface_folded_table():
    """Ids of the folded pieces, positions into the unfolded text, byte ids of the bytes as written."""
    table, pieces, scale, _ = unigram_table(uniref.LOG_VOCAB, ignore_case=True)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_unigram(pieces, 500 + np.arange(256), int(-10 * scale), unk_id=DROP)
        ids, pos = g.unigram(b"The PLAYer X.\n", positions=True)
        assert ids.tolist() == [1, 532, 2, 3, 532, 500 + ord("X"), 9, 510] and pos.tolist() == [0, 3, 4, 8, 10, 11, 12, 13]


def test_embedding_bag_takes_the_device_arrays():
    name = "docs-tiny"
    dev = device(name)
    nd = dev.prepare(name)
    want = want_of(name)
    n = int(want[0].size)
    d_ids = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_off = torch.zeros(nd + 1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert dev.g.unigram_records_documents(nd, d_input=dev.d_input(name), d_ids=d_ids, out_cap=n, d_tok_offsets=d_off) == n
    dev.g.sync(0)
    gen = torch.Generator().manual_seed(7)
    weight = torch.randn(int(want[0].max()) + 1, 8, generator=gen).to("cuda:0")
    got = torch.nn.functional.embedding_bag(d_ids, weight, d_off[:-1], mode="sum")
    ref_ids = torch.from_numpy(want[0].astype(np.int32)).to("cuda:0")
    ref_off = torch.from_numpy(want[2].astype(np.int64)).to("cuda:0")
    exp = torch.nn.functional.embedding_bag(ref_ids, weight, ref_off[:-1], mode="sum")
    assert tuple(got.shape) == (nd, 8) and torch.equal(got, exp)
    assert torch.equal(d_ids, ref_ids) and torch.equal(d_off, ref_off)
