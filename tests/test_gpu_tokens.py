"""Tokenization on the GPU (run with -m gpu on an MI355X): pfac_table_set_token_ids, pfac_tokenize_leftmost_longest,
pfac_tokenize_documents and their fetches against tests/tokref.py, whose cases tests/test_tokens_ref.py holds against a
second form of the rule and checks for their preconditions without a GPU.  Every named case runs through
passguard.exact_call with guard bands of exactly n_tokens x 4 (ids), n_tokens x 4 (positions) and (n_docs + 1) x 8
bytes, under both fills.  Integer work: bit-exact.  No expectation comes from the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import passguard
import tokref
from heapguard import FILLS, GuardedBuffer
from passguard import E_ARG, E_OVERFLOW, E_STATE, OK, TILE, Want, exact_call
from phfpfac_amd import PFAC_TOKENS_POSITIONS, GpuMatcher, PfacError, PfacTable
from phfpfac_amd.matcher import _ptr
from tokref import cases, check, ref, want_of

pytestmark = pytest.mark.gpu

_DEV = {}


class TokDevice(passguard.Device):
    """passguard.Device with the edge table ("E") and the named token tables."""

    def __init__(self, W, x):
        self.W, self.x, self.dev = W, x, 0
        self.table = x.the_table(W)
        self.g = GpuMatcher(0, 1)
        with passguard._Env({} if W == "E" else passguard.TABLES[W]["knobs"]):
            self.g.load_table(self.table)
        self.g.set_final_lengths(self.table.final_lengths())
        if W != "E":
            self.g.set_replacements(x.reps(W))
        self.inputs, self.cur, self.tokname = {}, None, None
        self.idmap = np.asarray(self.table.idmap, dtype=np.int64)

    def scan(self, key):
        if self.W != "E":
            return super().scan(key)
        if self.cur != key:
            self.cur = None
            self.g.reserve(0, 0, max(key[2], TILE))
            self.g.scan_resident(key[1], key[2], d_input=self.d_input(key[0]))
            self.cur = key

    def use_tokens(self, tokname):
        if self.tokname != tokname:
            tok, btok = self.x.tokens(self.W, tokname)
            self.g.set_token_ids(tokref.token_dict(tok), byte_ids=btok)
            self.tokname = tokname


def device(W):
    if W not in _DEV:
        _DEV[W] = TokDevice(W, ref())
    return _DEV[W]


@pytest.fixture(scope="module", autouse=True)
def _close_devices():
    yield
    for d in _DEV.values():
        d.close()
    _DEV.clear()


def prepare(name):
    """The device with the case's tokens, scan and selection as the slot's last -> (dev, want, n_docs or None)."""
    x = ref()
    W, key, entry, tokname, shape = cases(x)[name]
    dev = device(W)
    dev.use_tokens(tokname)
    dev.scan(key)
    want = want_of(x, name)
    if shape is None:
        n_sel, ex = dev.g.select_leftmost_longest(entry)
        assert ex == want[3], f"exit {ex}, want {want[3]}"
        return dev, want, None
    off = x.doc_offsets(W, key, shape)
    dev.g.set_doc_offsets(off)
    dev.g.select_leftmost_longest_documents(int(off.size) - 1)
    return dev, want, int(off.size) - 1


def run(dev, name, nd, **kw):
    """The pass over the case's prepared selection, reading the input the scan read."""
    d_in = dev.d_input(cases(ref())[name][1][0])
    return dev.g.tokenize_selection(d_input=d_in, **kw) if nd is None else dev.g.tokenize_selection_documents(d_input=d_in, **kw)


def exact(name, fill):
    dev, want, nd = prepare(name)
    g, key = dev.g, cases(ref())[name][1]
    n = int(want[0].size)
    buf = {"d_ids": GuardedBuffer(n * 4, fill=fill), "d_pos": GuardedBuffer(n * 4, fill=fill)}
    payloads = {"d_ids": want[0], "d_pos": want[1]}
    d_in = dev.d_input(key[0])
    if nd is None:
        def call(cap, bad=None):
            return dev._status(lambda: g.tokenize_selection(d_input=d_in, d_ids=buf["d_ids"].ptr, out_cap=cap, d_pos=buf["d_pos"].ptr), "n_tokens")
    else:
        buf["d_tok_offsets"] = GuardedBuffer((nd + 1) * 8, fill=fill)
        payloads["d_tok_offsets"] = want[2]

        def call(cap, bad=None):
            return dev._status(lambda: g.tokenize_selection_documents(d_input=d_in, d_ids=buf["d_ids"].ptr, out_cap=cap, d_pos=buf["d_pos"].ptr,
                                                                      d_tok_offsets=buf["d_tok_offsets"].ptr), "n_tokens")
    exact_call(g, call, Want(n, payloads), buf, fill, f"tokenize case {name} ({n} tokens" + (f", {nd} documents)" if nd is not None else ")"))


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name", tokref.NAMES)
def test_case_at_exact_capacity(name, fill):
    exact(name, fill)


@pytest.mark.parametrize("name", ["n0", "n17", "t65", "edge-nodrop", "edge-alldrop", "docs-words", "docs-emptygroup", "docs-alldrop"])
def test_slot_owned_result_and_ids_alone(name):
    """The slot-owned buffers through the fetches, windows of them, and the pass without positions into an exact d_ids."""
    dev, want, nd = prepare(name)
    g = dev.g
    n = int(want[0].size)
    assert run(dev, name, nd, positions=True) == n
    if nd is not None:
        check(want, *g.tokens_to_host(n, True), tok_off=g.token_offsets_to_host(nd), what=name)
    ids, pos = g.tokens_to_host(n, True)
    check(want, ids, pos, what=name)
    if n > 5:
        a, b = g.tokens_to_host(n - 5, True, first=3)
        assert np.array_equal(a, want[0][3:n - 2]) and np.array_equal(b, want[1][3:n - 2])
    e = dev._status(lambda: g.tokens_to_host(1, first=n))
    assert e[0] == E_ARG, "a window past the result"
    # without the flag: ids only, exact, and no positions to fetch
    buf = GuardedBuffer(n * 4, fill=FILLS[1])
    assert run(dev, name, nd, d_ids=buf.ptr, out_cap=n) == n
    if nd is not None:
        assert np.array_equal(g.token_offsets_to_host(nd), want[2])
    g.sync(0)
    buf.check(what="d_ids")
    check(want, buf.host().view(np.int32), what=name)
    assert dev._status(lambda: g.tokens_to_host(0))[0] == E_STATE, "the ids went to the caller's buffer"
    # the same call twice gives the same bytes
    got = []
    for _ in range(2):
        run(dev, name, nd, positions=True)
        got.append(g.tokens_to_host(n, True))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*got))


@pytest.mark.parametrize("chain", tokref.CHAINS, ids=["-".join(c) for c in tokref.CHAINS])
def test_chained_ranges_concatenate(chain):
    x = ref()
    W, key = 2, tokref.CHAIN_KEY
    dev = device(W)
    dev.use_tokens("mixed")
    dev.cur = None                                             # (the high-level call scans the slot's own input)
    cuts = tokref.chain_cuts(x, W)
    whole = x.want(W, key, 0, "mixed")
    data, M = x.input(key[0]), x.M(W)
    edges = [0] + [cuts[c] for c in chain] + [key[1]]
    ids, positions, entry = [], [], 0
    for a, b in zip(edges[:-1], edges[1:]):
        na = min(b + M - 1, key[2])
        i, p, entry = dev.g.tokenize(data[a:na], n_owned=b - a, entry=entry, positions=True)
        ids.append(i)
        positions.append(p.astype(np.int64) + a)
    check(whole, np.concatenate(ids), np.concatenate(positions), exit=entry, what=f"three ranges cut {chain}")
    i, p, ex = dev.g.tokenize(data[:key[2]], n_owned=key[1], positions=True)
    check(whole, i, p, exit=ex, what="one call")


# ---------------------------------------------------------------------------
# the ladder of errors, through the C ABI as it is

def raw(g, d_input=None, d_sel=None, flags=0, d_ids=None, cap=0, d_pos=None, docs=None):
    n = C.c_uint64(12345)
    if docs is None:
        rc = g._L.pfac_tokenize_leftmost_longest(g._ctx, 0, _ptr(d_input), _ptr(d_sel), int(flags), _ptr(d_ids), int(cap), _ptr(d_pos), C.byref(n))
    else:
        rc = g._L.pfac_tokenize_documents(g._ctx, 0, _ptr(d_input), _ptr(d_sel), _ptr(docs.get("off")), _ptr(docs.get("first")), int(flags),
                                          _ptr(d_ids), int(cap), _ptr(d_pos), _ptr(docs.get("tok_off")), C.byref(n))
    return rc, n.value


class Guards:
    def __init__(self, n=64, nd=8):
        self.ids, self.pos, self.off = GuardedBuffer(n * 4), GuardedBuffer(n * 4), GuardedBuffer((nd + 1) * 8)
        self.n = n

    def untouched(self, what):
        for name in ("ids", "pos", "off"):
            getattr(self, name).check(payload_untouched=True, what=f"{name} after {what}")


def _vocab(tmp_path, lines=tokref.LOG_VOCAB, **kw):
    path = str(tmp_path / "vocab.pat")
    open(path, "wb").write(b"".join(w + b"\n" for w in lines))
    return PfacTable.from_file(path, 256, **kw)


def _log_tokens(g):
    g.set_token_ids([100 + k for k in range(1, len(tokref.LOG_VOCAB) + 1)], byte_base=tokref.LOG_BYTE_BASE, drop_bytes=tokref.LOG_DROP)


def test_ladder_of_state_errors(tmp_path):
    table = _vocab(tmp_path)
    data = np.frombuffer(tokref.LOG, dtype=np.uint8)
    gd = Guards()
    with GpuMatcher(0, 1) as g:
        def refused(what, status=E_STATE, **kw):
            rc, n = raw(g, flags=PFAC_TOKENS_POSITIONS, d_ids=gd.ids.ptr, cap=gd.n, d_pos=gd.pos.ptr, **kw)
            g.sync(0)
            assert rc == status, f"{what}: {passguard.STATUS.get(rc, rc)}"
            gd.untouched(what)
        refused("no table")
        rc = g._L.pfac_table_set_token_ids(g._ctx, None, 0, None)
        assert rc == E_STATE, "token ids before a table"
        g.load_table(table)
        _log_tokens(g)
        refused("no final lengths (and no scan)")
        g.scan_bytes(data)
        refused("no selection")
        g.scan_leftmost_longest(data)
        assert raw(g)[0] == OK
        g.scan_bytes(data)
        refused("a selection older than the scan")
        g.scan_leftmost_longest(data)
        g.load_table(table)
        refused("a selection of an earlier table (no token ids either)")
        _log_tokens(g)
        g.set_final_lengths(table.final_lengths())
        refused("a selection of an earlier table")
        g.scan_leftmost_longest(data)
        assert raw(g)[0] == OK
        g.load_table(table)
        g.scan_leftmost_longest(data)
        refused("token ids dropped by an upload")
        assert "token ids" in g._L.pfac_last_error(g._ctx).decode()
        _log_tokens(g)
        assert raw(g)[0] == OK
        refused("pfac_tokenize_documents over a whole-stream selection", docs={"tok_off": gd.off.ptr})
        # a reserve that replaces a buffer leaves no scan to tokenize
        g.reserve(0, 1 << 20, 1 << 16)
        refused("a reserve that replaced a buffer")


def test_ladder_of_argument_errors(tmp_path):
    table = _vocab(tmp_path)
    data = np.frombuffer(tokref.LOG, dtype=np.uint8)
    gd = Guards(nd=4)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        nf = int(table.num_final)
        ok = np.zeros(nf, dtype=np.int32)
        L = g._L
        assert L.pfac_table_set_token_ids(g._ctx, ok.ctypes.data, nf - 1, None) == E_ARG, "n_states != num_final"
        assert L.pfac_table_set_token_ids(g._ctx, ok.ctypes.data, nf + 1, None) == E_ARG
        bad = ok.copy()
        bad[nf - 1] = -2
        assert L.pfac_table_set_token_ids(g._ctx, bad.ctypes.data, nf, None) == E_ARG, "an id of -2"
        bb = np.zeros(256, dtype=np.int32)
        bb[255] = -2
        assert L.pfac_table_set_token_ids(g._ctx, ok.ctypes.data, nf, bb.ctypes.data) == E_ARG, "a byte id of -2"
        _log_tokens(g)
        assert L.pfac_table_set_token_ids(g._ctx, bad.ctypes.data, nf, None) == E_ARG      # refused: the earlier ids stay in force
        d_in = torch.zeros(data.size + 64, dtype=torch.uint8, device="cuda:0")
        d_in[:data.size].copy_(torch.from_numpy(data.copy()))
        torch.cuda.synchronize()
        g.reserve(0, 0, 4096)
        g.set_final_lengths(table.final_lengths())
        g.scan_resident(data.size, data.size, d_input=d_in)
        nd = len(tokref.LOG_TOK_OFF) - 1
        g.set_doc_offsets(np.concatenate([[0], np.flatnonzero(data == 10) + 1]).astype(np.uint64))
        n_sel = g.select_leftmost_longest_documents(nd)
        sel, first = g.doc_selection_to_host(n_sel, nd)[::-1]
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
        refused("an unknown flag", flags=P | 0x80000000)
        refused("d_pos without the flag", flags=0, docs=docs)
        refused("d_pos without the flag", flags=0)
        # the call itself is fine
        rc, n = raw(g, **full, docs=docs)
        g.sync(0)
        assert (rc, n) == (OK, len(tokref.LOG_IDS))
        assert gd.ids.host().view(np.int32)[:n].tolist() == tokref.LOG_IDS
        assert gd.off.host().view(np.uint64).tolist() == tokref.LOG_TOK_OFF
        # a caller's d_sel that is no selection of this scan and table
        gd = Guards(nd=4)
        full.update(d_ids=gd.ids.ptr, d_pos=gd.pos.ptr)
        docs = {"tok_off": gd.off.ptr}
        lens = table.final_lengths()[sel["state"]]
        k = int(np.flatnonzero(lens[:-1] >= 2)[0])
        variants = {}
        v = sel.copy(); v["state"][1] = nf; variants["a state equal to num_final"] = v
        v = sel.copy(); v[[1, 2]] = v[[2, 1]]; variants["two picks swapped"] = v
        v = sel.copy(); v["pos"][k + 1] = v["pos"][k] + 1; variants["two overlapping"] = v
        v = sel.copy(); v["pos"][-1] = data.size; variants["one at n_owned"] = v
        assert sel["pos"][k + 1] > sel["pos"][k] + 1 and n_sel > 3
        for what, v in variants.items():
            d_bad = torch.from_numpy(v.view(np.uint8).copy()).to("cuda:0")
            torch.cuda.synchronize()
            refused(what, d_sel=d_bad, docs=docs)
            refused(what + " (whole-stream call)", d_sel=d_bad)
        rc, n = raw(g, **full, d_sel=d_sel, docs=docs)
        g.sync(0)
        assert (rc, n) == (OK, len(tokref.LOG_IDS)) and gd.ids.host().view(np.int32)[:n].tolist() == tokref.LOG_IDS
        # an end that disagrees with exit: the last pick taken away from a selection that ended in the halo
        at = tokref.LOG.index(b"dog")
        g.scan_resident(at + 1, data.size, d_input=d_in)         # "dog" starts below n_owned and ends in the halo
        n_sel, ex = g.select_leftmost_longest(0)
        assert ex == 2
        v = g.selection_to_host(n_sel).copy()
        fl = table.final_lengths()
        v["state"][-1] = int(np.flatnonzero((np.asarray(table.idmap)[:nf] == 5) & (fl[:nf] == 1))[0])     # the state of "a"
        d_bad = torch.from_numpy(v.view(np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        gd = Guards(nd=4)                                       # (the good call above wrote the earlier ones)
        full.update(d_ids=gd.ids.ptr, d_pos=gd.pos.ptr)
        refused("an end that disagrees with exit", d_sel=d_bad)
        rc, n = raw(g, **full)
        g.sync(0)
        assert (rc, n) == (OK, tokref.LOG_IDS.index(103) + 1)


def test_overflow_carries_the_exact_count():
    dev, want, nd = prepare("docs-words")
    g = dev.g
    n = int(want[0].size)
    gd = Guards(n=n - 1, nd=nd)
    with pytest.raises(PfacError) as e:
        g.tokenize_selection_documents(d_ids=gd.ids.ptr, out_cap=n - 1, d_pos=gd.pos.ptr, d_tok_offsets=gd.off.ptr,
                                       d_input=dev.d_input(cases(ref())["docs-words"][1][0]))
    assert e.value.status == E_OVERFLOW and e.value.n_tokens == n
    g.sync(0)
    gd.untouched("the overflow")
    with pytest.raises(PfacError) as e:                         # the positions alone are the caller's
        g.tokenize_selection(d_pos=gd.pos.ptr, out_cap=n - 1, d_input=dev.d_input(cases(ref())["docs-words"][1][0]))
    assert e.value.status == E_OVERFLOW and e.value.n_tokens == n
    gd.untouched("the overflow")


def test_lifetime_of_the_slot_owned_tokens():
    """The slot-owned ids survive a replace, an extraction and a score pass; the pass's own next call, and a refused
    call of it, discard them."""
    dev, want, _ = prepare("t3")
    g = dev.g
    n = run(dev, "t3", None, positions=True)
    g.replace_selection(d_input=dev.d_input("text"))
    g.extract_selection(d_input=dev.d_input("text"))
    g.set_pattern_weights(np.arange(17))
    g.set_doc_offsets(np.array([0, 100, cases(ref())["t3"][1][1]], dtype=np.uint64))
    g.document_scores(2)
    check(want, *g.tokens_to_host(n, True), what="after a replace, an extraction and a score pass")
    rep = g.replacement_to_host(16)
    run(dev, "t3", None)
    assert np.array_equal(g.replacement_to_host(16), rep), "the tokenize pass invalidates no other pass's output"
    assert dev._status(lambda: g.tokens_to_host(n, True))[0] == E_STATE, "the next call wrote no positions"
    check(want, g.tokens_to_host(n), what="ids of the next call")
    rc, _ = raw(g, flags=2)
    assert rc == E_ARG
    assert dev._status(lambda: g.tokens_to_host(n))[0] == E_STATE, "a refused call discards the earlier result"


# ---------------------------------------------------------------------------
# the surface

def test_surface_on_a_small_log(tmp_path):
    with GpuMatcher(0, 1) as g:
        g.load_table(_vocab(tmp_path))
        _log_tokens(g)
        ids, tok_off = g.tokenize_lines(tokref.LOG)
        assert ids.dtype == np.int32 and ids.tolist() == tokref.LOG_IDS and tok_off.tolist() == tokref.LOG_TOK_OFF
        ids, pos, tok_off = g.tokenize_lines(tokref.LOG, positions=True)
        assert ids.tolist() == tokref.LOG_IDS and pos.tolist() == tokref.LOG_POS and tok_off.tolist() == tokref.LOG_TOK_OFF
        docs = [line + b"\n" for line in tokref.LOG.split(b"\n")[:-1]]
        ids, pos, tok_off = g.tokenize_documents(docs, positions=True)
        assert ids.tolist() == tokref.LOG_IDS and pos.tolist() == tokref.LOG_POS and tok_off.tolist() == tokref.LOG_TOK_OFF
        ids, tok_off = g.tokenize_documents(docs)
        assert ids.tolist() == tokref.LOG_IDS and tok_off.tolist() == tokref.LOG_TOK_OFF
        ids, ex = g.tokenize(tokref.LOG)
        assert ids.tolist() == tokref.LOG_IDS and ex == 0
        ids, pos, ex = g.tokenize(tokref.LOG, positions=True)
        off = np.concatenate([[0], np.flatnonzero(np.frombuffer(tokref.LOG, dtype=np.uint8) == 10) + 1])
        assert pos.tolist() == (np.array(tokref.LOG_POS) + np.repeat(off[:-1], np.diff(tokref.LOG_TOK_OFF))).tolist()
        # whole words: "cat" (and "a") inside "concatenated" stay bytes
        assert g.tokenize(tokref.WORDS_TEXT)[0].tolist() == tokref.WORDS_IDS_PLAIN
        assert g.tokenize(tokref.WORDS_TEXT, whole_words=True)[0].tolist() == tokref.WORDS_IDS
        assert g.tokenize_lines(tokref.WORDS_TEXT + b"\n", whole_words=True)[0].tolist() == tokref.WORDS_IDS
        # byte ids given whole, and none at all
        g.set_token_ids({1: 5}, byte_ids=np.arange(256))
        assert g.tokenize(b"x a cat")[0].tolist() == [ord("x"), ord(" "), ord(" "), 5]      # ("a" is a pattern without a token)
        g.set_token_ids({1: 5})
        assert g.tokenize(b"x a cat")[0].tolist() == [5]
        with pytest.raises(ValueError):
            g.set_token_ids({1: 5}, byte_ids=np.arange(256), byte_base=3)
        with pytest.raises(PfacError) as e:
            g.tokenize_selection(d_ids=GuardedBuffer(0).ptr, out_cap=0)
        assert e.value.status == E_OVERFLOW and e.value.n_tokens == 1


def test_surface_folded_table(tmp_path):
    """Ids of the folded patterns, positions into (and byte tokens of) the unfolded text."""
    with GpuMatcher(0, 1) as g:
        g.load_table(_vocab(tmp_path, ignore_case=True))
        _log_tokens(g)
        ids, pos, _ = g.tokenize(b"The CAT X\n", positions=True)
        assert ids.tolist() == [104, 101, 1000 + ord("X")] and pos.tolist() == [0, 4, 8]


def test_surface_class_table():
    """A state that stands for several patterns takes its lowest id's token."""
    table = PfacTable.from_charclass(b"[a-c]x\nbx\n")
    assert int(np.diff(table.out_first).max()) == 2, "a state of two ids"
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_token_ids({1: 11, 2: 22}, byte_base=1000)
        assert g.tokenize(b"bx-ax")[0].tolist() == [11, 1000 + ord("-"), 11]
        g.set_token_ids({2: 22}, byte_base=1000)
        assert g.tokenize(b"bx-ax")[0].tolist() == [1000 + ord("-")]


def test_embedding_bag_takes_the_device_arrays():
    dev, want, nd = prepare("docs-tiny")
    g = dev.g
    n = int(want[0].size)
    d_ids = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_off = torch.zeros(nd + 1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert g.tokenize_selection_documents(d_input=dev.d_input("text"), d_ids=d_ids, out_cap=n, d_tok_offsets=d_off) == n
    g.sync(0)
    gen = torch.Generator().manual_seed(7)
    weight = torch.randn(int(want[0].max()) + 1, 8, generator=gen).to("cuda:0")
    got = torch.nn.functional.embedding_bag(d_ids, weight, d_off[:-1], mode="sum")
    ref_ids = torch.from_numpy(want[0].astype(np.int32)).to("cuda:0")
    ref_off = torch.from_numpy(want[2].astype(np.int64)).to("cuda:0")
    exp = torch.nn.functional.embedding_bag(ref_ids, weight, ref_off[:-1], mode="sum")
    assert tuple(got.shape) == (nd, 8) and torch.equal(got, exp)
    assert torch.equal(d_ids, ref_ids) and torch.equal(d_off, ref_off)
