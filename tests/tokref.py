"""Host reference for the tokenize passes (the checker, never the product): the rule of include/pfac.h held twice, and
the cases that tests/test_tokens_ref.py (no GPU) and tests/test_gpu_tokens.py share.

The rule: over [entry, n_owned), a position that starts a pick emits tok[state], a position outside every pick emits
btok[byte], a position inside a pick emits nothing, and DROP emits nothing.  `by_numpy` says it with a difference array
and masks, `by_walk` as a plain walk over the picks and the gaps between them.  Both take
    (data, entry, n_owned, pos, lens, states, tok, btok[, off])
with the picks (pos, lens, states) ascending -- here `states` are the CPU oracle's pattern ids and `tok` is indexed by
them; the device's states reach the same ids through the table's idmap -- and return (ids int32, positions uint32,
tok_off uint64 or None, exit).  Picks come from the CPU oracle's records through llref.greedy (per document: the records
cut by passguard.cut_by_hand, which tests/test_passguard_cases.py holds against docreplref.per_doc, and per_doc itself
for the small log); never from the device."""
import bisect
import os

import numpy as np

import passguard
from passguard import HALO, TILE, Cpu, cut_by_hand

DROP = -1


def by_numpy(data, entry, n_owned, pos, lens, states, tok, btok, off=None):
    data = np.asarray(data, dtype=np.uint8)
    pos, lens, states = (np.asarray(a, dtype=np.int64) for a in (pos, lens, states))
    tok = np.asarray(tok, dtype=np.int64)
    btok = np.full(256, DROP, dtype=np.int64) if btok is None else np.asarray(btok, dtype=np.int64)
    n, entry = int(n_owned), int(entry)
    diff = np.zeros(n + 1, dtype=np.int64)
    np.add.at(diff, pos, 1)
    np.add.at(diff, np.minimum(pos + lens, n), -1)
    covered = np.cumsum(diff)[:n] > 0
    val = np.where(covered, DROP, btok[data[:n]])
    val[pos] = tok[states]
    emits = (val != DROP) & (np.arange(n) >= entry)
    positions = np.flatnonzero(emits)
    c = int((pos + lens)[-1]) if pos.size else entry
    tok_off = None if off is None else np.searchsorted(positions, np.asarray(off, dtype=np.int64), side="left").astype(np.uint64)
    return val[emits].astype(np.int32), positions.astype(np.uint32), tok_off, max(c, n) - n


def by_walk(data, entry, n_owned, pos, lens, states, tok, btok, off=None):
    data = bytes(np.asarray(data, dtype=np.uint8)[:int(n_owned)])
    ids, positions = [], []
    c = int(entry)

    def gap(a, b):
        for i in range(a, b):
            t = DROP if btok is None else int(btok[data[i]])
            if t != DROP:
                ids.append(t)
                positions.append(i)
    for p, L, s in zip(np.asarray(pos).tolist(), np.asarray(lens).tolist(), np.asarray(states).tolist()):
        gap(c, p)
        if int(tok[s]) != DROP:
            ids.append(int(tok[s]))
            positions.append(p)
        c = p + L
    gap(c, int(n_owned))
    tok_off = None if off is None else np.array([bisect.bisect_left(positions, int(o)) for o in off], dtype=np.uint64)
    return np.array(ids, dtype=np.int32), np.array(positions, dtype=np.uint32), tok_off, max(c, int(n_owned)) - int(n_owned)


def check(want, ids, pos=None, tok_off=None, exit=None, what="tokens"):
    """Holds a result against want = (ids, positions, tok_off, exit) and names the first differing token.  `pos`,
    `tok_off` and `exit` are compared where given."""
    wi, wp, wo, wx = want
    ids = np.asarray(ids)
    m = min(ids.size, wi.size)
    ne = np.flatnonzero(ids[:m].astype(np.int64) != wi[:m])
    if pos is not None:
        pos = np.asarray(pos)
        assert pos.size == ids.size, f"{what}: {pos.size} positions for {ids.size} ids"
        ne = np.union1d(ne, np.flatnonzero(pos[:m].astype(np.int64) != wp[:m]))
    if ne.size:
        j = int(ne[0])
        got = f"id {int(ids[j])}" + (f" at {int(pos[j])}" if pos is not None else "")
        raise AssertionError(f"{what}: token {j} is {got}, want id {int(wi[j])} at {int(wp[j])} ({ne.size} tokens differ)")
    if ids.size != wi.size:
        nxt = f"; the first one missing is id {int(wi[m])} at {int(wp[m])}" if ids.size < wi.size else f"; the first extra one is id {int(ids[m])}"
        raise AssertionError(f"{what}: {ids.size} tokens, want {wi.size}{nxt}")
    if tok_off is not None:
        tok_off = np.asarray(tok_off)
        assert wo is not None and tok_off.size == wo.size, f"{what}: {tok_off.size} token offsets, want {None if wo is None else wo.size}"
        ne = np.flatnonzero(tok_off.astype(np.int64) != wo.astype(np.int64))
        assert ne.size == 0, (f"{what}: tok_off[{int(ne[0])}] is {int(tok_off[ne[0]])}, want {int(wo[ne[0]])} "
                              f"({ne.size} offsets differ, the last is [{int(ne[-1])}])")
    if exit is not None:
        assert int(exit) == wx, f"{what}: exit {int(exit)}, want {wx}"


# ---------------------------------------------------------------------------
# token tables, by name: tok indexed by pattern id (ids count from 1), btok by byte value (None: the caller gives none)

TOKENS = ("mixed", "alldrop", "nodrop", "nullbytes", "picksdropped")
TOK_BASE, BYTE_BASE = 1000, 300
DROPPED_BYTES = b" \n,."


def token_ids(name, n_lines):
    ids = np.arange(n_lines + 1, dtype=np.int64)
    tok = (TOK_BASE + ids).astype(np.int32)
    btok = (BYTE_BASE + np.arange(256)).astype(np.int32)
    if name in ("mixed", "nullbytes"):
        tok[ids % 3 == 0] = DROP
    if name == "mixed":
        btok[np.frombuffer(DROPPED_BYTES, dtype=np.uint8)] = DROP
    if name in ("alldrop", "picksdropped"):
        tok[:] = DROP
    if name == "alldrop":
        btok[:] = DROP
    if name == "nullbytes":
        btok = None
    tok[0] = DROP
    assert name in TOKENS
    return tok, btok


def token_dict(tok):
    """{pattern id: token id} of the kept patterns: what GpuMatcher.set_token_ids takes."""
    return {int(i): int(t) for i, t in enumerate(tok) if t != DROP}


# ---------------------------------------------------------------------------
# the edge table and its input: picks on tile edges, a 1000-byte pattern, the densest tile

EDGE_LINES = [b"q", b"wxyz", b"ab", b"Z" * 1000, b"abc"]
EDGE_LONG_AT = 3 * TILE - 520           # the 1000-byte pick: from tile 2 into tile 3
EDGE_DENSE_TILE = 4                     # 4096 picks of one byte
EDGE_OWNED = 6 * TILE + 1000            # a pick ends exactly here; EDGE_OWNED - 2 lies inside it
FILLER = b"-. #"                        # matches nothing; ' ' and '.' are dropped bytes of "mixed"


def edge_input():
    n = EDGE_OWNED + HALO
    buf = np.frombuffer(FILLER, dtype=np.uint8)[np.arange(n) % len(FILLER)].copy()

    def put(at, s):
        buf[at:at + len(s)] = np.frombuffer(s, dtype=np.uint8)
    put(0, b"wxyz")                                 # a pick at position 0
    put(TILE - 4, b"wxyz")                          # ... one that ends exactly on a tile end
    put(2 * TILE - 1, b"wxyz")                      # ... one whose start is the last byte of a tile
    put(EDGE_LONG_AT, b"Z" * 1000)
    put(EDGE_DENSE_TILE * TILE, b"q" * TILE)
    put(5 * TILE + 100, b"ab-abc.abcab#q")          # (tile 5 is otherwise one gap; under "dropq"-like tables tile 4 emits nothing)
    put(EDGE_OWNED - 4, b"wxyz")                    # ends at EDGE_OWNED; from EDGE_OWNED - 2 it ends in the halo
    return buf


EDGE_KEYS = {"edge-end": ("edges", EDGE_OWNED, EDGE_OWNED + HALO, False), "edge-halo": ("edges", EDGE_OWNED - 2, EDGE_OWNED + HALO - 2, False)}
SMALL = (0, 1, 15, 16, 17, 4095, 4096, 4097)

# the small log of the surface tests: vocabulary line k has token 100 + k, a byte b outside every word 1000 + b, spaces
# and newlines emit nothing
LOG_VOCAB = [b"cat", b"concatenate", b"dog", b"the", b"a", b"cats"]
LOG = b"the cat\nconcatenate cats\n\ndog a xy\n"
LOG_IDS = [104, 101, 102, 106, 103, 105, 1120, 1121]
LOG_POS = [0, 4, 0, 12, 0, 4, 6, 7]                # relative to the line
LOG_TOK_OFF = [0, 2, 4, 4, 8]
LOG_BYTE_BASE, LOG_DROP = 1000, b" \n"
WORDS_TEXT = b"concatenated cat"
WORDS_IDS = [1000 + b for b in b"concatenated"] + [101]        # whole words: "cat" and "a" inside a word stay bytes
WORDS_IDS_PLAIN = [102, 1000 + ord("d"), 101]


def maxmatch(line, vocab, byte_base, drop):
    """The tokenizer as a textbook has it -- longest dictionary word at the cursor, else one byte, skip `drop` -- over
    one line.  It never sees a record."""
    out, i = [], 0
    while i < len(line):
        w = max((v for v in vocab if line.startswith(v, i)), key=len, default=None)
        if w is not None:
            out.append(vocab[w])
            i += len(w)
        else:
            if line[i] not in drop:
                out.append(byte_base + line[i])
            i += 1
    return out


class Ref(Cpu):
    """passguard.Cpu with the edge table ("E"), its input, arbitrary document offsets and the tokens of every case."""

    def pat(self, name):
        if name != "tokedge":
            return super().pat(name)

        def make():
            from llref import line_lengths
            from orc import Oracle
            path = os.path.join(self.dir, "tokedge.pat")
            with open(path, "wb") as f:
                f.write(b"".join(p + b"\n" for p in EDGE_LINES))
            return dict(path=path, matcher=Oracle(path, 1, 1), ll=line_lengths(path), lines=list(EDGE_LINES))
        return self._memo(("pat", name), make)

    def input(self, name):
        return self._memo(("input", name), edge_input) if name == "edges" else super().input(name)

    def info(self, W):
        return self.pat("tokedge") if W == "E" else self.tinfo(W)

    def the_table(self, W):
        from phfpfac_amd import PfacTable
        if W == "E":
            return self._memo(("table", "tokedge"), lambda: PfacTable.from_file(self.info(W)["path"], 256))
        return self.table(W)

    def small_key(self, n):
        return "text", n, n, False

    def picks(self, W, key, entry=0):
        """(pos, ids, lens, exit) of the leftmost-longest selection from `entry`."""
        ll = self.info(W)["ll"]
        if W != "E":
            pos, ids, ex = self.sel(W, key, entry)
            return pos, ids, ll[ids], ex

        def make():
            from llref import greedy
            inp, no, na, _ = key
            pos, ids = self.info(W)["matcher"].scan_spec(np.ascontiguousarray(self.input(inp)[:na]), None)
            own = pos < no
            pos, ids = pos[own].astype(np.int64), ids[own].astype(np.int64)
            idx, ex = greedy(pos, ll[ids], entry, no)
            return pos[idx], ids[idx], ll[ids[idx]], int(ex)
        return self._memo(("picks", "tokedge", key, entry), make)

    def tokens(self, W, tokname):
        return token_ids(tokname, len(self.info(W)["lines"]))

    def want(self, W, key, entry, tokname):
        """(ids, positions, None, exit) of pfac_tokenize_leftmost_longest."""
        def make():
            pos, ids, lens, ex = self.picks(W, key, entry)
            tok, btok = self.tokens(W, tokname)
            out = by_numpy(self.input(key[0]), entry, key[1], pos, lens, ids, tok, btok)
            assert out[3] == ex
            return out
        return self._memo(("want", W, key, entry, tokname), make)

    def doc_offsets(self, W, key, shape):
        """Offsets of a passguard.DOC_SHAPES name, or "words": document starts on the first and the last position of
        bitmap words, directly behind picks and in the middle of gaps."""
        if shape != "words":
            return self.offsets(W, key, shape)

        def make():
            no = key[1]
            pos, ids, lens, _ = self.picks(W, key)
            ends = pos + lens
            behind = ends[ends < no][3::40]
            gaps = np.flatnonzero(pos[1:] - ends[:-1] >= 3)[5::40]
            mid = ends[gaps] + 1
            words = np.array([64, 127, 128, 191, TILE - 1, TILE, TILE + 63, TILE + 64, 64 * TILE - 1, 64 * TILE, 64 * TILE + 63])
            cuts = np.unique(np.concatenate([behind, mid, words[words < no]]))
            return np.concatenate([[0], cuts[(cuts > 0) & (cuts < no)], [no]]).astype(np.uint64)
        return self._memo(("tokoff", W, key, shape), make)

    def doc_picks(self, W, key, shape):
        """(doc_first, pos relative to the scan, ids, lens) of every document's own selection: no kept record crosses a
        document end, so one greedy over the kept records restarts at every document (passguard.Cpu.docsel's way)."""
        def make():
            from llref import greedy
            pos, ids, lens = self.scan(W, key)
            off = self.doc_offsets(W, key, shape)
            keep = cut_by_hand(pos, ids, lens, off)[3]
            kp, ki, kl = pos[keep], ids[keep], lens[keep]
            idx, ex = greedy(kp, kl, 0, key[1])
            assert ex == 0
            first = np.searchsorted(kp[idx], off.astype(np.int64), side="left").astype(np.uint64)
            first[-1] = idx.size
            return first, kp[idx], ki[idx], kl[idx]
        return self._memo(("docpicks", W, key, shape), make)

    def want_docs(self, W, key, shape, tokname):
        """(ids, positions relative to the scan, tok_off, 0) of pfac_tokenize_documents."""
        def make():
            _, pos, ids, lens = self.doc_picks(W, key, shape)
            tok, btok = self.tokens(W, tokname)
            return by_numpy(self.input(key[0]), 0, key[1], pos, lens, ids, tok, btok, self.doc_offsets(W, key, shape))
        return self._memo(("wantdocs", W, key, shape, tokname), make)


_REF = None


def ref():
    global _REF
    if _REF is None:
        import atexit
        _REF = Ref()
        atexit.register(_REF.close)
    return _REF


CHAIN_KEY = ("text", 3 * TILE + 17, 3 * TILE + 17 + HALO, False)
CHAINS = (("inside", "behind"), ("behind", "ingap"), ("inside", "ingap"))


def chain_cuts(x, W, key=CHAIN_KEY):
    """Offsets of the scan `key` at which a chain of ranges is cut: {"inside": inside a pick, "behind": directly behind a
    pick, "ingap": inside a gap}, ascending, from the picks of the whole range from entry 0."""
    pos, _, lens, _ = x.picks(W, key)
    ends = pos + lens
    k = int(np.flatnonzero((lens >= 3) & (pos > TILE // 2))[0])
    j = k + 40
    i = int(np.flatnonzero((pos[1:] - ends[:-1] >= 3) & (np.arange(pos.size - 1) > j + 40))[0])
    cuts = {"inside": int(pos[k]) + 1, "behind": int(ends[j]), "ingap": int(ends[i]) + 1}
    assert 0 < cuts["inside"] < cuts["behind"] < cuts["ingap"] < key[1]
    return cuts


# ---------------------------------------------------------------------------
# the named cases: name -> (W, scan key, entry, token table, document shape or None)

def cases(x):
    def make():
        out = {}
        for n in SMALL:
            out[f"n{n}"] = (2, x.small_key(n), 0, "mixed", None)
        for name in passguard.SIZE_CASES:
            out[name] = (2, x.size_key(name), 0, "mixed", None)
        out["w4-t65"] = (4, x.size_key("t65"), 0, "mixed", None)
        out["w8-t3"] = (8, x.size_key("t3"), 0, "mixed", None)
        out["w4-halo"] = (4, x.size_key("halo"), 0, "mixed", None)
        out[passguard.FILTERED] = (2, x.size_key(passguard.FILTERED), 0, "mixed", None)
        out["entry"] = (2, x.size_key("halo"), 2, "mixed", None)
        for c in passguard.SEL_COUNTS:
            out[f"sel{c}"] = (2, x.sel_key(2, c), 0, "mixed", None)
        for name, key in EDGE_KEYS.items():
            out[name] = ("E", key, 0, "mixed", None)
        for t in TOKENS[1:]:
            out[f"edge-{t}"] = ("E", EDGE_KEYS["edge-end"], 0, t, None)
            out[f"t3-{t}"] = (2, x.size_key("t3"), 0, t, None)
        for shape in passguard.DOC_SHAPES + ("words",):
            out[f"docs-{shape}"] = (2, x.doc_key(shape), 0, "mixed", shape)
        out["docs-w4-tiny"] = (4, x.doc_key("tiny"), 0, "mixed", "tiny")
        out["docs-alldrop"] = (2, x.doc_key("emptymid"), 0, "alldrop", "emptymid")
        return out
    return x._memo(("tokcases",), make)


TRIVIAL = tuple(f"n{n}" for n in SMALL) + ("none", "docs-nothing")       # too small, or without a pick, for the four-way mix
NAMES = (tuple(f"n{n}" for n in SMALL) + passguard.SIZE_CASES + ("w4-t65", "w8-t3", "w4-halo", passguard.FILTERED, "entry") +
         tuple(f"sel{c}" for c in passguard.SEL_COUNTS) + tuple(EDGE_KEYS) +
         tuple(f"{p}-{t}" for t in TOKENS[1:] for p in ("edge", "t3")) +
         tuple(f"docs-{s}" for s in passguard.DOC_SHAPES + ("words",)) + ("docs-w4-tiny", "docs-alldrop"))


MIXED = tuple(n for n in NAMES if not n.endswith(tuple("-" + t for t in TOKENS[1:])))       # the cases under the "mixed" table


def want_of(x, name):
    W, key, entry, tokname, shape = cases(x)[name]
    return x.want(W, key, entry, tokname) if shape is None else x.want_docs(W, key, shape, tokname)


def picks_of(x, name):
    """(pos, ids, lens) of a case's picks, positions relative to the scan."""
    W, key, entry, _, shape = cases(x)[name]
    if shape is None:
        return x.picks(W, key, entry)[:3]
    return x.doc_picks(W, key, shape)[1:]
