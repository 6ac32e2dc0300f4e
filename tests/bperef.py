"""Host reference for the BPE passes (the checker, never the product): THE RULE of include/pfac.h held twice, and the
cases that tests/test_bpe_ref.py (no GPU) and tests/test_gpu_bpe.py share.

The rule: a run is a maximal run of word bytes inside [0, n_owned); its word takes the one lead byte in front of it, if
there is one.  A word of at most max_word bytes starts as single bytes; two adjacent parts are a candidate iff their
concatenation is a vocabulary string whose split is 0 or the left part's length; the candidate of the lowest rank is
merged, the leftmost of equal ranks, until none is left.  A part of two or more bytes emits its string's id at its
start, a single byte and every byte outside words its byte id; DROP emits nothing.

  by_strings   per word, a list of parts and a dict string -> (id, rank, split).  It never sees a record.
  by_records   over a record list in heap order (position, length) with a first-record index per position, a boundary
               bitmap and a cached rank per boundary, as the kernel does it.

Both return (ids int32, positions uint32, tok_off uint64 or None).  No expectation comes from the device."""
import numpy as np

import uniref
import wpref
from wpref import DROP, TILE, put, spaced

NONE = 1 << 40                      # no candidate
DEFAULT_WORD = uniref.DEFAULT_WORD  # every byte but \t \n \v \f \r and space
CASE_WORD = wpref.DEFAULT_WORD      # [0-9A-Za-z_]


class Vocab:
    """A vocabulary as the rule sees it: `strings` maps a string of two or more bytes to (id, rank, split); built from
    `vocab` (token bytes -> id) and the ordered `merges` (left, right): merge k makes left + right with rank k and split
    len(left); the first merge that makes a string keeps it.  Single-byte tokens give the byte ids.  `drop`: strings
    whose id is DROP; `any_split`: every split 0.  Written apart from phfpfac_amd.table.bpe_table, which
    test_bpe_ref.py holds against it."""

    def __init__(self, vocab, merges, lead=0x20, max_word=64, word=CASE_WORD, fold=False, byte_ids=None, any_split=False,
                 drop=(), coarse=1):
        self.vocab = {bytes(k): int(i) for k, i in vocab.items()}
        self.merges = [(bytes(l), bytes(r)) for l, r in merges]
        self.lead, self.max_word, self.fold, self.any_split = int(lead), int(max_word), bool(fold), bool(any_split)
        self.word = np.zeros(256, dtype=bool)
        self.word[np.frombuffer(bytes(word), dtype=np.uint8)] = True
        self.strings, self.skipped = {}, []
        for k, (l, r) in enumerate(self.merges):
            s = l + r
            if self.fold:
                s = s.lower()
            why = self.refuses(s)
            if why is None and s not in self.vocab:
                why = "not in vocab"
            if why is None and s in self.strings:
                why = "ambiguous"
            if why is not None:
                self.skipped.append((k, (l, r), why))
                continue
            self.strings[s] = (DROP if s in drop else self.vocab[s], k // coarse, 0 if any_split else len(l))
        if byte_ids is None:
            byte_ids = np.full(256, DROP, dtype=np.int64)
            for tok, i in self.vocab.items():
                if len(tok) == 1:
                    byte_ids[tok[0]] = i
        self.byte_ids = np.asarray(byte_ids, dtype=np.int64).copy()
        self.pieces = sorted(self.strings)
        self.longest = max((len(p) for p in self.pieces), default=0)

    def refuses(self, s):
        """Why the rule can never produce the string s, or None."""
        if b"\n" in s:
            return "newline"
        if len(s) >= 1024:
            return "too long"
        for j, b in enumerate(s):
            if not self.word[b]:
                if b != self.lead:
                    return "non-word byte"
                if j:
                    return "lead inside"
        return None

    def with_any_split(self):
        v = Vocab.__new__(Vocab)
        v.__dict__.update(self.__dict__)
        v.any_split = True
        v.strings = {s: (i, r, 0) for s, (i, r, _) in self.strings.items()}
        return v

    def word_set(self):
        w = [0, 0, 0, 0]
        for b in np.flatnonzero(self.word).tolist():
            w[b >> 6] |= 1 << (b & 63)
        return np.array(w, dtype=np.uint64)

    def quad(self, piece):
        i, r, sp = self.strings[piece]
        return i, r, sp, 0


def records(data, n_owned, v):
    """Every occurrence of a vocabulary string that starts below n_owned, in heap order -> (pos, lens, piece index)."""
    return wpref.records(data, n_owned, v)


def words(data, n, v):
    """-> [(a, b)] of every word of [0, n), the lead rule applied, and the mask of the bytes inside words."""
    W = v.word[np.asarray(data, dtype=np.uint8)[:n]]
    prev = np.concatenate([[False], W[:-1]])
    nxt = np.concatenate([W[1:], [False]])
    starts, ends = np.flatnonzero(W & ~prev), np.flatnonzero(W & ~nxt) + 1
    if v.lead >= 0 and starts.size:
        front = np.asarray(data, dtype=np.uint8)[np.maximum(starts - 1, 0)]
        starts = starts - ((starts > 0) & (front == v.lead))
    return list(zip(starts.tolist(), ends.tolist()))


def _finish(val, off):
    positions = np.flatnonzero(val != DROP)
    tok_off = None if off is None else np.searchsorted(positions, np.asarray(off, dtype=np.int64), side="left").astype(np.uint64)
    return val[positions].astype(np.int32), positions.astype(np.uint32), tok_off


def by_strings(data, n_owned, v, off=None, stats=None):
    """(a): word by word over a list of parts; the candidates come from the dict.  `stats` (a dict) gathers: merge steps
    whose lowest rank two candidates shared ("ties"), words with a lead byte, words over the cap, parts of two or more
    bytes whose id is DROP."""
    data = np.asarray(data, dtype=np.uint8)
    n = int(n_owned)
    raw = bytes(data[:n])
    val = v.byte_ids[data[:n]].astype(np.int64)
    st = {"ties": 0, "lead": 0, "over": 0, "dropped": 0}
    solved = {}                                                 # word bytes -> (parts, tied steps): a text repeats its words
    for a, b in words(data, n, v):
        w = raw[a:b].lower() if v.fold else raw[a:b]
        st["lead"] += not v.word[data[a]]
        if b - a > v.max_word:
            st["over"] += 1
            continue
        if w not in solved:
            parts, ties = [w[i:i + 1] for i in range(b - a)], 0
            while True:
                ranks = []
                for i in range(len(parts) - 1):
                    hit = v.strings.get(parts[i] + parts[i + 1])
                    ranks.append(hit[1] if hit is not None and hit[2] in (0, len(parts[i])) else NONE)
                low = min(ranks, default=NONE)
                if low == NONE:
                    break
                ties += ranks.count(low) > 1
                i = ranks.index(low)
                parts[i:i + 2] = [parts[i] + parts[i + 1]]
            solved[w] = (parts, ties)
        parts, ties = solved[w]
        st["ties"] += ties
        at = a
        for p in parts:
            if len(p) > 1:
                val[at] = v.strings[p][0]
                val[at + 1:at + len(p)] = DROP
                st["dropped"] += v.strings[p][0] == DROP
            at += len(p)
    if stats is not None:
        stats.update(st)
    return _finish(val, off)


def by_records(data, n_owned, pos, lens, idx, v, off=None):
    """(b): over the records as the heap orders them: the first record of every position, a boundary bitmap, a cached
    rank per boundary; a lookup walks a position's records in ascending length."""
    data = np.asarray(data, dtype=np.uint8)
    n = int(n_owned)
    val = v.byte_ids[data[:n]].astype(np.int64)
    quads = [v.quad(p) for p in v.pieces]
    pos_l, len_l, idx_l = (np.asarray(x, dtype=np.int64).tolist() for x in (pos, lens, idx))
    n_rec = len(pos_l)
    first = {}
    for k in range(n_rec - 1, -1, -1):
        first[pos_l[k]] = k

    def find(l, length):
        k = first.get(l)
        while k is not None and k < n_rec and pos_l[k] == l:
            if len_l[k] >= length:
                return idx_l[k] if len_l[k] == length else None
            k += 1
        return None

    def cand(l, k, r):
        s = find(l, r - l)
        if s is None:
            return NONE
        _, rank, split, _ = quads[s]
        return rank if split in (0, k - l) else NONE

    for a, b in words(data, n, v):
        if b - a > v.max_word:
            continue
        P = [True] * (b - a + 1)                                # P[i]: a part starts at a + i (and one at b)
        rank = [NONE] * (b - a + 1)

        def prev(i):
            i -= 1
            while not P[i]:
                i -= 1
            return i

        def nxt(i):
            while not P[i]:
                i += 1
            return i
        for i in range(1, b - a):
            rank[i] = cand(a + i - 1, a + i, a + i + 1)
        while True:
            low, at = NONE, 0
            for i in range(1, b - a):
                if rank[i] < low:
                    low, at = rank[i], i
            if low == NONE:
                break
            P[at] = False
            rank[at] = NONE
            l, r = prev(at), nxt(at + 1)
            if l > 0:
                rank[l] = cand(a + prev(l), a + l, a + r)
            if r < b - a:
                rank[r] = cand(a + l, a + r, a + nxt(r + 1))
        i = 0
        while i < b - a:
            r = nxt(i + 1)
            if r - i > 1:
                s = find(a + i, r - i)
                val[a + i] = quads[s][0]
                val[a + i + 1:a + r] = DROP
            i = r
    return _finish(val, off)


def greedy(data, n_owned, v):
    """The leftmost-longest cut of every word over the same strings: only to count where BPE differs."""
    data = np.asarray(data, dtype=np.uint8)
    n = int(n_owned)
    raw = bytes(data[:n])
    val = v.byte_ids[data[:n]].astype(np.int64)
    for a, b in words(data, n, v):
        if b - a > v.max_word:
            continue
        w = raw[a:b].lower() if v.fold else raw[a:b]
        c = 0
        while c < len(w):
            for L in range(min(len(w) - c, v.longest), 1, -1):
                if w[c:c + L] in v.strings:
                    val[a + c] = v.strings[w[c:c + L]][0]
                    val[a + c + 1:a + c + L] = DROP
                    c += L
                    break
            else:
                c += 1
    return _finish(val, None)


def want(data, n_owned, v, off=None):
    """What the passes deliver for this input: by_records over every record of the scan."""
    p, l, k = records(data, n_owned, v)
    return by_records(data, n_owned, p, l, k, v, off)


def boundaries_ok(data, n_owned, off, v):
    """No offset strictly inside a word; between a lead byte and its run is inside."""
    data = np.asarray(data, dtype=np.uint8)
    inside = np.zeros(int(n_owned) + 1, dtype=bool)
    for a, b in words(data, int(n_owned), v):
        inside[a + 1:b] = True
    return not inside[np.asarray(off, dtype=np.int64)].any()


def to_boundary(data, n_owned, o, v):
    """The nearest offset at or behind o that is not inside a word."""
    o = int(o)
    while 0 < o < n_owned and v.word[data[o]] and (v.word[data[o - 1]] or int(data[o - 1]) == v.lead):
        o += 1
    return min(o, int(n_owned))


def check(wanted, ids, pos=None, tok_off=None, what="bpe"):
    """Holds a result against wanted = (ids, positions, tok_off) and names the first differing token."""
    wpref.check(wanted, ids, pos, tok_off, what)


# ---------------------------------------------------------------------------
# the vocabulary of the named cases: the merges in rank order; a string's id is 100 + the index of its merge, a byte's
# 300 + its value.  "abc" is `a bc` here (bc merges first, and abc is ab + c, not a + bc), `abc` greedily and `abc`
# under any_split.  "aaaa": three candidates of one rank, the leftmost first.  CHAIN is rebuilt byte by byte from the
# left, fifteen merges deep.  z^2 .. z^16 make the densest lattice.  "er" has no id (DROP).

CHAIN = b"tokenization_xyz"
assert len(CHAIN) == 16


def _merges():
    m = [(b" ", b"p"), (b" ", b"a"), (b"b", b"c"), (b"a", b"b"), (b"ab", b"c"), (b"a", b"a"), (b"aa", b"aa"), (b"p", b"l"),
         (b"a", b"y"), (b"pl", b"ay"), (b" a", b"b"), (b" p", b"l"), (b" pl", b"ay"), (b"h", b"e"), (b" ", b"t")]
    small = len(m)
    m += [(b" t", b"he"), (b"t", b"h"), (b"th", b"e"), (b"i", b"n"), (b"in", b"g"), (b"e", b"r"), (b"u", b"n"), (b"un", b"play"),
          (b"play", b"ing"), (b"play", b"er"), (b"x", b"x"), (b"b", b"cb"), (b"c", b"b"), (b"te", b"te"), (b"t", b"e"),
          (b"a", b" b"), (b"a", b".b"), (b"a", b"\nb"), (b"q", b"q"), (b"p", b"lay")]
    for k in range(1, len(CHAIN)):
        m.append((CHAIN[:k], CHAIN[k:k + 1]))
    for k in range(2, 17):
        m.append((b"z" * ((k + 1) // 2), b"z" * (k // 2)))
    return m, small


MERGES, N_SMALL = _merges()
# a lead inside, a non-word byte, a newline, not in the vocabulary (qq), and play again (pl + ay made it first)
SKIPPED = {30: "lead inside", 31: "non-word byte", 32: "newline", 33: "not in vocab", 34: "ambiguous"}
DROPPED = (b"er",)


def _vocab_dict(merges):
    d = {bytes([b]): 300 + b for b in range(256)}
    for k, (l, r) in enumerate(merges):
        if l + r != b"qq":
            d.setdefault(l + r, 100 + k)
    return d


VOCAB = _vocab_dict(MERGES)
SMALL_VOCAB = _vocab_dict(MERGES[:N_SMALL])     # 15 strings: its states fit the 16-bit record form


def byte_table(kind):
    b = np.full(256, DROP, dtype=np.int64)
    if kind == "all":                                           # every byte has an id, but y, Y and the comma
        b[:] = 300 + np.arange(256)
        for c in b"yY,":
            b[c] = DROP
    return b


def vocab(max_word=64, fold=False, bytes_="all", lead=0x20, any_split=False, word=CASE_WORD):
    return Vocab(VOCAB, MERGES, lead, max_word, word, fold, byte_table(bytes_), any_split, DROPPED)


def small_vocab(max_word=64, bytes_="all", lead=0x20):
    return Vocab(SMALL_VOCAB, MERGES[:N_SMALL], lead, max_word, CASE_WORD, False, byte_table(bytes_), False, ())


WORDS = uniref.WORDS + [CHAIN, CHAIN[:7], b"aaaa", b"aaa", b"bcb", b"tete", b"the", b"player", b"z" * 16, b"z" * 21, b"xx", b"xxx"]
SEPS = [b" ", b" ", b" ", b" ", b".", b", ", b"! ", b"\n", b"  ", b" . "]


def filler(n, seed):
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n:
        out += WORDS[int(rng.integers(len(WORDS)))] + SEPS[int(rng.integers(len(SEPS)))]
    return np.frombuffer(bytes(out[:n]), dtype=np.uint8).copy()


def text(s, n=None):
    buf = spaced(n or len(s))
    put(buf, 0, s)
    return buf


def dotted(n):
    return np.full(n, ord("."), dtype=np.uint8)


def at_edge(edge, left, word, n=None, fill=spaced):
    """`word` alone in spaces (or dots) with `left` of its bytes in front of position `edge`."""
    buf = fill(n or edge + TILE)
    put(buf, edge - left, word)
    return buf


def abab(L):
    return (b"ab" * (L // 2 + 1))[:L]


SMALL = (0, 1, 4095, 4096, 4097)
SIZES = {"t3": 3 * TILE + 17, "t65": 65 * TILE + 1, "t130": 130 * TILE + 5}
HALO = 64
G = 64 * TILE
DOC_OWNED = 66 * TILE + 123
DOC_SHAPES = wpref.DOC_SHAPES
EMPTY_RUN = wpref.EMPTY_RUN


def doc_offsets(data, n_owned, v, shape):
    """wpref.doc_offsets with the lead rule: every offset moved out of the words."""
    o = wpref.doc_offsets(data, n_owned, v, shape).astype(np.int64).tolist()
    return np.array(sorted(to_boundary(data, n_owned, c, v) for c in o), dtype=np.uint64)


def cases():
    """name -> (data uint8[n_avail], n_owned, Vocab, offsets or None)."""
    out = {}
    v, va, vn = vocab(), vocab(any_split=True), vocab(lead=-1)
    for n in SMALL:
        out[f"n{n}"] = (filler(n, 100 + n), n, v, None)
    for name, n in SIZES.items():
        data = filler(n + HALO, 7)
        put(data, n - 1, b".")
        out[name] = (data, n, v, None)
    out["t3-any-split"] = (out["t3"][0], out["t3"][1], va, None)
    out["t3-no-lead"] = (out["t3"][0], out["t3"][1], vn, None)
    s = b"abc.abc xabc abcab bcb.abcb"
    out["greedy-vs-bpe"] = (text(s), len(s), v, None)
    out["split-matters"] = (text(s), len(s), v, None)
    out["split-any"] = (text(s), len(s), va, None)
    s = b"aaaa.aaa aa aaaaa.aaaaaaaa tete"
    out["tie-leftmost"] = (text(s), len(s), v, None)
    s = CHAIN + b"." + CHAIN[:9] + b" " + CHAIN[1:] + b"." + CHAIN + CHAIN
    out["chain"] = (text(s), len(s), v, None)
    s = b"player.er er unplayer"
    out["part-drop"] = (text(s), len(s), v, None)
    # words across a tile edge and a group edge; the second tile's ids depend on the bytes in front of the edge
    for name, edge in (("edge", TILE), ("group", G)):
        n = edge + TILE
        out[f"{name}-piece-across"] = (at_edge(edge, 2, b"playing", n), n, v, None)
        out[f"{name}-lookback-bc"] = (at_edge(edge, 1, b"abc", n), n, v, None)
        out[f"{name}-lookback-un"] = (at_edge(edge, 2, b"unplaying", n), n, v, None)
        out[f"{name}-chain"] = (at_edge(edge, 9, CHAIN, n, dotted), n, v, None)    # (in dots: ` t` would break the chain)
        out[f"{name}-dense"] = (at_edge(edge, 37, b"z" * 60, n), n, v, None)
    out["dense"] = (text(b"..zzzzzzzzzzzzzzzz." + b"z" * 63 + b" " + b"z" * 64 + b" zzz", 256), 256, v, None)
    # lead cases: at position 0; at a tile's last byte with the run in the next tile; at the region's left edge of the
    # second tile; two in a row; in front of a non-word byte; no lead at all
    s = b" ab  ab . ab a.ab  play .play"
    out["lead-at-0"] = (text(s), len(s), v, None)
    out["lead-none"] = (text(s), len(s), vn, None)
    out["lead-tile-last"] = (at_edge(TILE, 1, b" play", 2 * TILE, dotted), 2 * TILE, v, None)
    out["lead-tile-last-ab"] = (at_edge(TILE, 1, b" ab", 2 * TILE, dotted), 2 * TILE, v, None)
    out["lead-region-edge"] = (at_edge(TILE - 256, 0, b" play", 2 * TILE, dotted), 2 * TILE, v, None)
    out["lead-region-edge-in"] = (at_edge(TILE - 256, 1, b" play", 2 * TILE, dotted), 2 * TILE, v, None)
    out["lead-two"] = (at_edge(TILE, 1, b"  ab", 2 * TILE, dotted), 2 * TILE, v, None)
    out["lead-word-after-word"] = (at_edge(TILE, 2, b"ab ab ab", 2 * TILE, dotted), 2 * TILE, v, None)
    for mw in (1, 2, 63, 64, 65, 255):                          # a word of exactly the cap, and one more
        buf = spaced(TILE + 600)
        at = 5
        for L in (mw - 1, mw, mw + 1, mw + 2):
            if L > 0:
                put(buf, at, b"." + abab(L) + b".")
                at += L + 3
        put(buf, at, abab(mw - 1))                              # (with its lead: the cap exactly)
        put(buf, TILE - mw // 2 - 1, b"." + abab(mw))           # ... and across the tile edge
        out[f"cap{mw}"] = (buf, TILE + 600, vocab(max_word=mw), None)
        out[f"cap{mw}-over-edge"] = (at_edge(TILE, mw // 2 + 1, abab(mw + 1), fill=dotted), 2 * TILE, vocab(max_word=mw), None)
        out[f"cap{mw}-lead-over-edge"] = (at_edge(TILE, mw // 2 + 1, b" " + abab(mw), fill=dotted), 2 * TILE, vocab(max_word=mw), None)
    out["long-word"] = (at_edge(TILE, 100, abab(2 * TILE + 200), 5 * TILE), 5 * TILE, vocab(max_word=255), None)
    buf = dotted(2 * TILE)
    buf[0:TILE:2] = ord("a")                                    # 2048 one-byte words in one tile
    buf[TILE + 1::2] = ord("y")                                 # ... and 2048 whose byte has no id
    out["one-byte-words"] = (buf, 2 * TILE, v, None)
    # the end of the input: a word that ends at n_owned; records that end in the halo must not be used
    buf = filler(TILE + 300 + HALO, 11)
    put(buf, TILE + 290, b" unplaying")
    put(buf, TILE + 300, b" ")
    out["end-at-owned"] = (buf, TILE + 300, v, None)
    buf = buf.copy()
    put(buf, TILE + 290, b"   playing  ")
    out["end-in-halo"] = (buf, TILE + 297, v, None)             # "play|ing": "play" ends at n_owned
    out["end-piece-in-halo"] = (buf, TILE + 295, v, None)       # "pl|aying": "play" ends in the halo, "pl" does not
    out["end-on-tile"] = (at_edge(TILE, 2, b"playing", TILE + HALO), TILE, v, None)
    out["alldrop-bytes"] = (filler(TILE + 17, 5), TILE + 17, vocab(bytes_="none"), None)
    folded = filler(2 * TILE + 5, 9)
    up = (folded >= 97) & (folded <= 122) & (np.arange(folded.size) % 3 == 0)
    folded[up] -= 32
    out["folded"] = (folded, folded.size, vocab(fold=True), None)
    vs = small_vocab()                                          # the 16-bit record form: the small vocabulary
    out["w2-n4097"] = (out["n4097"][0], 4097, vs, None)
    out["w2-t3"] = (out["t3"][0], out["t3"][1], vs, None)
    out["w2-t65"] = (out["t65"][0], out["t65"][1], vs, None)
    out["w2-edge-lookback-bc"] = (out["edge-lookback-bc"][0], 2 * TILE, vs, None)
    out["w2-lead-tile-last"] = (out["lead-tile-last"][0], 2 * TILE, vs, None)
    d3 = out["t3"][0]
    out["w2-docs"] = (d3, out["t3"][1], vs, doc_offsets(d3, out["t3"][1], vs, "cut"))
    data = filler(DOC_OWNED + HALO, 13)
    put(data, DOC_OWNED - 1, b".")
    for shape in DOC_SHAPES:
        d = data
        if shape == "nothing":
            d = data.copy()
            d[(d >= 97) & (d <= 122)] = ord("y")
        out[f"docs-{shape}"] = (d, DOC_OWNED, v, doc_offsets(d, DOC_OWNED, v, shape))
    return out


_MEMO = {}


def _cases():
    if "cases" not in _MEMO:
        _MEMO["cases"] = cases()
    return _MEMO["cases"]


def names():
    return tuple(_cases())


def case(name):
    return _cases()[name]


def _tokens(form, data, no, v):
    """(ids, positions) of one form over an input, computed once per distinct input and vocabulary."""
    key = (form, id(data), no, id(v))
    if key not in _MEMO:
        _MEMO[key] = want(data, no, v)[:2] if form == "records" else by_strings(data, no, v)[:2]
    return _MEMO[key]


def want_of(name, form="records"):
    """(ids, positions, tok_off) of a named case, computed once (tok_off is a search in the positions)."""
    data, no, v, off = case(name)
    ids, pos = _tokens(form, data, no, v)
    tok_off = None if off is None else np.searchsorted(pos.astype(np.int64), np.asarray(off, dtype=np.int64), side="left").astype(np.uint64)
    return ids, pos, tok_off


def random_merges(rng, letters, n_merges, max_len, lead=None):
    """A random merge list as a trainer would make one: every merge joins two symbols that exist by then."""
    symbols = [bytes([c]) for c in letters] + ([bytes([lead])] if lead is not None else [])
    merges = []
    for _ in range(20 * n_merges):
        if len(merges) == n_merges:
            break
        l, r = symbols[int(rng.integers(len(symbols)))], symbols[int(rng.integers(len(symbols)))]
        if len(l) + len(r) > max_len or (lead is not None and (lead in r or lead in l[1:])):
            continue
        merges.append((l, r))
        if l + r not in symbols:
            symbols.append(l + r)
    return merges


def random_case(seed):
    """A small seeded case with a merge list of its own over a few letters: random cap, lead or none, either split
    form, coarse ranks (ties between different strings), some ids DROP -> (data, n_owned, Vocab)."""
    rng = np.random.default_rng(seed)
    lead = 0x20 if rng.integers(5) else -1
    merges = random_merges(rng, b"ab" if seed % 3 else b"abc", int(rng.integers(8, 40)), 8, lead if lead >= 0 else None)
    d = {bytes([b]): 300 + b for b in b"abcx .A"}
    if rng.integers(2):
        del d[b"a"]
    drop = set()
    for k, (l, r) in enumerate(merges):
        d.setdefault(l + r, 100 + k)
        if rng.integers(5) == 0:
            drop.add(l + r)
    v = Vocab(d, merges, lead, int(rng.choice([1, 2, 3, 5, 8] + [64] * 7)), CASE_WORD, bool(rng.integers(4) == 0), None,
              bool(rng.integers(6) == 0), drop, int(rng.choice([1, 1, 3])))
    n = int(rng.integers(0, 90))
    alphabet = np.frombuffer(b"aaaaaabbbbbbcx .A", dtype=np.uint8)
    data = alphabet[rng.integers(0, alphabet.size, size=n + 8)].copy()
    return data, n, v


# the small log of the surface tests, ids written out by hand: GPT-2's form, `Ġ` is the space.  Merges in rank order;
# a token's id is its place in LOG_TOKENS.
LOG_TOKENS = ["t", "h", "e", "p", "l", "a", "y", "r", "s", "x", ".", "Ġ", "Ċ", "th", "the", "Ġthe", "ay", "pl", "play", "Ġplay", "er", "Ġa"]
LOG_MERGES = [("t", "h"), ("th", "e"), ("Ġ", "the"), ("a", "y"), ("p", "l"), ("pl", "ay"), ("Ġ", "play"), ("e", "r"), ("Ġ", "a")]
LOG = b"the player plays.\nthe  play ax\n\n a.\n"
#          the Ġplay er Ġplay s  .  Ċ | the Ġ Ġplay Ġa x Ċ | Ċ | Ġa . Ċ
LOG_IDS = [14, 19, 20, 19, 8, 10, 12, 14, 11, 19, 21, 9, 12, 12, 21, 10, 12]
LOG_POS = [0, 3, 8, 10, 15, 16, 17, 0, 3, 4, 9, 11, 12, 0, 0, 2, 3]      # relative to the line
LOG_TOK_OFF = [0, 7, 13, 14, 17]
