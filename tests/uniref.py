"""Host reference for the Unigram passes (the checker, never the product): THE RULE of include/pfac.h held twice, and
the cases that tests/test_unigram_ref.py (no GPU) and tests/test_gpu_unigram.py share.

The rule: a word is a maximal run of word bytes inside [0, n_owned).  Its nodes are 0..n; a record (p, s) inside a word
of at most max_word bytes is a piece edge carrying the first (id, score) of s at the word's start, the continuation
ones elsewhere, unless that id is DROP; every byte is a byte edge with byte_score.  best[j] is the maximum over the
edges into j; of equal candidates the smaller i wins, and of a one-byte piece and the byte edge the piece.  The path is
the backtrack from n.  A piece edge emits its id at its first byte; a run of byte edges emits one unk at its first byte,
or with unk == DROP every byte edge its byte id; a byte outside words emits its byte id.

  by_records   a forward ("push") DP over a record list in the order the heap gives it: (position, length).
  by_words     a per-word memoised ("pull") search that never sees a record: it tries the vocabulary's strings from a
               dict, and counts the optimal paths of every word on the way.

Both return (ids int32, positions uint32, tok_off uint64 or None).  No expectation comes from the device."""
import numpy as np

import wpref
from wpref import DROP, TILE, put, spaced

NEG = -(1 << 62)
PREFIX = "▁".encode()
DEFAULT_WORD = bytes(b for b in range(256) if b not in b"\t\n\v\f\r ")


class Vocab:
    """A vocabulary as the rule sees it: entry k = (piece, integer score) has id k; `▁x` is the word-initial piece x, a
    plain `x` the continuation piece.  Written apart from phfpfac_amd.table.unigram_table, which test_unigram_ref.py
    holds against it."""

    def __init__(self, entries, unk=0, max_word=100, word=DEFAULT_WORD, fold=False, byte_ids=None, byte_score=-10, prefix=PREFIX):
        self.entries = [(bytes(e), int(s)) for e, s in entries]
        self.max_word, self.fold, self.prefix = int(max_word), bool(fold), bytes(prefix)
        self.unk, self.byte_score = int(unk), int(byte_score)
        self.word = np.zeros(256, dtype=bool)
        self.word[np.frombuffer(bytes(word), dtype=np.uint8)] = True
        self.byte_ids = np.full(256, DROP, dtype=np.int64) if byte_ids is None else np.asarray(byte_ids, dtype=np.int64).copy()
        self.first, self.cont, self.skipped = {}, {}, []
        for k, (e, s) in enumerate(self.entries):
            is_first = e.startswith(self.prefix)
            piece = e[len(self.prefix):] if is_first else e
            if self.fold:
                piece = piece.lower()
            control = len(e) >= 2 and e[:1] == b"<" and e[-1:] == b">"
            d = self.first if is_first else self.cont
            if piece and not control and self.prefix not in piece and all(self.word[b] for b in piece) and piece not in d:
                d[piece] = (k, s)
            else:
                self.skipped.append((k, e))
        self.pieces = sorted(set(self.first) | set(self.cont))
        self.longest = max((len(p) for p in self.pieces), default=0)

    def quad(self, piece):
        f, c = self.first.get(piece, (DROP, 0)), self.cont.get(piece, (DROP, 0))
        return f[0], c[0], f[1], c[1]

    def word_set(self):
        w = [0, 0, 0, 0]
        for b in np.flatnonzero(self.word).tolist():
            w[b >> 6] |= 1 << (b & 63)
        return np.array(w, dtype=np.uint64)

    def bound_ok(self):
        top = max([abs(self.byte_score)] + [abs(s) for d in (self.first, self.cont) for _, s in d.values()])
        return top * (self.max_word + 1) < 2**31


def records(data, n_owned, v):
    """Every occurrence of a stripped piece that starts below n_owned, in heap order -> (pos, lens, piece index)."""
    return wpref.records(data, n_owned, v)


def _words(data, n, v):
    W = v.word[np.asarray(data, dtype=np.uint8)[:n]]
    prev = np.concatenate([[False], W[:-1]])
    nxt = np.concatenate([W[1:], [False]])
    return W, np.flatnonzero(W & ~prev), np.flatnonzero(W & ~nxt) + 1


def _emit(val, data, a, path, v):
    """path: (start in the word, id or None for a byte edge), ascending."""
    run = False
    for st, tid in path:
        if tid is not None:
            val[a + st] = tid
            run = False
        else:
            if v.unk >= 0:
                if not run:
                    val[a + st] = v.unk
            else:
                val[a + st] = v.byte_ids[data[a + st]]
            run = True


def _finish(val, off):
    positions = np.flatnonzero(val != DROP)
    tok_off = None if off is None else np.searchsorted(positions, np.asarray(off, dtype=np.int64), side="left").astype(np.uint64)
    return val[positions].astype(np.int32), positions.astype(np.uint32), tok_off


def by_records(data, n_owned, pos, lens, idx, v, off=None):
    """(a): the forward DP over the records as the heap orders them."""
    data = np.asarray(data, dtype=np.uint8)
    n = int(n_owned)
    W, starts, ends = _words(data, n, v)
    val = np.full(n, DROP, dtype=np.int64)
    val[~W] = v.byte_ids[data[:n][~W]]
    quads = [v.quad(p) for p in v.pieces]
    pos_l, len_l, idx_l = (np.asarray(x, dtype=np.int64).tolist() for x in (pos, lens, idx))
    first_rec = np.searchsorted(np.asarray(pos, dtype=np.int64), starts, side="left").tolist()
    n_rec, bs = len(pos_l), v.byte_score
    for a, b, k in zip(starts.tolist(), ends.tolist(), first_rec):
        nn = b - a
        best = [NEG] * (nn + 1)
        ch = [None] * (nn + 1)
        best[0] = 0
        pieces_on = nn <= v.max_word
        for i in range(nn):
            bi = best[i]
            while pieces_on and k < n_rec and pos_l[k] <= a + i:
                if pos_l[k] == a + i and i + len_l[k] <= nn:
                    q = quads[idx_l[k]]
                    tid, sc = (q[0], q[2]) if i == 0 else (q[1], q[3])
                    if tid != DROP and bi + sc > best[i + len_l[k]]:
                        best[i + len_l[k]] = bi + sc
                        ch[i + len_l[k]] = (len_l[k], tid)
                k += 1
            if bi + bs > best[i + 1]:
                best[i + 1] = bi + bs
                ch[i + 1] = (1, None)
        path, j = [], nn
        while j > 0:
            L, tid = ch[j]
            path.append((j - L, tid))
            j -= L
        _emit(val, data, a, path[::-1], v)
    return _finish(val, off)


def by_words(data, n_owned, v, off=None, stats=None):
    """(b): word by word, a memoised pull over the vocabulary's strings.  `stats` (a dict) gathers, per call: the
    optimal-path count of every word ("paths"), the words over the cap, the unk runs and the byte-fallback tokens."""
    data = np.asarray(data, dtype=np.uint8)
    n = int(n_owned)
    raw = bytes(data[:n])
    W, starts, ends = _words(data, n, v)
    val = np.full(n, DROP, dtype=np.int64)
    val[~W] = v.byte_ids[data[:n][~W]]
    st = {"paths": [], "over": 0, "unk_runs": 0, "fallback": 0}
    for a, b in zip(starts.tolist(), ends.tolist()):
        w = raw[a:b].lower() if v.fold else raw[a:b]
        nn = b - a
        over = nn > v.max_word
        st["over"] += over
        memo = {0: (0, None, 1)}                                # node -> (best, chosen edge (length, id), optimal paths)
        for j in range(1, nn + 1):
            cands = []                                          # in the order of the tie rule: longest first, the byte edge last
            if not over:
                for L in range(min(j, v.longest), 0, -1):
                    hit = (v.first if j == L else v.cont).get(w[j - L:j])
                    if hit is not None:
                        cands.append((memo[j - L][0] + hit[1], (L, hit[0]), memo[j - L][2]))
            cands.append((memo[j - 1][0] + v.byte_score, (1, None), memo[j - 1][2]))
            top = max(c[0] for c in cands)
            win = next(c for c in cands if c[0] == top)
            memo[j] = (top, win[1], sum(c[2] for c in cands if c[0] == top))
        st["paths"].append(memo[nn][2])
        path, j = [], nn
        while j > 0:
            L, tid = memo[j][1]
            path.append((j - L, tid))
            j -= L
        path = path[::-1]
        _emit(val, data, a, path, v)
        for i, (s0, tid) in enumerate(path):
            if tid is None:
                if v.unk >= 0:
                    st["unk_runs"] += i == 0 or path[i - 1][1] is not None
                else:
                    st["fallback"] += val[a + s0] != DROP
    if stats is not None:
        stats.update(st)
    return _finish(val, off)


def greedy_words(data, n_owned, v):
    """MaxMatch over the same halves (what tokenize_lines makes of such a vocabulary): the longest piece at the cursor,
    a byte edge where there is none.  Only to count where Viterbi differs."""
    data = np.asarray(data, dtype=np.uint8)
    n = int(n_owned)
    raw = bytes(data[:n])
    W, starts, ends = _words(data, n, v)
    val = np.full(n, DROP, dtype=np.int64)
    val[~W] = v.byte_ids[data[:n][~W]]
    for a, b in zip(starts.tolist(), ends.tolist()):
        w = raw[a:b].lower() if v.fold else raw[a:b]
        c, path = 0, []
        while c < len(w):
            hit = None
            if len(w) <= v.max_word:
                for L in range(min(len(w) - c, v.longest), 0, -1):
                    hit = (v.cont if c else v.first).get(w[c:c + L])
                    if hit is not None:
                        path.append((c, hit[0]))
                        c += L
                        break
            if hit is None:
                path.append((c, None))
                c += 1
        _emit(val, data, a, path, v)
    return _finish(val, None)


def want(data, n_owned, v, off=None):
    """What the passes deliver for this input: by_records over every record of the scan."""
    p, l, k = records(data, n_owned, v)
    return by_records(data, n_owned, p, l, k, v, off)


boundaries_ok = wpref.boundaries_ok


def check(wanted, ids, pos=None, tok_off=None, what="unigram"):
    """Holds a result against wanted = (ids, positions, tok_off) and names the first differing token."""
    wpref.check(wanted, ids, pos, tok_off, what)


# ---------------------------------------------------------------------------
# the vocabulary of the named cases (entry k has id k; scores are integers).  1..4 are the issue's example: "abc" is
# "▁ab c" (-6) greedily and "▁a bc" (-3) by Viterbi.  ▁t / e / ▁te tie at "te" (the longer edge wins); q and ▁q score
# what a byte edge scores (the piece wins).  ing, er, s are continuation-only: a word that is one of them has no edge at
# all.  x, y and the capitals have no piece.  z .. z^16 in both halves make the densest lattice.

def _entries():
    P = PREFIX
    e = [(b"<unk>", 0), (P + b"ab", -1), (b"c", -5), (P + b"a", -2), (b"bc", -1), (P + b"play", -3), (b"play", -4), (b"ing", -2),
         (b"er", -2), (b"s", -1), (P + b"un", -2), (P + b"the", -2), (b"a", -3), (b"b", -3), (P + b"b", -3), (b"ab", -2),
         (P + b"c", -4), (P + b"t", -2), (b"e", -1), (P + b"te", -3), (b"q", -10), (P + b"q", -10), (P, -1), (b"a" + P + b"b", -1),
         (b"pl.ay", -1), (b"", -1), (b"c", -1), (P + b"pl", -4), (b"ay", -3)]
    for k in range(1, 17):
        e.append((P + b"z" * k, -(3 + (k * 7) % 5)))
        e.append((b"z" * k, -(2 + (k * 3) % 7)))
    return e


ENTRIES = _entries()
SKIPPED = [0, 22, 23, 24, 25, 26]       # <unk>, the bare prefix, a prefix inside, a non-word byte, "", the second "c"
CASE_WORD = wpref.DEFAULT_WORD          # [0-9A-Za-z_]: punctuation is outside words and has byte ids
UNK = 0
BYTE_SCORE = -10


# ... and a vocabulary of 14 distinct stripped strings: its states fit the 16-bit record form
SMALL_ENTRIES = [e for e in ENTRIES[:22] if e[0] not in (b"b", PREFIX + b"b", b"a", b"ab", PREFIX + b"c")]


def byte_table(kind):
    b = np.full(256, DROP, dtype=np.int64)
    if kind == "punct":
        b[ord(".")], b[ord("!")] = 200, 201
    elif kind == "fallback":                                    # every byte has an id, but y, Y, the comma and the space
        b[:] = 300 + np.arange(256)
        for c in b"yY, ":
            b[c] = DROP
    return b


def vocab(max_word=100, fold=False, bytes_="punct", unk=UNK, word=CASE_WORD):
    return Vocab(ENTRIES, unk, max_word, word, fold, byte_table(bytes_), BYTE_SCORE)


def small_vocab(max_word=100, bytes_="punct", unk=UNK):
    return Vocab(SMALL_ENTRIES, unk, max_word, CASE_WORD, False, byte_table(bytes_), BYTE_SCORE)


def fallback(max_word=100, fold=False):
    return vocab(max_word, fold, "fallback", DROP)


WORDS = [b"play", b"playing", b"player", b"plays", b"unplaying", b"the", b"a", b"ab", b"abc", b"abcab", b"b", b"c", b"cc", b"x",
         b"playx", b"ing", b"abx", b"theplay", b"A", b"pl", b"te", b"tee", b"q", b"xq", b"qx", b"xxplay", b"playxxing", b"zzzzz",
         b"abzzzzzzzzzzzzzzzzzzab", b"s", b"y", b"xyx", b"play" * 3, b"bcbc", b"tete"]
SEPS = [b" ", b" ", b" ", b".", b", ", b"! ", b"\n", b"  "]


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


def at_edge(edge, left, word, n=None):
    """`word` alone in spaces with `left` of its bytes in front of position `edge`."""
    buf = spaced(n or edge + TILE)
    put(buf, edge - left, word)
    return buf


def abab(L):
    return (b"ab" * (L // 2 + 1))[:L]


SMALL = (0, 1, 15, 16, 17, 4095, 4096, 4097)
SIZES = {"t3": 3 * TILE + 17, "t65": 65 * TILE + 1, "t130": 130 * TILE + 5}
HALO = 64
G = 64 * TILE
DOC_OWNED = 66 * TILE + 123
DOC_SHAPES = wpref.DOC_SHAPES


def cases():
    """name -> (data uint8[n_avail], n_owned, Vocab, offsets or None)."""
    out = {}
    v, fb = vocab(), fallback()
    for n in SMALL:
        out[f"n{n}"] = (filler(n, 100 + n), n, v, None)
    for name, n in SIZES.items():
        data = filler(n + HALO, 7)
        put(data, n - 1, b" ")
        out[name] = (data, n, v, None)
    out["t3-fallback"] = (out["t3"][0], out["t3"][1], fb, None)
    out["greedy-vs-viterbi"] = (text(b"abc abc xabc abcab"), 18, v, None)
    out["tie-longer-edge"] = (text(b"te tee tete t e"), 15, v, None)
    out["tie-piece-or-byte"] = (text(b"q qq xq qx aq"), 13, v, None)
    out["role-drop"] = (text(b"ing s er e ing er"), 17, v, None)        # no record of these words has an id in its place
    out["unk-runs"] = (text(b"xplay playxing playx x xxplay playxxing xx"), 42, v, None)
    out["unk-runs-fallback"] = (text(b"xplay playxing playx x xxplay playyxing yy y"), 44, fb, None)
    # words across a tile edge and a group edge: the best cut has a piece across the edge; the second tile's ids
    # depend on the bytes in front of the edge (bc / playing / zz.. are other tokens, or none, at a word's start)
    for name, edge in (("edge", TILE), ("group", G)):
        n = edge + TILE
        out[f"{name}-piece-across"] = (at_edge(edge, 2, b"playing", n), n, v, None)
        out[f"{name}-lookback-bc"] = (at_edge(edge, 1, b"abc", n), n, v, None)
        out[f"{name}-lookback-un"] = (at_edge(edge, 2, b"unplaying", n), n, v, None)
        out[f"{name}-lookback-x"] = (at_edge(edge, 1, b"xplays", n), n, v, None)
        out[f"{name}-dense"] = (at_edge(edge, 37, b"z" * 100, n), n, v, None)
    buf = at_edge(TILE, 3, b"playing", 3 * TILE)                 # every tile edge of the input at once
    put(buf, 2 * TILE - 1, b"abc")
    put(buf, TILE - 20, b"xx")
    out["edges-fallback"] = (buf, 3 * TILE, fb, None)
    for mw in (1, 63, 64, 65):                                   # a word of exactly the cap, and one more
        buf = spaced(TILE + 300)
        at = 5
        for L in (mw - 1, mw, mw + 1, mw + 2):
            if L > 0:
                put(buf, at, abab(L))
                at += L + 3
        put(buf, TILE - mw // 2 - 1, abab(mw))                   # ... and across the tile edge
        put(buf, TILE + mw + 3, b"z" * mw)
        out[f"cap{mw}"] = (buf, TILE + 300, vocab(max_word=mw), None)
        out[f"cap{mw}-over-edge"] = (at_edge(TILE, mw // 2 + 1, abab(mw + 1)), 2 * TILE, vocab(max_word=mw), None)
    vmax = vocab(max_word=4095)
    out["cap4095"] = (at_edge(TILE, 95, abab(4095), 3 * TILE), 3 * TILE, vmax, None)
    out["cap4095-over"] = (at_edge(TILE, 96, abab(4096), 3 * TILE), 3 * TILE, vmax, None)
    out["cap4095-filler"] = (out["t3"][0], out["t3"][1], vmax, None)
    out["three-tiles"] = (at_edge(TILE, 100, abab(2 * TILE + 200), 5 * TILE), 5 * TILE, vmax, None)
    out["three-tiles-fallback"] = (out["three-tiles"][0], 5 * TILE, fallback(4095), None)
    buf = spaced(2 * TILE)
    buf[0:TILE:2] = ord("a")                                    # 2048 one-byte words in one tile
    buf[TILE + 1::2] = ord("x")                                 # ... and 2048 with no piece
    out["one-byte-words"] = (buf, 2 * TILE, v, None)
    out["dense"] = (text(b"  " + b"z" * 100 + b" " + b"z" * 101 + b" zzz", 256), 256, v, None)
    out["dense-255"] = (text(b" " + b"z" * 255, 300), 300, vocab(max_word=255), None)
    out["dense-256"] = (text(b" " + b"z" * 256, 300), 300, vocab(max_word=256), None)
    # the end of the input: a word that ends at n_owned; records that end in the halo must not be used
    buf = filler(TILE + 300 + HALO, 11)
    put(buf, TILE + 290, b" unplaying")
    put(buf, TILE + 300, b" ")
    out["end-at-owned"] = (buf, TILE + 300, v, None)
    buf = buf.copy()
    put(buf, TILE + 290, b"   playing  ")
    out["end-in-halo"] = (buf, TILE + 297, v, None)             # "play|ing": "play" ends at n_owned
    out["end-piece-in-halo"] = (buf, TILE + 295, v, None)       # "pl|aying": "play" ends in the halo, "pl" does not
    out["end-on-tile"] = (at_edge(TILE, 2, b"playing", TILE + HALO), TILE, v, None)    # "pl|aying" at a tile's end
    out["alldrop-bytes"] = (filler(TILE + 17, 5), TILE + 17, vocab(bytes_="none"), None)
    folded = filler(2 * TILE + 5, 9)
    up = (folded >= 97) & (folded <= 122) & (np.arange(folded.size) % 3 == 0)
    folded[up] -= 32
    out["folded"] = (folded, folded.size, fallback(fold=True), None)
    out["folded-unk"] = (folded, folded.size, vocab(fold=True), None)
    vs = small_vocab()                                          # the 16-bit record form: the small vocabulary
    out["w2-n4097"] = (out["n4097"][0], 4097, vs, None)
    out["w2-t3"] = (out["t3"][0], out["t3"][1], vs, None)
    out["w2-t3-fallback"] = (out["t3"][0], out["t3"][1], small_vocab(bytes_="fallback", unk=DROP), None)
    out["w2-t65"] = (out["t65"][0], out["t65"][1], vs, None)
    out["w2-edge-lookback-un"] = (out["edge-lookback-un"][0], 2 * TILE, vs, None)
    out["w2-edge-lookback-bc"] = (out["edge-lookback-bc"][0], 2 * TILE, vs, None)
    out["w2-group-piece-across"] = (out["group-piece-across"][0], G + TILE, vs, None)
    out["w2-cap4095"] = (at_edge(TILE, 95, (b"abc" * 1400)[:4095], 3 * TILE), 3 * TILE, small_vocab(max_word=4095), None)
    d3 = out["t3"][0]
    out["w2-docs"] = (d3, out["t3"][1], vs, wpref.doc_offsets(d3, out["t3"][1], vs, "cut"))
    data = filler(DOC_OWNED + HALO, 13)
    put(data, DOC_OWNED - 1, b" ")
    for shape in DOC_SHAPES:
        d = data
        if shape == "nothing":
            d = data.copy()
            d[(d >= 97) & (d <= 122)] = ord("x")
        out[f"docs-{shape}"] = (d, DOC_OWNED, v, wpref.doc_offsets(d, DOC_OWNED, v, shape))
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
        _MEMO[key] = want(data, no, v)[:2] if form == "records" else by_words(data, no, v)[:2]
    return _MEMO[key]


def want_of(name, form="records"):
    """(ids, positions, tok_off) of a named case, computed once (tok_off is a search in the positions)."""
    data, no, v, off = case(name)
    ids, pos = _tokens(form, data, no, v)
    tok_off = None if off is None else np.searchsorted(pos.astype(np.int64), np.asarray(off, dtype=np.int64), side="left").astype(np.uint64)
    return ids, pos, tok_off


def random_case(seed):
    """A small seeded case with a vocabulary of its own: short pieces over a few letters, scores in a narrow range (so
    that totals tie), random halves, random cap, either unk mode -> (data, n_owned, Vocab)."""
    rng = np.random.default_rng(seed)
    letters = b"abcx"
    ents = [(b"<unk>", 0)]
    for _ in range(int(rng.integers(3, 14))):
        p = bytes(letters[int(i)] for i in rng.integers(0, 3, size=int(rng.integers(1, 5))))
        ents.append(((PREFIX if rng.integers(2) else b"") + p, -int(rng.integers(1, 5))))
    mode = int(rng.integers(3))
    bt = byte_table("fallback" if mode == 0 else "punct")
    if mode == 0 and rng.integers(2):
        bt[ord("a")] = DROP
    v = Vocab(ents, DROP if mode == 0 else UNK, int(rng.choice([1, 2, 3, 5, 8, 100])), CASE_WORD, bool(rng.integers(4) == 0), bt,
              -int(rng.integers(3, 7)))
    n = int(rng.integers(0, 90))
    alphabet = np.frombuffer(b"aabbccx  .A", dtype=np.uint8)
    data = alphabet[rng.integers(0, alphabet.size, size=n + 8)].copy()
    return data, n, v


# the small log of the surface tests, ids written out by hand against LOG_VOCAB (entry k has id k; the default word
# set: everything but whitespace, so the dot belongs to its word)
LOG_VOCAB = [("<unk>", 0.0), ("▁the", -2.0), ("▁play", -3.0), ("er", -2.0), ("ing", -2.5), ("s", -1.0), ("▁un", -2.0), ("play", -4.0),
             ("▁a", -1.5), (".", -1.0), ("▁ab", -1.0), ("c", -5.0), ("bc", -1.0)]
LOG = b"the player plays.\nunplaying abc playx\n\nthe. x\n"
LOG_IDS = [1, 2, 3, 2, 5, 9, 6, 7, 4, 8, 12, 2, 0, 1, 9, 0]
LOG_POS = [0, 4, 8, 11, 15, 16, 0, 2, 6, 10, 11, 14, 18, 0, 3, 5]   # relative to the line
LOG_TOK_OFF = [0, 6, 13, 13, 16]
