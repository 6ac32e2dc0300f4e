"""Host reference for the WordPiece passes (the checker, never the product): the rule of include/pfac.h held twice, and
the cases that tests/test_wordpiece_ref.py (no GPU) and tests/test_gpu_wordpiece.py share.

The rule: a word is a maximal run of word bytes inside [0, n_owned); it is good iff it is at most max_word bytes long
and the picks cover every byte of it.  The first byte of a bad word emits unk; a pick start inside a good word emits
the id of its role (FIRST at a word's start, CONT behind a word byte) unless DROP; a byte outside words and outside
every pick emits byte_ids[byte] unless DROP.

  by_bitmaps   the rule as stated, in numpy, over the picks of the composition: every occurrence of a stripped piece
               (`records`), without those whose piece has no id for its place (`role_filter`), the leftmost-longest
               greedy over them (llref.greedy; per document: restarted at every offset over the records that do not
               cross one).
  by_words     WordPiece as a textbook has it, word by word: longest admissible piece at the cursor, the whole word
               [UNK] if the remainder fails or the word is too long.  It never sees a record, a pick or a bitmap.
               It agrees with by_bitmaps where no pick reaches past n_owned, i.e. where n_owned is a word boundary or
               the end of the buffer; a word that runs into the halo is by_bitmaps' alone (the header says so).

Both return (ids int32, positions uint32, tok_off uint64 or None).  No expectation comes from the device."""
import bisect

import numpy as np

from llref import greedy

DROP = -1
TILE = 4096
DEFAULT_WORD = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ_abcdefghijklmnopqrstuvwxyz"


class Vocab:
    """A vocabulary as the rule sees it: entry k has id k; `##x` is the continuation piece x.  Written apart from
    phfpfac_amd.table.wordpiece_table, which test_wordpiece_ref.py holds against it."""

    def __init__(self, entries, unk, max_word=100, word=DEFAULT_WORD, fold=False, prefix=b"##"):
        self.entries = [bytes(e) for e in entries]
        self.max_word, self.fold, self.prefix = int(max_word), bool(fold), bytes(prefix)
        self.word = np.zeros(256, dtype=bool)
        self.word[np.frombuffer(bytes(word), dtype=np.uint8)] = True
        self.first, self.cont = {}, {}
        self.byte_ids = np.full(256, DROP, dtype=np.int64)
        self.skipped = []
        for k, e in enumerate(self.entries):
            is_cont = e.startswith(self.prefix) and len(e) > len(self.prefix)
            piece = e[len(self.prefix):] if is_cont else e
            if self.fold:
                piece = piece.lower()
            if piece and b"\n" not in piece and all(self.word[b] for b in piece):
                d = self.cont if is_cont else self.first
                if piece not in d:
                    d[piece] = k
                    continue
            elif not is_cont and len(e) == 1 and not self.word[e[0]] and self.byte_ids[e[0]] == DROP:
                self.byte_ids[e[0]] = k
                continue
            self.skipped.append((k, e))
        self.unk = self.entries.index(unk) if isinstance(unk, bytes) else int(unk)
        self.pieces = sorted(set(self.first) | set(self.cont))

    def pair(self, piece):
        return self.first.get(piece, DROP), self.cont.get(piece, DROP)

    def word_set(self):
        w = [0, 0, 0, 0]
        for b in np.flatnonzero(self.word).tolist():
            w[b >> 6] |= 1 << (b & 63)
        return np.array(w, dtype=np.uint64)


def seen(data, v):
    """The bytes the matcher sees: folded under a case fold."""
    data = np.asarray(data, dtype=np.uint8)
    if not v.fold:
        return data
    up = (data >= 65) & (data <= 90)
    return np.where(up, data + 32, data).astype(np.uint8)


def records(data, n_owned, v):
    """Every occurrence of a piece that starts below n_owned and ends inside the buffer, in (position, length) order
    -> (pos, lens, piece index into v.pieces)."""
    s = seen(data, v)
    n = int(s.size)
    pos, lens, idx = [], [], []
    for k, p in enumerate(v.pieces):
        L = len(p)
        if L > n:
            continue
        hit = np.ones(n - L + 1, dtype=bool)
        for j, b in enumerate(p):
            hit &= s[j:n - L + 1 + j] == b
        at = np.flatnonzero(hit)
        at = at[at < n_owned]
        pos.append(at)
        lens.append(np.full(at.size, L, dtype=np.int64))
        idx.append(np.full(at.size, k, dtype=np.int64))
    if not pos:
        z = np.zeros(0, dtype=np.int64)
        return z, z.copy(), z.copy()
    pos, lens, idx = np.concatenate(pos), np.concatenate(lens), np.concatenate(idx)
    order = np.lexsort((lens, pos))
    return pos[order], lens[order], idx[order]


def is_cont(data, pos, v):
    """role(p) == CONT: p > 0 and the byte in front is a word byte (the byte as the caller wrote it)."""
    data = np.asarray(data, dtype=np.uint8)
    pos = np.asarray(pos, dtype=np.int64)
    out = np.zeros(pos.size, dtype=bool)
    nz = pos > 0
    out[nz] = v.word[data[pos[nz] - 1]]
    return out


def role_ids(data, pos, idx, v):
    pairs = np.array([v.pair(p) for p in v.pieces], dtype=np.int64).reshape(-1, 2)
    if not len(pos):
        return np.zeros(0, dtype=np.int64)
    return pairs[idx, is_cont(data, pos, v).astype(np.int64)]


def role_filter(data, pos, lens, idx, v):
    """The records pfac_records_filter_roles keeps, as a mask."""
    data = np.asarray(data, dtype=np.uint8)
    if not len(pos):
        return np.zeros(0, dtype=bool)
    return v.word[data[pos]] & (role_ids(data, pos, idx, v) != DROP)


def picks(data, n_owned, v, off=None):
    """(pos, lens, piece index) of the selection the composition makes: per document where `off` is given."""
    pos, lens, idx = records(data, n_owned, v)
    keep = role_filter(data, pos, lens, idx, v)
    pos, lens, idx = pos[keep], lens[keep], idx[keep]
    if off is None:
        sel, _ = greedy(pos, lens, 0, n_owned)
        return pos[sel], lens[sel], idx[sel]
    off = np.asarray(off, dtype=np.int64)
    d = np.searchsorted(off, pos, side="right") - 1
    d = np.clip(d, 0, off.size - 2)
    inside = pos + lens <= off[d + 1]
    pos, lens, idx = pos[inside], lens[inside], idx[inside]
    sel, _ = greedy(pos, lens, 0, n_owned)         # no kept record crosses an offset: one greedy restarts at each
    return pos[sel], lens[sel], idx[sel]


def by_bitmaps(data, n_owned, ppos, plens, pidx, v, off=None):
    data = np.asarray(data, dtype=np.uint8)
    n = int(n_owned)
    ppos, plens, pidx = (np.asarray(a, dtype=np.int64) for a in (ppos, plens, pidx))
    diff = np.zeros(n + 1, dtype=np.int64)
    np.add.at(diff, ppos, 1)
    np.add.at(diff, np.minimum(ppos + plens, n), -1)
    covered = np.cumsum(diff)[:n] > 0
    W = v.word[data[:n]]
    start = W.copy()
    start[1:] &= ~W[:-1]
    run = np.cumsum(start) - 1                                  # the word of every word byte
    n_runs = int(start.sum())
    length = np.bincount(run[W], minlength=n_runs)
    holes = np.bincount(run[W & ~covered], minlength=n_runs)
    bad_run = (length > v.max_word) | (holes > 0)
    bad = np.zeros(n, dtype=bool)
    bad[W] = bad_run[run[W]]
    val = np.full(n, DROP, dtype=np.int64)
    free = ~W & ~covered
    val[free] = v.byte_ids[data[:n][free]]
    val[start & bad] = v.unk
    rid = role_ids(data, ppos, pidx, v)
    ok = W[ppos] & ~bad[ppos] if ppos.size else np.zeros(0, dtype=bool)
    val[ppos[ok]] = rid[ok]
    positions = np.flatnonzero(val != DROP)
    tok_off = None if off is None else np.searchsorted(positions, np.asarray(off, dtype=np.int64), side="left").astype(np.uint64)
    return val[positions].astype(np.int32), positions.astype(np.uint32), tok_off


def by_words(data, n_owned, v, off=None):
    raw = bytes(np.asarray(data, dtype=np.uint8)[:int(n_owned)])
    ids, positions = [], []
    longest = max((len(p) for p in v.pieces), default=0)
    i, n = 0, len(raw)
    while i < n:
        if not v.word[raw[i]]:
            if v.byte_ids[raw[i]] != DROP:
                ids.append(int(v.byte_ids[raw[i]]))
                positions.append(i)
            i += 1
            continue
        j = i
        while j < n and v.word[raw[j]]:
            j += 1
        word = raw[i:j].lower() if v.fold else raw[i:j]
        out, c, failed = [], 0, len(word) > v.max_word
        while not failed and c < len(word):
            d = v.cont if c else v.first
            e = min(len(word), c + longest)                     # (no piece is longer)
            while e > c and word[c:e] not in d:
                e -= 1
            if e == c:
                failed = True
            else:
                out.append((d[word[c:e]], i + c))
                c = e
        if failed:
            out = [(v.unk, i)]
        for t, p in out:
            ids.append(t)
            positions.append(p)
        i = j
    tok_off = None if off is None else np.array([bisect.bisect_left(positions, int(o)) for o in off], dtype=np.uint64)
    return np.array(ids, dtype=np.int32), np.array(positions, dtype=np.uint32), tok_off


def want(data, n_owned, v, off=None):
    """What the passes deliver for this input: by_bitmaps over the composition's picks."""
    p, l, k = picks(data, n_owned, v, off)
    return by_bitmaps(data, n_owned, p, l, k, v, off)


def boundaries_ok(data, n_owned, off, v):
    """Every offset a word boundary: 0, n_owned, or a non-word byte on one side."""
    data = np.asarray(data, dtype=np.uint8)
    for o in np.asarray(off, dtype=np.int64).tolist():
        if 0 < o < n_owned and v.word[data[o - 1]] and v.word[data[o]]:
            return False
    return True


def check(wanted, ids, pos=None, tok_off=None, what="wordpiece"):
    """Holds a result against wanted = (ids, positions, tok_off) and names the first differing token."""
    import tokref
    tokref.check((wanted[0].astype(np.int64), wanted[1].astype(np.int64), wanted[2], 0), ids, pos, tok_off, None, what)


# ---------------------------------------------------------------------------
# the vocabulary of the named cases.  "play" has both halves with different ids; "ing", "er", "s" are ##-only; "un" and
# "the" are first-only; "x" is in neither half (a word that holds it is bad); '.' has a byte id, ',' and ' ' have none.

ENTRIES = [b"[UNK]", b"[CLS]", b"play", b"##play", b"##ing", b"##er", b"##s", b"un", b"the", b"a", b"##a", b"b", b"##b",
           b"ab", b"##ab", b"##abb", b".", b"!", b"##c", b"c", b"##-", b"", b"play", b"##ay", b"pl"]
CASE_WORD = DEFAULT_WORD


def vocab(max_word=100, fold=False, byte_ids=True):
    v = Vocab(ENTRIES, b"[UNK]", max_word, CASE_WORD, fold)
    if not byte_ids:
        v.byte_ids[:] = DROP
    return v


SKIPPED = [1, 20, 21, 22]               # [CLS], "##-" (a ## piece with a non-word byte), "", the second "play"


def filler(n, seed):
    """Text of n bytes: short words of the vocabulary's letters, spaces, dots, commas; a few bad words."""
    rng = np.random.default_rng(seed)
    words = [b"play", b"playing", b"player", b"plays", b"unplaying", b"the", b"a", b"ab", b"abb", b"b", b"abab", b"c", b"cc",
             b"x", b"playx", b"ing", b"abx", b"theplay", b"A", b"pl", b"play" * 3]
    seps = [b" ", b" ", b" ", b".", b", ", b"! ", b"\n", b"  "]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(len(words)))] + seps[int(rng.integers(len(seps)))]
    return np.frombuffer(bytes(out[:n]), dtype=np.uint8).copy()


def put(buf, at, s):
    buf[at:at + len(s)] = np.frombuffer(s, dtype=np.uint8)


def spaced(n):
    return np.full(n, ord(" "), dtype=np.uint8)


def _straddle(edge, left, right, hole=None, n=None):
    """A word of `left` + `right` bytes of "ab" pieces across position `edge`, alone in spaces; `hole`: the offset in
    the word of one byte made 'x' (in no piece)."""
    n = n or edge + TILE
    buf = spaced(n)
    w = (b"ab" * ((left + right) // 2 + 1))[:left + right]
    put(buf, edge - left, w)
    if hole is not None:
        buf[edge - left + hole] = ord("x")
    return buf


SMALL = (0, 1, 15, 16, 17, 4095, 4096, 4097)
SIZES = {"t3": 3 * TILE + 17, "t63": 63 * TILE, "t64": 64 * TILE, "t65": 65 * TILE + 1, "t130": 130 * TILE + 5}
HALO = 64
G = 64 * TILE


def cases():
    """name -> (data uint8[n_avail], n_owned, Vocab, offsets or None)."""
    out = {}
    v = vocab()
    for n in SMALL:
        out[f"n{n}"] = (filler(n, 100 + n), n, v, None)
    for name, n in SIZES.items():
        data = filler(n + HALO, 7)
        put(data, n - 1, b" ")                                  # (n_owned on a word boundary: both forms apply)
        out[name] = (data, n, v, None)
    # words across a tile edge: good; the one uncovered byte left, then right of the edge
    out["edge-good"] = (_straddle(TILE, 6, 6), 2 * TILE, v, None)
    out["edge-hole-left"] = (_straddle(TILE, 6, 6, hole=2), 2 * TILE, v, None)
    out["edge-hole-right"] = (_straddle(TILE, 6, 6, hole=9), 2 * TILE, v, None)
    out["edge-hole-first"] = (_straddle(TILE, 6, 6, hole=0), 2 * TILE, v, None)
    out["edge-hole-last"] = (_straddle(TILE, 6, 6, hole=11), 2 * TILE, v, None)
    v20 = vocab(max_word=20)
    out["edge-len-max"] = (_straddle(TILE, 7, 13), 2 * TILE, v20, None)
    out["edge-len-over"] = (_straddle(TILE, 7, 14), 2 * TILE, v20, None)
    out["group-good"] = (_straddle(G, 6, 6, n=G + TILE), G + TILE, v, None)
    out["group-hole-left"] = (_straddle(G, 6, 6, hole=2, n=G + TILE), G + TILE, v, None)
    out["group-hole-right"] = (_straddle(G, 6, 6, hole=9, n=G + TILE), G + TILE, v, None)
    out["group-len-max"] = (_straddle(G, 7, 13, n=G + TILE), G + TILE, v20, None)
    out["group-len-over"] = (_straddle(G, 7, 14, n=G + TILE), G + TILE, v20, None)
    vmax = vocab(max_word=4095)
    out["max4095-good"] = (_straddle(TILE, 95, 4000, n=3 * TILE), 3 * TILE, vmax, None)
    out["max4095-over"] = (_straddle(TILE, 96, 4000, n=3 * TILE), 3 * TILE, vmax, None)
    buf = spaced(3 * TILE)
    put(buf, TILE - 1, b"a")                                    # a word on a tile's last byte
    put(buf, 2 * TILE, b"play")                                 # a word on a tile's first byte behind a non-word byte
    put(buf, 2 * TILE - 2, b"b")
    out["tile-ends"] = (buf, 3 * TILE, v, None)
    buf = spaced(5 * TILE)
    put(buf, TILE - 100, b"ab" * (TILE + 100))                  # a tile of 4096 word bytes inside a word three tiles long
    out["three-tiles"] = (buf, 5 * TILE, vmax, None)
    buf = spaced(2 * TILE)
    buf[0:TILE:2] = ord("a")                                    # 2048 one-byte words in one tile
    buf[TILE + 1::2] = ord("x")                                 # ... and 2048 bad ones
    out["one-byte-words"] = (buf, 2 * TILE, v, None)
    # bitmap-word edges: words that end on bit 63, start on bit 0, and are cut by one uncovered byte there
    buf = spaced(TILE)
    put(buf, 60, b"abab")
    put(buf, 128, b"abab")
    put(buf, 188, b"abax")
    put(buf, 256, b"xbab")
    put(buf, 318, b"abab")                                      # across a bitmap word
    put(buf, 382, b"axab")
    put(buf, 446, b"abxb")
    put(buf, 500, b"ab" * 70)                                   # over two whole bitmap words
    put(buf, 700, b"ab" * 70)
    buf[763] = ord("x")
    out["bitmap-words"] = (buf, TILE, v, None)
    for mw in (1, 2, 3, 63, 64, 65, 127, 128):                  # the cap on every side of a bitmap word
        buf = spaced(TILE)
        at = 5
        for L in (mw - 1, mw, mw + 1, mw + 2):
            if L > 0:
                put(buf, at, (b"ab" * (L // 2 + 1))[:L])
                at += L + 3
        for L in (mw, mw + 1):                                  # ... the same ending on bit 63 and starting on bit 0
            at = (at + L + 64 + 63) // 64 * 64
            put(buf, at - L, (b"ab" * (L // 2 + 1))[:L])
            at += 64
            put(buf, at, (b"ab" * (L // 2 + 1))[:L])
            at += L + 1
        assert at < TILE
        out[f"cap{mw}"] = (buf, TILE, vocab(max_word=mw), None)
    # the end of the input: a word that ends at n_owned, one that runs into the halo
    buf = filler(TILE + 300 + HALO, 11)
    put(buf, TILE + 290, b" unplaying")
    put(buf, TILE + 300, b" ")
    out["end-at-owned"] = (buf, TILE + 300, v, None)
    buf = buf.copy()
    put(buf, TILE + 290, b"   playing  ")
    out["end-in-halo"] = (buf, TILE + 297, v, None)            # "play|ing": the pick "play" ends at n_owned
    out["end-pick-in-halo"] = (buf, TILE + 295, v, None)       # "pl|aying": the pick "play" ends in the halo
    out["alldrop-bytes"] = (filler(TILE + 17, 5), TILE + 17, vocab(byte_ids=False), None)
    folded = filler(2 * TILE + 5, 9)
    up = (folded >= 97) & (folded <= 122) & (np.arange(folded.size) % 3 == 0)
    folded[up] -= 32
    out["folded"] = (folded, folded.size, vocab(fold=True), None)
    # documents
    for shape in DOC_SHAPES:
        data, no = filler(DOC_OWNED + HALO, 13), DOC_OWNED
        if shape == "nothing":
            data[(data >= 97) & (data <= 122)] = ord("x")
        put(data, DOC_OWNED - 1, b" ")
        out[f"docs-{shape}"] = (data, no, v, doc_offsets(data, no, v, shape))
    return out


DOC_OWNED = 66 * TILE + 123
DOC_SHAPES = ("one", "big", "tiny", "empty0", "emptymid", "emptytile", "emptygroup", "emptyend", "cut", "nothing")
EMPTY_RUN = 230


def to_boundary(data, n_owned, o, v):
    """The nearest offset at or behind o that is a word boundary."""
    o = int(o)
    while 0 < o < n_owned and v.word[data[o - 1]] and v.word[data[o]]:
        o += 1
    return min(o, n_owned)


def doc_offsets(data, n_owned, v, shape):
    """Offsets in the shapes of passguard.DOC_SHAPES, every one moved to a word boundary."""
    rng = np.random.default_rng(sum(shape.encode()))
    no = int(n_owned)

    def run(at):
        return [at] * EMPTY_RUN
    if shape == "one":
        cuts = []
    elif shape == "nothing":                                    # (a text without a piece: every word is bad)
        cuts = [1000, 5 * TILE, 5 * TILE + 1]
    elif shape == "big":
        cuts = [no // 3, 2 * no // 3]
    elif shape == "tiny":
        cuts = np.cumsum(rng.integers(1, 40, size=no // 8)).tolist()
    elif shape == "empty0":
        cuts = run(0) + [5000, 9000]
    elif shape == "emptymid":
        cuts = [3000] + run(5 * TILE + 1234) + [40 * TILE]
    elif shape == "emptytile":
        cuts = [3000] + run(7 * TILE) + [40 * TILE]
    elif shape == "emptygroup":
        cuts = [3000] + run(G) + [G + 9000]
    elif shape == "emptyend":
        cuts = [3000, 60 * TILE] + run(no)
    else:                                                       # "cut": offsets on tile, word and group edges
        cuts = [63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 63, G - 1, G, G + 1, 65 * TILE]
    cuts = sorted(to_boundary(data, no, c, v) for c in cuts if c <= no)
    return np.array([0] + cuts + [no], dtype=np.uint64)


_MEMO = {}


def _cases():
    if "cases" not in _MEMO:
        _MEMO["cases"] = cases()
    return _MEMO["cases"]


def names():
    return tuple(_cases())


def case(name):
    return _cases()[name]


def want_of(name):
    """(ids, positions, tok_off) of a named case, computed once."""
    key = ("want", name)
    if key not in _MEMO:
        data, no, v, off = case(name)
        _MEMO[key] = want(data, no, v, off)
    return _MEMO[key]


# the small log of the surface tests, ids written out by hand against LOG_VOCAB (entry k has id k)
LOG_VOCAB = [b"[UNK]", b"[CLS]", b"play", b"##ing", b"##er", b"the", b"un", b"##play", b"##s", b".", b"a"]
LOG = b"the player plays.\nunplaying a playx\n\nthe. thes\n"
LOG_IDS = [5, 2, 4, 2, 8, 9, 6, 7, 3, 10, 0, 5, 9, 5, 8]
LOG_POS = [0, 4, 8, 11, 15, 16, 0, 2, 6, 10, 12, 0, 3, 5, 8]   # relative to the line
LOG_TOK_OFF = [0, 6, 11, 11, 15]
