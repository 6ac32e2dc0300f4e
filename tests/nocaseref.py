"""Host reference for case-insensitive scans (the checker, never the product), and the named inputs of the GPU tests.

The rule (include/pfac.h, pfac_table_set_case_fold): a folded scan reports what an EXACT scan of the folded input with
the table of the folded patterns reports, where folding turns the bytes 0x41..0x5A into 0x61..0x7A and changes nothing
else.  `expected` is that sentence with the CPU oracle; `brute` is a second matcher that shares nothing with it
(bytes.lower() on both sides, pure-ASCII cases only); `exact` is the oracle on the pattern file and the input as they
were written -- a case is worth running only if folding adds matches to those.

Every GPU case is a `Case` built here, so that tests/test_nocase_ref.py can hold each one against both matchers on the
host before a GPU sees it."""
import functools
import os
import tempfile

import numpy as np

from orc import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "data")
TILE = 4096

FOLD = np.arange(256, dtype=np.uint8)          # bytes.lower() restricted to ASCII
FOLD[0x41:0x5B] |= 0x20


def as_u8(data):
    return np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, dtype=np.uint8)


def fold(data):
    return FOLD[as_u8(data)]


def fold_bytes(b):
    return fold(b).tobytes()


def _oracle_scan(patterns, data, n_owned):
    with tempfile.NamedTemporaryFile(suffix=".pat") as f:
        f.write(patterns)
        f.flush()
        o = Oracle(f.name, 1, 1)
        pos, ids = o.scan_spec(np.ascontiguousarray(data))
        o.close()
    if n_owned is not None:
        keep = pos < int(n_owned)
        pos, ids = pos[keep], ids[keep]
    return pos, ids


class FoldedOracle:
    """The oracle on the folded pattern file, for references that scan pieces themselves (docref.oracle_per_doc): feed
    it folded bytes."""

    def __enter__(self):
        return self.o

    def __init__(self, patterns):
        self.f = tempfile.NamedTemporaryFile(suffix=".pat")
        self.f.write(fold_bytes(patterns))
        self.f.flush()
        self.o = Oracle(self.f.name, 1, 1)

    def __exit__(self, *exc):
        self.o.close()
        self.f.close()


def expected(patterns, data, n_owned=None):
    """(pos int64[], id int32[]) of a folded scan: the oracle on the folded pattern file and the folded data; walks start
    in [0, n_owned) and read all of data.  In the scan's output order (position, pattern length)."""
    return _oracle_scan(fold_bytes(patterns), fold(data), n_owned)


def exact(patterns, data, n_owned=None):
    """The oracle on the pattern file and the data as they are."""
    return _oracle_scan(bytes(patterns), as_u8(data), n_owned)


def brute(patterns, data, n_owned=None):
    """data[i:i + len(p)].lower() == p.lower() for every line p and offset i; the last of lines that are equal once
    lowered reports.  Sorted by (position, pattern length).  Pure-ASCII patterns and data only."""
    data = bytes(as_u8(data))
    assert data.isascii() and patterns.isascii()
    low = data.lower()
    n_owned = len(data) if n_owned is None else int(n_owned)
    winner = {}
    for i, p in enumerate(patterns[:-1].split(b"\n"), start=1):
        winner[p.lower()] = i
    out = []
    for p, i in winner.items():
        k = low.find(p)
        while k != -1 and k < n_owned:
            out.append((k, len(p), i))
            k = low.find(p, k + 1)
    out.sort()
    return np.array([o[0] for o in out], dtype=np.int64), np.array([o[2] for o in out], dtype=np.int32)


# ---------------------------------------------------------------------------
# inputs

def paragraph():
    return open(os.path.join(DATA, "paragraph402"), "rb").read()


def tiled(n, unit):
    return np.frombuffer((unit * (n // len(unit) + 1))[:n], dtype=np.uint8).copy()


def mixed_text(n, seed=402, symbols=False):
    """paragraph402 tiled to n bytes with a seeded half of its letters in upper case; `symbols`: a seeded eighth of its
    spaces becomes one of the bytes next to the letter blocks (@ [ ` {) or a byte >= 0x80 that is a letter in Latin-1."""
    rng = np.random.default_rng(seed)
    buf = tiled(n, paragraph())
    lower = (buf >= 0x61) & (buf <= 0x7A)
    buf[lower & (rng.random(n) < 0.5)] &= 0xDF
    if symbols:
        sp = np.flatnonzero(buf == 0x20)
        at = sp[rng.random(sp.size) < 0.125]
        buf[at] = np.frombuffer(b"@[`{\xc1\xda\xe1\xfa", dtype=np.uint8)[rng.integers(0, 8, at.size)]
    return buf


def cycle256(n, stride=37):
    """All 256 byte values, over and over, at a stride coprime to 16 (so every value meets every lane and dword byte)."""
    return ((np.arange(n, dtype=np.int64) * stride) & 255).astype(np.uint8)


EXPERIMENT = open(os.path.join(DATA, "experimentpattern"), "rb").read()


@functools.lru_cache(maxsize=None)
def symbol_patterns():
    """Patterns with @ [ ` {, digits and bytes >= 0x80 next to letters: the boundary bytes on their own, single letters
    and digits, windows of `mixed_text(symbols=True)` around its symbol bytes and windows of `cycle256` that start at a
    letter -- the letters of every window written in the OTHER case than the input has them."""
    rng = np.random.default_rng(7)
    lines = [b"@", b"[", b"`", b"{", b"\xc1", b"\xe1", b"\xda", b"\xfa", b"Z", b"a", b"0", b"9", b"2015 W", b"E-d"]
    text = mixed_text(40 * TILE, symbols=True)
    sym = np.flatnonzero(np.isin(text, np.frombuffer(b"@[`{\xc1\xda\xe1\xfa", dtype=np.uint8)))
    for at in sym[rng.integers(0, sym.size, 24)]:
        a, b = int(at) - int(rng.integers(1, 4)), int(at) + int(rng.integers(2, 5))
        lines.append(text[a:b].tobytes().swapcase())
    cyc = cycle256(256)
    for first in (0x41, 0x5A, 0x61, 0x7A, 0x47, 0x6D):
        k = int(np.flatnonzero(cyc == first)[0])
        lines.append(np.resize(cyc[k:], 256)[: int(rng.integers(2, 6))].tobytes().swapcase())
    lines = [l for l in lines if b"\n" not in l]
    return b"\n".join(lines) + b"\n"


class Case:
    def __init__(self, name, patterns, data, n_owned=None, width=256):
        self.name, self.patterns, self.data, self.width = name, bytes(patterns), as_u8(data), width
        self.n_owned = n_owned
        self.ascii_only = self.patterns.isascii() and int(self.data.max()) < 0x80     # `brute` applies

    def __repr__(self):
        return self.name

    @functools.cached_property
    def want(self):
        return expected(self.patterns, self.data, self.n_owned)


def _place(buf, at, text):
    buf[at:at + len(text)] = np.frombuffer(text, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def parity_cases():
    out = []
    for iname, data in (("mixed", mixed_text(9 * TILE + 5, symbols=True)), ("cycle", cycle256(5 * TILE + 3))):
        for pname, pats in (("experiment", EXPERIMENT), ("symbols", symbol_patterns())):
            for width in (64, 256, 1024):
                out.append(Case(f"parity-{iname}-{pname}-w{width}", pats, data, width=width))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def variant_cases():
    """The inputs run under every kernel variant: the four-line set whose root has ONE edge, and the symbol set."""
    return (Case("variant-experiment", EXPERIMENT, mixed_text(17 * TILE + 9)),
            Case("variant-symbols", symbol_patterns(), mixed_text(17 * TILE + 9, symbols=True)))


@functools.lru_cache(maxsize=None)
def dictionary_case():
    pats = b"".join(open(os.path.join(DATA, p), "rb").read() for p in ("xaa", "xab", "xac", "xad"))
    return Case("dictionary-mixed", pats, mixed_text(75 * TILE + 1, seed=5))


@functools.lru_cache(maxsize=None)
def root1_cases():
    """Every line begins with one letter, and the input has that letter in upper case only (the root test of ROOT == 1
    compares with the one root byte); the second byte is one of one / two / three child bytes, upper case only as well
    (l2f_mode 1 compares with at most two).  Each file also has a line the input holds exactly as written."""
    out = []
    for name, pats in (("one-child", b"Qa\nQab\nQaBc\n"), ("two-children", b"Qa\nQb\nQax\nQbY\n"),
                       ("three-children", b"Qa\nQb\nQc\nQcz\n")):
        unit = b"..Qa..QA.QAB.xa.QABC,QB;QBY QAX-QCZ.xcz..QC" + b"." * 21          # (no lower-case q anywhere)
        out.append(Case(f"root1-{name}", pats, tiled(3 * TILE + 11, unit)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def placement_cases():
    out = []
    needle, written = b"needle-in-a-stack", b"nEEdle-In-A-sTaCK"            # 17 bytes
    pats = needle + b"\nstack\n"

    def base(n):
        buf = np.full(n, ord("."), dtype=np.uint8)
        _place(buf, 100, needle)                                        # one occurrence as the file writes it
        return buf
    # halo: the match straddles a tile boundary, its tail comes from the halo registers
    buf = base(3 * TILE + 40)
    for t in (1, 2):
        _place(buf, t * TILE - 3, written)
    _place(buf, 3 * TILE - 16, written.upper())
    out.append(Case("halo-straddle", pats, buf))
    # owned range: starts in the last 15 bytes of the owned range, ends in the halo past n_owned
    for back in (1, 5, 15):
        n_owned = 3 * TILE + 100
        buf = base(n_owned + 16)
        _place(buf, n_owned - back, written)                            # (its "stack" starts past n_owned: not reported)
        out.append(Case(f"owned-end-{back}", pats, buf, n_owned=n_owned))
    # ragged tail: the last 16-byte unit is partial and patched byte by byte; an upper-case match ends in the last byte
    for rem in (1, 7, 15):
        n = 4 * TILE + 32 + rem
        buf = base(n)
        _place(buf, n - 17, written.upper())
        _place(buf, n - 40, b"STACK")
        out.append(Case(f"ragged-tail-{rem}", pats, buf))
    # max_pat_len: the longest line of the file in mixed case across a tile boundary, and at the very end
    rng = np.random.default_rng(1022)
    for m in (1, 2, 17, 1022):
        longest = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)[rng.integers(0, 26, m)].tobytes()
        lines = [longest] + ([longest[: m // 2]] if m // 2 else []) + ([b"k"] if m > 1 else [])
        buf = np.full(4 * TILE + 7, ord("-"), dtype=np.uint8)
        mixed = bytes(c & 0xDF if rng.random() < 0.5 else c for c in longest)
        if mixed == longest:
            mixed = longest.upper()
        _place(buf, 64, longest)
        _place(buf, 2 * TILE - m // 2 - 1 if m > 1 else 2 * TILE - 1, mixed)
        _place(buf, buf.size - m, longest.upper())
        out.append(Case(f"max-len-{m}", b"\n".join(lines) + b"\n", buf))
    return tuple(out)


def all_cases():
    return parity_cases() + variant_cases() + (dictionary_case(),) + root1_cases() + placement_cases() + (passes_case(),)


@functools.lru_cache(maxsize=None)
def passes_case():
    """The input of the passes behind the scan: lines of mixed-case text, words next to the matches."""
    pats = b"england\nEngland were\ncricket\nODI\nover\nruns per over\nteam\nlanD\n"          # (nothing of the text's second sentence)
    return Case("passes-lines", pats, mixed_text(6 * TILE + 77, seed=11))


# ---------------------------------------------------------------------------
# character classes

def fold_class_set(listed):
    """The listed set of a class (256 booleans) with its upper-case members turned into their lower-case letters."""
    out = np.array(listed, dtype=bool)
    up = out[0x41:0x5B].copy()
    out[0x41:0x5B] = False
    out[0x61:0x7B] |= up
    return out


def folded_classes(image):
    """The class image `image` as ClassMatcher's `parsed`: every single character folded, the LISTED set of every class
    folded, `[^...]` complementing the folded set -- the rule of from_charclass(..., ignore_case=True), written from its
    documentation.  For images without backslash escapes (the first `]` closes a class)."""
    assert b"\\" not in image and image.endswith(b"\n")
    pats = []
    for line in image[:-1].split(b"\n"):
        elems, k = [], 0
        while k < len(line):
            listed, negated = np.zeros(256, dtype=bool), False
            if line[k] == 0x5B:
                end = line.index(b"]", k + 1)
                body = line[k + 1:end]
                negated = body[:1] == b"^"
                body, j = body[1:] if negated else body, 0
                while j < len(body):
                    if j + 2 < len(body) and body[j + 1] == 0x2D:
                        listed[body[j]:body[j + 2] + 1] = True
                        j += 3
                    else:
                        listed[body[j]] = True
                        j += 1
                k = end + 1
            else:
                listed[line[k]] = True
                k += 1
            listed = fold_class_set(listed)
            elems.append(~listed if negated else listed)
        pats.append(elems)
    return pats
