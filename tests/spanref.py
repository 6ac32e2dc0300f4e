"""Host reference for the span filter (the checker, never the product), written from the rule in include/pfac.h.  A
record (pos, L) whose pattern carries the span (min_start, max_start, max_tail):

    d    = the last document with off[d] <= pos          (no offsets: the one document [0, n_avail))
    rel  = pos - off[d],  E = off[d + 1]
    C    = E - 1 if delimiter >= 0 and E > off[d] and buf[E - 1] == delimiter, else E
    tail = C - (pos + L) if pos + L <= C;  0 if C < pos + L <= E;  infinite if pos + L > E
    keep = min_start <= rel <= max_start and (max_tail is ANY or tail <= max_tail)

`filter_spans` returns the boolean keep mask over the records (pos, lens) of a scan of `buf`; the records come from a
CPU matcher (orc.Oracle), their lengths from the pattern file's own lines (llref.line_lengths), their spans from
`record_spans` -- the rules as the caller wrote them, parsed here and not by the product."""
import bisect

import numpy as np

ANY = 0xFFFFFFFF
INF = 1 << 62
ANCHORS = {None: (0, None, None), "^": (0, 0, None), "$": (0, None, 0), "^$": (0, 0, 0)}
LINE = (0, 0, 0)                           # what PFAC_SPANS_LINE judges every state as


def rule_bounds(rule):
    """One rule (None, "^", "$", "^$", or a triple with None = unbounded) -> (min_start, max_start, max_tail) as Python
    ints, an unbounded max_start as INF and an unjudged max_tail as ANY; a negative max_start admits no start."""
    lo, hi, tail = ANCHORS[rule] if rule is None or isinstance(rule, str) else rule
    return (0 if lo is None else int(lo), INF if hi is None or hi == ANY else int(hi), ANY if tail is None else int(tail))


def record_spans(rules, ids):
    """Per-record (smin, smax, stail) int64 arrays from `rules` indexed by the 1-based pattern id."""
    by_id = np.array([rule_bounds(r) for r in rules], dtype=np.int64).reshape(-1, 3)
    per = by_id[np.asarray(ids, dtype=np.int64)]
    return per[:, 0], per[:, 1], per[:, 2]


DRAW_SEED = 7


def drawn_rules(line_lengths, seed=DRAW_SEED):
    """Per-pattern rules drawn from {none, ^, $, ^$, (5, 25 - L, ANY)} -- the last one Snort's offset 5, depth 20 -- for
    the pattern lengths `line_lengths` (indexed by the 1-based id); entry 0 is the unused one."""
    ll = np.asarray(line_lengths, dtype=np.int64)
    pick = np.random.default_rng(seed).integers(0, 5, ll.size)
    return [None] + [(None, "^", "$", "^$", (5, 25 - int(ll[i]), None))[pick[i]] for i in range(1, ll.size)]


def line_spans(n):
    z = np.zeros(n, dtype=np.int64)
    return z, z, z


def _offsets(off, n_avail):
    return np.array([0, n_avail], dtype=np.int64) if off is None else np.asarray(off).astype(np.int64)


def filter_spans(buf, pos, lens, smin, smax, stail, delimiter=-1, off=None, n_avail=None):
    buf = np.asarray(buf, dtype=np.uint8)
    n_avail = int(buf.size) if n_avail is None else int(n_avail)
    pos = np.asarray(pos, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    off = _offsets(off, n_avail)
    assert -1 <= delimiter <= 255 and off.size >= 2 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] <= n_avail
    assert pos.size == 0 or (int(pos.max()) < off[-1] and int((pos + lens).max()) <= n_avail and int(lens.min()) >= 1)
    d = np.searchsorted(off, pos, side="right") - 1
    base, end = off[d], off[d + 1]
    term = np.zeros(pos.size, dtype=bool)
    if delimiter >= 0:
        some = end > base
        term[some] = buf[end[some] - 1] == delimiter
    cend = end - term
    pe = pos + lens
    tail = np.where(pe <= cend, cend - pe, np.where(pe <= end, 0, INF))
    rel = pos - base
    return (rel >= smin) & (rel <= smax) & ((np.asarray(stail) == ANY) | (tail <= stail))


def filter_spans_loop(buf, pos, lens, smin, smax, stail, delimiter=-1, off=None, n_avail=None):
    """The same rule record by record in plain Python (pins the vectorised form in the CPU tests)."""
    raw = bytes(np.asarray(buf, dtype=np.uint8))
    n_avail = len(raw) if n_avail is None else int(n_avail)
    off = [int(x) for x in _offsets(off, n_avail)]
    keep = []
    for p, l, lo, hi, mt in zip(*(np.asarray(a).tolist() for a in (pos, lens, smin, smax, stail))):
        d = bisect.bisect_right(off, p) - 1                    # the last document that starts at or before p
        base, end = off[d], off[d + 1]
        ok = lo <= p - base <= hi
        if ok and mt != ANY:
            c = end - 1 if delimiter >= 0 and end > base and raw[end - 1] == delimiter else end
            if p + l > end:
                ok = False
            elif p + l <= c:
                ok = c - (p + l) <= mt
        keep.append(ok)
    return np.array(keep, dtype=bool)


def split_offsets(buf, delimiter):
    """The offsets of pfac_slot_doc_offsets_split: a document ends behind every delimiter, an unterminated rest is the
    last document (int64[n_docs + 1])."""
    buf = np.asarray(buf, dtype=np.uint8)
    ends = np.flatnonzero(buf == delimiter) + 1
    off = np.concatenate(([0], ends)).astype(np.int64)
    return off if off[-1] == buf.size else np.append(off, buf.size)
