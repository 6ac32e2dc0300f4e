"""The checker of pfac_documents_gather_format (never the product): the segment rule of include/pfac.h in numpy
(`format_ref`), pinned to a second form that knows nothing of the first (`format_ref_loop`: b"%d" and b"".join) by
tests/test_format_ref.py, the named cases, and the check shared by the host and the GPU tests.  No expectation comes
from the device."""
import numpy as np

from gatherref import BLOCK, N_IDS, TILE, WIN, GatherCase

NL = 0x0A
LIMIT = 10 ** 18                        # every printed value is below it (18 digits)


class Fmt:
    """struct pfac_line_format as keywords (those of GpuMatcher.gather_documents_formatted)."""

    def __init__(self, number=False, byte_offset=False, terminate=None, context_sep=False, group_sep=b"", sep_first=False,
                 number_base=1, offset_base=0, sep_match=b":", sep_context=b"-"):
        self.number, self.byte_offset, self.terminate, self.context_sep = number, byte_offset, terminate, context_sep
        self.group_sep, self.sep_first, self.number_base, self.offset_base = bytes(group_sep), sep_first, number_base, offset_base
        self.sep_match, self.sep_context = sep_match, sep_context

    def kwargs(self):
        return dict(self.__dict__)

    def plain(self):
        """Whether the format asks for nothing (flags == 0 and group_sep_len == 0)."""
        return not (self.number or self.byte_offset or self.terminate is not None or self.context_sep or self.sep_first
                    or self.group_sep)


# ---------------------------------------------------------------------------
# the rule, twice

def _runs(lens):
    """(run, index inside the run) of every element of runs of the given lengths, in order."""
    lens = np.asarray(lens, dtype=np.int64)
    run = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    return run, np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)


def _digits(v):
    """(digit matrix int64[n, 18], most significant first, and the digit count of every value) of values below 10^18."""
    v = np.asarray(v, dtype=np.int64)
    assert v.size == 0 or (0 <= int(v.min()) and int(v.max()) < LIMIT)
    p = np.array([10 ** (17 - j) for j in range(18)], dtype=np.int64)
    nd = 1 + (v[:, None] >= p[None, :17]).sum(axis=1)
    return (v[:, None] // p[None, :]) % 10, nd


def format_ref(buf, offsets, ids, fmt, doc_first=None):
    """(out uint8[out_bytes], out_off uint64[n_ids + 1]) of pfac_documents_gather_format."""
    buf = np.asarray(buf, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    ids = np.asarray(ids, dtype=np.uint64).astype(np.int64)
    n = ids.size
    lo, hi = off[ids], off[ids + 1]
    body = hi - lo
    sepl = np.zeros(n, np.int64)
    if fmt.group_sep and n:
        apart = np.concatenate([[bool(fmt.sep_first)], ids[1:] != ids[:-1] + 1])
        sepl = apart * len(fmt.group_sep)
    label = np.full(n, fmt.sep_match[0], dtype=np.uint8)
    if fmt.context_sep:
        first = np.asarray(doc_first, dtype=np.uint64)
        label[first[ids + 1] == first[ids]] = fmt.sep_context[0]
    pieces = []                         # (values, digit counts) of the labels, in order
    if fmt.number:
        pieces.append(ids + int(fmt.number_base))
    if fmt.byte_offset:
        pieces.append(lo + int(fmt.offset_base))
    pieces = [(v,) + _digits(v) for v in pieces]
    term = np.zeros(n, bool)
    if fmt.terminate is not None:
        last = buf[np.maximum(hi - 1, 0)] if buf.size else np.zeros(n, np.uint8)
        term = (body == 0) | (last != fmt.terminate)
    seg = sepl + sum(nd + 1 for _, _, nd in pieces) + body + term
    out_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(seg)])
    out = np.zeros(int(out_off[-1]), dtype=np.uint8)
    at = out_off[:-1].copy()
    run, j = _runs(sepl)
    out[at[run] + j] = np.frombuffer(fmt.group_sep, dtype=np.uint8)[j] if fmt.group_sep else 0
    at += sepl
    for _, D, nd in pieces:
        run, j = _runs(nd)
        out[at[run] + j] = 48 + D[run, 18 - nd[run] + j]
        out[at + nd] = label
        at += nd + 1
    run, j = _runs(body)
    out[at[run] + j] = buf[lo[run] + j]
    at += body
    out[at[term]] = fmt.terminate if fmt.terminate is not None else 0
    return out, out_off.astype(np.uint64)


def format_ref_loop(buf, offsets, ids, fmt, doc_first=None):
    data = bytes(np.asarray(buf, dtype=np.uint8))
    off = [int(x) for x in offsets]
    first = None if doc_first is None else [int(x) for x in doc_first]
    segs, prev = [], None
    for k, i in enumerate(int(x) for x in ids):
        s = b""
        if fmt.group_sep and (fmt.sep_first if k == 0 else i != prev + 1):
            s += fmt.group_sep
        c = fmt.sep_context if fmt.context_sep and first[i + 1] == first[i] else fmt.sep_match
        if fmt.number:
            s += b"%d" % (i + fmt.number_base) + c
        if fmt.byte_offset:
            s += b"%d" % (off[i] + fmt.offset_base) + c
        line = data[off[i]:off[i + 1]]
        s += line
        if fmt.terminate is not None and not line.endswith(bytes([fmt.terminate])):
            s += bytes([fmt.terminate])
        segs.append(s)
        prev = i
    out_off = [0]
    for s in segs:
        out_off.append(out_off[-1] + len(s))
    return np.frombuffer(b"".join(segs), dtype=np.uint8), np.array(out_off, dtype=np.uint64)


# ---------------------------------------------------------------------------
# the cases

class FormatCase(GatherCase):
    """A GatherCase with a format and, under context_sep, a doc_first; `need` names a precondition that
    tests/test_format_ref.py asserts on the host."""

    def __init__(self, name, data, offsets, ids, fmt, doc_first=None, need=None):
        super().__init__(name, data, offsets, ids, need)
        self.fmt = fmt
        self.doc_first = None if doc_first is None else np.ascontiguousarray(doc_first, dtype=np.uint64)

    def want(self):
        if not hasattr(self, "_want"):
            self._want = format_ref(self.data, self.offsets, self.ids, self.fmt, self.doc_first)
        return self._want


def lines_data(lens, seed, lead=0, trail=0):
    """(data, offsets) of documents of the given lengths behind `lead` bytes that belong to none: seeded bytes; every
    third non-empty document (d % 3 == 2) does not end in a newline, every other one does."""
    lens = np.asarray(lens, dtype=np.int64)
    off = lead + np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)])
    data = np.random.default_rng(seed).integers(0, 256, int(off[-1]) + trail).astype(np.uint8)
    d = np.flatnonzero(lens > 0)
    end = off[d + 1] - 1
    data[end] = np.where(d % 3 == 2, np.where(data[end] == NL, 0x0B, data[end]), NL)
    return data, off


def seeded_first(n_docs, seed):
    """A doc_first in which about a third of the documents hold a record."""
    cnt = np.random.default_rng(seed).integers(0, 3, n_docs) // 2 * np.random.default_rng(seed + 1).integers(1, 4, n_docs)
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(cnt).astype(np.uint64)])


def _case(name, lens, ids, seed, fmt, need=None, lead=0, trail=0, with_first=None):
    data, off = lines_data(lens, seed, lead, trail)
    first = seeded_first(len(lens), seed + 77) if (fmt.context_sep if with_first is None else with_first) else None
    return FormatCase(name, data, off, ids, fmt, first, need)


ALL = dict(number=True, byte_offset=True, terminate=NL, context_sep=True, group_sep=b"--\n", sep_first=True)
FLAG_SETS = {"number": dict(number=True), "offset": dict(byte_offset=True), "terminate": dict(terminate=NL),
             "context_sep": dict(context_sep=True), "sep_first": dict(sep_first=True), "group_sep": dict(group_sep=b"--\n"),
             "all": ALL}


def count_cases():
    """gatherref.N_IDS ids over 300 documents of lengths 0..40, with repeats, under every single flag, under the group
    separator alone and under everything together."""
    out = []
    for n in N_IDS:
        rng = np.random.default_rng(4000 + n)
        lens, ids = rng.integers(0, 41, 300), rng.integers(0, 300, n)
        for k, kw in FLAG_SETS.items():
            out.append(_case(f"ids{n}_{k}", lens, ids, 5000 + n, Fmt(**kw)))
    return out


DIGIT_EDGES = (9, 99, 10 ** 9 - 1, LIMIT - 2)


def digit_cases():
    """Two documents of one byte: the printed numbers and offsets are base, base + 1.  The bases of DIGIT_EDGES put a
    digit count's edge between them (10^9: where the digits leave 32 bits; 10^18 - 1: the last value there is); base 0
    prints 0; 10^d - 3 walks six values across every other edge."""
    out = []
    for b in DIGIT_EDGES:
        out.append(_case(f"digits_{b}", [1, 1], [0, 1], 70, Fmt(number=True, byte_offset=True, number_base=b, offset_base=b),
                         ("prints", b, b + 1)))
    out.append(_case("digits_zero", [1, 1], [0, 1], 71, Fmt(number=True, byte_offset=True, number_base=0, offset_base=0),
                     ("prints", 0, 1)))
    for d in range(1, 19):
        b = min(10 ** d - 3, LIMIT - 6)
        out.append(_case(f"digits_1e{d}", np.ones(6, np.int64), np.arange(6), 72 + d,
                         Fmt(number=True, byte_offset=True, terminate=NL, number_base=b, offset_base=b), ("prints", b, b + 5)))
    return out


LADDER_BASE = 10 ** 17 + 12345          # 18 digits: a label of 19 bytes lies in two or three 16-byte chunks


def ladder_cases():
    """The residue mod 16 of the output offset of segment 1's label through 0..15 and, independently, the source residue
    of its body through 0..15 (the shape of gatherref.ladder_cases): segment 0 is a label of 19 bytes and a body that
    ends where the residue is wanted."""
    out = []
    for i in range(32):
        lab, src = (i, (7 * i + 3) % 16) if i < 16 else ((3 * i + 2) % 16, i - 16)
        len0 = 16 + (lab - 19) % 16                             # 19 + len0 = lab mod 16
        lead = (src - len0) % 16                                # document 1 starts at lead + len0
        out.append(_case(f"ladder_label{lab}_src{src}", [len0, 40, 21], [0, 1, 2], 600 + i,
                         Fmt(number=True, number_base=LADDER_BASE), ("ladder", lab, src), lead=lead))
    return out


def _crossing(name, edge, seed):
    """Documents of 20 bytes under both labels of 18 digits; the first document's length is the smallest at which a label
    lies on both sides of output byte `edge`."""
    fmt = Fmt(number=True, byte_offset=True, terminate=NL, number_base=LADDER_BASE, offset_base=LADDER_BASE)
    n = edge // 40 + 8
    for len0 in range(0, 64):
        lens = np.concatenate([[len0], np.full(n - 1, 20)])
        c = _case(name, lens, np.arange(n), seed, fmt, ("label_crosses", edge))
        if label_crossing(c, edge) is not None:
            return c
    raise AssertionError(name)


def label_spans(case):
    """(start, end) in the output of every label of a case (the number and the offset with their separators, as one)."""
    f = case.fmt
    _, out_off = case.want()
    o = out_off[:-1].astype(np.int64)
    ids = case.ids.astype(np.int64)
    if f.group_sep and ids.size:
        o = o + np.concatenate([[bool(f.sep_first)], ids[1:] != ids[:-1] + 1]) * len(f.group_sep)
    ln = np.zeros(ids.size, np.int64)
    if f.number:
        ln += _digits(ids + f.number_base)[1] + 1
    if f.byte_offset:
        ln += _digits(case.offsets.astype(np.int64)[ids] + f.offset_base)[1] + 1
    return o, o + ln


def label_crossing(case, edge):
    """The first segment whose label has bytes on both sides of output offset `edge`, or None."""
    a, b = label_spans(case)
    j = np.flatnonzero((a < edge) & (b > edge))
    return int(j[0]) if j.size else None


def edge_cases():
    big = 130 * TILE + 5
    short = np.random.default_rng(11).integers(1, 30, 40)
    every = Fmt(**ALL)
    out = [_crossing("label_crosses_window", WIN, 80), _crossing("label_crosses_4_windows", 4 * WIN, 81)]
    # the last segment of a block and the first of the next, both with labels of 18 digits
    out.append(_case("labels_at_block_edge", np.full(130, 3), np.arange(130), 82,
                     Fmt(number=True, byte_offset=True, number_base=LADDER_BASE, offset_base=LADDER_BASE), "block_edge"))
    for n in (15, 16, 17, 1023, 1024, 1025):                    # labels "1:" "2:" "3:", 6 bytes
        out.append(_case(f"out_{n}", [n - 15, 0, 9], [0, 1, 2], 40 + n, Fmt(number=True), ("out_bytes", n)))
    out += [
        _case("empty_x3000_labels", np.zeros(3000, np.int64), np.arange(3000), 83, Fmt(number=True, byte_offset=True, terminate=NL)),
        _case("empty_x3000_terminate", np.zeros(3000, np.int64), np.arange(3000), 84, Fmt(terminate=NL)),
        _case("empty_x3000_sep_only", np.zeros(3000, np.int64), np.arange(3000), 85, Fmt(group_sep=b"--\n"), "out_empty"),
        _case("empty_x3000_then_one_sep_only", np.concatenate([np.zeros(3000, np.int64), [37]]), np.arange(3001), 86,
              Fmt(group_sep=b"--\n"), "empty_blocks"),
        _case("long_doc_between_short", np.concatenate([short[:20], [big], short[20:]]), np.arange(41), 87, every, "long_doc"),
    ]
    return out


def separator_cases():
    """1100 ids over 1200 documents of lengths 0..12.  "adjacent": ids 0..1099; "apart": one document is left out in front
    of k = 64 and one in front of k = 1024, so exactly those two steps (and k = 0 under SEP_FIRST) get a separator.  Then
    a repeat, a descending list, and a permutation."""
    lens = np.random.default_rng(90).integers(0, 13, 1200)
    adjacent = np.arange(1100)
    apart = adjacent + (adjacent >= BLOCK) + (adjacent >= 1024)
    out = []
    for n, (sep, first) in enumerate(((b"\n", False), (b"--\n", True), (b"-=-=-=-\n", False))):
        for kind, ids in (("adjacent", adjacent), ("apart", apart)):
            out.append(_case(f"sep{len(sep)}_{kind}" + ("_first" if first else ""), lens, ids, 91,
                             Fmt(number=True, group_sep=sep, sep_first=first), ("steps", kind)))
    out.append(_case("sep_repeat", lens, [5, 5, 6, 6, 7], 92, Fmt(number=True, group_sep=b"--\n"), ("seps", [1, 3])))
    out.append(_case("sep_descending", lens, np.arange(69, -1, -1), 93, Fmt(group_sep=b"--\n", sep_first=True), ("seps", list(range(70)))))
    out.append(_case("sep_first_alone", lens, np.arange(70), 94, Fmt(group_sep=b"--\n", sep_first=True), ("seps", [0])))
    out.append(_case("sep_first_off", lens, np.arange(70), 94, Fmt(group_sep=b"--\n"), ("seps", [])))
    return out


def terminate_cases():
    """One document set (150 lengths 0..40; documents that end in the newline, that do not, and empty ones; the last one
    unterminated and n_bytes % 16 != 0) under four id lists, with and without labels."""
    lens = np.random.default_rng(21).integers(0, 41, 150)
    lens[-1] = 23
    lens[-2] = 0
    if int(lens.sum()) % 16 == 0:
        lens[0] += 1
    lists = {"all": np.arange(150), "last_only": np.array([149]), "reversed": np.arange(149, -1, -1),
             "tail": np.array([147, 148, 149])}
    out = []
    for k, v in lists.items():
        out.append(_case(f"terminate_{k}", lens, v, 23, Fmt(terminate=NL), ("terminate", k)))
        out.append(_case(f"terminate_{k}_labels", lens, v, 23, Fmt(number=True, byte_offset=True, terminate=NL), ("terminate", k)))
    out.append(_case("terminate_other_byte", lens, lists["all"], 23, Fmt(terminate=0x0B, number=True)))
    return out


def all_format_cases():
    return count_cases() + digit_cases() + ladder_cases() + edge_cases() + separator_cases() + terminate_cases()


# the large output: PERIOD_IDS over a small input, PERIODS times.  Every period prints the same bytes (the ids repeat,
# and under SEP_FIRST the step back to the first id gets the separator the first period has), an odd number of them
BIG_LENS = np.random.default_rng(95).integers(60, 140, 37)
BIG_PERIODS = 18000


def big_case():
    c = _case("big_period", BIG_LENS, np.arange(37), 96, Fmt(**ALL))
    if c.want()[0].size % 2 == 0:
        c = _case("big_period", np.concatenate([BIG_LENS[:-1], [BIG_LENS[-1] + 1]]), np.arange(37), 96, Fmt(**ALL))
    return c


def chain_cuts(offsets, n_cuts=3):
    """`n_cuts` document boundaries inside the buffer, as a reader that carries the unterminated rest over would cut it
    (tail_start of the split): strictly inside, ascending."""
    off = np.asarray(offsets, dtype=np.int64)
    inner = np.unique(off[(off > 0) & (off < off[-1])])
    return [int(inner[(i + 1) * inner.size // (n_cuts + 1)]) for i in range(n_cuts)]


# ---------------------------------------------------------------------------
# grep

LOG_PATTERNS = [b"error", b"timeout", b"disk net", b"ok"]


def make_log(seed=5, n_lines=400):
    """A small log: lines of 0..6 words (some in capitals), empty lines among them, the last line unterminated."""
    rng = np.random.default_rng(seed)
    words = [b"alpha", b"beta", b"gamma", b"delta", b"error", b"warn", b"timeout", b"retry", b"ok", b"disk", b"net", b"ERROR",
             b"Timeout", b"errors", b"oklahoma"]
    lines = []
    for _ in range(n_lines):
        lines.append(b" ".join(words[int(i)] for i in rng.integers(0, len(words), int(rng.integers(0, 7)))))
    lines[7], lines[90] = b"error", b"ok"
    return b"\n".join(lines) + b"\nlast line without its newline: error"


def python_grep(data, patterns, before=0, after=0, invert=False, ignore_case=False, whole_words=False, line_match=False):
    """(offsets, ids, doc_first, n_lines) of grep -F in Python: `before` lines in front of a selected line, `after`
    behind it; doc_first counts one record per line that holds a match."""
    import re
    lines = data.splitlines(keepends=True)
    fold = (lambda b: b.lower()) if ignore_case else (lambda b: b)
    pats = [fold(p) for p in patterns]
    if line_match:
        hit = [fold(line.rstrip(b"\n")) in pats for line in lines]
    elif whole_words:
        word = re.compile(rb"(?<![0-9A-Za-z_])(?:" + b"|".join(re.escape(p) for p in pats) + rb")(?![0-9A-Za-z_])")
        hit = [word.search(fold(line)) is not None for line in lines]
    else:
        hit = [any(p in fold(line) for p in pats) for line in lines]
    keep = [h != invert for h in hit]
    ids = [d for d in range(len(lines)) if any(keep[max(d - after, 0):d + before + 1])]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.uint64)
    first = np.concatenate([[0], np.cumsum(hit)]).astype(np.uint64)
    return off, np.array(ids, dtype=np.uint64), first, len(lines)


def grep_fmt(kw, before, after, **more):
    """The format GpuMatcher.grep_text asks for."""
    context = bool(before or after)
    return Fmt(terminate=NL, context_sep=context, group_sep=b"--\n" if context else b"", **kw, **more)


# ---------------------------------------------------------------------------
# the check

def assert_format(case, out_bytes, out_off, out, fill=None, what="", want=None):
    """The check of every case: the count, every offset, every byte (the first differing index in the message) and, with
    `fill`, that the bytes of `out` at and past out_bytes still hold it."""
    want, want_off = case.want() if want is None else want
    what = f"{case.name} {what}"
    assert out_bytes == want.size, f"{what}: out_bytes {out_bytes}, want {want.size}"
    got_off = np.asarray(out_off, dtype=np.uint64)
    assert got_off.size == want_off.size, f"{what}: {got_off.size} output offsets, want {want_off.size}"
    bad = np.flatnonzero(got_off != want_off)
    assert bad.size == 0, f"{what}: out_off[{int(bad[0])}] is {int(got_off[bad[0]])}, want {int(want_off[bad[0]])} ({bad.size} differ)"
    out = np.asarray(out, dtype=np.uint8)
    assert out.size >= want.size, f"{what}: {out.size} output bytes fetched, want {want.size}"
    bad = np.flatnonzero(out[:want.size] != want)
    if bad.size:
        k = int(np.searchsorted(want_off, bad[0], side="right")) - 1
        raise AssertionError(f"{what}: output byte {int(bad[0])} (segment {k}, its byte {int(bad[0]) - int(want_off[k])}) is "
                             f"0x{int(out[bad[0]]):02x}, want 0x{int(want[bad[0]]):02x} ({bad.size} differ, the last at "
                             f"{int(bad[-1])}; out_bytes {want.size})")
    if fill is not None:
        bad = np.flatnonzero(out[want.size:] != fill)
        assert bad.size == 0, f"{what}: a byte at out_bytes + {int(bad[0])} was written ({bad.size} past the output's end)"
