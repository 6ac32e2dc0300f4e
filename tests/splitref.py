"""Host references for the device-side delimiter split (pfac_slot_doc_offsets_split) and for pfac_documents_matching
(the checker, never the product), the named cases both test files run, and the protocol checks of the GPU tests.

The split's rule, from include/pfac.h: a document ends after every delimiter byte.
    E       = { i + 1 : 0 <= i < n, in[i] == delimiter }, ascending
    offsets = 0, then E, then n once more if n > 0 and in[n - 1] != delimiter
    n_docs  = number of offsets - 1;  tail_start = start of the unterminated last document, or n if there is none
`split_offsets` is that rule with numpy; `split_offsets_pieces` rebuilds the offsets from the piece lengths of
bytes.split and knows nothing of the first.  The matching rule: document d is reported iff
(doc_first[d + 1] > doc_first[d]) != invert, ids ascending (`matching_ids`, and `matching_ids_loop` in plain Python).

A case carries `storage` = the n input bytes followed by padding up to the next tile; the GPU tests fill that padding
with the delimiter (and with its complement): no byte at or past n may influence the result."""
import numpy as np

TILE = 4096
LENGTHS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 64 * 4096 - 1, 64 * 4096, 64 * 4096 + 1, 130 * 4096 + 5)
DELIMS = (0x0A, 0x00, 0xFF)
MATCH_DOCS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 64 * 64 * 4 + 1)
MATCH_KINDS = ("all_empty", "none_empty", "alternating", "runs")


# ---------------------------------------------------------------------------
# references

def split_offsets(buf, delim):
    """-> (offsets uint64[n_docs + 1], n_docs, tail_start)."""
    buf = np.asarray(buf, dtype=np.uint8)
    n = int(buf.size)
    ends = np.flatnonzero(buf == np.uint8(delim)).astype(np.uint64) + np.uint64(1)
    open_tail = n > 0 and int(buf[-1]) != int(delim)
    off = np.concatenate([np.zeros(1, np.uint64), ends, np.full(1 if open_tail else 0, n, np.uint64)])
    tail_start = (int(ends[-1]) if ends.size else 0) if open_tail else n
    return off, int(off.size) - 1, tail_start


def split_offsets_pieces(data, delim):
    """The same from bytes.split: every piece but the last is a document with its delimiter put back; the last piece is
    a document iff it is not empty."""
    data = bytes(data)
    pieces = data.split(bytes([delim]))
    lens = [len(p) + 1 for p in pieces[:-1]] + ([len(pieces[-1])] if pieces[-1] else [])
    off = [0]
    for x in lens:
        off.append(off[-1] + x)
    tail_start = off[-2] if pieces[-1] else len(data)
    return np.array(off, dtype=np.uint64), len(lens), tail_start


def matching_ids(doc_first, invert=False):
    first = np.asarray(doc_first, dtype=np.uint64)
    return np.flatnonzero((first[1:] > first[:-1]) != bool(invert)).astype(np.uint64)


def matching_ids_loop(doc_first, invert=False):
    first = [int(x) for x in doc_first]
    return np.array([d for d in range(len(first) - 1) if (first[d + 1] > first[d]) != bool(invert)], dtype=np.uint64)


# ---------------------------------------------------------------------------
# cases of the split

class SplitCase:
    """`data` (uint8[n]) cut at `delim`; `need` names a precondition that test_split_ref.py asserts on the host."""

    def __init__(self, name, data, delim, need=None):
        self.name, self.data, self.delim, self.need = name, np.ascontiguousarray(data, dtype=np.uint8), int(delim), need
        self.n = int(self.data.size)

    def storage(self, pad):
        """The input followed by `pad` bytes up to the next tile boundary (at least 16 of them)."""
        size = (self.n + 16 + TILE - 1) // TILE * TILE
        s = np.full(size, pad, dtype=np.uint8)
        s[:self.n] = self.data
        return s

    def __repr__(self):
        return self.name


def _text(rng, n, delim, every=40):
    """Seeded bytes of every value, the delimiter about once in `every`."""
    b = rng.integers(0, 256, n).astype(np.uint8)
    b[b == delim] = (delim + 1) & 0xFF
    b[rng.random(n) < 1.0 / every] = delim
    return b


def length_cases():
    out = []
    for n in LENGTHS:
        for d in DELIMS:
            rng = np.random.default_rng(1000 * d + n)
            out.append(SplitCase(f"len{n}_d{d:02x}", _text(rng, n, d), d))
    return out


def placement_cases(delim=0x0A):
    n = 3 * TILE + 100
    base = np.full(n, 0x61, dtype=np.uint8)

    def at(name, where, need=None, size=n):
        b = base[:size].copy()
        b[np.asarray(where, dtype=np.int64)] = delim
        return SplitCase(name, b, delim, need)

    run = lambda start, k: list(range(start, start + k))          # noqa: E731
    return [
        at("no_delimiter", [], "none"),
        at("first_and_last_byte", [0, n - 1], "first_last"),
        at("tile_last_and_next_first", [TILE - 1, TILE], None),
        at("lane_chunk_edges", [15, 16, 1023, 1024], None),
        at("tile_of_delimiters", run(TILE - 1, TILE + 1), "full_tile"),   # every byte of tile 1 starts a document
        at("run_of_2", run(777, 2), None),
        at("run_of_64", run(2 * TILE - 30, 64), None),
        at("run_of_65", run(1000, 65), None),
        at("delimiter_in_last_partial_chunk", [5, n - 2], "last_partial"),      # n % 16 == 4: byte n - 2 lies in the partial chunk
        at("only_delimiters_short", run(0, 33), "all", size=33),
    ]


def adversarial_cases():
    """Only the delimiter and its nearest neighbours (one bit off at either end, one above, one below), interleaved."""
    out = []
    for d in (0x0A, 0x00, 0x01, 0xFF):
        rng = np.random.default_rng(77 + d)
        alphabet = np.array([d, d ^ 0x01, d ^ 0x80, (d + 1) & 0xFF, (d - 1) & 0xFF], dtype=np.uint8)
        b = alphabet[rng.integers(0, alphabet.size, 2 * TILE + 37)]
        # the pair the classic has-zero-byte trick gets wrong: a delimiter with delimiter ^ 0x01 right behind it in one word
        b[64:68] = [d, d ^ 0x01, d ^ 0x01, d ^ 0x80]
        out.append(SplitCase(f"adversarial_d{d:02x}", b, d, "adversarial"))
    return out


def all_split_cases():
    return length_cases() + placement_cases() + adversarial_cases()


def assert_split(case, pad, n_docs, tail_start, fetch):
    """The check of every split case: n_docs, tail_start, every offset, and windows with first > 0, against the
    reference.  fetch(first, n) -> uint64[n] are the offsets [first, first + n) as the code under test reports them."""
    want, wn, wtail = split_offsets(case.data, case.delim)
    what = f"{case.name} (padding 0x{pad:02x})"
    assert n_docs == wn, f"{what}: n_docs {n_docs}, want {wn}"
    assert tail_start == wtail, f"{what}: tail_start {tail_start}, want {wtail}"
    got = np.asarray(fetch(0, wn + 1), dtype=np.uint64)
    assert got.size == want.size, f"{what}: {got.size} offsets, want {want.size}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: offset {int(bad[0])} is {int(got[bad[0]])}, want {int(want[bad[0]])} ({bad.size} differ)"
    for first, n in {(1, wn), (wn, 1), (wn // 2, wn + 1 - wn // 2), (min(3, wn), min(5, wn + 1 - min(3, wn)))}:
        if first > 0 and n > 0:
            win = np.asarray(fetch(first, n), dtype=np.uint64)
            assert np.array_equal(win, want[first:first + n]), f"{what}: window [{first}, {first + n}) differs"


# ---------------------------------------------------------------------------
# cases of pfac_documents_matching

def doc_first_case(kind, n_docs):
    """Synthetic doc_first uint64[n_docs + 1] (non-decreasing counts prefix)."""
    d = np.arange(n_docs)
    if kind == "all_empty":
        cnt = np.zeros(n_docs, dtype=np.uint64)
    elif kind == "none_empty":
        cnt = (1 + d % 3).astype(np.uint64)
    elif kind == "alternating":
        cnt = (d % 2).astype(np.uint64) * np.uint64(2)
    elif kind == "runs":
        # one long run of each kind across a block-of-64 edge (40..100: empty) and across a group edge (4000..4200:
        # matching), the rest a seeded mix
        cnt = (np.random.default_rng(n_docs).random(n_docs) < 0.3).astype(np.uint64)
        cnt[40:100] = 0
        cnt[100:140] = 5
        cnt[4000:4200] = 1
        cnt[4200:4300] = 0
    else:
        raise ValueError(kind)
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(cnt, dtype=np.uint64)])


def assert_matching(ids, n_matching, doc_first, invert, what=""):
    """The check of every matching case: the count, strictly ascending ids, and the ids themselves."""
    want = matching_ids(doc_first, invert)
    ids = np.asarray(ids, dtype=np.uint64)
    assert n_matching == want.size, f"{what}: n_matching {n_matching}, want {want.size}"
    assert ids.size == want.size, f"{what}: {ids.size} ids, want {want.size}"
    assert ids.size < 2 or bool((ids[1:] > ids[:-1]).all()), f"{what}: the ids do not ascend"
    assert np.array_equal(ids, want), f"{what}: ids differ"
