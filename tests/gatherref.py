"""The checker of pfac_documents_gather and pfac_documents_matching_context (never the product): the rules of
include/pfac.h in numpy (`gather_ref`, `context_ids`), each pinned to a second form that knows nothing of the first
(`gather_ref_loop`: Python slices and b"".join; `context_ids_loop`: the definition, two nested loops) by
tests/test_gather_ref.py, the named cases, and the checks shared by the host and the GPU tests.  No expectation comes
from the device."""
import numpy as np

from splitref import MATCH_DOCS, MATCH_KINDS, doc_first_case

TILE = 4096
WIN = 1024                              # output bytes per window of the write pass (16 per lane)
BLOCK = 64                              # ids per block
U64_MAX = 2 ** 64 - 1


# ---------------------------------------------------------------------------
# the gather

def gather_ref(buf, offsets, ids):
    """(out uint8[out_bytes], out_off uint64[n_ids + 1]): document ids[k] of buf, back to back."""
    buf = np.asarray(buf, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    ids = np.asarray(ids, dtype=np.uint64).astype(np.int64)
    lens = off[ids + 1] - off[ids]
    out_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)])
    src = np.repeat(off[ids] - out_off[:-1], lens) + np.arange(int(out_off[-1]), dtype=np.int64)
    return buf[src], out_off.astype(np.uint64)


def gather_ref_loop(buf, offsets, ids):
    data = bytes(np.asarray(buf, dtype=np.uint8))
    off = [int(x) for x in offsets]
    pieces = [data[off[int(i)]:off[int(i) + 1]] for i in ids]
    out_off = [0]
    for p in pieces:
        out_off.append(out_off[-1] + len(p))
    return np.frombuffer(b"".join(pieces), dtype=np.uint8), np.array(out_off, dtype=np.uint64)


class GatherCase:
    """`ids` select documents of `data` cut at `offsets`; `need` names a precondition that test_gather_ref.py asserts on
    the host.  The offsets need not cover the input from 0, and only those of the selected documents must ascend."""

    def __init__(self, name, data, offsets, ids, need=None):
        self.name, self.need = name, need
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.ids = np.ascontiguousarray(ids, dtype=np.uint64)
        self.n, self.n_docs, self.n_ids = int(self.data.size), int(self.offsets.size) - 1, int(self.ids.size)

    def storage(self, pad):
        """The input followed by `pad` bytes up to the next tile boundary (at least 16 of them)."""
        size = (self.n + 16 + TILE - 1) // TILE * TILE
        s = np.full(size, pad, dtype=np.uint8)
        s[:self.n] = self.data
        return s

    def __repr__(self):
        return self.name


def _bytes(rng, n):
    return rng.integers(0, 256, n).astype(np.uint8)


def _case(name, lens, ids, seed, need=None, lead=0, trail=0):
    """Documents of the given lengths behind `lead` bytes that belong to none (the first offset is `lead`)."""
    lens = np.asarray(lens, dtype=np.int64)
    off = lead + np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)])
    return GatherCase(name, _bytes(np.random.default_rng(seed), int(off[-1]) + trail), off, ids, need)


N_IDS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 64 * 64 + 1)


def count_cases():
    """Every id count at which the passes change shape (block of 64, group of 1024, more than one group of groups),
    over 300 documents of seeded lengths 0..40, drawn with repeats."""
    out = []
    for n in N_IDS:
        rng = np.random.default_rng(4000 + n)
        out.append(_case(f"ids{n}", rng.integers(0, 41, 300), rng.integers(0, 300, n), 5000 + n))
    return out


def length_cases():
    short = np.random.default_rng(11).integers(1, 30, 40)
    big = 130 * TILE + 5
    return [
        _case("all_empty", np.zeros(200, np.int64), np.arange(200), 1, "out_empty"),
        _case("all_1_x5000", np.ones(5000, np.int64), np.arange(5000), 2, "segments_per_window"),
        _case("all_16_res0", np.full(200, 16), np.arange(200), 3, "res0"),
        _case("all_16_res5", np.full(200, 16), np.arange(200), 4, "res5", lead=5),
        _case("len_15_16_17", np.tile([15, 16, 17], 100)[:299], np.arange(299), 5, "partial_tail"),
        _case("one_5000_between_short", np.concatenate([short[:20], [5000], short[20:]]), np.arange(41), 6, "long_doc"),
        _case("one_doc_whole_input", [big], [0], 7, "whole_input"),
        _case("many_empty_then_one", np.concatenate([np.zeros(3000, np.int64), [37]]), np.arange(3001), 8, "empty_blocks"),
        # the whole output one byte short of, exactly, and one byte past a lane's 16-byte chunk and a wave's 1 KiB window
    ] + [_case(f"out_{n}", [n - 9, 0, 9], [0, 1, 2], 40 + n) for n in (15, 16, 17, 1023, 1024, 1025)]


def ladder_cases():
    """The first selected document's source residue through 0..15 and, independently, the residue of the output boundary
    behind it through 0..15: 16 cases walk the one, 16 the other, the partner moving by an odd stride."""
    out = []
    for i in range(32):
        src, cut = (i, (7 * i + 3) % 16) if i < 16 else ((3 * i + 2) % 16, i - 16)
        out.append(_case(f"ladder_src{src}_cut{cut}", [32 + cut, 40, 21], [0, 1, 2], 600 + i, ("ladder", src, cut), lead=src))
    return out


def id_list_cases():
    """One document set (150 seeded lengths 0..40, the last document unterminated and n_bytes % 16 != 0) under five id
    lists."""
    lens = np.random.default_rng(21).integers(0, 41, 150)
    lens[-1] = 23
    if int(lens.sum()) % 16 == 0:
        lens[0] += 1
    rng = np.random.default_rng(22)
    lists = {"all": np.arange(150), "every_other": np.arange(0, 150, 2), "last_only": np.array([149]),
             "reversed": np.arange(149, -1, -1), "repeats": np.sort(rng.integers(0, 150, 400))[::-1] // 3 * 3}
    return [_case(f"ids_{k}", lens, v, 23, ("id_list", k)) for k, v in lists.items()]


def all_gather_cases():
    return count_cases() + length_cases() + ladder_cases() + id_list_cases()


def assert_gather(case, out_bytes, out_off, out, fill=None, what=""):
    """The check of every gather case: the count, every offset, every byte (the first differing index in the message)
    and, with `fill`, that the bytes of `out` at and past out_bytes still hold it.  `out`: the output buffer as the code
    under test left it, out_bytes bytes or more."""
    want, want_off = gather_ref(case.data, case.offsets, case.ids)
    what = f"{case.name} {what}"
    assert out_bytes == want.size, f"{what}: out_bytes {out_bytes}, want {want.size}"
    got_off = np.asarray(out_off, dtype=np.uint64)
    assert got_off.size == want_off.size, f"{what}: {got_off.size} output offsets, want {want_off.size}"
    bad = np.flatnonzero(got_off != want_off)
    assert bad.size == 0, f"{what}: out_off[{int(bad[0])}] is {int(got_off[bad[0]])}, want {int(want_off[bad[0]])} ({bad.size} differ)"
    out = np.asarray(out, dtype=np.uint8)
    assert out.size >= want.size, f"{what}: {out.size} output bytes fetched, want {want.size}"
    bad = np.flatnonzero(out[:want.size] != want)
    assert bad.size == 0, (f"{what}: output byte {int(bad[0])} is 0x{int(out[bad[0]]):02x}, want 0x{int(want[bad[0]]):02x} "
                           f"({bad.size} differ, the last at {int(bad[-1])}; out_bytes {want.size})")
    if fill is not None:
        bad = np.flatnonzero(out[want.size:] != fill)
        assert bad.size == 0, f"{what}: a byte at out_bytes + {int(bad[0])} was written ({bad.size} past the output's end)"


# ---------------------------------------------------------------------------
# context lines

def context_ids(doc_first, before, after):
    """The ids of pfac_documents_matching_context: a boolean dilation of the matching flags by cumulative sums."""
    first = np.asarray(doc_first, dtype=np.uint64)
    n = first.size - 1
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    b, a = min(int(before), n), min(int(after), n)
    c = np.concatenate([np.zeros(1, np.int64), np.cumsum(first[1:] > first[:-1])])
    d = np.arange(n, dtype=np.int64)
    lo, hi = np.maximum(d - a, 0), np.minimum(d + b, n - 1)
    return np.flatnonzero(c[hi + 1] > c[lo]).astype(np.uint64)


def context_ids_loop(doc_first, before, after):
    first = [int(x) for x in doc_first]
    n = len(first) - 1
    out = []
    for d in range(n):
        for e in range(max(d - after, 0), min(d + before, n - 1) + 1):
            if first[e + 1] > first[e]:
                out.append(d)
                break
    return np.array(out, dtype=np.uint64)


def context_windows(n_docs):
    return [(0, 0), (1, 0), (0, 1), (2, 3), (63, 0), (0, 64), (65, 65), (n_docs, n_docs), (U64_MAX, U64_MAX)]


def context_cases():
    """(kind, n_docs, before, after) of every named context case."""
    return [(k, n, b, a) for n in MATCH_DOCS for k in MATCH_KINDS for b, a in context_windows(n)]


def sparse_first(n_docs, hits):
    """doc_first with one record in each document of `hits`."""
    cnt = np.zeros(n_docs, dtype=np.uint64)
    cnt[np.asarray(hits, dtype=np.int64)] = 1
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(cnt, dtype=np.uint64)])


def assert_context(ids, n_matching, doc_first, before, after, what=""):
    """The check of every context case: the count, strictly ascending ids (so each once), and the ids themselves."""
    want = context_ids(doc_first, before, after)
    ids = np.asarray(ids, dtype=np.uint64)
    what = f"{what} before={before} after={after}"
    assert n_matching == want.size, f"{what}: n_matching {n_matching}, want {want.size}"
    assert ids.size == want.size, f"{what}: {ids.size} ids, want {want.size}"
    assert ids.size < 2 or bool((ids[1:] > ids[:-1]).all()), f"{what}: the ids do not ascend strictly"
    bad = np.flatnonzero(ids != want)
    assert bad.size == 0, f"{what}: id {int(bad[0])} is {int(ids[bad[0]])}, want {int(want[bad[0]])} ({bad.size} differ)"
