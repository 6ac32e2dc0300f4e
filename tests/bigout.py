"""One reference for "an output made of source runs" (the checker, never the product), and the cases whose outputs pass
2^32 bytes (shared by tests/test_bigout_ref.py, which pins both on the CPU, and tests/test_gpu_outputs_past_4g.py).

A gather, a find-and-replace and a per-document find-and-replace all produce a concatenation of runs, each copied from
the input or from the replacement bytes.  `Segments` describes such an output without materialising it:

    out_off uint64[n_seg + 1]   where run k starts in the output (the last entry: the output's length)
    src_off int64[n_seg]        where run k starts in `source` = cat(input, replacement bytes)

The tables are built on the CPU from the definitions of tests/gatherref.py, tests/replref.py and tests/docreplref.py and
from the CPU oracle's records -- never from the device.  `window` reads any byte range of the expected output from them;
it is written once over an array namespace, so the same lines run with numpy on the host and with torch on the device,
where `assert_device_equals` walks an output of several GB in chunks.  All index arithmetic is int64."""
import numpy as np

from docref import oracle_per_doc, random_offsets
from llref import greedy, line_lengths
from orc import Oracle
from replref import rep_table

G4 = 1 << 32
OUT_MIN, OUT_MAX = G4 + (1 << 20), G4 + (G4 >> 2)          # condition (a) of every big case
CHUNK = 64 << 20                        # output bytes compared at a time: about 2 GiB of int64 temporaries


class Segments:
    def __init__(self, out_off, src_off):
        self.out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
        self.src_off = np.ascontiguousarray(src_off, dtype=np.int64)
        assert self.out_off.size == self.src_off.size + 1 and self.out_off[0] == 0
        assert self.out_off[-1] < 1 << 62 and bool((self.out_off[1:] >= self.out_off[:-1]).all())
        self._dev = {}

    @property
    def total(self):
        return int(self.out_off[-1])

    @property
    def n_seg(self):
        return int(self.src_off.size)

    def tables(self, like):
        """(out_off as int64, src_off) as arrays of the kind of `like`: numpy, or torch tensors on its device."""
        if isinstance(like, np.ndarray):
            return self.out_off.view(np.int64), self.src_off
        key = str(like.device)
        if key not in self._dev:
            import torch
            self._dev[key] = (torch.from_numpy(self.out_off.view(np.int64).copy()).to(like.device),
                              torch.from_numpy(self.src_off.copy()).to(like.device))
        return self._dev[key]

    def release(self):
        self._dev.clear()


def _namespace(a):
    if isinstance(a, np.ndarray):
        return np, {}
    import torch
    return torch, {"device": a.device}


def window(seg, source, a, b):
    """Bytes [a, b) of the expected output: the run of byte i is the last one that starts at or before i (so of several
    empty runs at one offset, and the run behind them, the last), and the byte is source[src_off[k] + (i - out_off[k])]."""
    xp, dev = _namespace(source)
    out_off, src_off = seg.tables(source)
    i = xp.arange(int(a), int(b), dtype=xp.int64, **dev)
    k = xp.searchsorted(out_off, i, side="right") - 1
    return source[src_off[k] + (i - out_off[k])]


def segment_of(seg, i):
    return int(np.searchsorted(seg.out_off.view(np.int64), np.int64(i), side="right")) - 1


# ---------------------------------------------------------------------------
# the constructors

def gather_segments(offsets, ids):
    """gatherref.gather_ref's definition: run k is document ids[k] of the input."""
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    ids = np.asarray(ids, dtype=np.uint64).astype(np.int64)
    lens = off[ids + 1] - off[ids]
    out_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)])
    return Segments(out_off, off[ids])


def _replace_runs(n_source, entry, n_owned, pos, lens, ids, table):
    """(run lengths, run sources) of the formula at the top of tests/replref.py: for every pick the gap in front of it
    and its replacement, then the tail gap.  `n_source`: where the replacement bytes start in the source."""
    off, _ = table
    pos = np.asarray(pos, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    entry, n_owned = int(entry), int(n_owned)
    n = pos.size
    ends = pos + lens
    prev = np.concatenate(([entry], ends[:-1])) if n else np.empty(0, dtype=np.int64)
    assert bool((pos >= prev).all()), "picks overlap or start before the entry"
    run_len = np.empty(2 * n + 1, dtype=np.int64)
    run_src = np.empty(2 * n + 1, dtype=np.int64)
    run_len[0:2 * n:2], run_src[0:2 * n:2] = pos - prev, prev
    run_len[1:2 * n:2], run_src[1:2 * n:2] = off[ids + 1] - off[ids], int(n_source) + off[ids]
    c = int(ends[-1]) if n else entry
    run_len[-1], run_src[-1] = max(n_owned - c, 0), c
    return run_len, run_src


def replace_segments(entry, n_owned, pos, lens, ids, table, n_source=None):
    """The output of replref.splice for picks (pos, lens, ids) in ascending pos; the source is cat(input[:n_source],
    table's bytes), n_source = n_owned unless given (an input with a halo is longer than its owned range)."""
    n_source = n_owned if n_source is None else n_source
    run_len, run_src = _replace_runs(n_source, entry, n_owned, pos, lens, ids, table)
    return Segments(np.concatenate([np.zeros(1, np.int64), np.cumsum(run_len)]), run_src)


def doc_replace_segments(off, first, pos, lens, ids, table, n_source):
    """docreplref.per_doc's output: every document [off[d], off[d + 1]) replaced on its own from cursor 0 (`first`
    indexes its picks, positions relative to the document), concatenated.  -> (Segments, doc_out_off uint64[n_docs + 1])."""
    off = np.asarray(off, dtype=np.uint64).astype(np.int64)
    first = np.asarray(first, dtype=np.uint64).astype(np.int64)
    rl, rs, doc_out, at = [], [], [0], 0
    for d in range(off.size - 1):
        s = slice(int(first[d]), int(first[d + 1]))
        a, b = int(off[d]), int(off[d + 1])
        run_len, run_src = _replace_runs(n_source - a, 0, b - a, pos[s], lens[s], ids[s], table)
        rl.append(run_len)
        rs.append(run_src + a)
        at += int(run_len.sum())
        doc_out.append(at)
    rl = np.concatenate(rl) if rl else np.zeros(0, np.int64)
    rs = np.concatenate(rs) if rs else np.zeros(0, np.int64)
    return Segments(np.concatenate([np.zeros(1, np.int64), np.cumsum(rl)]), rs), np.array(doc_out, dtype=np.uint64)


def replace_source(data, table):
    _, rb = table
    return np.concatenate([np.asarray(data, dtype=np.uint8), np.frombuffer(rb, dtype=np.uint8)])


# ---------------------------------------------------------------------------
# the walk over a device output

def assert_device_equals(seg, d_source, d_out, out_bytes, chunk=CHUNK, what="output"):
    """Every byte of an output of `out_bytes` bytes against `window` in its torch form, `chunk` bytes at a time.  `d_out`:
    the output as a device tensor, or fetch(first, n) -> host bytes (a slot-owned output, read through the fetch under
    test and uploaded again).  A difference is reported by the first differing byte index and its run."""
    import torch
    assert out_bytes == seg.total, f"{what}: {out_bytes} output bytes, want {seg.total}"
    for a in range(0, seg.total, chunk):
        b = min(a + chunk, seg.total)
        want = window(seg, d_source, a, b)
        got = torch.from_numpy(np.asarray(d_out(a, b - a))).to(d_source.device) if callable(d_out) else d_out[a:b]
        if not torch.equal(got, want):
            bad = torch.nonzero(got != want).flatten()
            i = a + int(bad[0])
            k = segment_of(seg, i)
            raise AssertionError(f"{what}: output byte {i} is 0x{int(got[i - a]):02x}, want 0x{int(want[i - a]):02x} (run {k} of "
                                 f"{seg.n_seg}: output offset {int(seg.out_off[k])}, source offset {int(seg.src_off[k])}; "
                                 f"{int(bad.numel())} bytes differ in [{a}, {b}), out_bytes {seg.total})")
        del want, got


def conditions(seg, source, what):
    """Conditions (a) to (c) of a big case, asserted on the CPU from two 4 KiB windows: (a) the output ends between
    2^32 + 2^20 and 1.25 x 2^32 bytes, (b) a non-empty run starts below 2^32 and ends above it, (c) at least 90 % of the
    first 4096 bytes differ from the bytes 2^32 further on, so that a store whose offset wraps shows."""
    assert OUT_MIN <= seg.total <= OUT_MAX, f"{what}: (a) out_bytes {seg.total} outside [{OUT_MIN}, {OUT_MAX}]"
    k = segment_of(seg, G4)
    assert int(seg.out_off[k]) < G4 < int(seg.out_off[k + 1]), f"{what}: (b) a run boundary lies exactly at 2^32"
    low, high = window(seg, source, 0, 4096), window(seg, source, G4, G4 + 4096)
    differ = int((low != high).sum())
    assert differ >= 4096 * 9 // 10, f"{what}: (c) only {differ} of 4096 bytes differ between [0, 4096) and 2^32 + [0, 4096)"


# ---------------------------------------------------------------------------
# the big gather

class BigGather:
    """About 200 MB of seeded bytes in 50 000 documents of 0 .. 8191 bytes (some empty, one run of 100 empty ones) and
    about 1.1 M ids drawn with repeats, runs of 100 consecutive ids of empty documents among them: 4.5 GB of output."""
    N_DOCS, N_IDS, EMPTY_AT, EMPTY_RUN = 50_000, 1_100_003, 20_000, 100

    def __init__(self, with_data=True):
        rng = np.random.default_rng(20261019)
        lens = rng.integers(0, 8192, self.N_DOCS)
        lens[rng.integers(0, self.N_DOCS, 500)] = 0
        lens[self.EMPTY_AT:self.EMPTY_AT + self.EMPTY_RUN] = 0
        self.offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)]).astype(np.uint64)
        ids = rng.integers(0, self.N_DOCS, self.N_IDS)
        run = np.arange(self.EMPTY_AT, self.EMPTY_AT + self.EMPTY_RUN)
        self.empty_runs_at = [0, 64 * 1000 + 5, 1 << 20, self.N_IDS - self.EMPTY_RUN]     # at the start, inside a block, at 2^20, at the end
        for at in self.empty_runs_at:
            ids[at:at + self.EMPTY_RUN] = run
        self.ids = ids.astype(np.uint64)
        self.n = int(self.offsets[-1])
        self.n_docs, self.n_ids = self.N_DOCS, self.N_IDS
        self.seg = gather_segments(self.offsets, self.ids)
        self.data = np.random.default_rng(7).integers(0, 256, self.n, dtype=np.uint8) if with_data else None


class EdgeGather:
    """One document set of a little over 64 MiB for the outputs at which the write grid changes from one window per
    wave to four: ids drawn with repeats up to just under 64 MiB, then one last id whose document is trimmed so that
    the output has exactly the wanted length."""
    SIZES = tuple((64 << 20) + d for d in (-1, 0, 1, 1025, 3 * 1024 + 7, 16 * 1024 - 15))
    N_DOCS, LAST_LEN = 17_000, 40_000

    def __init__(self, with_data=True):
        rng = np.random.default_rng(6400)
        lens = rng.integers(0, 8192, self.N_DOCS)
        lens[-1] = self.LAST_LEN
        self.base_offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)])
        draw = rng.integers(0, self.N_DOCS - 1, 20_000)
        cum = np.cumsum(lens[draw])
        k = int(np.searchsorted(cum, min(self.SIZES) - 1, side="right"))        # the ids in front leave the last one >= 1 byte
        self.prefix = int(cum[k - 1])
        self.ids = np.append(draw[:k], self.N_DOCS - 1).astype(np.uint64)
        self.n_docs, self.n_ids = self.N_DOCS, int(self.ids.size)
        self.n = int(self.base_offsets[-1])
        assert 1 <= min(self.SIZES) - self.prefix and max(self.SIZES) - self.prefix <= self.LAST_LEN
        self.data = np.random.default_rng(8).integers(0, 256, self.n, dtype=np.uint8) if with_data else None

    def offsets(self, out_bytes):
        off = self.base_offsets.copy()
        off[-1] = off[-2] + (out_bytes - self.prefix)
        return off.astype(np.uint64)


# ---------------------------------------------------------------------------
# the big replace

class BigReplace:
    """1.74 MiB over {a, b, c, d} under five literal patterns: `ab` carries a replacement of 65 536 seeded bytes, `abc`
    overrides it by leftmost-longest with 1 000 bytes, `d` is deleted (picks back to back wherever d repeats), `cc`
    becomes 17 bytes and `ca` 2.  Records from Oracle.scan_spec, the selection from llref.greedy, lengths from the
    pattern lines.  Two configurations: the whole input from entry 0, and entry 2 with an owned range that ends inside
    a pick of `abc` (a halo of 37 bytes, exit 2).  The same input cut into 300 documents is the per-document case."""
    LINES = [b"ab", b"abc", b"d", b"cc", b"ca"]
    N, HALO, N_DOCS = 1_825_003, 37, 300

    def __init__(self, tmp_dir):
        rng = np.random.default_rng(650)
        self.reps = {1: rng.integers(0, 256, 65536).astype(np.uint8).tobytes(), 2: rng.integers(0, 256, 1000).astype(np.uint8).tobytes(),
                     3: b"", 4: rng.integers(0, 256, 17).astype(np.uint8).tobytes(), 5: b"AC"}
        self.table = rep_table(self.reps)
        data = np.frombuffer(b"abcd", dtype=np.uint8)[rng.integers(0, 4, self.N)]
        self.n = self.N
        self.n_owned_halo = self.N - self.HALO
        data[self.n_owned_halo - 3:self.n_owned_halo + 2] = np.frombuffer(b"ddabc", dtype=np.uint8)    # the pick that crosses
        self.data = data
        self.path = str(tmp_dir / "bigreplace.pat")
        with open(self.path, "wb") as f:
            f.write(b"".join(p + b"\n" for p in self.LINES))
        self.ll = line_lengths(self.path)
        self.source = replace_source(self.data, self.table)
        o = Oracle(self.path, 1, 1)
        self.pos, self.ids = o.scan_spec(self.data)
        self.doc_off = random_offsets(rng, self.n, self.N_DOCS, empties=5)
        self.docs = oracle_per_doc(o, self.data, self.doc_off)
        o.close()
        self.configs = {"whole": self._config(0, self.n), "halo": self._config(2, self.n_owned_halo)}

    def _config(self, entry, n_owned):
        keep = self.pos < n_owned
        pos, ids = self.pos[keep], self.ids[keep]
        sel, ex = greedy(pos, self.ll[ids], entry, n_owned)
        seg = replace_segments(entry, n_owned, pos[sel], self.ll[ids[sel]], ids[sel], self.table, n_source=self.n)
        return {"entry": entry, "n_owned": n_owned, "exit": ex, "seg": seg, "picks": (pos[sel], ids[sel])}

    def per_document(self):
        """-> (Segments, doc_out_off): llref.greedy on every document's own records."""
        first, pos, ids = self.docs
        sfirst, sp, si = [0], [], []
        for d in range(self.doc_off.size - 1):
            s = slice(int(first[d]), int(first[d + 1]))
            sel, _ = greedy(pos[s], self.ll[ids[s]], 0, int(self.doc_off[d + 1]) - int(self.doc_off[d]))
            sp.append(pos[s][sel])
            si.append(ids[s][sel])
            sfirst.append(sfirst[-1] + sel.size)
        sp, si = np.concatenate(sp), np.concatenate(si)
        return doc_replace_segments(self.doc_off, np.array(sfirst), sp, self.ll[si], si, self.table, self.n)


# ---------------------------------------------------------------------------
# the big text

def digits(x):
    """Decimal digits of every entry of a non-negative int64 array."""
    x = np.asarray(x, dtype=np.int64)
    d = np.ones(x.shape, dtype=np.int64)
    for k in range(1, 19):
        d += x >= 10 ** k
    return d


class BigText:
    """8 MiB of `a` broken by seeded other bytes, under the sixteen patterns a, aa, ..., a^16 (16 final states: 2-byte
    records): position p matches the first min(16, run to the next other byte) patterns, so a position has 0 to 16
    records; a few stretches of 10 000 other bytes leave tiles empty.  `base` puts 10^9 inside the scanned range.  The
    expected (pos, id) sequence comes from the run lengths; a line is 12 + max(4, digits(base + pos)) + 16 + digits(id)
    + 1 bytes."""
    N, BASE, N_PAT = (1 << 23) + 5, 10 ** 9 - 3_000_000, 16

    def __init__(self, tmp_dir):
        rng = np.random.default_rng(1600)
        runs = rng.integers(0, 130, self.N // 60)
        at = np.cumsum(runs + 1) - 1                        # a break behind every run
        at = at[at < self.N]
        data = np.full(self.N, ord("a"), dtype=np.uint8)
        data[at] = rng.integers(ord("b"), ord("z") + 1, at.size)
        for s in (40_000, 3_000_000 - 5_000, 6_000_000, self.N - 30_000):
            data[s:s + 10_000] = rng.integers(ord("b"), ord("z") + 1, 10_000)
        self.data, self.n, self.base = data, self.N, self.BASE
        self.path = str(tmp_dir / "bigtext.pat")
        with open(self.path, "wb") as f:
            f.write(b"".join(b"a" * k + b"\n" for k in range(1, self.N_PAT + 1)))
        # per position: bytes to the next byte that is not `a` (the input's end counts as one)
        other = np.flatnonzero(data != ord("a"))
        nxt = np.append(other, self.n)[np.searchsorted(other, np.arange(self.n), side="left")]
        self.count = np.minimum(nxt - np.arange(self.n), self.N_PAT).astype(np.int64)
        self.first = np.concatenate([np.zeros(1, np.int64), np.cumsum(self.count)])      # records in front of position p
        self.lines = int(self.first[-1])

    def records(self, lo=0, hi=None):
        """(pos int64, id int64) of the records of positions [lo, hi), in the oracle's order: ids 1 .. count at each."""
        hi = self.n if hi is None else hi
        c = self.count[lo:hi]
        pos = np.repeat(np.arange(lo, hi, dtype=np.int64), c)
        ids = np.arange(pos.size, dtype=np.int64) - np.repeat(self.first[lo:hi] - self.first[lo], c) + 1
        return pos, ids

    def line_lengths(self, pos, ids):
        return 12 + np.maximum(4, digits(self.base + pos)) + 16 + digits(ids) + 1

    def all_line_ends(self, hi=None):
        """(pos, ids, ends) of every record of the positions [0, hi): `line_lengths` with the position's digits taken
        once per position, and the text offset behind every line."""
        hi = self.n if hi is None else hi
        pos, ids = self.records(0, hi)
        dpos = np.maximum(4, digits(self.base + np.arange(hi, dtype=np.int64)))
        lens = np.repeat(29 + dpos, self.count[:hi]) + 1 + (ids >= 10)
        return pos, ids, np.cumsum(lens)

    def text_bytes(self, hi=None):
        """The text's length for the positions [0, hi), summed per position: count x (29 + position digits) + the digits
        of the ids 1 .. count."""
        c = self.count[:hi]
        p = np.arange(c.size, dtype=np.int64)
        return int((c * (29 + np.maximum(4, digits(self.base + p))) + c + np.maximum(c - 9, 0)).sum())

    def format(self, pos, ids):
        return "".join("At position %4d, match pattern %d\n" % (self.base + int(p), int(i)) for p, i in zip(pos, ids)).encode()

    def assert_oracle_agrees(self, span=256 << 10):
        """`records` against Oracle.scan_spec on the first and the last `span` bytes (the oracle reads the 15 bytes
        behind a range too, where there are any, and its records that start inside the range count)."""
        o = Oracle(self.path, 1, 1)
        for lo, hi in ((0, span), (self.n - span, self.n)):
            pos, ids = self.records(lo, hi)
            op, oi = o.scan_spec(np.ascontiguousarray(self.data[lo:min(hi + self.N_PAT - 1, self.n)]))
            keep = op < hi - lo
            np.testing.assert_array_equal(op[keep] + lo, pos)
            np.testing.assert_array_equal(oi[keep], ids)
        o.close()

    def quarter(self):
        """The end of a prefix of about a quarter of the input that ends behind a byte that is not `a`: the records of
        its positions are those of the whole input."""
        q = self.n // 4
        return q + int(np.flatnonzero(self.data[q:] != ord("a"))[0]) + 1
