"""Guard bands around the buffers a caller hands to the scan and to the record fetches, and the capacity contract of
include/pfac.h checked against them (shared by tests/test_gpu_heap_bounds.py, tests/test_heapguard_cases.py and
tools/fuzz.py guard).

The scan writes its records into a heap the caller may own, `capacity` records long.  The header promises that no byte
past capacity x record size is written, that the count is exact whatever the capacity, that the heap needs at most
capacity/16 + 1 % over the runs' own allocations, that pfac_scan_capacity_hint() names a capacity the same scan fits,
and that a walk never reads past n_avail.  Here a heap is a slice of a larger tensor whose other bytes hold a known
pattern (`GuardedBuffer`), the slice is exactly capacity x record size bytes long (not rounded up to a block), and
`verdict` states what one (scan, capacity) pair must deliver.  Every expectation comes from a CPU matcher (tests/orc.py,
tests/bigref.py, oracle/charclass_oracle.py) -- never from the device."""
import ctypes as C

import numpy as np

from orc import match_checksum

TILE = 4096
GUARD = 4096                            # bytes of guard on each side of a payload (a multiple of 16: the ABI's alignment)
FILLS = (0xA5, 0x3C)                    # every case runs with both: a stray write of one fill's own value shows under the other
E_ARG, E_STATE, E_OVERFLOW = -1, -7, -8
LADDER_SMALL = (0, 1, 7, 8, 9, 15, 16, 17)


class GuardError(AssertionError):
    """A byte outside a GuardedBuffer's payload changed (or, where the payload had to stay untouched, one inside)."""


class GuardedBuffer:
    """One uint8 tensor of front + n_bytes + back bytes, all `fill`; the payload is [front, front + n_bytes) and `ptr`
    its address.  n_bytes is taken as it is: a payload that ends inside a 16-byte block has its back guard start there,
    where a whole-block store past the end would land."""

    def __init__(self, n_bytes, front=GUARD, back=GUARD, fill=FILLS[0], device="cuda:0"):
        import torch
        assert front % 16 == 0 and front >= 0 and back >= 0 and n_bytes >= 0 and 0 <= fill < 256
        self.n_bytes, self.front, self.back, self.fill = int(n_bytes), int(front), int(back), int(fill)
        self.tensor = torch.full((self.front + self.n_bytes + self.back,), self.fill, dtype=torch.uint8, device=device)
        self.ptr = int(self.tensor.data_ptr()) + self.front
        assert self.ptr % 16 == 0, "the allocator returned a tensor that is not 16-byte aligned"
        if self.tensor.is_cuda:
            # the fill runs on torch's stream, what is tested writes on a slot's non-blocking stream: without this the
            # fill may land on top of a kernel launched right behind the constructor
            torch.cuda.synchronize(self.tensor.device)

    def payload(self):
        """The payload as a tensor view (uint8[n_bytes])."""
        return self.tensor[self.front:self.front + self.n_bytes]

    def host(self, n_bytes=None):
        """The payload's first n_bytes (default: all) on the host (a copy)."""
        return self.payload()[:self.n_bytes if n_bytes is None else n_bytes].cpu().numpy()

    def check(self, payload_untouched=False, what="buffer"):
        """Reads the guards back (with `payload_untouched` the whole tensor) and raises GuardError naming the first and
        last damaged offset of the front guard (relative to the payload's start: negative), of the back guard (relative
        to the payload's end) and, with `payload_untouched`, of the payload itself."""
        end = self.front + self.n_bytes
        parts = [("front guard", self.tensor[:self.front].cpu().numpy(), -self.front),
                 ("back guard", self.tensor[end:].cpu().numpy(), 0)]
        if payload_untouched:
            parts.append(("payload", self.tensor[self.front:end].cpu().numpy(), 0))
        bad = []
        for name, part, origin in parts:
            d = np.flatnonzero(part != self.fill)
            if d.size:
                rel = "the payload's end" if name == "back guard" else "the payload's start"
                bad.append(f"{name} of {what} damaged: {d.size} bytes, first at {int(d[0]) + origin:+d}, last at "
                           f"{int(d[-1]) + origin:+d} relative to {rel} (value 0x{int(part[d[0]]):02x}, fill 0x{self.fill:02x})")
        if bad:
            raise GuardError("; ".join(bad) + f" [payload {self.n_bytes} bytes]")


# ---------------------------------------------------------------------------
# the heap's layout

def heap_runs(tix):
    """(first, count) per tile of a tile index (PFAC_TIX_FIRST / PFAC_TIX_COUNT), int64."""
    tix = np.asarray(tix, dtype=np.uint64)
    return (tix & np.uint64((1 << 40) - 1)).astype(np.int64), (tix >> np.uint64(40)).astype(np.int64)


def padded_records(tile_counts, rec_bytes):
    """P: the heap records the runs themselves need -- every tile's count, rounded up to 8 for 2-byte records (a run
    leaves as whole 16-byte blocks and owns its padding)."""
    c = np.asarray(tile_counts, dtype=np.int64)
    return int(((c + 7) & ~7).sum()) if rec_bytes == 2 else int(c.sum())


def tix_of_wide_heap(records, n_tiles, fill):
    """The 8-byte form has no tile index a caller can fetch: rebuild one from the heap itself.  `records` is the heap
    [0, used) as {pos, state}; words still holding the buffer's fill are gaps.  Every tile's records must lie together
    and in ascending position."""
    gap = np.uint32(fill * 0x01010101)
    live = np.flatnonzero(~((records["pos"] == gap) & (records["state"] == gap)))
    tile = records["pos"][live].astype(np.int64) // TILE
    assert tile.size == 0 or int(tile.max()) < n_tiles, "8-byte heap: a record of a tile past the input"
    first = np.zeros(n_tiles, dtype=np.int64)
    cnt = np.bincount(tile, minlength=n_tiles).astype(np.int64)
    if live.size:
        start = np.flatnonzero(np.append(True, tile[1:] != tile[:-1]))
        assert np.unique(tile[start]).size == start.size, "8-byte heap: a tile's records lie in more than one run"
        run_len = np.diff(np.append(start, live.size))
        assert (live[start + run_len - 1] - live[start] + 1 == run_len).all(), "8-byte heap: a gap inside a tile's run"
        first[tile[start]] = live[start]
    return (first.astype(np.uint64) | (cnt.astype(np.uint64) << np.uint64(40)))


def check_heap(words_or_records, tix, rec_bytes, used, capacity, oracle_tile_counts, over=False):
    """The layout promises of one scan: `tix` its tile index, `used` / `over` what pfac_scan_format / pfac_scan_finish
    said, `words_or_records` the heap [0, used) (None after an overflow), `oracle_tile_counts` the CPU's records per
    4 KiB tile.  Returns P (padded_records)."""
    first, cnt = heap_runs(tix)
    want = np.asarray(oracle_tile_counts, dtype=np.int64)
    assert cnt.size == want.size, f"tile count: {cnt.size} index entries for {want.size} tiles"
    wrong = np.flatnonzero(cnt != want)
    assert wrong.size == 0, (f"tile count: {wrong.size} tiles differ from the oracle's histogram, first tile {int(wrong[0])}: "
                             f"{int(cnt[wrong[0]])} records, want {int(want[wrong[0]])}")
    assert (used <= capacity) == (not over), f"over flag: used {used}, capacity {capacity}, but overflow reported: {bool(over)}"
    live = cnt > 0
    f, c = first[live], cnt[live]
    alloc = (c + 7) & ~7 if rec_bytes == 2 else c
    if rec_bytes == 2:
        odd = np.flatnonzero(f % 8 != 0)
        assert odd.size == 0, f"alignment: {odd.size} runs of 2-byte records do not start on a multiple of 8, first at word {int(f[odd[0]]) if odd.size else 0}"
    o = np.argsort(f, kind="stable")
    f, c, alloc = f[o], c[o], alloc[o]
    if f.size:
        clash = np.flatnonzero(f[:-1] + c[:-1] > f[1:])
        assert clash.size == 0, (f"overlap: {clash.size} pairs of tile runs overlap, first [{int(f[clash[0]]) if clash.size else 0}, +"
                                 f"{int(c[clash[0]]) if clash.size else 0}) with the run at {int(f[clash[0] + 1]) if clash.size else 0}")
        clash = np.flatnonzero(f[:-1] + alloc[:-1] > f[1:])
        assert clash.size == 0, f"padding: {clash.size} runs start inside the padding of the run before them"
        assert f[0] >= 0 and int((f + alloc).max()) <= used, f"bounds: a run ends at {int((f + alloc).max())}, past used = {used}"
    P = int(alloc.sum())
    assert P == padded_records(want, rec_bytes)
    assert used >= P, f"bounds: used {used} is less than the runs' allocations {P}"
    slack = P + capacity // 16 + P // 100
    assert used <= slack, (f"slack: used {used} exceeds P + capacity/16 + P/100 = {P} + {capacity // 16} + {P // 100} = {slack} "
                           f"(capacity {capacity})")
    if words_or_records is not None:
        assert len(words_or_records) == used, f"heap: {len(words_or_records)} words fetched, used {used}"
    return P


def capacity_ladder(n_matches, padded, hint):
    """The capacities one scan is tried with, ascending, each once: the small block edges, the match count and the
    padded placement +- the block size, the hint, and a geometric ladder from 1024 to 4 x hint whose every second rung
    is moved off the block grid."""
    caps = set(LADDER_SMALL)
    caps.update((n_matches - 1, n_matches, n_matches + 1))
    caps.update((padded - 8, padded - 1, padded, padded + 1, padded + 8))
    caps.update((hint, hint + 3))
    c, k = 1024, 0
    while c <= 4 * hint:
        caps.add(c + (k % 2) * (1 + 2 * (k % 5)))
        c, k = c * 4, k + 1
    caps.add(4 * hint)
    return sorted(x for x in caps if x >= 0)


# ---------------------------------------------------------------------------
# what the CPU says about one scan, and the verdict on the device's

class Want:
    """The oracle's records of one scan (positions relative to the scan's start, all below n_owned)."""

    def __init__(self, pos, ids, n_owned):
        self.pos = np.asarray(pos, dtype=np.int64)
        self.ids = np.asarray(ids)
        assert self.pos.size == 0 or int(self.pos.max()) < n_owned
        self.n = int(self.pos.size)
        self.n_owned = int(n_owned)
        self.n_tiles = (self.n_owned + TILE - 1) // TILE
        self.tile_counts = np.bincount(self.pos // TILE, minlength=self.n_tiles).astype(np.int64)
        self.checksum = match_checksum(self.pos, self.ids)

    def padded(self, rec_bytes):
        return padded_records(self.tile_counts, rec_bytes)


def oracle_want(matcher, data, n_owned, n_avail):
    """Want of a scan of data[:n_avail] owning [0, n_owned); `matcher` has Oracle.scan_spec's interface."""
    pos, ids = matcher.scan_spec(np.ascontiguousarray(data[:n_avail]), None)
    keep = pos < n_owned
    return Want(pos[keep], ids[keep], n_owned)


def staging_of(g):
    """(buffers, records per buffer) the context's NEXT scan will use (pfac_scan_staging)."""
    i = g.info()
    return i["staging_buffers"], i["staging_records"]


def _overflow_codes(g, ptr, rec_bytes, n, n_tiles, fill):
    """The return codes of the record consumers after a scan that overflowed, each given buffers it could legally fill."""
    L, ctx = g._L, g._ctx
    one = np.zeros(1, dtype=np.dtype([("pos", "<u4"), ("state", "<u4")]))
    out = GuardedBuffer(8, fill=fill)
    tix = GuardedBuffer(max(n_tiles, 1) * 8, fill=fill)
    nb, chk = C.c_uint64(0), C.c_uint64(0)
    codes = {"pfac_records_d2h": L.pfac_records_d2h(ctx, 0, ptr, one.ctypes.data, 0, 1),
             "pfac_records_expand": L.pfac_records_expand(ctx, 0, ptr, 0, 1, out.ptr),
             "pfac_records_packed_device": L.pfac_records_packed_device(ctx, 0, ptr, 0, 0, tix.ptr),
             "pfac_emit_text_device": L.pfac_emit_text_device(ctx, 0, ptr, 0, C.byref(nb)),
             "pfac_records_checksum": L.pfac_records_checksum(ctx, 0, ptr, n, 0, C.byref(chk))}
    g.sync(0)
    out.check(payload_untouched=True, what="the expand output after an overflow")
    tix.check(payload_untouched=True, what="the tile index output after an overflow")
    return codes


def judge_scan(capacity, want, n, n_tiles, used, over, hints):
    """What the numbers of one finished scan must satisfy whatever its heap holds: `n` / `over` from pfac_scan_finish,
    `n_tiles` / `used` from pfac_scan_format, `hints` the capacity hints of the earlier scans of the same input."""
    assert n == want.n, f"count: {n} matches, the oracle has {want.n} (overflow {over})"
    assert n_tiles == want.n_tiles, f"{n_tiles} tiles, want {want.n_tiles}"
    assert over == (used > capacity), f"over flag: overflow reported {over}, used {used}, capacity {capacity}"
    if capacity < want.n:
        assert over, f"a capacity below the match count {want.n} did not overflow (used {used})"
    fits = [h for h in hints if capacity >= h]
    assert not (over and fits), f"hint: overflow (used {used}) at a capacity at or above an earlier hint of this scan {fits[:3]}"


def verdict(g, table, want, d_input, n_owned, n_avail, capacity, rec_bytes, fill, hints, where=""):
    """One scan into a GuardedBuffer of exactly `capacity` records, and everything the capacity contract says about it.
    `hints`: the hints of the earlier scans of this input in this context (a capacity at or above any of them must
    fit); this scan's own hint is appended.  Returns {"used", "P", "over", "staging", "hint"}; raises AssertionError
    (GuardError for a damaged guard) naming `where`."""
    stg = staging_of(g)                                     # the layout THIS scan runs with
    buf = GuardedBuffer(capacity * rec_bytes, fill=fill)
    tag = f"{where} capacity {capacity} fill 0x{fill:02x} staging {stg}"
    try:
        g.scan_async(n_owned, n_avail, d_input=d_input, d_records=buf.ptr, capacity=capacity)
        n, over = g.scan_finish(0, allow_overflow=True)
        rb, n_tiles, used = g.scan_format(0)
        hint = g.capacity_hint(0)
        assert rb == rec_bytes, f"record width {rb}, want {rec_bytes}"
        judge_scan(capacity, want, n, n_tiles, used, over, hints)
        P = want.padded(rb)
        if not over:
            rec = g.records_to_host(n, d_records=buf.ptr)
            assert np.array_equal(rec["pos"].astype(np.int64), want.pos), "records: positions differ from the oracle's"
            assert np.array_equal(table.idmap[rec["state"]], want.ids), "records: pattern ids differ from the oracle's"
            if rb == 8:
                heap = buf.host(used * 8).view(rec.dtype)
                tix = tix_of_wide_heap(heap, n_tiles, fill)
            else:
                heap, tix = g.packed_to_host(0, d_records=buf.ptr)
            check_heap(heap, tix, rb, used, capacity, want.tile_counts, over)
            assert g.checksum(n, d_records=buf.ptr) == want.checksum, "checksum differs from the oracle's"
        else:
            codes = _overflow_codes(g, buf.ptr, rb, n, n_tiles, fill)
            expect = dict.fromkeys(codes, E_OVERFLOW)
            if rb == 8:
                expect["pfac_records_packed_device"] = E_STATE      # (no compact form to hand out: checked first)
            assert codes == expect, f"after an overflow: return codes {codes}, want {expect}"
        buf.check(what="the record heap")
    except GuardError as e:
        raise GuardError(f"{tag}: {e}") from e
    except AssertionError as e:
        raise AssertionError(f"{tag}: {e}") from e
    hints.append(hint)
    return {"used": used, "P": P, "over": over, "staging": stg, "hint": hint}


# ---------------------------------------------------------------------------
# the read side: windows of one buffer whose bytes past n_avail would complete a match

READ_BUF = 8 * TILE + 2048              # bytes of the one device buffer the windows lie in
READ_KINDS = ("short", "long", "class")
READ_SEEDS = list(range(60))            # every kind x every halo distance x every size class
CLASS_SHAPE = "dag-26-to-1"             # the class table: tests/classfuzz.py SHAPES (two lines [a-z]bc / [a-z]bd, one DAG)
CLASS_LONGEST = b"qbd"                  # an instance of its longest line


class ReadCase:
    """One window of the read-side test: the buffer's bytes, the pattern set, d_input = base + off (off a multiple of
    16, text in front of it), n_owned and n_avail.  A copy of the longest pattern starts on the last owned byte, so it
    ends at n_owned + halo: past n_avail -- completed only by bytes the scan may not read -- whenever n_avail -
    n_owned < halo; another lies across a tile edge of the window.  `seed` alone fixes everything."""

    def __init__(self, seed):
        self.seed = seed
        rng = np.random.default_rng([seed, 0x52454144])
        self.kind = READ_KINDS[seed % 3]
        which_d = (seed // 3) % 5
        size_class = (seed // 15) % 4
        if self.kind == "short":
            alphabet = np.frombuffer(b"abc", dtype=np.uint8)
            self.lines = [b"a", b"ab", b"abc", b"bca", b"cc", b"abca"]
            longest = self.lines[-1]
        elif self.kind == "long":
            alphabet = np.frombuffer(b"abcd", dtype=np.uint8)
            base = np.random.default_rng(1022).integers(97, 101, 1022).astype(np.uint8).tobytes()     # (one table for all)
            self.lines = [base, base[:1021], base[3:1020], base[500:540], base[:2], base[:1], b"abd", b"dc"]
            longest = base
        else:
            alphabet = np.frombuffer(b"abcdq", dtype=np.uint8)
            self.lines = None
            longest = CLASS_LONGEST
        if self.kind == "class":
            from classfuzz import shape_image
            self.image = shape_image(CLASS_SHAPE)
        else:
            self.image = b"".join(p + b"\n" for p in self.lines)
        self.M = len(longest)
        self.halo = self.M - 1
        d = (0, 1, self.halo - 1, self.halo, self.halo + 1)[which_d]
        self.n_owned = int((1 + rng.integers(0, 3), 16 + rng.integers(-2, 3), TILE + rng.integers(-3, 4),
                            3 * TILE + rng.integers(1, TILE))[size_class])
        self.n_avail = self.n_owned + d
        self.off = 16 * int(rng.integers(1, 40))
        assert self.off + self.n_avail + self.M + 16 <= READ_BUF
        data = alphabet[rng.integers(0, alphabet.size, READ_BUF)]
        pat = np.frombuffer(longest, dtype=np.uint8)
        edge = self.off + self.n_owned - 1                      # the last owned byte
        if self.n_owned > TILE:                                 # across the window's first tile edge
            at = self.off + TILE - self.M // 2
            data[at:at + self.M] = pat
        data[edge:edge + self.M] = pat
        self.data = data
        self.crossing = d < self.halo                           # whether a match can start owned and end past n_avail

    def window(self, extra=0):
        return self.data[self.off:self.off + self.n_avail + extra]

    def describe(self):
        return (f"read case {self.seed} ({self.kind}): offset {self.off}, n_owned {self.n_owned}, n_avail {self.n_avail}, "
                f"halo {self.halo}")

    def expectations(self, matcher):
        """(bounded, unbounded): the records of the window as the scan may see it, and as it would look with the
        max_pat_len bytes behind n_avail."""
        bounded = oracle_want(matcher, self.window(), self.n_owned, self.n_avail)
        unbounded = oracle_want(matcher, self.window(self.M), self.n_owned, self.n_avail + self.M)
        return bounded, unbounded

    def check_poison(self, bounded, unbounded):
        """The precondition: the bytes past n_avail would add a record exactly when a match can cross n_avail."""
        if self.crossing:
            assert unbounded.n > bounded.n, f"{self.describe()}: the bytes past n_avail complete no match: the case proves nothing"
        else:
            assert unbounded.n == bounded.n, f"{self.describe()}: a match past the full halo?"


def read_case_matcher(case, path):
    """Writes the case's pattern image to `path` and returns its CPU matcher (Oracle.scan_spec's interface): the CPU
    oracle for plain lines, the brute-force class matcher (oracle/charclass_oracle.py) for the class image."""
    with open(path, "wb") as f:
        f.write(case.image)
    if case.kind == "class":
        from classfuzz import ClassMatcher
        return ClassMatcher(case.image)
    from orc import Oracle
    return Oracle(path, 1, 1)
