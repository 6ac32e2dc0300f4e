"""The checks of tests/heapguard.py against seeded defects, with no device: a small numpy model of the heap writer
places runs from a list of per-tile counts into a GuardedBuffer on the host, and every defect it can be switched to
must be caught by the check that is there for it, by name; without a defect every check passes.  Also the capacity
ladder's contents and the read-side cases' precondition (the bytes past n_avail do complete a match)."""
import numpy as np
import pytest

from heapguard import (FILLS, LADDER_SMALL, READ_SEEDS, TILE, GuardedBuffer, GuardError, ReadCase, Want, capacity_ladder,
                       check_heap, heap_runs, judge_scan, padded_records, read_case_matcher, tix_of_wide_heap)

GRID = 4                                 # workgroups of the model's chunked placement
DEFECTS = ("block_ignores_capacity", "misaligned_run", "overlapping_runs", "count_off_by_one", "over_flag", "small_hint",
           "byte_before_ptr")


class HeapModel:
    """Writes the records of `tile_counts` into a heap of `capacity` records as the scan does: runs placed one after
    the other (`policy` "exact") or in chunks of capacity / (32 x GRID) records per workgroup, tiles dealt round robin
    ("chunked"; a run that does not fit the rest of its chunk opens the next one); 2-byte runs are allocated in
    multiples of 8.  `block_stores`: 2-byte runs leave as whole 16-byte blocks where the heap has room for the block,
    else record by record, each checked.  `defect` switches one rule off."""

    def __init__(self, tile_counts, rec_bytes, capacity, policy="exact", block_stores=True, defect=None, fill=FILLS[0]):
        counts = np.asarray(tile_counts, dtype=np.int64)
        self.rec_bytes, self.capacity, self.fill = rec_bytes, capacity, fill
        self.buf = GuardedBuffer(capacity * rec_bytes, fill=fill, device="cpu")
        mem = self.buf.tensor.numpy()
        dt = {2: np.uint16, 4: np.uint32, 8: np.uint64}[rec_bytes]
        alloc = (counts + 7) & ~7 if rec_bytes == 2 else counts
        first = np.zeros(counts.size, dtype=np.int64)
        chunk = (capacity // (32 * GRID)) & ~7 if policy == "chunked" else 0
        if chunk < 1024:
            chunk = 0
        cursor = 0
        room = [(0, 0)] * GRID                                  # (next free word, end) of every workgroup's chunk
        for t in range(counts.size):
            if alloc[t] == 0:
                continue
            if chunk == 0 or alloc[t] > chunk:
                first[t], cursor = cursor, cursor + int(alloc[t])
                continue
            at, end = room[t % GRID]
            if at + alloc[t] > end:
                at, end, cursor = cursor, cursor + chunk, cursor + chunk
            first[t] = at
            room[t % GRID] = (at + int(alloc[t]), end)
        self.used = cursor
        if defect == "misaligned_run":
            first[np.flatnonzero(counts)[1]] += 4
        if defect == "overlapping_runs":
            live = np.flatnonzero(counts)
            first[live[2]] = first[live[1]]
        for t in np.flatnonzero(counts):                        # the stores
            base, cnt = int(first[t]), int(counts[t])
            words = ((np.arange(cnt) * 13) & 4095 | (1 + t % 7) << 12).astype(dt)
            n_store = int(alloc[t]) if block_stores and rec_bytes == 2 else cnt
            fits = base + n_store <= capacity
            if defect == "block_ignores_capacity" and block_stores and base < capacity:
                fits = True                                     # (a block that starts inside the heap leaves whole)
            if not fits:
                n_store = max(0, min(cnt, capacity - base))
            run = np.zeros(n_store, dtype=dt)
            run[:min(cnt, n_store)] = words[:n_store]
            lo = self.buf.front + base * rec_bytes
            mem[lo:lo + n_store * rec_bytes] = run.view(np.uint8)
        if defect == "byte_before_ptr":
            mem[self.buf.front - 1] = 0
        shown = counts.copy()
        if defect == "count_off_by_one":
            shown[np.flatnonzero(counts)[0]] += 1
        self.tix = first.astype(np.uint64) | (shown.astype(np.uint64) << np.uint64(40))
        self.n = int(counts.sum())
        self.over = (self.used > capacity) != (defect == "over_flag")
        P = padded_records(counts, rec_bytes)
        self.hint = (self.n if defect == "small_hint" else P + P // 8 + 1024)

    def heap(self):
        dt = {2: np.uint16, 4: np.uint32, 8: np.uint64}[self.rec_bytes]
        return self.buf.host()[:min(self.used, self.capacity) * self.rec_bytes].view(dt)


def counts_for(seed, n_tiles=200):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 40, n_tiles)
    c[rng.random(n_tiles) < 0.3] = 0
    c[:4] = (5, 8, 9, 17)
    return c


def want_of(counts):
    pos = np.repeat(np.arange(counts.size) * TILE, counts) + np.concatenate([np.arange(c) for c in counts])
    return Want(pos, np.ones(pos.size, dtype=np.int32), counts.size * TILE)


def run_checks(m, counts, hints=()):
    """Everything the suite asks of one scan, over the model."""
    want = want_of(counts)
    judge_scan(m.capacity, want, m.n, counts.size, m.used, m.over, list(hints))
    if not m.over:
        check_heap(m.heap(), m.tix, m.rec_bytes, m.used, m.capacity, want.tile_counts, m.over)
    m.buf.check(what="the record heap")


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("block_stores", [True, False])
@pytest.mark.parametrize("policy", ["exact", "chunked"])
@pytest.mark.parametrize("rec_bytes", [2, 4, 8])
def test_no_defect_passes(rec_bytes, policy, block_stores, fill):
    counts = counts_for(1)
    P = padded_records(counts, rec_bytes)
    for cap in capacity_ladder(int(counts.sum()), P, P + P // 8 + 1024) + [80 * P, 80 * P + 5]:
        m = HeapModel(counts, rec_bytes, cap, policy, block_stores, None, fill)
        run_checks(m, counts)
        if policy == "chunked" and cap >= 80 * P:
            assert m.used > P                                   # (the model does reach the chunked placement)


def caught(defect, rec_bytes=2, policy="exact", capacity=None, hints=()):
    counts = counts_for(2)
    P = padded_records(counts, rec_bytes)
    m = HeapModel(counts, rec_bytes, P if capacity is None else capacity, policy, True, defect)
    if defect == "small_hint":                                  # the retry at the hint the defective model gave
        hints = [m.hint]
        m = HeapModel(counts, rec_bytes, m.hint, policy, True, None)
    run_checks(m, counts, hints)


def test_block_store_past_the_end_of_the_heap_is_caught():
    counts = counts_for(2)
    P = padded_records(counts, 2)
    with pytest.raises(GuardError, match=r"back guard of the record heap damaged: \d+ bytes, first at \+0"):
        caught("block_ignores_capacity", capacity=P - 3)        # the last run's block ends 3 records past the heap
    m = HeapModel(counts, 2, P - 3, "exact", True, None)        # the same heap without the defect: overflow, guards whole
    assert m.over
    m.buf.check()


def test_misaligned_run_is_caught():
    with pytest.raises(AssertionError, match="alignment: 1 runs of 2-byte records"):
        caught("misaligned_run")


@pytest.mark.parametrize("rec_bytes", [2, 4, 8])
def test_overlapping_runs_are_caught(rec_bytes):
    with pytest.raises(AssertionError, match="overlap: "):
        caught("overlapping_runs", rec_bytes)


@pytest.mark.parametrize("rec_bytes", [2, 4, 8])
def test_tile_count_off_by_one_is_caught(rec_bytes):
    with pytest.raises(AssertionError, match="tile count: 1 tiles differ"):
        caught("count_off_by_one", rec_bytes)


@pytest.mark.parametrize("capacity", [None, 100])
def test_over_flag_that_disagrees_is_caught(capacity):
    with pytest.raises(AssertionError, match="over flag: "):
        caught("over_flag", capacity=capacity)


def test_hint_below_the_padded_placement_is_caught():
    with pytest.raises(AssertionError, match="hint: overflow"):
        caught("small_hint")
    counts = counts_for(2)
    good = HeapModel(counts, 2, 0, "exact", True, None).hint
    run_checks(HeapModel(counts, 2, good, "chunked", True, None), counts, [good])


def test_byte_before_the_pointer_is_caught():
    with pytest.raises(GuardError, match=r"front guard of the record heap damaged: 1 bytes, first at -1, last at -1"):
        caught("byte_before_ptr")


@pytest.mark.parametrize("defect", [None] + list(DEFECTS))
def test_defects_are_named(defect):
    """Every defect fails, none passes (the table the tests above spell out one by one)."""
    if defect is None:
        caught(None)
        return
    with pytest.raises(AssertionError):
        caught(defect, capacity={"block_ignores_capacity": padded_records(counts_for(2), 2) - 3}.get(defect))


def test_payload_untouched_and_fill_value_writes():
    b = GuardedBuffer(37, fill=FILLS[0], device="cpu")
    b.check(payload_untouched=True)
    b.tensor.numpy()[b.front + 36] = 1
    b.check()
    with pytest.raises(GuardError, match=r"payload of buffer damaged: 1 bytes, first at \+36"):
        b.check(payload_untouched=True)
    # a stray write of the fill's own value hides under that fill and shows under the other one
    seen = []
    for fill in FILLS:
        b = GuardedBuffer(37, fill=fill, device="cpu")
        assert b.ptr % 16 == 0 and b.tensor.numel() == 37 + 2 * 4096
        b.tensor.numpy()[b.front + 37] = FILLS[0]
        try:
            b.check()
            seen.append(False)
        except GuardError:
            seen.append(True)
    assert seen == [False, True]


def test_wide_heap_index():
    counts = counts_for(3, 50)
    m = HeapModel(counts, 8, 5000, "exact")
    want = want_of(counts)
    rec = np.zeros(m.used, dtype=[("pos", "<u4"), ("state", "<u4")])
    gap = np.uint32(FILLS[0] * 0x01010101)
    rec["pos"], rec["state"] = gap, gap
    first, cnt = heap_runs(m.tix)
    for t in np.flatnonzero(cnt):
        rec["pos"][first[t]:first[t] + cnt[t]] = t * TILE + np.arange(cnt[t])
        rec["state"][first[t]:first[t] + cnt[t]] = 1
    tix = tix_of_wide_heap(rec, counts.size, FILLS[0])
    np.testing.assert_array_equal(tix[cnt > 0], m.tix[cnt > 0])
    check_heap(rec, tix, 8, m.used, 5000, want.tile_counts)
    rec[["pos", "state"]][first[3] + 1] = rec[first[2]]          # a record of another tile inside a run
    rec["pos"][first[3] + 1] = rec["pos"][first[2]]
    with pytest.raises(AssertionError, match="8-byte heap"):
        tix_of_wide_heap(rec, counts.size, FILLS[0])


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 10**6])
def test_ladder_holds_every_promised_edge_once(n):
    for padded in (n, (n + 7) & ~7, n + 8 * 250):
        hint = padded + padded // 8 + 65536
        lad = capacity_ladder(n, padded, hint)
        edges = set(LADDER_SMALL) | {n - 1, n, n + 1, padded - 8, padded - 1, padded, padded + 1, padded + 8, hint, hint + 3}
        assert min(lad) >= 0 and lad == sorted(lad)
        for e in edges:
            assert lad.count(e) == (1 if e >= 0 else 0), (e, lad)
        rungs = [c for c in lad if c >= 1024 and c not in edges]
        assert len(rungs) >= 4 and max(lad) == 4 * hint
        assert any(c % 8 for c in rungs) and any(c % 8 == 0 for c in rungs)


@pytest.mark.parametrize("seed", READ_SEEDS)
def test_read_cases_are_deterministic_and_their_poison_differs(seed, tmp_path):
    a, b = ReadCase(seed), ReadCase(seed)
    assert np.array_equal(a.data, b.data) and a.describe() == b.describe() and a.image == b.image
    assert a.off % 16 == 0 and a.off > 0 and a.n_owned <= a.n_avail
    m = read_case_matcher(a, str(tmp_path / "p.pat"))
    bounded, unbounded = a.expectations(m)
    m.close()
    a.check_poison(bounded, unbounded)
    assert unbounded.n > 0 and (bounded.n > 0 or a.n_avail < 64)


def test_read_cases_cover_what_they_claim():
    cases = [ReadCase(s) for s in READ_SEEDS]
    for kind in ("short", "long", "class"):
        mine = [c for c in cases if c.kind == kind]
        assert {c.n_avail - c.n_owned for c in mine} == {0, 1, mine[0].halo - 1, mine[0].halo, mine[0].halo + 1}
        assert min(c.n_owned for c in mine) <= 3 and max(c.n_owned for c in mine) > 3 * TILE
        assert any(c.crossing for c in mine) and any(not c.crossing for c in mine)
    assert max(c.M for c in cases) == 1022 and len({c.off for c in cases}) > 10
