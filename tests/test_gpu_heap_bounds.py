"""Where the scan writes, and what a record capacity means (GPU tests, -m gpu on an MI355X).  Every record heap, every
fetch output here is a tests/heapguard.py GuardedBuffer of exactly the size the ABI asks for, with 4 KiB of known bytes
on both sides, run once with each of two fills; the promises of include/pfac.h about capacity, overflow, the capacity
hint and n_avail are asserted for every kernel variant of tests/passfuzz.py's KNOBS.  Expectations come from the CPU
oracle and the brute-force class matcher, never from the device.  No case provokes a fault: every capacity is a legal
argument, every pointer lies inside a tensor the test owns, and a guard is checked by reading it back."""
import os
import time

import numpy as np
import pytest

from heapguard import (E_ARG, E_STATE, FILLS, READ_BUF, READ_SEEDS, TILE, GuardedBuffer, ReadCase, capacity_ladder, oracle_want,
                       read_case_matcher, staging_of, verdict)
from orc import Oracle
from passfuzz import KNOB_NAMES, KNOBS, knob_label, record_width
from phfpfac_amd import GpuMatcher, PfacTable
from phfpfac_amd.dist import packed_to_records
from phfpfac_amd.matcher import splitmix64_bytes, tiled_bytes

pytestmark = pytest.mark.gpu

PAD = 2 * TILE                           # bytes owned behind every input (the scan's tile loads are the caller's to cover)
SPARSE_LINES = [b"\x00\x01", b"\x10\x7f", b"ab", b"\xff\xfe", b"zz\x00", b"\x80\x80", b"Qq", b"\x33\x44\x55", b"\xaa\xbb",
                b"\x01\x02\x03\x04", b"\xee\x11", b"\x7f\x7f", b"~\x00", b"\xc3\xa9"]
# name -> (pattern file, input kind, knobs added to every knob set, whether the sweep must meet a dense AND a sparse staging layout)
WORKLOADS = {
    "exp-text": ("experimentpattern", "text", {}, True),                 # 2-byte records, dense
    "dict-text": ("xaa+xab+xac+xad", "text", {}, True),                  # 4-byte records, dense (FORCE_L2 + DENSE: second dense form)
    "sparse": (None, "random", {}, False),                               # 2-byte records, most tiles hold 0 or 1: padding dominates
    "snort-random": ("bytefile/1000000byte", "random", {}, False),       # 4-byte records, sparse, tables via L2
    # 8-byte records go straight to the heap: the library has no dense staging for them and pfac_scan_staging never
    # reports one, so the "both layouts" claim does not apply
    "exp-text-wide": ("experimentpattern", "text", {"PFAC_WIDE": "1"}, False),
}
LARGEST = (16 << 20) + 3 * TILE + 17
RICH = 96 * TILE + 333                   # the last size: for the text workloads of experimentpattern an 'a'-rich input (below)
SIZES = [TILE, 63 * TILE, 64 * TILE, 64 * TILE + 777, (3 << 20) + 1235, LARGEST, RICH]
PINNING = ("PFAC_DENSE", "PFAC_LAG")     # knobs that pin the staging layout: such contexts never adapt it
_CACHE = {}


def set_knobs(monkeypatch, knobs):
    for k in KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


class Workload:
    """A pattern file with its host table, its CPU matcher's records per input size, and its inputs."""

    def __init__(self, name, resolve, tmp):
        pat, self.kind, self.env, self.dense = WORKLOADS[name]
        self.name = name
        if pat is None:
            self.path = os.path.join(tmp, "sparse.pat")
            with open(self.path, "wb") as f:
                f.write(b"".join(p + b"\n" for p in SPARSE_LINES))
        else:
            self.path = resolve(pat)
        self.table = PfacTable.from_file(self.path, 256)
        self.para = open(resolve("paragraph402"), "rb").read()
        self._want, self._data = {}, {}

    def data(self, n):
        if n not in self._data:
            if n == RICH and self.kind == "text" and self.path.endswith("experimentpattern"):
                # a, aa, aaa, aaaa on the paragraph leave about 300 records per tile, inside the sparse staging; with
                # 30 % of the bytes 'a' a tile holds some 1 700 and an unpinned context goes dense after its first scan
                rng = np.random.default_rng(RICH)
                self._data[n] = np.where(rng.random(n) < 0.3, ord("a"), ord("b")).astype(np.uint8)
            else:
                self._data[n] = tiled_bytes(n, self.para) if self.kind == "text" else splitmix64_bytes(n, 0x48454150)
        return self._data[n]

    def want(self, n):
        if n not in self._want:                                 # (one oracle build for all sizes)
            o = Oracle(self.path, 1, 1)
            for k in SIZES:
                self._want[k] = oracle_want(o, self.data(k), k, k)
            o.close()
        return self._want[n]

    def device_input(self, n):
        """The input in a tensor of its own with PAD more bytes of the same kind of text behind it."""
        import torch
        more = tiled_bytes(PAD, self.para, n) if self.kind == "text" else splitmix64_bytes(n + PAD, 0x48454150)[n:]
        if n == RICH and self.kind == "text":
            more = np.full(PAD, ord("a"), np.uint8)
        return torch.from_numpy(np.concatenate([self.data(n), more])).to("cuda:0")


def workload(name, resolve, tmp_path_factory):
    key = "exp-text" if name == "exp-text-wide" else name       # (the same file and inputs: one oracle run)
    if key not in _CACHE:
        _CACHE[key] = Workload(key, resolve, str(tmp_path_factory.mktemp("heap")))
    w = _CACHE[key]
    if name != key:
        wide = Workload.__new__(Workload)
        wide.__dict__.update(w.__dict__)
        wide.name, wide.env, wide.dense = name, WORKLOADS[name][2], WORKLOADS[name][3]
        return wide
    return w


def workload_env(knobs, w):
    """The knob set with the workload's own knobs on top.  A workload that pins the record width (PFAC_WIDE) drops the
    knob set's PFAC_REC_BYTES, which the library would honour in its place: that knob set then runs as the default
    variant with 8-byte records."""
    env = {**knobs, **w.env}
    if "PFAC_WIDE" in w.env:
        env.pop("PFAC_REC_BYTES", None)
    return env


# ---------------------------------------------------------------------------
# a. the capacity ladder under every kernel variant

@pytest.mark.parametrize("name", list(WORKLOADS))
def test_capacity_ladder_under_every_kernel_variant(name, resolve, tmp_path_factory, monkeypatch):
    """Every knob set x every input size (one tile; 63, 64, 65 tiles; a ragged 3 MiB; 16 MiB; 97 dense tiles): one context walks
    capacity_ladder upwards with one fill and downwards with the other, a fresh GuardedBuffer of exactly the capacity
    each time, and `verdict` holds for every scan (count exact, over == used > capacity, overflow below the count,
    none at or above any earlier hint, records / layout / checksum when it fits, PFAC_E_OVERFLOW from the consumers
    when not, guards whole).  The 16 MiB size also gets one very generous capacity.  The sweep must have met, at one
    size, a scan that used exactly its runs' allocations and one that used more (chunked placement).  For the dense
    workloads, one ladder -- one size in one context whose knob set pins neither PFAC_DENSE nor PFAC_LAG, so that only
    pfac_scan_finish's adaptation can change the layout -- must have run scans with a sparse AND with the dense staging
    layout: capacities, hints and paddings of one layout are then consumed under the other.  Contexts with a pinned
    layout do not count towards that."""
    w = workload(name, resolve, tmp_path_factory)
    t0 = time.time()
    placements, layouts, scans = {n: set() for n in SIZES}, {}, 0
    for knobs in KNOBS:
        env = workload_env(knobs, w)
        set_knobs(monkeypatch, env)
        rb = record_width(w.table.num_final, env)
        with GpuMatcher(0, 1) as g:
            g.load_table(w.table)
            for n in SIZES:
                want, d_in, hints = w.want(n), w.device_input(n), []
                where = f"{name} [{knob_label(env)}] n {n}"
                first = verdict(g, w.table, want, d_in, n, n, 0, rb, FILLS[0], hints, where)
                placements[n].add("exact" if first["used"] == first["P"] else "chunked")
                ladder = capacity_ladder(want.n, want.padded(rb), first["hint"])
                mine = layouts.setdefault((knob_label(env), n), set()) if not set(env) & set(PINNING) else set()
                mine.add("dense" if first["staging"][0] == 1 else "sparse")
                if n == LARGEST:
                    # one rung far above 4 x hint, so that the large input too can meet a placement with used > P.  (How
                    # far is read off the library's chunk rule; nothing is asserted from it: placements are told apart
                    # by the observed used and P alone.)
                    ladder.append(max(ladder[-1] + 8, 33 * 1024 * g.info()["grid_blocks"] + 5))
                for fill, caps in ((FILLS[0], ladder), (FILLS[1], ladder[::-1])):
                    for cap in caps:
                        r = verdict(g, w.table, want, d_in, n, n, cap, rb, fill, hints, where)
                        placements[n].add("exact" if r["used"] == r["P"] else "chunked")
                        mine.add("dense" if r["staging"][0] == 1 else "sparse")
                        scans += 1
                del d_in
    print(f"{name}: {scans} scans in {time.time() - t0:.0f} s; placements per size "
          f"{ {n: sorted(p) for n, p in placements.items()} }; unpinned ladders that ran both staging layouts: "
          f"{sorted(k for k, v in layouts.items() if len(v) == 2)}")
    assert any(p == {"exact", "chunked"} for p in placements.values()), f"{name}: no size met both placements: {placements}"
    if w.dense:
        assert any(v == {"dense", "sparse"} for v in layouts.values()), \
            f"{name}: no ladder of an unpinned context ran both a sparse and the dense staging layout: {layouts}"


# ---------------------------------------------------------------------------
# b. the hint is enough, in one retry

@pytest.mark.parametrize("name", list(WORKLOADS))
def test_hint_fits_in_one_retry(name, resolve, tmp_path_factory, monkeypatch):
    """Under every knob set: a scan with capacity 0 (a non-NULL heap whose guard starts at the pointer itself), 1 and
    half the match count, each followed by ONE rescan into a GuardedBuffer of exactly pfac_scan_capacity_hint()
    records, through scan_async / scan_finish themselves (no retry loop in between): it must fit, records exact."""
    w = workload(name, resolve, tmp_path_factory)
    for knobs in KNOBS:
        env = workload_env(knobs, w)
        set_knobs(monkeypatch, env)
        rb = record_width(w.table.num_final, env)
        for fill in FILLS:
            with GpuMatcher(0, 1) as g:
                g.load_table(w.table)
                for n in (SIZES[3], SIZES[4]):
                    want, d_in = w.want(n), w.device_input(n)
                    for cap in (0, 1, want.n // 2):
                        where = f"{name} [{knob_label(env)}] n {n} after capacity {cap}"
                        r = verdict(g, w.table, want, d_in, n, n, cap, rb, fill, [], where)
                        assert r["over"] or want.n == 0, where
                        again = verdict(g, w.table, want, d_in, n, n, r["hint"], rb, fill, [r["hint"]], where + ": retry at the hint")
                        assert not again["over"]


FLIPS = [("abc", 0.3, 0.02), ("abc", 0.02, 0.3), ("abc", 0.02, 0.08), ("abc", 0.08, 0.02), ("abc", 0.3, 0.08),
         ("dict", "random", "text"), ("dict", "text", "random")]


def density_input(rng, n, density):
    u = rng.random(n)
    return np.where(u < density, ord("a"), np.where(u < density + 0.3, ord("b"), ord("c"))).astype(np.uint8)


@pytest.mark.parametrize("which,before,density", FLIPS, ids=[f"{w}-{a}-then-{b}" for w, a, b in FLIPS])
def test_hint_fits_after_the_staging_mode_flips(which, before, density, tmp_path, resolve):
    """pfac_scan_finish adapts the staging layout after an overflowed scan too, so the retry the hint was made for runs
    with another layout than the scan that made it.  "abc": the patterns and densities of
    test_staging_layout_follows_the_match_density (2-byte records; three, two and one staging buffers).  "dict": the
    10 400 patterns of xaa .. xad (4-byte records, tables via L2) on random bytes (a handful of records per tile) and on
    the paragraph (some 1 700 per tile: the dense layout, in its second form where the library has it).  Two scans of
    the input of the other density set the layout, the overflowed scan of this one flips it (asserted through
    pfac_scan_staging), and the one retry at its hint must still fit -- for capacities 0, 1 and half the count, each
    with both fills.  Default knobs: every other knob set pins a layout or runs this same adaptation."""
    import torch
    n = 3 * 1024 * 1024 + 77
    if which == "abc":
        path = str(tmp_path / "p")
        with open(path, "wb") as f:
            f.write(b"a\nab\nabc\n")
        rng = np.random.default_rng(17)
        other, data = density_input(rng, n, before), density_input(rng, n, density)
    else:
        path = resolve("xaa+xab+xac+xad")
        kinds = {"random": splitmix64_bytes(n, 0x464C4950), "text": tiled_bytes(n, open(resolve("paragraph402"), "rb").read())}
        other, data = kinds[before], kinds[density]
    table = PfacTable.from_file(path, 256)
    rb = record_width(table.num_final, {})
    o = Oracle(path, 1, 1)
    want, want_other = oracle_want(o, data, n, n), oracle_want(o, other, n, n)
    o.close()
    d_in = torch.from_numpy(np.concatenate([data, np.full(PAD, ord("a"), np.uint8)])).to("cuda:0")
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        for cap in (0, 1, want.n // 2):
            for fill in FILLS:
                for _ in range(2):
                    rec = g.scan_bytes(other)
                    assert rec.size == want_other.n
                mode_before = staging_of(g)
                where = f"{which}: {before} then {density}, capacity {cap}"
                r = verdict(g, table, want, d_in, n, n, cap, rb, fill, [], where)
                assert r["over"] and r["staging"] == mode_before
                mode_after = staging_of(g)
                assert mode_after[0] != mode_before[0], f"{where}: the staging layout did not change ({mode_before} -> {mode_after})"
                again = verdict(g, table, want, d_in, n, n, r["hint"], rb, fill, [r["hint"]], where + ": retry at the hint")
                assert not again["over"] and again["staging"] == mode_after
                print(f"{where}: {mode_before} -> {mode_after}; used {r['used']} -> {again['used']}, P {again['P']}, hint {r['hint']}")


# ---------------------------------------------------------------------------
# c. the read side: nothing past n_avail shows

def read_cases(tmp):
    """Every ReadCase with its table source and its two expectations (once per session)."""
    if "read" not in _CACHE:
        out, paths = [], {}
        for seed in READ_SEEDS:
            c = ReadCase(seed)
            path = os.path.join(tmp, f"read_{seed}.pat")
            m = read_case_matcher(c, path)
            bounded, unbounded = c.expectations(m)
            m.close()
            c.check_poison(bounded, unbounded)                  # else the case proves nothing
            path = paths.setdefault(c.kind, path)               # (one image per kind: one table)
            out.append((c, path, bounded))
        _CACHE["read"] = out
    return _CACHE["read"]


@pytest.mark.parametrize("knobs", KNOBS, ids=[knob_label(k) for k in KNOBS])
def test_nothing_past_n_avail_shows(knobs, tmp_path_factory, monkeypatch):
    """One device buffer of match-rich text; every scan reads a window d_input = base + 16 k of it, with text in front
    of the pointer and, behind n_avail, the bytes that complete a copy of the longest pattern started on the last
    owned byte (checked on the CPU: with them the oracle reports more).  n_owned around 1, 16, one tile and several
    tiles; n_avail - n_owned of 0, 1, halo - 1, halo, halo + 1; short patterns, 1022-byte patterns across the n_avail
    and a tile edge, a character-class table.  Expected: the oracle's matches of data[:n_avail] that start below
    n_owned.  The heap is a GuardedBuffer of exactly the padded placement, so the scan must also fit it."""
    import torch
    cases = read_cases(str(tmp_path_factory.mktemp("read")))
    set_knobs(monkeypatch, knobs)
    buf = torch.full((READ_BUF + PAD,), ord("a"), dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    with GpuMatcher(0, 1) as g:
        loaded = None
        for c, path, want in sorted(cases, key=lambda x: x[1]):
            if ("table", path) not in _CACHE:
                _CACHE["table", path] = PfacTable.from_charclass(path, 256) if c.kind == "class" else PfacTable.from_file(path, 256)
            table = _CACHE["table", path]
            if loaded != path:
                g.load_table(table)
                loaded = path
            assert table.max_pat_len == c.M and table.halo == c.halo
            buf[:READ_BUF].copy_(torch.from_numpy(c.data))
            rb = record_width(table.num_final, knobs)
            for fill in FILLS:
                r = verdict(g, table, want, buf.data_ptr() + c.off, c.n_owned, c.n_avail, want.padded(rb), rb, fill, [],
                            f"{c.describe()} [{knob_label(knobs)}]")
                assert not r["over"], c.describe()


# ---------------------------------------------------------------------------
# d. fetch windows into guarded buffers

def windows(want, rng):
    cum = np.cumsum(want.tile_counts)
    n = want.n
    w = [(0, min(n, 1000)), (0, n), (int(cum[5] - want.tile_counts[5] // 2), 700), (n - 333, 333), (0, 1), (n - 1, 1),
         (int(cum[40]) + 3, 1), (int(cum[63]) - 10, 25), (int(cum[127]) - 3, 9), (int(cum[127]), 4000),
         (int(cum[69]) - 5, 12), (int(cum[69]), 1)]
    for _ in range(32):
        first = int(rng.integers(0, n))
        w.append((first, int(rng.integers(1, min(n - first, 5000) + 1))))
    assert all(0 <= f and k >= 1 and f + k <= n for f, k in w)
    return w


@pytest.mark.parametrize("fill", FILLS, ids=[f"fill-{f:02x}" for f in FILLS])
@pytest.mark.parametrize("pat,env,rb", [("experimentpattern", {}, 2), ("xaa+xab+xac+xad", {}, 4),
                                        ("experimentpattern", {"PFAC_WIDE": "1"}, 8)], ids=["2-byte", "4-byte", "8-byte"])
def test_fetch_windows_into_guarded_buffers(pat, env, rb, fill, resolve, monkeypatch):
    """After one scan that fits its heap exactly: pfac_records_expand of windows [first, first + n) into a
    GuardedBuffer of exactly n x 8 bytes, and pfac_records_d2h of the same windows -- from 0, from the middle of a
    tile's run, up to the last record, single records, across a boundary between groups of 64 tiles, across a stretch
    of empty tiles, 32 random ones -- each equal to the same slice of the oracle's list; pfac_records_packed_device
    into guarded buffers of exactly used x record size and n_tiles x 8 bytes; a window one past the count is
    PFAC_E_ARG and leaves its buffer as it was."""
    import torch
    set_knobs(monkeypatch, env)
    para = open(resolve("paragraph402"), "rb").read()
    n_in = 200 * TILE - 123
    data = tiled_bytes(n_in, para).copy()
    data[70 * TILE:78 * TILE] = 0                               # tiles 70 .. 77 hold no record
    o = Oracle(resolve(pat), 1, 1)
    want = oracle_want(o, data, n_in, n_in)
    o.close()
    assert want.tile_counts[70:78].sum() == 0 and want.tile_counts[69] > 5 and want.tile_counts[78] > 5
    table = PfacTable.from_file(resolve(pat), 256)
    d_in = torch.from_numpy(np.concatenate([data, np.zeros(PAD, np.uint8)])).to("cuda:0")
    ids = lambda rec: table.idmap[rec["state"]]
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        cap = want.padded(rb)
        heap = GuardedBuffer(cap * rb, fill=fill)
        g.scan_async(n_in, n_in, d_input=d_in, d_records=heap.ptr, capacity=cap)
        n, over = g.scan_finish(0, allow_overflow=True)
        assert (n, over) == (want.n, False) and g.scan_format(0) == (rb, want.n_tiles, cap)
        for first, k in windows(want, np.random.default_rng(rb)):
            out = GuardedBuffer(k * 8, fill=fill)
            g.expand_records(k, out.ptr, d_records=heap.ptr, first=first)
            g.sync(0)
            rec = out.host().view([("pos", "<u4"), ("state", "<u4")])
            assert np.array_equal(rec["pos"].astype(np.int64), want.pos[first:first + k]), f"expand [{first}, +{k}): positions"
            assert np.array_equal(ids(rec), want.ids[first:first + k]), f"expand [{first}, +{k}): pattern ids"
            out.check(what=f"the expand output of window [{first}, +{k})")
            rec = g.records_to_host(k, d_records=heap.ptr, first=first)
            assert np.array_equal(rec["pos"].astype(np.int64), want.pos[first:first + k]), f"d2h [{first}, +{k}): positions"
            assert np.array_equal(ids(rec), want.ids[first:first + k]), f"d2h [{first}, +{k}): pattern ids"
        # one past the count
        out = GuardedBuffer(16 * 8, fill=fill)
        host = np.zeros(16, dtype=rec.dtype)
        assert g._L.pfac_records_expand(g._ctx, 0, heap.ptr, want.n - 15, 16, out.ptr) == E_ARG
        assert g._L.pfac_records_d2h(g._ctx, 0, heap.ptr, host.ctypes.data, want.n - 15, 16) == E_ARG
        g.sync(0)
        out.check(payload_untouched=True, what="the output of a window one past the count")
        assert not host.view(np.uint8).any()
        # the compact form itself
        words, tix = GuardedBuffer(cap * rb, fill=fill), GuardedBuffer(want.n_tiles * 8, fill=fill)
        rc = g._L.pfac_records_packed_device(g._ctx, 0, heap.ptr, words.ptr, cap, tix.ptr)
        g.sync(0)
        if rb == 8:
            assert rc == E_STATE
            words.check(payload_untouched=True), tix.check(payload_untouched=True)
        else:
            assert rc == 0
            got = packed_to_records(words.host(), tix.host().view(np.uint64), rb)
            assert np.array_equal(got["pos"].astype(np.int64), want.pos) and np.array_equal(ids(got), want.ids)
            words.check(what="the packed words"), tix.check(what="the packed tile index")
        heap.check(what="the record heap")
