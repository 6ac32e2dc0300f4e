"""Counts per pattern on the GPU (run with -m gpu on an MI355X): pfac_records_count_states and
pfac_selection_count_states histogram the final states of a scan / a leftmost-longest selection on the device, and
PfacTable.counts_by_pattern turns them into counts by pattern id.  The checker is never the device's own output: numpy's
bincount over the CPU oracle's records (through tests/wordref.py / tests/llref.py where a filter or a selection sits in
between, tests/bigref.py for the large automaton), and the committed reference outputs.  Integer work: bit-exact."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import bigsets
import countref
import wordref
from bigref import BigRef
from docref import random_offsets
from heapguard import GuardedBuffer
from llref import greedy, line_lengths
from orc import Oracle, match_checksum
from phfpfac_amd import GpuMatcher, PfacError, PfacTable, _ffi
from phfpfac_amd.matcher import tiled_bytes
from test_gpu_whole_words import VARIANTS
from test_pattern_counts_ref import CHAIN_FORMS, CHAIN_N, CUT_LISTS, _chain_whole, chain_cuts, chain_parts, chain_reference

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FP = json.load(open(os.path.join(HERE, "golden", "fingerprints.json")))
TILE = 4096
N = 65536 + 123                         # 17 tiles, the last one ragged
N_BIG = (1 << 20) + 123                 # 257 tiles
E_ARG, E_STATE, E_OVERFLOW = _ffi.PFAC_E_ARG, _ffi.PFAC_E_STATE, _ffi.PFAC_E_OVERFLOW
BINS_MUL = 0x9E3779B1                   # count_slot_of (pfac_hip.hip): slot = ((state * BINS_MUL mod 2^32) * bins) >> 32


@functools.lru_cache(maxsize=None)
def _para(path, n):
    buf = tiled_bytes(n, open(path, "rb").read())
    buf.setflags(write=False)
    return buf


def para_bytes(resolve, n):
    return _para(resolve("paragraph402"), n)


@functools.lru_cache(maxsize=None)
def _oracle(path, para_path, n):
    """(pos, ids, lens) of the CPU oracle over n bytes of the tiled paragraph: computed once, shared, read-only."""
    o = Oracle(path, 1, 1)
    pos, ids = o.scan_spec(np.ascontiguousarray(_para(para_path, n)))
    o.close()
    lens = line_lengths(path)[ids]
    for a in (pos, ids, lens):
        a.setflags(write=False)
    return pos, ids, lens


def oracle_records(resolve, pat, n):
    return _oracle(resolve(pat), resolve("paragraph402"), n)


def scan(g, buf, n_owned=None):
    n_owned = buf.size if n_owned is None else n_owned
    g.reserve(0, max(buf.size, 1), max(buf.size // 8, 4096))
    if buf.size:
        g.h2d(buf)
    return g.scan_resident(n_owned, buf.size)


def status_of(fn):
    with pytest.raises(PfacError) as e:
        fn()
    return e.value.status


def guarded_counts(table, fill=0xA5):
    return GuardedBuffer(int(table.num_final) * 8, fill=fill)


def counts_of(guard):
    return guard.host().view(np.uint64).copy()


def raw_count(g, d_counts=0, n_states=None, flags=0, d_records=0, selection=False):
    """The C call itself: (status, n_counted)."""
    n = C.c_uint64(0)
    n_states = g.table.num_final if n_states is None else n_states
    fn = g._L.pfac_selection_count_states if selection else g._L.pfac_records_count_states
    return fn(g._ctx, 0, d_records, d_counts, n_states, flags, C.byref(n)), n.value


def count_both_ways(g, table, want, n, what=""):
    """The slot-owned buffer and a guarded caller's buffer of exactly num_final x 8 bytes."""
    guard = guarded_counts(table)
    assert g.count_states(d_counts=guard.ptr) == n, what
    g.sync()
    guard.check(what="the caller's d_counts " + what)
    np.testing.assert_array_equal(counts_of(guard), want, err_msg=what)
    assert g.count_states() == n == g.last_count(), what
    own = g.state_counts_to_host()
    np.testing.assert_array_equal(own, want, err_msg=what)
    assert int(own.sum()) == n
    return guard


# ---------------------------------------------------------------------------
# every record form and scan variant

SHAPES = {"experimentpattern": (4900, 1, 4), "xaa+xab+xac+xad": (27596, 91, 7989), "xaa": (6859, 26, None)}


@pytest.mark.parametrize("pat,env,width", VARIANTS, ids=[f"{p}-{'+'.join(e) or 'default'}" for p, e, _ in VARIANTS])
def test_counts_of_every_record_form(pat, env, width, resolve, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    buf = para_bytes(resolve, N)
    pos, ids, _ = oracle_records(resolve, pat, N)
    table = PfacTable.from_file(resolve(pat), 256)
    want = countref.state_counts(table, ids)
    matches, hit, num_final = SHAPES[pat]
    assert pos.size == matches and int((want > 0).sum()) == hit                 # the shapes the issue names
    assert num_final is None or table.num_final == num_final
    if pat == "experimentpattern":
        assert want.max() == matches                                            # ONE hot state: every add of a chunk collides
    if pat == "xaa+xab+xac+xad":
        assert np.bincount(pos // TILE).max() == 1731                           # many chunks of 64 per tile
        assert 0.13 < want.max() / matches < 0.15
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.scan_bytes(buf)                                       # (a first scan, so that the adapted staging is what runs)
        assert scan(g, buf) == pos.size
        assert g.scan_format()[0] == width
        rec = g.records_to_host(pos.size)
        chk = g.checksum(pos.size)
        assert chk == match_checksum(pos, ids)
        count_both_ways(g, table, want, pos.size, pat)
        np.testing.assert_array_equal(table.counts_by_pattern(g.state_counts_to_host()), countref.pattern_counts(ids, table.n_patterns))
        # read-only: the scan is what it was
        assert g.scan_finish()[0] == pos.size
        assert np.array_equal(g.records_to_host(pos.size), rec) and g.checksum(pos.size) == chk


# ---------------------------------------------------------------------------
# the committed reference outputs

@pytest.mark.parametrize("case,lines", [("exp_x_expinput_s1_w256", 47), ("b10000_x_b1000000_s1_w256", 1999)])
def test_reference_outputs(case, lines, resolve):
    c = FP["cases"][case]
    table = PfacTable.from_file(resolve(c["pattern"]), c["width"])
    want, n = countref.parse_counts(open(os.path.join(HERE, "golden", "out", case + ".txt"), "rb").read(), table.n_patterns)
    assert n == lines == c["lines"]
    data = open(resolve(c["input"]), "rb").read()[:-1]          # the reference drops the last byte (main.cc:138)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        got = g.count_patterns(data)
    assert got.dtype == np.uint64
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------------------
# the cache regime and the grid-stride loop

@pytest.mark.parametrize("env,n", [({"PFAC_COUNT_BINS": "64"}, N), ({"PFAC_COUNT_GRID": "2"}, N_BIG),
                                   ({"PFAC_COUNT_BINS": "64", "PFAC_COUNT_GRID": "2"}, N_BIG),
                                   ({"PFAC_COUNT_BINS": "1"}, N)],
                         ids=["bins64", "grid2", "bins64+grid2", "bins1"])
def test_small_cache_and_small_grid(env, n, resolve, monkeypatch):
    """7989 final states behind 64 (or 1) cache slots: the 91 states that occur collide, the losers add to memory at
    once; 2 workgroups over 257 tiles: every wave walks 32 tiles or more."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pat = "xaa+xab+xac+xad"
    buf = para_bytes(resolve, n)
    pos, ids, _ = oracle_records(resolve, pat, n)
    table = PfacTable.from_file(resolve(pat), 256)
    want = countref.state_counts(table, ids)
    bins = int(env.get("PFAC_COUNT_BINS", 0))
    if bins:
        assert table.num_final > bins
        slots = ((np.flatnonzero(want).astype(np.uint64) * np.uint64(BINS_MUL) & np.uint64(0xFFFFFFFF)) * np.uint64(bins)) >> np.uint64(32)
        assert np.unique(slots).size < np.flatnonzero(want).size                # states that occur do share slots
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        assert scan(g, buf) == pos.size
        assert g.scan_format()[1] == -(-n // TILE)
        count_both_ways(g, table, want, pos.size, str(env))


def test_two_hot_states_share_a_cache_slot(tmp_path, monkeypatch):
    """200 patterns behind 64 slots; the text is made of two words whose states hash to ONE slot (the one seen first
    claims it, the other one's adds all go to memory) and a sprinkling of the others."""
    monkeypatch.setenv("PFAC_COUNT_BINS", "64")
    lines = [b"w%03dq" % k for k in range(200)]
    pf = tmp_path / "w.pat"
    pf.write_bytes(b"".join(p + b"\n" for p in lines))
    table = PfacTable.from_file(str(pf), 256)
    st = countref.state_of_id(table)
    slot = ((st[1:].astype(np.uint64) * np.uint64(BINS_MUL) & np.uint64(0xFFFFFFFF)) * np.uint64(64)) >> np.uint64(32)
    by_slot = {}
    for i, s in enumerate(slot.tolist()):
        by_slot.setdefault(s, []).append(i)
    a, b = next(v for v in by_slot.values() if len(v) >= 2)[:2]
    rng = np.random.default_rng(3)
    pick = np.where(rng.random(14000) < 0.9, np.where(rng.random(14000) < 0.5, a, b), rng.integers(0, 200, 14000))
    buf = np.frombuffer(b" ".join(lines[i] for i in pick.tolist()), dtype=np.uint8)
    assert buf.size > 16 * TILE
    o = Oracle(str(pf), 1, 1)
    pos, ids = o.scan_spec(np.ascontiguousarray(buf))
    o.close()
    want = countref.state_counts(table, ids)
    hot = np.argsort(want)[-2:]
    assert slot[table.idmap[hot[0]] - 1] == slot[table.idmap[hot[1]] - 1] and want[hot].min() > 5000
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        assert scan(g, buf) == pos.size == 14000
        count_both_ways(g, table, want, pos.size)


def test_more_final_states_than_the_default_table():
    """65 535 final states, 18 980 of them hit: the cache regime without any knob, its 16 384 slots oversubscribed."""
    s = bigsets.final_set(65535)
    table = PfacTable.from_bytes(s.image(), 256)
    assert table.num_final == 65535 > 8192
    buf = bigsets.word_text(s, N)
    pos, ids = BigRef(s.image()).scan_spec(buf)
    want = countref.state_counts(table, ids)
    assert int((want > 0).sum()) > 16384                         # more states than the cache has slots
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        assert scan(g, buf) == pos.size
        count_both_ways(g, table, want, pos.size)


# ---------------------------------------------------------------------------
# after the whole-word filter

def test_counts_follow_the_whole_word_filter(resolve):
    pat = "xaa+xab+xac+xad"
    buf = para_bytes(resolve, N)
    pos, ids, lens = oracle_records(resolve, pat, N)
    keep = wordref.filter_words(buf, pos, lens)
    assert 0 < keep.sum() < pos.size
    table = PfacTable.from_file(resolve(pat), 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        scan(g, buf)
        count_both_ways(g, table, countref.state_counts(table, ids), pos.size, "before the filter")
        kept = g.filter_whole_words()
        assert kept == int(keep.sum())
        count_both_ways(g, table, countref.state_counts(table, ids[keep]), kept, "after the filter")
        np.testing.assert_array_equal(g.count_patterns(buf, whole_words=True), countref.pattern_counts(ids[keep], table.n_patterns))


# ---------------------------------------------------------------------------
# accumulate

def test_accumulated_ranges_equal_one_scan(resolve):
    pat = "xaa+xab+xac+xad"
    buf = para_bytes(resolve, N)
    pos, ids, lens = oracle_records(resolve, pat, N)
    table = PfacTable.from_file(resolve(pat), 256)
    want = countref.state_counts(table, ids)
    cut = int(pos[np.flatnonzero((lens > 2) & (pos > 7 * TILE))[0]]) + 2        # inside a match: it ends in the first range's halo
    first, second = pos < cut, pos >= cut
    assert (pos[first] + lens[first] > cut).any() and cut % TILE
    parts = [(np.ascontiguousarray(buf[:cut + table.halo]), cut), (np.ascontiguousarray(buf[cut:]), N - cut)]
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        # the slot-owned buffer, through the one-call form
        np.testing.assert_array_equal(g.count_patterns(parts[0][0], parts[0][1]), countref.pattern_counts(ids[first], table.n_patterns))
        np.testing.assert_array_equal(g.count_patterns(parts[1][0], parts[1][1], accumulate=True),
                                      countref.pattern_counts(ids, table.n_patterns))
        # without the flag the second call replaces the first
        np.testing.assert_array_equal(g.count_patterns(parts[1][0], parts[1][1]), countref.pattern_counts(ids[second], table.n_patterns))
        # a caller's buffer: accumulate adds onto whatever is there
        guard = guarded_counts(table)
        for k, (part, n_owned) in enumerate(parts):
            scan(g, part, n_owned)
            assert g.count_states(d_counts=guard.ptr, accumulate=k > 0) == int((first if k == 0 else second).sum())
        g.sync()
        guard.check(what="the caller's d_counts")
        np.testing.assert_array_equal(counts_of(guard), want)
        assert g.count_states(d_counts=guard.ptr) == int(second.sum())
        np.testing.assert_array_equal(counts_of(guard), countref.state_counts(table, ids[second]))
        np.testing.assert_array_equal(g.state_counts_to_host(), countref.state_counts(table, ids[second]))   # (the slot's own: untouched)
        # accumulate from nothing starts from zero
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        scan(g, parts[0][0], parts[0][1])
        g.count_states(accumulate=True)
        np.testing.assert_array_equal(g.state_counts_to_host(), countref.state_counts(table, ids[first]))
        # ... and across a table upload the slot's counts cannot be added to
        before = g.state_counts_to_host()
        g.load_table(table)
        scan(g, parts[1][0], parts[1][1])
        assert status_of(lambda: g.count_states(accumulate=True)) == E_STATE
        np.testing.assert_array_equal(g.state_counts_to_host(), before)
        g.count_states()
        np.testing.assert_array_equal(g.state_counts_to_host(), countref.state_counts(table, ids[second]))


@pytest.mark.parametrize("name", CUT_LISTS)
@pytest.mark.parametrize("form", range(len(CHAIN_FORMS)), ids=[f[0] for f in CHAIN_FORMS])
def test_chained_and_chunked_counts_equal_one_scan(form, name, resolve, monkeypatch):
    """The header's promise: counts accumulated over chained ranges "are the counts of one scan of the whole" -- for
    2-, 4- and 8-byte records, seeded random cuts into 2, 5 and 17 ranges and the fixed list of shapes where chaining goes
    wrong (test_pattern_counts_ref.chain_cuts), and for four accumulations, each into the slot-owned buffer and into a
    guarded caller's buffer: the scan's counts, the counts after the whole-word filter (prev_byte / next_byte from the
    neighbours), and the selection's counts without and with the filter (entry chained from the previous exit).  Every
    step's n_counted is the reference's count for that range; the sums are the histograms of ONE oracle scan of the
    whole through wordref.filter_words and llref.greedy (the CPU twin in test_pattern_counts_ref.py shows the parts'
    references sum to them for these very cuts)."""
    pat, env, width = CHAIN_FORMS[form]
    assert (pat, env, width) in VARIANTS and CHAIN_N == N
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    path, para = resolve(pat), resolve("paragraph402")
    table = PfacTable.from_file(path, 256)
    buf, pos, _, lens, M = _chain_whole(path, para)
    ref = chain_reference(path, para, name, form)
    parts = chain_parts(buf, chain_cuts(name, form, buf, pos, lens, M), M)
    assert M == table.max_pat_len and len(parts) == len(ref["ranges"])
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        for what in ("plain", "kept", "sel", "fsel"):
            guard = guarded_counts(table, fill=0x3C)
            entry = 0
            for k, ((a, b, part, prev, nxt), r) in enumerate(zip(parts, ref["ranges"])):
                tag = f"{pat} {name} {what}: range {k} [{a}, {b})"
                assert scan(g, part, b - a) == r["plain"].size, tag
                if k == 0:
                    assert g.scan_format()[0] == width
                if what in ("kept", "fsel"):
                    assert g.filter_whole_words(prev_byte=prev, next_byte=nxt) == r["kept"].size, tag
                if what in ("sel", "fsel"):
                    assert entry == r["entry" if what == "sel" else "fentry"], tag
                    n_sel, entry = g.select_leftmost_longest(entry)
                    assert n_sel == r[what].size, tag
                count = g.count_selection_states if what in ("sel", "fsel") else g.count_states
                assert count(accumulate=k > 0) == r[what].size, tag
                assert count(d_counts=guard.ptr, accumulate=k > 0) == r[what].size, tag
            g.sync()
            guard.check(what=f"the caller's d_counts ({pat} {name} {what})")
            want = countref.state_counts(table, ref["whole"][what])
            np.testing.assert_array_equal(g.state_counts_to_host(), want, err_msg=f"{pat} {name} {what}: the slot's counts")
            np.testing.assert_array_equal(counts_of(guard), want, err_msg=f"{pat} {name} {what}: the caller's counts")
            assert int(want.sum()) == ref["whole"][what].size > 0


# ---------------------------------------------------------------------------
# the selection form

def test_selection_counts(resolve):
    import torch
    pat = "xaa"
    path = resolve(pat)
    buf = para_bytes(resolve, N)
    pos, ids, lens = oracle_records(resolve, pat, N)
    table = PfacTable.from_file(path, 256)
    pick, _ = greedy(pos, lens, 0, N)
    want = countref.state_counts(table, ids[pick])
    assert 0 < pick.size < pos.size
    off = random_offsets(np.random.default_rng(5), N, 40, empties=3)
    dpick = []
    for a, b in zip(off[:-1].astype(np.int64).tolist(), off[1:].astype(np.int64).tolist()):
        m = np.flatnonzero((pos >= a) & (pos < b) & (pos + lens <= b))
        dpick.append(m[greedy(pos[m] - a, lens[m], 0, b - a)[0]])
    dpick = np.concatenate(dpick)
    dwant = countref.state_counts(table, ids[dpick])
    assert not np.array_equal(dwant, want)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        scan(g, buf)
        assert status_of(g.count_selection_states) == E_STATE                   # no selection yet
        n_sel, _ = g.select_leftmost_longest(0)
        assert n_sel == pick.size
        sel = g.selection_to_host(n_sel)
        guard = guarded_counts(table)
        assert g.count_selection_states(d_counts=guard.ptr) == n_sel
        g.sync()
        guard.check(what="d_counts of the selection")
        np.testing.assert_array_equal(counts_of(guard), want)
        assert g.count_selection_states() == n_sel
        np.testing.assert_array_equal(g.state_counts_to_host(), want)
        assert np.array_equal(g.selection_to_host(n_sel), sel)                  # read-only
        # the scan's own counts and the selection's share the slot-owned buffer: accumulate adds one onto the other
        g.count_states(accumulate=True)
        np.testing.assert_array_equal(g.state_counts_to_host(), want + countref.state_counts(table, ids))
        # per document
        g.set_doc_offsets(off)
        assert g.select_leftmost_longest_documents(off.size - 1) == dpick.size
        assert g.count_selection_states(d_counts=guard.ptr) == dpick.size
        guard.check(what="d_counts of the document selection")
        np.testing.assert_array_equal(counts_of(guard), dwant)
        # the selection in the caller's d_out, passed as d_sel
        d_out = torch.zeros(pos.size, dtype=torch.int64, device="cuda:0")
        n2, _ = g.select_leftmost_longest(0, d_out=d_out, out_cap=pos.size)
        assert n2 == pick.size
        assert status_of(g.count_selection_states) == E_STATE                   # it went to the caller's buffer
        assert g.count_selection_states(d_sel=d_out) == n2
        np.testing.assert_array_equal(g.state_counts_to_host(), want)
        assert status_of(lambda: g.count_selection_states(d_sel=int(d_out.data_ptr()) + 4)) == E_ARG
        # ... and a buffer that holds no selection of this table: refused before a counter changes
        junk = torch.full((pos.size,), -1, dtype=torch.int64, device="cuda:0")
        assert status_of(lambda: g.count_selection_states(d_sel=junk, d_counts=guard.ptr)) == E_ARG
        np.testing.assert_array_equal(counts_of(guard), dwant)
        # stale: a new scan, a filter
        g.select_leftmost_longest(0)
        scan(g, buf)
        assert status_of(g.count_selection_states) == E_STATE
        g.select_leftmost_longest(0)
        assert g.count_selection_states() == pick.size
        assert 0 < g.filter_whole_words() < pos.size
        assert status_of(lambda: g.count_selection_states(d_counts=guard.ptr)) == E_STATE
        guard.check(what="d_counts after the refused calls")
        np.testing.assert_array_equal(counts_of(guard), dwant)
        np.testing.assert_array_equal(g.state_counts_to_host(), want)           # the slot's counts: as they were
        # an earlier table
        g.select_leftmost_longest(0)
        g.load_table(table)
        assert status_of(g.count_selection_states) == E_STATE


# ---------------------------------------------------------------------------
# errors: the status, and the counts as they were

def test_errors_leave_the_counts_alone(resolve):
    import torch
    pat = "xaa"
    buf = para_bytes(resolve, N)
    pos, ids, _ = oracle_records(resolve, pat, N)
    table = PfacTable.from_file(resolve(pat), 256)
    other = PfacTable.from_file(resolve("experimentpattern"), 256)
    want = countref.state_counts(table, ids)
    guard = guarded_counts(table, fill=0x3C)

    def refused(fn, status, what):
        assert status_of(fn) == status, what
        guard.check(payload_untouched=True, what="d_counts after " + what)

    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        refused(lambda: g.count_states(d_counts=guard.ptr), E_STATE, "no scan")
        assert status_of(g.state_counts_to_host) == E_STATE                     # fetch before any count
        g.reserve(0, buf.size, 1 << 16)
        g.h2d(buf)
        g.scan_async(buf.size)
        refused(lambda: g.count_states(d_counts=guard.ptr), E_STATE, "a scan that is not finished")
        assert g.scan_finish()[0] == pos.size
        nf = table.num_final
        for n_states in (nf - 1, nf + 1, 0):
            assert raw_count(g, guard.ptr, n_states)[0] == E_ARG
        assert raw_count(g, guard.ptr, flags=2)[0] == E_ARG and raw_count(g, guard.ptr, flags=0x80000001)[0] == E_ARG
        refused(lambda: g.count_states(d_counts=guard.ptr + 4), E_ARG, "a misaligned d_counts")
        refused(lambda: g.count_states(d_counts=guard.ptr, d_records=g.records_ptr() + 16), E_ARG, "a foreign heap")
        assert status_of(g.state_counts_to_host) == E_STATE                     # still nothing counted
        # the scan's state is judged before the arguments
        g.load_table(table)
        assert raw_count(g, guard.ptr, nf + 1, flags=2)[0] == E_STATE           # an earlier table
        refused(lambda: g.count_states(d_counts=guard.ptr), E_STATE, "a scan made with an earlier table")
        scan(g, buf)
        assert g.count_states() == pos.size
        own = g.state_counts_to_host()
        np.testing.assert_array_equal(own, want)
        g.reserve(0, 0, 1 << 22)                                                # drops the scan
        refused(lambda: g.count_states(d_counts=guard.ptr), E_STATE, "a reserve that dropped the scan")
        assert status_of(g.count_states) == E_STATE
        np.testing.assert_array_equal(g.state_counts_to_host(), own)            # the slot's counts outlive it
        # a heap that is too small
        heap = torch.zeros(64 * 4, dtype=torch.uint8, device="cuda:0")
        g.h2d(buf)
        g.scan_async(buf.size, d_records=heap, capacity=64)
        assert g.scan_finish(allow_overflow=True)[1]
        refused(lambda: g.count_states(d_counts=guard.ptr, d_records=heap), E_OVERFLOW, "an overflowed scan")
        assert raw_count(g, guard.ptr, nf + 1, d_records=int(heap.data_ptr()))[0] == E_OVERFLOW
        assert status_of(g.count_states) == E_OVERFLOW
        np.testing.assert_array_equal(g.state_counts_to_host(), own)
        guard.check(payload_untouched=True, what="d_counts after every refused call")
        # another table: its own n_states, the slot's counts replaced
        g.load_table(other)
        scan(g, buf)
        assert raw_count(g, 0, nf)[0] == E_ARG
        np.testing.assert_array_equal(g.state_counts_to_host(), own)            # (counted with the table before)
        assert status_of(lambda: g.count_states(accumulate=True)) == E_STATE
        assert g.count_states() == 4900
        assert g.state_counts_to_host().size == 4


def test_empty_ranges_count_nothing(resolve):
    table = PfacTable.from_file(resolve("xaa"), 256)
    buf = para_bytes(resolve, 2 * TILE + 5)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        guard = guarded_counts(table)
        for part, n_owned in ((buf, 0), (buf[:0], 0)):
            assert scan(g, np.ascontiguousarray(part), n_owned) == 0
            assert g.count_states(d_counts=guard.ptr) == 0
            g.sync()
            guard.check(what="d_counts of an empty range")
            assert not counts_of(guard).any()
            guard.payload().fill_(0xA5)
            assert g.count_states() == 0 and not g.state_counts_to_host().any()
        assert not g.count_patterns(b"").any()
        # nothing added either
        scan(g, buf)
        n = g.count_states()
        own = g.state_counts_to_host()
        scan(g, buf, 0)
        assert g.count_states(accumulate=True) == 0
        np.testing.assert_array_equal(g.state_counts_to_host(), own)
        assert n == int(own.sum()) > 0
