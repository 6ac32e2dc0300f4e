"""tests/bigout.py pinned on the CPU: `window` over segment tables equals replref.splice, gatherref.gather_ref and
docreplref.per_doc on the small gather cases and on a dozen seeded pass cases, whatever the chunk; a twin of it made
wrong in one way at a time differs on a small case; and the cases whose outputs pass 2^32 bytes, built as segment
tables only, satisfy the conditions under which a 32-bit offset cannot hide.  Nothing of 4 GB is materialised.

A walk in chunks of 1 and 17 bytes covers the whole output where it has at most 64 KiB, else its first and last KiB and
the KiB around each of 8 seeded run boundaries: `window` keeps no state between calls, so the chunk shows only at the
two ends of a window, and those windows put such ends on and next to run boundaries of every kind."""
import numpy as np
import pytest

import bigout
from bigout import G4, BigGather, BigReplace, BigText, EdgeGather, Segments, window
from docreplref import per_doc
from gatherref import all_gather_cases, gather_ref
from orc import Oracle
from passfuzz import Case, Expect
from replref import splice

WHOLE = 1 << 16
DEFECTS = ("out_off_truncated_to_32_bits", "search_right_false", "replacement_runs_not_rebased", "tail_gap_dropped")


def ranges(seg):
    total = seg.total
    if total <= WHOLE:
        return [(0, total)]
    at = seg.out_off[np.random.default_rng(seg.n_seg).integers(0, seg.n_seg, 8)].astype(np.int64)
    at = np.clip(at - 512, 0, total - 1024)
    return [(0, 1024), (total - 1024, total)] + [(int(a), int(a) + 1024) for a in at]


def assert_window_equals(seg, source, want, what):
    want = np.asarray(want, dtype=np.uint8)
    assert seg.total == want.size, f"{what}: {seg.total} bytes in the table, want {want.size}"
    assert np.array_equal(window(seg, source, 0, seg.total), want), f"{what}: one window over the whole output"
    assert window(seg, source, total := seg.total, total).size == 0
    for chunk in (1, 17):
        for a, b in ranges(seg):
            got = [window(seg, source, x, min(x + chunk, b)) for x in range(a, b, chunk)]
            got = np.concatenate(got) if got else np.zeros(0, np.uint8)
            bad = np.flatnonzero(got != want[a:b])
            assert bad.size == 0, f"{what}: chunk {chunk}: byte {a + int(bad[0])} differs"


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", all_gather_cases(), ids=repr)
def test_gather_segments_equal_gather_ref(case):
    want, want_off = gather_ref(case.data, case.offsets, case.ids)
    seg = bigout.gather_segments(case.offsets, case.ids)
    np.testing.assert_array_equal(seg.out_off, want_off)
    assert_window_equals(seg, case.data, want, case.name)


@pytest.fixture(scope="module")
def pass_cases(tmp_path_factory):
    """(case, Expect, pattern file) of the first dozen seeds of tests/passfuzz.py with n <= 70001 and at most 8 MiB of
    output (one seed's replacements make 94 MB of it)."""
    d = tmp_path_factory.mktemp("bigout")
    out, seed = [], 0
    while len(out) < 12:
        c = Case(seed)
        seed += 1
        if c.n > 70001:
            continue
        path = c.write_patterns(str(d / f"{c.seed}.pat"))
        want = Expect(c, path)
        p, l, i = want.sel
        if bigout.replace_segments(c.entry, c.n_owned, p, l, i, want.table, n_source=c.n).total <= 8 << 20:
            out.append((c, want, path))
    return out


def test_replace_segments_equal_splice(pass_cases):
    picks = 0
    for c, want, _ in pass_cases:
        p, l, i = want.sel
        seg = bigout.replace_segments(c.entry, c.n_owned, p, l, i, want.table, n_source=c.n)
        assert seg.n_seg == 2 * p.size + 1
        assert_window_equals(seg, bigout.replace_source(c.data, want.table),
                             splice(c.data, c.entry, c.n_owned, p, l, i, want.table), c.describe())
        picks += p.size
    assert picks > 1000


def test_doc_replace_segments_equal_per_doc(pass_cases):
    docs = 0
    for c, want, path in pass_cases:
        o = Oracle(path, 1, 1)
        sfirst, pos, ids, out_off, out = per_doc(o, c.data, c.off, want.ll, want.table)
        o.close()
        seg, doc_out = bigout.doc_replace_segments(c.off, sfirst, pos, want.ll[ids], ids, want.table, c.n)
        np.testing.assert_array_equal(doc_out, out_off, err_msg=c.describe())
        assert_window_equals(seg, bigout.replace_source(c.data, want.table), out, c.describe() + " per document")
        docs += c.off.size - 1
    assert docs > 100


# ---------------------------------------------------------------------------
# seeded defects

def twin_window(seg, source, a, b, defect):
    """bigout.window, wrong in the way `defect` names (the two defects of the tables are made by `twin_segments`)."""
    out_off, src_off = seg.tables(source)
    i = np.arange(int(a), int(b), dtype=np.int64)
    if defect == "out_off_truncated_to_32_bits":
        out_off = out_off & np.int64(0xFFFFFFFF)
    k = np.searchsorted(out_off, i, side="left" if defect == "search_right_false" else "right") - 1
    return source[src_off[k] + (i - out_off[k])]


def twin_segments(seg, n_source, defect):
    """The table of a replace as a constructor with `defect` would have built it."""
    out_off, src_off = seg.out_off.copy(), seg.src_off.copy()
    if defect == "replacement_runs_not_rebased":
        src_off[1::2] -= n_source
    if defect == "tail_gap_dropped":
        out_off[-1] = out_off[-2]
    return Segments(out_off, src_off)


def synthetic_past_4g():
    """3 000 runs of 2 MiB from seeded places of a 4 MiB source: 6.3 GB of output as a table of 3 001 offsets."""
    rng = np.random.default_rng(32)
    source = rng.integers(0, 256, 4 << 20, dtype=np.uint8)
    seg = Segments(np.arange(3001, dtype=np.int64) * (2 << 20), rng.integers(0, 2 << 20, 3000))
    return seg, source


def differs(fn, want):
    try:
        got = fn()
    except IndexError:
        return True
    return got.size != want.size or not np.array_equal(got, want)


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_defect_is_caught(defect, pass_cases):
    caught = 0
    if defect == "out_off_truncated_to_32_bits":
        seg, source = synthetic_past_4g()
        for a in (G4 - 2048, G4 + 4096):                        # only these two windows of the 6.3 GB exist
            want = window(seg, source, a, a + 4096)
            k = bigout.segment_of(seg, a)
            assert np.array_equal(want[:64], source[int(seg.src_off[k]) + a - int(seg.out_off[k]):][:64])
            caught += differs(lambda: twin_window(seg, source, a, a + 4096, defect), want)
        assert caught == 2
        return
    for c, want, _ in pass_cases:
        p, l, i = want.sel
        seg = bigout.replace_segments(c.entry, c.n_owned, p, l, i, want.table, n_source=c.n)
        source = bigout.replace_source(c.data, want.table)
        whole = window(seg, source, 0, seg.total)
        if defect == "search_right_false":
            caught += differs(lambda: twin_window(seg, source, 0, seg.total, defect), whole)
        else:
            bad = twin_segments(seg, c.n, defect)
            caught += differs(lambda: window(bad, source, 0, bad.total), whole)
    assert caught >= 1, f"no small case shows {defect}"


# ---------------------------------------------------------------------------
# the big cases, as tables

def test_big_gather_case():
    g = BigGather()
    bigout.conditions(g.seg, g.data, "the big gather")
    assert g.n_ids > (1 << 20) + 4096                                            # (d)
    assert 190e6 < g.n < 215e6 and g.seg.n_seg == g.n_ids
    lens = np.diff(g.offsets.astype(np.int64))
    empty = lens[g.ids.astype(np.int64)] == 0
    for at in g.empty_runs_at:
        assert bool(empty[at:at + 64].all()), f"no run of 64 ids of empty documents at {at}"
    assert int((lens == 0).sum()) > 300 and int(lens.max()) == 8191
    assert np.unique(g.ids).size < g.n_ids                                       # repeats


def test_edge_gather_cases():
    e = EdgeGather(with_data=False)
    assert e.n > (64 << 20) + (16 << 10)
    for size in e.SIZES:
        seg = bigout.gather_segments(e.offsets(size), e.ids)
        assert seg.total == size and int(seg.out_off[-2]) == e.prefix
    assert [s - (64 << 20) for s in e.SIZES] == [-1, 0, 1, 1025, 3 * 1024 + 7, 16 * 1024 - 15]


@pytest.fixture(scope="module")
def big_replace(tmp_path_factory):
    return BigReplace(tmp_path_factory.mktemp("bigreplace"))


@pytest.mark.parametrize("config", ["whole", "halo"])
def test_big_replace_case(big_replace, config):
    r = big_replace
    c = r.configs[config]
    bigout.conditions(c["seg"], r.source, f"the big replace ({config})")
    assert (1 << 20) <= r.n <= (2 << 20)
    pos, ids = c["picks"]
    n_of = np.bincount(ids, minlength=6)
    assert n_of[1] > 60_000 and n_of[2] > 10_000 and n_of[3] > 100_000 and n_of[4] > 10_000, n_of      # every kind is picked
    d = ids == 3
    assert int((d[1:] & d[:-1] & (pos[1:] == pos[:-1] + 1)).sum()) > 10_000     # deletions back to back
    assert len(r.reps[1]) == 65536 and len(r.reps[4]) == 17 and r.reps[3] == b""
    if config == "halo":
        assert c["entry"] > 0 and c["n_owned"] < r.n and c["exit"] == 2
    else:
        assert (c["entry"], c["n_owned"], c["exit"]) == (0, r.n, 0)
    # the table is the splice: the first and the last 200 picks, materialised
    for sl in (slice(0, 200), slice(pos.size - 200, pos.size)):
        p, i = pos[sl], ids[sl]
        a = c["entry"] if sl.start == 0 else int(pos[sl.start - 1] + r.ll[ids[sl.start - 1]])
        b = int(p[-1] + r.ll[i[-1]]) if sl.start == 0 else c["n_owned"]
        part = splice(r.data, a, b, p, r.ll[i], i, r.table)
        at = 0 if sl.start == 0 else c["seg"].total - part.size
        assert np.array_equal(window(c["seg"], r.source, at, at + part.size), part)


def test_big_doc_replace_case(big_replace):
    r = big_replace
    seg, doc_out = r.per_document()
    bigout.conditions(seg, r.source, "the big per-document replace")
    assert doc_out.size == r.doc_off.size and int(doc_out[-1]) == seg.total
    assert int((doc_out > G4).sum()) >= 5 and int((doc_out[1:] == doc_out[:-1]).sum()) >= 5        # above 2^32; empty documents
    assert 200 < r.doc_off.size - 1 < 400


def test_big_text_case(tmp_path):
    t = BigText(tmp_path)
    nbytes = t.text_bytes()
    assert bigout.OUT_MIN <= nbytes <= bigout.OUT_MAX                            # (a)
    assert t.base < 10 ** 9 < t.base + t.n
    assert sorted(np.unique(t.count).tolist()) == list(range(17))
    tiles = np.add.reduceat(t.count, np.arange(0, t.n, 4096))
    assert int((tiles == 0).sum()) >= 4 and int(tiles.max()) > 14 * 4096       # empty tiles, and tiles of 14 records a byte
    t.assert_oracle_agrees()
    pos, ids = t.records(0, 4096)
    assert len(t.format(pos[:500], ids[:500])) == int(t.line_lengths(pos, ids)[:500].sum())
    q = t.quarter()
    assert t.data[q - 1] != ord("a") and t.text_bytes(q) < G4 and t.text_bytes(q) > nbytes // 5
    pos, ids, ends = t.all_line_ends(300_000)
    np.testing.assert_array_equal(ends, np.cumsum(t.line_lengths(pos, ids)))
    cross = 10 ** 9 - t.base
    for lo, hi in ((0, 300_000), (cross - 100_000, cross + 100_000)):            # per line = per position
        pos, ids = t.records(lo, hi)
        assert int(t.line_lengths(pos, ids).sum()) == t.text_bytes(hi) - t.text_bytes(lo)


def test_assert_device_equals_names_the_first_difference():
    """The walk of tests/test_gpu_outputs_past_4g.py on torch's CPU tensors: an output given as a tensor and as a
    fetch, chunks that do not divide it, and one wrong byte reported by its index and its run."""
    import torch
    case = next(c for c in all_gather_cases() if c.name == "ids_repeats")
    want, _ = gather_ref(case.data, case.offsets, case.ids)
    seg = bigout.gather_segments(case.offsets, case.ids)
    source, out = torch.from_numpy(case.data.copy()), torch.from_numpy(want.copy())
    assert np.array_equal(window(seg, source, 5, want.size - 3).numpy(), want[5:want.size - 3])
    for chunk in (7, 1000, want.size + 1):
        bigout.assert_device_equals(seg, source, out, want.size, chunk=chunk)
        bigout.assert_device_equals(seg, source, lambda first, n: want[first:first + n], want.size, chunk=chunk)
    at = want.size // 2 + 3
    bad = want.copy()
    bad[at] ^= 0x40
    bad[at + 20] ^= 1
    k = bigout.segment_of(seg, at)
    for d_out in (torch.from_numpy(bad), lambda first, n: bad[first:first + n]):
        with pytest.raises(AssertionError, match=rf"output byte {at} is 0x{int(bad[at]):02x}, want 0x{int(want[at]):02x} \(run {k} of"):
            bigout.assert_device_equals(seg, source, d_out, want.size, chunk=1000)
    with pytest.raises(AssertionError, match="output bytes, want"):
        bigout.assert_device_equals(seg, source, out, want.size - 1)
