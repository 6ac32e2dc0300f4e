"""Sessions: ONE GpuMatcher context driven through long sequences of calls (tests/session.py) -- many tables under different
kernel knobs, many sizes, two slots, passes in any order, results fetched late, documented errors in between -- every
result compared bit for bit with what include/pfac.h promises for that history.  The random plans are the suite's seeds;
the named sessions are histories random plans reach rarely; half of the plans and the sessions at the end of this file
have the whole-word filter among their calls, a third of the plans and a group of sessions the per-pattern counts, and a
fourth family of plans and a group of sessions the line path (split, matching documents, context lines, gather), and a
fifth family and the last group of sessions the case fold (pfac_table_set_case_fold) as a setting with a life of its own.
Run with -m gpu on an MI355X.  Expectations come from the
CPU oracle, llref, replref, docref, docreplref, splitref, gatherref and the pattern files, never from the device.  No session aims at the
scan's wait protocol: they provoke the errors the header documents, nothing else."""
import gc
import weakref

import numpy as np
import pytest

import session as S
from passfuzz import knob_label
from phfpfac_amd import GpuMatcher
from phfpfac_amd.matcher import splitmix64_bytes, tiled_bytes

pytestmark = pytest.mark.gpu

X = S.expectations()
TILE_BYTES = S.TILE


def k(tab, **knobs):
    i = S.KNOBS.index(knobs)
    assert i in S.POOL[tab]["knobs"]
    return i


def load(tab, rkey="r0", cknob=None, **knobs):
    """Upload, lengths, replacements; `cknob`: the entry of S.CKNOBS (the count knobs) the table is installed under."""
    up = dict(op="load_table", tab=tab, knob=k(tab, **knobs), **({} if cknob is None else {"cknob": cknob}))
    return [up, dict(op="set_flen"), dict(op="set_reps", rkey=rkey)]


def scan(tab, inp, slot=0, no=None):
    return dict(op="scan_bytes", slot=slot, inp=inp, no=X.input_size(tab, inp) if no is None else no)


def fkey(tab, *applied):
    """The filter state of a scan of `tab` after the (descriptor, dkey) pairs `applied`."""
    return tuple(sorted({X.applied(tab, f, dkey) for f, dkey in applied}))


def flt(f, slot=0, heap="own"):
    return dict(op="filter", slot=slot, f=f, heap=heap)


def records(tab, inp, slot=0, no=None, first=0, n=None, f=()):
    total = X.count(tab, inp, X.input_size(tab, inp) if no is None else no, f)
    return dict(op="records", slot=slot, first=first, n=total - first if n is None else n)


def doc(tab, inp, dkey, slot=0, no=None):
    return dict(op="set_doc", slot=slot, tab=tab, inp=inp, no=X.input_size(tab, inp) if no is None else no, dkey=dkey)


def pss(kind, slot=0, own=True, entry=0):
    op = dict(op=kind, slot=slot, own=own, small=False)
    if kind == "select":
        op["entry"] = entry
    return op


def fetch(kind, slot=0, **kw):
    return dict(op=kind, slot=slot, **kw)


def cnt(slot=0, dst="own", acc=False, heap="own", ns="ok"):
    return dict(op="count", slot=slot, dst=dst, acc=acc, heap=heap, ns=ns)


def cnt_sel(slot=0, dst="own", acc=False, sel="own"):
    return dict(op="count_sel", slot=slot, dst=dst, acc=acc, sel=sel)


def cnt_fetch(slot=0):
    return dict(op="cnt_fetch", slot=slot)


def run(ops, want=None):
    """The operations on one fresh context; `want`: the statuses the model must give, as a check of the session itself."""
    m = S.Model()
    if want is not None:
        probe = S.Model()
        got = [probe.apply(op).status for op in ops]
        assert got == want, [(S.fmt(op), S.STATUS_NAMES[g]) for op, g in zip(ops, got)]
    with GpuMatcher(0, S.N_SLOTS) as g:
        return S.run(g, ops, m, seed="named")


@pytest.mark.parametrize("seed,family", [(s, "") for s in S.SEEDS] + [(s, "words") for s in S.WORD_SEEDS] + [(s, "counts") for s in S.COUNT_SEEDS]
                         + [(s, "lines") for s in S.LINE_SEEDS] + [(s, "fold") for s in S.FOLD_SEEDS],
                         ids=[str(s) for s in S.SEEDS] + [f"words-{s}" for s in S.WORD_SEEDS] + [f"counts-{s}" for s in S.COUNT_SEEDS]
                         + [f"lines-{s}" for s in S.LINE_SEEDS] + [f"fold-{s}" for s in S.FOLD_SEEDS])
def test_session(seed, family):
    """One random plan on one context; `family`: "words" = a plan that filters whole words, "counts" = one that also
    counts matches per pattern, "lines" = one that also splits at a delimiter, lists the matching documents and gathers
    their bytes, "fold" = one that also toggles the case fold, over the larger pool with the nocase tables."""
    ops = S.plan(seed, words=family == "words", counts=family == "counts", lines=family == "lines", fold=family == "fold")
    tag = f" ({family})" if family else ""
    with GpuMatcher(0, S.N_SLOTS) as g:
        st = S.run(g, ops, S.Model(), seed=f"{seed}{tag}" if family else seed)
    print(f"session {seed}{tag}: {st['ops']} operations ({st['errors']} documented errors), {st['compared']} records and bytes compared, "
          f"record widths {sorted(st['widths'])}, staging {sorted(st['staging'])}, {sorted(st['variants'])}, {st['counts']} counts under "
          f"{sorted(st['regimes'])}, {st['splits']} splits, {st['matchings']} matching calls, {st['gathers']} gathers, {st['ids']} document ids "
          f"and offsets compared, {st['folded']} folded scans, {st['toggles']} toggles and {st['modes']} modes compared")


def test_large_dense_then_tiny_sparse_then_every_pass():
    """Every scratch and output buffer is sized by the large scan and then used by a tiny one: what a pass does not
    clear of d_gsum, the tile counts, the bitmaps or the outputs still holds the large call's data."""
    t = "abc2"
    ops = load(t) + [scan(t, 0), records(t, 0), doc(t, 0, "d0"), pss("segment"), pss("select"), pss("replace"), pss("select_docs"),
                     pss("replace_docs"), fetch("text", base=0), fetch("checksum", base=0)]
    for inp in (3, 2):                                           # 17 bytes, then 64 tiles + 1 byte at 2 % density
        total = len(X.text(t, inp, X.input_size(t, inp), 999_999_990))
        ops += [scan(t, inp), records(t, inp), fetch("packed"), fetch("checksum", base=999_999_990), fetch("text", base=999_999_990),
                fetch("text_fetch", first=total // 2, n=total - total // 2),
                doc(t, inp, "d1"), pss("segment"), fetch("seg_fetch"), pss("select", entry=1), fetch("sel_fetch"), pss("replace"),
                fetch("rp_fetch", first=0, n=int(X.replace(t, inp, X.input_size(t, inp), 1, "r0").size)),
                pss("select_docs"), fetch("docsel_fetch"), fetch("seg_fetch"), pss("replace_docs"), fetch("rpd_fetch"),
                pss("segment", own=False), pss("select_docs", own=False), pss("replace_docs", own=False), pss("select", own=False),
                pss("replace", own=False)]
    st = run(ops, want=[S.OK] * len(ops))
    assert st["compared"] > 300_000


def test_staging_layout_flips_both_ways_with_exact_records():
    """Dense and matchless inputs of 74 tiles in turn, no knob pinned: the staging layout of the NEXT scan follows the
    density of the last one, for the whole context -- so slot 1's scan runs in the mode slot 0's scan chose."""
    t = "abc2"
    seen = []
    with GpuMatcher(0, S.N_SLOTS) as g:
        ex = S.Executor(g, S.Model())
        for op in load(t):
            ex.step(op)
        seen.append(g.info()["staging_buffers"])
        for rnd, inp in enumerate((0, 1, 0, 0, 1, 1, 0, 1)):
            ex.step(scan(t, inp, slot=rnd % 2))
            seen.append(g.info()["staging_buffers"])
            ex.step(records(t, inp, slot=rnd % 2))
            ex.step(fetch("checksum", slot=rnd % 2, base=0))
    to_dense = sum(a != 1 and b == 1 for a, b in zip(seen, seen[1:]))
    from_dense = sum(a == 1 and b != 1 for a, b in zip(seen, seen[1:]))
    assert to_dense >= 1 and from_dense >= 1, seen


def test_record_width_2_then_8_then_4_on_one_heap():
    """The record width follows the table while the slot's heap and tile index are reused; the records of a scan made
    with an earlier table stay fetchable in THEIR width after the upload, while what needs that table's idmap, lengths
    or replacements is refused (and a refused selection leaves no selection to fetch)."""
    ops = load("abc2") + [scan("abc2", 0), records("abc2", 0), pss("select")]
    ops += load("wide8", PFAC_WIDE="1") + [records("abc2", 0, first=5, n=1000), fetch("packed"), fetch("checksum", base=0), fetch("text", base=0),
                                            pss("select"), pss("replace"), fetch("sel_fetch"),
                                            scan("wide8", 1), records("wide8", 1), fetch("packed"), fetch("checksum", base=0), pss("select")]
    ops += load("mid4") + [records("wide8", 1), pss("segment"), scan("mid4", 2), records("mid4", 2), fetch("packed"), pss("select"),
                           fetch("sel_fetch"), pss("replace"), fetch("rp_fetch", first=0, n=64)]
    E = S.E_STATE
    st = run(ops, want=[0] * 3 + [0, 0, 0] + [0] * 3 + [0, 0, E, E, E, E, E, 0, 0, E, 0, 0] + [0] * 3 + [0, E, 0, 0, 0, 0, 0, 0, 0])
    assert st["widths"] == {2, 4, 8}


def test_bad_document_offsets_then_good_ones():
    """PFAC_E_ARG for offsets that break the rules, and the very next call with good ones is exact (the error word of
    the check is the pass's to clear); new offsets for the slot, even equal ones, end the right of the per-document replace
    to the selection cut with the old ones; an empty scan's per-document selection zeroes every doc_first."""
    t = "l2"
    A = S.E_ARG
    ops = load(t, PFAC_FORCE_L2="1") + [scan(t, 0), doc(t, 0, "bad_end"), pss("segment"), doc(t, 0, "d0"), pss("segment"), fetch("seg_fetch"),
                                        doc(t, 0, "bad_order"), pss("select_docs"), fetch("docsel_fetch"), doc(t, 0, "d1"), pss("select_docs"),
                                        fetch("docsel_fetch"), doc(t, 0, "d1"), pss("replace_docs"), fetch("docsel_fetch"),
                                        doc(t, 0, "bad_order"), pss("segment"), doc(t, 0, "d1"), pss("segment", own=False),
                                        doc(t, 0, "bad_end"), pss("select_docs", own=False), doc(t, 0, "d0"), pss("select_docs", own=False)]
    run(ops, want=[0] * 3 + [0, 0, A, 0, 0, 0, 0, A, S.E_STATE, 0, 0, 0, 0, S.E_STATE, 0, 0, A, 0, 0, 0, A, 0, 0])
    t = "dups"
    ops = load(t) + [scan(t, 0), doc(t, 0, "d1"), pss("select_docs"), fetch("docsel_fetch"), pss("segment"),
                     scan(t, 2), doc(t, 2, "d1"), pss("select_docs"), fetch("docsel_fetch"), pss("segment"), fetch("seg_fetch"),
                     pss("replace_docs"), fetch("rpd_fetch"), doc(t, 2, "bad_end"), pss("select_docs"), doc(t, 2, "d0"), pss("select_docs", own=False)]
    run(ops, want=[0] * 3 + [0] * 13 + [0, A, 0, 0])


def test_replace_output_outlives_new_replacements():
    """replace_selection into the slot-owned buffer, then another table of replacements, then the fetch: the bytes are
    those of the replacements set when the replace ran."""
    t = "mid4"
    n = int(X.replace(t, 2, X.input_size(t, 2), 0, "r0").size)
    ops = load(t, rkey="r0") + [scan(t, 2), pss("select"), pss("replace"), dict(op="set_reps", rkey="r1"), fetch("rp_fetch", first=0, n=n),
                                dict(op="set_reps", rkey="redact"), fetch("rp_fetch", first=n // 3, n=n - n // 3), pss("replace"),
                                fetch("rp_fetch", first=0, n=int(X.replace(t, 2, X.input_size(t, 2), 0, "redact").size))]
    run(ops, want=[S.OK] * len(ops))


@pytest.mark.parametrize("share", [True, False], ids=["shared-stream", "own-streams"])
def test_two_slots_select_and_replace_interleaved(share):
    t = "l2"
    ops = [dict(op="set_stream", slot=1, share=share)] if share else []
    ops += load(t, PFAC_FORCE_L2="1") + [scan(t, 0, slot=0), scan(t, 0, slot=1, no=(300_007 * 5) // 8), pss("select", slot=0, entry=0),
                                         pss("select", slot=1, entry=X.M(t)), pss("replace", slot=0), fetch("sel_fetch", slot=1),
                                         pss("replace", slot=1), fetch("sel_fetch", slot=0),
                                         fetch("rp_fetch", slot=0, first=0, n=int(X.replace(t, 0, 300_007, 0, "r0").size)),
                                         fetch("rp_fetch", slot=1, first=0, n=int(X.replace(t, 0, (300_007 * 5) // 8, X.M(t), "r0").size))]
    if share:
        ops += [dict(op="set_stream", slot=1, share=False), pss("select", slot=1, entry=1), fetch("sel_fetch", slot=1)]
    run(ops, want=[S.OK] * len(ops))


def test_reserve_that_replaces_a_buffer_leaves_no_finished_scan():
    """pfac_slot_reserve growing the record heap or the input after a finished scan, and while one is pending: it waits
    for the scan, and nothing reads the new, uninitialised buffer as if it held the last scan -- PFAC_E_STATE from
    everything that needs one, exact results from the next scan.  Outputs of earlier passes stay fetchable."""
    t = "mid4"
    E = S.E_STATE
    cnt = X.count(t, 2, X.input_size(t, 2))
    grow = lambda which, n: dict(op="reserve_grow", slot=0, which=which, k=n)      # noqa: E731
    ops = load(t) + [scan(t, 2), pss("select"), grow("records", 1), records(t, 2), fetch("checksum", base=0), fetch("text", base=0),
                     fetch("packed"), pss("segment"), pss("select"), pss("replace"), dict(op="scan_finish", slot=0),
                     scan(t, 2), records(t, 2), pss("select"), grow("input", 2), pss("replace"), fetch("sel_fetch"), records(t, 2, n=3),
                     scan(t, 1), records(t, 1),
                     dict(op="scan_start", slot=0, inp=2, no=X.input_size(t, 2), cap=cnt + cnt // 4 + 65536), grow("both", 3),
                     dict(op="scan_finish", slot=0), records(t, 2, n=1), fetch("checksum", base=0),
                     dict(op="scan_start", slot=0, inp=2, no=X.input_size(t, 2), cap=cnt + cnt // 4 + 65536), dict(op="scan_finish", slot=0),
                     records(t, 2), grow("both", 4), records(t, 2, n=2)]
    run(ops, want=[0] * 3 + [0, 0, 0] + [E] * 8 + [0, 0, 0, 0, E, 0, E, 0, 0, 0, 0, E, E, E, 0, 0, 0, 0, E])


def test_scan_finish_keeps_the_copy_queued_after_scan_async():
    """scan_async, h2d of the next chunk, scan_finish: the next chunk's host array is still referenced, or its copy has
    left it -- and the scan after it sees the right bytes."""
    t = "abc2"
    first, nxt = X.input(t, 1), X.input(t, 0).copy()
    with GpuMatcher(0, 1) as g:
        g.load_table(X.table(t))
        g.reserve(0, nxt.size, 1 << 20)
        g.h2d(first.copy(), 0)
        g.scan_async(first.size, slot=0)
        ref = weakref.ref(nxt)
        g.h2d(nxt, 0)
        del nxt
        n0, over = g.scan_finish(0)
        gc.collect()
        alive = ref() is not None
        done = g.h2d_done(0)
        assert alive or done, "scan_finish released a host array whose copy had not finished"
        assert (n0, over) == (X.count(t, 1, first.size), False)
        g.scan_async(first.size, slot=0)
        n1, over = g.scan_finish(0)
        rec = g.records_to_host(n1)
        pos, ids, _ = X.scan(t, 0, first.size)
    assert ref() is None, "sync released the array"
    assert n1 == pos.size and not over
    np.testing.assert_array_equal(rec["pos"].astype(np.int64), pos)
    np.testing.assert_array_equal(X.table(t).idmap[rec["state"]], ids)


def test_fill_then_partial_h2d_into_the_same_buffer():
    """fill_random of a 1 GiB slot input, then 4 KiB of known bytes into its last tile: the fills return once the slot's
    stream is idle, so the copy -- which is ordered behind what the slot's stream has queued when pfac_slot_h2d is called,
    and a fill on another stream would not be -- cannot be overtaken by the fill.
    The tile is read back through a scan with no match and a replace without picks, which copies its input."""
    t, n = "abc2", 1 << 30
    rng = np.random.default_rng(5)
    known = rng.integers(0, 256, 4096).astype(np.uint8)
    known[known == ord("a")] = 0
    with GpuMatcher(0, 1) as g:
        g.load_table(X.table(t))
        g.set_final_lengths(X.table(t).final_lengths())
        g.set_replacements(X.reps(t, "r0"))
        g.reserve(0, n, 4096)
        g.fill_random(g.input_ptr(0), n, 0x1234)
        g.h2d(known, 0, dst_offset=n - 4096)
        g.sync(0)
        off = n - 4096
        g.scan_async(4096, 4096, d_input=g.input_ptr(0) + off, slot=0)
        assert g.scan_finish(0) == (0, False)
        assert g.select_leftmost_longest(0) == (0, 0)
        assert g.replace_selection(d_input=g.input_ptr(0) + off) == 4096
        np.testing.assert_array_equal(g.replacement_to_host(4096), known)
        g.scan_async(4096, 4096, d_input=g.input_ptr(0) + off - 4096, slot=0)      # the tile before it still holds the fill
        n_before = g.scan_finish(0)[0]
        g.select_leftmost_longest(0)
        m = g.replace_selection(d_input=g.input_ptr(0) + off - 4096)
        want = splitmix64_bytes(n, 0x1234)[off - 4096:off]
        assert n_before == int((want == ord("a")).sum())
        if n_before == 0:
            np.testing.assert_array_equal(g.replacement_to_host(m), want)


# The input's readers and the next upload.  Three passes return to the host as soon as a count is known and read the slot's
# input AGAIN from a kernel queued behind that: the write kernels of the replace, of the split and of the gather.  The next
# chunk's pfac_slot_h2d into the same slot must wait for them (include/pfac.h), not for the slot's last scan only.  1 GiB of
# input makes the write kernel long enough for a 4 KiB copy to overtake it where the order is missing; every expectation is
# analytic or a window of splitmix64, so no host array is larger than a few KiB.  A wrong byte, never a fault.
UP_N, UP_TAIL = 1 << 30, 4096


def _random_window(first, n, seed):
    """Bytes [first, first + n) of what fill_random(.., seed) writes (first a multiple of 8)."""
    assert first % 8 == 0
    return splitmix64_bytes(n, seed + first // 8)


def _upload_over_the_tail(g, original_tail):
    """The next chunk's upload, at once: 4 KiB into the end of the slot's input, every byte different from what is there."""
    assert original_tail.size == UP_TAIL
    g.h2d(original_tail ^ np.uint8(0xFF), 0, dst_offset=UP_N - UP_TAIL)


def test_upload_waits_for_the_replace_that_reads_the_input():
    """Tiled bytes outside the table's alphabet: no match, so the replace's output is its input.  The upload of other
    bytes over the input's last 4 KiB right behind the replace must not show in the output's last 8 KiB."""
    t = "abc2"
    period = bytes(range(0x20, 0x20 + 61))                      # (61 bytes, none of them a, b or c: a period that is no divisor of the tile)
    assert not set(period) & set(b"abc")
    want = tiled_bytes(2 * UP_TAIL, period, phase=(UP_N - 2 * UP_TAIL) % len(period))
    with GpuMatcher(0, 1) as g:
        g.load_table(X.table(t))
        g.set_final_lengths(X.table(t).final_lengths())
        g.set_replacements(X.reps(t, "r0"))
        g.reserve(0, UP_N, 1 << 20)
        g.fill_tiled(g.input_ptr(0), UP_N, period)
        g.scan_async(UP_N, UP_N, slot=0)
        assert g.scan_finish(0) == (0, False)
        assert g.select_leftmost_longest(0) == (0, 0)
        assert g.replace_selection() == UP_N
        _upload_over_the_tail(g, want[UP_TAIL:])
        got = g.replacement_to_host(2 * UP_TAIL, first=UP_N - 2 * UP_TAIL)
        g.sync(0)
    bad = np.flatnonzero(got != want)
    print(f"replace, then the upload: {bad.size} of {got.size} bytes of the output's tail are not the original's")
    assert bad.size == 0, f"{bad.size} bytes of the output come from the NEXT upload, the first at {UP_N - 2 * UP_TAIL + int(bad[0])}"


@pytest.mark.parametrize("order", ["ascending", "reversed"])
def test_upload_waits_for_the_gather_that_reads_the_input(order):
    """1024 documents of 1 MiB cut by the caller's offsets, ids 0..1023 or 1023..0, over fill_random's bytes: ascending
    the output is the input; reversed its first MiB is the input's last document, which the upload goes into, and its
    last is document 0."""
    import torch
    seed, n_docs = 0x51DE, 1024
    size = UP_N // n_docs
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")      # noqa: E731
    d_off = to_dev(np.arange(n_docs + 1, dtype=np.uint64) * np.uint64(size))
    ids = np.arange(n_docs, dtype=np.uint64)
    d_ids = to_dev(ids if order == "ascending" else ids[::-1])
    torch.cuda.synchronize()
    in_tail = _random_window(UP_N - 2 * UP_TAIL, 2 * UP_TAIL, seed)
    doc0_tail = _random_window(size - 2 * UP_TAIL, 2 * UP_TAIL, seed)
    with GpuMatcher(0, 1) as g:
        g.reserve(0, UP_N, 4096)
        g.fill_random(g.input_ptr(0), UP_N, seed)
        assert g.gather_documents(n_docs, n_docs, UP_N, d_doc_offsets=d_off.data_ptr(), d_ids=d_ids.data_ptr()) == UP_N
        _upload_over_the_tail(g, in_tail[UP_TAIL:])
        # where the input's last 8 KiB and document 0's last 8 KiB are in the output
        at_in, at_doc0 = (UP_N - 2 * UP_TAIL, size - 2 * UP_TAIL) if order == "ascending" else (size - 2 * UP_TAIL, UP_N - 2 * UP_TAIL)
        got_in = g.gathered_to_host(2 * UP_TAIL, first=at_in)
        got_doc0 = g.gathered_to_host(2 * UP_TAIL, first=at_doc0)
        got_off = g.gathered_offsets_to_host(n_docs)
        g.sync(0)
    bad = np.flatnonzero(got_in != in_tail)
    print(f"gather ({order}), then the upload: {bad.size} of {got_in.size} bytes of the input's tail in the output are not the original's")
    np.testing.assert_array_equal(got_off, np.arange(n_docs + 1, dtype=np.uint64) * np.uint64(size))
    np.testing.assert_array_equal(got_doc0, doc0_tail)
    assert bad.size == 0, f"{bad.size} bytes of the output come from the NEXT upload, the first at {at_in + int(bad[0])}"


def test_upload_waits_for_the_split_that_reads_the_input():
    """One delimiter per period of 509 bytes: document k starts at 509 k and the rest behind the last delimiter is an
    unterminated tail.  The split's second read of the input places the offsets; the upload right behind the call holds no
    delimiter, so offsets of the last two tiles that are wrong or missing show that it came first."""
    P, delim = 509, 0x0A
    period = bytes([0x41 + k % 26 for k in range(P - 1)]) + bytes([delim])
    full = UP_N // P
    assert UP_N % P and (UP_N - 2 * TILE_BYTES) // P < full - 8
    k = 2 * TILE_BYTES // P + 4                                # the offsets fetched: every delimiter of the last two tiles, and more
    want = np.concatenate([np.arange(full + 1 - (k - 1), full + 1, dtype=np.uint64) * np.uint64(P), np.array([UP_N], dtype=np.uint64)])
    tail = tiled_bytes(UP_TAIL, period, phase=(UP_N - UP_TAIL) % P)
    with GpuMatcher(0, 1) as g:
        g.reserve(0, UP_N, 4096)
        g.fill_tiled(g.input_ptr(0), UP_N, period)
        n_docs, tail_start = g.split_documents(UP_N, bytes([delim]))
        up = tail ^ np.uint8(0xFF)
        assert not (up == delim).any()
        g.h2d(up, 0, dst_offset=UP_N - UP_TAIL)
        got = g.doc_offsets_to_host(n_docs, first=max(n_docs + 1 - k, 0), n=k)
        g.sync(0)
    assert (n_docs, tail_start) == (full + 1, full * P)
    bad = np.flatnonzero(got != want)
    print(f"split, then the upload: {bad.size} of the last {k} offsets are not the original's")
    assert bad.size == 0, f"offset {n_docs + 1 - k + int(bad[0])} is {int(got[bad[0]])}, not {int(want[bad[0]])}"


def test_stream_change_between_a_selection_and_its_replace():
    """A selection's writes are asynchronous on the slot's stream; set_stream then moves the slot to another stream, where
    the replace reads them.  The change of stream waits for the old one (found by `tools/fuzz.py session`: without the
    wait the replace now and then saw a half-written selection and refused it with PFAC_E_ARG)."""
    t = "mid4"
    n = X.input_size(t, 0)
    ops = load(t) + [scan(t, 0, slot=1)]
    for rnd in range(6):
        entry = rnd % 3
        ops += [pss("select", slot=1, entry=entry), dict(op="set_stream", slot=1, share=rnd % 2 == 0), pss("replace", slot=1),
                fetch("rp_fetch", slot=1, first=0, n=int(X.replace(t, 0, n, entry, "r0").size))]
    run(ops, want=[S.OK] * len(ops))


# ---------------------------------------------------------------------------
# the whole-word filter as one call among many on a long-lived context

def rp_n(t, inp, entry=0, rkey="r0", f=(), no=None):
    return int(X.replace(t, inp, X.input_size(t, inp) if no is None else no, entry, rkey, f).size)


def test_filter_in_buffers_sized_by_a_large_scan():
    """A dense 300 007-byte scan filtered to nothing (every byte is a word byte and so is prev_byte: every tile's count
    goes to 0), then 17 bytes and 64 tiles + 1 byte through filters and every pass and reader: scratch, index and
    outputs are the large call's."""
    t = "abc2"
    wipe = fkey(t, (4, ""))
    assert X.count(t, 0, 300_007, wipe) == 0 < X.count(t, 0, 300_007, fkey(t, (2, "")))
    ops = load(t) + [scan(t, 0), doc(t, 0, "d0"), pss("segment"), pss("select"), pss("replace"), fetch("text", base=0), flt(2), records(t, 0, f=fkey(t, (2, ""))),
                     flt(4), records(t, 0, f=wipe), fetch("checksum", base=0), fetch("text", base=0), pss("select_docs"), pss("replace_docs"),
                     fetch("rpd_fetch"), dict(op="scan_finish", slot=0)]
    for inp in (3, 2):
        no = X.input_size(t, inp)
        f1, f2 = fkey(t, (1, "")), fkey(t, (1, ""), (6, "d1"))
        total = len(X.text(t, inp, no, 999_999_990, f1))
        ops += [scan(t, inp), flt(1), records(t, inp, f=f1), fetch("packed"), fetch("checksum", base=999_999_990), fetch("text", base=999_999_990),
                fetch("text_fetch", first=total // 2, n=total - total // 2), dict(op="scan_finish", slot=0),
                doc(t, inp, "d1"), flt(6), records(t, inp, f=f2), pss("segment"), fetch("seg_fetch"), pss("select", entry=1), fetch("sel_fetch"),
                pss("replace"), fetch("rp_fetch", first=0, n=rp_n(t, inp, 1, f=f2)), pss("select_docs"), fetch("docsel_fetch"), fetch("seg_fetch"),
                pss("replace_docs"), fetch("rpd_fetch"), pss("segment", own=False), pss("select_docs", own=False), pss("replace_docs", own=False),
                pss("select", own=False), pss("replace", own=False)]
    st = run(ops, want=[S.OK] * len(ops))
    assert st["compared"] > 100_000


def test_scan_after_a_filter_reports_its_full_count_again():
    """Filter, every reader of the scan, then the same input scanned again on the same slot: the unfiltered count and
    records come back, from scan_bytes and from scan_start / scan_finish (whose count the filter had overwritten)."""
    for t, inp, knobs in (("abc2", 2, {}), ("mid4", 2, dict(PFAC_LAG="2"))):
        no = X.input_size(t, inp)
        f1 = fkey(t, (1, ""))
        cnt = X.count(t, inp, no)
        assert 0 < X.count(t, inp, no, f1) < cnt
        start = dict(op="scan_start", slot=0, inp=inp, no=no, cap=cnt + cnt // 4 + 65536)
        ops = load(t, **knobs) + [scan(t, inp), flt(1), dict(op="scan_finish", slot=0), records(t, inp, f=f1), records(t, inp, f=f1, n=X.count(t, inp, no, f1) + 1),
                                  fetch("packed"), fetch("checksum", base=0), fetch("text", base=0), pss("select"), pss("replace"),
                                  scan(t, inp), dict(op="scan_finish", slot=0), records(t, inp), fetch("checksum", base=0), flt(1), flt(3),
                                  start, dict(op="scan_finish", slot=0), records(t, inp), fetch("packed"), flt(2), dict(op="scan_finish", slot=0),
                                  records(t, inp, f=fkey(t, (2, ""))), start, flt(1), dict(op="scan_finish", slot=0), dict(op="scan_finish", slot=0)]
        run(ops, want=[0] * 3 + [0, 0, 0, 0, S.E_ARG] + [0] * 18 + [0, S.E_STATE, 0, 0])


def test_results_made_before_a_filter_outlive_it():
    """Segment, per-document selection, replace_docs and text, then a filter: every output is fetched unchanged, both
    replaces refuse the selection made before, and a new selection is exact.  The same for select / replace."""
    t, inp = "l2", 0
    no = X.input_size(t, inp)
    f3 = fkey(t, (3, ""))
    txt = len(X.text(t, inp, no, 0))
    E = S.E_STATE
    ops = load(t, PFAC_FORCE_L2="1") + [scan(t, inp), doc(t, inp, "d0"), pss("segment"), pss("select_docs"), pss("replace_docs"), fetch("text", base=0),
                                        flt(3), fetch("seg_fetch"), fetch("docsel_fetch"), fetch("sel_fetch"), fetch("rpd_fetch"),
                                        fetch("rp_fetch", first=0, n=int(X.docsel(t, inp, no, "d0", (), "r0")[4].size)), fetch("text_fetch", first=0, n=txt),
                                        pss("replace_docs"), pss("replace"), fetch("sel_fetch"), pss("select_docs"), fetch("docsel_fetch"), pss("replace_docs"),
                                        fetch("rp_fetch", first=0, n=int(X.docsel(t, inp, no, "d0", f3, "r0")[4].size)),
                                        pss("select", entry=2), pss("replace"), flt(1), fetch("sel_fetch"), fetch("rp_fetch", first=0, n=rp_n(t, inp, 2, f=f3)),
                                        pss("replace"), pss("replace_docs"), fetch("rp_fetch", first=0, n=1), pss("select", entry=2), fetch("sel_fetch"), pss("replace"),
                                        fetch("rp_fetch", first=0, n=rp_n(t, inp, 2, f=fkey(t, (3, ""), (1, ""))))]
    run(ops, want=[0] * 3 + [0] * 13 + [E, E, 0, 0, 0, 0, 0] + [0, 0, 0, 0, 0, E, E, E, 0, 0, 0, 0])


def test_filter_of_a_scan_into_the_callers_heap():
    """A caller's heap and a caller's input: NULL (the slot's heap) and the slot's own heap are not the scan's --
    PFAC_E_ARG, records still unfiltered; the right pointers filter exactly; an overflowed scan is PFAC_E_OVERFLOW."""
    t, inp = "mid4", 2
    no = X.input_size(t, inp)
    cnt = X.count(t, inp, no)
    f1 = fkey(t, (1, ""))
    ext = lambda cap: dict(op="scan_ext", slot=0, inp=inp, no=no, cap=cap)      # noqa: E731
    A = S.E_ARG
    ops = load(t) + [scan(t, 1), ext(cnt + cnt // 4 + 65536), flt(1, heap="none"), records(t, inp), flt(1, heap="slot"), records(t, inp), fetch("checksum", base=0),
                     flt(1), records(t, inp, f=f1), fetch("packed"), fetch("text", base=0), pss("select"), pss("replace", own=False), flt(3, heap="none"),
                     records(t, inp, f=f1), flt(3), records(t, inp, f=fkey(t, (1, ""), (3, ""))),
                     ext(cnt // 2), flt(1), flt(1, heap="none"), records(t, inp, n=1), scan(t, inp), flt(1), records(t, inp, f=f1)]
    run(ops, want=[0] * 3 + [0, 0, A, 0, A, 0, 0, 0, 0, 0, 0, 0, 0, A, 0, 0, 0, 0, S.E_OVERFLOW, S.E_OVERFLOW, S.E_OVERFLOW, 0, 0, 0])


def test_filter_across_table_changes():
    """Width 2, then 8, then 4 on one heap: the filtered records of the earlier scan stay fetchable in their width after
    an upload, while the filter is refused until the next scan AND the new table's lengths."""
    E = S.E_STATE
    a, w, m4 = fkey("abc2", (1, "")), fkey("wide8", (1, "")), fkey("mid4", (2, ""))
    up = lambda tab, **knobs: dict(op="load_table", tab=tab, knob=k(tab, **knobs))      # noqa: E731
    ops = load("abc2") + [scan("abc2", 0), flt(1), records("abc2", 0, f=a), up("wide8", PFAC_WIDE="1"), records("abc2", 0, f=a, first=5, n=1000), fetch("packed"),
                          flt(1), dict(op="set_flen"), flt(1), records("abc2", 0, f=a, n=7), scan("wide8", 1), flt(1), records("wide8", 1, f=w),
                          fetch("checksum", base=0), up("mid4"), records("wide8", 1, f=w), flt(2), scan("mid4", 2), flt(2), dict(op="set_flen"), flt(2),
                          records("mid4", 2, f=m4), fetch("packed"), dict(op="set_reps", rkey="r1"), pss("select"), pss("replace")]
    st = run(ops, want=[0] * 3 + [0, 0, 0, 0, 0, 0, E, 0, E, 0, 0, 0, 0, 0, 0, 0, E, 0, E, 0, 0, 0, 0, 0, 0, 0])
    assert st["widths"] == {2, 4, 8}


def test_filter_after_a_reserve_and_on_a_pending_scan():
    t = "mid4"
    E = S.E_STATE
    cnt = X.count(t, 2, X.input_size(t, 2))
    f1 = fkey(t, (1, ""))
    grow = lambda which, n: dict(op="reserve_grow", slot=0, which=which, k=n)      # noqa: E731
    start = dict(op="scan_start", slot=0, inp=2, no=X.input_size(t, 2), cap=cnt + cnt // 4 + 65536)
    ops = load(t) + [scan(t, 2), flt(1), grow("records", 1), flt(1), records(t, 2, f=f1, n=1), scan(t, 2), records(t, 2), flt(1), records(t, 2, f=f1),
                     grow("input", 2), flt(3), scan(t, 1), flt(3), records(t, 1, f=fkey(t, (3, ""))),
                     start, flt(1), dict(op="scan_finish", slot=0), records(t, 2), flt(1), records(t, 2, f=f1), start, grow("both", 3), flt(1),
                     dict(op="scan_finish", slot=0), scan(t, 2), flt(1), records(t, 2, f=f1)]
    run(ops, want=[0] * 3 + [0, 0, 0, E, E, 0, 0, 0, 0, 0, E, 0, 0, 0, 0, E, 0, 0, 0, 0, 0, 0, E, E, 0, 0, 0])


def test_filter_with_bad_offsets_then_good_ones_and_composition():
    """Bad offsets leave the scan alone and the next filter exact; left-with-documents and right-without compose; new
    offsets between a filter and the per-document passes; an n_docs that is not the slot's."""
    t, inp = "l2", 1
    A, E = S.E_ARG, S.E_STATE
    f5, both = fkey(t, (5, "d0")), fkey(t, (5, "d0"), (3, ""))
    ops = load(t, PFAC_FORCE_L2="1") + [scan(t, inp), flt(5), flt(10), doc(t, inp, "bad_end"), flt(5), records(t, inp), doc(t, inp, "bad_order"), flt(7),
                                        records(t, inp), fetch("checksum", base=0), doc(t, inp, "d0"), flt(10), flt(5), records(t, inp, f=f5), flt(3),
                                        records(t, inp, f=both), flt(5), records(t, inp, f=both), doc(t, inp, "d1"), pss("select_docs"),
                                        fetch("docsel_fetch"), doc(t, inp, "d0"), pss("replace_docs"), pss("select_docs"), pss("replace_docs"), fetch("rpd_fetch"),
                                        doc(t, inp, "bad_end"), flt(6), pss("segment"), doc(t, inp, "d1"), flt(6), pss("segment"), fetch("seg_fetch"),
                                        records(t, inp, f=fkey(t, (5, "d0"), (3, ""), (6, "d1")))]
    run(ops, want=[0] * 3 + [0, E, E, 0, A, 0, 0, A, 0, 0, 0, E, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, E, 0, 0, 0, 0, A, A, 0, 0, 0, 0, 0])


@pytest.mark.parametrize("share", [True, False], ids=["shared-stream", "own-streams"])
def test_two_slots_filtered_differently(share):
    """Two slots with scans of the same input under different filters, interleaved; and a change of stream between a
    filter and the selection that reads what it wrote."""
    t = "l2"
    n1 = (300_007 * 5) // 8
    fa, fb, fb2 = fkey(t, (1, "")), fkey(t, (2, "")), fkey(t, (2, ""), (3, ""))
    ops = [dict(op="set_stream", slot=1, share=share)] if share else []
    ops += load(t, PFAC_FORCE_L2="1") + [scan(t, 0, slot=0), scan(t, 0, slot=1, no=n1), flt(1, slot=0), flt(2, slot=1), records(t, 0, slot=0, f=fa),
                                         records(t, 0, slot=1, no=n1, f=fb), pss("select", slot=0), flt(3, slot=1),
                                         dict(op="set_stream", slot=1, share=not share), pss("select", slot=1, entry=X.M(t)), fetch("sel_fetch", slot=1),
                                         pss("replace", slot=0), pss("replace", slot=1), fetch("sel_fetch", slot=0),
                                         fetch("rp_fetch", slot=0, first=0, n=rp_n(t, 0, 0, f=fa)),
                                         fetch("rp_fetch", slot=1, first=0, n=rp_n(t, 0, X.M(t), f=fb2, no=n1)),
                                         dict(op="scan_finish", slot=0), dict(op="scan_finish", slot=1), fetch("checksum", slot=0, base=0),
                                         fetch("checksum", slot=1, base=999_999_990)]
    run(ops, want=[S.OK] * len(ops))


@pytest.mark.parametrize("t,inp,knobs,a,b", [("cclass", 0, {}, 1, 9), ("negcc", 0, dict(PFAC_FORCE_L2="1", PFAC_DENSE="1"), 1, 9),
                                             ("nlesc", 0, dict(PFAC_DENSE="1"), 1, 9), ("dups", 1, {}, 2, 6)], ids=["cclass", "negcc", "nlesc", "dups"])
def test_class_and_escaped_tables_through_the_filter(t, inp, knobs, a, b):
    """Multi-id final states, a record or two per byte, newline and NUL patterns, final states of length -1: filter,
    records, text, select, replace -- then a second filter with documents and the per-document passes."""
    no = X.input_size(t, inp)
    f1, f2 = fkey(t, (a, "")), fkey(t, (a, ""), (b, "d0"))
    assert 0 < X.count(t, inp, no, f2) < X.count(t, inp, no, f1) < X.count(t, inp, no)
    ops = load(t, **knobs) + [scan(t, inp), flt(a), records(t, inp, f=f1), fetch("text", base=999_999_990), fetch("checksum", base=0), pss("select"),
                              fetch("sel_fetch"), pss("replace"), fetch("rp_fetch", first=0, n=rp_n(t, inp, f=f1)), doc(t, inp, "d0"), flt(b),
                              records(t, inp, f=f2), pss("segment"), fetch("seg_fetch"), pss("select_docs"), fetch("docsel_fetch"), pss("replace_docs"),
                              fetch("rpd_fetch")]
    if S.expectations().width(t, k(t, **knobs)) != 8:
        ops.append(fetch("packed"))
    run(ops, want=[S.OK] * len(ops))


# ---------------------------------------------------------------------------
# the per-pattern counts as calls among many on a long-lived context

BINS16 = S.CKNOBS.index({"PFAC_COUNT_BINS": "16"})
A, E, O = S.E_ARG, S.E_STATE, S.E_OVERFLOW


@pytest.mark.parametrize("cknob", [0, BINS16], ids=["default", "bins16"])
def test_counts_in_buffers_sized_by_a_large_scan(cknob):
    """2 000 003 bytes, then 4097 on the same slot: the tile index, the scratch and the staging are the large scan's, longer
    than the small one; the 150 final states behind a table or behind 16 cache slots."""
    t = "mid4"
    ops = load(t, cknob=cknob) + [scan(t, 0), cnt(), cnt(dst="caller"), cnt_fetch(), scan(t, 1), cnt(), cnt(dst="caller"), cnt_fetch(),
                                  flt(1), cnt(acc=True), cnt(dst="caller", acc=True), pss("select"), cnt_sel(acc=True), cnt_sel(dst="caller"),
                                  cnt_fetch(), records(t, 1, f=fkey(t, (1, "")))]
    st = run(ops, want=[S.OK] * len(ops))
    assert st["regimes"] == {(cknob, "cache" if cknob else "direct")}


def test_counts_across_record_widths_2_8_4():
    """A count after each width; the slot's counts fetched before the next upload and once more after it, when they are
    still the old table's num_final entries."""
    up = lambda tab, **knobs: dict(op="load_table", tab=tab, knob=k(tab, **knobs), cknob=BINS16)      # noqa: E731
    ops = [up("abc2"), scan("abc2", 0), cnt(), cnt_fetch(), cnt(dst="caller"),
           up("wide8", PFAC_WIDE="1"), cnt_fetch(), cnt(acc=True), scan("wide8", 1), cnt(acc=True), cnt(), cnt(dst="caller"), cnt_fetch(),
           up("mid4"), cnt_fetch(), scan("mid4", 2), cnt(dst="caller", acc=True), cnt_fetch(), cnt(), cnt_fetch(), records("mid4", 2)]
    st = run(ops, want=[0] * 5 + [0, 0, E, 0, E, 0, 0, 0] + [0] * 8)
    assert st["widths"] == {2, 4, 8} and st["regimes"] == {(BINS16, "direct"), (BINS16, "cache")}


def test_slot_counts_across_reserve_upload_filter_and_every_pass():
    """The five passes run between a count and its fetch, slot-owned outputs each, on the same slot; then every pass's
    result is what it was, also after another count; then a filter, a reserve that drops the scan and an upload."""
    t, inp = "l2", 0
    no = X.input_size(t, inp)
    rp = fetch("rp_fetch", first=0, n=int(X.docsel(t, inp, no, "d0", (), "r0")[4].size))
    late = [fetch("seg_fetch"), fetch("docsel_fetch"), fetch("sel_fetch"), rp, fetch("rpd_fetch")]
    ops = load(t, PFAC_FORCE_L2="1") + [scan(t, inp), doc(t, inp, "d0"), cnt(), pss("segment"), pss("select"), pss("replace"), pss("select_docs"),
                                        pss("replace_docs"), cnt_fetch()] + late + [cnt_sel(acc=True), cnt(dst="caller"), cnt_fetch()] + late
    ops += [flt(1), cnt_fetch(), cnt(acc=True), dict(op="reserve_grow", slot=0, which="records", k=1), cnt_fetch(), cnt(), cnt_sel(), cnt_fetch(),
            dict(op="load_table", tab="abc2", knob=k("abc2")), cnt_fetch(), cnt(acc=True), cnt_fetch()] + late[:3]
    run(ops, want=[0] * 3 + [0] * 9 + [0] * 5 + [0] * 3 + [0] * 5 + [0, 0, 0, 0, 0, E, E, 0, 0, 0, E, 0] + [0] * 3)


def test_accumulate_over_scan_filtered_scan_and_selection():
    """The slot-owned and the caller's buffer side by side, a refused call of each kind in between: a wrong n_states, a
    misaligned d_counts, a stale selection, a foreign heap.  Both buffers are what they were after each."""
    t, inp = "mid4", 2
    no = X.input_size(t, inp)
    c = X.count(t, inp, no)
    both = lambda **kw: [cnt(acc=True, **kw), cnt(dst="caller", acc=True, **kw)]      # noqa: E731
    ops = load(t) + [scan(t, inp), cnt(), cnt(dst="caller"), cnt(ns="plus", acc=True), cnt(dst="caller", ns="minus", acc=True), cnt(dst="caller", ns="zero"),
                     cnt_fetch(), flt(1)] + both() + [cnt(dst="misaligned", acc=True), pss("select"), cnt_sel(acc=True), cnt_sel(dst="caller", acc=True), flt(3),
                     cnt_sel(acc=True), cnt_sel(dst="caller", acc=True), cnt_fetch(), dict(op="scan_ext", slot=0, inp=inp, no=no, cap=c + c // 4 + 65536)]
    ops += both(heap="none") + both(heap="slot") + [cnt_fetch()] + both() + [cnt_fetch(), records(t, inp)]
    run(ops, want=[0] * 3 + [0, 0, 0, A, A, A, 0, 0, 0, 0, A, 0, 0, 0, 0, E, E, 0, 0, A, A, A, A, 0, 0, 0, 0, 0])


@pytest.mark.parametrize("share", [True, False], ids=["shared-stream", "own-streams"])
def test_two_slots_count_while_the_other_scans(share):
    """Slot 0 has a scan pending while slot 1 counts and fetches, then the reverse; the counts never leak between slots."""
    t = "l2"
    c = X.count(t, 0, 300_007)
    start = lambda slot: dict(op="scan_start", slot=slot, inp=0, no=300_007, cap=c + c // 4 + 65536)      # noqa: E731
    fin = lambda slot: dict(op="scan_finish", slot=slot)      # noqa: E731
    ops = [dict(op="set_stream", slot=1, share=True)] if share else []
    ops += load(t, PFAC_FORCE_L2="1") + [scan(t, 1, slot=1), start(0), cnt(slot=1), cnt_fetch(slot=1), cnt(slot=0), cnt_fetch(slot=0), cnt(slot=1, dst="caller"),
                                         fin(0), cnt(slot=0), cnt(slot=0, dst="caller"), start(1), cnt(slot=1, acc=True), cnt(slot=0, acc=True), cnt_fetch(slot=0),
                                         cnt_fetch(slot=1), fin(1), cnt(slot=1, acc=True), cnt(slot=1, dst="caller", acc=True), cnt_fetch(slot=1), cnt_fetch(slot=0),
                                         records(t, 0, slot=0), records(t, 0, slot=1)]
    run(ops, want=[0] * (4 if share else 3) + [0, 0, 0, 0, E, E, 0, 0, 0, 0, 0, E, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def test_counts_of_a_scan_into_the_callers_heap():
    """The right pointer counts; NULL and the slot's own heap are not the scan's (PFAC_E_ARG); an overflowed rescan is
    PFAC_E_OVERFLOW whatever the arguments; the counts made before survive."""
    t, inp = "mid4", 2
    no = X.input_size(t, inp)
    c = X.count(t, inp, no)
    ext = lambda cap: dict(op="scan_ext", slot=0, inp=inp, no=no, cap=cap)      # noqa: E731
    ops = load(t) + [scan(t, 1), cnt(), ext(c + c // 4 + 65536), cnt(acc=True), cnt(dst="caller"), cnt(heap="none"), cnt(dst="caller", heap="slot", acc=True),
                     cnt_fetch(), flt(1), cnt(dst="caller", acc=True), ext(c // 2), cnt(), cnt(dst="caller", acc=True), cnt(heap="none", ns="plus"), cnt_fetch(),
                     scan(t, inp), cnt(acc=True), cnt_fetch()]
    run(ops, want=[0] * 3 + [0, 0, 0, 0, 0, A, A, 0, 0, 0, 0, O, O, O, 0, 0, 0, 0])


def test_selection_counts_as_calls_in_a_session():
    """The selection in the caller's d_out; a failed select into a too-small d_out leaves no selection to count (the
    earlier one's buffer included); a per-document selection is still counted after new offsets, which end only the
    per-document replace's right to it."""
    t, inp = "l2", 1
    small = dict(op="select", slot=0, own=False, small=True, entry=0)
    assert X.sel(t, inp, X.input_size(t, inp), 0)[0].size > 1
    ops = load(t, PFAC_FORCE_L2="1") + [scan(t, inp), cnt_sel(), pss("select", own=False), cnt_sel(sel="caller"), cnt_sel(sel="own"), cnt_sel(sel="junk", acc=True),
                                        cnt_sel(sel="misaligned"), cnt_sel(sel="caller", dst="caller"), cnt_fetch(), small, cnt_sel(sel="caller"), cnt_sel(sel="own"),
                                        cnt_fetch(), doc(t, inp, "d0"), pss("select_docs"), cnt_sel(acc=True), doc(t, inp, "d1"), cnt_sel(acc=True),
                                        cnt_sel(dst="caller", acc=True), pss("replace_docs"), cnt_fetch(), fetch("docsel_fetch")]
    run(ops, want=[0] * 3 + [0, E, 0, 0, E, A, A, 0, 0, O, E, E, 0, 0, 0, 0, 0, 0, 0, E, 0, 0])


@pytest.mark.parametrize("t,inp,knobs", [("cclass", 0, {}), ("negcc", 0, dict(PFAC_FORCE_L2="1", PFAC_DENSE="1")), ("nlesc", 0, dict(PFAC_DENSE="1"))],
                         ids=["cclass", "negcc", "nlesc"])
def test_class_and_escaped_tables_counted_by_id(t, inp, knobs):
    """Final states that stand for several patterns, a record or two per byte, newline and NUL patterns: the scan's, the
    filtered scan's and both selections' counts, compared by pattern id."""
    ops = load(t, cknob=1, **knobs) + [scan(t, inp), cnt(), cnt(dst="caller"), cnt_fetch(), pss("select"), cnt_sel(acc=True), cnt_sel(dst="caller", acc=True),
                                       flt(1), cnt(acc=True), cnt_fetch(), doc(t, inp, "d0"), pss("select_docs", own=False), cnt_sel(sel="caller"),
                                       cnt_sel(sel="caller", dst="caller"), cnt_fetch()]
    st = run(ops, want=[S.OK] * len(ops))
    assert st["regimes"] == {(1, "cache")}


def test_same_table_uploaded_twice_is_a_new_generation():
    """An accumulate onto the slot's counts of the upload before is PFAC_E_STATE, onto the caller's buffer it is allowed."""
    t = "dups"
    ops = load(t) + [scan(t, 0), cnt(), cnt(dst="caller")] + load(t) + [cnt_fetch(), cnt(acc=True), scan(t, 1), cnt(acc=True), cnt(dst="caller", acc=True),
                                                                        cnt_fetch(), cnt_sel(acc=True), cnt(), cnt(acc=True), cnt_fetch()]
    run(ops, want=[0] * 3 + [0, 0, 0] + [0] * 3 + [0, E, 0, E, 0, 0, E, 0, 0, 0])


# ---------------------------------------------------------------------------
# the line path as calls on a long-lived context: split, matching documents, context lines, gather

def spl(tab, inp, slot=0, nb=None, which=0, src="slot", delim=None):
    """A split of input `inp`; which: 0 = at its most frequent byte, 1 = at its rarest, 2 = at a byte that does not occur."""
    return dict(op="split", slot=slot, src=src, tab=tab, inp=inp, nb=X.input_size(tab, inp) if nb is None else nb,
                delim=X.delims(tab, inp)[which] if delim is None else delim)


def mat(slot=0, first="own", out="own", flags=0, ctx=None, nd="ok"):
    return dict(S._matching_op(slot, first=first, out=out, flags=flags, context=ctx), nd=nd)


def gat(tab, inp, slot=0, nb=None, **kw):
    op = dict(op="gather", slot=slot, src="slot", tab=tab, inp=inp, nb=X.input_size(tab, inp) if nb is None else nb, off="slot", nd="ok", ids="own",
              ni="ok", out="own", oo="own")
    op.update(kw)
    return op


def whole(ops):
    """The operations with every doc_fetch / ga_fetch that has no window yet asking for all there is at that point."""
    m, out = S.Model(), []
    for op in ops:
        s = m.slots[op.get("slot", 0)]
        if op["op"] == "doc_fetch" and "n" not in op:
            op = dict(op, first=0, n=int(X.offsets(*s.doc).size))
        if op["op"] == "ga_fetch" and "n" not in op:
            op = dict(op, first=0, n=int(X.gather(*s.ga[0])[0].size))
        m.apply(op)
        out.append(op)
    return out


def test_large_lines_then_tiny_lines():
    """Split and gather of the largest pool input at its most frequent byte, then of a 17-byte input, then matching,
    context and gather: the per-tile arrays, group sums, offsets, ids and outputs are sized by the large call, and nothing
    of it may show in the small one."""
    big, t = "mid4", "abc2"
    ops = load(big) + [scan(big, 0), spl(big, 0), fetch("doc_fetch"), pss("segment"), mat(), gat(big, 0), fetch("ga_fetch"), fetch("gaoff_fetch")]
    ops += load(t) + [scan(t, 3), spl(t, 3), fetch("doc_fetch"), gat(t, 3, ids="all"), fetch("ga_fetch"), fetch("gaoff_fetch"), pss("segment"), mat(),
                      fetch("ids_fetch"), mat(ctx=(1, 1)), fetch("ids_fetch"), gat(t, 3), fetch("ga_fetch"), fetch("gaoff_fetch"),
                      mat(flags=1, out="caller"), gat(t, 3, ids="rev", out="caller", oo="caller"), spl(t, 3, which=2), fetch("doc_fetch")]
    ops = whole(ops)
    st = run(ops, want=[S.OK] * len(ops))
    print(f"large lines, then tiny ones: {st['compared']} bytes and {st['ids']} document ids and offsets compared")
    assert st["splits"] == 3 and st["gathers"] == 4 and st["compared"] > 2_000_000


def test_slot_buffers_regrow_behind_a_queued_gather():
    """A gather with everything slot-owned returns before its bytes are written; the very next call makes the slot's
    offsets buffer (set_doc with more documents, then a split into many), or its ids (a matching call over many more
    documents), outgrow their allocation.  The gather's output, fetched afterwards, is that of the old offsets and ids."""
    t = "abc2"
    first = [scan(t, 0), spl(t, 0, which=2), pss("segment"), mat(flags=1), gat(t, 0)]             # one document without a delimiter, reported by invert
    late = [fetch("ga_fetch"), fetch("gaoff_fetch")]
    ops = load(t) + first + [doc(t, 0, "d1")] + late
    ops += [spl(t, 0, which=2), gat(t, 0, ids="all"), spl(t, 0)] + late + [fetch("doc_fetch")]
    ops += [doc(t, 0, "d0"), pss("segment"), mat(), gat(t, 0), spl(t, 0), pss("segment"), mat(ctx=(1, 1))] + late + [fetch("ids_fetch"), gat(t, 0)] + late
    ops = whole(ops)
    st = run(ops, want=[S.OK] * len(ops))
    assert st["gathers"] == 4


def test_stream_change_between_matching_and_its_gather():
    """The ids of a matching call are written asynchronously on the slot's stream; set_stream moves the slot to another
    stream, where the gather reads them through NULL.  The line-path twin of the selection and its replace above."""
    t = "mid4"
    ops = load(t) + [scan(t, 0, slot=1), spl(t, 0, slot=1), pss("segment", slot=1)]
    for rnd in range(6):
        ops += [mat(slot=1, flags=rnd % 2) if rnd % 3 else mat(slot=1, ctx=(rnd, 1)), dict(op="set_stream", slot=1, share=rnd % 2 == 0),
                gat(t, 0, slot=1), fetch("ga_fetch", slot=1), fetch("gaoff_fetch", slot=1)]
    ops = whole(ops)
    run(ops, want=[S.OK] * len(ops))


def test_matching_and_context_are_one_pass():
    """The two calls share one id buffer and one fetch: each replaces the other's ids, a refused call of either discards
    them, ids that went to the caller cannot be fetched, and an overflow carries the exact count."""
    t = "abc2"
    E, A, V = S.E_STATE, S.E_ARG, S.E_OVERFLOW
    ops = load(t) + [scan(t, 2), doc(t, 2, "d0"), pss("segment"),
                     mat(), fetch("ids_fetch"), mat(ctx=(1, 0)), fetch("ids_fetch"), mat(flags=1), fetch("ids_fetch"),
                     mat(flags=2), fetch("ids_fetch"), mat(ctx=(0, 1)), mat(ctx=(0, 1), flags=1), fetch("ids_fetch"),
                     mat(), mat(ctx=(2, 3), out="small"), fetch("ids_fetch"), mat(ctx=(S.U64_MAX, 0)), mat(nd="plus"), fetch("ids_fetch"),
                     mat(out="caller"), fetch("ids_fetch"), mat(ctx=(0, 0), out="caller"), fetch("ids_fetch"), mat(ctx=(0, 0)), fetch("ids_fetch"),
                     mat(out="odd"), gat(t, 2), mat(flags=1), gat(t, 2), fetch("ga_fetch"), fetch("gaoff_fetch")]
    ops = whole(ops)
    run(ops, want=[0] * 3 + [0, 0, 0] + [0, 0, 0, 0, 0, 0] + [A, E, 0, A, E] + [0, V, E, 0, A, E] + [0, E, 0, E, 0, 0] + [A, E, 0, 0, 0, 0])


def test_a_chunked_reader_carries_the_tail_over():
    """tail_start is what a chunked reader carries over: three chunks of one pool input cut at arbitrary places, each
    uploaded behind the unterminated rest of the one before, split, and its complete lines gathered.  The offsets and the
    gathered bytes of the chunks, put together, are those of one split of the whole input (splitref, gatherref)."""
    import torch
    from gatherref import gather_ref
    from splitref import split_offsets
    t = "abc2"
    data = X.input(t, 0)
    delim = X.delims(t, 0)[1]
    want_off, want_docs, want_tail = split_offsets(data, delim)
    assert want_docs > 64 * 64 and want_tail != data.size, "the input must end in an unterminated line"
    cuts = [0, 100_003, 100_003 + 131_072 + 5, data.size]
    offsets, pieces, carry, base = [np.zeros(1, np.uint64)], [], data[:0], 0
    with GpuMatcher(0, 1) as g:
        g.reserve(0, data.size, 4096)
        for a, b in zip(cuts[:-1], cuts[1:]):
            buf = np.concatenate([carry, data[a:b]])
            g.h2d(buf, 0)
            n_docs, tail = g.split_documents(buf.size, delim)
            last = b == data.size
            n_lines = n_docs if last or tail == buf.size else n_docs - 1      # the unterminated rest waits for the next chunk
            off = g.doc_offsets_to_host(n_docs)
            ids = torch.arange(max(n_lines, 1), dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            n = g.gather_documents(n_docs, n_lines, buf.size, d_ids=ids.data_ptr())
            pieces.append(g.gathered_to_host(n))
            assert n == int(off[n_lines])
            offsets.append(off[1:n_lines + 1] + np.uint64(base))
            carry = buf[int(off[n_lines]):].copy()
            assert last or carry.size == buf.size - tail
            base += int(off[n_lines])
            g.sync(0)
    np.testing.assert_array_equal(np.concatenate(offsets), want_off)
    want, _ = gather_ref(data, want_off, np.arange(want_docs, dtype=np.uint64))
    np.testing.assert_array_equal(np.concatenate(pieces), want)


# ---------------------------------------------------------------------------
# the case fold as a setting on a long-lived context: it belongs to the uploaded table, is fixed for a scan when the scan
# is queued, and no pass behind a folded scan sees a folded byte

def fold(mode):
    return dict(op="set_fold", mode=mode)


GET = dict(op="get_fold")


def filled(ops):
    """The operations with every records / rp_fetch / ga_fetch that has no window yet asking for all there is at that point."""
    m, out = S.Model(), []
    for op in ops:
        s = m.slots[op.get("slot", 0)]
        if "n" not in op and op["op"] == "records":
            op = dict(op, first=0, n=m._count(s.scan))
        if "n" not in op and op["op"] == "rp_fetch":
            op = dict(op, first=0, n=int(s.rp["out"]().size))
        if "n" not in op and op["op"] == "ga_fetch":
            op = dict(op, first=0, n=int(X.gather(*s.ga[0])[0].size))
        m.apply(op)
        out.append(op)
    return out


def ok(ops):
    return run(ops, want=[S.OK] * len(ops))


def test_staging_layout_flips_both_ways_folded():
    """test_staging_layout_flips_both_ways_with_exact_records with the fold on throughout: wordsi with no knob pinned, its
    dense input (a record every other byte once folded) and its matchless one in turn -- the twin of whichever kernel
    the staging mode picks is the one that runs.  Then the old-table case: negcc's record-heavy input under the fold, with
    no knob pinned and in dense mode."""
    t = "wordsi"
    seen, folded = [], 0
    with GpuMatcher(0, S.N_SLOTS) as g:
        ex = S.Executor(g, S.Model())
        for op in load(t):
            ex.step(op)
        seen.append(g.info()["staging_buffers"])
        for rnd, inp in enumerate((0, 1, 0, 0, 1, 1, 0, 1)):
            ex.step(GET)
            ex.step(scan(t, inp, slot=rnd % 2))
            assert ex.m.slots[rnd % 2].scan["fold"]
            seen.append(g.info()["staging_buffers"])
            ex.step(dict(op="records", slot=rnd % 2, first=0, n=X.count(t, inp, 300_007, (), True)))
            ex.step(fetch("checksum", slot=rnd % 2, base=0))
        folded = ex.stats["folded"]
        for knobs in ({}, dict(PFAC_DENSE="1")):
            for op in filled(load("negcc", **knobs) + [fold(1), scan("negcc", 1), dict(op="records", slot=0), fetch("packed"), fetch("text", base=0)]):
                ex.step(op)
    to_dense = sum(a != 1 and b == 1 for a, b in zip(seen, seen[1:]))
    from_dense = sum(a == 1 and b != 1 for a, b in zip(seen, seen[1:]))
    assert to_dense >= 1 and from_dense >= 1 and folded == 8, (seen, folded)
    assert X.count("negcc", 1, 70_001, (), True) > 70_001 and X.fold_differs("negcc", 1)


def test_record_width_2_then_8_then_4_on_one_heap_fold_on():
    """test_record_width_2_then_8_then_4_on_one_heap with every scan folded: wordsi (two-byte records, the fold on from
    its upload), wide8 and mid4 (eight and four bytes, the fold set by hand after each upload)."""
    E = S.E_STATE
    ops = load("wordsi") + [GET, scan("wordsi", 0), dict(op="records", slot=0), pss("select")]
    ops += load("wide8", PFAC_WIDE="1") + [GET, fold(1), dict(op="records", slot=0, first=5, n=1000), fetch("packed"), fetch("checksum", base=0),
                                            fetch("text", base=0), pss("select"), pss("replace"), fetch("sel_fetch"),
                                            scan("wide8", 3), dict(op="records", slot=0), fetch("packed"), fetch("checksum", base=0), pss("select")]
    ops += load("mid4") + [fold(1), dict(op="records", slot=0), pss("segment"), scan("mid4", 1), dict(op="records", slot=0), fetch("packed"), pss("select"),
                           fetch("sel_fetch"), pss("replace"), dict(op="rp_fetch", slot=0)]
    st = run(filled(ops), want=[0] * 3 + [0, 0, 0, 0] + [0] * 3 + [0, 0, 0, 0, E, E, E, E, E, 0, 0, E, 0, 0] + [0] * 3 + [0, 0, E, 0, 0, 0, 0, 0, 0, 0])
    assert st["widths"] == {2, 4, 8} and st["folded"] == 3
    assert X.fold_differs("wide8", 3) and X.fold_differs("mid4", 1)


@pytest.mark.parametrize("share", [True, False], ids=["shared-stream", "own-streams"])
def test_toggle_between_two_slots_queued_scans(share):
    """Fold on, scan_start on slot 0; fold off, scan_start on slot 1; fold on again; then both finishes: each scan keeps the
    mode it was queued with, and the filter (which judges the bytes as written), the selection, the replace and the count
    behind each are those of ITS scan."""
    t, inp = "wordsi", 2
    no = X.input_size(t, inp)
    cf, ce = X.count(t, inp, no, (), True), X.count(t, inp, no)
    assert cf > ce > 0
    start = lambda slot, c: dict(op="scan_start", slot=slot, inp=inp, no=no, cap=c + c // 4 + 65536)      # noqa: E731
    ops = [dict(op="set_stream", slot=1, share=True)] if share else []
    ops += load(t, rkey="redact") + [GET, start(0, cf), fold(0), start(1, ce), fold(1), GET, dict(op="scan_finish", slot=0), dict(op="scan_finish", slot=1)]
    for slot in (0, 1):
        ops += [dict(op="records", slot=slot), flt(1, slot=slot), dict(op="records", slot=slot), pss("select", slot=slot), fetch("sel_fetch", slot=slot),
                pss("replace", slot=slot), dict(op="rp_fetch", slot=slot), cnt(slot=slot), cnt_fetch(slot=slot), cnt(slot=slot, dst="caller")]
    ops = filled(ops)
    probe = S.Model()
    for op in ops:
        probe.apply(op)
    assert probe.slots[0].scan["fold"] and not probe.slots[1].scan["fold"] and probe.fold
    f1 = fkey(t, (1, ""))
    assert 0 < X.count(t, inp, no, f1) < ce and X.count(t, inp, no, f1) < X.count(t, inp, no, f1, True) < cf
    st = ok(ops)
    assert st["folded"] == 1 and st["toggles"] == 2


def test_an_upload_resets_the_fold_and_the_folded_records_survive():
    """A folded scan, then the same table's image uploaded again by pfac_table_upload_device alone: the fold reads off,
    the next scan is exact; the first scan's records are still the folded ones (records, packed), while its text and a
    selection from it need the table it was scanned with: PFAC_E_STATE."""
    t, E = "wordsi", S.E_STATE
    again = dict(op="load_table", tab=t, knob=k(t), via="device")
    ops = load(t) + [GET, scan(t, 0, slot=0), again, GET, dict(op="set_flen"), scan(t, 0, slot=1), dict(op="records", slot=1), dict(op="records", slot=0),
                     fetch("packed", slot=0), fetch("text", slot=0, base=0), pss("select", slot=0), fetch("checksum", slot=1, base=0)]
    st = run(filled(ops), want=[0] * 3 + [0, 0, 0, 0, 0, 0, 0, 0, 0, E, E, 0])
    assert st["folded"] == 1 and X.count(t, 0, 300_007, (), True) > X.count(t, 0, 300_007)


def test_a_word_set_that_separates_the_cases_sees_the_input_as_written():
    """wordsi, a folded scan, the filter with the lower-case letters as the word set: an upper-case neighbour is no word
    byte, so the kept set is the one wordref gives on the ORIGINAL bytes and not the one on folded bytes; the selection's
    replace and the per-document one copy the original bytes around their picks."""
    import wordref
    t, inp = "wordsi", 2
    no = X.input_size(t, inp)
    f1 = fkey(t, (1, ""))
    pos, ids, lens = X.scan(t, inp, no, (), True)
    bits = np.zeros(4, dtype=np.uint64)
    for b in S.WORD_TAB[t]:
        bits[b >> 6] |= np.uint64(1 << (b & 63))
    on_folded = wordref.filter_words(S.nocaseref.fold(X.input(t, inp)), pos, lens, bits, wordref.BOTH, -1, -1, None)
    kept = X.scan(t, inp, no, f1, True)[0]
    assert 0 < int(on_folded.sum()) < kept.size < pos.size, "the word set does not separate the cases on this input"
    out = X.replace(t, inp, no, 0, "redact", f1, True)
    spos, sids, _ = X.sel(t, inp, no, 0, f1, True)
    outside = np.ones(no, dtype=bool)
    for p, n in zip(spos.tolist(), X.tinfo(t)["ll"][sids].tolist()):
        outside[p:p + n] = False
    assert out.size == no and np.array_equal(out[outside], X.input(t, inp)[:no][outside]) and (out[~outside] == ord("#")).all()
    assert (X.input(t, inp)[:no][outside] != S.nocaseref.fold(X.input(t, inp)[:no])[outside]).any()
    ops = load(t, rkey="redact") + [scan(t, inp), flt(1), dict(op="records", slot=0), pss("select"), fetch("sel_fetch"), pss("replace"),
                                    dict(op="rp_fetch", slot=0), doc(t, inp, "d0"), pss("select_docs"), fetch("docsel_fetch"), pss("replace_docs"),
                                    dict(op="rp_fetch", slot=0), fetch("rpd_fetch"), pss("replace_docs", own=False), pss("replace", own=False)]
    ok(filled(ops))


def test_folded_scan_of_the_callers_guarded_buffers():
    """A folded scan reads the caller's input between guard bands, odd-aligned by 16 bytes into its tensor, and writes the
    caller's heap at exactly the capacity the hint names: the records are the folded ones, and neither the guard bands
    nor one byte of the input have changed afterwards (the fold happens on the way into the kernel's on-chip copy)."""
    import torch
    from heapguard import GuardedBuffer
    t, inp = "wordsi", 2
    data = X.input(t, inp)
    no = data.size
    pos, ids, _ = X.scan(t, inp, no, (), True)
    with GpuMatcher(0, 1) as g:
        g.load_table(X.table(t))
        assert g.case_fold
        d_in = GuardedBuffer(no, front=4096 + 16, fill=0xA5)
        d_in.payload().copy_(torch.from_numpy(data))
        torch.cuda.synchronize()
        roomy = GuardedBuffer(4 << 20)                          # (a roomy heap first, for the hint)
        g.scan_async(no, no, d_input=d_in.ptr, d_records=roomy.ptr, capacity=(4 << 20) // 8, slot=0)
        n, over = g.scan_finish(0, allow_overflow=True)
        cap = int(g.capacity_hint(0))
        heap = GuardedBuffer(cap * g.scan_format(0)[0], fill=0x3C)
        g.scan_async(no, no, d_input=d_in.ptr, d_records=heap.ptr, capacity=cap, slot=0)
        n, over = g.scan_finish(0, allow_overflow=True)
        assert (n, over) == (pos.size, False)
        rec = g.records_to_host(n, 0, d_records=heap.ptr)
        g.sync(0)
        heap.check(what="the caller's heap of a folded scan")
        d_in.check(what="the caller's input of a folded scan")
        np.testing.assert_array_equal(d_in.host(), data)
    np.testing.assert_array_equal(rec["pos"].astype(np.int64), pos)
    np.testing.assert_array_equal(np.asarray(X.table(t).idmap)[rec["state"]], ids)


@pytest.mark.parametrize("t,knob", [(t, kn) for t in ("cclassi", "root1i") for kn in S.FOLD_TABLES[t]["knobs"]],
                         ids=[f"{t}-{knob_label(S.KNOBS[kn])}" for t in ("cclassi", "root1i") for kn in S.FOLD_TABLES[t]["knobs"]])
def test_class_and_one_edge_root_tables_through_the_fold(t, knob):
    """from_charclass(..., ignore_case=True) and the root with ONE edge, folded on a GPU under each of their knobs: the
    scan, its counts by pattern id, the matching lines with one line of context each side, and their bytes -- in the case
    they were written in."""
    inp = 0
    no = X.input_size(t, inp)
    assert X.fold_differs(t, inp)
    ops = [dict(op="load_table", tab=t, knob=knob, cknob=0), dict(op="set_flen"), GET, scan(t, inp), dict(op="records", slot=0), cnt(), cnt_fetch(),
           cnt(dst="caller"), spl(t, inp, which=0), pss("segment"), mat(), fetch("ids_fetch"), mat(ctx=(1, 1)), fetch("ids_fetch"), gat(t, inp),
           dict(op="ga_fetch", slot=0), fetch("gaoff_fetch")]
    ops = filled(ops)
    probe = S.Model()
    for op in ops:
        probe.apply(op)
    out = X.gather(*probe.slots[0].ga[0])[0]
    assert out.size and (out != S.nocaseref.fold(out)).any(), "the gathered lines hold no upper-case letter"
    st = ok(ops)
    assert st["folded"] == 1 and st["gathers"] == 1
