"""The three post-scan passes -- documents (pfac_records_segment), leftmost-longest selection
(pfac_records_leftmost_longest) and find-and-replace (pfac_replace_leftmost_longest) -- on seeded random automata under
every kernel knob set of tools/fuzz.py, and on the paths inside them that fixed files do not reach: chunked compose and
walk of the selection's functions (max_pat_len 1022, more than 16 groups / more than 1024 groups), replacements longer
than an output window, tables at the 64-final-state register boundary, tiles at the 63-document-start window boundary.
Run with -m gpu on an MI355X.  Expectations come from the CPU oracle, tests/llref.py, tests/replref.py,
tests/docref.py and the pattern files -- never from the device or PfacTable.final_lengths.  Bit-exact."""
import numpy as np
import pytest

from docref import oracle_per_doc, random_offsets
from llref import check_greedy, greedy, line_lengths
from orc import Oracle, ac_whole_shard
from passfuzz import GROUP, KNOB_NAMES, KNOBS, SEEDS, TILE, Case, knob_label, record_width, run_case
from phfpfac_amd import GpuMatcher, PfacTable
from phfpfac_amd import _ffi
from phfpfac_amd.matcher import tiled_bytes
from replref import re_replace, rep_table, splice

pytestmark = pytest.mark.gpu

LL_CHUNK_U16 = 16384                         # u16 entries the compose / walk kernels stage at a time


def set_knobs(monkeypatch, knobs):
    for k in KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def write_patterns(tmp_path, pats, name="p.pat"):
    f = tmp_path / name
    f.write_bytes(b"".join(p + b"\n" for p in pats))
    return str(f)


def oracle_records(path, data, n_owned=None):
    o = Oracle(path, 1, 1)
    pos, ids = o.scan_spec(np.ascontiguousarray(data))
    o.close()
    if n_owned is not None:
        keep = pos < n_owned
        pos, ids = pos[keep], ids[keep]
    return pos, ids


def chain(g, table, data, cuts, entry):
    """The selection of the owned ranges [cuts[i], cuts[i + 1]) in turn, each with a halo of max_pat_len - 1 bytes and
    the previous call's exit as its entry -> (pos, pattern ids, exit)."""
    pos, ids = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        rec, entry = g.scan_leftmost_longest(np.ascontiguousarray(data[a:min(b + table.halo, data.size)]), b - a, entry)
        pos.append(rec["pos"].astype(np.int64) + a)
        ids.append(table.idmap[rec["state"]])
    return np.concatenate(pos), np.concatenate(ids), entry


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS, ids=[f"s{s}-{knob_label(KNOBS[s % len(KNOBS)])}" for s in SEEDS])
def test_passes_fuzz(seed, monkeypatch, tmp_path):
    """One random case (tests/passfuzz.py): scan twice, then selection, replace, documents and a chained selection."""
    case = Case(seed)
    set_knobs(monkeypatch, case.knobs)
    n = run_case(lambda: GpuMatcher(0, 1), case, str(tmp_path))
    print(f"case {case.describe()}: {n} records compared")


# ---------------------------------------------------------------------------
def max_length_set(tmp_path):
    """One pattern of exactly 1022 bytes, forty of 700 to 1 000 cut from a random base string, and short ones; the
    input is tiled from the base, so long picks cross tile and group boundaries."""
    rng = np.random.default_rng(1022)
    base = rng.integers(97, 101, 3001).astype(np.uint8)          # a..d
    pats = [base[:1022].tobytes()]
    for _ in range(40):
        L = int(rng.integers(700, 1001))
        s = int(rng.integers(0, base.size - L))
        pats.append(base[s:s + L].tobytes())
    pats += [b"bd", b"abca", b"dcb"]
    return write_patterns(tmp_path, pats), base.tobytes()


def chunk_counts(n, M):
    """(n_groups, nb, nfc) of a selection over n owned bytes with max_pat_len M (the host side of the selection)."""
    n_groups = -(-(-(-n // TILE)) // 64)
    return n_groups, -(-n_groups // 64), LL_CHUNK_U16 // ((M + 1 + 7) & ~7)


@pytest.mark.parametrize("n", [(8 << 20) + 4097, (300 << 20) + 777], ids=["8MiB-compose-chunks", "300MiB-walk-chunks"])
def test_max_length_pattern_chunked_compose_and_walk(n, tmp_path):
    """max_pat_len 1022: 1 024-entry functions, 16 staged per chunk.  8 MiB has 33 groups (compose runs three chunks;
    with one block its result is the exit, so the owned range ends inside a long pick), 300 MiB has 1 200 groups in 19
    blocks (every block's entry comes from four composed chunks, and the walk over the blocks runs two chunks).  The
    scan is pinned against one serial Aho-Corasick pass (count + checksum), every selection against all its records by
    check_greedy, the replace output against splice; chained calls cut at group edges +- 1 equal the one-shot
    selection."""
    import torch
    path, base = max_length_set(tmp_path)
    ll = line_lengths(path)
    table = PfacTable.from_file(path, 256)
    assert table.max_pat_len == 1022
    n_owned = n - 2000
    n_groups, nb, nfc = chunk_counts(n_owned, 1022)
    print(f"n_owned {n_owned}: n_groups {n_groups}, nb {nb}, nfc {nfc}")
    assert min(n_groups, 64) > nfc                              # compose: block 0 stages more than one chunk
    if n > 256 << 20:
        assert nb > nfc                                         # walk over the blocks: more than one chunk
    rng = np.random.default_rng(5)
    reps = {i: rng.integers(0, 256, int(rng.integers(0, 40))).astype(np.uint8).tobytes() for i in range(1, ll.size)}
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_replacements(reps)
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, base)
        g.reserve(0, 0, n // 8)
        total = g.scan_resident(n_owned, n, d_input=buf)
        chk = g.checksum(total)
        whole = g.records_to_host(total)
        sels, outs = {}, {}
        for entry in (0, 1, 1022):
            n_sel, ex = g.select_leftmost_longest(entry)
            sels[entry] = (g.selection_to_host(n_sel), ex)
            if entry == 1022 or n < 64 << 20:
                outs[entry] = g.replacement_to_host(g.replace_selection(d_input=buf))
        host = buf[:n].cpu().numpy()
        del buf
        torch.cuda.empty_cache()
        cuts = [0, 5 * GROUP - 1, 16 * GROUP, 17 * GROUP + 1, n_owned] if n < 64 << 20 else \
            [0, 1024 * GROUP - 1, 1024 * GROUP + 1, n_owned]
        cpos, cids, cex = chain(g, table, host, cuts, 1)
    assert (total, chk) == ac_whole_shard(path, host, n_owned)
    wpos = whole["pos"].astype(np.int64)
    lens = ll[table.idmap[whole["state"]]]
    del whole
    for entry, (sel, ex) in sels.items():
        spos, sids = sel["pos"].astype(np.int64), table.idmap[sel["state"]]
        assert check_greedy(wpos, lens, (spos, ll[sids]), entry, n_owned) == ex, entry
        assert 0 < spos.size < total and (ll[sids] >= 700).any() and ex > 0
        if entry == 1:
            np.testing.assert_array_equal(cpos, spos)
            np.testing.assert_array_equal(cids, sids)
            assert cex == ex
        if entry in outs:
            want = splice(host, entry, n_owned, spos, ll[sids], sids, rep_table(reps))
            assert outs[entry].size == want.size and np.array_equal(outs[entry], want), entry


@pytest.mark.parametrize("M", [1, 2])
def test_single_byte_patterns_every_record_a_pick(M, tmp_path):
    """max_pat_len 1 (every record is a pick) and 2; 3 MiB over more than ten groups, chained at group edges +- 1."""
    pats = [b"a", b"c", b"a"] if M == 1 else [b"a", b"ab", b"ba", b"c", b"ab"]
    path = write_patterns(tmp_path, pats)
    table = PfacTable.from_file(path, 256)
    assert table.max_pat_len == M
    rng = np.random.default_rng(M)
    data = np.frombuffer(b"abcd", dtype=np.uint8)[rng.integers(0, 4, (3 << 20) + 5)]
    reps = [b"", b"\x00\xff", b"", b"XYZ", b"Q"][:len(pats)]
    ll = line_lengths(path)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_replacements(reps)
        for n_owned in (data.size, data.size - 1):
            pos, ids = oracle_records(path, data, n_owned)
            for entry in range(M + 1):
                rec, ex = g.scan_leftmost_longest(data, n_owned, entry)
                sel, wex = greedy(pos, ll[ids], entry, n_owned)
                if M == 1:
                    assert sel.size == int((pos >= entry).sum())
                np.testing.assert_array_equal(rec["pos"].astype(np.int64), pos[sel])
                np.testing.assert_array_equal(table.idmap[rec["state"]], ids[sel])
                assert ex == wex
                out, ex = g.replace(data, n_owned, entry)
                want = splice(data, entry, n_owned, pos[sel], ll[ids[sel]], ids[sel], rep_table(reps))
                assert np.array_equal(out, want) and ex == wex
                assert np.array_equal(out, re_replace(pats, reps, data, entry, n_owned)[0])
        whole, wex = g.scan_leftmost_longest(data, entry=M)
        cpos, cids, cex = chain(g, table, data, [0, GROUP - 1, 2 * GROUP, 7 * GROUP + 1, data.size], M)
    np.testing.assert_array_equal(cpos, whole["pos"].astype(np.int64))
    np.testing.assert_array_equal(cids, table.idmap[whole["state"]])
    assert cex == wex


# ---------------------------------------------------------------------------
LONG_REPS = {1: 1023, 2: 1024, 3: 1025, 4: 65536, 5: 0, 6: 0, 7: 3}


@pytest.mark.parametrize("big", [False, True], ids=["below-64MiB", "above-64MiB"])
def test_long_replacements(big, tmp_path):
    """Replacements of 1 023, 1 024, 1 025 and exactly 65 536 bytes (holding 0x00 and 0xFF), so windows lie wholly
    inside one replacement and one 64-pick block spans thousands of windows; runs of deletions between them make
    blocks with no output at all.  Outputs below and above 64 MiB: one and four windows per wave."""
    pats = [b"Q1", b"Q22", b"Q333", b"Q4444", b"zz", b"yyy", b"Q"]
    path = write_patterns(tmp_path, pats)
    rng = np.random.default_rng(7 + big)
    reps = {}
    for i, L in LONG_REPS.items():
        r = rng.integers(0, 256, L).astype(np.uint8)
        if L:
            r[0], r[-1] = 0x00, 0xFF
        reps[i] = r.tobytes()
    data = np.frombuffer(b"abcdefgh", dtype=np.uint8)[rng.integers(0, 8, (1 << 20) + 17)].copy()
    n_big = 1100 if big else 300                                # 65 536-byte picks: about 72 MB or 20 MB out
    at = np.sort(rng.choice(np.arange(0, data.size - 400, 400), n_big + 600, replace=False))
    for k, p in enumerate(at):
        tok = [b"Q4444", b"Q1", b"Q22", b"Q333"][k % 4] if k >= n_big else b"Q4444"
        run = b"z" * int(rng.choice([0, 2, 128, 300])) + b"y" * int(rng.choice([0, 3, 192]))
        seg = np.frombuffer(tok + run + tok, dtype=np.uint8)
        data[p:p + seg.size] = seg
    table = PfacTable.from_file(path, 256)
    ll = line_lengths(path)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_replacements(reps)
        for n_owned, entry in ((data.size, 0), (data.size - 3, 1)):
            out, ex = g.replace(data, n_owned, entry)
            pos, ids = oracle_records(path, data, n_owned)
            sel, wex = greedy(pos, ll[ids], entry, n_owned)
            want = splice(data, entry, n_owned, pos[sel], ll[ids[sel]], ids[sel], rep_table(reps))
            assert (want.size >= 64 << 20) == big
            assert out.size == want.size and ex == wex
            assert np.array_equal(out, want), f"first difference at byte {int(np.argmax(out != want))}"
            assert np.array_equal(out, re_replace(pats, reps, data, entry, n_owned)[0])
        too_long = {**reps, 4: b"\xff" * 65537}
        with pytest.raises(ValueError):
            g.set_replacements(too_long)
        off = np.zeros(table.num_final + 1, dtype=np.uint32)      # the C-ABI itself refuses it too
        off[1:] = 65537
        blob = np.full(65537, 0xFF, dtype=np.uint8)
        assert g._L.pfac_table_set_replacements(g._ctx, off.ctypes.data, table.num_final, blob.ctypes.data,
                                                blob.size) == _ffi.PFAC_E_ARG
        off[1:] = 65536                                         # and takes exactly the limit
        assert g._L.pfac_table_set_replacements(g._ctx, off.ctypes.data, table.num_final, blob.ctypes.data,
                                                65536) == 0


# ---------------------------------------------------------------------------
def states_set(n_lines):
    """n_lines pattern lines (two of them duplicates: final states of length -1) over a..d of 1 to 3 bytes."""
    rng = np.random.default_rng(n_lines)
    words = [bytes(w) for L in (1, 2, 3) for w in np.array(np.meshgrid(*[list(b"abcd")] * L)).reshape(L, -1).T.tolist()]
    lines = [words[i] for i in rng.permutation(len(words))[:n_lines - 2]]
    lines.insert(n_lines // 3, lines[1])
    lines.insert(n_lines // 2, lines[5])
    return lines


@pytest.mark.parametrize("env", [{}, {"PFAC_WIDE": "1"}], ids=["natural-width", "wide"])
@pytest.mark.parametrize("n_final", [16, 17, 64, 65])
def test_final_states_at_the_register_boundary(n_final, env, tmp_path, monkeypatch):
    """Pattern lengths come from a lane register up to 64 final states, from memory above (documents and selection);
    16 / 17 states cross the 2-byte record boundary.  Duplicate lines count as states."""
    set_knobs(monkeypatch, env)
    lines = states_set(n_final)
    path = write_patterns(tmp_path, lines)
    table = PfacTable.from_file(path, 256)
    assert table.num_final == n_final
    rng = np.random.default_rng(n_final)
    data = np.frombuffer(b"abcd", dtype=np.uint8)[rng.integers(0, 4, 300_001)]
    off = random_offsets(rng, data.size, 900, empties=5)
    ll = line_lengths(path)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        got_first, got = g.scan_documents((data, off))
        assert g.scan_format()[0] == record_width(n_final, env)
        picks = {}
        for e in (0, 1, 3):
            n, ex = g.select_leftmost_longest(e)
            picks[e] = (g.selection_to_host(n), ex)
    o = Oracle(path, 1, 1)
    wfirst, wpos, wids = oracle_per_doc(o, data, off)
    o.close()
    np.testing.assert_array_equal(got_first, wfirst)
    np.testing.assert_array_equal(got["pos"].astype(np.int64), wpos)
    np.testing.assert_array_equal(table.idmap[got["state"]], wids)
    pos, ids = oracle_records(path, data)
    assert set(ids.tolist()) == set({p: i for i, p in enumerate(lines, start=1)}.values())   # every winning line occurs
    for e, (rec, ex) in picks.items():
        s, wex = greedy(pos, ll[ids], e, data.size)
        np.testing.assert_array_equal(rec["pos"].astype(np.int64), pos[s])
        np.testing.assert_array_equal(table.idmap[rec["state"]], ids[s])
        assert ex == wex


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pat,env", [("xaa", {}), ("xaa", {"PFAC_WIDE": "1"}), ("experimentpattern", {})])
def test_tiles_at_the_document_window_boundary(pat, env, resolve, monkeypatch):
    """Tiles holding 58 to 66 document starts (the lane-shuffle search covers 63 candidate documents, a binary search
    in memory the rest), with and without a start on the tile's first byte; three tiles inside one document."""
    set_knobs(monkeypatch, env)
    buf = tiled_bytes(40 * TILE + 99, open(resolve("paragraph402"), "rb").read())
    rng = np.random.default_rng(63)
    cuts = [0, buf.size]
    for k, S in enumerate(range(58, 67)):
        t = 2 + 2 * k
        starts = rng.choice(np.arange(t * TILE + 1, (t + 1) * TILE), S, replace=False).tolist()
        if k % 2:
            starts[0] = t * TILE                                # one start on the tile's first byte
        cuts += starts
    cuts += [21 * TILE + 100, 25 * TILE - 5]                    # tiles 22 to 24 inside one document
    off = np.array(sorted(cuts), dtype=np.uint64)
    table = PfacTable.from_file(resolve(pat), 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        first, rec = g.scan_documents((buf, off))
    o = Oracle(resolve(pat), 1, 1)
    wfirst, wpos, wids = oracle_per_doc(o, buf, off)
    o.close()
    np.testing.assert_array_equal(first, wfirst)
    assert rec.size == wpos.size
    np.testing.assert_array_equal(rec["pos"].astype(np.int64), wpos)
    np.testing.assert_array_equal(table.idmap[rec["state"]], wids)
    assert rec.size > 1000
