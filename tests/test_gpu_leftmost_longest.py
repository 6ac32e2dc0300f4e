"""Leftmost-longest non-overlapping selection on the GPU (run with -m gpu on an MI355X): pfac_records_leftmost_longest
against the host references of tests/llref.py.  The expectation is built from the CPU oracle's records (or, for
character classes, the brute-force matcher's) with pattern lengths from the pattern file's own lines -- never from the
device or from PfacTable.final_lengths.  Integer work: bit-exact."""
import importlib.util
import json
import os

import numpy as np
import pytest

from llref import check_greedy, greedy, line_lengths
from orc import Oracle, ac_whole_shard
from phfpfac_amd import GpuMatcher, PfacError, PfacTable
from phfpfac_amd import _ffi
from phfpfac_amd.matcher import tiled_bytes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 4096


def para_bytes(resolve, n):
    return tiled_bytes(n, open(resolve("paragraph402"), "rb").read())


def write_patterns(tmp_path, pats, name="p.pat"):
    f = tmp_path / name
    f.write_bytes(b"".join(p + b"\n" for p in pats))
    return str(f)


def expected(path, data, n_owned, entry):
    """(pos, len) of the greedy selection over the oracle's records that start in [0, n_owned), and the exit."""
    o = Oracle(path, 1, 1)
    pos, ids = o.scan_spec(np.ascontiguousarray(data))
    o.close()
    keep = pos < n_owned
    pos, ids = pos[keep], ids[keep]
    lens = line_lengths(path)[ids]
    sel, ex = greedy(pos, lens, entry, n_owned)
    return pos[sel], lens[sel], ex


def assert_selection(path, table, got, want):
    rec, ex = got
    wpos, wlen, wex = want
    assert rec.size == wpos.size, (rec.size, wpos.size)
    np.testing.assert_array_equal(rec["pos"].astype(np.int64), wpos)
    np.testing.assert_array_equal(line_lengths(path)[table.idmap[rec["state"]]], wlen)
    assert ex == wex


def check(path, data, n_owned=None, entry=0, table=None, g=None):
    table = table or PfacTable.from_file(path, 256)
    n_owned = data.size if n_owned is None else n_owned
    if g is None:
        with GpuMatcher(0, 1) as g:
            g.load_table(table)
            got = g.scan_leftmost_longest(data, n_owned, entry)
    else:
        got = g.scan_leftmost_longest(data, n_owned, entry)
    assert_selection(path, table, got, expected(path, data, n_owned, entry))
    return got


def status_of(fn):
    with pytest.raises(PfacError) as e:
        fn()
    return e.value


# ---------------------------------------------------------------------------
def test_worked_example(tmp_path):
    path = write_patterns(tmp_path, [b"a", b"ab", b"bc", b"abcd"])
    table = PfacTable.from_file(path, 256)
    data = np.frombuffer(b"xabcabcd", dtype=np.uint8)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        ids = lambda rec: table.idmap[rec["state"]].tolist()
        rec, ex = g.scan_leftmost_longest(data, entry=0)
        assert (rec["pos"].tolist(), ids(rec), ex) == ([1, 4], [2, 4], 0)
        rec, ex = g.scan_leftmost_longest(data, entry=2)
        assert (rec["pos"].tolist(), ids(rec), ex) == ([2, 4], [3, 4], 0)
        rec, ex = g.scan_leftmost_longest(data[:5], n_owned=2, entry=0)        # owned [0, 2), halo max_pat_len - 1
        assert (rec["pos"].tolist(), ids(rec), ex) == ([1], [2], 1)
        rec, ex = g.scan_leftmost_longest(np.ascontiguousarray(data[2:]), entry=ex)
        assert (rec["pos"].tolist(), ids(rec), ex) == ([2], [4], 0)
        rec, _ = g.scan_leftmost_longest(np.ascontiguousarray(data[2:]), entry=0)
        assert (rec["pos"][0], ids(rec)[0]) == (0, 3)                         # what a wrong entry would pick


def fingerprint_cases():
    cases = json.load(open(os.path.join(HERE, "golden", "fingerprints.json")))["cases"]
    return sorted({(c["pattern"], c["input"], c["width"]) for c in cases.values()})


@pytest.mark.parametrize("pat,inp,width", fingerprint_cases())
def test_fingerprint_cases(pat, inp, width, resolve):
    path = resolve(pat)
    data = np.fromfile(resolve(inp), dtype=np.uint8)
    table = PfacTable.from_file(path, width)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        for entry in (0, 1):
            check(path, data, entry=entry, table=table, g=g)


@pytest.mark.parametrize("env", [{}, {"PFAC_WIDE": "1"}, {"PFAC_DENSE": "1"}, {"PFAC_FORCE_L2": "1"},
                                 {"PFAC_DENSE": "1", "PFAC_FORCE_L2": "1"}])
@pytest.mark.parametrize("pat", ["experimentpattern", "xaa+xab+xac+xad"])
def test_record_forms_and_kernel_variants(pat, env, resolve, monkeypatch):
    """2-byte records (experimentpattern), 4-byte (the dictionary), 8-byte (PFAC_WIDE); dense staging, tables via L2."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    path = resolve(pat)
    data = para_bytes(resolve, (1 << 20) + 77)
    table = PfacTable.from_file(path, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.scan_bytes(data)                      # (dense mode: a first scan, so that the adapted mode is what runs)
        if "PFAC_WIDE" in env:
            assert g.scan_format()[0] == 8
        rec, _ = check(path, data, table=table, g=g)
        check(path, data, n_owned=data.size - 3000, entry=1, table=table, g=g)
    assert rec.size > 10000


def a_runs(n, seed, breaks):
    rng = np.random.default_rng(seed)
    data = np.full(n, ord("a"), dtype=np.uint8)
    data[rng.integers(0, n, breaks)] = ord("b")
    return data


@pytest.mark.parametrize("pats", [[b"aa"], [b"aaa", b"aaaaa"]])
def test_non_converging_runs(pats, tmp_path):
    """Runs of `a` over many 64-tile groups: chains that enter at different offsets never meet until a `b` break."""
    path = write_patterns(tmp_path, pats)
    table = PfacTable.from_file(path, 256)
    n = (3 << 20) + 1234
    data = a_runs(n, 5, 40)
    data[: 700 * TILE] = ord("a")                          # one run across more than ten groups
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        for entry, n_owned in ((0, n), (1, n - 1), (2, n - 4097), (1, 64 * TILE * 3 + 5)):
            rec, ex = check(path, data, n_owned, entry, table=table, g=g)
            assert rec.size > n_owned // 6


def test_long_patterns_straddle_tiles_and_groups(tmp_path):
    """Patterns of 700 to 1 000 bytes cut from a random string, inputs tiled from it: matches cross tile and group
    boundaries and the tile functions are about 1 000 entries wide."""
    rng = np.random.default_rng(21)
    base = rng.integers(97, 101, 3001).astype(np.uint8)      # a..d
    pats = []
    for _ in range(40):
        L = int(rng.integers(700, 1001))
        s = int(rng.integers(0, base.size - L))
        pats.append(base[s:s + L].tobytes())
    pats.append(base[: 1000].tobytes())
    path = write_patterns(tmp_path, pats)
    table = PfacTable.from_file(path, 256)
    assert table.max_pat_len == 1000
    data = tiled_bytes((70 * 64 * TILE) // 16 + 999, base.tobytes())
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        for entry in (0, 1, 999, 1000):
            rec, ex = check(path, data, entry=entry, table=table, g=g)
            assert rec.size > 100


def chain(g, data, cuts, halo, entry):
    """Scan the owned ranges [cuts[i], cuts[i + 1]) in turn with a halo, each call's exit the next one's entry."""
    pos, st = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        rec, entry = g.scan_leftmost_longest(np.ascontiguousarray(data[a: min(b + halo, data.size)]), b - a, entry)
        pos.append(rec["pos"].astype(np.int64) + a)
        st.append(rec["state"])
    return np.concatenate(pos), np.concatenate(st), entry


@pytest.mark.parametrize("case", ["text", "runs", "long"])
def test_chaining_equals_one_scan(case, resolve, tmp_path):
    rng = np.random.default_rng({"text": 1, "runs": 2, "long": 3}[case])
    if case == "text":
        path, data = resolve("xaa+xab+xac+xad"), para_bytes(resolve, 900_001)
    elif case == "runs":                                     # the parity of the `aa` chain carries across every cut
        path, data = write_patterns(tmp_path, [b"aa"]), a_runs(600_000, 3, 7)
    else:
        base = rng.integers(97, 99, 2000).astype(np.uint8)
        path = write_patterns(tmp_path, [base[s: s + 900].tobytes() for s in (0, 17, 400, 1000)] + [b"ab", b"b"])
        data = tiled_bytes(500_000, base.tobytes())
    table = PfacTable.from_file(path, 256)
    halo = table.max_pat_len - 1
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        for entry in (0, 1):
            whole, wex = g.scan_leftmost_longest(data, entry=entry)
            for parts in (2, 3, 7):
                inner = rng.integers(1, data.size - 1, parts - 1)
                if case == "runs":
                    inner[0] |= 1                            # an odd cut inside a run
                cuts = [0] + sorted(inner.tolist()) + [data.size]
                pos, st, ex = chain(g, data, cuts, halo, entry)
                np.testing.assert_array_equal(pos, whole["pos"].astype(np.int64))
                np.testing.assert_array_equal(st, whole["state"])
                assert ex == wex
    assert_selection(path, table, (whole, wex), expected(path, data, data.size, 1))


# ---------------------------------------------------------------------------
def test_edges(tmp_path):
    path = write_patterns(tmp_path, [b"ab", b"abcde", b"c"])
    table = PfacTable.from_file(path, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        rec, ex = g.scan_leftmost_longest(np.zeros(0, dtype=np.uint8), entry=3)     # empty scan
        assert rec.size == 0 and ex == 3
        rec, ex = g.scan_leftmost_longest(np.frombuffer(b"abc", dtype=np.uint8), entry=5)   # entry > n_owned
        assert rec.size == 0 and ex == 2
        data = np.full(5 * TILE + 100, ord("x"), dtype=np.uint8)                   # records only in the ragged tile
        data[5 * TILE + 10: 5 * TILE + 15] = np.frombuffer(b"abcde", dtype=np.uint8)
        data[-2:] = np.frombuffer(b"ab", dtype=np.uint8)
        for n_owned in (data.size, data.size - 1, 5 * TILE + 12):
            for entry in (0, 5):
                check(path, data, n_owned, entry, table=table, g=g)
        rec, ex = g.scan_leftmost_longest(data, 5 * TILE + 11)
        assert rec["pos"].tolist() == [5 * TILE + 10] and ex == 4
        assert status_of(lambda: g.select_leftmost_longest(6)).status == _ffi.PFAC_E_ARG    # entry > max_pat_len
        assert g.select_leftmost_longest(5) == (1, 4)


def test_state_errors(resolve):
    data = para_bytes(resolve, 20_000)
    table = PfacTable.from_file(resolve("xaa"), 256)
    other = PfacTable.from_file(resolve("experimentpattern"), 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        assert status_of(lambda: g.select_leftmost_longest()).status == _ffi.PFAC_E_STATE      # before a scan
        assert status_of(lambda: g.selection_to_host(0)).status == _ffi.PFAC_E_STATE
        g.scan_bytes(data)
        assert g.select_leftmost_longest()[0] > 0
        g.load_table(table)                                                                  # an upload clears the lengths
        g.scan_bytes(data)
        assert status_of(lambda: g.select_leftmost_longest()).status == _ffi.PFAC_E_STATE
        g.load_table(other)
        g.set_final_lengths(other.final_lengths())
        g.scan_bytes(data)
        g.load_table(table)                                                                  # the scan ran with `other`
        g.set_final_lengths(table.final_lengths())
        assert status_of(lambda: g.select_leftmost_longest()).status == _ffi.PFAC_E_STATE
        import torch
        small = torch.zeros(64, dtype=torch.int64, device="cuda")                          # a scan that overflows
        g.scan_async(data.size, d_records=small, capacity=64)
        assert g.scan_finish(allow_overflow=True)[1]
        assert status_of(lambda: g.select_leftmost_longest()).status == _ffi.PFAC_E_STATE


def test_caller_buffer_overflow_and_sentinels(resolve):
    import torch
    data = para_bytes(resolve, 100_000)
    table = PfacTable.from_file(resolve("experimentpattern"), 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        rec, ex = g.scan_leftmost_longest(data)
        n = rec.size
        assert n > 100
        sentinel = int(np.uint64(0xABABABABABABABAB).view(np.int64))
        out = torch.full((n + 1,), sentinel, dtype=torch.int64, device="cuda")
        e = status_of(lambda: g.select_leftmost_longest(d_out=out, out_cap=n - 1))
        assert e.status == _ffi.PFAC_E_OVERFLOW and e.n_selected == n
        g.sync()
        assert (out.cpu() == sentinel).all()
        assert g.select_leftmost_longest(d_out=out, out_cap=n) == (n, ex)
        g.sync()
        got = out.cpu().numpy()
        assert got[n] == sentinel
        np.testing.assert_array_equal(got[:n].view(np.uint64), rec.view(np.uint64))
        assert status_of(lambda: g.selection_to_host(n)).status == _ffi.PFAC_E_STATE         # nothing slot-owned


def test_documents_and_selection_share_a_slot(resolve):
    data = para_bytes(resolve, 300_000)
    off = np.array([0, 1000, 150_000, data.size], dtype=np.uint64)
    table = PfacTable.from_file(resolve("xaa"), 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        first, docs = g.scan_documents((data, off))
        n_docs = g.segment_records(off.size - 1)
        n_sel, ex = g.select_leftmost_longest()
        f2, d2 = g.segment_to_host(n_docs, off.size - 1)
        sel = g.selection_to_host(n_sel)
        n_docs = g.segment_records(off.size - 1)
        sel2 = g.selection_to_host(n_sel)
        f3, d3 = g.segment_to_host(n_docs, off.size - 1)
    np.testing.assert_array_equal(f2, first)
    np.testing.assert_array_equal(d2, docs)
    np.testing.assert_array_equal(f3, first)
    np.testing.assert_array_equal(d3, docs)
    np.testing.assert_array_equal(sel2, sel)
    assert_selection(resolve("xaa"), table, (sel, ex), expected(resolve("xaa"), data, data.size, 0))


def test_two_slots_stay_independent(resolve):
    path = resolve("xaa+xab+xac+xad")
    table = PfacTable.from_file(path, 256)
    a = para_bytes(resolve, 300_000)
    b = np.ascontiguousarray(para_bytes(resolve, 250_000 + 401)[401:])
    with GpuMatcher(0, 2) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        for s, buf in ((0, a), (1, b)):
            g.reserve(s, buf.size, 2 * buf.size)
            g.h2d(buf, s)
            g.scan_async(buf.size, slot=s)
        for s in (0, 1):
            g.scan_finish(s)
        na, ea = g.select_leftmost_longest(0, slot=0)
        nb, eb = g.select_leftmost_longest(2, slot=1)
        rb = g.selection_to_host(nb, slot=1)
        ra = g.selection_to_host(na, slot=0)
    assert_selection(path, table, (ra, ea), expected(path, a, a.size, 0))
    assert_selection(path, table, (rb, eb), expected(path, b, b.size, 2))


def test_charclass():
    spec = importlib.util.spec_from_file_location("charclass_oracle", os.path.join(os.path.dirname(HERE), "oracle", "charclass_oracle.py"))
    cco = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cco)
    patterns = b"[a-c]x\nax\n[^a-z0-9 ]\nq[0-9][0-9]\n[a-c]\n[-a]z\nax[xy]\n[a-c]x\n"
    plen = np.array([0] + [len(p) for p in cco.parse(patterns)], dtype=np.int64)
    table = PfacTable.from_charclass(patterns, 256)
    rng = np.random.default_rng(3)
    alphabet = np.frombuffer(b"abcxyzq0123456789 AB\nCD-Z!", dtype=np.uint8)
    data = alphabet[rng.integers(0, alphabet.size, 300_000)]
    pos, ids = cco.match(patterns, data)
    lens = plen[ids]
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        for entry in (0, 1, 3):
            rec, ex = g.scan_leftmost_longest(data, entry=entry)
            sel, wex = greedy(pos, lens, entry, data.size)
            np.testing.assert_array_equal(rec["pos"].astype(np.int64), pos[sel])
            first_id = table.out_ids[table.out_first[rec["state"]]]             # every pattern of a state: one length
            np.testing.assert_array_equal(plen[first_id], lens[sel])
            assert ex == wex and rec.size > 10000


# ---------------------------------------------------------------------------
def test_one_gib_experimentpattern_text(resolve):
    """1 GiB of tiled text, experimentpattern (2-byte records, 80 M records).  The scan is pinned first against one
    serial Aho-Corasick pass (count + checksum); the selection is then checked against all its records."""
    import torch
    n = 1 << 30
    path = resolve("experimentpattern")
    para = open(resolve("paragraph402"), "rb").read()
    table = PfacTable.from_file(path, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, para)
        g.reserve(0, 0, n // 8)
        total = g.scan_resident(n, n, d_input=buf)
        chk = g.checksum(total)
        host = buf[:n].cpu().numpy()
        del buf
        whole = g.records_to_host(total)
        n_sel, ex = g.select_leftmost_longest(1)
        sel = g.selection_to_host(n_sel)
    torch.cuda.empty_cache()
    assert (total, chk) == ac_whole_shard(path, host)
    del host
    lens = line_lengths(path)[table.idmap[whole["state"]]]
    slens = line_lengths(path)[table.idmap[sel["state"]]]
    assert check_greedy(whole["pos"].astype(np.int64), lens, (sel["pos"].astype(np.int64), slens), 1, n) == ex
    assert 0 < n_sel <= total
