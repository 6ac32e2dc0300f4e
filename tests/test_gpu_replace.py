"""Find-and-replace over the leftmost-longest selection on the GPU (run with -m gpu on an MI355X):
pfac_replace_leftmost_longest against the host references of tests/replref.py.  The expectation comes from the CPU
oracle's records, pattern lengths from the pattern file's own lines and replacements keyed by pattern id -- never from
the device.  Bit-exact."""
import json
import os

import numpy as np
import pytest

from llref import check_greedy, greedy, line_lengths
from orc import Oracle, ac_whole_shard
from phfpfac_amd import GpuMatcher, PfacError, PfacTable
from phfpfac_amd import _ffi
from phfpfac_amd.matcher import tiled_bytes
from replref import greedy_replace, re_replace, rep_table, splice

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKED = [b"a", b"ab", b"bc", b"abcd"]


def write_patterns(tmp_path, pats, name="p.pat"):
    f = tmp_path / name
    f.write_bytes(b"".join(p + b"\n" for p in pats))
    return str(f)


def random_reps(n_ids, seed, max_len=12):
    rng = np.random.default_rng(seed)
    return {i: bytes(rng.integers(0, 256, int(rng.integers(0, max_len + 1))).astype(np.uint8))
            for i in range(1, n_ids + 1)}


def expected(path, reps, data, n_owned, entry):
    o = Oracle(path, 1, 1)
    pos, ids = o.scan_spec(np.ascontiguousarray(data))
    o.close()
    lens = line_lengths(path)[ids]
    return greedy_replace(data, entry, n_owned, pos, lens, ids, rep_table(reps))


def check(g, path, reps, data, n_owned=None, entry=0):
    n_owned = data.size if n_owned is None else n_owned
    out, ex = g.replace(data, n_owned, entry)
    want, wex = expected(path, reps, data, n_owned, entry)
    assert out.size == want.size, (out.size, want.size)
    assert bytes(out) == bytes(want)
    assert ex == wex
    return out, ex


def matcher_for(path, reps, width=256):
    table = PfacTable.from_file(path, width)
    g = GpuMatcher(0, 1)
    g.load_table(table)
    g.set_replacements(reps)
    return g, table


def status_of(fn):
    with pytest.raises(PfacError) as e:
        fn()
    return e.value


# ---------------------------------------------------------------------------
def test_worked_example(tmp_path):
    path = write_patterns(tmp_path, WORKED)
    reps = {1: b"", 2: b"Z", 3: b"BC", 4: b"L" * 5000}          # deletion, shorter, equal, longer than 4 KiB
    data = np.frombuffer(b"xabcabcd", dtype=np.uint8)
    g, _ = matcher_for(path, reps)
    with g:
        out, ex = g.replace(data)
        assert (bytes(out), ex) == (b"xZc" + b"L" * 5000, 0)
        out, ex = g.replace(data, entry=2)
        assert (bytes(out), ex) == (b"BC" + b"L" * 5000, 0)
        out, ex = g.replace(data[:5], n_owned=2)                # the pick at 1 runs into the halo
        assert (bytes(out), ex) == (b"xZ", 1)
        out, ex = g.replace(np.ascontiguousarray(data[2:]), entry=ex)
        assert (bytes(out), ex) == (b"c" + b"L" * 5000, 0)
        for entry in range(4):
            check(g, path, reps, data, entry=entry)


def fingerprint_cases():
    cases = json.load(open(os.path.join(HERE, "golden", "fingerprints.json")))["cases"]
    return sorted({(c["pattern"], c["input"]) for c in cases.values()
                   if (c["pattern"], c["input"]) in {("experimentpattern", "paragraph402"), ("experimentpattern", "1M")}
                   or (c["pattern"] == "xaa+xab+xac+xad" and c["input"].startswith("bytefile"))})


@pytest.mark.parametrize("pat,inp", fingerprint_cases())
def test_golden_cases(pat, inp, resolve):
    path = resolve(pat)
    data = np.fromfile(resolve(inp), dtype=np.uint8)
    n_ids = line_lengths(path).size - 1
    for seed, max_len in ((1, 12), (2, 40)):
        reps = random_reps(n_ids, seed, max_len)
        g, _ = matcher_for(path, reps)
        with g:
            out, _ = check(g, path, reps, data)
            check(g, path, reps, data, n_owned=data.size - 37, entry=1)
    assert out.size > 0


@pytest.mark.parametrize("env", [{}, {"PFAC_WIDE": "1"}, {"PFAC_FORCE_L2": "1"}])
@pytest.mark.parametrize("pat", ["experimentpattern", "xaa+xab+xac+xad"])
def test_record_forms_and_l2(pat, env, resolve, monkeypatch):
    """2-byte records (experimentpattern), 4-byte (the dictionary), 8-byte (PFAC_WIDE); tables via L2."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    path = resolve(pat)
    data = tiled_bytes((1 << 20) + 77, open(resolve("paragraph402"), "rb").read())
    reps = random_reps(line_lengths(path).size - 1, 5)
    g, _ = matcher_for(path, reps)
    with g:
        g.scan_bytes(data)
        if "PFAC_WIDE" in env:
            assert g.scan_format()[0] == 8
        check(g, path, reps, data)


def test_no_matches(tmp_path):
    path = write_patterns(tmp_path, [b"zzzq", b"qqqz"])
    rng = np.random.default_rng(4)
    data = rng.integers(ord("a"), ord("y"), (1 << 20) + 13).astype(np.uint8)
    g, _ = matcher_for(path, {1: b"1", 2: b"2"})
    with g:
        for n_owned, entry in ((data.size, 0), (data.size, 3), (data.size - 5, 2), (4097, 1)):
            out, ex = g.replace(data, n_owned, entry)
            assert bytes(out) == bytes(data[entry:n_owned]) and ex == 0


def a_runs(n, run):
    data = np.full(n, ord("a"), dtype=np.uint8)
    data[run::run + 1] = ord("b")
    return data


@pytest.mark.parametrize("run", [100_003, 7, 64 * 64 * 2 + 1])
def test_aa_runs_deletion_and_doubling(run, tmp_path):
    path = write_patterns(tmp_path, [b"aa"])
    data = a_runs((4 << 20) + 3, run)
    g, _ = matcher_for(path, {1: b""})
    with g:
        out, _ = check(g, path, {1: b""}, data)
        assert set(bytes(out[:-1]).split(b"b")) <= {b"", b"a"}  # only the odd leftovers
        g.set_replacements({1: b"aaaa"})
        out, _ = check(g, path, {1: b"aaaa"}, data)
        assert out.size > data.size


def test_edges(tmp_path):
    path = write_patterns(tmp_path, [b"abcdefg", b"bc", b"fgh", b"h"])
    reps = {1: b"<7>", 2: b"", 3: b"FGH!", 4: b"hhhhhhhhhhhhhhhhhh"}
    para = b"xxabcdefghyhbcfgh"
    g, _ = matcher_for(path, reps)
    with g:
        for n in (0, 1, 15, 16, 17, 4095, 4096, 4097, 70001):
            data = tiled_bytes(n, para)
            for n_owned in sorted({n, max(n - 1, 0), max(n - 6, 0)}):
                for entry in (0, 1, 6):
                    check(g, path, reps, data, n_owned, entry)
        data = tiled_bytes(100, para)
        out, ex = g.replace(data, 3, 7)                        # entry past n_owned
        assert out.size == 0 and ex == 4
        out, ex = g.replace(np.frombuffer(b"zzabcdefg", dtype=np.uint8), 3)   # the last pick runs into the halo
        assert (bytes(out), ex) == (b"zz<7>", 6)


def test_chaining_equals_one_shot(resolve, tmp_path):
    para = open(resolve("paragraph402"), "rb").read()
    words = sorted({w for w in para.split() if 2 <= len(w) <= 12})
    path = write_patterns(tmp_path, words + [w[:3] for w in words if len(w) > 5])
    data = np.fromfile(resolve("1M"), dtype=np.uint8)
    halo = PfacTable.from_file(path, 256).halo
    reps = random_reps(line_lengths(path).size - 1, 11, 30)
    g, _ = matcher_for(path, reps)
    with g:
        whole, wex = check(g, path, reps, data)
        o = Oracle(path, 1, 1)
        pos, ids = o.scan_spec(data)
        o.close()
        lens = line_lengths(path)[ids]
        sel, _ = greedy(pos, lens, 0, data.size)
        long_picks = sel[lens[sel] > 2]
        assert long_picks.size > 100
        rng = np.random.default_rng(8)
        for trial in range(4):
            k = int(rng.integers(2, 5))
            if trial < 2:                                       # cuts inside picks
                cuts = sorted(set(int(pos[i]) + 1 + trial for i in rng.choice(long_picks, k)))
            else:
                cuts = sorted(set(int(c) for c in rng.integers(1, data.size, k)))
            bounds = [0] + cuts + [data.size]
            parts, entry = [], 0
            for a, b in zip(bounds[:-1], bounds[1:]):
                piece = np.ascontiguousarray(data[a:min(data.size, b + halo)])
                out, entry = g.replace(piece, b - a, entry)
                parts.append(bytes(out))
            assert b"".join(parts) == bytes(whole) and entry == wex


def test_caller_buffers(resolve):
    import torch
    path = resolve("experimentpattern")
    data = np.fromfile(resolve("paragraph402"), dtype=np.uint8)
    reps = random_reps(line_lengths(path).size - 1, 3)
    want, _ = expected(path, reps, data, data.size, 0)
    g, _ = matcher_for(path, reps)
    with g:
        d_in = torch.from_numpy(data.copy()).to("cuda:0")
        g.reserve(0, 0, 1 << 16)
        g.set_final_lengths(g.table.final_lengths())
        g.scan_resident(data.size, data.size, d_input=d_in)
        n_sel, _ = g.select_leftmost_longest(0)
        # caller's selection buffer (d_sel)
        d_sel = torch.zeros(n_sel * 8 + 64, dtype=torch.uint8, device="cuda:0")
        assert g.select_leftmost_longest(0, d_out=d_sel, out_cap=n_sel + 8)[0] == n_sel
        e = status_of(lambda: g.replace_selection(d_input=d_in))   # the selection is in the caller's buffer
        assert e.status == _ffi.PFAC_E_STATE
        cap = want.size + 100
        d_out = torch.full((cap + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        e = status_of(lambda: g.replace_selection(d_input=d_in, d_sel=d_sel, d_out=d_out, out_cap=want.size - 1))
        assert e.status == _ffi.PFAC_E_OVERFLOW and e.out_bytes == want.size
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0xA5).all()              # nothing written
        n = g.replace_selection(d_input=d_in, d_sel=d_sel, d_out=d_out, out_cap=cap)
        g.sync()
        host = d_out.cpu().numpy()
        assert n == want.size and bytes(host[:n]) == bytes(want)
        assert (host[n:] == 0xA5).all()                         # no byte at or past out_bytes
        # an offset into an aligned buffer; and the slot-owned selection again
        g.select_leftmost_longest(0)
        d_out.fill_(0x5A)
        n = g.replace_selection(d_input=d_in, d_out=d_out[16:], out_cap=cap - 16)
        g.sync()
        host = d_out.cpu().numpy()
        assert bytes(host[16:16 + n]) == bytes(want) and (host[:16] == 0x5A).all() and (host[16 + n:] == 0x5A).all()
        e = status_of(lambda: g.replace_selection(d_input=d_in, d_out=d_out[1:], out_cap=cap))
        assert e.status == _ffi.PFAC_E_ARG


def test_state_errors(tmp_path):
    path = write_patterns(tmp_path, WORKED)
    data = np.frombuffer(b"xabcabcd" * 100, dtype=np.uint8)
    table = PfacTable.from_file(path, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.scan_leftmost_longest(data)
        assert status_of(lambda: g.replace_selection()).status == _ffi.PFAC_E_STATE     # no replacements
        g.set_replacements([b"1", b"2", b"3", b"4"])
        g.scan_bytes(data)
        assert status_of(lambda: g.replace_selection()).status == _ffi.PFAC_E_STATE     # no selection since the scan
        g.scan_leftmost_longest(data)
        g.replace_selection()
        g.load_table(table)                                     # a re-upload clears replacements
        assert status_of(lambda: g.replace_selection()).status == _ffi.PFAC_E_STATE
        g.set_replacements([b"1", b"2", b"3", b"4"])
        assert status_of(lambda: g.replace_selection()).status == _ffi.PFAC_E_STATE     # selection of the earlier table
        assert status_of(lambda: g.replacement_to_host(1)).status == _ffi.PFAC_E_STATE
        off = np.zeros(table.num_final, dtype=np.uint32)        # one state short
        rc = g._L.pfac_table_set_replacements(g._ctx, off.ctypes.data, table.num_final - 1, None, 0)
        assert rc == _ffi.PFAC_E_ARG
        off = np.zeros(table.num_final + 1, dtype=np.uint32)
        off[1:] = 70000                                         # longer than the limit
        blob = np.zeros(70000, dtype=np.uint8)
        rc = g._L.pfac_table_set_replacements(g._ctx, off.ctypes.data, table.num_final, blob.ctypes.data, blob.size)
        assert rc == _ffi.PFAC_E_ARG
        out, _ = g.replace(data)
        assert bytes(out) == bytes(re_replace(WORKED, [b"1", b"2", b"3", b"4"], data, 0, data.size)[0])


def test_redaction(resolve):
    path = resolve("experimentpattern")
    data = np.fromfile(resolve("1M"), dtype=np.uint8)
    ll = line_lengths(path)
    table = PfacTable.from_file(path, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_redaction(b"#")
        out, ex = g.replace(data, entry=2)
        assert ex == 0 and out.size == data.size - 2
        want, _ = expected(path, {i: b"#" * int(ll[i]) for i in range(1, ll.size)}, data, data.size, 2)
        assert bytes(out) == bytes(want)
        masked = np.flatnonzero(out != data[2:])
        assert masked.size > 0 and (out[masked] == ord("#")).all()


def test_determinism(resolve):
    path = resolve("xaa+xab+xac+xad")
    data = np.fromfile(resolve("bytefile/1000000byte"), dtype=np.uint8)
    g, _ = matcher_for(path, random_reps(line_lengths(path).size - 1, 9, 70))
    with g:
        a, _ = g.replace(data)
        b, _ = g.replace(data)
    assert bytes(a) == bytes(b)


# ---------------------------------------------------------------------------
def test_one_gib_experimentpattern_text(resolve):
    """1 GiB of tiled text: the scan pinned against serial Aho-Corasick, the selection against all its records by
    check_greedy, the output against the vectorised splice of that selection."""
    import torch
    n = 1 << 30
    path = resolve("experimentpattern")
    para = open(resolve("paragraph402"), "rb").read()
    ll = line_lengths(path)
    reps = random_reps(ll.size - 1, 21, 16)
    table = PfacTable.from_file(path, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_replacements(reps)
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, para)
        g.reserve(0, 0, n // 8)
        total = g.scan_resident(n, n, d_input=buf)
        chk = g.checksum(total)
        whole = g.records_to_host(total)
        n_sel, ex = g.select_leftmost_longest(1)
        sel = g.selection_to_host(n_sel)
        n_out = g.replace_selection(d_input=buf)
        out = g.replacement_to_host(n_out)
        host = buf[:n].cpu().numpy()
        del buf
    torch.cuda.empty_cache()
    assert (total, chk) == ac_whole_shard(path, host)
    lens = ll[table.idmap[whole["state"]]]
    wpos = whole["pos"].astype(np.int64)
    del whole
    sids = table.idmap[sel["state"]]
    spos = sel["pos"].astype(np.int64)
    del sel
    assert check_greedy(wpos, lens, (spos, ll[sids]), 1, n) == ex
    del wpos, lens
    assert 0 < n_sel <= total
    want = splice(host, 1, n, spos, ll[sids], sids, rep_table(reps))
    assert out.size == want.size == n_out
    assert np.array_equal(out, want)
