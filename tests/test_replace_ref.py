"""The host references of find-and-replace (tests/replref.py) checked against each other, the chaining identity on the
host, and replacement_table.  CPU only."""
import numpy as np
import pytest

from orc import Oracle
from phfpfac_amd import PfacTable, replacement_table
from replref import greedy_replace, re_replace, rep_table, splice

PATTERNS = [b"a", b"ab", b"bc", b"abcd"]


def write_patterns(tmp_path, pats, name="p.pat"):
    f = tmp_path / name
    f.write_bytes(b"".join(p + b"\n" for p in pats))
    return str(f)


def oracle_records(path, data):
    o = Oracle(path, 1, 1)
    pos, ids = o.scan_spec(np.ascontiguousarray(data))
    o.close()
    return pos.astype(np.int64), ids.astype(np.int64)


def ref_a(path, pats, reps, data, entry, n_owned):
    pos, ids = oracle_records(path, data)
    lens = np.array([len(pats[i - 1]) for i in ids], dtype=np.int64)
    return greedy_replace(data, entry, n_owned, pos, lens, ids, rep_table(reps))


def random_case(rng):
    alpha = b"abc"[: int(rng.integers(2, 4))]
    pats = [bytes(rng.choice(list(alpha), int(rng.integers(1, 6)))) for _ in range(int(rng.integers(1, 12)))]
    if rng.random() < 0.5:
        pats.append(pats[0])                                   # a duplicate line
    reps = [bytes(rng.choice(list(b"XYZ"), int(rng.integers(0, 9)))) for _ in pats]
    data = np.frombuffer(bytes(rng.choice(list(alpha + b"d"), int(rng.integers(0, 400)))), dtype=np.uint8)
    return pats, reps, data


def test_worked_example():
    reps = [b"", b"<2>", b"BC", b"<abcd-long>"]
    data = np.frombuffer(b"xabcabcd", dtype=np.uint8)
    out, ex = re_replace(PATTERNS, reps, data, 0, data.size)
    assert (bytes(out), ex) == (b"x<2>c<abcd-long>", 0)
    out, ex = re_replace(PATTERNS, reps, data, 2, data.size)
    assert (bytes(out), ex) == (b"BC<abcd-long>", 0)
    out, ex = re_replace(PATTERNS, reps, data[:5], 0, 2)       # the pick at 1 runs into the halo
    assert (bytes(out), ex) == (b"x<2>", 1)
    out, ex = re_replace(PATTERNS, reps, data, 9, data.size)   # entry past n_owned: nothing
    assert (bytes(out), ex) == (b"", 1)


def test_the_references_agree(tmp_path):
    rng = np.random.default_rng(20261016)
    for t in range(60):
        pats, reps, data = random_case(rng)
        path = write_patterns(tmp_path, pats, f"p{t}.pat")
        halo = max(len(p) for p in pats) - 1
        n_owned = int(rng.integers(0, data.size + 1))
        avail = data[: min(data.size, n_owned + halo)]
        entry = int(rng.integers(0, halo + 2))
        reps_d = {i + 1: r for i, r in enumerate(reps)}
        a = ref_a(path, pats, reps_d if t % 2 else reps, avail, entry, n_owned)
        b = re_replace(pats, reps, avail, entry, n_owned)
        assert bytes(a[0]) == bytes(b[0]) and a[1] == b[1], (pats, reps, bytes(data), entry, n_owned)


def test_chaining_identity(tmp_path):
    rng = np.random.default_rng(7)
    for t in range(30):
        pats, reps, data = random_case(rng)
        path = write_patterns(tmp_path, pats, f"p{t}.pat")
        halo = max(len(p) for p in pats) - 1
        whole, wex = ref_a(path, pats, reps, data, 0, data.size)
        cuts = sorted(set(int(c) for c in rng.integers(0, data.size + 1, int(rng.integers(2, 5)))))
        bounds = [0] + cuts + [data.size]
        out, entry = [], 0
        for a, b in zip(bounds[:-1], bounds[1:]):
            piece = np.ascontiguousarray(data[a:min(data.size, b + halo)])
            o, entry = ref_a(path, pats, reps, piece, entry, b - a)
            out.append(bytes(o))
        assert b"".join(out) == bytes(whole) and entry == wex


def test_chaining_cuts_inside_a_pick():
    pats = [b"abcd", b"cd"]
    reps = [b"[4]", b"[2]"]
    data = np.frombuffer(b"xxabcdyyabcdzz", dtype=np.uint8)
    whole, _ = re_replace(pats, reps, data, 0, data.size)
    assert bytes(whole) == b"xx[4]yy[4]zz"
    for cut in range(1, data.size):
        first, ex = re_replace(pats, reps, data[:cut + 3], 0, cut)
        second, ex2 = re_replace(pats, reps, data[cut:], ex, data.size - cut)
        assert bytes(first) + bytes(second) == bytes(whole) and ex2 == 0, cut


def test_splice_in_chunks():
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, 10000).astype(np.uint8)
    starts = np.sort(rng.choice(np.arange(5, 9000, 9), 500, replace=False))
    lens = rng.integers(1, 9, starts.size)
    ids = rng.integers(1, 5, starts.size)
    table = rep_table({1: b"", 2: b"q", 3: b"rrrr", 4: b"s" * 40})
    one = splice(data, 3, 9500, starts, lens, ids, table)
    assert bytes(splice(data, 3, 9500, starts, lens, ids, table, chunk=7)) == bytes(one)
    expect, c = [], 3
    for p, n, i in zip(starts, lens, ids):
        expect += [bytes(data[c:p]), table[1][table[0][i]:table[0][i + 1]]]
        c = p + n
    expect.append(bytes(data[c:9500]))
    assert bytes(one) == b"".join(expect)


def test_replacement_table_duplicates():
    table = PfacTable.from_bytes(b"ab\ncd\nab\n")
    lens = table.final_lengths()
    off, rb = replacement_table(table, [b"first", b"CD", b"last"])
    got = {int(table.idmap[s]): rb[off[s]:off[s + 1]] for s in range(table.num_final) if lens[s] >= 1}
    assert got == {3: b"last", 2: b"CD"}                        # the winning line of the duplicates
    for s in range(table.num_final):
        if lens[s] < 1:
            assert off[s] == off[s + 1]                         # unreachable: empty
    off2, rb2 = replacement_table(table, {2: b"CD", 3: b"last"})
    assert (off2 == off).all() and rb2 == rb
    assert off.dtype == np.uint32 and off.size == table.num_final + 1


def test_replacement_table_charclass():
    table = PfacTable.from_charclass(b"[a-c]x\nax\n[a-c]\n", 256)
    off, rb = replacement_table(table, {1: b"one", 2: b"two", 3: b"three"})
    reps = {1: b"one", 2: b"two", 3: b"three"}
    multi = False
    for s in range(table.num_final):
        ids = table.out_ids[table.out_first[s]:table.out_first[s + 1]]
        if ids.size:
            assert rb[off[s]:off[s + 1]] == reps[int(ids.min())]
            multi |= ids.size > 1
    assert multi                                                # "ax" stands for patterns 1 and 2


def test_replacement_table_missing_id():
    table = PfacTable.from_bytes(b"ab\ncd\nef\nab\n")
    with pytest.raises(ValueError, match="pattern id 2"):
        replacement_table(table, {3: b"x", 4: b"y"})
    with pytest.raises(ValueError, match="pattern id 3"):
        replacement_table(table, [b"a", b"b"])
    replacement_table(table, {2: b"", 3: b"", 4: b""})         # id 1 lost to id 4: not needed
