"""The host references of tests/tplref.py held against each other, against tests/replref.py and against the input
itself (no GPU); `template_table`; and the pick counts of the named inputs that tests/test_gpu_templates.py runs, so
that no GPU case passes by being empty."""
import os

import numpy as np
import pytest

import tplref
from llref import line_lengths
from orc import Oracle
from phfpfac_amd import PfacTable
from phfpfac_amd.table import TEMPLATE_PLAIN, replacement_table, template_table
from replref import greedy_replace, rep_table

HERE = os.path.dirname(os.path.abspath(__file__))
PARA = open(os.path.join(HERE, "golden", "data", "paragraph402"), "rb").read()


def write_patterns(tmp_path, pats, name="p.pat"):
    f = tmp_path / name
    f.write_bytes(b"".join(p + b"\n" for p in pats))
    return str(f)


def records(path, data, fold=False):
    o = Oracle(path, 1, 1)
    pos, ids = o.scan_spec(np.ascontiguousarray(data))
    o.close()
    return pos, line_lengths(path)[ids], ids


def seeded_case(seed, tmp_path, fold=False):
    rng = np.random.default_rng(seed)
    words = sorted({w for w in PARA.split() if 1 <= len(w) <= 9})
    pats = [words[i] for i in rng.choice(len(words), 25, replace=False)]
    pats += [p[:2] for p in pats[:8] if len(p) > 3] + [pats[0]]                 # prefixes, and a duplicate line
    if fold:
        pats = [p.lower() for p in pats]
    tpl = {}
    for i in range(1, len(pats) + 1):
        r = bytes(rng.integers(33, 127, int(rng.integers(0, 14))).astype(np.uint8))
        tpl[i] = r if rng.random() < 0.3 else (r[:int(rng.integers(0, len(r) + 1))], bytes(rng.integers(33, 127, int(rng.integers(0, 5))).astype(np.uint8)))
    n = int(rng.integers(3000, 9000))
    data = np.frombuffer((PARA * (n // len(PARA) + 2))[int(rng.integers(0, 300)):][:n], dtype=np.uint8).copy()
    if fold:
        lower = (data >= 0x61) & (data <= 0x7A)
        data[lower & (rng.random(n) < 0.5)] &= 0xDF
    return pats, tpl, data, write_patterns(tmp_path, pats, f"s{seed}.pat"), rng


def equal(a, b):
    assert (a.replaced, a.extracted, a.exit, a.n_picks) == (b.replaced, b.extracted, b.exit, b.n_picks)
    assert np.array_equal(a.pick_off, b.pick_off) and int(a.pick_off[-1]) == len(a.extracted) and a.pick_off.size == a.n_picks + 1


@pytest.mark.parametrize("seed", range(6))
def test_loop_against_re(seed, tmp_path):
    pats, tpl, data, path, rng = seeded_case(seed, tmp_path)
    rec = records(path, data)
    picks = 0
    for n_owned, entry in [(data.size, 0), (data.size - 1, 1), (data.size - 6, 6)] + [
            (int(rng.integers(1, data.size)), int(rng.integers(0, 12))) for _ in range(4)]:
        a = tplref.from_records(data, entry, n_owned, *rec, tpl)
        equal(a, tplref.re_templates(pats, tpl, data, entry, n_owned))
        picks += a.n_picks
    assert picks > 500


@pytest.mark.parametrize("seed", range(3))
def test_loop_against_re_ignore_case(seed, tmp_path):
    """The folded scan is the oracle on the folded patterns and the folded input; the templates quote the input as it
    was written."""
    pats, tpl, data, path, rng = seeded_case(100 + seed, tmp_path, fold=True)
    folded = data.copy()
    folded[(folded >= 0x41) & (folded <= 0x5A)] |= 0x20
    rec = records(path, folded)
    a = tplref.from_records(data, 2, data.size - 3, *rec, tpl)
    equal(a, tplref.re_templates(pats, tpl, data, 2, data.size - 3, ignore_case=True))
    assert a.n_picks > 100 and a.extracted != tplref.from_records(folded, 2, data.size - 3, *rec, tpl).extracted


@pytest.mark.parametrize("seed", range(4))
def test_templates_are_fixed_replacements_for_exact_case_literals(seed, tmp_path):
    """prefix + pattern + suffix as a fixed replacement writes what the template writes: (a) against
    replref.greedy_replace.  (The timing baseline of tools/template_bench.py rests on this.)"""
    pats, tpl, data, path, rng = seeded_case(200 + seed, tmp_path)
    rec = records(path, data)
    fixed = rep_table(tplref.fixed_replacements(pats, tpl))
    for n_owned, entry in ((data.size, 0), (data.size - 4, 3)):
        a = tplref.from_records(data, entry, n_owned, *rec, tpl)
        out, ex = greedy_replace(data, entry, n_owned, *rec, fixed)
        assert bytes(out) == a.replaced and ex == a.exit


@pytest.mark.parametrize("seed", range(3))
def test_empty_templates_are_the_identity(seed, tmp_path):
    pats, _, data, path, rng = seeded_case(300 + seed, tmp_path)
    rec = records(path, data)
    tpl = {i: (b"", b"") for i in range(1, len(pats) + 1)}
    for n_owned, entry in ((data.size, 0), (data.size - 4, 3), (int(data.size // 2), 1)):
        a = tplref.from_records(data, entry, n_owned, *rec, tpl)
        assert a.replaced == bytes(data[entry:n_owned + a.exit])
        assert a.n_picks > 50 and len(a.extracted) < len(a.replaced)


# ---------------------------------------------------------------------------
def test_template_table_through_idmap(tmp_path):
    pats = [b"ab", b"abc", b"ab", b"zz"]                                       # line 3 repeats line 1: one state, the winner's id
    path = write_patterns(tmp_path, pats)
    table = PfacTable.from_file(path, 256)
    tpl = {1: b"first", 2: (b"<", b">"), 3: (b"[[", b"]"), 4: b""}
    offsets, splits, blob = template_table(table, tpl)
    lens = table.final_lengths()
    assert offsets.dtype == np.uint32 and splits.dtype == np.uint32 and offsets.size == table.num_final + 1 == splits.size + 1
    seen = {}
    for s in range(int(table.num_final)):
        r = blob[int(offsets[s]):int(offsets[s + 1])]
        if lens[s] < 1:
            assert r == b"" and splits[s] == TEMPLATE_PLAIN
            continue
        i = int(table.idmap[s])
        want = tplref.by_id(tpl)[i]
        if isinstance(want, bytes):
            assert r == want and splits[s] == TEMPLATE_PLAIN
        else:
            assert r == want[0] + want[1] and splits[s] == len(want[0])
        seen[i] = s
    assert sorted(seen) in ([1, 2, 4], [2, 3, 4])                           # one of the duplicate lines has no state
    # a sequence, one entry per line; plain templates alone are replacement_table
    seq = [b"x", b"yy", b"x", b""]
    o2, s2, b2 = template_table(table, seq)
    o1, b1 = replacement_table(table, seq)
    assert np.array_equal(o1, o2) and b1 == b2 and (s2 == TEMPLATE_PLAIN).all()
    with pytest.raises(ValueError, match="no template for pattern id"):
        template_table(table, {2: b"", 4: b""})
    with pytest.raises(ValueError, match="longer than"):
        template_table(table, {1: b"", 2: (b"p" * 40000, b"s" * 30000), 3: b"", 4: b""})
    with pytest.raises(ValueError, match="pair"):
        template_table(table, {1: 5, 2: b"", 3: 5, 4: b""})


def test_template_table_class_conflict():
    image = b"[ab]x\n[bc]x\nqq\n"                                             # "bx" ends in a state of ids 1 and 2
    table = PfacTable.from_charclass(image, 256)
    multi = np.flatnonzero(np.diff(table.out_first.astype(np.int64)) > 1)
    assert multi.size >= 1
    offsets, splits, blob = template_table(table, {1: (b"<", b">"), 2: (b"<", b">"), 3: b"Q"})
    s = int(multi[0])
    assert blob[int(offsets[s]):int(offsets[s + 1])] == b"<>" and splits[s] == 1
    with pytest.raises(ValueError, match="different templates"):
        template_table(table, {1: (b"<", b">"), 2: (b"<>", b""), 3: b"Q"})
    with pytest.raises(ValueError, match="different templates"):
        template_table(table, {1: b"<>", 2: (b"<>", b""), 3: b"Q"})


# ---------------------------------------------------------------------------
# the named inputs of the GPU tests

def test_worked_sets(tmp_path):
    path = write_patterns(tmp_path, [b"a", b"ab", b"bc", b"abcd"])
    data = np.frombuffer(tplref.WORKED_DATA, dtype=np.uint8)
    rec = records(path, data)
    kinds = set()
    for tpl in tplref.WORKED_SETS:
        for t in tpl.values():
            kinds.add("plain" if isinstance(t, bytes) and t else "deletion" if isinstance(t, bytes) else
                      "split0" if not t[0] else "splitR" if not t[1] else "inner")
        for entry in range(4):
            a = tplref.from_records(data, entry, data.size, *rec, tpl)
            equal(a, tplref.re_templates([b"a", b"ab", b"bc", b"abcd"], tpl, data, entry, data.size))
            assert a.n_picks == (2, 2, 2, 1)[entry]
    assert kinds == {"plain", "deletion", "split0", "splitR", "inner"}
    assert any(isinstance(t, tuple) and len(t[0]) > 4096 and t[1] for t in tplref.WORKED_SETS[0].values())
    a = tplref.from_records(data[:5], 0, 2, *records(path, data[:5]), tplref.WORKED_SETS[0])
    assert (a.replaced, a.extracted, a.exit) == (b"xabZ", b"abZ", 1)


def test_named_inputs_have_their_picks(tmp_path):
    path = write_patterns(tmp_path, tplref.COUNT_PATTERNS)
    for k in tplref.PICK_COUNTS:
        data = tplref.count_input(k)
        a = tplref.from_records(data, 0, data.size, *records(path, data), tplref.COUNT_TEMPLATES)
        assert a.n_picks == k and len(a.extracted) == 10 * k and len(a.replaced) == data.size + 8 * k
    # empty blocks: 70, 4101 and 64 deletions in a row, each run followed by a quoting pick
    path = write_patterns(tmp_path, tplref.EMPTY_PATTERNS, "e.pat")
    data = tplref.empty_blocks_input()
    pos, lens, ids = records(path, data)
    a = tplref.from_records(data, 0, data.size, pos, lens, ids, tplref.EMPTY_TEMPLATES)
    assert a.n_picks == pos.size == 70 + 4101 + 64 + 4 and a.replaced == b"pre[q]xyz[q][q][q].tail"
    run = np.diff(np.flatnonzero(np.concatenate(([True], ids == 2))))
    assert sorted(run.tolist()) == [1, 65, 71, 4102]                        # picks from one quoting pick to the next
    # edges
    path = write_patterns(tmp_path, tplref.EDGE_PATTERNS, "g.pat")
    for n in tplref.EDGE_SIZES:
        data = np.frombuffer((tplref.EDGE_PARA * (n // 17 + 1))[:n], dtype=np.uint8)
        a = tplref.from_records(data, 0, n, *records(path, data), tplref.EDGE_TEMPLATES)
        # a period holds abcdefg at 2, h at 9 and 11, bc at 12, fgh at 14: a pick counts once its last byte is there
        assert a.n_picks == (n // 17) * 5 + sum(end <= n % 17 for end in (9, 10, 12, 14)), n
    # the identity inputs
    for run in (7, 64 * 64 * 2 + 1):
        n = (1 << 16) + 3
        data = tplref.a_runs(n, run)
        p = write_patterns(tmp_path, [b"aa"], f"aa{run}.pat")
        a = tplref.from_records(data, 0, n, *records(p, data), {1: (b"", b"")})
        assert a.n_picks == tplref.aa_picks(n, run) > 0 and a.replaced == bytes(data)
    assert tplref.aa_picks((1 << 20) + 3, 7) > 390_000 and tplref.aa_picks((1 << 20) + 3, 8193) > 500_000    # the GPU's size
    # the large output: one pick per period, odd periods, both outputs past 64 MiB
    unit = np.frombuffer(tplref.BIG_UNIT, dtype=np.uint8)
    one = tplref.re_templates(tplref.BIG_PATTERNS, tplref.BIG_TEMPLATES, unit, 0, unit.size)
    two = tplref.re_templates(tplref.BIG_PATTERNS, tplref.BIG_TEMPLATES, np.tile(unit, 2), 0, 2 * unit.size)
    assert one.n_picks == 1 and two.replaced == one.replaced * 2 and two.extracted == one.extracted * 2
    assert len(one.replaced) % 2 == 1 and len(one.extracted) % 2 == 1
    assert min(len(one.replaced), len(one.extracted)) * tplref.BIG_PERIODS > 64 << 20
