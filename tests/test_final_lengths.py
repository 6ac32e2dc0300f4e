"""pfac_table_final_lengths: the pattern length of every final state, computed from the table alone (the edges of the
perfect hash + s0, BFS from the root) -- what pfac_records_segment needs to drop the matches that run across a document
end.  Checked against the pattern files' own lines, for every table source."""
import importlib.util
import os

import numpy as np
import pytest

from phfpfac_amd import PfacTable

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("charclass_oracle", os.path.join(REPO, "oracle", "charclass_oracle.py"))
cco = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cco)

SETS = ["experimentpattern", "xaa", "xaa+xab+xac+xad", "bytefile/1000000byte"]


def pattern_lines(path):
    raw = open(path, "rb").read()
    assert raw.endswith(b"\n")
    return raw[:-1].split(b"\n")


def expect_lengths(table, lines):
    """Every reachable final state has its line's length; of a group of identical lines exactly one state is reachable
    (the others are the duplicates' own, unreachable states: -1)."""
    lens = table.final_lengths()
    assert lens.dtype == np.int32 and lens.size == table.num_final
    lines_of = [lines[int(i) - 1] for i in table.idmap]
    groups = {}
    for s, line in enumerate(lines_of):
        groups.setdefault(line, []).append(s)
    for line, states in groups.items():
        got = sorted(int(lens[s]) for s in states)
        assert got == [-1] * (len(states) - 1) + [len(line)], (line, states, got)
    return lens


@pytest.mark.parametrize("name", SETS)
def test_lengths_equal_the_pattern_lines(name, resolve):
    path = resolve(name)
    lines = pattern_lines(path)
    t = PfacTable.from_file(path, 256)
    lens = expect_lengths(t, lines)
    assert int(lens.max()) == t.max_pat_len
    n_dup = len(lines) - len(set(lines))
    assert int((lens == -1).sum()) == n_dup


def test_duplicate_lines_get_minus_one(tmp_path):
    pf = tmp_path / "dup.pat"
    pf.write_bytes(b"abc\nab\nabc\nx\nabc\n")
    t = PfacTable.from_file(str(pf), 256)
    lens = t.final_lengths()
    assert sorted(lens.tolist()) == [-1, -1, 1, 2, 3]
    expect_lengths(t, pattern_lines(str(pf)))


@pytest.mark.parametrize("width", [16, 256, 4096])
def test_lengths_survive_the_blob_round_trip_and_widths(width, resolve):
    path = resolve("xaa+xab+xac+xad")
    t = PfacTable.from_file(path, width)
    lens = t.final_lengths()
    expect_lengths(t, pattern_lines(path))
    t2 = PfacTable.from_blob(t.blob())
    np.testing.assert_array_equal(t2.final_lengths(), lens)
    t3 = PfacTable.from_reference_arrays(t.s0, t.r, t.HT, t.val, t.idmap, t.width, t.state_num, t.num_final, t.ht_size,
                                         t.max_pat_len)
    np.testing.assert_array_equal(t3.final_lengths(), lens)


@pytest.mark.parametrize("n_parts", [2, 3])
def test_lengths_of_partition_tables(n_parts, resolve):
    path = resolve("xaa+xab+xac+xad")
    lines = pattern_lines(path)
    for k in range(n_parts):
        t = PfacTable.from_file_part(path, 256, k, n_parts)
        lens = t.final_lengths()
        for s in range(t.num_final):
            if lens[s] != -1:
                assert lens[s] == len(lines[int(t.idmap[s]) - 1])
        reach = sorted({lines[int(i) - 1] for i in t.idmap})
        assert int((lens != -1).sum()) == len(reach)


def test_charclass_lengths_are_element_counts():
    img = (b"[a-c]x\n" b"ax\n" b"[^a-z0-9 ]\n" b"q[0-9][0-9]\n" b"[a-c]\n" b"\\x41[\\x42-\\x44]\\n\n" b"[-a]z\n"
           b"ax[xy]\n" b"[a-c]x\n")
    elems = [len(p) for p in cco.parse(img)]
    t = PfacTable.from_charclass(img, 256)
    lens = t.final_lengths()
    for s in range(t.num_final):
        ids = t.out_ids[t.out_first[s]: t.out_first[s + 1]]
        assert ids.size
        for i in ids:
            assert lens[s] == elems[int(i) - 1], (s, i)


def test_charclass_fuzz_lengths():
    rng = np.random.default_rng(7)
    atoms = [b"a", b"b", b"z", b"[ab]", b"[^a]", b"[a-c]", b"\\x61", b"[0-9a]"]
    for _ in range(30):
        img = b"".join(b"".join(atoms[int(k)] for k in rng.integers(0, len(atoms), int(rng.integers(1, 7)))) + b"\n"
                       for _ in range(int(rng.integers(1, 8))))
        elems = [len(p) for p in cco.parse(img)]
        t = PfacTable.from_charclass(img, 256)
        lens = t.final_lengths()
        for s in range(t.num_final):
            for i in t.out_ids[t.out_first[s]: t.out_first[s + 1]]:
                assert lens[s] == elems[int(i) - 1]
