"""CPU side of the class / escaped-file fuzzer (tests/classfuzz.py): the suite's seeds reach every knob set, record
width, both front ends and the automaton shapes no literal file has; every case is well formed and parses; on a reduced
input the brute-force matcher, a host walk of the built table and (escaped files) the CPU oracle's escape-aware reader
agree; and the shape probe pins the named automata of classfuzz.SHAPES to the numbers the GPU tests rely on."""
import numpy as np
import pytest

from classfuzz import (SEEDS, SHAPES, ClassCase, ClassMatcher, assert_text, cco, cpu_walk, expand, format_lines, shape, shape_brute,
                       shape_image, shape_input, shape_table)
from orc import Oracle
from passfuzz import KNOBS, knob_label, record_width
from phfpfac_amd import PfacTable

REDUCED = 3000                              # bytes of every case's input the host walk covers


@pytest.fixture(scope="module")
def cases():
    return {s: ClassCase(s) for s in SEEDS}


def test_seeds_cover_knobs_widths_kinds_and_shapes(cases, tmp_path):
    runs, widths, kinds, seen = {}, set(), set(), {"fan 256": 0, "256 columns": 0, "256 columns in dense rows": 0, "multi-id state": 0, "negated byte": 0, "M >= 100": 0}
    for s, c in cases.items():
        cco.parse(c.image)                                      # every image parses: no case is skipped
        assert ClassCase(s).image == c.image and np.array_equal(ClassCase(s).data, c.data) if s < 3 else True
        runs[knob_label(c.knobs)] = runs.get(knob_label(c.knobs), 0) + 1
        table = c.build_table(c.write_patterns(str(tmp_path / f"p{s}")))
        assert table.max_pat_len == c.M and table.n_patterns == len(c.lines)
        widths.add(record_width(table.num_final, c.knobs))
        kinds.add(c.kind)
        assert (b"[" in c.image) <= (c.kind == "charclass")
        assert c.off[0] == 0 and c.off[-1] == c.n_owned and (np.diff(c.off.astype(np.int64)) >= 0).all()
        assert c.cuts[0] == 0 and c.cuts[-1] == c.n_owned and (all(a < b for a, b in zip(c.cuts, c.cuts[1:])) or c.cuts == [0, 0])
        assert 0 <= c.entry <= c.M and 0 <= c.n_owned <= c.n == c.data.size
        assert {0, 10} <= set(np.unique(c.data).tolist()) or c.n < 300
        fan, _, cols, _ = shape(table)
        seen["fan 256"] += fan == 256
        seen["256 columns"] += cols == 256
        if cols == 256 and fan * 256 * 4 <= 32 << 10:          # ... in a table small enough to keep dense depth-1 rows, with
            root = table.num_final + 1                          # byte 255 (the last column) behind a first byte of the input
            first = np.array([table.lookup(root, b) >= 0 for b in range(256)])
            d = c.data[:c.n_owned + 1]
            seen["256 columns in dense rows"] += bool(d.size > 1 and ((d[1:] == 255) & first[d[:-1]]).any())
        seen["multi-id state"] += c.kind == "charclass" and bool((np.diff(table.out_first) > 1).any())
        seen["negated byte"] += any(len(ln) == 1 and ln[0].sum() == 255 for ln in c.sets)
        seen["M >= 100"] += c.M >= 100
    assert sorted(runs) == sorted(knob_label(k) for k in KNOBS) and min(runs.values()) >= 2
    assert widths == {2, 4, 8} and kinds == {"charclass", "escaped"}
    assert min(seen.values()) >= 1, seen


def test_reduced_inputs_matcher_walk_and_oracle_agree(cases, tmp_path):
    compared = 0
    for s, c in cases.items():
        path = c.write_patterns(str(tmp_path / f"p{s}"))
        table = c.build_table(path)
        data = np.ascontiguousarray(c.data[:REDUCED])
        brute = c.brute()
        wpos, wst = cpu_walk(table, data)
        flen = table.final_lengths()
        if c.kind == "charclass":
            fpos, fids = brute.full(data)
            gpos, gids = expand(table, wpos, wst)
            np.testing.assert_array_equal(gpos, fpos, err_msg=c.describe())
            np.testing.assert_array_equal(gids, fids, err_msg=c.describe())
            for st in np.unique(wst):                           # every id of a reached state has the state's length
                assert (brute.lens[table.out_ids[table.out_first[st]:table.out_first[st + 1]]] == flen[st]).all(), c.describe()
        pos, ids = brute.scan_spec(data)
        np.testing.assert_array_equal(wpos, pos, err_msg=c.describe())
        np.testing.assert_array_equal(table.idmap[wst], ids, err_msg=c.describe())
        np.testing.assert_array_equal(flen[wst], brute.lens[ids], err_msg=c.describe())
        if c.kind == "escaped":
            o = Oracle(path, 1, 1, escapes=True)
            opos, oids = o.scan_spec(data)
            o.close()
            np.testing.assert_array_equal(opos, pos, err_msg=c.describe())
            np.testing.assert_array_equal(oids, ids, err_msg=c.describe())
        compared += pos.size
    assert compared > 20 * len(cases)


def test_duplicate_rules_of_the_two_front_ends(tmp_path):
    """An escaped file reports a duplicated pattern once, under its last line ('a' and '\\x61' are duplicates); a class
    file reports every id and the record carries the lowest."""
    img = b"a\nab\n\\x61\n"
    data = np.frombuffer(b"abab", dtype=np.uint8)
    (tmp_path / "p").write_bytes(img)
    o = Oracle(str(tmp_path / "p"), 1, 1, escapes=True)
    pos, ids = o.scan_spec(data)
    o.close()
    assert (pos.tolist(), ids.tolist()) == ([0, 0, 2, 2], [3, 2, 3, 2])
    last, low = ClassMatcher(img, "last"), ClassMatcher(img, "lowest")
    assert [a.tolist() for a in last.scan_spec(data)] == [[0, 0, 2, 2], [3, 2, 3, 2]]
    assert [a.tolist() for a in low.scan_spec(data)] == [[0, 0, 2, 2], [1, 2, 1, 2]]
    assert [a.tolist() for a in low.full(data)] == [[0, 0, 0, 2, 2, 2], [1, 3, 2, 1, 3, 2]]
    t = PfacTable.from_charclass(img, 256)
    wpos, wst = cpu_walk(t, data)
    assert t.idmap[wst].tolist() == [1, 2, 1, 2]
    e = PfacTable.from_file(str(tmp_path / "p"), 256, escapes=True)
    assert e.idmap[cpu_walk(e, data)[1]].tolist() == [3, 2, 3, 2]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_named_shapes(name, tmp_path):
    """(fan, depth-1 states, used columns, row entries) of every named automaton, read through PfacTable.lookup."""
    table = shape_table(name, str(tmp_path / "p"))
    assert shape(table) == SHAPES[name]["shape"]
    if name == "random-60-lines":
        assert table.num_final == 198 and int((np.diff(table.out_first) > 1).sum()) == 95


def test_a_case_that_claims_256_columns_has_them(tmp_path):
    """The probe tells 256 used columns from 255: `a[^q]` alone leaves column 'q' unused, `b[^r]` fills it; a literal
    file never gets there (no byte 10 inside a line)."""
    assert shape(PfacTable.from_charclass(b"a[^q]\n", 256)) == (1, 1, 255, 255)
    assert shape(PfacTable.from_charclass(shape_image("columns-256"), 256)) == (2, 2, 256, 510)
    assert shape(shape_table("literal-255x255", str(tmp_path / "p")))[2] == 255


@pytest.mark.parametrize("name", [k for k, d in SHAPES.items() if d["kind"] != "charclass"])
def test_brute_force_reference_of_the_file_shapes_equals_the_oracle(name, tmp_path):
    """The two named automata built from files: the brute-force reference the GPU tests use next to the CPU oracle
    (classfuzz.shape_brute) gives the oracle's records on the GPU tests' input."""
    path = str(tmp_path / "p")
    shape_table(name, path)
    data = shape_input(name)
    o = Oracle(path, 1, 1, escapes=SHAPES[name]["kind"] == "escaped")
    opos, oids = o.scan_spec(data)
    o.close()
    pos, ids = shape_brute(name).scan_spec(data)
    assert pos.size > 3000
    np.testing.assert_array_equal(pos, opos)
    np.testing.assert_array_equal(ids, oids)


def test_text_is_compared_in_full_at_any_length():
    pos, ids = np.arange(0, 3 * 450_001, 3), np.arange(450_001) % 7 + 1
    text = format_lines(pos, ids, 999_999_990)
    assert_text(text, pos, ids, 999_999_990)
    for bad in (text[:-1], text + b"\n", text[:len(text) - 40] + b"9" + text[len(text) - 39:]):
        with pytest.raises(AssertionError):
            assert_text(bad, pos, ids, 999_999_990)
