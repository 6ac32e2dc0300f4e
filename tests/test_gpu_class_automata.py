"""The scan and every post-scan pass on automata no literal pattern file can produce: tables built from character
classes (PfacTable.from_charclass) and from escaped files (PfacTable.from_file(..., escapes=True)) -- all 256 bytes as
root edges and as second bytes (newline an edge like any other), DAGs instead of tries, final states that stand for
several pattern ids, one-byte negated classes.  Run with -m gpu on an MI355X.

Every named case asserts its shape on the host (tests/classfuzz.py: shape) before it scans, and the configuration the
device reports for it (its PFAC_VERBOSE line) wherever the case is there for a threshold, so a case cannot say "256"
and run 255.  Expectations come from the brute-force matcher oracle/charclass_oracle.py, the CPU oracle's escape-aware
reader, tests/llref.py, tests/replref.py, tests/docref.py and tests/docreplref.py, with lengths from the parsed lines --
never from the device or PfacTable.final_lengths.  Bit-exact."""
import re

import numpy as np
import pytest

from classfuzz import (BIG, COLUMNS_256, SEEDS, SHAPES, ClassCase, ClassMatcher, ShapeCase, assert_text, expand, run_class_case,
                       shape, shape_brute, shape_input, shape_table)
from docref import oracle_per_doc, random_offsets
from docreplref import per_doc
from llref import greedy
from orc import Oracle
from passfuzz import KNOB_NAMES, KNOBS, _run, knob_label, record_width
from phfpfac_amd import GpuMatcher, PfacTable, emit_records_multi
from replref import rep_table

pytestmark = pytest.mark.gpu

L2 = {"PFAC_FORCE_L2": "1"}
SHAPE_KNOBS = [{}, L2, {**L2, "PFAC_DENSE": "1"}, {**L2, "PFAC_DENSE": "1", "PFAC_NO_DENSE2": "1"}, {**L2, "PFAC_NO_D1": "1"},
               {**L2, "PFAC_NO_FUSE": "1"}, {"PFAC_DENSE": "1"}, {"PFAC_WIDE": "1"},
               {**L2, "PFAC_DENSE": "1", "PFAC_REC_BYTES": "4"}]    # (4-byte records: the only way these small tables get dense mode's second form)
PASS_KNOBS = [{}, {**L2, "PFAC_DENSE": "1"}]
VERBOSE = re.compile(r"pfac: variant (\d) fused (\d) .*; dense( \(second form\))?: .*; dense rows (\d+) x (\d+), (\d+) depth-2 states, "
                     r"level-2 filter mode (\d)")


def set_knobs(monkeypatch, knobs, verbose=True):
    for k in KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    if verbose:
        monkeypatch.setenv("PFAC_VERBOSE", "1")


def install(g, table, capfd):
    """Uploads `table` and returns what the device says it configured."""
    capfd.readouterr()
    g.load_table(table)
    err = capfd.readouterr().err
    m = VERBOSE.search(err)
    assert m, f"no configuration line in {err!r}"
    return dict(variant=int(m.group(1)), fused=int(m.group(2)), second_form=bool(m.group(3)), rows=f"{m.group(4)} x {m.group(5)}",
                n2=int(m.group(6)), mode=int(m.group(7)))


def second_bytes_seen(table, data):
    """The bytes that follow a first byte (a root edge) somewhere in `data`."""
    root = table.num_final + 1
    first = np.array([table.lookup(root, b) >= 0 for b in range(256)])
    return set(np.unique(data[1:][first[data[:-1]]]).tolist())


def check_config(name, knobs, table, cfg, info):
    """The thresholds the named cases stand at: which tables keep dense depth-1 rows and with what stride, where the
    packed rows switch off, which level-2 filter form is picked."""
    d = SHAPES[name]
    l2 = "PFAC_FORCE_L2" in knobs or name in BIG
    assert info["variant"] == ("tables_via_l2" if l2 else "tables_in_lds") and cfg["variant"] == int(l2)
    fused = l2 and "PFAC_NO_FUSE" not in knobs
    assert cfg["fused"] == int(fused)
    d1 = "PFAC_NO_D1" not in knobs
    assert cfg["rows"] == (d["rows"] if d1 else "0 x 0"), "dense depth-1 rows"
    n2 = d["n2"] if fused and d1 else 0
    assert cfg["n2"] == n2, "packed rows"
    want_w = record_width(table.num_final, knobs)
    assert cfg["second_form"] == (n2 > 0 and want_w == 4 and "PFAC_NO_DENSE2" not in knobs), "dense mode's second form"
    assert cfg["mode"] == d["mode"], "level-2 filter mode"


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", SHAPE_KNOBS, ids=[knob_label(k) for k in SHAPE_KNOBS])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_scan(name, knobs, tmp_path, monkeypatch, capfd):
    """Every named automaton: shape on the host, configuration on the device, then every record of 150 001 bytes against
    the brute-force matcher (class tables: through idmap and through the outputs lists; files: also against the CPU
    oracle, escape-aware for the escaped one)."""
    set_knobs(monkeypatch, knobs)
    path = str(tmp_path / "p")
    table = shape_table(name, path)
    assert shape(table) == SHAPES[name]["shape"]
    data = shape_input(name)
    assert data.size >= 150_001
    if name in COLUMNS_256:
        assert second_bytes_seen(table, data) == set(range(256)), "the input does not put every byte behind a first byte"
    kind = SHAPES[name]["kind"]
    with GpuMatcher(0, 1) as g:
        cfg = install(g, table, capfd)
        check_config(name, knobs, table, cfg, g.info())
        rec = g.scan_bytes(data)
        assert g.scan_format()[0] == record_width(table.num_final, knobs)
    brute = shape_brute(name)
    pos, ids = brute.scan_spec(data)
    if kind != "charclass":                                     # files: the CPU oracle, and the brute force agrees with it
        o = Oracle(path, 1, 1, escapes=kind == "escaped")
        opos, oids = o.scan_spec(data)
        o.close()
        np.testing.assert_array_equal(pos, opos, err_msg="the brute-force reference and the CPU oracle: positions")
        np.testing.assert_array_equal(ids, oids, err_msg="the brute-force reference and the CPU oracle: pattern ids")
        pos, ids = opos, oids
    assert pos.size > 3000
    assert rec.size == pos.size, f"{rec.size} records, want {pos.size}"
    np.testing.assert_array_equal(rec["pos"].astype(np.int64), pos)
    np.testing.assert_array_equal(table.idmap[rec["state"]], ids)
    if kind == "charclass":
        fpos, fids = brute.full(data)
        gpos, gids = expand(table, rec["pos"], rec["state"])
        np.testing.assert_array_equal(gpos, fpos)
        np.testing.assert_array_equal(gids, fids)


@pytest.mark.parametrize("knobs", PASS_KNOBS, ids=[knob_label(k) for k in PASS_KNOBS])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_passes(name, knobs, tmp_path, monkeypatch):
    """Every pass on every named automaton: the product's final lengths, selection from entry 1, replace, documents and
    a chained selection (passfuzz._run), then select_documents and replace_documents against the per-document reference."""
    set_knobs(monkeypatch, knobs, verbose=False)
    c = ShapeCase(name, knobs)
    path = c.write_patterns(str(tmp_path / "p"))
    matcher = c.reference(path)
    try:
        n = _run(lambda: GpuMatcher(0, 1), c, path, matcher, table_factory=c.build_table, lengths=c.lens)
        assert n > 3000
        table = c.build_table(path)
        assert shape(table) == SHAPES[name]["shape"]
        pos, ids = matcher.scan_spec(c.data)
        reached = np.unique(ids)
        flen = table.final_lengths()
        hit = np.isin(table.idmap, reached)                     # final lengths: the parsed length of the state's first id
        assert hit.any() and (flen[hit] == c.lens[table.idmap[hit]]).all(), "final lengths"
        docs = (c.data[:c.n_owned], c.off)
        tab = rep_table(c.reps)
        wfirst, wpos, wids, wout_off, wout = per_doc(matcher, docs[0], c.off, c.lens, tab)
    finally:
        matcher.close()
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_replacements(c.reps)
        first, rec = g.select_documents(docs)
        np.testing.assert_array_equal(first, wfirst, err_msg="select_documents: doc_first")
        np.testing.assert_array_equal(rec["pos"].astype(np.int64), wpos, err_msg="select_documents: positions")
        np.testing.assert_array_equal(table.idmap[rec["state"]], wids, err_msg="select_documents: pattern ids")
        out_off, out = g.replace_documents(docs)
        np.testing.assert_array_equal(out_off, wout_off, err_msg="replace_documents: offsets")
        assert out.size == wout.size and np.array_equal(out, wout), "replace_documents: output"
    assert wpos.size > 1000


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS, ids=[f"s{s}-{knob_label(KNOBS[s % len(KNOBS)])}" for s in SEEDS])
def test_class_fuzz(seed, monkeypatch, tmp_path):
    """One random class or escaped case (tests/classfuzz.py): scan twice, selection, replace, documents, a chained
    selection, the full (position, id) list through the outputs lists, emit_records_multi and the GPU text emitter."""
    case = ClassCase(seed)
    set_knobs(monkeypatch, case.knobs, verbose=False)
    n = run_class_case(lambda: GpuMatcher(0, 1), case, str(tmp_path))
    print(f"case {case.describe()}: {n} records compared")


# ---------------------------------------------------------------------------
NEGATED = {"one": b"[^a]\n", "three": b"[^a]\n[^b]\nab[^c]\n"}


@pytest.mark.parametrize("knobs", [{}, {"PFAC_DENSE": "1"}, {**L2, "PFAC_DENSE": "1"}], ids=["default", "dense", "l2-dense"])
@pytest.mark.parametrize("which", sorted(NEGATED))
def test_one_byte_negated_classes(which, knobs, tmp_path, monkeypatch):
    """255 of 256 bytes are a complete match at depth 1: about one (`[^a]`) and two (`[^a]` `[^b]` `ab[^c]`) records per
    input byte of random bytes.  Count and every record, two scans (the staging adapts after the first), the outputs
    lists, and the GPU text emitter."""
    set_knobs(monkeypatch, knobs, verbose=False)
    image = NEGATED[which]
    table = PfacTable.from_charclass(image, 256)
    assert shape(table)[0] == (255 if which == "one" else 256)      # root edges; every one of them ends a pattern
    rng = np.random.default_rng(len(image))
    data = rng.integers(0, 256, 300_001).astype(np.uint8)
    at = rng.integers(0, data.size - 3, 3000)
    data[at], data[at + 1] = ord("a"), ord("b")
    brute = ClassMatcher(image)
    pos, ids = brute.scan_spec(data)
    fpos, fids = brute.full(data)                               # (`[^a]` and `[^b]` end in one state: one record, two ids)
    per_byte, ids_per_byte = pos.size / data.size, fpos.size / data.size
    assert 0.98 < per_byte < 1.02 and ((0.98 < ids_per_byte < 1.0) if which == "one" else (1.97 < ids_per_byte < 2.02)), (per_byte, ids_per_byte)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        for rep in range(2):
            rec = g.scan_bytes(data)
            assert rec.size == pos.size, f"scan {rep}: {rec.size} records, want {pos.size}"
            np.testing.assert_array_equal(rec["pos"].astype(np.int64), pos)
            np.testing.assert_array_equal(table.idmap[rec["state"]], ids)
        text = g.text_to_host(g.emit_text_device(999_999_990))
    assert_text(text, pos, ids, 999_999_990, "GPU text emitter")
    gpos, gids = expand(table, rec["pos"], rec["state"])
    np.testing.assert_array_equal(gpos, fpos)
    np.testing.assert_array_equal(gids, fids)
    out = tmp_path / "multi.txt"
    emit_records_multi(str(out), rec, table)
    assert_text(out.read_bytes(), fpos, fids, 0, "emit_records_multi")


# ---------------------------------------------------------------------------
def multi_id_states(n_final):
    """An image with n_final final states, each standing for two pattern ids or three: every word over a..d of 1 to 3
    bytes once as it is and once with its first byte as a class; every fifth a third time with a range."""
    rng = np.random.default_rng(n_final)
    words = [bytes(w) for L in (1, 2, 3) for w in np.array(np.meshgrid(*[list(b"abcd")] * L)).reshape(L, -1).T.tolist()]
    lines = []
    for k, i in enumerate(rng.permutation(len(words))[:n_final]):
        w = words[int(i)]
        lines += [w, b"[" + w[:1] + b"]" + w[1:]]
        if k % 5 == 0:
            lines.append(b"[" + w[:1] + b"-" + w[:1] + b"]" + w[1:])
    return b"".join(lines[int(i)] + b"\n" for i in rng.permutation(len(lines)))


@pytest.mark.parametrize("n_final", [16, 17, 64, 65])
def test_class_final_states_at_the_register_boundary(n_final, tmp_path, monkeypatch):
    """16 / 17 final states cross the 2-byte record boundary, 64 / 65 the lane register that holds the pattern lengths
    (documents and selection) -- here with every final state standing for several ids."""
    set_knobs(monkeypatch, {}, verbose=False)
    image = multi_id_states(n_final)
    table = PfacTable.from_charclass(image, 256)
    assert table.num_final == n_final and (np.diff(table.out_first) >= 2).all()
    brute = ClassMatcher(image)
    rng = np.random.default_rng(n_final)
    data = np.frombuffer(b"abcd", dtype=np.uint8)[rng.integers(0, 4, 300_001)]
    off = random_offsets(rng, data.size, 900, empties=5)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        got_first, got = g.scan_documents((data, off))
        assert g.scan_format()[0] == (2 if n_final <= 16 else 4)
        picks = {}
        for e in (0, 1, 3):
            n, ex = g.select_leftmost_longest(e)
            picks[e] = (g.selection_to_host(n), ex)
        rec = g.scan_bytes(data)
    wfirst, wpos, wids = oracle_per_doc(brute, data, off)
    np.testing.assert_array_equal(got_first, wfirst)
    np.testing.assert_array_equal(got["pos"].astype(np.int64), wpos)
    np.testing.assert_array_equal(table.idmap[got["state"]], wids)
    pos, ids = brute.scan_spec(data)
    assert np.unique(ids).size == n_final                       # every final state occurs
    for e, (sel, ex) in picks.items():
        s, wex = greedy(pos, brute.lens[ids], e, data.size)
        np.testing.assert_array_equal(sel["pos"].astype(np.int64), pos[s])
        np.testing.assert_array_equal(table.idmap[sel["state"]], ids[s])
        assert ex == wex
    fpos, fids = brute.full(data)
    gpos, gids = expand(table, rec["pos"], rec["state"])
    np.testing.assert_array_equal(gpos, fpos)
    np.testing.assert_array_equal(gids, fids)


# ---------------------------------------------------------------------------
NEWLINE_NUL = (b"\\na\n" b"a\\nb\n" b"ab\\n\n" b"\\x00a\n" b"a\\x00b\n" b"ab\\000\n" b"\\n\\x00\n" b"\\n\n" b"b\\n\\x00a\n")


@pytest.mark.parametrize("kind", ["charclass", "escaped"])
def test_newline_and_nul_in_patterns_and_at_document_ends(kind, tmp_path, monkeypatch):
    """Byte 10 and byte 0 as the first, a middle and the last byte of a pattern, and as the last byte of every
    document (a cut after each of them): scan, per-document records, per-document selection and replace."""
    set_knobs(monkeypatch, {}, verbose=False)
    image = NEWLINE_NUL + (b"[\\n\\x00]b\n" if kind == "charclass" else b"")
    path = tmp_path / "p"
    path.write_bytes(image)
    table = PfacTable.from_charclass(str(path), 256) if kind == "charclass" else PfacTable.from_file(str(path), 256, escapes=True)
    brute = ClassMatcher(image, "lowest" if kind == "charclass" else "last")
    root = table.num_final + 1
    assert table.lookup(root, 10) >= 0 and table.lookup(root, 0) >= 0 and table.lookup(table.lookup(root, ord("a")), 10) >= 0
    rng = np.random.default_rng(10)
    data = np.frombuffer(b"ab\n\x00", dtype=np.uint8)[rng.integers(0, 4, 200_003)]
    ends = np.flatnonzero((data == 10) | (data == 0)) + 1
    off = np.unique(np.concatenate([[0], ends[rng.random(ends.size) < 0.05], [data.size]])).astype(np.uint64)
    assert off.size > 2000
    reps = {i: bytes(rng.integers(0, 256, int(rng.integers(0, 9))).astype(np.uint8)) for i in range(1, brute.lens.size)}
    pos, ids = brute.scan_spec(data)
    if kind == "escaped":
        o = Oracle(str(path), 1, 1, escapes=True)
        opos, oids = o.scan_spec(data)
        o.close()
        np.testing.assert_array_equal(opos, pos)
        np.testing.assert_array_equal(oids, ids)
    assert set(np.unique(ids).tolist()) == set(range(1, brute.lens.size))
    wfirst, wpos, wids = oracle_per_doc(brute, data, off)
    sfirst, spos, sids, wout_off, wout = per_doc(brute, data, off, brute.lens, rep_table(reps))
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_replacements(reps)
        rec = g.scan_bytes(data)
        np.testing.assert_array_equal(rec["pos"].astype(np.int64), pos)
        np.testing.assert_array_equal(table.idmap[rec["state"]], ids)
        first, drec = g.scan_documents((data, off))
        np.testing.assert_array_equal(first, wfirst)
        np.testing.assert_array_equal(drec["pos"].astype(np.int64), wpos)
        np.testing.assert_array_equal(table.idmap[drec["state"]], wids)
        first, srec = g.select_documents((data, off))
        np.testing.assert_array_equal(first, sfirst)
        np.testing.assert_array_equal(srec["pos"].astype(np.int64), spos)
        np.testing.assert_array_equal(table.idmap[srec["state"]], sids)
        out_off, out = g.replace_documents((data, off))
        np.testing.assert_array_equal(out_off, wout_off)
        assert out.size == wout.size and np.array_equal(out, wout)
    assert wpos.size > 10_000 and spos.size > 10_000


# ---------------------------------------------------------------------------
def large_class_set(n_lines=260):
    rng = np.random.default_rng(40)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    classes = [b"[abc]", b"[a-f]", b"[^a-w]", b"[xyz0]", b"[m-p]"]
    lines = set()
    while len(lines) < n_lines:
        elems = [bytes([int(b)]) for b in letters[rng.integers(0, 26, int(rng.integers(4, 9)))]]
        for at in rng.integers(0, len(elems), int(rng.integers(1, 3))):
            elems[int(at)] = classes[int(rng.integers(0, len(classes)))]
        lines.add(b"".join(elems))
    return b"".join(ln + b"\n" for ln in sorted(lines))


def test_large_class_set_goes_through_l2_without_a_knob(tmp_path, monkeypatch):
    """A few hundred class lines: tables above the LDS limit, so the L2 variant with fused slots is what a production
    process runs for them.  2 000 003 bytes, every record and the outputs lists."""
    set_knobs(monkeypatch, {}, verbose=False)
    image = large_class_set()
    table = PfacTable.from_charclass(image, 256)
    brute = ClassMatcher(image)
    rng = np.random.default_rng(41)
    data = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0", dtype=np.uint8)[rng.integers(0, 27, 2_000_003)]
    sets = brute.parsed
    for at in rng.integers(0, data.size - 16, data.size // 150):
        p = sets[int(rng.integers(0, len(sets)))]
        data[int(at):int(at) + len(p)] = [int(rng.choice(np.flatnonzero(e & (np.arange(256) < 128)))) for e in p]
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        assert g.info()["variant"] == "tables_via_l2"
        rec = g.scan_bytes(data)
    pos, ids = brute.scan_spec(data)
    assert pos.size > 10_000 and np.unique(ids).size > 200       # (13 333 instances were planted)
    assert rec.size == pos.size
    np.testing.assert_array_equal(rec["pos"].astype(np.int64), pos)
    np.testing.assert_array_equal(table.idmap[rec["state"]], ids)
    fpos, fids = brute.full(data)
    gpos, gids = expand(table, rec["pos"], rec["state"])
    np.testing.assert_array_equal(gpos, fpos)
    np.testing.assert_array_equal(gids, fids)
