"""The span reference (tests/spanref.py) over the CPU oracle's records: it is the checker of tests/test_gpu_spans.py, so
it is pinned here without a GPU -- against its own plain-loop form, against Python's `re` with re.MULTILINE for the
anchors, and in the counts the GPU cases rely on.  The host half of the feature (PfacTable.state_spans, strip_anchors)
is tested here too."""
import re

import numpy as np
import pytest

import spanref
from docref import random_offsets
from llref import line_lengths
from orc import Oracle
from phfpfac_amd import SPAN_DTYPE, PfacTable, strip_anchors
from phfpfac_amd.matcher import tiled_bytes

N = 65536 + 123
TILE = 4096
ANY = spanref.ANY
SP, W = ord(" "), ord("w")
# (pattern file, delimiter) -> (records, documents, kept under ^, $, -x, records that cross a document end, most
# document starts in a tile) of the 64 KiB + 123 bytes of paragraph402 tiled
TABLE = {("xaa+xab+xac+xad", SP): (27596, 10292, 11266, 10454, 5716, 0, 646),
         ("experimentpattern", SP): (4900, 10292, 980, 164, 164, 0, 646),
         ("xaa+xab+xac+xad", W): (27596, 818, 816, 164, 0, 1305, 53)}


@pytest.fixture(scope="module")
def text(data_dir):
    return tiled_bytes(N, open(f"{data_dir}/paragraph402", "rb").read())


@pytest.fixture(scope="module")
def scans(text, resolve):
    """name -> (pos, lens, ids) of the oracle's scan of `text`."""
    out = {}
    for name in ("experimentpattern", "xaa+xab+xac+xad"):
        path = resolve(name)
        o = Oracle(path, 1, 1)
        pos, ids = o.scan_spec(text)
        o.close()
        out[name] = (pos, line_lengths(path)[ids], ids)
    return out


@pytest.mark.parametrize("name,delim", list(TABLE))
def test_fixture_counts_and_preconditions(scans, text, name, delim):
    pos, lens, _ = scans[name]
    records, docs, head, tail, whole, cross, starts = TABLE[(name, delim)]
    off = spanref.split_offsets(text, delim)
    z, inf, any_ = np.zeros(pos.size, np.int64), np.full(pos.size, spanref.INF), np.full(pos.size, ANY)
    count = lambda a, b, t: int(spanref.filter_spans(text, pos, lens, a, b, t, delim, off).sum())   # noqa: E731
    d = np.searchsorted(off, pos, side="right") - 1
    assert (pos.size, off.size - 1) == (records, docs)
    assert (count(z, z, any_), count(z, inf, z), count(z, z, z)) == (head, tail, whole)
    assert int((pos + lens > off[d + 1]).sum()) == cross
    assert int(np.bincount(off[:-1] // TILE).max()) == starts
    # which document lookup the kernel takes: lane shuffles below 63 starts in a tile, the search in memory from there
    assert (starts >= 63) == (delim == SP)
    if name == "xaa+xab+xac+xad":
        assert np.bincount(pos // TILE).max() > 1700           # the compaction of one tile runs over many chunks


@pytest.mark.parametrize("name", ["experimentpattern", "xaa+xab+xac+xad"])
def test_drawn_rules_keep_and_drop(scans, text, resolve, name):
    pos, lens, ids = scans[name]
    rules = spanref.drawn_rules(line_lengths(resolve(name)), spanref.DRAW_SEED)
    keep = spanref.filter_spans(text, pos, lens, *spanref.record_spans(rules, ids), SP, spanref.split_offsets(text, SP))
    assert 0 < keep.sum() < pos.size
    assert {type(r) for r in rules[1:]} >= ({tuple, str} if name == "experimentpattern" else {tuple, str, type(None)})


@pytest.mark.parametrize("name", ["experimentpattern", "xaa+xab+xac+xad"])
def test_loop_form_agrees(scans, text, resolve, name):
    pos, lens, ids = scans[name]
    if pos.size > 6000:                                         # (the loop is plain Python)
        take = np.sort(np.random.default_rng(2).choice(pos.size, 6000, replace=False))
        pos, lens, ids = pos[take], lens[take], ids[take]
    rng = np.random.default_rng(5)
    n_ids = int(line_lengths(resolve(name)).size)
    differ = 0
    for seed, delim, off in ((1, SP, spanref.split_offsets(text, SP)), (2, W, spanref.split_offsets(text, W)),
                             (3, -1, random_offsets(rng, N, 300, empties=9)), (4, SP, None), (5, -1, None),
                             (6, SP, random_offsets(rng, N, 2000, empties=40))):
        r = np.random.default_rng(seed)
        rules = [None] + [(None, "^", "$", "^$", (int(r.integers(0, 9)), int(r.integers(-2, 30)), None),
                           (None, None, int(r.integers(0, 12))), (2, 40, 3))[r.integers(0, 7)] for _ in range(n_ids - 1)]
        sp = spanref.record_spans(rules, ids)
        a = spanref.filter_spans(text, pos, lens, *sp, delim, off)
        b = spanref.filter_spans_loop(text, pos, lens, *sp, delim, off)
        assert np.array_equal(a, b)
        differ += int(0 < a.sum() < pos.size)
    assert differ >= 3                                          # (a handful of rules in one document may keep nothing)


def lines_text(seed, terminated):
    rng = np.random.default_rng(seed)
    words = [b"the", b"cat", b"a", b"mat", b"he", b"at", b"on", b"that"]
    lines = [b" ".join(words[k] for k in rng.integers(0, len(words), rng.integers(0, 5))) for _ in range(400)]
    lines += [b"a cat", b"the cat", b"cat"]
    return b"\n".join(lines) + (b"\n" if terminated else b"")


@pytest.mark.parametrize("terminated", [True, False])
def test_anchors_equal_re_multiline(tmp_path, terminated):
    """^pat, pat$, ^pat$ and a free pattern: the kept (start, id) pairs are those of re.MULTILINE, one lookahead-wrapped
    alternative per pattern line (so that overlapping matches are all found)."""
    anchored = [b"^the", b"cat$", b"^a cat$", b"at", b"^he", b"mat$", b"^on$", b"hat", b"^the cat", b"on a$", b"^that$", b"t"]
    lines, rules = strip_anchors(anchored)
    assert len(set(lines)) == len(lines)                        # (one literal, one final state, one rule)
    pf = tmp_path / "p.pat"
    pf.write_bytes(b"".join(p + b"\n" for p in lines))
    raw = lines_text(3, terminated)
    assert raw.endswith(b"\n") == terminated and not raw.endswith(b"\n\n")
    buf = np.frombuffer(raw, dtype=np.uint8)
    o = Oracle(str(pf), 1, 1)
    pos, ids = o.scan_spec(buf)
    o.close()
    lens = line_lengths(str(pf))[ids]
    keep = spanref.filter_spans(buf, pos, lens, *spanref.record_spans(rules, ids), 10, spanref.split_offsets(buf, 10))
    got = set(zip(pos[keep].tolist(), ids[keep].tolist()))
    want = set()
    for i, a in enumerate(anchored, 1):
        head, tail = a.startswith(b"^"), a.endswith(b"$")
        rx = b"(?=(" + (b"^" if head else b"") + re.escape(lines[i - 1]) + (b"$" if tail else b"") + b"))"
        want |= {(m.start(), i) for m in re.finditer(rx, raw, re.MULTILINE)}
    assert got == want
    assert 0 < len(want) < pos.size
    for i in range(1, len(anchored) + 1):                       # every rule keeps something and, if anchored, drops something
        kept, seen = sum(1 for _, k in want if k == i), int((ids == i).sum())
        assert 0 < kept and (kept < seen or rules[i] is None)
    # grep -x: the lines that ARE a pattern
    whole = spanref.filter_spans(buf, pos, lens, *spanref.line_spans(pos.size), 10, spanref.split_offsets(buf, 10))
    doc = np.searchsorted(spanref.split_offsets(buf, 10), pos[whole], side="right") - 1
    want_x = [k for k, l in enumerate(raw.split(b"\n")) if l in set(lines)]
    assert sorted(set(doc.tolist())) == want_x and len(want_x) > 3


def test_tail_rules_at_a_document_end():
    """tail is 0 where the match covers the delimiter, infinite where it runs across the document's end; a document of
    its delimiter alone and an empty document judge nothing wrongly."""
    buf = np.frombuffer(b"foo\n\nxfoo\nfoo", dtype=np.uint8)
    off = np.array([0, 4, 5, 5, 10, 13])
    pos = np.array([0, 0, 0, 6, 6, 7, 10])                      # foo, foo\n, foo\n\n (crosses), foo, foo\n, oo\nf (crosses), foo
    lens = np.array([3, 4, 5, 3, 4, 4, 3])
    n = pos.size
    z, inf = np.zeros(n, np.int64), np.full(n, spanref.INF)
    end = spanref.filter_spans(buf, pos, lens, z, inf, z, 10, off)
    assert end.tolist() == [True, True, False, True, True, False, True]
    assert np.array_equal(end, spanref.filter_spans_loop(buf, pos, lens, z, inf, z, 10, off))
    start = spanref.filter_spans(buf, pos, lens, z, z, np.full(n, ANY), 10, off)
    assert start.tolist() == [True, True, True, False, False, False, True]       # a crossing record's start is judged as usual
    no_delim = spanref.filter_spans(buf, pos, lens, z, inf, z, -1, off)
    assert no_delim.tolist() == [False, True, False, False, True, False, True]
    one_doc = spanref.filter_spans(buf, pos, lens, z, inf, z, 10, None)
    assert one_doc.tolist() == [False] * 6 + [True]


# ---------------------------------------------------------------------------
# the host half of the feature

def expect(rule):
    lo, hi, tail = spanref.rule_bounds(rule)
    if hi < 0:
        lo, hi = 1, 0
    return (lo, ANY if hi == spanref.INF else hi, tail, 0)


def test_state_spans_maps_through_idmap_with_duplicate_lines():
    t = PfacTable.from_bytes(b"foo\nbar\nfoo\nbaz\nquux\n")
    rules = [None, "^", "$", (5, -3, None), "^$", (3, 17, 2)]
    spans = t.state_spans(rules)
    assert spans.dtype == SPAN_DTYPE and spans.dtype.itemsize == 16 and spans.shape == (t.num_final,)
    assert (t.final_lengths() == -1).sum() == 1                 # the state of the duplicate line
    assert sorted(t.idmap.tolist()) == [1, 2, 3, 4, 5]
    for s in range(t.num_final):
        assert tuple(spans[s]) == expect(rules[t.idmap[s]]), s
    assert tuple(spans[list(t.idmap).index(3)]) == (1, 0, ANY, 0)               # a negative max_start admits no start
    assert (spans["reserved"] == 0).all()
    with pytest.raises(ValueError):
        t.state_spans(rules[:-1])
    with pytest.raises(ValueError):
        t.state_spans(rules[:-1] + ["^^"])
    with pytest.raises(ValueError):
        t.state_spans(rules[:-1] + [(0, 1 << 32, None)])


def test_state_spans_on_a_character_class_table():
    t = PfacTable.from_charclass(b"[ab]c\nac\nxy\n")
    shared = [s for s in range(t.num_final) if t.out_first[s + 1] - t.out_first[s] > 1]
    assert shared and sorted(t.out_ids[t.out_first[shared[0]]:t.out_first[shared[0] + 1]].tolist()) == [1, 2]
    spans = t.state_spans([None, "^", "^", "$"])
    assert tuple(spans[shared[0]]) == (0, 0, ANY, 0)
    for s in range(t.num_final):
        for i in t.out_ids[t.out_first[s]:t.out_first[s + 1]]:
            assert tuple(spans[s]) == expect([None, "^", "^", "$"][i])
    with pytest.raises(ValueError, match=r"1 and 2"):
        t.state_spans([None, "^", "$", None])


def test_strip_anchors():
    lines, rules = strip_anchors([b"^foo", b"bar$", b"^baz$", b"q", b"$x^", b"a^b$c"])
    assert lines == [b"foo", b"bar", b"baz", b"q", b"$x^", b"a^b$c"]
    assert rules == [None, "^", "$", "^$", None, None, None]
    for bad in (b"^", b"$", b"^$", b""):
        with pytest.raises(ValueError, match="line 2"):
            strip_anchors([b"ok", bad])
    t = PfacTable.from_bytes(b"".join(p + b"\n" for p in lines))
    assert t.state_spans(rules).shape == (t.num_final,)
