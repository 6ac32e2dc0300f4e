"""Replacement templates (pfac_table_set_replacement_templates) and match extraction (pfac_extract_leftmost_longest) on
the GPU (run with -m gpu on an MI355X), bit-exact against the host references of tests/tplref.py.  Expectations come
from the CPU oracle's records (oracle/charclass_oracle.py for the class table), Python's `re`, or the input itself --
never from the device.  tests/test_template_ref.py holds the two references against each other and asserts the pick
counts of the named inputs used here."""
import importlib.util
import os
import re

import numpy as np
import pytest

import nocaseref
import spanref
import tplref
import wordref
from docreplref import per_doc
from heapguard import FILLS, GuardedBuffer
from llref import greedy, line_lengths
from orc import Oracle
from passguard import Want, exact_call
from phfpfac_amd import GpuMatcher, PfacError, PfacTable, _ffi, strip_anchors
from phfpfac_amd.matcher import tiled_bytes
from phfpfac_amd.table import TEMPLATE_PLAIN, template_table

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("charclass_oracle", os.path.join(REPO, "oracle", "charclass_oracle.py"))
charclass_oracle = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(charclass_oracle)

WORKED = [b"a", b"ab", b"bc", b"abcd"]


def u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def write_patterns(tmp_path, pats, name="p.pat"):
    f = tmp_path / name
    f.write_bytes(b"".join(p + b"\n" for p in pats))
    return str(f)


def matcher_for(path, templates, width=256):
    table = PfacTable.from_file(path, width)
    g = GpuMatcher(0, 1)
    g.load_table(table)
    g.set_replacement_templates(templates)
    return g


def oracle_records(path, data):
    o = Oracle(path, 1, 1)
    pos, ids = o.scan_spec(np.ascontiguousarray(data))
    o.close()
    return pos, line_lengths(path)[ids], ids


def expected(path, templates, data, n_owned, entry):
    return tplref.from_records(data, entry, n_owned, *oracle_records(path, data), templates)


def same(got, want, what):
    got, want = bytes(got), bytes(want)
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{what}: {len(got)} bytes, want {len(want)}; first difference at {k}: "
                             f"{got[max(k - 8, 0):k + 24]!r} / {want[max(k - 8, 0):k + 24]!r}")


def check_both(g, want, data, n_owned=None, entry=0, **kw):
    """One replace and one extraction of `data` against a tplref.Result."""
    n_owned = data.size if n_owned is None else n_owned
    out, ex = g.replace(data, n_owned, entry, **kw)
    same(out, want.replaced, "replace")
    assert ex == want.exit
    ext, off, ex = g.extract(data, n_owned, entry, **kw)
    same(ext, want.extracted, "extraction")
    assert ex == want.exit and off.dtype == np.uint64 and np.array_equal(off, want.pick_off)
    return out, ext


def status_of(fn):
    with pytest.raises(PfacError) as e:
        fn()
    return e.value


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(len(tplref.WORKED_SETS)))
def test_worked_example(which, tmp_path):
    path = write_patterns(tmp_path, WORKED)
    tpl = tplref.WORKED_SETS[which]
    data = u8(tplref.WORKED_DATA)
    with matcher_for(path, tpl) as g:
        if which == 0:                                          # picks: ab at 1, abcd at 4
            out, ex = g.replace(data)
            assert (bytes(out), ex) == (b"xabZc" + b"L" * 5000 + b"abcdR", 0)
            ext, off, ex = g.extract(data)
            assert (bytes(ext), off.tolist(), ex) == (b"abZ" + b"L" * 5000 + b"abcdR", [0, 3, 5008], 0)
            out, ex = g.replace(data, entry=2)                  # bc at 2, abcd at 4
            assert (bytes(out), ex) == (b"BCbc" + b"L" * 5000 + b"abcdR", 0)
        for entry in range(4):
            want = expected(path, tpl, data, data.size, entry)
            same(want.replaced, tplref.re_templates(WORKED, tpl, data, entry, data.size).replaced, "the references")
            check_both(g, want, data, entry=entry)
        # the pick at 1 runs into the halo: emitted whole by the range that owns its start; then the chained continuation
        head = np.ascontiguousarray(data[:5])
        want = expected(path, tpl, head, 2, 0)
        assert want.exit == 1 and want.n_picks == 1
        check_both(g, want, head, n_owned=2)
        rest = np.ascontiguousarray(data[2:])
        want2 = expected(path, tpl, rest, rest.size, want.exit)
        check_both(g, want2, rest, entry=want.exit)
        whole = expected(path, tpl, data, data.size, 0)
        assert want.replaced + want2.replaced == whole.replaced and want.extracted + want2.extracted == whole.extracted


@pytest.mark.parametrize("pat,run", [(b"a", 7), (b"aa", 7), (b"aa", 64 * 64 * 2 + 1)])
def test_identity(pat, run, tmp_path):
    """Empty prefix and suffix on every state: the replace is the input slice.  `a` picks at almost every byte (sixteen
    segments in a 16-byte chunk); the extraction is the picked bytes alone."""
    path = write_patterns(tmp_path, [pat])
    n = (1 << 20) + 3
    data = tplref.a_runs(n, run)
    n_picks = int((data == ord("a")).sum()) if pat == b"a" else tplref.aa_picks(n, run)
    table = PfacTable.from_file(path, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_highlight(b"", b"")
        for n_owned, entry in ((n, 0), (n - 5, len(pat) - 1)):   # (an entry lies inside a pick: below the longest pattern)
            out, ex = g.replace(data, n_owned, entry)
            end = n_owned + ex
            assert 0 <= ex < len(pat)
            assert np.array_equal(out, data[entry:end])
        ext, off, ex = g.extract(data)
        assert ex == 0 and ext.size == n_picks * len(pat) and bytes(ext) == pat * n_picks
        assert np.array_equal(off, np.arange(n_picks + 1, dtype=np.uint64) * np.uint64(len(pat)))


def test_edges(tmp_path):
    path = write_patterns(tmp_path, tplref.EDGE_PATTERNS)
    tpl, para = tplref.EDGE_TEMPLATES, tplref.EDGE_PARA
    with matcher_for(path, tpl) as g:
        for n in tplref.EDGE_SIZES:
            data = tiled_bytes(n, para)
            rec = oracle_records(path, data)
            for n_owned in sorted({n, max(n - 1, 0), max(n - 6, 0)}):
                for entry in (0, 1, 6):
                    check_both(g, tplref.from_records(data, entry, n_owned, *rec, tpl), data, n_owned, entry)
        # a match at position 0; a match that ends exactly at n_avail, n_avail no multiple of 16 (51 = 3 x 17, 9, 26)
        for data in (tiled_bytes(70, para[2:] + para[:2]), tiled_bytes(51, para), tiled_bytes(9, para), tiled_bytes(26, para)):
            want = expected(path, tpl, data, data.size, 0)
            assert want.n_picks >= 1
            check_both(g, want, data)
        data = tiled_bytes(51, para)
        assert data.size % 16 and bytes(data[-3:]) == b"fgh"
        want = expected(path, tpl, data, 49, 0)                 # ... and it starts in the owned range, ends in the halo
        assert want.exit == 2
        check_both(g, want, data, n_owned=49)
        out, ex = g.replace(tiled_bytes(100, para), 3, 7)       # entry past n_owned
        assert out.size == 0 and ex == 4
        ext, off, ex = g.extract(tiled_bytes(100, para), 3, 7)
        assert ext.size == 0 and off.tolist() == [0] and ex == 4


@pytest.mark.parametrize("k", tplref.PICK_COUNTS)
def test_block_and_group_edges(k, tmp_path):
    path = write_patterns(tmp_path, tplref.COUNT_PATTERNS)
    data = tplref.count_input(k)
    want = expected(path, tplref.COUNT_TEMPLATES, data, data.size, 0)
    assert want.n_picks == k
    with matcher_for(path, tplref.COUNT_TEMPLATES) as g:
        check_both(g, want, data)


def test_empty_blocks(tmp_path):
    """Blocks of 64 picks that write nothing (plain deletions, no gap), then a quoting pick: rp_find gallops over them."""
    path = write_patterns(tmp_path, tplref.EMPTY_PATTERNS)
    data = tplref.empty_blocks_input()
    want = expected(path, tplref.EMPTY_TEMPLATES, data, data.size, 0)
    assert want.replaced == b"pre[q]xyz[q][q][q].tail" and want.extracted == b"[q][q][q][q]"
    with matcher_for(path, tplref.EMPTY_TEMPLATES) as g:
        check_both(g, want, data)
        check_both(g, expected(path, tplref.EMPTY_TEMPLATES, data, data.size - 8, 1), data, data.size - 8, 1)


# ---------------------------------------------------------------------------
# tables

def test_class_table_quotes_what_matched(tmp_path):
    """One final state matches different bytes at different places: only a template can write them back."""
    image = b"[a-c][0-9]x\n[Qq]uo[tT]e\n[^a-z ]![^a-z ]\n"
    text = b"a1x b7x c0x Quote quoTe qte c9x.. #!# 7!Z a!b a1 x " * 300 + b"b3x"
    data = u8(text)
    tpl = {1: (b"<", b">"), 2: (b"\"", b"\""), 3: (b"", b"")}
    pos, ids = charclass_oracle.match(image, data)
    lens = np.array([0, 3, 5, 3], dtype=np.int64)[ids]
    want = tplref.from_records(data, 0, data.size, pos, lens, ids, tpl)
    assert want.n_picks == 300 * 8 + 1 and b"<c9x>" in want.replaced and b"<b7x>" in want.replaced and b"\"quoTe\"" in want.replaced
    table = PfacTable.from_charclass(image, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_replacement_templates(tpl)
        check_both(g, want, data)
        want = tplref.from_records(data, 2, data.size - 2, pos, lens, ids, tpl)    # the last pick ends in the halo
        assert want.exit == 2 and want.n_picks == 300 * 8
        check_both(g, want, data, data.size - 2, 2)


def test_case_fold_keeps_the_callers_case():
    case = nocaseref.passes_case()
    lines = case.patterns[:-1].split(b"\n")
    tpl = {i: (b"<mark>", b"</mark>") if i % 3 else b"#" for i in range(1, len(lines) + 1)}
    pos, ids = case.want
    ll = np.array([0] + [len(x) for x in lines], dtype=np.int64)
    data = case.data
    want = tplref.from_records(data, 0, data.size, pos, ll[ids], ids, tpl)
    other = tplref.re_templates(lines, tpl, data, 0, data.size, ignore_case=True)
    assert (want.replaced, want.extracted, want.exit, want.n_picks) == (other.replaced, other.extracted, other.exit, other.n_picks)
    assert np.array_equal(want.pick_off, other.pick_off)
    quoted = re.findall(rb"<mark>(.*?)</mark>", want.replaced)
    assert any(q != q.lower() for q in quoted) and want.n_picks > 50      # the output carries upper case the matcher never saw
    table = PfacTable.from_bytes(case.patterns, 256, ignore_case=True)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_replacement_templates(tpl)
        check_both(g, want, data)


@pytest.mark.parametrize("env", [{}, {"PFAC_WIDE": "1"}, {"PFAC_FORCE_L2": "1"}], ids=["dictionary", "wide", "force-l2"])
def test_record_forms_and_l2(env, resolve, monkeypatch):
    """4-byte records (the dictionary), 8-byte (PFAC_WIDE), tables via L2."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    path = resolve("xaa+xab+xac+xad" if not env else "experimentpattern")
    data = tiled_bytes((1 << 17) + 77, open(resolve("paragraph402"), "rb").read())
    n_ids = line_lengths(path).size - 1
    rng = np.random.default_rng(5)
    tpl = {}
    for i in range(1, n_ids + 1):
        r = bytes(rng.integers(33, 127, int(rng.integers(0, 9))).astype(np.uint8))
        tpl[i] = r if i % 4 == 0 else (r[:int(rng.integers(0, len(r) + 1))], r[::-1][:3])
    want = expected(path, tpl, data, data.size - 9, 1)
    assert want.n_picks > 1000
    with matcher_for(path, tpl) as g:
        g.scan_bytes(data)
        if "PFAC_FORCE_L2" not in env:
            assert g.scan_format()[0] == (8 if env else 4)
        check_both(g, want, data, data.size - 9, 1)


# ---------------------------------------------------------------------------
# compositions

LINES_PATTERNS = [b"england", b"cricket", b"over", b"runs per over", b"team", b"the"]
LINES_TEMPLATES = {1: (b"[LOC:", b"]"), 2: (b"\x1b[31m", b"\x1b[0m"), 3: b"", 4: (b"", b"!"), 5: (b"<b>", b"</b>"), 6: b"THE"}


def lines_text(n=6 * 4096 + 77):
    text = tiled_bytes(n, open(os.path.join(HERE, "golden", "data", "paragraph402"), "rb").read()).copy()
    text[np.flatnonzero(text == ord("."))] = ord("\n")
    text[97::211] = ord("\n")
    return text


def test_behind_the_whole_word_filter(tmp_path):
    path = write_patterns(tmp_path, LINES_PATTERNS)
    data = lines_text()
    pos, lens, ids = oracle_records(path, data)
    keep = wordref.filter_words(data, pos, lens)
    assert 0 < keep.sum() < pos.size
    want = tplref.from_records(data, 0, data.size, pos[keep], lens[keep], ids[keep], LINES_TEMPLATES)
    assert want.n_picks > 100
    with matcher_for(path, LINES_TEMPLATES) as g:
        check_both(g, want, data, whole_words=True)


def test_behind_the_span_filter_and_per_line(tmp_path):
    """^ and $ rules (strip_anchors) through replace_lines / extract_lines, against `re` line by line."""
    anchored = [b"^the", b"over", b"team$", b"^a"]
    stripped, rules = strip_anchors(anchored)
    path = write_patterns(tmp_path, stripped)
    tpl = {1: (b"<", b">"), 2: (b"", b"\n"), 3: (b"[", b"]"), 4: b"A"}
    data = lines_text()
    nl = np.flatnonzero(data == ord("\n"))
    nl = nl[(nl > 8) & (nl < data.size - 8)]
    for k, word in ((3, b"the "), (5, b"a ")):                  # lines that begin with "the" / "a", lines that end in "team"
        for i in nl[k::7]:
            data[i + 1:i + 1 + len(word)] = u8(word)
    for i in nl[1::4]:
        data[i - 4:i] = u8(b"team")
    text = bytes(data)
    alt = re.compile(rb"^the|over|team$|^a")
    by_line = {b"the": 1, b"over": 2, b"team": 3, b"a": 4}
    outs, exts, first, offs = [], [], [0], [0]
    cut = spanref.split_offsets(data, ord("\n"))
    for line in (text[int(a):int(b)] for a, b in zip(cut[:-1], cut[1:])):
        body = line[:-1] if line.endswith(b"\n") else line
        ms = list(alt.finditer(body))
        rw = [tplref.rewrite(tpl[by_line[m.group(0)]], m.group(0)) for m in ms]
        c, o = 0, []
        for m, e in zip(ms, rw):
            o += [line[c:m.start()], e]
            c = m.end()
        outs.append(b"".join(o) + line[c:])
        exts.append(b"".join(rw))
        first.append(first[-1] + len(ms))
        for e in rw:
            offs.append(offs[-1] + len(e))
    assert first[-1] > 50 and any(b"<the>" in o for o in outs) and any(b"[team]" in o for o in outs)
    with matcher_for(path, tpl) as g:
        g.set_pattern_spans(rules)
        out_off, out, off = g.replace_lines(data, spans=True)
        same(out, b"".join(outs), "replace_lines")
        assert np.array_equal(out_off, np.concatenate(([0], np.cumsum([len(o) for o in outs]))).astype(np.uint64))
        ext, pick_off, doc_first = g.extract_lines(data, spans=True)
        same(ext, b"".join(exts), "extract_lines")
        assert np.array_equal(pick_off, np.array(offs, dtype=np.uint64)) and np.array_equal(doc_first, np.array(first, dtype=np.uint64))
        for d in (0, 1, len(exts) // 2, len(exts) - 1):         # the doc_first slicing rule
            assert bytes(ext[int(pick_off[int(doc_first[d])]):int(pick_off[int(doc_first[d + 1])])]) == exts[d]


def test_documents_and_lines(tmp_path):
    """replace_documents / replace_lines with templates against docreplref.per_doc's selection, every document's output
    from tplref; grep -o (set_highlight(b"", b"\\n") + extract_lines) against re.finditer per line."""
    path = write_patterns(tmp_path, LINES_PATTERNS)
    data = lines_text()
    ll = line_lengths(path)
    off = spanref.split_offsets(data, ord("\n")).astype(np.uint64)
    o = Oracle(path, 1, 1)
    sfirst, spos, sids, _, _ = per_doc(o, data, off, ll)
    o.close()
    outs, exts = [], []
    for d in range(off.size - 1):
        a, b = int(off[d]), int(off[d + 1])
        k0, k1 = int(sfirst[d]), int(sfirst[d + 1])
        r = tplref.assemble(data[a:b], 0, b - a, spos[k0:k1], ll[sids[k0:k1]], sids[k0:k1], LINES_TEMPLATES)
        outs.append(r.replaced)
        exts.append(r.extracted)
    want_off = np.concatenate(([0], np.cumsum([len(x) for x in outs]))).astype(np.uint64)
    assert int(sfirst[-1]) > 100
    with matcher_for(path, LINES_TEMPLATES) as g:
        out_off, out, offsets = g.replace_lines(data)
        assert np.array_equal(offsets, off) and np.array_equal(out_off, want_off)
        same(out, b"".join(outs), "replace_lines")
        docs = [bytes(data[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])]
        out_off, out = g.replace_documents(docs)
        assert np.array_equal(out_off, want_off)
        same(out, b"".join(outs), "replace_documents")
        ext, pick_off, doc_first = g.extract_lines(data)
        same(ext, b"".join(exts), "extract_lines")
        assert np.array_equal(doc_first, sfirst) and int(pick_off[-1]) == ext.size
        # grep -o
        g.set_highlight(b"", b"\n")
        ext, pick_off, doc_first = g.extract_lines(data)
        alt = re.compile(b"|".join(re.escape(p) for p in sorted(LINES_PATTERNS, key=len, reverse=True)))
        grep_o = [b"".join(m.group(0) + b"\n" for m in alt.finditer(line)) for line in docs]
        same(ext, b"".join(grep_o), "grep -o")
        for d in (0, 3, len(docs) - 1):
            assert bytes(ext[int(pick_off[int(doc_first[d])]):int(pick_off[int(doc_first[d + 1])])]) == grep_o[d]


# ---------------------------------------------------------------------------
def test_large_output_past_64_mib(tmp_path):
    """write_grid's wins = 4 regime: one pick per period, an odd output length per period (the 16-byte phase rotates)."""
    import torch
    path = write_patterns(tmp_path, tplref.BIG_PATTERNS)
    unit, k = tplref.BIG_UNIT, tplref.BIG_PERIODS
    one = tplref.re_templates(tplref.BIG_PATTERNS, tplref.BIG_TEMPLATES, u8(unit), 0, len(unit))
    assert one.n_picks == 1 and len(one.replaced) % 2 == 1 and len(one.extracted) % 2 == 1
    assert len(one.replaced) * k > 64 << 20 and len(one.extracted) * k > 64 << 20
    data = np.tile(u8(unit), k)
    with matcher_for(path, tplref.BIG_TEMPLATES) as g:
        g._ensure_final_lengths()
        g.reserve(0, data.size, max(data.size // 8, 4096))
        g.h2d(data, 0)
        g.scan_resident(data.size, data.size)
        n_sel, ex = g.select_leftmost_longest(0)
        assert (n_sel, ex) == (k, 0)
        for what, piece, call, fetch in (("replace", one.replaced, g.replace_selection, g.replacement_to_host),
                                         ("extraction", one.extracted, g.extract_selection, g.extracted_to_host)):
            n = call()
            assert n == len(piece) * k, what
            got = torch.from_numpy(fetch(n))
            tiled = torch.from_numpy(u8(piece).copy()).repeat(k)
            assert torch.equal(got, tiled), what
        off = g.extract_offsets_to_host(n_sel)
        assert np.array_equal(off, np.arange(k + 1, dtype=np.uint64) * np.uint64(len(one.extracted)))


def test_chaining_equals_one_shot(resolve, tmp_path):
    para = open(resolve("paragraph402"), "rb").read()
    words = sorted({w for w in para.split() if 2 <= len(w) <= 12})
    pats = words + [w[:3] for w in words if len(w) > 5]
    path = write_patterns(tmp_path, pats)
    data = np.fromfile(resolve("1M"), dtype=np.uint8)[:200_000]
    halo = PfacTable.from_file(path, 256).halo
    rng = np.random.default_rng(11)
    tpl = {}
    for i in range(1, len(pats) + 1):
        r = bytes(rng.integers(33, 127, int(rng.integers(0, 30))).astype(np.uint8))
        tpl[i] = r if i % 5 == 0 else (r[:len(r) // 2], r[len(r) // 2:])
    pos, lens, ids = oracle_records(path, data)
    want = tplref.from_records(data, 0, data.size, pos, lens, ids, tpl)
    sel, _ = greedy(pos, lens, 0, data.size)
    long_picks = sel[lens[sel] > 2]
    assert long_picks.size > 100
    with matcher_for(path, tpl) as g:
        check_both(g, want, data)
        for trial in range(3):
            k = int(rng.integers(2, 5))
            if trial < 2:                                       # cuts inside picks
                cuts = sorted(set(int(pos[i]) + 1 + trial for i in rng.choice(long_picks, k)))
            else:
                cuts = sorted(set(int(c) for c in rng.integers(1, data.size, k)))
            bounds = [0] + cuts + [data.size]
            for fn in ("replace", "extract"):
                parts, offs, entry, base = [], [np.zeros(1, dtype=np.uint64)], 0, 0
                for a, b in zip(bounds[:-1], bounds[1:]):
                    piece = np.ascontiguousarray(data[a:min(data.size, b + halo)])
                    got = getattr(g, fn)(piece, b - a, entry)
                    entry = got[-1]
                    parts.append(bytes(got[0]))
                    if fn == "extract":                         # the caller rebases the offsets
                        offs.append(got[1][1:] + np.uint64(base))
                        base += got[0].size
                same(b"".join(parts), want.replaced if fn == "replace" else want.extracted, f"chained {fn}")
                assert entry == want.exit
                if fn == "extract":
                    assert np.array_equal(np.concatenate(offs), want.pick_off)


# ---------------------------------------------------------------------------
# contracts

def test_setter_errors_leave_the_templates_in_force(tmp_path):
    path = write_patterns(tmp_path, WORKED)
    data = u8(tplref.WORKED_DATA * 50)
    tpl = tplref.WORKED_SETS[1]
    table = PfacTable.from_file(path, 256)
    want = expected(path, tpl, data, data.size, 0)
    nf = int(table.num_final)
    with GpuMatcher(0, 1) as g:
        L = g._L
        off0 = np.zeros(nf + 1, dtype=np.uint32)
        assert L.pfac_table_set_replacement_templates(g._ctx, off0.ctypes.data, None, nf, None, 0) == _ffi.PFAC_E_STATE   # no table
        g.load_table(table)
        g.set_replacement_templates(tpl)
        offsets, splits, blob = template_table(table, tpl)
        buf = u8(blob)

        def call(off=offsets, spl=splits, n=nf, bytes_=buf, n_bytes=None):
            return L.pfac_table_set_replacement_templates(g._ctx, off.ctypes.data, None if spl is None else spl.ctypes.data, n,
                                                          None if bytes_ is None else bytes_.ctypes.data,
                                                          len(blob) if n_bytes is None else n_bytes)
        refused = []
        refused.append(call(n=nf - 1))                          # one state short
        refused.append(L.pfac_table_set_replacement_templates(g._ctx, None, splits.ctypes.data, nf, buf.ctypes.data, len(blob)))
        refused.append(call(bytes_=None))                       # bytes missing
        refused.append(call(n_bytes=1 << 32))
        d = offsets.copy(); d[1], d[2] = d[2] + 1, d[1]         # descending
        refused.append(call(off=d))
        refused.append(call(n_bytes=int(offsets[-1]) - 1))      # offsets past n_bytes
        long_off = np.zeros(nf + 1, dtype=np.uint32); long_off[1:] = 70000
        refused.append(call(off=long_off, bytes_=np.zeros(70000, dtype=np.uint8), n_bytes=70000))    # above PFAC_MAX_REPLACEMENT
        quoting = int(np.flatnonzero(splits != TEMPLATE_PLAIN)[0])
        s = splits.copy(); s[quoting] = offsets[quoting + 1] - offsets[quoting] + 1                   # split past R
        refused.append(call(spl=s))
        s = splits.copy(); s[quoting] = 0xFFFFFFFE
        refused.append(call(spl=s))
        assert refused == [_ffi.PFAC_E_ARG] * len(refused)
        check_both(g, want, data)                               # the earlier templates are still in force
        # splits NULL = every state plain = pfac_table_set_replacements
        assert call(spl=None) == 0
        plain = {i: tplref.rewrite(t, b"") for i, t in tplref.by_id(tpl).items()}
        check_both(g, expected(path, plain, data, data.size, 0), data)
        g.set_replacement_templates(tpl)
        check_both(g, want, data)
        g.set_replacements(plain)                               # pfac_table_set_replacements clears the splits
        check_both(g, expected(path, plain, data, data.size, 0), data)
        g.set_replacement_templates(tpl)
        g.load_table(table)                                     # a table upload drops replacements and splits
        g.scan_leftmost_longest(data)
        assert status_of(lambda: g.replace_selection()).status == _ffi.PFAC_E_STATE
        assert status_of(lambda: g.extract_selection()).status == _ffi.PFAC_E_STATE
        g.set_replacements(plain)
        check_both(g, expected(path, plain, data, data.size, 0), data)      # ... plain, not the old splits


def test_extraction_preconditions_and_outputs_of_their_own(tmp_path):
    import torch
    path = write_patterns(tmp_path, WORKED)
    data = u8(tplref.WORKED_DATA * 100)
    tpl = tplref.WORKED_SETS[1]
    table = PfacTable.from_file(path, 256)
    want = expected(path, tpl, data, data.size, 0)
    E = lambda fn: status_of(fn).status                                     # noqa: E731
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        assert E(lambda: g.extracted_to_host(1)) == _ffi.PFAC_E_STATE           # no extraction yet
        assert E(lambda: g.extract_selection()) == _ffi.PFAC_E_STATE            # no scan, no selection
        g.scan_leftmost_longest(data)
        assert E(lambda: g.extract_selection()) == _ffi.PFAC_E_STATE            # no replacements
        g.set_replacement_templates(tpl)
        g.scan_bytes(data)
        assert E(lambda: g.extract_selection()) == _ffi.PFAC_E_STATE            # no selection since the scan
        recs, _ = g.scan_leftmost_longest(data)
        n_sel = recs.size
        d_out = torch.zeros(len(want.extracted) + 64, dtype=torch.uint8, device="cuda:0")
        d_off = torch.zeros(n_sel + 2, dtype=torch.int64, device="cuda:0")
        assert E(lambda: g.extract_selection(d_out=d_out[1:], out_cap=d_out.numel())) == _ffi.PFAC_E_ARG
        assert E(lambda: g.extract_selection(d_pick_offsets=d_off.view(torch.uint8)[4:])) == _ffi.PFAC_E_ARG
        e = status_of(lambda: g.extract_selection(d_out=d_out, out_cap=len(want.extracted) - 1, d_pick_offsets=d_off))
        assert e.status == _ffi.PFAC_E_OVERFLOW and e.out_bytes == len(want.extracted)
        g.sync()
        assert int(d_out.count_nonzero()) == 0 and int(d_off.count_nonzero()) == 0      # nothing written
        # slot-owned outputs: a replace and an extraction do not invalidate each other's
        n_ext = g.extract_selection()
        n_rep = g.replace_selection()
        same(g.extracted_to_host(n_ext), want.extracted, "the extraction behind a replace")
        assert np.array_equal(g.extract_offsets_to_host(n_sel), want.pick_off)
        n_ext = g.extract_selection()
        same(g.replacement_to_host(n_rep), want.replaced, "the replace behind an extraction")
        # a caller's buffers: the slot-owned fetches then refuse
        n = g.extract_selection(d_out=d_out, out_cap=d_out.numel(), d_pick_offsets=d_off)
        g.sync()
        same(d_out.cpu().numpy()[:n], want.extracted, "the caller's d_out")
        assert np.array_equal(d_off.cpu().numpy()[:n_sel + 1].astype(np.uint64), want.pick_off) and int(d_off[n_sel + 1]) == 0
        assert E(lambda: g.extracted_to_host(1)) == _ffi.PFAC_E_STATE
        assert E(lambda: g.extract_offsets_to_host(n_sel)) == _ffi.PFAC_E_STATE
        same(g.replacement_to_host(n_rep), want.replaced, "the replace behind a caller's extraction")
        # no picks: zero bytes, pick_off[0] = 0
        ext, off, ex = g.extract(u8(b"zzzz"))
        assert ext.size == 0 and off.tolist() == [0] and ex == 0


# ---------------------------------------------------------------------------
# guards

GUARD_PATTERNS = [b"the", b"he", b"and", b"in", b"ing", b"that"]
GUARD_TEMPLATES = {1: (b"", b""), 2: b"", 3: (b"&", b""), 4: (b"<", b">"), 5: b"ING", 6: (b"", b"!")}


@pytest.mark.parametrize("fill", FILLS)
def test_guarded_exact_capacity(fill, resolve, tmp_path):
    """d_out and d_pick_offsets as GuardedBuffers of exactly the bytes the ABI names, through passguard.exact_call: one
    too small is refused with the exact size and nothing written, the exact capacity delivers the CPU's bytes with the
    guards intact.  n_owned walks down until the output sizes have met every residue mod 16, for the extraction and
    for the templated replace."""
    import torch
    path = write_patterns(tmp_path, GUARD_PATTERNS)
    text = tiled_bytes(3 * 4096 + 64, open(resolve("paragraph402"), "rb").read())
    rec = oracle_records(path, text)
    seen = {"extract": set(), "replace": set()}
    with matcher_for(path, GUARD_TEMPLATES) as g:
        d_in = torch.from_numpy(text.copy()).to("cuda:0")
        torch.cuda.synchronize()
        g._ensure_final_lengths()
        g.reserve(0, 0, 1 << 16)
        n_owned = text.size - 64
        while (len(seen["extract"]) < 16 or len(seen["replace"]) < 16) and n_owned > 2 * 4096:
            want = tplref.from_records(text, 0, n_owned, *rec, GUARD_TEMPLATES)
            new = {"extract": len(want.extracted) % 16 not in seen["extract"], "replace": len(want.replaced) % 16 not in seen["replace"]}
            if new["extract"] or new["replace"]:
                g.scan_resident(n_owned, text.size, d_input=d_in)
                n_sel, ex = g.select_leftmost_longest(0)
                assert (n_sel, ex) == (want.n_picks, want.exit)
            if new["extract"]:
                buf = {"d_out": GuardedBuffer(len(want.extracted), fill=fill), "d_pick_offsets": GuardedBuffer((n_sel + 1) * 8, fill=fill)}

                def call(cap, bad=None):
                    try:
                        return 0, g.extract_selection(d_input=d_in, d_out=buf["d_out"].ptr, out_cap=cap, d_pick_offsets=buf["d_pick_offsets"].ptr)
                    except PfacError as e:
                        return e.status, getattr(e, "out_bytes", None)
                exact_call(g, call, Want(len(want.extracted), {"d_out": u8(want.extracted), "d_pick_offsets": want.pick_off}),
                           buf, fill, f"pfac_extract_leftmost_longest n_owned {n_owned}")
                seen["extract"].add(len(want.extracted) % 16)
            if new["replace"]:
                buf = {"d_out": GuardedBuffer(len(want.replaced), fill=fill)}

                def call(cap, bad=None):
                    try:
                        return 0, g.replace_selection(d_input=d_in, d_out=buf["d_out"].ptr, out_cap=cap)
                    except PfacError as e:
                        return e.status, getattr(e, "out_bytes", None)
                exact_call(g, call, Want(len(want.replaced), {"d_out": u8(want.replaced)}), buf, fill,
                           f"templated pfac_replace_leftmost_longest n_owned {n_owned}")
                seen["replace"].add(len(want.replaced) % 16)
            n_owned -= 1
    assert len(seen["extract"]) == 16 and len(seen["replace"]) == 16


def test_determinism(resolve):
    path = resolve("xaa+xab+xac+xad")
    data = np.fromfile(resolve("bytefile/1000000byte"), dtype=np.uint8)
    table = PfacTable.from_file(path, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.set_highlight(b"<mark>", b"</mark>")
        a, _ = g.replace(data)
        b, _ = g.replace(data)
        x, xo, _ = g.extract(data)
        y, yo, _ = g.extract(data)
    assert a.size > data.size and bytes(a) == bytes(b) and x.size > 0 and bytes(x) == bytes(y) and np.array_equal(xo, yo)
