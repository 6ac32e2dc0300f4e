"""CPU side of the pass fuzzer (tests/passfuzz.py, tests/docref.py): the suite's seeds reach every knob set and every
record width, the generated cases are well formed, and the per-document reference agrees with a brute-force search."""
import numpy as np

from docref import oracle_per_doc, random_offsets
from orc import Oracle
from passfuzz import KNOBS, SEEDS, Case, knob_label, record_width
from phfpfac_amd import PfacTable


def test_seeds_cover_every_knob_set_and_record_width(tmp_path):
    runs, widths, M = {}, set(), set()
    for s in SEEDS:
        c = Case(s)
        runs[knob_label(c.knobs)] = runs.get(knob_label(c.knobs), 0) + 1
        table = PfacTable.from_file(c.write_patterns(str(tmp_path / f"p{s}")), c.width)
        assert table.max_pat_len == c.M
        widths.add(record_width(table.num_final, c.knobs))
        M.add(c.M)
        assert c.off[0] == 0 and c.off[-1] == c.n_owned and (np.diff(c.off.astype(np.int64)) >= 0).all()
        assert c.cuts[0] == 0 and c.cuts[-1] == c.n_owned and all(a < b for a, b in zip(c.cuts, c.cuts[1:]))
        assert 0 <= c.entry <= c.M and 0 <= c.n_owned <= c.n == c.data.size
    assert sorted(runs) == sorted(knob_label(k) for k in KNOBS) and min(runs.values()) >= 2
    assert widths == {2, 4, 8}
    assert max(M) >= 100 and 1 in M


def brute_per_doc(pats, buf, off):
    winner = {p: i for i, p in enumerate(pats, start=1)}
    first, recs = [], []
    for d in range(off.size - 1):
        first.append(len(recs))
        doc = bytes(buf[int(off[d]):int(off[d + 1])])
        recs += sorted((i, len(p), winner[p]) for p in winner for i in range(len(doc) - len(p) + 1)
                       if doc.startswith(p, i))
    first.append(len(recs))
    return np.array(first, dtype=np.uint64), [r[0] for r in recs], [r[2] for r in recs]


def test_oracle_per_doc_matches_brute_force(tmp_path):
    pats = [b"ab", b"b", b"abab", b"ba", b"b"]
    path = tmp_path / "p.pat"
    path.write_bytes(b"".join(p + b"\n" for p in pats))
    rng = np.random.default_rng(4)
    buf = np.frombuffer(b"ab", dtype=np.uint8)[rng.integers(0, 2, 3000)]
    off = random_offsets(rng, buf.size, 60, empties=6)
    assert off[0] == 0 and off[-1] == buf.size and off.size == 67 and (np.diff(off.astype(np.int64)) == 0).sum() >= 1
    o = Oracle(str(path), 1, 1)
    first, pos, ids = oracle_per_doc(o, buf, off)
    o.close()
    wfirst, wpos, wids = brute_per_doc(pats, buf, off)
    np.testing.assert_array_equal(first, wfirst)
    assert pos.tolist() == wpos and ids.tolist() == wids
