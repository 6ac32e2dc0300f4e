"""Seeded random cases for the scan and its three post-scan passes (documents, leftmost-longest selection, find-and-
replace), shared by tests/test_gpu_passes_fuzz.py and tools/fuzz.py.  Every expectation comes from the CPU oracle's
records with lengths from the pattern file's own lines (tests/llref.py, tests/replref.py, tests/docref.py) -- never
from the device or from PfacTable.final_lengths."""
import os

import numpy as np

from docref import oracle_per_doc, random_offsets
from llref import check_greedy, greedy, line_lengths
from orc import Oracle
from phfpfac_amd import PfacTable
from replref import re_replace, rep_table, splice

TILE = 4096
GROUP = 64 * TILE                       # tiles per group of the selection's tile functions
KNOBS = [{}, {"PFAC_FORCE_L2": "1"}, {"PFAC_FORCE_L2": "1", "PFAC_DENSE": "1"}, {"PFAC_DENSE": "1"}, {"PFAC_LAG": "1"},
         {"PFAC_LAG": "2"}, {"PFAC_FORCE_L2": "1", "PFAC_NO_FUSE": "1"}, {"PFAC_FORCE_L2": "1", "PFAC_NO_D1": "1"},
         {"PFAC_REC_BYTES": "4"}, {"PFAC_WIDE": "1"}, {"PFAC_FORCE_L2": "1", "PFAC_NO_NW4": "1", "PFAC_DENSE": "1"},
         {"PFAC_L2F": "0"}, {"PFAC_L2F": "2"}, {"PFAC_L2F": "3"}, {"PFAC_L2F": "3", "PFAC_FORCE_L2": "1"}, {"PFAC_NO_SECF": "1", "PFAC_FORCE_L2": "1"}, {"PFAC_NWB": "4"},
         {"PFAC_FORCE_L2": "1", "PFAC_DENSE": "1", "PFAC_D2_LOGCAP": "64"}, {"PFAC_FORCE_L2": "1", "PFAC_DENSE": "1", "PFAC_NO_DENSE2": "1"},
         {"PFAC_FORCE_L2": "1", "PFAC_DENSE": "1", "PFAC_NWB": "5"}, {"PFAC_TICKET_WAYS": "1"}, {"PFAC_TICKET_WAYS": "2"}]
KNOB_NAMES = sorted({k for d in KNOBS for k in d})
SEEDS = list(range(3 * len(KNOBS)))     # the suite's cases: every knob set three times
GREEDY_MAX = 1_000_000                   # llref.greedy (a Python loop) up to this many records, check_greedy beyond


def knob_label(knobs):
    return "+".join(f"{k[5:]}={v}" for k, v in sorted(knobs.items())) or "default"


def record_width(num_final, knobs):
    """The record width a scan of a table with num_final final states uses under `knobs` (include/pfac.h)."""
    w = 2 if num_final <= 16 else (4 if num_final <= 1 << 20 else 8)
    want = 8 if knobs.get("PFAC_WIDE") else int(knobs.get("PFAC_REC_BYTES", 0))
    return max(w, want) if want in (4, 8) else w


class Case:
    """One random case: a pattern file (with duplicate lines now and then) over a random alphabet, an input with the
    patterns planted in it, an owned range, an entry, replacements, document offsets and the cuts of a chained
    selection.  `seed` alone fixes everything; `knobs` defaults to KNOBS[seed % len(KNOBS)]."""

    def __init__(self, seed, knobs=None):
        self.seed = seed
        self.knobs = KNOBS[seed % len(KNOBS)] if knobs is None else knobs
        rng = np.random.default_rng([seed, 0x5041535346555A5A])
        alpha = int(rng.choice([2, 3, 4, 8, 26, 60, 200]))
        symbols = rng.permutation(np.array([b for b in range(256) if b != 10], dtype=np.uint8))[:alpha]
        npat = int(rng.choice([1, 3, 20, 200, 1500]))
        maxlen = int(rng.choice([1, 2, 4, 8, 14, 40])) if rng.random() < 0.85 else int(rng.integers(100, 1023))
        pats = set()
        for _ in range(npat * 3):
            if len(pats) >= npat:
                break
            L = int(rng.integers(1, maxlen + 1))
            pats.add(bytes(symbols[rng.integers(0, alpha, L)]))
        lines = sorted(pats, key=lambda x: rng.random())
        if rng.random() < 0.4:                                  # duplicate lines: unreachable final states
            for _ in range(int(rng.integers(1, 4))):
                lines.insert(int(rng.integers(0, len(lines) + 1)), lines[int(rng.integers(0, len(lines)))])
        self.alpha, self.lines = alpha, lines
        self.width = int(rng.choice([64, 256, 256, 1024]))
        n = int(rng.choice([1, 17, 4095, 4097, 70001, GROUP - 1, GROUP + 1, 300007, 2_000_003],
                           p=[.06, .06, .1, .1, .2, .14, .14, .14, .06]))
        data = symbols[rng.integers(0, alpha, n)]
        plist = sorted(pats)
        for at in rng.integers(0, max(n - 1, 1), max(n // 50, 1)):
            pt = np.frombuffer(plist[int(rng.integers(0, len(plist)))], dtype=np.uint8)
            m = min(len(pt), n - int(at))
            data[int(at):int(at) + m] = pt[:m]
        self.data = data
        self.n = n
        self.n_owned = n if rng.random() < 0.7 else int(rng.integers(0, n + 1))
        self.M = max(len(p) for p in lines)
        self.entry = int(rng.integers(0, self.M + 1))
        self.reps = self.replacements(rng)
        self.plan_passes(rng)

    def replacements(self, rng):
        """{pattern id: bytes}: 0 to 64 bytes, now and then 1 000 to 5 000."""
        reps = {}
        for i in range(1, len(self.lines) + 1):
            L = int(rng.integers(1000, 5001)) if rng.random() < 0.01 else int(rng.integers(0, 65))
            reps[i] = rng.integers(0, 256, L).astype(np.uint8).tobytes()
        return reps

    def plan_passes(self, rng):
        """Document offsets and the cuts of a chained selection over the owned range."""
        # documents: random cuts with empty documents, cuts at 4096k - 1, 4096k, 4096k + 1, runs of documents under
        # 64 bytes in some tiles
        no = self.n_owned
        off = random_offsets(rng, no, int(rng.integers(1, 400)), empties=int(rng.integers(0, 6)))
        extra = []
        for k in rng.integers(1, max(no // TILE, 1) + 1, 3):
            extra += [int(k) * TILE - 1, int(k) * TILE, int(k) * TILE + 1]
        for t in rng.integers(0, max(no // TILE, 1), int(rng.integers(0, 3))):
            c = int(t) * TILE + int(rng.integers(0, 64))
            for _ in range(int(rng.integers(50, 80))):
                c += int(rng.integers(1, 64))
                extra.append(c)
        extra = [c for c in extra if 0 <= c <= no]
        self.off = np.sort(np.concatenate([off, np.array(extra, dtype=np.uint64)]))
        # chained selection: a random cut and, where the owned range has one, a cut at a group (else tile) edge +- 1
        cuts = set()
        if no > 2:
            cuts.add(int(rng.integers(1, no)))
            unit = GROUP if no > GROUP + 1 else TILE
            if no > unit + 1:
                cuts.add(int(rng.integers(1, no // unit + 1)) * unit + int(rng.integers(-1, 2)))
        self.cuts = [0] + sorted(c for c in cuts if 0 < c < no) + [no]

    def describe(self):
        return (f"seed {self.seed} knobs {knob_label(self.knobs)} alpha {self.alpha} lines {len(self.lines)} M {self.M} "
                f"width {self.width} n {self.n} n_owned {self.n_owned} entry {self.entry} docs {self.off.size - 1} "
                f"cuts {self.cuts}")

    def write_patterns(self, path):
        with open(path, "wb") as f:
            f.write(b"".join(p + b"\n" for p in self.lines))
        return path


class Expect:
    """What the CPU says for a case (never reads the device)."""

    def __init__(self, case, path, matcher=None, lengths=None):
        """`matcher`: an object with ``Oracle.scan_spec``'s interface (tests/bigref.py); None = the CPU oracle.
        `lengths`: int64[n_lines + 1], [id] = bytes of pattern id; None = the lines of the plain pattern file `path`."""
        c = case
        self.entry, self.n_owned = c.entry, c.n_owned
        o = Oracle(path, 1, 1) if matcher is None else matcher
        pos, ids = o.scan_spec(c.data, None)
        own = pos < c.n_owned                       # (the rest of the buffer is halo: read, not scanned from)
        self.pos, self.ids = pos[own], ids[own]
        self.docs = oracle_per_doc(o, c.data, c.off)
        if matcher is None:
            o.close()
        self.ll = line_lengths(path) if lengths is None else np.asarray(lengths, dtype=np.int64)
        self.lens = self.ll[self.ids]
        if self.pos.size <= GREEDY_MAX:
            sel, self.exit = greedy(self.pos, self.lens, c.entry, c.n_owned)
            self.sel = (self.pos[sel], self.lens[sel], self.ids[sel])
        else:
            self.sel = None                         # pinned by check_greedy against the device's selection instead
        self.table = rep_table(c.reps)

    def check_selection(self, spos, sids):
        """Asserts that the device's selection (positions, pattern ids) is the greedy one; returns its exit."""
        slen = self.ll[sids]
        if self.sel is not None:
            np.testing.assert_array_equal(spos, self.sel[0])
            np.testing.assert_array_equal(sids, self.sel[2])
            return self.exit
        return check_greedy(self.pos, self.lens, (spos, slen), self.entry, self.n_owned)


def run_case(g_factory, case, tmp_dir, matcher=None):
    """Runs one case through scan (twice), selection, replace, documents and a chained selection, each compared bit
    for bit with the CPU (`matcher`: see Expect).  `g_factory()` -> a GpuMatcher.  Returns the number of records
    compared; raises AssertionError naming the case."""
    c = case
    path = c.write_patterns(os.path.join(tmp_dir, f"fuzz_{c.seed}.pat"))
    where = c.describe()
    try:
        return _run(g_factory, c, path, matcher)
    except AssertionError as e:
        raise AssertionError(f"{where}: {e}") from e


def _run(g_factory, c, path, matcher=None, table_factory=None, lengths=None):
    """`table_factory(path, width)` -> the PfacTable of the case (None = a plain pattern file) and `lengths` (see
    Expect) let the cases of tests/classfuzz.py, whose files are no plain lines, through the same checks."""
    table = PfacTable.from_file(path, c.width) if table_factory is None else table_factory(path, c.width)
    assert table.max_pat_len == c.M
    want = Expect(c, path, matcher, lengths)
    compared = 0
    with g_factory() as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_replacements(c.reps)
        for rep in range(2):                        # twice: the staging layout may adapt after the first scan
            rec = g.scan_bytes(c.data, c.n_owned)
            assert rec.size == want.pos.size, f"scan {rep}: {rec.size} records, want {want.pos.size}"
            np.testing.assert_array_equal(rec["pos"].astype(np.int64), want.pos, err_msg=f"scan {rep}: positions")
            np.testing.assert_array_equal(table.idmap[rec["state"]], want.ids, err_msg=f"scan {rep}: pattern ids")
            compared += rec.size
        if c.n_owned:
            assert g.scan_format()[0] == record_width(table.num_final, c.knobs), "record width"
        # selection
        n_sel, ex = g.select_leftmost_longest(c.entry)
        sel = g.selection_to_host(n_sel)
        spos, sids = sel["pos"].astype(np.int64), table.idmap[sel["state"]]
        assert ex == want.check_selection(spos, sids), "selection exit"
        compared += n_sel
        # replace
        n_out = g.replace_selection()
        out = g.replacement_to_host(n_out)
        rwant = splice(c.data, c.entry, c.n_owned, spos, want.ll[sids], sids, want.table)
        assert out.size == rwant.size, f"replace: {out.size} bytes, want {rwant.size}"
        assert np.array_equal(out, rwant), f"replace: first difference at byte {int(np.argmax(out != rwant))}"
        if table_factory is None and len(c.lines) <= 20 and c.n <= 300_007:      # (plain literal lines only)
            r2, ex2 = re_replace(c.lines, c.reps, c.data, c.entry, c.n_owned)
            assert np.array_equal(out, r2) and ex2 == ex, "replace: differs from the regular-expression reference"
        # documents of the same scan
        nd = c.off.size - 1
        g.set_doc_offsets(c.off)
        kept = g.segment_records(nd)
        first, drec = g.segment_to_host(kept, nd)
        wfirst, wpos, wids = want.docs
        assert drec.size == wpos.size, f"documents: {drec.size} records kept, want {wpos.size}"
        np.testing.assert_array_equal(first, wfirst, err_msg="documents: doc_first")
        np.testing.assert_array_equal(drec["pos"].astype(np.int64), wpos, err_msg="documents: positions")
        np.testing.assert_array_equal(table.idmap[drec["state"]], wids, err_msg="documents: pattern ids")
        compared += drec.size
        # the selection in chained calls, each with a halo of M - 1 bytes and the previous exit as its entry
        if len(c.cuts) > 2:
            halo = table.halo
            cp, cs, entry = [], [], c.entry
            for a, b in zip(c.cuts[:-1], c.cuts[1:]):
                r, entry = g.scan_leftmost_longest(np.ascontiguousarray(c.data[a:min(b + halo, c.n)]), b - a, entry)
                cp.append(r["pos"].astype(np.int64) + a)
                cs.append(table.idmap[r["state"]])
            np.testing.assert_array_equal(np.concatenate(cp), spos, err_msg="chained selection: positions")
            np.testing.assert_array_equal(np.concatenate(cs), sids, err_msg="chained selection: pattern ids")
            assert entry == ex, "chained selection: exit"
    return compared
