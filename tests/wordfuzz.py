"""Seeded random cases for the whole-word filter, shared by tests/test_gpu_whole_words.py and tools/fuzz.py words:
pattern sets of words and phrases (some with non-word bytes at their ends), inputs that mix word and non-word bytes
with the patterns planted whole and inside longer words, random edges, word sets, neighbour bytes and document cuts.
Every expectation is the CPU oracle's records passed through tests/wordref.py, then tests/llref.py and
tests/replref.py for the passes behind the filter -- never the device's own output."""
import os

import numpy as np

import wordref
from docref import random_offsets
from llref import greedy, line_lengths
from orc import Oracle
from phfpfac_amd import PfacTable
from phfpfac_amd.matcher import word_set
from replref import rep_table, splice

TILE = 4096
KNOBS = [{}, {"PFAC_WIDE": "1"}, {"PFAC_DENSE": "1"}, {"PFAC_FORCE_L2": "1"}, {"PFAC_FORCE_L2": "1", "PFAC_DENSE": "1"},
         {"PFAC_REC_BYTES": "4"}]
KNOB_NAMES = sorted({k for d in KNOBS for k in d})
SEEDS = list(range(40))                  # the suite's cases
EDGES = {wordref.LEFT: "left", wordref.RIGHT: "right", wordref.BOTH: "both"}


class WordCase:
    """`seed` alone fixes everything; `knobs` defaults to KNOBS[seed % len(KNOBS)]."""

    def __init__(self, seed, knobs=None):
        self.seed = seed
        self.knobs = KNOBS[seed % len(KNOBS)] if knobs is None else knobs
        rng = np.random.default_rng([seed, 0x574F524453])
        letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCXYZ0123456789_\xc3\xa9\x80\xff", dtype=np.uint8)
        seps = np.frombuffer(b" \t.,;-'\"()/\x00\x7f", dtype=np.uint8)
        wl = letters[:int(rng.choice([2, 4, 26, letters.size]))]
        sp = seps[:int(rng.choice([1, 3, seps.size]))]
        # the word set: the default, the case's letters, or letters and some separators swapped
        kind = int(rng.integers(0, 3))
        if kind == 0:
            self.word_bytes = None
        elif kind == 1:
            self.word_bytes = bytes(wl)
        else:
            self.word_bytes = bytes(wl[rng.random(wl.size) < 0.7]) + bytes(sp[rng.random(sp.size) < 0.3])
        self.ws = None if self.word_bytes is None else word_set(self.word_bytes)

        def word(maxlen):
            return bytes(wl[rng.integers(0, wl.size, int(rng.integers(1, maxlen + 1)))])

        def sep():
            return bytes(sp[rng.integers(0, sp.size, 1)])

        npat = int(rng.choice([1, 4, 12, 16, 17, 60, 300]))
        pats = set()
        for _ in range(npat * 4):
            if len(pats) >= npat:
                break
            r = rng.random()
            p = word(int(rng.choice([1, 2, 3, 6, 12])))
            if r < 0.15:
                p = p + sep() + word(4)                         # a phrase
            elif r < 0.25:
                p = sep() + p                                   # unconstrained on the left
            elif r < 0.35:
                p = p + sep()                                   # ... on the right
            elif r < 0.4:
                p = sep()
            if b"\n" not in p:
                pats.add(p)
        self.lines = sorted(pats, key=lambda x: rng.random())
        self.M = max(len(p) for p in self.lines)
        self.width = int(rng.choice([64, 256, 1024]))
        n = int(rng.choice([1, 17, 4095, 4097, 12289, 70001, 64 * TILE + 1, 300007], p=[.05, .05, .1, .15, .2, .2, .15, .1]))
        plist = sorted(pats)
        parts, size = [], 0
        while size < n:
            r = rng.random()
            if r < 0.35:
                piece = plist[int(rng.integers(0, len(plist)))]                     # a pattern as a word of its own
            elif r < 0.55:
                piece = word(3) + plist[int(rng.integers(0, len(plist)))] + (word(2) if rng.random() < 0.5 else b"")
            elif r < 0.6:
                piece = plist[int(rng.integers(0, len(plist)))] * int(rng.integers(2, 40))     # a run: dense tiles
            else:
                piece = word(9)
            if rng.random() < 0.85:
                piece += sep() * int(rng.integers(1, 3))
            parts.append(piece)
            size += len(piece)
        self.data = np.frombuffer(b"".join(parts), dtype=np.uint8)[:n].copy()
        self.n = n
        self.n_owned = n if rng.random() < 0.6 else int(rng.integers(0, n + 1))
        self.edges = int(rng.choice([wordref.LEFT, wordref.RIGHT, wordref.BOTH], p=[.2, .2, .6]))
        nb = [-1, int(wl[0]), int(sp[0]), int(rng.integers(0, 256))]
        self.prev, self.next = int(rng.choice(nb)), int(rng.choice(nb))
        self.entry = int(rng.integers(0, self.M + 1))
        self.reps = {i: rng.integers(0, 256, int(rng.integers(0, 12))).astype(np.uint8).tobytes() for i in range(1, len(self.lines) + 1)}
        self.off = None
        if rng.random() < 0.5:
            no = self.n_owned
            off = random_offsets(rng, no, int(rng.integers(1, 200)), empties=int(rng.integers(0, 5)))
            extra = []
            for k in rng.integers(1, max(no // TILE, 1) + 1, 3):
                extra += [int(k) * TILE - 1, int(k) * TILE, int(k) * TILE + 1]
            if rng.random() < 0.4:                              # more than 62 documents in one tile: the searched path
                c = int(rng.integers(0, max(no // TILE, 1))) * TILE
                for _ in range(int(rng.integers(70, 200))):
                    c += int(rng.integers(0, 9))
                    extra.append(c)
            extra = [c for c in extra if 0 <= c <= no]
            self.off = np.sort(np.concatenate([off, np.array(extra, dtype=np.uint64)]))

    def describe(self):
        knobs = "+".join(f"{k[5:]}={v}" for k, v in sorted(self.knobs.items())) or "default"
        return (f"WordCase({self.seed}) knobs {knobs} lines {len(self.lines)} M {self.M} n {self.n} n_owned {self.n_owned} "
                f"edges {EDGES[self.edges]} word_bytes {self.word_bytes!r} prev {self.prev} next {self.next} "
                f"docs {None if self.off is None else self.off.size - 1}")

    def write_patterns(self, path):
        with open(path, "wb") as f:
            f.write(b"".join(p + b"\n" for p in self.lines))
        return path


def run_word_case(g_factory, case, tmp_dir):
    """One case on the GPU: scan, filter, then the records, the selection and the replacement (without documents) or
    the document cut (with them), each against the CPU.  Returns the records compared."""
    c = case
    path = c.write_patterns(os.path.join(tmp_dir, f"words_{c.seed}.pat"))
    try:
        return _run(g_factory, c, path)
    except AssertionError as e:
        raise AssertionError(f"{c.describe()}: {e}") from e


def _run(g_factory, c, path):
    table = PfacTable.from_file(path, c.width)
    o = Oracle(path, 1, 1)
    pos, ids = o.scan_spec(c.data, None)
    o.close()
    own = pos < c.n_owned
    pos, ids = pos[own], ids[own]
    ll = line_lengths(path)
    lens = ll[ids]
    keep = wordref.filter_words(c.data, pos, lens, c.ws, c.edges, c.prev, c.next, c.off)
    kpos, kids, klens = pos[keep], ids[keep], lens[keep]
    nd = 0 if c.off is None else c.off.size - 1
    with g_factory() as g:
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_replacements(c.reps)
        g.reserve(0, max(c.n, 1), max(c.n // 8, 4096))
        g.h2d(c.data)
        total = g.scan_resident(c.n_owned, c.n)
        assert total == pos.size, f"scan: {total} records, want {pos.size}"
        fmt = g.scan_format()
        if nd:
            g.set_doc_offsets(c.off)
        n = g.filter_whole_words(0, c.word_bytes, EDGES[c.edges], c.prev, c.next, n_docs=nd)
        assert n == kpos.size, f"filter: {n} records kept, want {kpos.size} of {pos.size}"
        assert g.scan_format() == fmt and g.last_count() == n
        rec = g.records_to_host(n)
        np.testing.assert_array_equal(rec["pos"].astype(np.int64), kpos, err_msg="kept positions")
        np.testing.assert_array_equal(table.idmap[rec["state"]], kids, err_msg="kept pattern ids")
        if nd:
            kept = g.segment_records(nd)
            first, drec = g.segment_to_host(kept, nd)
            off = c.off.astype(np.int64)
            d = np.searchsorted(off, kpos, side="right") - 1
            inside = kpos + klens <= off[np.minimum(d + 1, nd)]
            np.testing.assert_array_equal(drec["pos"].astype(np.int64), (kpos - off[d])[inside], err_msg="documents: positions")
            np.testing.assert_array_equal(table.idmap[drec["state"]], kids[inside], err_msg="documents: pattern ids")
            np.testing.assert_array_equal(first, np.searchsorted(d[inside], np.arange(nd + 1), side="left").astype(np.uint64),
                                          err_msg="documents: doc_first")
            return pos.size + 2 * n
        n_sel, ex = g.select_leftmost_longest(c.entry)
        sel = g.selection_to_host(n_sel)
        pick, wex = greedy(kpos, klens, c.entry, c.n_owned)
        np.testing.assert_array_equal(sel["pos"].astype(np.int64), kpos[pick], err_msg="selection: positions")
        np.testing.assert_array_equal(table.idmap[sel["state"]], kids[pick], err_msg="selection: pattern ids")
        assert ex == wex, "selection: exit"
        out = g.replacement_to_host(g.replace_selection())
        want = splice(c.data, c.entry, c.n_owned, kpos[pick], klens[pick], kids[pick], rep_table(c.reps))
        assert np.array_equal(out, want), "replace: output differs"
    return pos.size + 2 * n + n_sel
