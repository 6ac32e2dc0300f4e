"""Guard bands around the DEVICE buffers a caller hands to the post-scan passes, and the exact-capacity contract of
include/pfac.h checked against them (shared by tests/test_gpu_pass_bounds.py and tests/test_passguard_cases.py).

The header promises the same about every buffer a caller owns: a pass writes what it reports and no byte more, and a
refused call writes nothing.  Here every output of pfac_records_expand, pfac_records_packed_device, pfac_records_segment,
both selections and both replaces is a heapguard.GuardedBuffer of EXACTLY the bytes the ABI names (n x 8 for records,
out_bytes -- not rounded to 16 -- for the replace output, (n_docs + 1) x 8 for doc_first and the output offsets, used x
record_bytes and n_tiles x 8 for the packed form), and `exact_call` drives one protocol through all of them: one below
the capacity (PFAC_E_OVERFLOW, the exact count, every buffer of the call untouched), rule-breaking document offsets
(PFAC_E_ARG, untouched), the exact capacity (success, payloads equal to the CPU's, guards intact).  A zero result is the
same protocol with a zero-length payload behind a non-NULL pointer.

Three parts:
  exact_call / Want / Judge   the protocol; it knows no pass, so tests/test_passguard_cases.py runs it against fakes
  Cpu                         the cases and what the CPU says about them: tests/orc.py (the oracle), wordref, llref,
                              replref, docref / docreplref -- never the device.  Sizes come from here alone (the packed
                              form's `used` is the one number the ABI itself takes from pfac_scan_format).
  Device                      one context per record width, and one method per pass that builds the guarded buffers of
                              a case and drives exact_call (imports torch lazily; nothing here needs a GPU to import).
                              A GuardedBuffer is filled on torch's stream and the pass writes on the slot's non-blocking
                              one: the buffer's constructor synchronises the device behind its fill, as `upload` does
                              behind its copy, so no fill can land on top of a pass launched right behind it."""
import atexit
import os
import tempfile

import numpy as np

from heapguard import E_ARG, E_OVERFLOW, E_STATE, FILLS, GUARD, TILE, GuardError, GuardedBuffer, padded_records

OK = 0
GROUP = 64 * TILE                       # the passes work in groups of 64 tiles
REC = np.dtype([("pos", "<u4"), ("state", "<u4")])
WIDTHS = (2, 4, 8)
HALO = 64                               # bytes behind n_owned a scan with a halo may read (above both tables' max_pat_len)
STATUS = {OK: "PFAC_OK", E_ARG: "PFAC_E_ARG", E_STATE: "PFAC_E_STATE", E_OVERFLOW: "PFAC_E_OVERFLOW"}


# ---------------------------------------------------------------------------
# the protocol

class Judge:
    """A payload that is not compared byte for byte: `n_bytes` it must have, `fn(raw uint8[n_bytes])` raises
    AssertionError when its content is wrong (None: judged together with the others, Want.joint)."""

    def __init__(self, n_bytes, fn=None):
        self.n_bytes, self.fn = int(n_bytes), fn


class Want:
    """What the CPU says one pass call delivers.  `n`: the result's size in the unit of out_cap (records, or bytes for
    the replaces); `payloads`: per buffer of the call its exact bytes (an array) or a Judge; `bad`: how many
    rule-breaking variants call(n, bad=k) has, each refused with PFAC_E_ARG; `capped`: the call has an out_cap;
    `status`: what the call at the exact capacity returns (not PFAC_OK: every buffer untouched); `joint`: fn({name: raw
    bytes}) over all payloads together."""

    def __init__(self, n, payloads, bad=0, capped=True, status=OK, joint=None):
        self.n, self.bad, self.capped, self.status, self.joint = int(n), int(bad), bool(capped), status, joint
        self.payloads = {k: v if isinstance(v, Judge) else np.ascontiguousarray(v).view(np.uint8).ravel() for k, v in payloads.items()}

    def size(self, name):
        p = self.payloads[name]
        return p.n_bytes if isinstance(p, Judge) else int(p.size)


def _same_bytes(name, got, want):
    assert got.size == want.size, f"{name}: {got.size} bytes, want {want.size}"
    ne = np.flatnonzero(got != want)
    assert ne.size == 0, (f"{name}: {ne.size} bytes differ from the CPU's, first at {int(ne[0])} (0x{int(got[ne[0]]):02x}, want "
                          f"0x{int(want[ne[0]]):02x}), last at {int(ne[-1])}")


def exact_call(g, call, want, buffers, fill, what="pass"):
    """The exact-capacity protocol of one pass call.  `call(cap, bad=None)` performs the call with out_cap = cap into
    `buffers` ({name: GuardedBuffer}, each exactly want.size(name) bytes, all `fill`) and returns (status, reported
    size or None); `g.sync(0)` completes it.  Raises AssertionError (GuardError for a damaged guard or a touched payload)
    naming `what` and the fill."""
    tag = f"{what} fill 0x{fill:02x}"
    try:
        assert set(buffers) == set(want.payloads), f"buffers {sorted(buffers)}, the expectation has {sorted(want.payloads)}"
        for name, b in buffers.items():
            assert b.fill == fill and b.n_bytes == want.size(name), (f"{name}: a buffer of {b.n_bytes} bytes (fill 0x{b.fill:02x}) "
                                                                     f"for a payload of {want.size(name)}")

        def untouched(after):
            for name, b in buffers.items():
                b.check(payload_untouched=True, what=f"{name} after {after}")

        if want.capped and want.n > 0:                          # 1. one too small: refused, exact count, nothing written
            st, n = call(want.n - 1)
            g.sync(0)
            assert st == E_OVERFLOW, f"out_cap {want.n - 1} (one too small): {STATUS.get(st, st)}, want PFAC_E_OVERFLOW"
            assert n == want.n, f"the overflow reports {n}, want {want.n}"
            untouched(f"the refused call (out_cap {want.n - 1})")
        for k in range(want.bad):                               # 3. rule-breaking arguments: refused, nothing written
            st, _ = call(want.n, bad=k)
            g.sync(0)
            assert st == E_ARG, f"rule-breaking variant {k}: {STATUS.get(st, st)}, want PFAC_E_ARG"
            untouched(f"the refused call (rule-breaking variant {k})")
        st, n = call(want.n)                                    # 2. (and 4. for n = 0) the exact capacity
        g.sync(0)
        assert st == want.status, f"out_cap {want.n} (exact): {STATUS.get(st, st)}, want {STATUS.get(want.status, want.status)}"
        if st != OK:
            untouched("the refused call")
            return
        assert n is None or n == want.n, f"the call reports {n}, want {want.n}"
        raw = {}
        for name, b in buffers.items():
            b.check(what=name)
            raw[name] = b.host()
        for name, p in want.payloads.items():
            if not isinstance(p, Judge):
                _same_bytes(name, raw[name], p)
            elif p.fn is not None:
                p.fn(raw[name])
        if want.joint is not None:
            want.joint(raw)
    except GuardError as e:
        raise GuardError(f"{tag}: {e}") from e
    except AssertionError as e:
        raise AssertionError(f"{tag}: {e}") from e


# ---------------------------------------------------------------------------
# the cases: tables, inputs, scans, offsets, windows -- every one a function of its name (and a fixed seed) alone

# 16 lines, all of two bytes or more (so that one-byte documents keep nothing), with prefixes and suffixes of one another
LINES16 = [b"the", b"he", b"th", b"and", b"an", b"in", b"ing", b"ed", b" t", b"er", b"that", b"re", b"at", b"en", b"on", b"with"]
REPS16 = [b"", b"HE!!", b"", b"&", b"an indefinite article", b"", b"ING", b"", b" T", b"err", b"THAT IS", b"", b"@", b"", b"upon", b"w/"]
TABLES = {2: dict(pat="lines16", knobs={}), 4: dict(pat="dictionary", knobs={}), 8: dict(pat="lines16", knobs={"PFAC_WIDE": "1"})}
KNOB_NAMES = ("PFAC_WIDE", "PFAC_REC_BYTES")

# name -> (input, n_owned, n_avail or None = n_owned).  "halo": n_owned < n_avail; "none": a scan without a record.
SIZES = {"t3": ("text", 3 * TILE + 17, None), "t63": ("text", 63 * TILE, None), "t64": ("text", 64 * TILE, None),
         "t65": ("text", 65 * TILE, None), "t130": ("text", 130 * TILE + 17, None), "halo": ("text", None, "halo"),
         "none": ("none", 3 * TILE + 17, None)}
SIZE_CASES = tuple(SIZES)
FILTERED = "t65+words"                  # the t65 scan after pfac_records_filter_words (default set, both edges)
DOC_SHAPES = ("one", "big", "tiny", "empty0", "emptymid", "emptytile", "emptygroup", "emptyend", "cut", "nothing")
EMPTY_RUN = 230                         # empty documents in a run (>= 200)
EMPTY_AT = {"empty0": 0, "emptymid": 5 * TILE + 1234, "emptytile": 7 * TILE, "emptygroup": GROUP, "emptyend": None}
SEL_COUNTS = (63, 64, 65, 1023, 1024, 1025)       # picks on both sides of the replace count kernel's block and group
LADDER = tuple(f"res{r}" for r in range(16)) + ("lt16", "zero", "k1", "k4", "gallop", "entry")
LADDER_STRETCH = 200                    # consecutive picks with empty replacements and no gap between them (> 64)
LADDER_ENTRY = 2
WINDOW_N = (0, 1, 63, 64, 65)


def bad_offsets(off, n_owned):
    """The three rule-breaking sets the document tests use: off[0] != 0, descending, off[n_docs] != n_owned; each as
    long as `off`."""
    off = np.asarray(off, dtype=np.uint64)
    b0, b1, b2 = off.copy(), off.copy(), off.copy()
    b0[0] = 1
    k = (off.size - 1) // 2
    b1[k] = b1[k + 1] + np.uint64(1)
    b2[-1] = np.uint64(n_owned - 1)
    return [b0, b1, b2]


def cut_by_hand(pos, ids, lens, off):
    """The whole-buffer records cut at the documents by the header's rule (keep iff pos + len <= off[d + 1], d the last
    document with off[d] <= pos) -> (doc_first, pos relative to the document, ids, keep mask, document of every kept)."""
    o = np.asarray(off, dtype=np.int64)
    d = np.searchsorted(o, pos, side="right") - 1
    d = np.minimum(d, o.size - 2)
    keep = pos + lens <= o[d + 1]
    kd = d[keep]
    first = np.searchsorted(kd, np.arange(o.size), side="left").astype(np.uint64)
    return first, pos[keep] - o[kd], ids[keep], keep, kd


class DocCut:
    """Stands where the CPU oracle stands in docref.oracle_per_doc / docreplref.per_doc for a FILTERED scan (the filter
    judged the records in the whole buffer, which no scan of a document repeats): asked for the non-empty documents in
    turn, it answers with the scan's kept records that lie inside each one."""

    def __init__(self, rows, off):
        self.rows = rows
        o = np.asarray(off, dtype=np.int64)
        self.ranges = iter([(int(a), int(b)) for a, b in zip(o[:-1], o[1:]) if b > a])

    def scan_spec(self, buf, *_):
        a, b = next(self.ranges)
        assert buf.size == b - a
        pos, ids, lens = self.rows
        lo, hi = np.searchsorted(pos, [a, b], side="left")
        inside = pos[lo:hi] + lens[lo:hi] <= b
        return pos[lo:hi][inside] - a, ids[lo:hi][inside]


class Cpu:
    """What the CPU says, computed once per key.  A scan is keyed (input name, n_owned, n_avail, filtered)."""

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="pfac_passguard_")
        self._c = {}

    def _memo(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    def close(self):
        for key in [k for k in self._c if k[0] == "pat"]:
            self._c.pop(key)["matcher"].close()

    # -- tables -------------------------------------------------------------
    def pat(self, name):
        def make():
            from llref import line_lengths
            from orc import Oracle
            path = os.path.join(self.dir, name + ".pat")
            data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
            with open(path, "wb") as f:
                if name == "lines16":
                    f.write(b"".join(p + b"\n" for p in LINES16))
                else:
                    for part in ("xaa", "xab", "xac", "xad"):
                        f.write(open(os.path.join(data, part), "rb").read())
            lines = open(path, "rb").read().split(b"\n")[:-1]
            return dict(path=path, matcher=Oracle(path, 1, 1), ll=line_lengths(path), lines=lines)
        return self._memo(("pat", name), make)

    def tinfo(self, W):
        return self.pat(TABLES[W]["pat"])

    def table(self, W):
        """The PfacTable of record width W (its knobs: TABLES[W]["knobs"], read when it is installed)."""
        from phfpfac_amd import PfacTable
        return self._memo(("table", TABLES[W]["pat"]), lambda: PfacTable.from_file(self.tinfo(W)["path"], 256))

    def M(self, W):
        return int(self.tinfo(W)["ll"].max())

    def reps(self, W):
        """{pattern id: bytes}: empty, shorter and longer replacements mixed."""
        def make():
            if TABLES[W]["pat"] == "lines16":
                return {i + 1: r for i, r in enumerate(REPS16)}
            rng = np.random.default_rng([0x5245, 4])
            ll = self.tinfo(W)["ll"]
            out = {}
            for i in range(1, ll.size):
                u = rng.random()
                n = 0 if u < 0.3 else int(rng.integers(1, max(int(ll[i]), 2))) if u < 0.6 else int(ll[i]) + int(rng.integers(0, 12))
                out[i] = rng.integers(33, 127, n).astype(np.uint8).tobytes()
            return out
        return self._memo(("reps", TABLES[W]["pat"]), make)

    def rep_table(self, W):
        from replref import rep_table
        return self._memo(("reptab", TABLES[W]["pat"]), lambda: rep_table(self.reps(W)))

    # -- inputs -------------------------------------------------------------
    def input(self, name):
        def make():
            data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data", "paragraph402")
            para = np.frombuffer(open(data, "rb").read(), dtype=np.uint8)
            n = 130 * TILE + 17 + HALO
            text = para[np.arange(n, dtype=np.int64) % para.size]
            if name == "text":
                return text
            if name == "noi":                                   # no "i": the dictionary's one line of one byte
                t = text[:3 * TILE + 17].copy()
                t[t == ord("i")] = ord("o")
                return t
            if name == "none":
                return np.full(3 * TILE + 17, ord("#"), dtype=np.uint8)
            assert name == "thes"                               # the replace ladder's: a stretch of "the", then text
            return np.concatenate([np.frombuffer(b"the" * LADDER_STRETCH, dtype=np.uint8), text[:2 * TILE + 100]])
        return self._memo(("input", name), make)

    def doc_owned(self):
        """n_owned of the document shapes: just above 65 tiles, and inside a "the" of the text, so that with a halo
        behind it a record of either table runs past n_owned (one document then keeps fewer than were scanned)."""
        at = bytes(self.input("text")).find(b" the ", 65 * TILE + 17)
        assert 0 < at < 66 * TILE
        return at + 2

    def size_key(self, name):
        """The scan (input, n_owned, n_avail, filtered) of a SIZE_CASES name or of FILTERED."""
        if name == FILTERED:
            return self.size_key("t65")[:3] + (True,)
        inp, no, na = SIZES[name]
        if na == "halo":
            at = bytes(self.input("text")).find(b" the ", 5 * TILE + 100)
            no, na = at + 2, at + 2 + HALO
        return inp, no, no if na is None else na, False

    def doc_key(self, shape, filt=False):
        if shape == "nothing":
            return "noi", 3 * TILE + 17, 3 * TILE + 17, filt
        no = self.doc_owned()
        return "text", no, no + HALO, filt

    # -- the scan -----------------------------------------------------------
    def scan(self, W, key):
        """(pos, ids, lens) of the records that start in [0, n_owned) of a scan that may read [0, n_avail)."""
        inp, no, na, filt = key

        def make():
            info = self.tinfo(W)
            pos, ids = info["matcher"].scan_spec(np.ascontiguousarray(self.input(inp)[:na]), None)
            own = pos < no
            pos, ids = pos[own].astype(np.int64), ids[own].astype(np.int64)
            return pos, ids, info["ll"][ids]

        def filtered():
            import wordref
            pos, ids, lens = self.scan(W, (inp, no, na, False))
            keep = wordref.filter_words(self.input(inp)[:na], pos, lens)
            return pos[keep], ids[keep], lens[keep]
        return self._memo(("scan", TABLES[W]["pat"], key), filtered if filt else make)

    def tile_counts(self, W, key):
        no = key[1]
        return np.bincount(self.scan(W, key)[0] // TILE, minlength=(no + TILE - 1) // TILE).astype(np.int64)

    def windows(self, W, key):
        """The [first, first + n) windows of the expand test: starts at a tile's and a group's first and last record."""
        tc = self.tile_counts(W, key)
        c0, G, T = int(tc[0]), int(tc[:64].sum()), int(tc.sum())
        assert 1 < c0 < G - 1 and G + 1 < T - 1, "the window scan needs more than one group and records in tile 0"
        out = []
        for first in (0, 1, c0 - 1, c0, c0 + 1, G - 1, G, G + 1, T - 1, T):
            for n in WINDOW_N + (T - first,):
                if first + n <= T and (first, n) not in out:
                    out.append((first, n))
        return out, (c0, G, T)

    # -- selection and replace ------------------------------------------------
    def sel(self, W, key, entry=0):
        """(pos, ids, exit) of the leftmost-longest selection from `entry`."""
        def make():
            from llref import greedy
            pos, ids, lens = self.scan(W, key)
            idx, ex = greedy(pos, lens, entry, key[1])
            return pos[idx], ids[idx], int(ex)
        return self._memo(("sel", TABLES[W]["pat"], key, entry), make)

    def replace(self, W, key, entry=0):
        def make():
            from replref import splice
            spos, sids, _ = self.sel(W, key, entry)
            return splice(self.input(key[0]), entry, key[1], spos, self.tinfo(W)["ll"][sids], sids, self.rep_table(W))
        return self._memo(("replace", TABLES[W]["pat"], key, entry), make)

    def sel_key(self, W, count):
        """A scan of the text (with a halo, so that trimming n_owned only drops picks) that selects exactly `count`."""
        full = ("text", 3 * TILE, 3 * TILE + HALO, False)
        spos = self.sel(W, full)[0]
        assert spos.size > count
        no = int(spos[count])
        return "text", no, no + HALO, False

    # -- the replace ladder -------------------------------------------------------
    def _ladder_sizes(self, W):
        """out_bytes of ("thes", x, all, entry 0) for every x, by arithmetic over the picks of the whole input (with the
        whole input readable a smaller n_owned only drops picks); `ladder_key` chooses from it, the real reference
        (`replace`) is what a case is compared with, and tests/test_passguard_cases.py checks the two agree."""
        def make():
            n = int(self.input("thes").size)
            spos, sids, _ = self.sel(W, ("thes", n, n, False))
            ll, (roff, _) = self.tinfo(W)["ll"], self.rep_table(W)
            delta = np.concatenate([[0], np.cumsum((roff[sids + 1] - roff[sids]) - ll[sids])])
            ends = np.concatenate([[0], np.maximum.accumulate(spos + ll[sids])])
            x = np.arange(n + 1, dtype=np.int64)
            k = np.searchsorted(spos, x, side="left")           # picks that start below x
            return x + np.maximum(ends[k], x) - x + delta[k]    # n_owned + exit - entry + sum (R - L)
        return self._memo(("ladder", TABLES[W]["pat"]), make)

    def ladder_key(self, W, name):
        """(scan key, entry) of a LADDER case."""
        n = int(self.input("thes").size)
        sizes = self._ladder_sizes(W)

        def first_in(lo, hi, start=0):
            hit = np.flatnonzero((sizes[start:] >= lo) & (sizes[start:] <= hi))
            assert hit.size, f"no n_owned gives an output of {lo}..{hi} bytes"
            return start + int(hit[0])
        if name.startswith("res"):                              # n_owned = N0 - j, the smallest j with this residue
            N0 = n - 50
            j = np.flatnonzero(sizes[N0::-1][:N0 - 3 * LADDER_STRETCH] % 16 == int(name[3:]))
            assert j.size and j[0] < 200, f"no small j gives out_bytes = {name[3:]} mod 16"
            return ("thes", N0 - int(j[0]), n, False), 0
        if name == "zero":
            return ("thes", 30, n, False), 0                    # ten times "the", each replaced by nothing
        if name == "lt16":
            return ("thes", first_in(1, 15), n, False), 0
        if name == "k1":
            return ("thes", first_in(1008, 1040), n, False), 0
        if name == "k4":
            return ("thes", first_in(4080, 4112), n, False), 0
        if name == "gallop":
            return ("thes", 3 * LADDER_STRETCH + 700, n, False), 0
        assert name == "entry"                                  # entry > 0, and the last pick runs past n_owned
        spos, sids, _ = self.sel(W, ("thes", n, n, False), LADDER_ENTRY)
        ll = self.tinfo(W)["ll"]
        k = int(np.flatnonzero((spos > 3 * LADDER_STRETCH + 500) & (ll[sids] >= 3))[0])
        return ("thes", int(spos[k]) + 1, n, False), LADDER_ENTRY

    # -- documents ----------------------------------------------------------
    def offsets(self, W, key, shape):
        """Document offsets (uint64[n_docs + 1]) of a DOC_SHAPES name, or "rand" for the size cases."""
        inp, no, na, _ = key

        def spaced(rng, a, b, lo, hi):
            """cuts in (a, b), lo..hi bytes apart and at least lo in front of b"""
            if b - a <= lo:
                return np.empty(0, dtype=np.int64)
            c = a + np.cumsum(rng.integers(lo, hi + 1, (b - a) // lo + 1))
            return c[c <= b - lo]

        def make():
            from docref import random_offsets
            rng = np.random.default_rng([0x444F43, no, (("rand",) + DOC_SHAPES).index(shape)])
            if shape == "rand":
                off = random_offsets(rng, no, max(2, no // 300), empties=5).astype(np.int64)
                edges = [c for t in range(1, no // TILE + 1, 7) for c in (t * TILE - 1, t * TILE, t * TILE + 1) if c <= no]
                return np.sort(np.concatenate([off, np.array(edges, dtype=np.int64)])).astype(np.uint64)
            if shape == "one":
                return np.array([0, no], dtype=np.uint64)
            if shape == "nothing":
                return np.arange(no + 1, dtype=np.uint64)
            if shape == "tiny":                                 # 1..40 bytes in tiles 1, 2 and 63, 64 (across the group edge)
                parts = [spaced(rng, 0, TILE, 64, 600), spaced(rng, TILE, 3 * TILE, 1, 40), spaced(rng, 3 * TILE, 63 * TILE, 64, 600),
                         spaced(rng, 63 * TILE, 65 * TILE, 1, 40), spaced(rng, 65 * TILE, no, 64, 600)]
                cuts = np.concatenate(parts)
            elif shape == "cut":                                # document ends inside matches: behind the first byte of
                pos, _, lens = self.scan(W, key[:3] + (False,))   # every fifth record of two bytes or more
                long_ = pos[lens >= 2]
                cuts = np.unique(long_[::5] + 1)
                cuts = cuts[(cuts > 0) & (cuts < no)]
            else:
                cuts = spaced(rng, 0, no, 64, 600)
            if shape in EMPTY_AT:
                at = no if EMPTY_AT[shape] is None else EMPTY_AT[shape]
                cuts = np.concatenate([cuts, np.full(EMPTY_RUN, at, dtype=np.int64)])
            return np.sort(np.concatenate([[0], cuts, [no]])).astype(np.uint64)
        name = ("off", key[:3], shape) + ((TABLES[W]["pat"],) if shape == "cut" else ())
        return self._memo(name, make)

    def seg(self, W, key, shape):
        """(doc_first, pos relative to the document, ids) of pfac_records_segment: the whole-buffer records cut by hand
        (tests/test_passguard_cases.py holds it against docref.oracle_per_doc)."""
        def make():
            pos, ids, lens = self.scan(W, key)
            return cut_by_hand(pos, ids, lens, self.offsets(W, key, shape))[:3]
        return self._memo(("seg", TABLES[W]["pat"], key, shape), make)

    def docsel(self, W, key, shape):
        """(doc_first, pos relative to the SCAN, ids, out_off, out) of every document's own selection and output.  No kept
        record crosses a document end, so one greedy over the kept records of the whole buffer restarts at every
        document, and one splice of the whole buffer is the documents' outputs concatenated (tests/
        test_passguard_cases.py holds both against docreplref.per_doc, document by document)."""
        def make():
            from llref import greedy
            from replref import splice
            pos, ids, lens = self.scan(W, key)
            off = self.offsets(W, key, shape)
            _, _, _, keep, _ = cut_by_hand(pos, ids, lens, off)
            kp, ki, kl = pos[keep], ids[keep], lens[keep]
            idx, ex = greedy(kp, kl, 0, key[1])
            assert ex == 0
            sp, si, sl = kp[idx], ki[idx], kl[idx]
            o = off.astype(np.int64)
            first = np.searchsorted(sp, o, side="left").astype(np.uint64)
            first[-1] = sp.size
            out = splice(self.input(key[0]), 0, key[1], sp, sl, si, self.rep_table(W))
            roff = self.rep_table(W)[0]
            delta = np.concatenate([[0], np.cumsum((roff[si + 1] - roff[si]) - sl)])
            out_off = (o + delta[first.astype(np.int64)]).astype(np.uint64)
            return first, sp, si, out_off, out
        return self._memo(("docsel", TABLES[W]["pat"], key, shape), make)


_CPU = None


def cpu():
    global _CPU
    if _CPU is None:
        _CPU = Cpu()
        atexit.register(_CPU.close)
    return _CPU


# ---------------------------------------------------------------------------
# the device: one context per record width, one method per pass

class _Env:
    """The scan knobs of a table in the environment while it is installed (they are read at the upload)."""

    def __init__(self, knobs):
        self.knobs = knobs

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in KNOB_NAMES}
        for k in KNOB_NAMES:
            os.environ.pop(k, None)
        os.environ.update(self.knobs)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class Device:
    """One GpuMatcher with the table of record width W, its lengths and replacements; `scan(key)` leaves the slot's
    last finished scan at `key` (and scans only when it is another)."""

    def __init__(self, W, x=None, device=0):
        from phfpfac_amd import GpuMatcher
        self.W, self.x, self.dev = W, x or cpu(), device
        self.table = self.x.table(W)
        self.g = GpuMatcher(device, 1)
        with _Env(TABLES[W]["knobs"]):
            self.g.load_table(self.table)
        self.g.set_final_lengths(self.table.final_lengths())
        self.g.set_replacements(self.x.reps(W))
        self.inputs, self.cur = {}, None
        self.idmap = np.asarray(self.table.idmap, dtype=np.int64)

    def close(self):
        self.g.close()

    def upload(self, arr, slack=0):
        """`arr` as a device tensor of its own (uint8), `slack` bytes behind it."""
        import torch
        raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
        t = torch.zeros(max(raw.size + slack, 16), dtype=torch.uint8, device=f"cuda:{self.dev}")
        if raw.size:
            t[:raw.size].copy_(torch.from_numpy(raw.copy()))
        torch.cuda.synchronize(self.dev)
        return t

    def d_input(self, inp):
        if inp not in self.inputs:
            self.inputs[inp] = self.upload(self.x.input(inp), slack=TILE)
        return self.inputs[inp]

    def scan(self, key):
        if self.cur == key:
            return
        inp, no, na, filt = key
        g = self.g
        self.cur = None
        g.reserve(0, 0, max(na, TILE))
        n = g.scan_resident(no, na, d_input=self.d_input(inp))
        assert n == self.x.scan(self.W, key[:3] + (False,))[0].size, f"the scan counts {n} records"
        assert g.scan_format()[0] == self.W, f"record width {g.scan_format()[0]}, want {self.W}"
        if filt:
            n = g.filter_whole_words(0, d_input=self.d_input(inp))
            assert n == self.x.scan(self.W, key)[0].size, f"the filter keeps {n} records"
        self.cur = key

    # -- judges -------------------------------------------------------------
    def records(self, pos, ids, what="records"):
        """Judge of a pfac_record payload: positions and pattern ids (the device's states through the idmap)."""
        pos, ids = np.asarray(pos, dtype=np.int64), np.asarray(ids, dtype=np.int64)

        def fn(raw):
            rec = raw.view(REC)
            ne = np.flatnonzero(rec["pos"].astype(np.int64) != pos)
            assert ne.size == 0, f"{what}: {ne.size} positions differ, first at record {int(ne[0])}: {int(rec['pos'][ne[0]])}, want {int(pos[ne[0]])}"
            st = rec["state"].astype(np.int64)
            assert st.size == 0 or int(st.max()) < self.idmap.size, f"{what}: a state past num_final"
            ne = np.flatnonzero(self.idmap[st] != ids)
            assert ne.size == 0, f"{what}: {ne.size} pattern ids differ, first at record {int(ne[0])}"
        return Judge(pos.size * 8, fn)

    def _status(self, fn, attr=None):
        from phfpfac_amd import PfacError
        try:
            return OK, fn()
        except PfacError as e:
            return e.status, getattr(e, attr, None) if attr else None

    # -- the passes -----------------------------------------------------------
    def expand(self, key, first, n, fill, refuse_past_end=False):
        """Records [first, first + n) into a d_out of exactly n x 8 bytes; with `refuse_past_end` (first + n = the match
        count) the window one longer is refused first."""
        self.scan(key)
        pos, ids, _ = self.x.scan(self.W, key)
        buf = {"d_out": GuardedBuffer(n * 8, fill=fill)}

        def call(cap, bad=None):
            return self._status(lambda: self.g.expand_records(n + (bad is not None), buf["d_out"].ptr, first=first))[0], None
        want = Want(n, {"d_out": self.records(pos[first:first + n], ids[first:first + n])}, bad=int(refuse_past_end), capped=False)
        exact_call(self.g, call, want, buf, fill, f"pfac_records_expand width {self.W} scan {key} window [{first}, +{n})")

    def packed(self, key, fill, variant="both"):
        """The packed form into d_words_out (exactly used x record_bytes) and d_tile_index_out (exactly n_tiles x 8).
        variant: "both"; "null" / "heap" (d_words_out NULL / the heap itself: only the index is copied); "zero"
        (n_words = 0).  A scan of 8-byte records is refused with PFAC_E_STATE, both buffers untouched."""
        from phfpfac_amd.dist import packed_to_records
        from phfpfac_amd.matcher import _ptr
        self.scan(key)
        g, W = self.g, self.W
        pos, ids, _ = self.x.scan(W, key)
        rb, n_tiles, used = g.scan_format()
        tc = self.x.tile_counts(W, key)
        assert n_tiles == tc.size, f"{n_tiles} tiles, want {tc.size}"
        assert used >= padded_records(tc, rb), f"used {used} is less than the runs' own allocations"
        words = variant == "both"
        buf = {"d_tile_index_out": GuardedBuffer(n_tiles * 8, fill=fill),
               "d_words_out": GuardedBuffer(used * rb if words or W == 8 else 0, fill=fill)}
        d_words = {"both": buf["d_words_out"].ptr, "zero": buf["d_words_out"].ptr, "null": 0, "heap": g.records_ptr(0)}[variant]
        n_words = 0 if variant == "zero" else used

        def call(cap, bad=None):
            rc = g._L.pfac_records_packed_device(g._ctx, 0, _ptr(None), _ptr(d_words), int(n_words), _ptr(buf["d_tile_index_out"].ptr))
            return rc, None

        def joint(raw):
            tix = raw["d_tile_index_out"].view(np.uint64)
            cnt = (tix >> np.uint64(40)).astype(np.int64)
            assert np.array_equal(cnt, tc), "the tile index's counts differ from the oracle's histogram"
            if words:
                heap = raw["d_words_out"]
            else:                                               # the words stayed where the scan wrote them
                heap, _ = g.packed_to_host(0)
            rec = packed_to_records(heap, tix, rb)
            assert np.array_equal(rec["pos"].astype(np.int64), pos), "packed form: positions differ from the oracle's"
            assert np.array_equal(self.idmap[rec["state"].astype(np.int64)], ids), "packed form: pattern ids differ from the oracle's"
        want = Want(0, {"d_tile_index_out": Judge(n_tiles * 8), "d_words_out": Judge(buf["d_words_out"].n_bytes)}, capped=False,
                    status=E_STATE if W == 8 else OK, joint=joint)
        exact_call(g, call, want, buf, fill, f"pfac_records_packed_device ({variant}) width {W} scan {key}")
        if not words and W != 8:
            buf["d_words_out"].check(payload_untouched=True, what="a d_words_out the call was not to write")

    def _doc_args(self, key, shape, refuse):
        off = self.x.offsets(self.W, key, shape)
        d_off = self.upload(off)
        d_bad = [self.upload(b) for b in bad_offsets(off, key[1])] if refuse else []
        return off, int(off.size - 1), d_off, d_bad

    def segment(self, key, shape, fill):
        self.scan(key)
        g = self.g
        first, pos, ids = self.x.seg(self.W, key, shape)
        off, nd, d_off, d_bad = self._doc_args(key, shape, True)
        buf = {"d_out": GuardedBuffer(pos.size * 8, fill=fill), "d_doc_first": GuardedBuffer((nd + 1) * 8, fill=fill)}

        def call(cap, bad=None):
            return self._status(lambda: g.segment_records(nd, d_doc_offsets=d_off if bad is None else d_bad[bad], d_out=buf["d_out"].ptr,
                                                          out_cap=cap, d_doc_first=buf["d_doc_first"].ptr), "n_kept")
        want = Want(pos.size, {"d_out": self.records(pos, ids, "kept records"), "d_doc_first": first}, bad=len(d_bad))
        exact_call(g, call, want, buf, fill, f"pfac_records_segment width {self.W} scan {key} offsets {shape} ({nd} documents)")

    def select(self, key, fill, entry=0):
        """-> the GuardedBuffer that holds the selection (the slot's last: a replace may take it as d_sel)."""
        self.scan(key)
        g = self.g
        pos, ids, ex = self.x.sel(self.W, key, entry)
        buf = {"d_out": GuardedBuffer(pos.size * 8, fill=fill)}

        def call(cap, bad=None):
            st, got = self._status(lambda: g.select_leftmost_longest(entry, d_out=buf["d_out"].ptr, out_cap=cap), "n_selected")
            if st != OK:
                return st, got
            assert got[1] == ex, f"exit {got[1]}, want {ex}"
            return st, got[0]
        want = Want(pos.size, {"d_out": self.records(pos, ids, "picks")})
        exact_call(g, call, want, buf, fill, f"pfac_records_leftmost_longest width {self.W} scan {key} entry {entry}")
        return buf["d_out"]

    def select_docs(self, key, shape, fill, refuse=True):
        """-> (d_out, d_doc_first, the offsets' tensor, n_docs) of the selection, for pfac_replace_documents."""
        self.scan(key)
        g = self.g
        first, pos, ids, _, _ = self.x.docsel(self.W, key, shape)
        off, nd, d_off, d_bad = self._doc_args(key, shape, refuse)
        buf = {"d_out": GuardedBuffer(pos.size * 8, fill=fill), "d_doc_first": GuardedBuffer((nd + 1) * 8, fill=fill)}

        def call(cap, bad=None):
            return self._status(lambda: g.select_leftmost_longest_documents(nd, d_doc_offsets=d_off if bad is None else d_bad[bad],
                                                                            d_out=buf["d_out"].ptr, out_cap=cap,
                                                                            d_doc_first=buf["d_doc_first"].ptr), "n_selected")
        want = Want(pos.size, {"d_out": self.records(pos, ids, "picks"), "d_doc_first": first}, bad=len(d_bad))
        exact_call(g, call, want, buf, fill, f"pfac_records_leftmost_longest_documents width {self.W} scan {key} offsets {shape} ({nd} documents)")
        return buf["d_out"], buf["d_doc_first"], d_off, nd

    def replace(self, key, fill, entry=0, front=GUARD):
        """The selection into an exact guarded d_out, then the replace with that buffer as d_sel into a d_out of exactly
        out_bytes bytes whose payload starts `front` bytes into its tensor."""
        sel = self.select(key, fill, entry)
        g = self.g
        was = sel.host()
        out = self.x.replace(self.W, key, entry)
        buf = {"d_out": GuardedBuffer(out.size, front=front, fill=fill)}

        def call(cap, bad=None):
            return self._status(lambda: g.replace_selection(d_input=self.d_input(key[0]), d_out=buf["d_out"].ptr, out_cap=cap,
                                                            d_sel=sel.ptr), "out_bytes")
        exact_call(g, call, Want(out.size, {"d_out": out}), buf, fill,
                   f"pfac_replace_leftmost_longest width {self.W} scan {key} entry {entry} payload at +{front}")
        sel.check(what="the d_sel of a replace")
        assert np.array_equal(sel.host(), was), "a replace changed its d_sel"

    def replace_docs(self, key, shape, fill):
        sel, dfirst, d_off, nd = self.select_docs(key, shape, fill, refuse=False)
        g = self.g
        was = sel.host(), dfirst.host()
        _, _, _, out_off, out = self.x.docsel(self.W, key, shape)
        buf = {"d_out": GuardedBuffer(out.size, fill=fill), "d_out_offsets": GuardedBuffer((nd + 1) * 8, fill=fill)}

        def call(cap, bad=None):
            return self._status(lambda: g.replace_selection_documents(d_input=self.d_input(key[0]), d_out=buf["d_out"].ptr, out_cap=cap,
                                                                      d_out_offsets=buf["d_out_offsets"].ptr, d_sel=sel.ptr,
                                                                      d_doc_offsets=d_off, d_doc_first=dfirst.ptr), "out_bytes")
        exact_call(g, call, Want(out.size, {"d_out": out, "d_out_offsets": out_off}), buf, fill,
                   f"pfac_replace_documents width {self.W} scan {key} offsets {shape} ({nd} documents)")
        sel.check(what="the d_sel of a replace")
        dfirst.check(what="the d_doc_first of a replace")
        assert np.array_equal(sel.host(), was[0]) and np.array_equal(dfirst.host(), was[1]), "a replace changed the selection it read"
