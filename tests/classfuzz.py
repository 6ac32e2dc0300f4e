"""Seeded random cases for the two front ends that are no plain pattern file -- character classes
(PfacTable.from_charclass) and escaped files (PfacTable.from_file(..., escapes=True)) -- shared by
tests/test_classfuzz_cases.py, tests/test_gpu_class_automata.py and tools/fuzz.py: the sibling of tests/passfuzz.py.
Their automata have shapes no literal file can produce: byte 10 (and every other byte) as an edge, a DAG instead of a
trie, final states that stand for several pattern ids, one-byte negated classes.

Every expectation comes from the brute-force matcher oracle/charclass_oracle.py (and, for escaped files, from the CPU
oracle's escape-aware reader) with lengths from the parsed lines -- never from the device or from
PfacTable.final_lengths.  The post-scan passes go through passfuzz._run with a table factory and a lengths source."""
import importlib.util
import os
import re
import zlib

import numpy as np

from orc import Oracle
from passfuzz import GROUP, KNOBS, Case, _run, knob_label
from phfpfac_amd import PfacTable, emit_records_multi

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("charclass_oracle", os.path.join(_REPO, "oracle", "charclass_oracle.py"))
cco = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cco)

SEEDS = list(range(3 * len(KNOBS)))     # the suite's cases: every knob set three times
TEXT_BASES = (0, 999_999_990, 3 << 32)
TEXT_CHUNK = 200_000                    # lines of expected text formatted and compared at a time
# bytes the generator never writes as a pattern byte or a class member: '[' opens and ']' closes a class even when
# escaped (the readers decode escapes first), '^' negates as a class's first element, '-' after an element is a range
_NEVER = (0x5B, 0x5D, 0x5E, 0x2D)
_PLAIN = frozenset(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789")


class ClassMatcher:
    """Oracle.scan_spec's interface over the brute-force matcher: one record per (position, length).  A class table's
    record carries the LOWEST pattern id that ends there (idmap[state] of the one DFA state reached); an escaped file
    reports duplicate lines once, under the LAST of them (`pick="last"`).  `full(data)` is the matcher's own list:
    every (position, id) in (position, length, id) order.  The list of the last input is kept, keyed by the array and
    a checksum of its bytes, so a buffer changed in place is matched again.  `parsed` replaces the matcher's own parse
    of the image (lines its class grammar cannot spell: byte 0x5B as a literal)."""

    def __init__(self, image, pick="lowest", parsed=None):
        assert pick in ("lowest", "last")
        self.image, self.pick = image, pick
        self.parsed = cco.parse(image) if parsed is None else parsed
        self.lens = np.array([0] + [len(p) for p in self.parsed], dtype=np.int64)
        self._last = None

    def full(self, data):
        data = np.asarray(data, dtype=np.uint8)
        crc = zlib.crc32(np.ascontiguousarray(data))
        if self._last is None or self._last[0] is not data or self._last[1] != crc:
            self._last = (data, crc) + cco.match(self.image, data, self.parsed)
        return self._last[2], self._last[3]

    def close(self):
        """(Oracle's interface: nothing to free.)"""

    def scan_spec(self, data, n=None):
        pos, ids = self.full(data)
        if pos.size == 0:
            return pos, ids
        ln = self.lens[ids]
        edge = (pos[1:] != pos[:-1]) | (ln[1:] != ln[:-1])                  # (sorted by position, length, id)
        keep = np.append(True, edge) if self.pick == "lowest" else np.append(edge, True)
        return pos[keep], ids[keep]


def shape(table):
    """(fan, depth-1 states, used columns, row entries) of a table, read through PfacTable.lookup: root edges, the
    distinct states they lead to, the bytes that are an edge of some depth-1 state, and the edges of the depth-1
    states counted once per ROOT EDGE that leads to them -- the entries of the dense rows the device builds (one row
    per root edge), which is what its install code compares with its packed-row limit."""
    root = table.num_final + 1
    d1 = [table.lookup(root, b) for b in range(256)]
    rows = {s: np.array([table.lookup(s, c) >= 0 for c in range(256)]) for s in set(d1) if s >= 0}
    fan = sum(s >= 0 for s in d1)
    used = np.zeros(256, dtype=bool)
    for r in rows.values():
        used |= r
    entries = sum(int(rows[s].sum()) for s in d1 if s >= 0)
    return fan, len(rows), int(used.sum()), entries


def cpu_walk(t, data):
    """The PFAC walk on the host table (the device lookup contract) -> (pos, final state) per record."""
    pos, st = [], []
    n = data.size
    root = t.num_final + 1
    for i in range(n):
        s = root
        for j in range(i, n):
            s = t.lookup(s, int(data[j]))
            if s < 0:
                break
            if s < t.num_final:
                pos.append(i)
                st.append(s)
    return np.array(pos, dtype=np.int64), np.array(st, dtype=np.int64)


def expand(table, pos, states):
    """Records -> every (position, id) through the outputs lists of a class table."""
    first = np.asarray(table.out_first, dtype=np.int64)
    states = np.asarray(states, dtype=np.int64)
    cnt = first[states + 1] - first[states]
    idx = np.repeat(first[states] - np.append(0, np.cumsum(cnt)[:-1]), cnt) + np.arange(int(cnt.sum()))
    return np.repeat(np.asarray(pos, dtype=np.int64), cnt), np.asarray(table.out_ids)[idx]


def format_lines(pos, ids, base=0):
    return "".join("At position %4d, match pattern %d\n" % (p + base, k) for p, k in zip(pos.tolist(), ids.tolist())).encode()


def assert_text(text, pos, ids, base=0, what="text"):
    """Asserts that `text` is the lines of (pos + base, ids), formatting and comparing TEXT_CHUNK lines at a time, so a
    list of any length is checked in full."""
    at = 0
    for a in range(0, pos.size, TEXT_CHUNK):
        want = format_lines(pos[a:a + TEXT_CHUNK], ids[a:a + TEXT_CHUNK], base)
        assert text[at:at + len(want)] == want, f"{what}: differs in lines {a} to {a + TEXT_CHUNK - 1}"
        at += len(want)
    assert len(text) == at, f"{what}: {len(text)} bytes, want {at}"


def _spell(rng, b):
    """One byte as pattern text: plain letters and digits mostly as themselves, everything else as a full-width
    escape (\\xNN, \\ooo, now and then \\n for byte 10)."""
    if b in _PLAIN and rng.random() < 0.85:
        return bytes([b])
    r = rng.random()
    if b == 10 and r < 0.4:
        return b"\\n"
    return b"\\x%02x" % b if r < 0.75 else b"\\%03o" % b


class ClassCase(Case):
    """One random case: lines of atoms (literal bytes in several spellings, small classes, ranges, negated classes, now
    and then the full class), duplicates and prefixes among them, an input over the bytes the atoms mention (always
    with 10 and 0) with instances of the lines planted, and the owned range, entry, replacements, document offsets and
    chain cuts of passfuzz.Case.  `kind`: "charclass" or "escaped" (no classes).  `seed` alone fixes everything."""

    def __init__(self, seed, knobs=None):
        self.seed = seed
        self.knobs = KNOBS[seed % len(KNOBS)] if knobs is None else knobs
        rng = np.random.default_rng([seed, 0x434C41535346555A])
        self.kind = "escaped" if rng.random() < 0.3 else "charclass"
        alpha = int(rng.choice([2, 3, 4, 8, 26, 60]))
        ok = np.array([b for b in range(256) if b not in _NEVER and b not in (0, 10, 255)], dtype=np.uint8)
        symbols = np.concatenate([rng.permutation(ok)[:alpha], np.array([10, 0, 255], dtype=np.uint8)[:int(rng.integers(1, 4))]])
        n = int(rng.choice([1, 17, 4095, 4097, 70001, GROUP - 1, GROUP + 1, 300007, 2_000_003],
                           p=[.06, .06, .1, .1, .2, .14, .14, .14, .06]))
        long_line = rng.random() < 0.12
        npat = int(rng.choice([1, 3, 12, 60, 200]))
        if n > 300_007 or long_line:                            # (the brute-force matcher costs lines x elements x bytes)
            npat = min(npat, 20)
        if long_line:
            n = min(n, 300_007)
        maxlen = int(rng.choice([1, 2, 4, 8, 14]))
        atoms = self._atoms(rng, symbols)
        wide = [k for k, a in enumerate(atoms) if a[1].sum() > 8]
        lines, seen = [], set()
        for _ in range(npat * 4):
            if len(lines) >= npat:
                break
            L = int(rng.integers(1, maxlen + 1))
            pick = rng.integers(0, len(atoms), L)
            n_wide = 0                                          # (at most two wide classes per line: the subset
            for j in range(L):                                  # construction's states grow with their product)
                if int(pick[j]) in wide:
                    n_wide += 1
                    if n_wide > 2:
                        pick[j] = 0
            key = tuple(int(k) for k in pick)
            if key not in seen:
                seen.add(key)
                lines.append([atoms[k] for k in key])
        if long_line:                                           # one long line: the halo and the chained selection
            L = int(rng.integers(100, 1023))
            lit = [a for a in atoms if a[1].sum() == 1]
            line = [lit[int(k)] for k in rng.integers(0, len(lit), L)]
            for at in rng.integers(0, L, 3):
                line[int(at)] = atoms[int(rng.integers(0, len(atoms)))]
            lines.insert(int(rng.integers(0, len(lines) + 1)), line)
        for _ in range(int(rng.integers(0, 4))):                # duplicates, spelled again, and proper prefixes
            src = lines[int(rng.integers(0, len(lines)))]
            cut = len(src) if rng.random() < 0.5 else int(rng.integers(1, len(src) + 1))
            lines.insert(int(rng.integers(0, len(lines) + 1)), [self._respell(rng, a) for a in src[:cut]])
        self.alpha = alpha
        self.sets = [[a[1] for a in ln] for ln in lines]
        self.lines = [b"".join(a[0] for a in ln) for ln in lines]
        self.image = b"".join(ln + b"\n" for ln in self.lines)
        self.width = int(rng.choice([64, 256, 256, 1024]))
        mention = np.zeros(256, dtype=bool)
        mention[symbols] = True
        mention[[10, 0]] = True
        if rng.random() < 0.3:
            mention[:] = True                                   # every byte, 255 included
        alphabet = np.flatnonzero(mention).astype(np.uint8)
        data = alphabet[rng.integers(0, alphabet.size, n)]
        # (an instance of a line: its one-byte elements as they are, a random member for every other element)
        fixed = [np.array([int(np.argmax(s)) if s.sum() == 1 else -1 for s in ln]) for ln in self.sets]
        for at in rng.integers(0, max(n - 1, 1), max(n // 50, 1)):
            k = int(rng.integers(0, len(self.sets)))
            inst = fixed[k][:n - int(at)].copy()
            for j in np.flatnonzero(inst < 0):
                inst[j] = self._member(rng, self.sets[k][j], mention)
            data[int(at):int(at) + inst.size] = inst
        self.data = data
        self.n = n
        self.n_owned = n if rng.random() < 0.7 else int(rng.integers(0, n + 1))
        self.M = max(len(ln) for ln in lines)
        self.entry = int(rng.integers(0, self.M + 1))
        self.text_base = int(rng.choice(TEXT_BASES))
        self.reps = self.replacements(rng)
        self.plan_passes(rng)

    def _atoms(self, rng, symbols):
        """(text, members bool[256]) of about a dozen atoms; the first is a plain literal."""
        def lit(b):
            s = np.zeros(256, dtype=bool)
            s[b] = True
            return (_spell(rng, int(b)), s)
        atoms = [lit(symbols[0])] + [lit(b) for b in symbols[rng.integers(0, symbols.size, 7)]]
        atoms += [lit(b) for b in symbols[-3:]]
        if self.kind == "escaped":
            return atoms
        for _ in range(int(rng.integers(2, 7))):
            r = rng.random()
            members = symbols[rng.integers(0, symbols.size, int(rng.integers(1, 5)))]
            neg = r >= 0.6
            text = b"[" + (b"^" if neg else b"")
            s = np.full(256, neg, dtype=bool)
            if r < 0.08:                                        # the full class, in both spellings
                atoms.append((b"[\\x00-\\xff]" if r < 0.04 else b"[^]", np.ones(256, dtype=bool)))
                continue
            for b in members:
                lo = int(b)
                if rng.random() < 0.35:
                    hi = min(lo + int(rng.integers(0, 12)), 255)
                    while hi in _NEVER:
                        hi -= 1
                    text += _spell(rng, lo) + b"-" + _spell(rng, hi)
                    s[lo:hi + 1] = not neg
                else:
                    text += _spell(rng, lo)
                    s[lo] = not neg
            atoms.append((text + b"]", s))
        return atoms

    @staticmethod
    def _respell(rng, atom):
        s = atom[1]
        return (_spell(rng, int(np.flatnonzero(s)[0])), s) if s.sum() == 1 else atom

    @staticmethod
    def _member(rng, s, mention):
        """A member of the set: mostly one the input's alphabet has, now and then any, the lowest or the highest (byte
        255 of a negated class: the last column of a table in which every byte is a second byte)."""
        r = rng.random()
        both = np.flatnonzero(s & mention)
        pool = both if both.size and r < 0.7 else np.flatnonzero(s)
        if r >= 0.85:
            return int(pool[0] if r < 0.92 else pool[-1])
        return int(pool[int(rng.integers(0, pool.size))])

    def describe(self):
        return (f"seed {self.seed} {self.kind} knobs {knob_label(self.knobs)} alpha {self.alpha} lines {len(self.lines)} M {self.M} "
                f"width {self.width} n {self.n} n_owned {self.n_owned} entry {self.entry} docs {self.off.size - 1} "
                f"cuts {self.cuts} text base {self.text_base}")

    def write_patterns(self, path):
        with open(path, "wb") as f:
            f.write(self.image)
        return path

    def build_table(self, path, width=None):
        width = self.width if width is None else width
        if self.kind == "charclass":
            return PfacTable.from_charclass(path, width)
        return PfacTable.from_file(path, width, escapes=True)

    def brute(self):
        """The brute-force matcher with the kind's duplicate rule."""
        return ClassMatcher(self.image, "lowest" if self.kind == "charclass" else "last")

    def reference(self, path):
        """What the device is pinned to (close it after use): the brute-force matcher for a class table, the CPU
        oracle's escape-aware reader for an escaped file."""
        return self.brute() if self.kind == "charclass" else Oracle(path, 1, 1, escapes=True)


def run_class_case(g_factory, case, tmp_dir):
    """One case through passfuzz._run (scan twice, selection, replace, documents, chained selection) and then: the full
    (position, id) list through the outputs lists and the text of emit_records_multi (class tables), and the GPU text
    emitter at the case's base.  Escaped cases are pinned to the CPU oracle's escape-aware reader, and the brute-force
    matcher must agree with it.  Returns the number of records compared; raises AssertionError naming the case."""
    c = case
    path = c.write_patterns(os.path.join(tmp_dir, f"classfuzz_{c.seed}.pat"))
    try:
        return _run_class(g_factory, c, path, tmp_dir)
    except AssertionError as e:
        raise AssertionError(f"{c.describe()}: {e}") from e


def _run_class(g_factory, c, path, tmp_dir):
    brute = c.brute()
    matcher = brute if c.kind == "charclass" else c.reference(path)
    compared = _run(g_factory, c, path, matcher, table_factory=c.build_table, lengths=brute.lens)
    pos, ids = matcher.scan_spec(c.data, None)
    if c.kind == "escaped":
        matcher.close()
        bpos, bids = brute.scan_spec(c.data, None)
        np.testing.assert_array_equal(bpos, pos, err_msg="the brute-force matcher and the escape-aware oracle: positions")
        np.testing.assert_array_equal(bids, ids, err_msg="the brute-force matcher and the escape-aware oracle: pattern ids")
    own = pos < c.n_owned
    pos, ids = pos[own], ids[own]
    assert compared > 0 or pos.size == 0, "a non-empty reference list, and nothing compared"
    table = c.build_table(path)
    with g_factory() as g:
        g.load_table(table)
        rec = g.scan_bytes(c.data, c.n_owned)
        assert rec.size == pos.size, f"third scan: {rec.size} records, want {pos.size}"
        if c.kind == "charclass":
            fpos, fids = brute.full(c.data)
            keep = fpos < c.n_owned
            fpos, fids = fpos[keep], fids[keep]
            gpos, gids = expand(table, rec["pos"], rec["state"])
            assert gpos.size == fpos.size, f"outputs lists: {gpos.size} (position, id) pairs, want {fpos.size}"
            np.testing.assert_array_equal(gpos, fpos, err_msg="outputs lists: positions")
            np.testing.assert_array_equal(gids, fids, err_msg="outputs lists: pattern ids")
            compared += int(gpos.size)
            out = os.path.join(tmp_dir, f"classfuzz_{c.seed}.txt")
            emit_records_multi(out, rec, table)
            with open(out, "rb") as f:
                assert_text(f.read(), fpos, fids, 0, "emit_records_multi")
            os.remove(out)
        if c.n_owned:
            text = g.text_to_host(g.emit_text_device(c.text_base))
            assert_text(text, pos, ids, c.text_base, "GPU text emitter")      # (the first id of the state, once per record)
            compared += int(pos.size)
    return compared


# ---------------------------------------------------------------------------
# named automata whose shape no literal file reaches (and, as a yardstick, the most a literal file can do)

def _literal_255():
    bs = [b for b in range(256) if b != 10]
    return b"".join(bytes([a, b, 10]) for a in bs for b in bs)


def _escaped_newline_edges():
    return b"".join(b"\\x%02x\\x0a\n\\x%02x\\x%02x\n" % (a, a, a) for a in range(256))


def _random_lines(seed=60, n_lines=60, max_len=6):
    rng = np.random.default_rng(seed)
    atoms = [b"a", b"b", b"\\n", b"\\x00", b"\\xff", b"[ab]", b"[^a]", b"[^\\n]", b"[a-c]", b"[\\x00-\\xff]", b"[^b-y]", b"q"]
    return b"".join(b"".join(atoms[int(k)] for k in rng.integers(0, len(atoms), int(rng.integers(1, max_len + 1)))) + b"\n"
                    for _ in range(n_lines))


# name -> kind ("literal": a plain file; "escaped"; "charclass"), the pattern image, its (fan, depth-1 states, used
# columns, row entries), and what the device's install line must say for it: `rows` = "dense rows R x S" wherever
# depth-1 rows are allowed (R = 0: none kept), `n2` = the "depth-2 states" figure (the row entries while the packed rows
# are on, else 0) under L2 tables with fused slots, `mode` = the level-2 filter mode without a filter knob (3: most
# (first byte, second byte) combinations of the flagged bytes are prefixes).  BIG: tables beyond LDS without a knob.
SHAPES = {
    "literal-255x255": dict(kind="literal", image=_literal_255, shape=(255, 255, 255, 65025), rows="0 x 0", n2=0, mode=3),
    "columns-256": dict(kind="charclass", image=b"a[^q]\nb[^r]\n", shape=(2, 2, 256, 510), rows="2 x 256", n2=510, mode=3),
    "fan-256": dict(kind="charclass", image=b"[^q]ab\nqx\n", shape=(256, 2, 2, 256), rows="0 x 0", n2=0, mode=3),
    "fan-256-one-state": dict(kind="charclass", image=b"[^]x\n", shape=(256, 1, 1, 256), rows="0 x 0", n2=0, mode=3),
    "fan-256-full-range": dict(kind="charclass", image=b"[\\x00-\\xff]x\n", shape=(256, 1, 1, 256), rows="0 x 0", n2=0, mode=3),
    "entries-2048": dict(kind="charclass", image=b"[a-h][\\x00-\\xff]\n", shape=(8, 1, 256, 2048), rows="8 x 256", n2=2048, mode=3),
    "entries-2049": dict(kind="charclass", image=b"[a-h][\\x00-\\xff]\nix\n", shape=(9, 2, 256, 2049), rows="9 x 256", n2=0, mode=3),
    "rows-32x256": dict(kind="charclass", image=b"[a-z0-5][\\x00-\\xff]q\n", shape=(32, 1, 256, 8192), rows="32 x 256", n2=0, mode=3),
    "rows-33x256": dict(kind="charclass", image=b"[a-z0-6][\\x00-\\xff]q\n", shape=(33, 1, 256, 8448), rows="0 x 0", n2=0, mode=3),
    "root-1-255-children": dict(kind="charclass", image=b"a[^q]x\n", shape=(1, 1, 255, 255), rows="1 x 256", n2=255, mode=2),
    "root-1-two-children": dict(kind="charclass", image=b"a[bc]d\n", shape=(1, 1, 2, 2), rows="1 x 3", n2=2, mode=1),
    "dag-26-to-1": dict(kind="charclass", image=b"[a-z]bc\n[a-z]bd\n", shape=(26, 1, 1, 26), rows="26 x 2", n2=26, mode=3),
    "escaped-newline-edges": dict(kind="escaped", image=_escaped_newline_edges, shape=(256, 256, 256, 511), rows="0 x 0", n2=0, mode=2),
    "random-60-lines": dict(kind="charclass", image=_random_lines, shape=(256, 9, 256, 65536), rows="0 x 0", n2=0, mode=2),
}
BIG = ("literal-255x255", "random-60-lines")
COLUMNS_256 = [k for k, d in SHAPES.items() if d["shape"][2] == 256]


def shape_image(name):
    img = SHAPES[name]["image"]
    return img() if callable(img) else img


def shape_table(name, path, width=256):
    """Writes the image of SHAPES[name] to `path` and builds its table."""
    kind = SHAPES[name]["kind"]
    with open(path, "wb") as f:
        f.write(shape_image(name))
    if kind == "charclass":
        return PfacTable.from_charclass(path, width)
    return PfacTable.from_file(path, width, escapes=kind == "escaped")


def shape_input(name, n=150_001, seed=0):
    """Random bytes over a small alphabet plus, in places, all 256 bytes, with instances of the lines planted and -- for
    every first byte -- every byte (255 included) behind it."""
    rng = np.random.default_rng([seed, sorted(SHAPES).index(name)])
    image = shape_image(name)
    kind = SHAPES[name]["kind"]
    alphabet = np.frombuffer(b"abcdhiqrxz056\n\x00\xff", dtype=np.uint8)
    data = alphabet[rng.integers(0, alphabet.size, n)]
    wide = rng.integers(0, n - 4096, 12)
    for at in wide:
        data[int(at):int(at) + 4096] = rng.integers(0, 256, 4096)
    if kind == "charclass":
        sets = [np.array(p) for p in cco.parse(image)]
        firsts = np.flatnonzero(np.any([s[0] for s in sets], axis=0))
    else:
        lit = [ln if kind == "literal" else bytes(int(h, 16) for h in re.findall(rb"\\x(..)", ln)) for ln in image.split(b"\n") if ln]
        sets = None
        firsts = np.unique([p[0] for p in lit])
    for at in rng.integers(0, n - 8, n // 40):                  # instances of the lines
        if sets is not None:
            p = sets[int(rng.integers(0, len(sets)))]
            inst = [int(rng.choice(np.flatnonzero(e))) for e in p]
        else:
            inst = list(lit[int(rng.integers(0, len(lit)))])
        data[int(at):int(at) + len(inst)] = inst
    at = 1000                                                   # every byte behind first bytes
    for f in rng.permutation(firsts)[:24]:
        pairs = np.empty(512, dtype=np.uint8)
        pairs[0::2] = f
        pairs[1::2] = rng.permutation(256)
        data[at:at + 512] = pairs
        at += 5000
    return data

def shape_brute(name):
    """The brute-force reference of SHAPES[name], with Oracle.scan_spec's interface.  Class images go through the
    matcher as they are.  The escaped image spells byte 0x5B, which the matcher's class grammar would open a class
    with, so its lines are decoded here (two \\xNN per line) and handed to the matcher's engine as one-byte sets, the
    last of duplicate lines winning.  The 65 025 two-byte lines of the literal file have a closed form: every
    position whose byte and whose next byte are not 10 matches line 255 * rank(first) + rank(second) + 1."""
    kind, image = SHAPES[name]["kind"], shape_image(name)
    if kind == "charclass":
        return ClassMatcher(image)
    if kind == "escaped":
        eye = np.eye(256, dtype=bool)
        return ClassMatcher(image, "last", parsed=[[eye[int(h, 16)] for h in re.findall(rb"\\x(..)", ln)] for ln in image.split(b"\n") if ln])
    assert name == "literal-255x255"
    return _AllPairs()


class _AllPairs:
    def scan_spec(self, data, n=None):
        d = np.asarray(data, dtype=np.int64)
        pos = np.flatnonzero((d[:-1] != 10) & (d[1:] != 10))
        rank = d - (d > 10)
        return pos, (255 * rank[pos] + rank[pos + 1] + 1).astype(np.int32)

    def close(self):
        pass


def shape_lengths(name):
    """int64[n_lines + 1]: elements of every line of SHAPES[name], from the image's own text."""
    kind, image = SHAPES[name]["kind"], shape_image(name)
    if kind == "charclass":
        return ClassMatcher(image).lens
    return np.array([0] + [len(ln) if kind == "literal" else ln.count(b"\\x") for ln in image.split(b"\n")[:-1]], dtype=np.int64)


class ShapeCase(Case):
    """A named automaton as a case of passfuzz._run: shape_input with the last 777 bytes as halo, entry 1, random
    replacements, document offsets and chain cuts."""

    def __init__(self, name, knobs, n=150_001):
        self.seed = self.name = name
        self.knobs = knobs
        self.kind = SHAPES[name]["kind"]
        self.image = shape_image(name)
        rng = np.random.default_rng([sorted(SHAPES).index(name), 0x5348])
        self.lens = shape_lengths(name)
        self.lines = [b""] * (self.lens.size - 1)               # (only their number matters: one replacement per line)
        self.alpha, self.width = 256, 256
        self.data = shape_input(name, n)
        self.n, self.n_owned = n, n - 777
        self.M = int(self.lens.max())
        self.entry = 1
        self.reps = self.replacements(rng)
        self.plan_passes(rng)

    def write_patterns(self, path):
        with open(path, "wb") as f:
            f.write(self.image)
        return path

    def build_table(self, path, width=256):
        return shape_table(self.name, path, width)

    def brute(self):
        return shape_brute(self.name)

    def reference(self, path):
        """What the device is pinned to (close it after use): the brute-force matcher for a class table, the CPU
        oracle for a file."""
        return self.brute() if self.kind == "charclass" else Oracle(path, 1, 1, escapes=self.kind == "escaped")
