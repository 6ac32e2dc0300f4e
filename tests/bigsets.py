"""Seeded pattern sets whose automata sit exactly at the bit-width limits of the scan's packed words (include/pfac.h,
phfpfac_amd/csrc/pfac_hip.hip build_plan, pfac_table.c's size check), and the inputs that drive them.

What the generators rely on (pfac_table.c build_from_patterns):
- the final states are 0..F-1 in sorted pattern order (F = lines, duplicates included), so the greatest pattern owns
  final state F - 1; the root is F + 1;
- state_num = distinct non-empty prefixes + duplicate lines + 2, and the other states are numbered in the order the
  sorted list first reaches them, so a byte added to a leaf pattern adds exactly one state and the last new prefix of
  the greatest pattern is state state_num - 1.
``trie_stats`` computes these numbers from the lines alone; every set states what it must hit and ``check`` compares
that with the ``PfacTable`` the product builds."""
import numpy as np

from passfuzz import Case

LIMIT = (2**31 - 1) // 256           # largest state_num + pattern bytes the builder accepts (pfac_table.c)
TILE = 4096                          # the 12 position bits of a compact record
LOWER = np.arange(97, 123, dtype=np.uint8)


def trie_stats(lines):
    """{state_num, num_final, max_pat_len, n2} of the trie of `lines` (no byte 0 or newline in them), n2 = states at
    depth 2 = distinct two-byte prefixes."""
    uniq = sorted(set(lines))
    lens = np.array([len(p) for p in uniq], dtype=np.int64)
    M = int(lens.max())
    rows = np.frombuffer(b"".join(p.ljust(M, b"\0") for p in uniq), dtype=np.uint8).reshape(len(uniq), M)
    eq = rows[1:] == rows[:-1]
    lcp = np.where(eq.all(axis=1), M, np.argmin(eq, axis=1))       # (distinct rows: never all equal)
    prefixes = int(lens.sum() - lcp.sum())
    two = rows[lens >= 2, :2].astype(np.int64)
    n2 = np.unique(two[:, 0] * 256 + two[:, 1]).size
    return {"state_num": prefixes + len(lines) - len(uniq) + 2, "num_final": len(lines), "max_pat_len": M, "n2": int(n2)}


class PatternSet:
    """A named pattern list (file order) with the statistics it was built to hit and the symbols of its inputs."""

    def __init__(self, name, lines, want, alphabet, greatest):
        self.name, self.lines, self.want = name, lines, want
        self.alphabet = np.asarray(alphabet, dtype=np.uint8)
        self.greatest = greatest                         # the pattern of final state F - 1
        self.M = max(len(p) for p in lines)

    def image(self):
        return b"\n".join(self.lines) + b"\n"

    def write(self, path):
        with open(path, "wb") as f:
            f.write(self.image())
        return str(path)

    def check(self, table):
        """The product's table has the statistics the set was built to hit (``want``: a subset of trie_stats's keys,
        plus ``walks``: (bytes, state) pairs the table's own lookup must reach)."""
        for k in ("state_num", "num_final", "max_pat_len"):
            if k in self.want:
                assert getattr(table, k) == self.want[k], (self.name, k, getattr(table, k), self.want[k])
        assert table.idmap[table.num_final - 1] == self.lines.index(self.greatest) + 1
        for path, state in self.want.get("walks", []):
            assert walk(table, path) == state, (self.name, path, walk(table, path), state)
        if "n2" in self.want:
            d1 = [int(s) for s in table.s0 if s >= 0]
            n2 = sum(table.lookup(s, c) >= 0 for s in d1 for c in range(256))
            assert n2 == self.want["n2"], (self.name, "n2", n2, self.want["n2"])


def walk(table, path):
    s = int(table.s0[path[0]])
    for ch in path[1:]:
        s = table.lookup(s, ch)
    return s


def _unique_random(rng, n, lengths, alphabet, exclude=(), heads=None):
    """n distinct random strings over `alphabet` with lengths drawn from `lengths`, none in `exclude`; with `heads`
    their first two bytes come from that alphabet instead."""
    out = dict.fromkeys(exclude)
    k = len(out)
    while len(out) < n + k:
        m = int((n + k - len(out)) * 1.1) + 16
        lens = rng.choice(lengths, m)
        rows = alphabet[rng.integers(0, alphabet.size, (m, max(lengths)))]
        if heads is not None:
            rows[:, :2] = heads[rng.integers(0, heads.size, (m, 2))]
        for r, L in zip(rows, lens.tolist()):
            out.setdefault(r[:L].tobytes())
            if len(out) == n + k:
                break
    return list(out)[k:]


def _shuffle(rng, lines):
    return [lines[i] for i in rng.permutation(len(lines))]


def _stretch(rng, leaves, deficit, alphabet):
    """Append `deficit` random bytes over the leaf patterns `leaves` (each byte adds one state)."""
    q, r = divmod(deficit, len(leaves))
    out = []
    for i, p in enumerate(leaves):
        k = q + (i < r)
        out.append(p + alphabet[rng.integers(0, alphabet.size, k)].tobytes() if k else p)
    return out


def dict_set(seed=1):
    """DICT: 466 544 lowercase words, lengths 1 to 45, 1.4 M states or more -- the shape of the reference's largest
    dictionary: 26 dense depth-1 rows, left unpacked because the state count exceeds 2^20."""
    rng = np.random.default_rng([seed, 0xD1C7])
    n = 466_544
    p = np.exp(-0.5 * ((np.arange(1, 46) - 8.0) / 2.6) ** 2) + 2e-4     # most words 5 to 11 letters, a tail to 45
    lens = np.arange(1, 46)
    freq = np.array([8.2, 1.5, 2.8, 4.3, 12.7, 2.2, 2.0, 6.1, 7.0, .2, .8, 4.0, 2.4, 6.7, 7.5, 1.9, .1, 6.0, 6.3, 9.1,
                     2.8, 1.0, 2.4, .2, 2.0, .1])                    # English letter frequencies
    words = dict()
    while len(words) < n:
        m = n - len(words) + 1000
        ls = rng.choice(lens, m, p=p / p.sum())
        rows = LOWER[rng.choice(26, (m, 45), p=freq / freq.sum())]
        for r, L in zip(rows, ls.tolist()):
            words.setdefault(r[:L].tobytes())
    lines = _shuffle(rng, list(words)[:n])
    st = trie_stats(lines)
    assert st["state_num"] >= 1_400_000 and st["max_pat_len"] == 45 and st["num_final"] == n
    return PatternSet("DICT", lines, st, LOWER, max(lines))


def final_set(F, seed=2):
    """F65535 / F65536: exactly F final states, state_num <= 2^20, at most 2048 depth-2 states; the greatest pattern
    is the single byte '~', so a depth-1 state is final state F - 1 (dense mode's second form writes "not final" as
    0xFFFF in its root table)."""
    rng = np.random.default_rng([seed, F])
    first = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEF", dtype=np.uint8)
    lines = _unique_random(rng, F - 1, [3, 4, 5], LOWER, heads=first)
    lines.insert(int(rng.integers(0, len(lines) + 1)), b"~")
    st = trie_stats(lines)
    assert st["num_final"] == F and st["state_num"] <= 1 << 20 and st["n2"] <= 2048
    alpha = np.unique(np.concatenate([first, LOWER, [ord("~")]]))
    return PatternSet(f"F{F}", lines, dict(st, walks=[(b"~", F - 1)]), alpha, b"~")


def state_set(S, seed=3):
    """S2^20 / S2^20+1: state_num exactly S, at most 65 535 final states and 2048 depth-2 states; the greatest pattern
    "~}a" makes its depth-2 prefix "~}" the last state numbered, S - 1."""
    rng = np.random.default_rng([seed, S])
    first = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCD", dtype=np.uint8)
    F = 60_000
    base = _unique_random(rng, F, [19], LOWER, heads=first)             # all 19 bytes long and distinct: leaves
    greatest = b"~}a"
    st = trie_stats(base + [greatest])
    assert st["state_num"] <= S
    lines = _stretch(rng, base, S - st["state_num"], LOWER) + [greatest]
    lines = _shuffle(rng, lines)
    st = trie_stats(lines)
    assert st["state_num"] == S and st["num_final"] <= 65535 and st["n2"] <= 2048
    alpha = np.unique(np.concatenate([first, LOWER, np.frombuffer(b"~}", dtype=np.uint8)]))
    return PatternSet(f"S{S}", lines, dict(st, walks=[(b"~}", S - 1), (greatest, st["num_final"] - 1)]), alpha, greatest)


def depth2_set(n2, seed=4):
    """N2048 / N2049: exactly n2 depth-2 states (46 symbols: 45^2 = 2025 pairs are too few), some of them final."""
    rng = np.random.default_rng([seed, n2])
    sym = np.arange(0x30, 0x30 + 46, dtype=np.uint8)
    pairs = rng.permutation(46 * 46)[:n2]
    pairs = np.sort(pairs)
    pairs = pairs[pairs != 45 * 46 + 45]                               # ']]' is the greatest pattern's prefix
    pairs = np.append(pairs[:n2 - 1], 45 * 46 + 45)
    lines = []
    for k, pr in enumerate(pairs.tolist()):
        head = bytes([sym[pr // 46], sym[pr % 46]])
        if k % 3 == 0:
            lines.append(head)                                         # a final depth-2 state
        lines += [head + t for t in _unique_random(rng, 8, [1, 2, 3, 4], sym)]
    greatest = bytes([sym[45]]) * 6
    lines = [p for p in lines if p < greatest] + [greatest]
    lines = _shuffle(rng, lines)
    st = trie_stats(lines)
    assert st["n2"] == n2 and st["num_final"] <= 65535
    return PatternSet(f"N{n2}", lines, st, sym, greatest)


def wide_set(F, seed=5):
    """F2^20 / F2^20+1: exactly F patterns of 5 or 6 lowercase letters; the greatest, "zzzzzz", is the last line, so
    its final state is F - 1 and its id F.  F2^20's is the 4-byte record word pos:12 | state:20 = 0xFFFFFFFF at tile
    offset 4095; F2^20+1 needs 8-byte records, with state 2^20 and id 2^20 + 1."""
    rng = np.random.default_rng([seed, F])
    greatest = b"zzzzzz"
    lines = _unique_random(rng, F - 1, [5, 6], LOWER, exclude=[greatest]) + [greatest]
    st = trie_stats(lines)
    assert st["num_final"] == F and st["max_pat_len"] == 6
    return PatternSet(f"F{F}", lines, st, LOWER, greatest)


def near_limit_set(seed=6):
    """NEAR_LIMIT: lines + 2 + pattern bytes exactly at the builder's limit (keys (state << 8) + byte in int32):
    493 447 patterns of 16 letters, 6 of them 17."""
    rng = np.random.default_rng([seed, LIMIT])
    n = (LIMIT - 2) // 17
    extra = LIMIT - 2 - 17 * n
    lines = _unique_random(rng, n, [16], LOWER)
    lines = _stretch(rng, lines[:extra], extra, LOWER) + lines[extra:]
    greatest = max(lines)
    assert len(lines) + 2 + sum(len(p) for p in lines) == LIMIT
    return PatternSet("NEAR_LIMIT", lines, {"num_final": n, "max_pat_len": 17}, LOWER, greatest)


def over_limit(s):
    """NEAR_LIMIT with one byte more: the builder must refuse it."""
    lines = list(s.lines)
    lines[0] = lines[0] + b"q"
    return b"\n".join(lines) + b"\n"


BUILDERS = {"DICT": dict_set, "F65535": lambda: final_set(65535), "F65536": lambda: final_set(65536),
            "S2^20": lambda: state_set(1 << 20), "S2^20+1": lambda: state_set((1 << 20) + 1),
            "N2048": lambda: depth2_set(2048), "N2049": lambda: depth2_set(2049),
            "F2^20": lambda: wide_set(1 << 20), "F2^20+1": lambda: wide_set((1 << 20) + 1), "NEAR_LIMIT": near_limit_set}


# ---------------------------------------------------------------------------- inputs
def word_text(s, n, seed=7):
    """`n` bytes of the set's own words separated by spaces (the match-dense "dictionary on text" case)."""
    rng = np.random.default_rng([seed, n])
    pick = rng.integers(0, len(s.lines), n // 3 + 16)
    out, size = [], 0
    for i in pick.tolist():
        out.append(s.lines[i])
        size += len(s.lines[i]) + 1
        if size >= n:
            break
    return np.frombuffer(b" ".join(out)[:n], dtype=np.uint8).copy()


def planted_random(s, n, seed=8):
    """`n` random bytes over the set's symbols with one pattern planted every ~50 bytes."""
    rng = np.random.default_rng([seed, n])
    data = s.alphabet[rng.integers(0, s.alphabet.size, n)]
    for at in rng.integers(0, max(n - 1, 1), max(n // 50, 1)).tolist():
        p = np.frombuffer(s.lines[int(rng.integers(0, len(s.lines)))], dtype=np.uint8)
        m = min(p.size, n - at)
        data[at:at + m] = p[:m]
    return data


def adversarial(s, n, seed=9):
    """(data, n_owned): random symbols with the greatest pattern (final state F - 1) at tile offsets 0 and 4095 of
    several tiles, on the last owned byte, straddling the owned end into the halo, on the first halo byte and cut off
    by the end of the buffer.  n_owned = n - (M - 1), a shard's owned range."""
    rng = np.random.default_rng([seed, n])
    data = s.alphabet[rng.integers(0, s.alphabet.size, n)]
    g = np.frombuffer(s.greatest, dtype=np.uint8)
    n_owned = n - (s.M - 1)
    spots = []
    for t in range(0, n_owned // TILE - 1, 7):
        spots += [t * TILE, t * TILE + TILE - 1]
    spots += [n_owned - 1, n_owned - max(g.size // 2, 1), n_owned, n - g.size + 1]
    for at in spots:
        m = min(g.size, n - at)
        data[at:at + m] = g[:m]
    return data, n_owned


class BigCase(Case):
    """A tests/passfuzz.py case over one of these sets: the set's lines, a given input and owned range, and seeded
    entry, replacements (0 to 64 bytes each, drawn in one go), documents and chained-selection cuts."""

    def __init__(self, s, data, n_owned, seed, width=256, knobs=None):
        self.seed, self.knobs = seed, dict(knobs or {})
        self.lines, self.alpha, self.M, self.width = s.lines, int(s.alphabet.size), s.M, width
        self.data, self.n, self.n_owned = data, int(data.size), int(n_owned)
        rng = np.random.default_rng([seed, 0xB16CA5E])
        self.entry = int(rng.integers(0, self.M + 1))
        self.reps = self.replacements(rng)
        self.plan_passes(rng)

    def replacements(self, rng):
        lens = rng.integers(0, 65, len(self.lines))
        off = np.concatenate([[0], np.cumsum(lens)]).tolist()
        blob = rng.integers(0, 256, off[-1]).astype(np.uint8).tobytes()
        return {i + 1: blob[off[i]:off[i + 1]] for i in range(len(self.lines))}
