"""Two independent host references for replacement templates and match extraction (the checker, never the product),
and the named inputs of the GPU tests.

A template belongs to a pattern id: bytes (a plain replacement R) or a pair (prefix, suffix), which rewrites a pick
(p, L) to prefix + input[p : p + L] + suffix -- the input's bytes as they were written, whatever the matcher folded.
With picks (p_k, L_k) made from `entry` over a range that owns [0, n_owned), E_k the rewritten pick k:

    replace    input[entry : p_0] + E_0 + input[p_0 + L_0 : p_1] + E_1 + ... + E_{n-1} + input[p_{n-1} + L_{n-1} : n_owned]
    extract    E_0 + E_1 + ... + E_{n-1},   pick_off[k] = |E_0| + ... + |E_{k-1}|,   pick_off[n] = the length

(a) `from_records`: `llref.greedy` over a matcher's records (the CPU oracle's), then `assemble`, a plain loop over
    the picks that builds both outputs.
(b) `re_templates`: for plain literal sets, Python `re` over the longest-first alternation (`replref.re_replace`'s),
    `re.sub` with a function replacement for the replace and `re.finditer` for the extraction; `re.IGNORECASE` for a
    folded table.

Both return `Result(replaced, extracted, pick_off, exit, n_picks)`.  Templates are kept as this file's own dict
{id: bytes | (prefix, suffix)} (`by_id`); nothing here reads the product's table layout."""
import collections
import re

import numpy as np

from llref import greedy

Result = collections.namedtuple("Result", "replaced extracted pick_off exit n_picks")


def by_id(templates):
    """dict {id: template} or one template per pattern line -> dict {id: bytes | (bytes, bytes)}."""
    items = templates.items() if isinstance(templates, dict) else enumerate(templates, start=1)
    out = {}
    for i, t in items:
        out[int(i)] = bytes(t) if isinstance(t, (bytes, bytearray)) else (bytes(t[0]), bytes(t[1]))
    return out


def rewrite(template, matched):
    return template if isinstance(template, bytes) else template[0] + matched + template[1]


def assemble(data, entry, n_owned, pos, lens, ids, templates):
    """The plain loop: picks (pos, lens, ids) in ascending pos, made from `entry`."""
    data = bytes(np.asarray(data, dtype=np.uint8))
    tpl = by_id(templates)
    entry, n_owned = int(entry), int(n_owned)
    rep, ext, off, c = [], [], [0], entry
    for p, L, i in zip(np.asarray(pos).tolist(), np.asarray(lens).tolist(), np.asarray(ids).tolist()):
        assert p >= c and L >= 1 and p < n_owned
        e = rewrite(tpl[i], data[p:p + L])
        rep.append(data[c:p])
        rep.append(e)
        ext.append(e)
        off.append(off[-1] + len(e))
        c = p + L
    if c < n_owned:
        rep.append(data[c:n_owned])
    return Result(b"".join(rep), b"".join(ext), np.array(off, dtype=np.uint64), max(c, n_owned) - n_owned, len(ext))


def from_records(data, entry, n_owned, pos, lens, ids, templates):
    """(a): the greedy over the records (pos, lens, ids) that start in [0, n_owned), in (pos, len) order."""
    pos = np.asarray(pos, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    keep = pos < int(n_owned)
    pos, lens, ids = pos[keep], lens[keep], ids[keep]
    sel, ex = greedy(pos, lens, entry, n_owned)
    r = assemble(data, entry, n_owned, pos[sel], lens[sel], ids[sel], templates)
    assert r.exit == ex
    return r


def re_templates(patterns, templates, data, entry, n_owned, ignore_case=False):
    """(b): plain literal patterns (one per line, id = line number; the last of equal lines wins)."""
    data = bytes(np.asarray(data, dtype=np.uint8))
    tpl = by_id(templates)
    entry, n_owned = int(entry), int(n_owned)
    key = (lambda b: b.lower()) if ignore_case else (lambda b: b)       # (bytes.lower() folds ASCII only, as the scan does)
    winner = {}
    for i, p in enumerate(patterns, start=1):
        winner[key(bytes(p))] = i
    alt = re.compile(b"|".join(re.escape(p) for p in sorted(winner, key=len, reverse=True)), re.IGNORECASE if ignore_case else 0)
    # the picks that start in the owned range, and where the output ends
    ext, off, c = [], [0], entry
    if entry < n_owned:
        for m in alt.finditer(data, entry):
            if m.start() >= n_owned:
                break
            e = rewrite(tpl[winner[key(m.group(0))]], m.group(0))
            ext.append(e)
            off.append(off[-1] + len(e))
            c = m.end()
    end = max(c, n_owned)
    # no pick is cut by `end` and none starts in [n_owned, end): the substitution over data[entry:end] is the replace
    replaced = alt.sub(lambda m: rewrite(tpl[winner[key(m.group(0))]], m.group(0)), data[entry:end]) if entry < end else b""
    return Result(replaced, b"".join(ext), np.array(off, dtype=np.uint64), end - n_owned, len(ext))


def fixed_replacements(patterns, templates):
    """Exact-case literal sets only: the fixed replacement that writes what the template writes, per line --
    prefix + pattern + suffix.  (The identity behind the timing baseline of tools/template_bench.py.)"""
    tpl = by_id(templates)
    return [rewrite(tpl[i], bytes(p)) for i, p in enumerate(patterns, start=1)]


# ---------------------------------------------------------------------------
# named inputs of tests/test_gpu_templates.py; tests/test_template_ref.py asserts their pick counts on the host

WORKED_DATA = b"xabcabcd"
WORKED_SETS = (
    # a deletion, split = 0, split = R, 0 < split < R with a prefix longer than 4 KiB
    {1: b"", 2: (b"", b"Z"), 3: (b"BC", b""), 4: (b"L" * 5000, b"R")},
    {1: (b"<", b">"), 2: b"", 3: (b"[", b"]"), 4: (b"<<", b">>")},
    {1: b"1", 2: (b"(", b")"), 3: b"", 4: b""},
)

EDGE_PATTERNS = [b"abcdefg", b"bc", b"fgh", b"h"]
EDGE_PARA = b"xxabcdefghyhbcfgh"
EDGE_TEMPLATES = {1: (b"<", b"/7>"), 2: b"", 3: (b"", b"!"), 4: (b"hhhhhhhhhhhhhhhhh", b"")}
EDGE_SIZES = (0, 1, 15, 16, 17, 4095, 4096, 4097, 70001)

COUNT_PATTERNS = [b"ab"]
COUNT_UNIT = b"xab.."
COUNT_TEMPLATES = {1: (b"<b>", b"</b>!")}
PICK_COUNTS = (63, 64, 65, 1023, 1024, 1025)


def count_input(k):
    """Exactly k picks of `ab`, one per 5 bytes, and 3 bytes behind the last."""
    return np.frombuffer(COUNT_UNIT * k + b"end", dtype=np.uint8)


EMPTY_PATTERNS = [b"d", b"q"]
EMPTY_TEMPLATES = {1: b"", 2: (b"[", b"]")}


def empty_blocks_input():
    """Runs of plain deletions with nothing between them -- 70 (past one block of 64 picks), 64 * 64 + 5 (past one round
    of the gallop) -- each followed by a quoting pick."""
    return np.frombuffer(b"pre" + b"d" * 70 + b"q" + b"xyz" + b"d" * (64 * 64 + 5) + b"qq" + b"d" * 64 + b"q.tail", dtype=np.uint8)


BIG_PATTERNS = [b"ab"]
BIG_UNIT = b"ab" + b"." * 12                     # 14 bytes in; 12 + 1001 out replaced, 1001 extracted: odd periods
BIG_TEMPLATES = {1: (b"P" * 500, b"S" * 499)}
BIG_PERIODS = 70_000                            # 70 000 * 1013 B = 67.6 MiB replaced, 70 000 * 1001 B = 66.8 MiB extracted


def a_runs(n, run):
    data = np.full(n, ord("a"), dtype=np.uint8)
    data[run::run + 1] = ord("b")
    return data


def aa_picks(n, run):
    """How many non-overlapping `aa` the greedy takes from a_runs(n, run): floor(r / 2) of every run of r a's."""
    full, rest = divmod(n, run + 1)
    return full * (run // 2) + min(rest, run) // 2
