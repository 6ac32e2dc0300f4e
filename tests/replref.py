"""Two independent host references for find-and-replace over the leftmost-longest selection (the checker, never the
product).  The output of a range scanned from `entry` with picks (p_k, L_k) and replacements R_k is

    input[entry : p_0] + R_0 + input[p_0 + L_0 : p_1] + ... + R_{n-1} + input[p_{n-1} + L_{n-1} : n_owned]

(a slice with end <= start is empty).

(a) `greedy_replace`: `llref.greedy` over a matcher's records, then `splice`, which is vectorised with numpy and works
    through the picks in chunks, so it also builds the expectation of a 1 GiB selection that `check_greedy` has pinned.
(b) `re_replace`: for plain literal sets, Python `re` over an alternation of the escaped patterns sorted longest first --
    leftmost-longest for literals -- with the replacement of the matched text's winning (last) line.

Replacements are keyed by pattern id: `rep_table(reps)` -> (offsets int64[max_id + 2], bytes), id i = bytes[off[i] :
off[i + 1]] for a dict {id: bytes} or a sequence with one entry per line (reps[id - 1])."""
import re

import numpy as np

from llref import greedy


def rep_table(reps):
    if isinstance(reps, dict):
        top = max(reps) if reps else 0
        items = [bytes(reps.get(i, b"")) for i in range(top + 1)]
    else:
        items = [b""] + [bytes(r) for r in reps]
    off = np.zeros(len(items) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in items])
    return off, b"".join(items)


def _gather_ranges(starts, lens):
    """int64 indices of the concatenation of the ranges [starts[i], starts[i] + lens[i])."""
    keep = lens > 0
    starts, lens = starts[keep], lens[keep]
    total = int(lens.sum())
    if total == 0:
        return np.empty(0, dtype=np.int64)
    step = np.ones(total, dtype=np.int64)
    at = np.cumsum(lens)[:-1]
    step[0] = starts[0]
    step[at] = starts[1:] - (starts[:-1] + lens[:-1] - 1)
    return np.cumsum(step)


def splice(data, entry, n_owned, pos, lens, ids, table, chunk=1 << 20):
    """The output for picks (pos, lens) in ascending pos with pattern ids `ids`, replacements from `rep_table`."""
    data = np.asarray(data, dtype=np.uint8)
    off, rb = table
    rep = np.frombuffer(rb, dtype=np.uint8) if rb else np.zeros(0, dtype=np.uint8)
    pos = np.asarray(pos, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    entry, n_owned = int(entry), int(n_owned)
    n = pos.size
    rstart = off[ids] if n else np.empty(0, dtype=np.int64)
    rlen = off[ids + 1] - rstart if n else np.empty(0, dtype=np.int64)
    ends = pos + lens
    prev = np.concatenate(([entry], ends[:-1])) if n else np.empty(0, dtype=np.int64)
    assert (pos >= prev).all(), "picks overlap or start before the entry"
    parts = []
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        glen = pos[a:b] - prev[a:b]
        tot = int(glen.sum() + rlen[a:b].sum())
        out = np.empty(tot, dtype=np.uint8)
        # piece order: gap_k, rep_k; place each into `out` through its output offset
        seg = glen + rlen[a:b]
        o = np.concatenate(([0], np.cumsum(seg)[:-1]))
        out[_gather_ranges(o, glen)] = data[_gather_ranges(prev[a:b], glen)]
        out[_gather_ranges(o + glen, rlen[a:b])] = rep[_gather_ranges(rstart[a:b], rlen[a:b])]
        parts.append(out)
    c = int(ends[-1]) if n else entry
    parts.append(data[c:n_owned] if c < n_owned else np.zeros(0, dtype=np.uint8))
    return np.concatenate(parts) if len(parts) > 1 else parts[0].copy()


def greedy_replace(data, entry, n_owned, pos, lens, ids, table):
    """(a): the greedy over the records (pos, lens, ids) that start in [0, n_owned), in (pos, len) order -> (output,
    exit)."""
    pos = np.asarray(pos, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    keep = pos < int(n_owned)
    pos, lens, ids = pos[keep], lens[keep], ids[keep]
    sel, ex = greedy(pos, lens, entry, n_owned)
    return splice(data, entry, n_owned, pos[sel], lens[sel], ids[sel], table), ex


def re_replace(patterns, reps, data, entry, n_owned):
    """(b): plain literal patterns (one per line, id = line number); -> (output, exit)."""
    data = bytes(np.asarray(data, dtype=np.uint8))
    entry, n_owned = int(entry), int(n_owned)
    off, rb = rep_table(reps)
    winner = {}
    for i, p in enumerate(patterns, start=1):
        winner[bytes(p)] = i                                    # the last of duplicate lines wins
    alt = b"|".join(re.escape(p) for p in sorted(winner, key=len, reverse=True))
    out, c = [], entry
    if entry < n_owned:
        for m in re.finditer(alt, data[entry:]):
            s = entry + m.start()
            if s >= n_owned:
                break
            i = winner[m.group(0)]
            out.append(data[c:s])
            out.append(rb[off[i]:off[i + 1]])
            c = entry + m.end()
    if c < n_owned:
        out.append(data[c:n_owned])
    return np.frombuffer(b"".join(out), dtype=np.uint8), max(c, n_owned) - n_owned
