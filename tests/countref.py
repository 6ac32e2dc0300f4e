"""Host reference for the per-pattern counts (the checker, never the product): pattern ids <-> final states of a
table, histograms of a CPU matcher's records, and the counts a file of the reference's output lines holds.

A literal table's final states are the lines of the pattern file in sorted order; ``idmap[s]`` is the line (1-based id)
state s reports, and of identical lines only the last one is ever reported.  So the ids a CPU matcher returns map back
to states one to one."""
import re

import numpy as np

LINE = re.compile(rb"At position +(\d+), match pattern (\d+)\n")


def state_of_id(table):
    """int64[max id + 1]: the final state that reports pattern id i, -1 for an id no state reports (index 0, the
    losing lines of duplicates)."""
    idmap = np.asarray(table.idmap, dtype=np.int64)
    out = np.full(max(int(table.n_patterns), int(idmap.max()) if idmap.size else 0) + 1, -1, dtype=np.int64)
    out[idmap] = np.arange(idmap.size)
    return out


def states_of(table, ids):
    """The final states behind a CPU matcher's pattern ids."""
    st = state_of_id(table)[np.asarray(ids, dtype=np.int64)]
    assert (st >= 0).all(), "a reported id has no final state"
    return st


def state_counts(table, ids):
    """uint64[num_final]: how often each final state occurs among the records whose pattern ids are `ids`."""
    return np.bincount(states_of(table, ids), minlength=int(table.num_final)).astype(np.uint64)


def pattern_counts(ids, n_patterns):
    """uint64[n_patterns + 1]: how often each 1-based pattern id occurs in `ids` (entry 0 unused)."""
    return np.bincount(np.asarray(ids, dtype=np.int64), minlength=int(n_patterns) + 1).astype(np.uint64)


def parse_counts(text, n_patterns):
    """Counts by pattern id of the lines "At position %4d, match pattern %d" in `text` (bytes); every byte of the text
    must belong to such a line.  Returns (counts uint64[n_patterns + 1], lines)."""
    ids = [int(m.group(2)) for m in LINE.finditer(text)]
    assert sum(m.end() - m.start() for m in LINE.finditer(text)) == len(text), "text holds something else than match lines"
    return pattern_counts(np.array(ids, dtype=np.int64), n_patterns), len(ids)


def walk_state_counts(table, data):
    """uint64[num_final] by the table's own lookup, walked from every start offset on the host (small inputs)."""
    data = np.asarray(data, dtype=np.uint8)
    counts = np.zeros(int(table.num_final), dtype=np.uint64)
    root = table.num_final + 1
    for i in range(data.size):
        s = root
        for j in range(i, data.size):
            s = table.lookup(s, int(data[j]))
            if s < 0:
                break
            if s < table.num_final:
                counts[s] += np.uint64(1)
    return counts


def brute_counts(lines, data):
    """uint64[len(lines) + 1]: occurrences (overlapping) of every distinct line in `data`, credited to the LAST of
    identical lines (the reference's duplicate rule)."""
    data = bytes(np.asarray(data, dtype=np.uint8))
    out = np.zeros(len(lines) + 1, dtype=np.uint64)
    winner = {p: i for i, p in enumerate(lines, start=1)}
    for p, i in winner.items():
        out[i] = sum(data.startswith(p, k) for k in range(len(data)))
    return out
