"""Two independent host references for leftmost-longest, non-overlapping selection (the checker, never the product).

The rule: from a cursor c = entry take the smallest position p >= c that has a record, select the longest record there,
set c = p + len, repeat; exit = max(c_final, n_owned) - n_owned (c_final = entry when nothing is picked).

`greedy` is that rule as a plain loop.  `check_greedy` characterises a given selection with vectorised searches over the
candidate positions, so it runs on the hundreds of millions of records of a 1 GiB scan.  Both take the records as
(pos, len) arrays sorted by (pos, len) -- the scan's output order -- with lengths from the pattern file's own lines."""
import numpy as np


def line_lengths(pattern_path):
    """int64[n_lines + 1]: [id] = byte length of line id of a plain pattern file (ids count from 1)."""
    lines = open(pattern_path, "rb").read()
    if lines.endswith(b"\n"):
        lines = lines[:-1]
    return np.array([0] + [len(x) for x in lines.split(b"\n")], dtype=np.int64)


def greedy(pos, lens, entry, n_owned):
    """-> (indices into pos of the selected records, exit)."""
    pos = np.asarray(pos, dtype=np.int64).tolist()
    lens = np.asarray(lens, dtype=np.int64).tolist()
    sel = []
    c = int(entry)
    i, n = 0, len(pos)
    while i < n:
        p = pos[i]
        best = i
        j = i + 1
        while j < n and pos[j] == p:
            if lens[j] >= lens[best]:
                best = j
            j += 1
        if p >= c:
            sel.append(best)
            c = p + lens[best]
        i = j
    return np.array(sel, dtype=np.int64), max(c, int(n_owned)) - int(n_owned)


def check_greedy(pos, lens, selected, entry, n_owned):
    """Asserts that `selected` = (sel_pos, sel_len) is THE greedy selection of the records (pos, lens) from `entry`;
    returns the exit it implies."""
    pos = np.asarray(pos, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    sp = np.asarray(selected[0], dtype=np.int64)
    sl = np.asarray(selected[1], dtype=np.int64)
    assert sp.size == sl.size
    # candidates: every position with a record, with its greatest length
    if pos.size:
        last = np.append(pos[1:] != pos[:-1], True)
        cp = pos[last]
        cl = np.maximum.reduceat(lens, np.flatnonzero(np.append(True, pos[1:] != pos[:-1])))
    else:
        cp = cl = np.empty(0, dtype=np.int64)
    first = np.searchsorted(cp, int(entry), side="left")
    if sp.size == 0:
        assert first == cp.size, "nothing selected, but a record lies at or after the entry"
        return max(int(entry), int(n_owned)) - int(n_owned)
    # a subset of the candidates, each the longest at its position
    at = np.searchsorted(cp, sp, side="left")
    assert (at < cp.size).all(), "a selected position has no record"
    assert (cp[at] == sp).all(), "a selected position has no record"
    assert (cl[at] == sl).all(), "a selected record is not the longest at its position"
    # the first pick is the first candidate >= entry; each next one the first at or after the previous end
    assert at[0] == first, "the first pick is not the first candidate at or after the entry"
    ends = sp + sl
    assert (at[1:] == np.searchsorted(cp, ends[:-1], side="left")).all(), "a pick is not the first after the previous end"
    # nothing at or after the last end
    assert np.searchsorted(cp, ends[-1], side="left") == cp.size, "a candidate lies after the last pick's end"
    return max(int(ends[-1]), int(n_owned)) - int(n_owned)
