"""Host reference for the per-document selection and find-and-replace (the checker, never the product): the CPU oracle
run on every document on its own (docref.oracle_per_doc), then llref.greedy and replref.splice applied to each document,
lengths from the pattern file's own lines."""
import numpy as np

from docref import oracle_per_doc
from llref import greedy
from replref import splice


def per_doc(o, buf, off, ll, table=None):
    """-> (doc_first uint64[n_docs + 1], pos (relative to the document), ids, out_off uint64[n_docs + 1], out): every
    document's leftmost-longest selection from cursor 0, and with `table` (replref.rep_table) its output, concatenated.
    `o` is anything with Oracle.scan_spec's interface."""
    buf = np.asarray(buf, dtype=np.uint8)
    first, pos, ids = oracle_per_doc(o, buf, off)
    n_docs = off.size - 1
    sfirst = np.zeros(off.size, dtype=np.uint64)
    out_off = np.zeros(off.size, dtype=np.uint64)
    sp, si, outs = [], [], []
    k = ob = 0
    for d in range(n_docs):
        a, b = int(off[d]), int(off[d + 1])
        p, i = pos[int(first[d]):int(first[d + 1])], ids[int(first[d]):int(first[d + 1])]
        s, _ = greedy(p, ll[i], 0, b - a)
        sfirst[d], out_off[d] = k, ob
        k += s.size
        sp.append(p[s])
        si.append(i[s])
        if table is not None:
            od = splice(buf[a:b], 0, b - a, p[s], ll[i[s]], i[s], table)
            outs.append(od)
            ob += od.size
    sfirst[-1], out_off[-1] = k, ob
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.empty(0, dt)      # noqa: E731
    return sfirst, cat(sp, np.int64), cat(si, np.int32), out_off, cat(outs, np.uint8)
