"""Host reference for batches of documents (the checker, never the product): every document scanned on its own by the
CPU oracle, positions relative to the document; and seeded document cuts."""
import numpy as np


def oracle_per_doc(o, buf, off):
    """(doc_first, pos, ids) of scanning every document [off[d], off[d+1]) of buf on its own."""
    first = np.zeros(off.size, dtype=np.uint64)
    pos, ids = [], []
    k = 0
    for d in range(off.size - 1):
        a, b = int(off[d]), int(off[d + 1])
        first[d] = k
        if b > a:
            p, i = o.scan_spec(np.ascontiguousarray(buf[a:b]))
            pos.append(p)
            ids.append(i)
            k += p.size
    first[-1] = k
    pos = np.concatenate(pos) if pos else np.empty(0, np.int64)
    ids = np.concatenate(ids) if ids else np.empty(0, np.int32)
    return first, pos, ids


def random_offsets(rng, n, n_docs, empties=0):
    cuts = np.sort(rng.integers(0, n + 1, n_docs - 1))
    off = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
    if empties:
        at = rng.integers(0, off.size, empties)
        off = np.sort(np.concatenate([off, off[at]]))
    return off
