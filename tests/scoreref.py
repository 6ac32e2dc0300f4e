"""Host reference for document scores (the checker, never the product): a weighted match sum and a match count per
document, the predicate over them, and the preconditions that make the cases of tests/test_gpu_scores.py test what
they are named for.  Nothing comes from the device.

The reference (`scores_cut`): the whole-buffer records (pos, pattern id, length) cut by the rule of include/pfac.h --
record -> the last document with off[d] <= pos, kept iff pos + len <= off[d + 1] -- then per document the count of the
kept records and the sum of their patterns' weights in int64.  `scores_by_find` is held against it in
tests/test_score_ref.py: overlapping bytes.find of every pattern in the document's own bytes, no matcher involved.
Weights are given per 1-based pattern id; `weights_for` cycles through a zero, a cancelling pair and both int32
extremes.  The scans and offsets are those of tests/groupref.py (`cases()`, `TILES`, `SHAPES`)."""
import numpy as np

from groupref import RANGE, SHAPES, TILES, cases  # noqa: F401  (the GPU tests take them from here)

SCORE = np.dtype([("score", "<i8"), ("count", "<u8")])          # struct pfac_doc_score, written apart from the product's
CYCLE = (3, 0, -3, 1, -(2 ** 31), 2 ** 31 - 1, -1)
I64_MIN, I64_MAX, U64_MAX = -(2 ** 63), 2 ** 63 - 1, 2 ** 64 - 1


def weights_for(n_ids):
    """The `weights` argument of PfacTable.state_weights for ids 1..n_ids (entry 0 unused)."""
    return [0] + [CYCLE[(i - 1) % len(CYCLE)] for i in range(1, n_ids + 1)]


def w_by_id(weights):
    return np.array([0] + [int(w) for w in list(weights)[1:]], dtype=np.int64)


def make(score, count):
    out = np.zeros(len(score), dtype=SCORE)
    out["score"], out["count"] = score, count
    return out


def scores_of(n_docs, doc, w):
    """Per document the sum of `w` (int64, wrapping) and the number of entries of `doc` that name it."""
    doc = np.asarray(doc, dtype=np.int64)
    score = np.zeros(n_docs, dtype=np.int64)
    with np.errstate(over="ignore"):
        np.add.at(score, doc, np.asarray(w, dtype=np.int64))
    return make(score, np.bincount(doc, minlength=n_docs).astype(np.uint64))


def scores_cut(pos, ids, lens, off, by_id):
    """THE reference: the whole-buffer records cut by the header's rule."""
    o = np.asarray(off, dtype=np.int64)
    d = np.minimum(np.searchsorted(o, pos, side="right") - 1, o.size - 2)
    keep = pos + lens <= o[d + 1]
    return scores_of(o.size - 1, d[keep], by_id[ids[keep]])


def scores_by_find(buf, off, lines, by_id):
    """Independent of any matcher: every occurrence (overlapping ones too) of pattern `lines[i - 1]` in the document's
    own bytes brings by_id[i] and one count."""
    data = bytes(np.asarray(buf, dtype=np.uint8))
    score, count = [0] * (off.size - 1), [0] * (off.size - 1)
    for d in range(off.size - 1):
        doc = data[int(off[d]):int(off[d + 1])]
        for i, line in enumerate(lines, 1):
            at = doc.find(line)
            while at >= 0:
                score[d] += int(by_id[i])
                count[d] += 1
                at = doc.find(line, at + 1)
    return make(np.array(score, dtype=np.int64), np.array(count, dtype=np.uint64))


def scores_of_selection(first, states, w_by_state):
    """The scores of a record array that is cut per document: document d owns [first[d], first[d + 1])."""
    f = np.asarray(first, dtype=np.int64)
    doc = np.repeat(np.arange(f.size - 1, dtype=np.int64), np.diff(f))
    return scores_of(f.size - 1, doc, np.asarray(w_by_state, dtype=np.int64)[np.asarray(states, dtype=np.int64)])


def totals(sc):
    """(score, count) over all documents, the score wrapped to int64 as the device's sum wraps."""
    s = sum(int(x) for x in sc["score"])
    return (s + 2 ** 63) % 2 ** 64 - 2 ** 63, int(sc["count"].sum())


def predicate(sc, off=None, min_score=None, max_score=None, min_count=None, max_count=None, density=None, invert=False):
    """The ids pfac_documents_matching_scores reports for scores `sc`, ascending (uint64).  The windows with numpy; the
    density through Python integers in object arrays, which no product overflows."""
    s, c = sc["score"], sc["count"]
    ok = np.ones(s.size, dtype=bool)
    if min_score is not None:
        ok &= s >= np.int64(min_score)
    if max_score is not None:
        ok &= s <= np.int64(max_score)
    if min_count is not None:
        ok &= c >= np.uint64(min_count)
    if max_count is not None:
        ok &= c <= np.uint64(max_count)
    if density is not None:
        num, den = int(density[0]), int(density[1])
        length = np.diff(np.asarray(off, dtype=np.uint64)).astype(object)
        ok &= (s.astype(object) * den >= num * length).astype(bool)
    return np.flatnonzero(ok != bool(invert)).astype(np.uint64)


def predicate_loop(sc, off=None, min_score=None, max_score=None, min_count=None, max_count=None, density=None, invert=False):
    """`predicate` with Python integers, one document at a time, in the header's words."""
    lo_s, hi_s = I64_MIN if min_score is None else min_score, I64_MAX if max_score is None else max_score
    lo_c, hi_c = 0 if min_count is None else min_count, U64_MAX if max_count is None else max_count
    out = []
    for d in range(sc.size):
        s, c = int(sc["score"][d]), int(sc["count"][d])
        ok = lo_c <= c <= hi_c and lo_s <= s <= hi_s
        if density is not None:
            ok = ok and s * int(density[1]) >= int(density[0]) * (int(off[d + 1]) - int(off[d]))
        if ok != bool(invert):
            out.append(d)
    return np.array(out, dtype=np.uint64)


# ---------------------------------------------------------------------------
# the cases: groupref's scans and offsets, weighted

def by_id_of(W):
    return w_by_id(weights_for(cases().x.tinfo(W)["ll"].size - 1))


_WANT = {}


def want(W, tiles, shape):
    """scores_cut of groupref's scan (W, tiles) under its offsets `shape`, computed once."""
    c = cases()
    key = (c.x.tinfo(W)["path"], tiles, shape)
    if key not in _WANT:
        pos, ids, lens = c.scan(W, tiles)
        _WANT[key] = scores_cut(pos, ids, lens, c.offsets(W, tiles, shape), by_id_of(W))
    return _WANT[key]


def check_preconditions(W, tiles):
    """What the GPU tests rely on, over the shapes of one scan: some document has kept records whose weights cancel,
    some document keeps weight-0 records only, from 65 tiles on some document straddles a 64-tile boundary with kept
    records on both sides, and at 130 tiles the single document of shape "one" is fed by three waves."""
    c = cases()
    pos, ids, lens = c.scan(W, tiles)
    by_id = by_id_of(W)
    cancels = zero_only = straddles = False
    for shape in SHAPES:
        off = c.offsets(W, tiles, shape).astype(np.int64)
        n_docs = off.size - 1
        sc = want(W, tiles, shape)
        d = np.minimum(np.searchsorted(off, pos, side="right") - 1, n_docs - 1)
        keep = pos + lens <= off[d + 1]
        nonzero = np.bincount(d[keep & (by_id[ids] != 0)], minlength=n_docs)
        cancels |= bool(((sc["count"] > 0) & (sc["score"] == 0) & (nonzero > 0)).any())
        zero_only |= bool(((sc["count"] > 0) & (nonzero == 0)).any())
        for edge in range(RANGE, int(off[-1]), RANGE):
            k = int(np.searchsorted(off, edge, side="right")) - 1
            if off[k] < edge < off[k + 1]:
                mine = keep & (d == k)
                straddles |= bool((mine & (pos < edge)).any() and (mine & (pos >= edge)).any())
        if shape == "one" and tiles == 130:
            fed = np.unique(pos[keep] // RANGE)
            assert n_docs == 1 and fed.tolist() == [0, 1, 2], "the single document is not fed by three waves"
    assert cancels, "no document whose kept weights cancel"
    assert zero_only, "no document that keeps weight-0 records only"
    assert tiles < 65 or straddles, "no document with kept records on both sides of a 64-tile boundary"
