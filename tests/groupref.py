"""Host reference for pattern groups (the checker, never the product): a group mask per document and the predicate
over the masks, the case list of tests/test_gpu_groups.py with the preconditions that make each case test what it is
named for, and nothing from the device.

The reference (`masks_per_doc`): mask[d] = OR of the groups of the patterns among the records that
docref.oracle_per_doc keeps -- every document scanned on its own by the CPU oracle.  Two more forms are held against it
in tests/test_groups_ref.py: `masks_by_find` (bytes.find of every pattern in the document's own bytes) and `masks_cut`
(the whole-buffer records cut by the header's rule, vectorised: the form the GPU tests use on inputs of 130 tiles).
Groups are given per 1-based pattern id; `GROUPING` maps an id to group 0, group 63, one group in between, two groups,
or none."""
import numpy as np

from heapguard import TILE

RANGE = 64 * TILE                       # the bytes of one wave's 64 tiles
TILES = (3, 64, 65, 130)                # one wave range, its edge, two ranges, three
SHAPES = ("one", "tiny", "mid", "huge", "edges", "empties", "cut")
PLANT = b" that "                       # its "that" is put across a boundary of every kind (both tables hold it)
PLANT_EDGES = (1, 2, 63, 64, 65, 128, 129)    # tile edges that get one
ALL = (1 << 64) - 1


def grouping(pid):
    """The groups of pattern id `pid` in every test: None (in no group), 0, 63, 7, or (1, 2)."""
    return (None, 0, 63, 7, (1, 2))[pid % 5]


def groups_for(n_ids):
    """The `groups` argument of PfacTable.state_group_masks for ids 1..n_ids (entry 0 unused)."""
    return [None] + [grouping(i) for i in range(1, n_ids + 1)]


def masks_by_id(groups):
    """uint64[len(groups)]: the mask of every pattern id, from the same argument -- written apart from the product's."""
    out = []
    for e in groups:
        gs = [] if e is None else [e] if isinstance(e, (int, np.integer)) else list(e)
        out.append(sum({1 << int(g) for g in gs}))
    return np.array(out, dtype=np.uint64)


def _or_by_doc(n_docs, doc, m):
    out = np.zeros(n_docs, dtype=np.uint64)
    np.bitwise_or.at(out, np.asarray(doc, dtype=np.int64), np.asarray(m, dtype=np.uint64))
    return out


def masks_per_doc(o, buf, off, by_id):
    """THE reference: the records docref.oracle_per_doc keeps, their patterns' masks OR-ed per document."""
    from docref import oracle_per_doc
    first, _, ids = oracle_per_doc(o, buf, off)
    doc = np.repeat(np.arange(off.size - 1, dtype=np.int64), np.diff(first.astype(np.int64)))
    return _or_by_doc(off.size - 1, doc, by_id[np.asarray(ids, dtype=np.int64)])


def masks_by_find(buf, off, lines, by_id):
    """Independent of any matcher: pattern `lines[i - 1]` is in document d iff bytes.find sees it in the document's own
    bytes."""
    data = bytes(np.asarray(buf, dtype=np.uint8))
    out = np.zeros(off.size - 1, dtype=np.uint64)
    for d in range(off.size - 1):
        doc = data[int(off[d]):int(off[d + 1])]
        for i, line in enumerate(lines, 1):
            if by_id[i] and doc.find(line) >= 0:
                out[d] |= by_id[i]
    return out


def masks_cut(pos, ids, lens, off, by_id):
    """The whole-buffer records (pos, pattern id, length) cut by the rule of include/pfac.h: record -> the last document
    with off[d] <= pos, kept iff pos + len <= off[d + 1]."""
    o = np.asarray(off, dtype=np.int64)
    d = np.minimum(np.searchsorted(o, pos, side="right") - 1, o.size - 2)
    keep = pos + lens <= o[d + 1]
    return _or_by_doc(o.size - 1, d[keep], by_id[ids[keep]])


def predicate(m, all_of=0, any_of=0, none_of=0, invert=False):
    """The ids pfac_documents_matching_groups reports for masks `m`, ascending (uint64)."""
    m = np.asarray(m, dtype=np.uint64)
    a, y, n = np.uint64(all_of & ALL), np.uint64(any_of & ALL), np.uint64(none_of & ALL)
    ok = ((m & a) == a) & ((m & n) == 0)
    if any_of & ALL:
        ok &= (m & y) != 0
    return np.flatnonzero(ok != bool(invert)).astype(np.uint64)


def predicate_loop(m, all_of=0, any_of=0, none_of=0, invert=False):
    """`predicate` with Python integers, one document at a time."""
    out = []
    for d, v in enumerate(int(x) for x in m):
        ok = (v & all_of) == all_of and (any_of == 0 or (v & any_of) != 0) and (v & none_of) == 0
        if ok != bool(invert):
            out.append(d)
    return np.array(out, dtype=np.uint64)


# ---------------------------------------------------------------------------
# the cases

def planted_text():
    """passguard's text with PLANT's "that" across the tile edges PLANT_EDGES: two bytes on either side."""
    from passguard import cpu
    t = cpu().input("text").copy()
    p = np.frombuffer(PLANT, dtype=np.uint8)
    for e in PLANT_EDGES:
        t[e * TILE - 3:e * TILE - 3 + p.size] = p
    return t


class Cases:
    """The inputs, scans and offsets of the group tests, each computed once.  A scan is (W, tiles): passguard's table of
    record width W over the first `n_owned(tiles)` bytes of the planted text, no halo; n_owned is chosen so that the
    input ends with the last byte of a match."""

    def __init__(self):
        from passguard import cpu
        self.x = cpu()
        self.text = planted_text()
        self._c = {}

    def _memo(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    def n_owned(self, tiles):
        at = bytes(self.text).find(b" the ", (tiles - 1) * TILE + 100)
        assert (tiles - 1) * TILE < at + 4 <= tiles * TILE
        return at + 4                                           # "the" ends at the input's last byte

    def by_id(self, W):
        return masks_by_id(groups_for(self.x.tinfo(W)["ll"].size - 1))

    def scan(self, W, tiles):
        def make():
            info = self.x.tinfo(W)
            no = self.n_owned(tiles)
            pos, ids = info["matcher"].scan_spec(np.ascontiguousarray(self.text[:no]), None)
            pos, ids = pos.astype(np.int64), ids.astype(np.int64)
            return pos, ids, info["ll"][ids]
        return self._memo(("scan", self.x.tinfo(W)["path"], tiles), make)

    def offsets(self, W, tiles, shape):
        no = self.n_owned(tiles)

        def spaced(rng, lo, hi):
            c = np.cumsum(rng.integers(lo, hi + 1, no // lo + 1))
            return c[c < no]

        def make():
            rng = np.random.default_rng([0x47524F, tiles, SHAPES.index(shape)])
            tile_edges = np.arange(TILE, no, TILE, dtype=np.int64)
            if shape == "one":
                cuts = np.empty(0, dtype=np.int64)
            elif shape == "tiny":
                cuts = spaced(rng, 1, 40)
            elif shape == "mid":
                cuts = spaced(rng, 64, 4000)
            elif shape == "huge":
                cuts = spaced(rng, 290 << 10, 310 << 10)
            elif shape == "edges":                              # every tile edge (the 64-tile edges among them), and between
                cuts = np.concatenate([tile_edges, spaced(rng, 64, 4000)])
            elif shape == "empties":                            # runs of empty documents: front, a range edge, the end
                at = [0, min(RANGE, (tiles - 1) * TILE), no]
                cuts = np.concatenate([spaced(rng, 64, 4000)] + [np.full(70, a, dtype=np.int64) for a in at])
            else:                                               # "cut": document ends inside matches, mid-tile and at tile edges
                pos, _, lens = self.scan(W, tiles)
                inside = pos[lens >= 2][::5] + 1
                inside = inside[(inside > 0) & (inside < no) & (inside % TILE >= 8) & (inside % TILE < TILE - 8)]
                cuts = np.concatenate([inside, tile_edges])         # (none so near a tile edge that it would shield it)
            return np.unique(np.concatenate([[0], cuts, [no]])).astype(np.uint64) if shape != "empties" else \
                np.sort(np.concatenate([[0], cuts, [no]])).astype(np.uint64)
        return self._memo(("off", tiles, shape) + ((self.x.tinfo(W)["path"],) if shape == "cut" else ()), make)

    def want(self, W, tiles, shape):
        def make():
            pos, ids, lens = self.scan(W, tiles)
            return masks_cut(pos, ids, lens, self.offsets(W, tiles, shape), self.by_id(W))
        return self._memo(("want", self.x.tinfo(W)["path"], tiles, shape), make)

    # -- what makes a case the case it is named for ---------------------------------
    def check_preconditions(self, W, tiles, shape):
        no = self.n_owned(tiles)
        off = self.offsets(W, tiles, shape).astype(np.int64)
        pos, ids, lens = self.scan(W, tiles)
        by_id = self.by_id(W)
        n_docs = off.size - 1
        assert off[0] == 0 and off[-1] == no and (np.diff(off) >= 0).all()
        assert (no + TILE - 1) // TILE == tiles
        assert (pos + lens == no).any(), "no match ends at the input's last byte"
        starts = np.bincount(off[:-1] // TILE, minlength=tiles)          # document starts per tile
        # the documents that straddle an end of a wave's range: off[d] < k * RANGE < off[d + 1]
        edges = np.arange(RANGE, no, RANGE, dtype=np.int64)
        d_at = np.searchsorted(off, edges, side="right") - 1
        straddlers = d_at[(off[d_at] < edges) & (off[np.minimum(d_at + 1, n_docs)] > edges)]
        d = np.minimum(np.searchsorted(off, pos, side="right") - 1, n_docs - 1)
        crossing = pos + lens > off[d + 1]
        if shape == "one":
            assert n_docs == 1 and (tiles <= 64 or straddlers.size == edges.size)
        if shape == "tiny":
            assert (np.diff(off) <= 40).all() and starts[:-1].min() >= 63, "a tile with fewer than 63 document starts"
            want = self.want(W, tiles, shape)
            ungrouped = np.zeros(n_docs, dtype=bool)
            keep = ~crossing & (by_id[ids] == 0)
            ungrouped[d[keep]] = True
            assert (ungrouped & (want == 0)).any(), "no document holds an ungrouped match alone"
        if shape == "mid":
            assert starts.max() < 63 and (np.diff(off)[:-1] >= 64).all()
        if shape == "huge" and tiles > 64:
            assert straddlers.size == edges.size and (np.diff(off)[:-1] > RANGE).all()
        if shape == "edges":
            assert np.isin(np.arange(TILE, no, TILE), off).all() and straddlers.size == 0
        if shape == "empties":
            lens_d = np.diff(off)
            assert lens_d[:69].max() == 0 and lens_d[-69:].max() == 0 and (lens_d == 0).sum() >= 3 * 69
        if shape in ("cut", "edges", "tiny", "mid"):
            assert crossing.any(), "no record crosses a document end"
        if shape == "cut":
            at_tile_edge = crossing & (off[d + 1] % TILE == 0)
            assert at_tile_edge.any(), "no record crosses a document end at a tile edge"
            if tiles > 64:
                assert (crossing & (off[d + 1] % RANGE == 0)).any(), "no record crosses a document end at a 64-tile edge"
        return dict(n_docs=n_docs, starts_max=int(starts.max()), straddlers=int(straddlers.size), crossing=int(crossing.sum()))


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = Cases()
    return _CASES
