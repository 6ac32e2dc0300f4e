"""The whole-word reference (tests/wordref.py) over the CPU oracle's records: it is the checker of
tests/test_gpu_whole_words.py, so it is pinned here without a GPU -- against Python's `re`, against its own plain-loop
form, and against the algebra the header promises (idempotent, left then right = both, chained ranges concatenate,
documents = every document on its own)."""
import re

import numpy as np
import pytest

import wordref
from docref import random_offsets
from llref import line_lengths
from orc import Oracle
from phfpfac_amd.matcher import tiled_bytes, word_set

N = 65536 + 123
WORD = rb"[0-9A-Za-z_]"
# (pattern file, matches, kept) of the 64 KiB + 123 bytes of paragraph402 tiled: counted with a pure-Python matcher
TABLE = [("experimentpattern", 4900, 164), ("xaa", 6859, 1796), ("xaa+xab+xac+xad", 27596, 6532)]


@pytest.fixture(scope="module")
def text(data_dir):
    return tiled_bytes(N, open(f"{data_dir}/paragraph402", "rb").read())


@pytest.fixture(scope="module")
def scans(text, resolve):
    """name -> (pos, lens, ids, pattern lines) of the oracle's scan of `text`."""
    out = {}
    for name, _, _ in TABLE:
        path = resolve(name)
        o = Oracle(path, 1, 1)
        pos, ids = o.scan_spec(text)
        o.close()
        lines = open(path, "rb").read().split(b"\n")[:-1]
        out[name] = (pos, line_lengths(path)[ids], ids, lines)
    return out


@pytest.mark.parametrize("name,matches,kept", TABLE)
def test_fixture_counts_and_vacuity(scans, text, name, matches, kept):
    pos, lens, _, _ = scans[name]
    keep = wordref.filter_words(text, pos, lens)
    assert pos.size == matches
    assert int(keep.sum()) == kept
    assert 0 < keep.sum() < pos.size / 2


def test_equals_re_for_word_only_patterns(scans, text):
    pos, lens, ids, lines = scans["xaa"]
    keep = wordref.filter_words(text, pos, lens)
    word_only = np.array([False] + [re.fullmatch(WORD + b"+", p) is not None for p in lines])
    assert word_only.sum() > 1000
    got = set(zip(pos[keep & word_only[ids]].tolist(), lens[keep & word_only[ids]].tolist()))
    raw = bytes(text)
    want = set()
    for p in set(p for p in lines if re.fullmatch(WORD + b"+", p)):
        for m in re.finditer(b"(?<!" + WORD + b")" + re.escape(p) + b"(?!" + WORD + b")", raw):
            want.add((m.start(), len(p)))
    assert got == want and len(want) > 500


@pytest.mark.parametrize("name", [t[0] for t in TABLE])
def test_loop_form_agrees(scans, text, name):
    pos, lens, _, _ = scans[name]
    rng = np.random.default_rng(5)
    off = random_offsets(rng, N, 40, empties=3)
    for edges in (wordref.LEFT, wordref.RIGHT, wordref.BOTH):
        for ws, prev, nxt, o in ((None, -1, -1, None), (None, ord("a"), ord("z"), None), (word_set(b"aeiou "), 32, -1, None),
                                 (None, -1, -1, off)):
            a = wordref.filter_words(text, pos, lens, ws, edges, prev, nxt, o)
            b = wordref.filter_words_loop(text, pos, lens, ws, edges, prev, nxt, o)
            assert np.array_equal(a, b)


def test_idempotent_and_left_then_right_is_both(scans, text):
    pos, lens, _, _ = scans["xaa+xab+xac+xad"]
    both = wordref.filter_words(text, pos, lens)
    again = wordref.filter_words(text, pos[both], lens[both])
    assert again.all()
    left = wordref.filter_words(text, pos, lens, edges=wordref.LEFT)
    right = wordref.filter_words(text, pos[left], lens[left], edges=wordref.RIGHT)
    assert np.array_equal(np.flatnonzero(left)[right], np.flatnonzero(both))
    assert left.sum() > both.sum() and wordref.filter_words(text, pos, lens, edges=wordref.RIGHT).sum() > both.sum()


def test_chained_ranges_concatenate(scans, text):
    pos, lens, _, _ = scans["xaa"]
    whole = wordref.filter_words(text, pos, lens)
    halo = int(lens.max()) - 1
    cuts = [0, 20011, 20012, 47000, N]                       # (one range of a single byte)
    got = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        avail = min(b + halo, N)
        mine = (pos >= a) & (pos < b)
        assert (pos[mine] + lens[mine] <= avail).all()
        k = wordref.filter_words(text[a:avail], pos[mine] - a, lens[mine], prev=int(text[a - 1]) if a else -1,
                                 next=int(text[avail]) if avail < N else -1)
        got.append(np.flatnonzero(mine)[k])
    assert np.array_equal(np.concatenate(got), np.flatnonzero(whole))
    # ... and without the neighbours' bytes it would not: the cut at 20011 lies inside a word
    k = wordref.filter_words(text[20011:20012 + halo], pos[pos == 20011] - 20011, lens[pos == 20011])
    assert wordref.word_table()[int(text[20010]) + 1] and wordref.word_table()[int(text[20011]) + 1]
    assert k.sum() >= whole[pos == 20011].sum()


def test_documents_equal_every_document_alone(scans, text):
    pos, lens, _, _ = scans["xaa+xab+xac+xad"]
    rng = np.random.default_rng(11)
    off = random_offsets(rng, N, 300, empties=5).astype(np.int64)
    keep = wordref.filter_words(text, pos, lens, off=off)
    want = np.zeros(pos.size, dtype=bool)
    mid_word = 0
    for a, b in zip(off[:-1], off[1:]):
        mine = np.flatnonzero((pos >= a) & (pos + lens <= b))
        want[mine] = wordref.filter_words(text[a:b], pos[mine] - a, lens[mine])
        mid_word += int(0 < a < N and wordref.cuts(text)[a])
    inside = np.zeros(pos.size, dtype=bool)                  # records that end inside their document
    d = np.searchsorted(off, pos, side="right") - 1
    inside = pos + lens <= off[np.minimum(d + 1, off.size - 1)]
    assert mid_word > 50                                     # the cuts do fall inside words
    assert np.array_equal(keep[inside], want[inside])
    assert keep[inside].sum() > wordref.filter_words(text, pos, lens)[inside].sum()


def test_seeded_cases_are_not_vacuous(tmp_path):
    """The cases of tests/wordfuzz.py (the GPU suite runs them): as a set they keep and drop records on both edges,
    with and without documents, in every record width."""
    import wordfuzz
    from phfpfac_amd import PfacTable
    dropped = {wordref.LEFT: 0, wordref.RIGHT: 0, wordref.BOTH: 0}
    kept = with_docs = 0
    finals = set()
    for seed in wordfuzz.SEEDS:
        c = wordfuzz.WordCase(seed)
        path = c.write_patterns(str(tmp_path / f"{seed}.pat"))
        finals.add(2 if PfacTable.from_file(path, c.width).num_final <= 16 else 4)
        o = Oracle(path, 1, 1)
        pos, ids = o.scan_spec(c.data)
        o.close()
        own = pos < c.n_owned
        pos, lens = pos[own], line_lengths(path)[ids[own]]
        keep = wordref.filter_words(c.data, pos, lens, c.ws, c.edges, c.prev, c.next, c.off)
        dropped[c.edges] += int((~keep).sum())
        kept += int(keep.sum())
        if c.off is not None:
            with_docs += int(keep.sum() - wordref.filter_words(c.data, pos, lens, c.ws, c.edges, c.prev, c.next).sum())
    assert min(dropped.values()) > 1000 and kept > 10000 and with_docs > 100
    assert finals == {2, 4}
