"""The Unigram reference against itself (no GPU): tests/uniref.py holds THE RULE of include/pfac.h twice -- a forward
DP over the records in heap order, and a per-word memoised search over the vocabulary's strings that never sees a
record -- and the two must agree on every named case and on 2 400 seeded random ones.  Also: what the cases reach, the
cases' preconditions, that `check` refuses wrong results, unigram_table, and the `tokenizers` library where it is
installed."""
import numpy as np
import pytest

import uniref
from uniref import DROP, TILE, Vocab, by_records, by_words, case, check, names, random_case, want_of


def same(a, b, what):
    for x, y, part in zip(a, b, ("ids", "positions", "tok_off")):
        if x is None or y is None:
            assert x is None and y is None, f"{what}: {part}"
        else:
            assert np.array_equal(np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)), f"{what}: the two forms differ in the {part}"


@pytest.mark.parametrize("name", names())
def test_the_two_forms_agree_on_a_named_case(name):
    same(want_of(name, "records"), want_of(name, "words"), name)


def test_preconditions_of_the_named_cases():
    assert [k for k, _ in uniref.vocab().skipped] == uniref.SKIPPED
    for name in names():
        data, no, v, off = case(name)
        assert data.dtype == np.uint8 and 0 <= no <= data.size, name
        assert v.bound_ok() and 1 <= v.max_word <= 4095, name
        assert v.longest < 1024 and all(t >= DROP for t in v.byte_ids.tolist()), name
        assert (v.unk >= 0) or v.unk == DROP, name
        if off is not None:
            o = off.astype(np.int64)
            assert o[0] == 0 and o[-1] == no and (np.diff(o) >= 0).all(), name
            assert uniref.boundaries_ok(data, no, off, v), f"{name}: an offset inside a word"
    # what the names promise
    d, no, v, _ = case("edge-piece-across")
    w = want_of("edge-piece-across")
    assert w[1].tolist() == [TILE - 2, TILE + 2] and w[0].tolist() == [v.first[b"play"][0], v.cont[b"ing"][0]]
    assert want_of("edge-lookback-bc")[0].tolist() == [v.first[b"a"][0], v.cont[b"bc"][0]]
    assert want_of("greedy-vs-viterbi")[0].tolist()[:2] == [3, 4]
    assert want_of("tie-longer-edge")[0].tolist()[0] == v.first[b"te"][0]
    assert want_of("tie-piece-or-byte")[0].tolist()[0] == v.first[b"q"][0]
    assert want_of("role-drop")[0].tolist() == [v.unk] * 6
    w = want_of("three-tiles")
    assert w[0].tolist() == [v.unk] and w[1].tolist() == [TILE - 100]
    assert want_of("cap4095")[0].size > 1000 and want_of("cap4095-over")[0].tolist() == [v.unk]
    assert want_of("one-byte-words")[0].size == 4096
    for name in ("end-piece-in-halo", "end-on-tile"):
        data, no, v, _ = case(name)
        pos, lens, _ = uniref.records(data, no, v)
        assert ((pos < no) & (pos + lens > no)).any(), f"{name}: no record ends in the halo"
    assert int(want_of("end-piece-in-halo")[0][-1]) == v.first[b"pl"][0]
    assert (want_of("folded")[0] >= 300 + 65).any() and (want_of("folded")[0] <= 300 + 90).any()


def test_the_two_forms_agree_on_random_cases_and_reach_the_rule():
    n_diff = n_tie = n_unk = n_fb = n_over = 0
    for seed in range(2400):
        data, no, v = random_case(seed)
        off = None
        if seed % 3 == 0:
            cuts = sorted(uniref.wpref.to_boundary(data, no, int(c), v) for c in np.random.default_rng(seed).integers(0, no + 1, size=3))
            off = np.array([0] + cuts + [no], dtype=np.uint64)
        st = {}
        a = uniref.want(data, no, v, off)
        b = by_words(data, no, v, off, st)
        same(a, b, f"random case {seed}: {bytes(data)!r} under {v.entries}, cap {v.max_word}")
        g = uniref.greedy_words(data, no, v)
        n_diff += not (np.array_equal(g[0], a[0]) and np.array_equal(g[1], a[1]))
        n_tie += any(p > 1 for p in st["paths"])
        n_unk += st["unk_runs"] > 0
        n_fb += st["fallback"] > 0
        n_over += st["over"] > 0
    assert min(n_diff, n_tie, n_unk, n_fb, n_over) > 200, (n_diff, n_tie, n_unk, n_fb, n_over)


def refused(wanted, ids, pos, tok_off=None):
    with pytest.raises(AssertionError):
        check(wanted, ids, pos, tok_off, what="seeded")


def test_check_refuses_seeded_wrong_results():
    v = uniref.vocab()
    data, no, _, _ = case("t3")
    w = want_of("t3")
    text = bytes(data[:no])
    check(w, w[0], w[1])
    # the greedy cut of "abc"
    p = text.index(b" abc ") + 1
    j = int(np.searchsorted(w[1], p))
    assert w[0][j:j + 2].tolist() == [v.first[b"a"][0], v.cont[b"bc"][0]]
    wrong, moved = w[0].copy(), w[1].copy()
    wrong[j:j + 2] = [v.first[b"ab"][0], v.cont[b"c"][0]]
    moved[j + 1] = p + 2
    refused(w, wrong, moved)
    # one unk per byte edge, not per run
    p = text.index(b" xxplay ") + 1
    j = int(np.searchsorted(w[1], p))
    assert int(w[0][j]) == v.unk and int(w[1][j + 1]) == p + 2
    refused(w, np.insert(w[0], j + 1, v.unk), np.insert(w[1], j + 1, p + 1))
    # the FIRST id where CONT is due
    p = text.index(b" unplaying ") + 3
    j = int(np.searchsorted(w[1], p))
    assert int(w[0][j]) == v.cont[b"play"][0]
    wrong = w[0].copy()
    wrong[j] = v.first[b"play"][0]
    refused(w, wrong, w[1])
    # a straddling word solved per tile: the right tile alone starts a word at the edge
    data, no, _, _ = case("edge-lookback-un")
    w = want_of("edge-lookback-un")
    left, right = by_words(data[:TILE], TILE, v), by_words(data[TILE:], no - TILE, v)
    per_tile = (np.concatenate([left[0], right[0]]), np.concatenate([left[1], right[1] + TILE]))
    assert not np.array_equal(per_tile[0], w[0])
    refused(w, *per_tile)
    # tok_off short by a tile's count
    w = want_of("docs-big")
    check(w, w[0], w[1], w[2])
    in_tile1 = int(((w[1] >= TILE) & (w[1] < 2 * TILE)).sum())
    short = w[2].copy()
    short[1:] -= in_tile1
    assert in_tile1 > 0
    refused(w, w[0], w[1], short)


# ---------------------------------------------------------------------------
# unigram_table

def test_unigram_table_on_a_written_vocabulary():
    from phfpfac_amd import UNIGRAM_PIECE_DTYPE, unigram_table
    from phfpfac_amd.table import unigram_scale_fits
    ents = [(e, float(s)) for e, s in uniref.ENTRIES]
    table, pieces, scale, skipped = unigram_table(ents, word_bytes=uniref.CASE_WORD, scale=1.0)
    v = uniref.vocab()
    assert scale == 1.0 and [k for k, _ in skipped] == uniref.SKIPPED and skipped == v.skipped
    nf = int(table.num_final)
    assert pieces.dtype == UNIGRAM_PIECE_DTYPE and pieces.shape == (nf,) and pieces.itemsize == 16
    lens = table.final_lengths()
    lines = []
    for e, _ in uniref.ENTRIES:                                 # the distinct stripped strings, in order
        p = e[len(uniref.PREFIX):] if e.startswith(uniref.PREFIX) else e
        if p in v.pieces and p not in lines:
            lines.append(p)
    got = {lines[int(i) - 1]: tuple(int(x) for x in pieces[s]) for s, i in enumerate(np.asarray(table.idmap)[:nf]) if lens[s] >= 1}
    assert got == {p: v.quad(p) for p in v.pieces}
    assert got[b"play"] == (5, 6, -3, -4) and got[b"ing"] == (DROP, 7, 0, -2) and got[b"un"] == (10, DROP, -2, 0)
    # the scale: the largest power of two <= 2^16 that keeps |score| * (max_word_bytes + 1) < 2^31
    _, p2, s2, _ = unigram_table(ents, word_bytes=uniref.CASE_WORD)
    assert s2 == 2.0**16 and int(p2["first_score"].min()) == -10 * 65536
    _, p3, s3, _ = unigram_table(ents, word_bytes=uniref.CASE_WORD, max_word_bytes=4095)
    assert s3 == 2.0**15 and unigram_scale_fits(10 * s3, 4095) and not unigram_scale_fits(10 * 2 * s3, 4095)
    assert int(np.abs(p3["cont_score"]).max()) * 4096 < 2**31
    with pytest.raises(ValueError):                             # the bound the runtime answers PFAC_E_ARG for
        unigram_table(ents, word_bytes=uniref.CASE_WORD, max_word_bytes=4095, scale=2.0**16)
    with pytest.raises(ValueError):
        unigram_table([("<unk>", 0.0), ("▁", -1.0)])
    # the default word set: everything but whitespace; str entries; folded
    t4, p4, _, s4 = unigram_table([("▁a.b", -1.0), ("a b", -1.0), ("▁A.B", -2.0), ("<s>", 0.0)], ignore_case=True)
    assert t4.ignore_case and [k for k, _ in s4] == [1, 2, 3] and int(p4["first_id"].max()) == 0


# ---------------------------------------------------------------------------
# the library

def test_against_the_tokenizers_library():
    """Per word on "▁" + word, no pre-tokenizer.  Scores are multiples of 2^-16 in [-2, -1), words of at most 6
    characters, every character has a `▁c` and a `c` piece: the library's unknown edge (min score - 10) cannot lie on
    an optimal path.  The segmentation is compared where the memoised search counts exactly one optimal path."""
    tokenizers = pytest.importorskip("tokenizers")
    from tokenizers.models import Unigram
    rng = np.random.default_rng(78)
    letters = "abc"
    n_words = n_skipped = 0
    for k in range(250):
        ents = [("<unk>", 0)]
        for c in letters:
            ents += [("▁" + c, -int(rng.integers(65537, 131073))), (c, -int(rng.integers(65537, 131073)))]
        seen = {e for e, _ in ents}
        for _ in range(int(rng.integers(2, 10))):
            p = "".join(letters[int(i)] for i in rng.integers(0, 3, size=int(rng.integers(2, 5))))
            e = ("▁" if rng.integers(2) else "") + p
            if e not in seen:
                seen.add(e)
                ents.append((e, -int(rng.integers(65537, 131073))))
        v = Vocab([(e.encode(), s) for e, s in ents], unk=0, max_word=100, word=b"abc", byte_score=-(10 << 16))
        model = Unigram([(e, s / 65536.0) for e, s in ents], unk_id=0, byte_fallback=False)
        for _ in range(8):
            word = "".join(letters[int(i)] for i in rng.integers(0, 3, size=int(rng.integers(1, 7))))
            data = np.frombuffer(word.encode(), dtype=np.uint8)
            st = {}
            ids, _, _ = by_words(data, data.size, v, None, st)
            lib = [t.id for t in model.tokenize("▁" + word)]
            assert 0 not in lib, f"vocabulary {k}: the library put its unknown edge on the path of {word!r}"
            n_words += 1
            if st["paths"] != [1]:
                n_skipped += 1
                continue
            assert ids.tolist() == lib, f"vocabulary {k}: {word!r} under {ents}: {ids.tolist()}, the library says {lib}"
    assert n_words == 2000 and n_skipped <= n_words // 20, (n_words, n_skipped)
