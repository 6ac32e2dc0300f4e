"""The WordPiece reference (tests/wpref.py) without a GPU: its two forms of the rule against each other -- the numpy form
over the bitmaps of the composition's picks and the textbook per-word loop that never sees a record -- on every named
case of tests/test_gpu_wordpiece.py and on 2 400 seeded random ones; both against tokenizers.models.WordPiece where that
package is installed; the preconditions of every case; what the cases reach; seeded wrong results that `check` must
refuse; and phfpfac_amd.table.wordpiece_table against the reference's own reading of a vocabulary."""
import numpy as np
import pytest

import wpref
from wpref import DROP, TILE, Vocab, by_bitmaps, by_words, case, check, names, picks, want_of

# cases in which a pick reaches past n_owned: the rule on bitmaps alone defines them
HALO_CASES = ("end-in-halo", "end-pick-in-halo")


def same(a, b, what):
    for x, y, part in zip(a, b, ("ids", "positions", "tok_off")):
        assert (x is None) == (y is None), what
        if x is not None:
            assert np.array_equal(np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)), f"{what}: the {part} differ"


@pytest.mark.parametrize("name", names())
def test_both_forms_agree_on_the_named_cases(name):
    data, no, v, off = case(name)
    assert 0 <= no <= data.size and 1 <= v.max_word <= 4095 and v.unk >= 0
    assert all(all(v.word[b] for b in p) and 0 < len(p) < 1024 for p in v.pieces), "a piece with a non-word byte"
    if off is not None:
        o = off.astype(np.int64)
        assert o[0] == 0 and o[-1] == no and (np.diff(o) >= 0).all()
        assert wpref.boundaries_ok(data, no, off, v), "an offset inside a word"
    w = want_of(name)
    assert w[0].size == w[1].size and (np.diff(w[1].astype(np.int64)) > 0).all() and (w[0] >= 0).all()
    if name in HALO_CASES:
        assert v.word[data[no - 1]] and v.word[data[no]], "n_owned is meant to cut a word"
        return
    assert no == data.size or no == 0 or not (v.word[data[no - 1]] and v.word[data[no]]), "n_owned cuts a word"
    same(w, by_words(data, no, v, off), name)


def test_the_halo_cases_differ_from_the_cut_text():
    """A pick that ends in the halo covers its word's owned bytes: `play|ing` cut behind `pl` is the piece `play`, which
    the textbook form of the cut text cannot know."""
    data, no, v, _ = case("end-pick-in-halo")
    w = want_of("end-pick-in-halo")
    assert int(w[0][-1]) == v.first[b"play"] and int(w[1][-1]) == no - 2
    x = by_words(data, no, v)
    assert int(x[0][-1]) == v.first[b"pl"] and not np.array_equal(w[0], x[0])
    data, no, v, _ = case("end-in-halo")
    same(want_of("end-in-halo"), by_words(data, no, v), "a pick that ends at n_owned")


def test_what_the_cases_reach():
    v = wpref.vocab()
    assert v.first[b"play"] != v.cont[b"play"] and b"ing" not in v.first and b"un" not in v.cont
    assert v.byte_ids[ord(".")] >= 0 and v.byte_ids[ord(",")] == DROP and v.byte_ids[ord(" ")] == DROP
    data, no, _, _ = case("t3")
    text = bytes(data[:no])
    ids, pos, _ = want_of("t3")
    at = dict(zip(pos.tolist(), ids.tolist()))
    p = text.index(b" unplaying ") + 1                          # a good word of three pieces, x and ##x with different ids
    assert [at.get(p + k) for k in range(9)] == [v.first[b"un"], None, v.cont[b"play"], None, None, None, v.cont[b"ing"], None, None]
    p = text.index(b" play ") + 1
    assert at[p] == v.first[b"play"]
    p = text.index(b" playx ") + 1                              # a bad word: one [UNK], nothing of "play"
    assert [at.get(p + k) for k in range(5)] == [v.unk, None, None, None, None]
    p = text.index(b" ing ") + 1                                # ##-only at a word's start
    assert [at.get(p + k) for k in range(3)] == [v.unk, None, None]
    assert at[text.index(b".")] == v.byte_ids[ord(".")] and text.index(b",") not in at       # an emitted byte, a dropped one
    data, no, v20, _ = case("edge-len-over")                    # an over-long word whose every byte is covered
    pp, pl, _ = picks(data, no, v20)
    assert pp.size > 1 and int(pl.sum()) == 21
    assert want_of("edge-len-over")[0].tolist() == [v20.unk]
    assert v20.unk not in want_of("edge-len-max")[0].tolist()


def random_case(rng):
    alpha = b"abc" if rng.integers(2) else b"abcde"
    entries = [b"[UNK]"]
    for _ in range(int(rng.integers(1, 15))):
        s = bytes(alpha[int(k)] for k in rng.integers(len(alpha), size=int(rng.integers(1, 5))))
        entries.append((b"##" if rng.integers(2) else b"") + s)
    for b in b".,":
        if rng.integers(2):
            entries.append(bytes([b]))
    v = Vocab(entries, b"[UNK]", max_word=(3, 6, 100)[int(rng.integers(3))], word=b"abcde")
    chars = alpha + b" .,"
    n = int(rng.integers(0, 61))
    weights = np.array([3.0] * len(alpha) + [2.0, 0.5, 0.5])
    data = np.frombuffer(bytes(chars[int(k)] for k in rng.choice(len(chars), size=n, p=weights / weights.sum())), dtype=np.uint8)
    return data, v


def test_both_forms_agree_on_random_cases():
    rng = np.random.default_rng(20240611)
    seen_unk = seen_multi = 0
    for k in range(2400):
        data, v = random_case(rng)
        if not v.pieces:
            continue
        off = None
        if k % 3 == 0:                                          # every third as documents cut at word boundaries
            cuts = sorted(wpref.to_boundary(data, data.size, int(c), v) for c in rng.integers(0, data.size + 1, size=3))
            off = np.array([0] + cuts + [data.size], dtype=np.uint64)
        w = wpref.want(data, data.size, v, off)
        same(w, by_words(data, data.size, v, off), f"random case {k}: {bytes(data)!r} under {v.entries}")
        seen_unk += int((w[0] == v.unk).any())
        seen_multi += int(any(t in v.cont.values() for t in w[0].tolist()))
    assert seen_unk > 200 and seen_multi > 200


def test_against_the_tokenizers_library():
    tokenizers = pytest.importorskip("tokenizers")
    from tokenizers.models import WordPiece
    rng = np.random.default_rng(77)
    n_words = 0
    for k in range(1500):
        data, v = random_case(rng)
        if v.skipped != [(0, b"[UNK]")] or not v.pieces:        # (a dict holds no duplicate entry)
            continue
        vocab = {e.decode(): i for i, e in enumerate(v.entries)}
        model = WordPiece(vocab=vocab, unk_token="[UNK]", max_input_chars_per_word=v.max_word, continuing_subword_prefix="##")
        ids, pos, _ = wpref.want(data, data.size, v)
        got = dict(zip(pos.tolist(), ids.tolist()))
        text = bytes(data)
        i = 0
        while i < len(text):
            if not v.word[text[i]]:
                i += 1
                continue
            j = i
            while j < len(text) and v.word[text[j]]:
                j += 1
            want_ids = [t.id for t in model.tokenize(text[i:j].decode())]
            mine = [got[p] for p in range(i, j) if p in got]
            assert mine == want_ids, f"case {k}: {text[i:j]!r} under {v.entries}: {mine}, the library says {want_ids}"
            n_words += 1
            i = j
    assert n_words > 2000


# ---------------------------------------------------------------------------
# check refuses wrong results

def refused(wanted, ids, pos, tok_off=None):
    with pytest.raises(AssertionError):
        check(wanted, ids, pos, tok_off, what="seeded")


def test_check_refuses_seeded_wrong_results():
    v = wpref.vocab()
    # a bad word's pieces next to its [UNK]; [UNK] at the word's last byte
    data, no, _, _ = case("t3")
    w = want_of("t3")
    text = bytes(data[:no])
    check(w, w[0], w[1])
    p = text.index(b" playx ") + 1
    j = int(np.searchsorted(w[1], p))
    assert int(w[0][j]) == v.unk
    refused(w, np.insert(w[0], j + 1, v.first[b"play"]), np.insert(w[1], j + 1, p))
    moved = w[1].copy()
    moved[j] = p + 4
    refused(w, w[0], moved)
    # the FIRST id where CONT is due
    p = text.index(b" unplaying ") + 3
    j = int(np.searchsorted(w[1], p))
    assert int(w[0][j]) == v.cont[b"play"]
    wrong = w[0].copy()
    wrong[j] = v.first[b"play"]
    refused(w, wrong, w[1])
    # a straddling word judged per tile: the hole is left of the edge, the right tile alone sees a good "bab.."
    data, no, _, _ = case("edge-hole-left")
    w = want_of("edge-hole-left")
    right = by_words(data[TILE:], no - TILE, v)
    left = by_words(data[:TILE], TILE, v)
    per_tile = (np.concatenate([left[0], right[0]]), np.concatenate([left[1], right[1] + TILE]))
    assert per_tile[0].size > w[0].size
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
# wordpiece_table

VOCAB_LINES = [b"[UNK]", b"[CLS]", b"play", b"##play", b"##ing", b"Un", b".", b"##.", b"", b"play", b"##", b"a b", b"!", b"x" * 1024]


def test_wordpiece_table_on_a_written_vocabulary(tmp_path):
    from phfpfac_amd import wordpiece_table
    table, first, cont, byte_ids, skipped = wordpiece_table(VOCAB_LINES)
    v = Vocab(VOCAB_LINES[:-1], b"[UNK]")
    assert [k for k, _ in skipped] == [0, 1, 7, 8, 9, 10, 11, 13]
    assert skipped[:-1] == v.skipped and skipped[-1][1] == b"x" * 1024
    assert byte_ids.dtype == np.int32 and byte_ids.shape == (256,)
    assert np.array_equal(byte_ids, v.byte_ids) and byte_ids[ord(".")] == 6 and byte_ids[ord("!")] == 12
    lens = table.final_lengths()
    nf = int(table.num_final)
    assert first.shape == cont.shape == (nf,) and first.dtype == cont.dtype == np.int32
    lines = [b"play", b"ing", b"Un"]                            # the distinct stripped strings, in order
    by_piece = {lines[int(i) - 1]: (int(first[s]), int(cont[s])) for s, i in enumerate(np.asarray(table.idmap)[:nf]) if lens[s] >= 1}
    assert by_piece == {b"play": (2, 3), b"ing": (DROP, 4), b"Un": (5, DROP)}
    # the same from a file, one entry per line; and folded
    path = tmp_path / "vocab.txt"
    path.write_bytes(b"".join(e + b"\n" for e in VOCAB_LINES))
    t2, f2, c2, b2, s2 = wordpiece_table(str(path))
    assert np.array_equal(f2, first) and np.array_equal(c2, cont) and np.array_equal(b2, byte_ids) and s2 == skipped
    t3, f3, c3, _, _ = wordpiece_table(VOCAB_LINES, ignore_case=True)
    assert t3.ignore_case and sorted(f3[f3 >= 0].tolist()) == [2, 5]
    with pytest.raises(ValueError):
        wordpiece_table([b"[UNK]", b"."])
    # another prefix and another word set
    _, f4, c4, b4, s4 = wordpiece_table([b"ab", b"@@ab", b"-", b"a-b"], prefix=b"@@", word_bytes=b"ab-")
    assert sorted(f4[f4 >= 0].tolist()) == [0, 2, 3] and c4[c4 >= 0].tolist() == [1] and (b4 == DROP).all() and s4 == []
