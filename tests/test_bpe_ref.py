"""The BPE reference against itself (no GPU): tests/bperef.py holds THE RULE of include/pfac.h twice -- per word over a
list of parts and a dict of strings, which never sees a record, and over the records in heap order with a boundary
bitmap and cached ranks, as the kernel does it -- and the two must agree on every named case and on 2 400 seeded random
ones.  Also: what the cases reach, the cases' preconditions, that `check` refuses wrong results, bpe_table, and the
`tokenizers` library where it is installed."""
import numpy as np
import pytest

import bperef
from bperef import DROP, TILE, Vocab, by_strings, case, check, names, random_case, want_of


def same(a, b, what):
    for x, y, part in zip(a, b, ("ids", "positions", "tok_off")):
        if x is None or y is None:
            assert x is None and y is None, f"{what}: {part}"
        else:
            assert np.array_equal(np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)), f"{what}: the two forms differ in the {part}"


def differ(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


@pytest.mark.parametrize("name", names())
def test_the_two_forms_agree_on_a_named_case(name):
    same(want_of(name, "records"), want_of(name, "strings"), name)


def test_preconditions_of_the_named_cases():
    v = bperef.vocab()
    assert {k: why for k, _, why in v.skipped} == bperef.SKIPPED
    assert len(bperef.small_vocab().pieces) == bperef.N_SMALL and not bperef.small_vocab().skipped
    for name in names():
        data, no, v, off = case(name)
        assert data.dtype == np.uint8 and 0 <= no <= data.size, name
        assert 1 <= v.max_word <= 255 and -1 <= v.lead <= 255 and (v.lead < 0 or not v.word[v.lead]), name
        assert v.longest < 1024 and all(t >= DROP for t in v.byte_ids.tolist()), name
        assert all(i >= DROP and r >= 0 for i, r, _ in v.strings.values()), name
        if off is not None:
            o = off.astype(np.int64)
            assert o[0] == 0 and o[-1] == no and (np.diff(o) >= 0).all(), name
            assert bperef.boundaries_ok(data, no, off, v), f"{name}: an offset inside a word"
    # what the names promise
    v = bperef.vocab()
    sid = {s: i for s, (i, _, _) in v.strings.items()}
    byte = lambda c: 300 + ord(c)                                       # noqa: E731
    w = want_of("greedy-vs-bpe")
    assert w[0].tolist()[:2] == [byte("a"), sid[b"bc"]] and w[1].tolist()[:2] == [0, 1]
    assert differ(bperef.greedy(*case("greedy-vs-bpe")[:3]), w)
    assert want_of("split-any")[0].tolist()[0] == sid[b"abc"] and differ(want_of("split-any"), want_of("split-matters"))
    assert want_of("tie-leftmost")[0].tolist()[:4] == [sid[b"aaaa"], byte("."), sid[b"aa"], byte("a")]
    w = want_of("chain")
    assert w[0].tolist()[:3] == [sid[bperef.CHAIN], byte("."), sid[bperef.CHAIN[:9]]] and w[1].tolist()[:3] == [0, 16, 17]
    w = want_of("part-drop")                                            # "er" has no id: a part that emits nothing
    assert sid[b"er"] == DROP and w[0].tolist() == [sid[b"player"], byte("."), byte(" "), byte(" "), sid[b"unplay"]]
    assert w[1].tolist() == [0, 6, 9, 12, 13]
    w = want_of("edge-piece-across")
    j = int(np.searchsorted(w[1], TILE - 3))
    assert w[0][j:j + 2].tolist() == [sid[b" play"], sid[b"ing"]] and w[1][j:j + 2].tolist() == [TILE - 3, TILE + 2]
    w = want_of("edge-lookback-bc")
    j = int(np.searchsorted(w[1], TILE - 2))
    assert w[0][j:j + 2].tolist() == [sid[b" a"], sid[b"bc"]] and w[1][j:j + 2].tolist() == [TILE - 2, TILE]
    assert want_of("edge-chain")[0].tolist().count(sid[bperef.CHAIN]) == 1 and want_of("group-chain")[1].tolist().count(64 * TILE - 9) == 1
    w = want_of("lead-at-0")
    assert w[0].tolist()[:3] == [sid[b" ab"], byte(" "), sid[b" ab"]] and w[1].tolist()[:3] == [0, 3, 4]
    assert want_of("lead-none")[0].tolist()[:2] == [byte(" "), sid[b"ab"]]
    for name, p in (("lead-tile-last", b" play"), ("lead-tile-last-ab", b" ab")):
        w = want_of(name)
        j = int(np.searchsorted(w[1], TILE - 1))
        assert int(w[1][j]) == TILE - 1 and int(w[0][j]) == sid[p] and int(w[1][j + 1]) == TILE - 1 + len(p), name
    w = want_of("lead-two")
    j = int(np.searchsorted(w[1], TILE - 1))
    assert w[0][j:j + 2].tolist() == [byte(" "), sid[b" ab"]]
    w = want_of("lead-word-after-word")
    j = int(np.searchsorted(w[1], TILE - 2))
    assert w[0][j:j + 3].tolist() == [sid[b"ab"], sid[b" ab"], sid[b" ab"]]
    for mw in (1, 2, 63, 64, 65, 255):
        st = {}
        data, no, vv, _ = case(f"cap{mw}")
        by_strings(data, no, vv, None, st)
        assert st["over"] >= 2 and (mw == 1 or st["lead"] >= 1), mw
        assert (want_of(f"cap{mw}-over-edge")[0] >= 300).all(), "over the cap: single bytes"
        assert (want_of(f"cap{mw}-lead-over-edge")[0] >= 300).all()
    assert (want_of("cap255")[0] < 300).any() and (want_of("long-word")[0] >= 300).all()
    assert want_of("one-byte-words")[0].size == 2 * TILE - 2048 and want_of("alldrop-bytes")[0].max() < 300
    for name in ("end-piece-in-halo", "end-on-tile"):
        data, no, v, _ = case(name)
        pos, lens, _ = bperef.records(data, no, v)
        assert ((pos < no) & (pos + lens > no)).any(), f"{name}: no record ends in the halo"
    assert int(want_of("end-piece-in-halo")[0][-1]) == sid[b" pl"]
    assert (want_of("folded")[0] >= 300 + 65).any() and (want_of("folded")[0] < 300).any()


def test_the_two_forms_agree_on_random_cases_and_reach_the_rule():
    n_greedy = n_split = n_tie = n_lead = n_over = n_drop = 0
    for seed in range(2400):
        data, no, v = random_case(seed)
        off = None
        if seed % 3 == 0:
            cuts = sorted(bperef.to_boundary(data, no, int(c), v) for c in np.random.default_rng(seed).integers(0, no + 1, size=3))
            off = np.array([0] + cuts + [no], dtype=np.uint64)
            assert bperef.boundaries_ok(data, no, off, v)
        st = {}
        a = bperef.want(data, no, v, off)
        b = by_strings(data, no, v, off, st)
        same(a, b, f"random case {seed}: {bytes(data)!r} under {v.merges}, cap {v.max_word}, lead {v.lead}")
        n_greedy += differ(bperef.greedy(data, no, v), a)
        n_split += not v.any_split and differ(by_strings(data, no, v.with_any_split()), a)
        n_tie += st["ties"] > 0
        n_lead += st["lead"] > 0
        n_over += st["over"] > 0
        n_drop += st["dropped"] > 0
    assert min(n_greedy, n_split, n_tie, n_lead, n_over, n_drop) > 200, (n_greedy, n_split, n_tie, n_lead, n_over, n_drop)


def refused(wanted, ids, pos, tok_off=None):
    with pytest.raises(AssertionError):
        check(wanted, ids, pos, tok_off, what="seeded")


def test_check_refuses_seeded_wrong_results():
    v = bperef.vocab()
    sid = {s: i for s, (i, _, _) in v.strings.items()}
    data, no, _, _ = case("greedy-vs-bpe")
    w = want_of("greedy-vs-bpe")
    check(w, w[0], w[1])
    # the greedy cut of "abc": one token where BPE has two
    assert w[0][:2].tolist() == [300 + ord("a"), sid[b"bc"]]
    refused(w, np.concatenate([[sid[b"abc"]], w[0][2:]]).astype(np.int32), np.concatenate([[0], w[1][2:]]).astype(np.uint32))
    # the rightmost of equal ranks: "aaa" as a + aa
    w = want_of("tie-leftmost")
    j = int(np.searchsorted(w[1], 5))
    assert w[0][j:j + 2].tolist() == [sid[b"aa"], 300 + ord("a")]
    wrong, moved = w[0].copy(), w[1].copy()
    wrong[j:j + 2] = [300 + ord("a"), sid[b"aa"]]
    moved[j + 1] = 6
    refused(w, wrong, moved)
    # the lead left outside its word
    w = want_of("lead-at-0")
    refused(w, np.concatenate([[300 + 32, sid[b"ab"]], w[0][1:]]).astype(np.int32), np.concatenate([[0, 1], w[1][1:]]).astype(np.uint32))
    # a straddling word solved per tile: the right tile alone starts a word at the edge
    data, no, _, _ = case("edge-lookback-un")
    w = want_of("edge-lookback-un")
    left, right = by_strings(data[:TILE], TILE, v), by_strings(data[TILE:], no - TILE, v)
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
# bpe_table

def state_strings(table):
    """final state -> its pattern line (bytes), through the table's id map"""
    nf = int(table.num_final)
    return [int(i) - 1 for i in np.asarray(table.idmap)[:nf]]


def test_bpe_table_on_a_written_vocabulary():
    from phfpfac_amd import BPE_PIECE_DTYPE, bpe_byte_alphabet, bpe_table
    v = bperef.vocab()
    table, pieces, byte_ids, skipped = bpe_table(bperef.VOCAB, bperef.MERGES, byte_level=False, word_bytes=bperef.CASE_WORD)
    nf = int(table.num_final)
    assert pieces.dtype == BPE_PIECE_DTYPE and pieces.shape == (nf,) and pieces.itemsize == 16 and (pieces["reserved"] == 0).all()
    assert {k: why for k, _, why in skipped if why != "no merge"} == bperef.SKIPPED
    assert [(k, m, why) for k, m, why in skipped if why != "no merge"] == v.skipped
    # the tokens of two or more bytes that no merge makes: a lead inside, a dot, a newline
    assert sorted(t for _, t, why in skipped if why == "no merge") == [b"a\nb", b"a b", b"a.b"]
    lines = [l + r for k, (l, r) in enumerate(bperef.MERGES) if k not in bperef.SKIPPED]
    lens = table.final_lengths()
    got = {lines[ln]: tuple(int(x) for x in pieces[s]) for s, ln in enumerate(state_strings(table)) if lens[s] >= 1}
    undropped = Vocab(bperef.VOCAB, bperef.MERGES, word=bperef.CASE_WORD)
    assert got == {p: undropped.quad(p) for p in undropped.pieces}
    assert got[b"abc"] == (104, 4, 2, 0) and got[b" ab"] == (110, 10, 2, 0) and got[b"play"] == (109, 9, 2, 0)
    assert byte_ids.dtype == np.int32 and byte_ids.tolist() == (300 + np.arange(256)).tolist()
    # any_split: every split 0, nothing else moves
    _, p2, _, s2 = bpe_table(bperef.VOCAB, bperef.MERGES, byte_level=False, word_bytes=bperef.CASE_WORD, any_split=True)
    assert (p2["split"] == 0).all() and np.array_equal(p2["rank"], pieces["rank"]) and np.array_equal(p2["id"], pieces["id"]) and s2 == skipped
    # the byte alphabet: a bijection of the 256 bytes onto printable characters, GPT-2's spellings
    alpha = bpe_byte_alphabet()
    assert sorted(alpha) == list(range(256)) and len(set(alpha.values())) == 256
    assert alpha[0x20] == "Ġ" and alpha[0x0A] == "Ċ" and alpha[ord("a")] == "a" and alpha[0xC3] == "Ã" and alpha[0xAD] == chr(256 + 33 + 34)
    assert all(len(c) == 1 and c.isprintable() and not c.isspace() for c in alpha.values())
    every = {alpha[b]: b for b in range(256)}                   # 256 single-byte tokens, each with its byte as its id
    every.update({"Ġa": 256, alpha[0xC3] + alpha[0xA9]: 257})
    t3, p3, b3, s3 = bpe_table(every, [("Ġ", "a"), "Ã ©"], lead=b" ")
    assert b3.tolist() == list(range(256)) and s3 == []
    assert sorted(int(x) for x in p3["id"] if x >= 0) == [256, 257] and sorted(t3.final_lengths().tolist()) == [2, 2]
    # a written vocabulary in GPT-2's form, and the remaining reasons
    voc = {"a": 0, "b": 1, "Ġ": 2, "ab": 3, "Ġab": 4, "aĠ": 5, "AB": 6, "€": 7, "x" * 1024: 8, "Ċ": 9, "aĊ": 10}
    mer = ["a b", "Ġ ab", "a Ġ", "A B", "b a", "x" * 512 + " " + "x" * 512, "a Ċ", "€ a"]
    _, p4, b4, s4 = bpe_table(voc, mer)
    assert [(k, why) for k, _, why in s4] == [(7, "not byte-level"), (2, "lead inside"), (4, "not in vocab"), (5, "too long"), (6, "newline"),
                                              (7, "not byte-level"), (5, "no merge"), (8, "no merge"), (10, "no merge")]
    assert sorted(int(x) for x in p4["id"] if x >= 0) == [3, 4, 6] and b4[ord("a")] == 0 and b4[32] == 2 and b4[10] == 9
    _, p5, _, s5 = bpe_table(voc, mer[:4], ignore_case=True)
    assert (3, ("A", "B"), "ambiguous") in s5 and sorted(int(x) for x in p5["id"] if x >= 0) == [3, 4]
    with pytest.raises(ValueError):
        bpe_table(voc, mer, max_word_bytes=256)
    with pytest.raises(ValueError):
        bpe_table(voc, mer, lead=b"a")
    with pytest.raises(ValueError):
        bpe_table(voc, ["b a"])


def test_the_small_log_written_by_hand():
    """The ids of the surface tests' log, written out by hand in bperef.py, are what the rule gives."""
    from phfpfac_amd import bpe_byte_alphabet
    back = {c: b for b, c in bpe_byte_alphabet().items()}
    enc = lambda t: bytes(back[c] for c in t)                   # noqa: E731
    v = Vocab({enc(t): i for i, t in enumerate(bperef.LOG_TOKENS)}, [(enc(l), enc(r)) for l, r in bperef.LOG_MERGES], lead=0x20,
              max_word=64, word=bperef.DEFAULT_WORD)
    data = np.frombuffer(bperef.LOG, dtype=np.uint8)
    off = np.concatenate([[0], np.flatnonzero(data == 10) + 1])
    ids, pos, tok_off = by_strings(data, data.size, v, off)
    assert ids.tolist() == bperef.LOG_IDS and tok_off.tolist() == bperef.LOG_TOK_OFF
    assert (pos.astype(np.int64) - np.repeat(off[:-1], np.diff(tok_off.astype(np.int64)))).tolist() == bperef.LOG_POS
    assert bperef.boundaries_ok(data, data.size, off, v)


# ---------------------------------------------------------------------------
# the library

def test_merge_lists_against_the_tokenizers_library():
    """(a) BPE(vocab, merges).tokenize(word) on random unambiguous merge lists over a 4-letter alphabet: 150 merges,
    tokens of at most 6 bytes, words of 1..16 bytes.  All must agree and none is skipped."""
    pytest.importorskip("tokenizers")
    from tokenizers.models import BPE
    rng = np.random.default_rng(29)
    letters = b"abcd"
    n_words = 0
    for k in range(8):
        merges, made = [], set()
        while len(merges) < 150:
            for m in bperef.random_merges(rng, letters, 150, 6):
                if m[0] + m[1] not in made and len(merges) < 150:
                    made.add(m[0] + m[1])
                    merges.append(m)
        # a merge list as a trainer makes it: both halves exist before the merge
        have = {bytes([c]) for c in letters}
        ordered = []
        for l, r in merges:
            if l in have and r in have:
                ordered.append((l, r))
                have.add(l + r)
        merges = ordered
        d = {bytes([c]): i for i, c in enumerate(letters)}
        for j, (l, r) in enumerate(merges):
            d[l + r] = 10 + j
        v = Vocab(d, merges, lead=-1, max_word=64, word=letters)
        assert not v.skipped and len(merges) >= 100, len(merges)
        model = BPE({t.decode(): i for t, i in d.items()}, [(l.decode(), r.decode()) for l, r in merges])
        for _ in range(250):
            word = bytes(letters[int(i)] for i in rng.integers(0, 4, size=int(rng.integers(1, 17))))
            data = np.frombuffer(word, dtype=np.uint8)
            ids, _, _ = by_strings(data, data.size, v)
            lib = [t.id for t in model.tokenize(word.decode())]
            assert ids.tolist() == lib, f"list {k}: {word!r}: {ids.tolist()}, the library says {lib}"
            n_words += 1
    assert n_words == 2000


def test_a_trained_byte_level_tokenizer_through_bpe_table():
    """(b) A tokenizer trained here with BpeTrainer behind ByteLevel(add_prefix_space=False), fed through
    bpe_table(byte_level=True): encode(text).ids against the rule on texts of lowercase letters separated by one or
    two spaces or a newline."""
    tokenizers = pytest.importorskip("tokenizers")
    import json
    from tokenizers import Tokenizer, pre_tokenizers
    from tokenizers.models import BPE
    from tokenizers.trainers import BpeTrainer
    from phfpfac_amd import bpe_table
    rng = np.random.default_rng(31)
    stems = ["play", "the", "token", "merge", "rank", "byte", "pair", "er", "ing", "s", "un", "re", "a", "ab", "abc", "zz"]

    def sentence():
        out = []
        for _ in range(int(rng.integers(1, 12))):
            out.append("".join(stems[int(i)] for i in rng.integers(0, len(stems), size=int(rng.integers(1, 4)))))
            out.append([" ", " ", "  ", "\n"][int(rng.integers(4))])
        return "".join(out[:-1])                                # (separated: a trailing run of spaces would be one `ĠĠ`)
    tok = Tokenizer(BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.train_from_iterator([sentence() for _ in range(400)],
                            BpeTrainer(vocab_size=400, initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False))
    model = json.loads(tok.to_str())["model"]
    table, pieces, byte_ids, skipped = bpe_table(model["vocab"], model["merges"], byte_level=True)
    assert [s for s in skipped if s[2] != "no merge"] == [] and len(model["merges"]) > 100
    # the rule over the table's own strings: state -> string through the id map, as the scan would report them
    lines = []
    back = {c: b for b, c in __import__("phfpfac_amd").bpe_byte_alphabet().items()}
    for m in model["merges"]:
        l, r = m.split(" ") if isinstance(m, str) else m
        lines.append((bytes(back[c] for c in l), bytes(back[c] for c in r)))
    d = {bytes(back[c] for c in t): i for t, i in model["vocab"].items()}
    v = Vocab(d, lines, lead=0x20, max_word=64, word=bperef.DEFAULT_WORD)
    lens = table.final_lengths()
    made = [l + r for l, r in lines]
    got = {made[ln]: tuple(int(x) for x in pieces[s]) for s, ln in enumerate(state_strings(table)) if lens[s] >= 1}
    assert got == {p: v.quad(p) for p in v.pieces}
    assert np.array_equal(byte_ids, v.byte_ids)
    for k in range(300):
        text = sentence()
        data = np.frombuffer(text.encode(), dtype=np.uint8)
        ids, _, _ = by_strings(data, data.size, v)
        assert ids.tolist() == tok.encode(text).ids, f"text {k}: {text!r}"
