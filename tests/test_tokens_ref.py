"""The tokenize reference and its cases, without a GPU: tests/tokref.py's two forms of the rule held against each other
on every named case, every case's precondition, the small log against a textbook tokenizer that never sees a record,
token_table against replacement_table's state mapping, and tokref.check against wrong results."""
import numpy as np
import pytest

import passguard
import tokref
from passguard import TILE
from phfpfac_amd import PfacTable, replacement_table, token_table
from tokref import DROP, by_numpy, by_walk, cases, check, picks_of, ref, want_of


@pytest.fixture(scope="module")
def x():
    return ref()


def _inputs(x, name):
    W, key, entry, tokname, shape = cases(x)[name]
    pos, ids, lens = picks_of(x, name)
    tok, btok = x.tokens(W, tokname)
    off = None if shape is None else x.doc_offsets(W, key, shape)
    return (x.input(key[0]), entry, key[1], pos, lens, ids, tok, btok, off), (W, key, entry, tokname, shape)


def test_names_are_the_cases(x):
    assert tuple(cases(x)) == tokref.NAMES
    assert tuple(n for n, c in cases(x).items() if c[3] == "mixed") == tokref.MIXED


@pytest.mark.parametrize("name", tokref.NAMES)
def test_two_forms_agree(x, name):
    args, _ = _inputs(x, name)
    a, b = by_numpy(*args), by_walk(*args)
    check(a, b[0], b[1], b[2], b[3], what=name)
    assert a[0].dtype == np.int32 and a[1].dtype == np.uint32
    w = want_of(x, name)
    check(w, a[0], a[1], a[2], a[3], what=name)
    assert (np.diff(a[1].astype(np.int64)) > 0).all(), "every position emits at most one token, ascending"
    assert a[1].size == 0 or (int(a[1][0]) >= args[1] and int(a[1][-1]) < args[2])


@pytest.mark.parametrize("name", [n for n in tokref.MIXED if n not in tokref.TRIVIAL])
def test_mixed_cases_have_all_four(x, name):
    (data, entry, n_owned, pos, lens, ids, tok, btok, _), _ = _inputs(x, name)
    assert (tok[ids] != DROP).any(), "no pick token is emitted"
    assert (tok[ids] == DROP).any(), "no pick is dropped"
    cov = np.zeros(n_owned + 1, dtype=np.int64)
    np.add.at(cov, pos, 1)
    np.add.at(cov, np.minimum(pos + lens, n_owned), -1)
    gap = (np.cumsum(cov)[:n_owned] == 0) & (np.arange(n_owned) >= entry)
    assert (btok[data[:n_owned]][gap] != DROP).any(), "no gap byte is emitted"
    assert (btok[data[:n_owned]][gap] == DROP).any(), "no gap byte is dropped"


def test_preconditions_of_the_sizes(x):
    c = cases(x)
    for n in tokref.SMALL:
        assert c[f"n{n}"][1][1] == n
    tiles = {name: -(-c[name][1][1] // TILE) for name in ("t3", "t63", "t64", "t65", "t130")}
    assert tiles == {"t3": 4, "t63": 63, "t64": 64, "t65": 65, "t130": 131}
    assert picks_of(x, "none")[0].size == 0 and want_of(x, "none")[0].size > 0, "one gap over the whole input, with tokens"
    for n in passguard.SEL_COUNTS:
        assert picks_of(x, f"sel{n}")[0].size == n
    assert c["entry"][2] == 2 and want_of(x, "entry")[1][0] >= 2
    W, key, _, _, _ = c["halo"]
    assert key[2] > key[1] and c["w4-halo"][1] == key, "n_owned < n_avail"
    assert want_of(x, "w4-halo")[3] > 0, "the last pick of the dictionary's halo case ends in the halo"
    assert picks_of(x, passguard.FILTERED)[0].size < picks_of(x, "t65")[0].size


def test_preconditions_of_the_edges(x):
    pos, ids, lens = picks_of(x, "edge-end")
    at = dict(zip(pos.tolist(), lens.tolist()))
    no = tokref.EDGE_OWNED
    assert at[0] == 4, "a pick at position 0"
    assert at[TILE - 4] == 4, "a pick that ends exactly on a tile end"
    assert at[2 * TILE - 1] == 4, "a pick whose start is the last byte of a tile"
    assert at[no - 4] == 4 and want_of(x, "edge-end")[3] == 0, "a pick ending at n_owned"
    p = tokref.EDGE_LONG_AT
    assert at[p] == 1000 and (p + 999) // 64 - p // 64 + 1 >= 16 and p // TILE != (p + 999) // TILE
    t = tokref.EDGE_DENSE_TILE
    assert ((pos >= t * TILE) & (pos < (t + 1) * TILE)).sum() == TILE, "4096 picks of one byte in one tile"
    hp, _, hl = picks_of(x, "edge-halo")
    assert hp[-1] == no - 4 and hp[-1] < no - 2 < hp[-1] + hl[-1] and want_of(x, "edge-halo")[3] == 2
    # the token tables on it
    w = want_of(x, "edge-nodrop")
    per_tile = np.bincount(w[1] // TILE, minlength=7)
    assert per_tile[t] == TILE, "a tile that emits 4096 tokens"
    per_tile = np.bincount(want_of(x, "edge-picksdropped")[1] // TILE, minlength=7)
    assert per_tile[t] == 0 and per_tile[t - 1] > 0 and per_tile[t + 1] > 0, "a tile that emits nothing between tiles that do"
    assert want_of(x, "edge-alldrop")[0].size == 0 and want_of(x, "t3-alldrop")[0].size == 0
    wn = want_of(x, "t3-nullbytes")
    assert wn[0].size > 0 and (wn[0] >= tokref.TOK_BASE).all(), "byte_ids NULL: pick tokens only"
    wd = want_of(x, "t3-picksdropped")
    assert wd[0].size > 0 and (wd[0] < tokref.TOK_BASE).all(), "every pick dropped, the bytes kept"
    assert (want_of(x, "docs-alldrop")[2] == 0).all()


def test_preconditions_of_the_documents(x):
    c = cases(x)
    for shape, at in passguard.EMPTY_AT.items():
        W, key, _, _, _ = c[f"docs-{shape}"]
        off = x.doc_offsets(W, key, shape).astype(np.int64)
        where = key[1] if at is None else at
        assert (off == where).sum() >= passguard.EMPTY_RUN, f"{shape}: a run of empty documents at {where}"
    W, key, _, _, _ = c["docs-words"]
    off = x.doc_offsets(W, key, "words").astype(np.int64)
    pos, _, lens = x.picks(W, key)[:3]
    ends = pos + lens
    assert (off % 64 == 0).any() and (off % 64 == 63).any(), "starts on the first and the last position of a bitmap word"
    assert np.isin(off[1:-1], ends).any(), "a document start directly behind a pick"
    k = np.searchsorted(pos, off[1:-1], side="right") - 1
    assert ((k >= 0) & (off[1:-1] > ends[np.maximum(k, 0)]) & (np.searchsorted(pos, off[1:-1], side="left") == k + 1)).any(), \
        "a document start in the middle of a gap"
    w = want_of(x, "docs-words")
    assert w[2][0] == 0 and w[2][-1] == w[0].size and (np.diff(w[2].astype(np.int64)) >= 0).all()


def test_every_document_alone(x):
    """ids[tok_off[d] : tok_off[d + 1]] is what tokenizing document d alone gives (docreplref.per_doc: the oracle run
    on every document on its own)."""
    from docreplref import per_doc
    W, key, _, tokname, shape = cases(x)["docs-tiny"]
    off = x.doc_offsets(W, key, shape)
    sub = off[(off >= TILE) & (off <= 3 * TILE)]            # the tiny documents of tiles 1 and 2
    a, b = int(sub[0]), int(sub[-1])
    data = x.input(key[0])
    info = x.info(W)
    first, pos, ids, _, _ = per_doc(info["matcher"], data[a:b], (sub - sub[0]).astype(np.uint64), info["ll"])
    first = first.astype(np.int64)
    tok, btok = x.tokens(W, tokname)
    w = want_of(x, "docs-tiny")
    lo, hi = int(w[2][np.searchsorted(off, a)]), int(w[2][np.searchsorted(off, b)])
    got = []
    for d in range(sub.size - 1):
        s, e = int(sub[d]), int(sub[d + 1])
        p, i = pos[first[d]:first[d + 1]], ids[first[d]:first[d + 1]]
        got.append(by_walk(data[s:e], 0, e - s, p, info["ll"][i], i, tok, btok)[0])
    assert np.array_equal(np.concatenate(got), w[0][lo:hi])


def test_chained_ranges_concatenate(x):
    from llref import greedy
    W, key = 2, tokref.CHAIN_KEY
    cuts = tokref.chain_cuts(x, W)
    pos, _, lens, _ = x.picks(W, key)
    ends = pos + lens
    assert ((pos < cuts["inside"]) & (ends > cuts["inside"])).any(), "a cut inside a pick"
    assert np.isin(cuts["behind"], ends), "a cut directly behind a pick"
    assert not ((pos <= cuts["ingap"]) & (ends > cuts["ingap"])).any() and not np.isin(cuts["ingap"], ends), "a cut inside a gap"
    whole = x.want(W, key, 0, "mixed")
    data, M = x.input(key[0]), x.M(W)
    tok, btok = x.tokens(W, "mixed")
    for chain in tokref.CHAINS:
        edges = [0] + [cuts[c] for c in chain] + [key[1]]
        ids, positions, entry = [], [], 0
        for a, b in zip(edges[:-1], edges[1:]):
            na = min(b + M - 1, key[2])
            rp, ri = x.info(W)["matcher"].scan_spec(np.ascontiguousarray(data[a:na]), None)
            own = rp < b - a
            rp, ri = rp[own].astype(np.int64), ri[own].astype(np.int64)
            idx, ex = greedy(rp, x.info(W)["ll"][ri], entry, b - a)
            r = by_numpy(data[a:na], entry, b - a, rp[idx], x.info(W)["ll"][ri[idx]], ri[idx], tok, btok)
            assert r[3] == ex
            ids.append(r[0])
            positions.append(r[1].astype(np.int64) + a)
            entry = ex
        check(whole, np.concatenate(ids), np.concatenate(positions), what=f"chain {chain}")


def test_small_log_against_a_textbook_tokenizer(x, tmp_path):
    """tokenize_lines' expectation: the log's hand-written ids are what the textbook tokenizer gives line by line, and
    what the reference gives from the oracle's records of every line."""
    from docreplref import per_doc
    from llref import line_lengths
    from orc import Oracle
    vocab = {w: 100 + k for k, w in enumerate(tokref.LOG_VOCAB, 1)}
    lines = tokref.LOG.split(b"\n")[:-1]
    got = [tokref.maxmatch(line + b"\n", vocab, tokref.LOG_BYTE_BASE, tokref.LOG_DROP) for line in lines]
    assert sum(got, []) == tokref.LOG_IDS
    assert np.cumsum([0] + [len(g) for g in got]).tolist() == tokref.LOG_TOK_OFF
    path = str(tmp_path / "vocab.pat")
    open(path, "wb").write(b"".join(w + b"\n" for w in tokref.LOG_VOCAB))
    o = Oracle(path, 1, 1)
    try:
        data = np.frombuffer(tokref.LOG, dtype=np.uint8)
        off = np.concatenate([[0], np.flatnonzero(data == 10) + 1]).astype(np.uint64)
        ll = line_lengths(path)
        first, pos, ids, _, _ = per_doc(o, data, off, ll)
        doc = np.repeat(np.arange(off.size - 1), np.diff(first.astype(np.int64)))
        tok = np.array([DROP] + [100 + k for k in range(1, len(vocab) + 1)], dtype=np.int32)
        btok = (tokref.LOG_BYTE_BASE + np.arange(256)).astype(np.int32)
        btok[list(tokref.LOG_DROP)] = DROP
        for form in (by_numpy, by_walk):
            r = form(data, 0, data.size, pos + off[doc].astype(np.int64), ll[ids], ids, tok, btok, off)
            assert r[0].tolist() == tokref.LOG_IDS and r[2].tolist() == tokref.LOG_TOK_OFF
            d = np.repeat(np.arange(off.size - 1), np.diff(r[2].astype(np.int64)))
            assert (r[1].astype(np.int64) - off[d].astype(np.int64)).tolist() == tokref.LOG_POS
    finally:
        o.close()
    assert tokref.maxmatch(tokref.WORDS_TEXT, vocab, tokref.LOG_BYTE_BASE, tokref.LOG_DROP) == tokref.WORDS_IDS_PLAIN


def test_token_table_maps_ids_as_replacement_table(tmp_path):
    """A file with a duplicate line: the state of the winning line carries its token, as it carries its replacement."""
    lines = [b"he", b"she", b"he", b"hers"]
    path = str(tmp_path / "dup.pat")
    open(path, "wb").write(b"".join(p + b"\n" for p in lines))
    table = PfacTable.from_file(path, 256)
    ids = {k: 10 * k for k in range(1, len(lines) + 1)}
    tok = token_table(table, ids)
    roff, rbytes = replacement_table(table, {k: b"%d," % v for k, v in ids.items()})
    assert tok.dtype == np.int32 and tok.size == table.num_final
    for s in range(table.num_final):
        r = rbytes[int(roff[s]):int(roff[s + 1])]
        assert (tok[s] == DROP and r == b"") or r == b"%d," % tok[s], f"state {s}: token {tok[s]}, replacement {r!r}"
    assert sorted(t for t in tok.tolist() if t != DROP) == sorted({int(ids[int(table.idmap[s])]) for s in range(table.num_final) if table.final_lengths()[s] >= 1})
    assert np.array_equal(token_table(table, [10, 20, 30, 40]), tok), "one entry per line"
    part = token_table(table, {2: 7})
    assert sorted(part.tolist()).count(7) == 1 and (part[part != 7] == DROP).all(), "patterns that are not named are DROP"
    with pytest.raises(ValueError):
        token_table(table, {2: -2})


WRONG = ("missing at a tile's first position", "a covered byte emitted", "tok_off short by a tile's count", "a dropped pick emitted",
         "positions off by entry")


@pytest.mark.parametrize("kind", WRONG)
def test_check_refuses(x, kind):
    if kind == "positions off by entry":
        w = want_of(x, "entry")
        ids, pos = w[0].copy(), w[1] - np.uint32(cases(x)["entry"][2])
        with pytest.raises(AssertionError, match="token 0 is"):
            check(w, ids, pos, what=kind)
        return
    name = "docs-words"
    w = want_of(x, name)
    args, _ = _inputs(x, name)
    data, _, n_owned, pos, lens, states, tok, btok, off = args
    ids, positions, tok_off = w[0].copy(), w[1].copy(), w[2].copy()
    if kind == "missing at a tile's first position":
        j = int(np.flatnonzero(positions % TILE == 0)[1])
        ids, positions = np.delete(ids, j), np.delete(positions, j)
        with pytest.raises(AssertionError, match=f"token {j} is"):
            check(w, ids, positions, what=kind)
    elif kind == "a covered byte emitted":
        k = int(np.flatnonzero(lens >= 2)[10])
        p = int(pos[k]) + 1
        j = int(np.searchsorted(positions, p))
        ids, positions = np.insert(ids, j, tokref.BYTE_BASE + int(data[p])), np.insert(positions, j, p)
        with pytest.raises(AssertionError, match=f"token {j} is"):
            check(w, ids, positions, what=kind)
    elif kind == "tok_off short by a tile's count":
        d = int(np.searchsorted(off, 2 * TILE))
        tok_off[d:] -= np.uint64(((positions >= TILE) & (positions < 2 * TILE)).sum())
        with pytest.raises(AssertionError, match=rf"tok_off\[{d}\]"):
            check(w, ids, positions, tok_off, what=kind)
    else:
        k = int(np.flatnonzero(tok[states] == DROP)[3])
        j = int(np.searchsorted(positions, int(pos[k])))
        ids, positions = np.insert(ids, j, tokref.TOK_BASE + int(states[k])), np.insert(positions, j, int(pos[k]))
        with pytest.raises(AssertionError, match=f"token {j} is"):
            check(w, ids, positions, what=kind)
    check(w, w[0], w[1], w[2], w[3], what="the right result")
