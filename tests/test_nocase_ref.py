"""Case-insensitive matching on the host: the fold function (pfac_fold_ascii, the one definition the scan kernel
shares), the nocase table builders against the plain builders on pre-folded images, the nocase character-class builder
against oracle/charclass_oracle.py, and the reference of the GPU tests (tests/nocaseref.py) against a second matcher on
every named GPU case."""
import importlib.util
import os

import numpy as np
import pytest

import nocaseref
import orc
from phfpfac_amd import PfacTable, fold_ascii
from phfpfac_amd._ffi import host_lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(REPO, "tests", "golden", "data")
_spec = importlib.util.spec_from_file_location("charclass_oracle", os.path.join(REPO, "oracle", "charclass_oracle.py"))
cco = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cco)

FOLD = nocaseref.FOLD


# ---------------------------------------------------------------------------
# the fold function

def test_fold_table_is_ascii_lower():
    assert bytes(FOLD) == bytes(bytes([b]).lower()[0] if b < 0x80 else b for b in range(256))


def test_fold_boundary_bytes():
    got = fold_ascii(bytes([0x40, 0x41, 0x5A, 0x5B, 0x60, 0x61, 0x7A, 0x7B, 0xC1, 0xDA, 0xE1, 0xFA]))
    assert bytes(got) == bytes([0x40, 0x61, 0x7A, 0x5B, 0x60, 0x61, 0x7A, 0x7B, 0xC1, 0xDA, 0xE1, 0xFA])


@pytest.mark.parametrize("at", range(4))
def test_fold_every_value_at_every_byte_of_a_dword(at):
    for fill in (0x00, 0x41, 0x5A, 0x7F, 0xFF):
        buf = np.full((256, 4), fill, dtype=np.uint8)
        buf[:, at] = np.arange(256)
        np.testing.assert_array_equal(fold_ascii(buf.ravel()), FOLD[buf.ravel()])


@pytest.mark.parametrize("at", range(3))
def test_fold_every_pair_of_adjacent_bytes(at):
    """All 65536 values of two neighbouring bytes of a dword: no carry crosses from one byte into the next."""
    v = np.arange(65536)
    for fill in (0x00, 0x5A, 0xFF):
        buf = np.full((65536, 4), fill, dtype=np.uint8)
        buf[:, at] = v & 255
        buf[:, at + 1] = v >> 8
        np.testing.assert_array_equal(fold_ascii(buf.ravel()), FOLD[buf.ravel()])


def test_fold_every_length_and_misalignment():
    L = host_lib()
    rng = np.random.default_rng(67)
    raw = np.zeros(256, dtype=np.uint8)
    base = (-raw.ctypes.data) % 16                      # raw[base] is 16-byte aligned
    for mis in range(16):
        for n in range(68):
            raw[:] = rng.integers(0, 256, raw.size)
            raw[base + mis: base + mis + n] = rng.choice(np.arange(0x38, 0x80, dtype=np.uint8), n)    # dense in letters
            src = raw.copy()
            dst = np.full(n + 32, 0xEE, dtype=np.uint8)
            d_at = 8 + (mis * 5) % 8                    # (the destination is misaligned on its own)
            assert L.pfac_fold_ascii(dst.ctypes.data + d_at, raw.ctypes.data + base + mis, n) == 0
            np.testing.assert_array_equal(raw, src)     # the source is only read
            np.testing.assert_array_equal(dst[d_at: d_at + n], FOLD[src[base + mis: base + mis + n]])
            assert (dst[:d_at] == 0xEE).all() and (dst[d_at + n:] == 0xEE).all()
            # in place
            assert L.pfac_fold_ascii(raw.ctypes.data + base + mis, raw.ctypes.data + base + mis, n) == 0
            want = src.copy()
            want[base + mis: base + mis + n] = FOLD[src[base + mis: base + mis + n]]
            np.testing.assert_array_equal(raw, want)
    assert L.pfac_fold_ascii(None, None, 0) == 0 and L.pfac_fold_ascii(None, raw.ctypes.data, 4) == -1


# ---------------------------------------------------------------------------
# the builders

def same_table(a, b):
    np.testing.assert_array_equal(a.blob(), b.blob())


def test_nocase_builder_equals_plain_builder_on_the_folded_image():
    for name in ("experimentpattern", "xaa", "bytefile_10000byte"):
        img = open(os.path.join(DATA, name), "rb").read()
        img = bytes(b & 0xDF if (0x61 <= b <= 0x7A and i % 3 == 0) else b for i, b in enumerate(img))   # some upper case
        assert (nocaseref.fold_bytes(img) != img) == (name != "bytefile_10000byte")      # (that one is UTF-8 without a letter)
        for width in (64, 256):
            t = PfacTable.from_bytes(img, width, ignore_case=True)
            assert t.ignore_case and not PfacTable.from_bytes(img, width).ignore_case
            same_table(t, PfacTable.from_bytes(nocaseref.fold_bytes(img), width))
    sym = nocaseref.symbol_patterns()
    same_table(PfacTable.from_bytes(sym, 256, ignore_case=True), PfacTable.from_bytes(nocaseref.fold_bytes(sym), 256))


@pytest.mark.parametrize("n_parts", [4, 7])
def test_nocase_partitions_equal_plain_partitions_of_the_folded_image(n_parts, tmp_path):
    img = open(os.path.join(DATA, "xab"), "rb").read().title() + b"Foo\nfoo\nFOO\nfoO\n" * 3     # duplicates once folded, near a cut or not
    pf = tmp_path / "mixed.pat"
    pf.write_bytes(img)
    for k in range(n_parts):
        want = PfacTable.from_bytes(nocaseref.fold_bytes(img), 256, part=k, n_parts=n_parts)
        same_table(PfacTable.from_bytes(img, 256, part=k, n_parts=n_parts, ignore_case=True), want)
        same_table(PfacTable.from_file_part(str(pf), 256, k, n_parts, ignore_case=True), want)


def escape_all(lines):
    """A pattern file for the escaped reader that decodes to exactly `lines`: every byte as \\xNN."""
    return b"".join(b"".join(b"\\x%02x" % b for b in l) + b"\n" for l in lines)


def lines_of(table):
    """The byte strings a literal table matches, by pattern id (walks the table's own lookup from the root)."""
    out = {}
    stack = [(table.num_final + 1, b"")]
    while stack:
        s, path = stack.pop()
        for ch in range(256):
            nxt = table.lookup(s, ch)
            if nxt >= 0:
                if nxt < table.num_final:
                    out[int(table.idmap[nxt])] = path + bytes([ch])
                stack.append((nxt, path + bytes([ch])))
    return out


def test_nocase_escaped_builder_folds_after_decoding(tmp_path):
    images = [orc.ESCAPED, b"hex\\x41\\x5a\\x5B\\x61x\\101\n"] + orc.escape_fuzz_images()[:12]
    folded_some = 0
    for n, img in enumerate(images):
        pf = tmp_path / f"e{n}.pat"
        pf.write_bytes(img)
        plain = PfacTable.from_file(str(pf), 256, escapes=True)
        got = PfacTable.from_file(str(pf), 256, escapes=True, ignore_case=True)
        assert got.ignore_case
        # the pre-folded image of an ESCAPED file: decode (the plain table's own strings, by line), fold, encode again
        by_id = lines_of(plain)
        if len(by_id) != plain.n_patterns:               # duplicate lines: their text is not in the table; skip the image
            continue
        lines = [by_id[i] for i in range(1, plain.n_patterns + 1)]
        folded = [nocaseref.fold_bytes(l) for l in lines]
        if len(set(folded)) != len(folded):
            continue
        folded_some += folded != lines
        pre = tmp_path / f"e{n}.folded.pat"
        pre.write_bytes(escape_all(folded))
        same_table(got, PfacTable.from_file(str(pre), 256, escapes=True))
    assert folded_some >= 5


def test_nocase_escape_letters_are_not_folded(tmp_path):
    """\\x41 and A give the same table; the X of an escape is not a letter of the pattern ("\\X41" is no escape at all:
    a backslash, then the letters)."""
    def build(img, **kw):
        pf = tmp_path / "p.pat"
        pf.write_bytes(img)
        return PfacTable.from_file(str(pf), 256, escapes=True, **kw)
    same_table(build(b"b\\x41d\n", ignore_case=True), build(b"bAd\n", ignore_case=True))
    same_table(build(b"b\\x41d\n", ignore_case=True), build(b"bad\n"))
    same_table(build(b"\\101\\x5A\\n\\T\n", ignore_case=True), build(b"az\\n\\\\t\n"))
    same_table(build(b"\\X41\n", ignore_case=True), build(b"\\\\x41\n"))


def test_nocase_duplicates_resolve_on_folded_bytes():
    same_table(PfacTable.from_bytes(b"Foo\nfoo\n", 256, ignore_case=True), PfacTable.from_bytes(b"foo\nfoo\n", 256))
    t = PfacTable.from_bytes(b"foo\nbar\nFOO\n", 256, ignore_case=True)
    assert sorted(lines_of(t).items()) == [(2, b"bar"), (3, b"foo")]          # the last line wins


def test_nocase_file_builder(tmp_path):
    pf = tmp_path / "p.pat"
    pf.write_bytes(b"Hello\nWORLD\\x41\n")
    same_table(PfacTable.from_file(str(pf), 64, ignore_case=True), PfacTable.from_bytes(b"hello\nworld\\x41\n", 64))
    same_table(PfacTable.from_file(str(pf), 64, escapes=True, ignore_case=True), PfacTable.from_bytes(b"hello\nworlda\n", 64))
    same_table(PfacTable.from_blob(PfacTable.from_file(str(pf), 64, ignore_case=True).blob(), ignore_case=True),
               PfacTable.from_bytes(b"hello\nworld\\x41\n", 64))
    assert PfacTable.from_blob(PfacTable.from_file(str(pf), 64).blob(), ignore_case=True).ignore_case


def test_plain_builders_are_unchanged():
    """The committed reference digests of the plain builders still hold (tests/test_table.py pins them too); here: a
    pattern file with upper case gives another table with and without the flag."""
    img = b"Foo\nbar\n"
    assert not np.array_equal(PfacTable.from_bytes(img, 256).blob(), PfacTable.from_bytes(img, 256, ignore_case=True).blob())
    assert sorted(lines_of(PfacTable.from_bytes(img, 256)).values()) == [b"Foo", b"bar"]


# ---------------------------------------------------------------------------
# character classes

def fold_set(s, negated):
    """The class rule of the nocase builders on a parsed 256-entry set: the LISTED set is folded (upper-case members
    become their lower-case letters), a negated class complements the folded set."""
    listed = ~s if negated else s.copy()
    up = listed[0x41:0x5B].copy()
    listed[0x41:0x5B] = False
    listed[0x61:0x7B] |= up
    return ~listed if negated else listed


CC_ATOMS = [(b"a", False), (b"B", False), (b"Z", False), (b"0", False), (b"\\x41", False), (b"\\101", False), (b"@", False),
            (b"[ab]", False), (b"[AB]", False), (b"[^a]", True), (b"[^A]", True), (b"[A-Z]", False), (b"[a-z]", False),
            (b"[Z-a]", False), (b"[@-\\x5b]", False), (b"[X-c]", False), (b"[^A-Z]", True), (b"[^Q]", True), (b"[0-9A-F]", False),
            (b"[\\x41-\\x43]", False), (b"[^\\x00-\\x60]", True), (b"[^Z-a]", True)]


def cc_walk(t, data):
    pos, ids = [], []
    n, root = data.size, t.num_final + 1
    for i in range(n):
        s = root
        for j in range(i, n):
            s = t.lookup(s, int(data[j]))
            if s < 0:
                break
            if s < t.num_final:
                for k in range(t.out_first[s], t.out_first[s + 1]):
                    pos.append(i)
                    ids.append(int(t.out_ids[k]))
    return np.array(pos, dtype=np.int64), np.array(ids, dtype=np.int32)


def test_fold_set_rule_on_the_named_classes():
    def one(atom, negated):
        return fold_set(cco.parse(atom + b"\n")[0][0], negated)
    na = one(b"[^a]", True)
    assert not na[ord("a")] and na[ord("A")] and na[ord("b")]           # rejects a -- and A once the input is folded
    nA = one(b"[^A]", True)
    assert not nA[ord("a")] and nA[ord("A")]
    np.testing.assert_array_equal(np.flatnonzero(one(b"[A-Z]", False)), np.arange(0x61, 0x7B))
    np.testing.assert_array_equal(np.flatnonzero(one(b"[Z-a]", False)), [0x5B, 0x5C, 0x5D, 0x5E, 0x5F, 0x60, 0x61, 0x7A])
    np.testing.assert_array_equal(np.flatnonzero(~one(b"[^Q]", True)), [ord("q")])     # a one-byte negated class


@pytest.mark.parametrize("width", [64, 256])
def test_nocase_charclass_against_the_oracle_on_folded_classes(width, tmp_path):
    rng = np.random.default_rng(500 + width)
    alphabet = np.frombuffer(b"abzqABZQ0@[`{\xc1", dtype=np.uint8)
    folded_more = 0
    for trial in range(30):
        lines, parsed = [], []
        for _ in range(int(rng.integers(1, 8))):
            atoms = [CC_ATOMS[int(k)] for k in rng.integers(0, len(CC_ATOMS), int(rng.integers(1, 5)))]
            lines.append(b"".join(a for a, _ in atoms) + b"\n")
            parsed.append([fold_set(cco.parse(a + b"\n")[0][0], neg) for a, neg in atoms])
        img = b"".join(lines)
        assert len(cco.parse(img)) == len(lines)                          # the atoms parse alone as they do in a line
        t = PfacTable.from_charclass(img, width, ignore_case=True)
        if trial % 5 == 0:
            pf = tmp_path / "cc.pat"
            pf.write_bytes(img)
            np.testing.assert_array_equal(PfacTable.from_charclass(str(pf), width, ignore_case=True).blob(), t.blob())
        data = alphabet[rng.integers(0, alphabet.size, 1200)]
        want_pos, want_ids = cco.match(img, nocaseref.fold(data), parsed=parsed)
        got_pos, got_ids = cc_walk(t, nocaseref.fold(data))
        np.testing.assert_array_equal(got_pos, want_pos, err_msg=repr(img))
        np.testing.assert_array_equal(got_ids, want_ids, err_msg=repr(img))
        folded_more += want_pos.size > cco.match(img, data)[0].size
    assert folded_more >= 10
    # the plain class builder is the one it was
    t0 = PfacTable.from_charclass(b"[^a]B\n", width)
    assert t0.lookup(t0.num_final + 1, ord("A")) >= 0 and not t0.ignore_case


# ---------------------------------------------------------------------------
# the reference of the GPU tests, and its named cases

@pytest.mark.parametrize("case", nocaseref.all_cases(), ids=repr)
def test_named_gpu_case_on_the_host(case):
    """Every input of tests/test_gpu_nocase.py: the reference agrees with the second matcher where that one applies
    (pure ASCII), the pattern file finds something as it is written, and folding finds strictly more."""
    pos, ids = case.want
    if case.ascii_only:
        bpos, bids = nocaseref.brute(case.patterns, case.data, case.n_owned)
        np.testing.assert_array_equal(pos, bpos)
        np.testing.assert_array_equal(ids, bids)
    epos, _ = nocaseref.exact(case.patterns, case.data, case.n_owned)
    assert epos.size >= 1
    assert pos.size > epos.size
    if case.n_owned is not None:
        assert pos.size and pos.max() < case.n_owned


def test_enough_cases_reach_the_second_matcher():
    assert sum(c.ascii_only for c in nocaseref.all_cases()) >= 12


def test_placement_cases_are_where_they_claim():
    by = {c.name: c for c in nocaseref.placement_cases()}
    pos, _ = by["halo-straddle"].want
    assert {4096 - 3, 2 * 4096 - 3, 3 * 4096 - 16} <= set(pos.tolist())
    for back in (1, 5, 15):
        c = by[f"owned-end-{back}"]
        assert c.n_owned < c.data.size and (c.want[0] == c.n_owned - back).any()
        assert c.n_owned - back + 17 > c.n_owned
    for rem in (1, 7, 15):
        c = by[f"ragged-tail-{rem}"]
        assert c.data.size % 16 == rem and (c.want[0] == c.data.size - 17).any() and (c.want[0] == c.data.size - 5).any()
    for m in (1, 2, 17, 1022):
        c = by[f"max-len-{m}"]
        assert PfacTable.from_bytes(c.patterns, 256, ignore_case=True).max_pat_len == m
        assert (c.want[0] == c.data.size - m).any()
    for c in nocaseref.root1_cases():
        t = PfacTable.from_bytes(c.patterns, 256, ignore_case=True)
        assert (t.s0 >= 0).sum() == 1 and t.s0[ord("q")] >= 0
        assert not (c.data == ord("q")).any()
