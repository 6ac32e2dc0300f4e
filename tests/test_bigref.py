"""CPU side of the large-automaton tests: the trie-free matcher of tests/bigref.py against the CPU oracle and brute
force (also with hashes weak enough to collide), and the sets of tests/bigsets.py against the tables the product
builds -- each must hit the exact state, final-state and depth-2 counts it was made for."""
import numpy as np
import pytest

from bigref import BigRef, format_lines
from bigsets import BUILDERS, LIMIT, near_limit_set, over_limit, word_text
from orc import Oracle
from passfuzz import SEEDS, Case
from phfpfac_amd import PfacError, PfacTable, emit_records
from phfpfac_amd._ffi import PFAC_E_PATTERN


def same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def brute(lines, data, n_owned=None):
    winner = {}
    for i, p in enumerate(lines, start=1):
        winner[p] = i
    data = bytes(data)
    n_owned = len(data) if n_owned is None else n_owned
    recs = sorted((i, len(p), w) for p, w in winner.items() for i in range(min(n_owned, len(data) - len(p) + 1))
                  if data.startswith(p, i))
    return np.array([r[0] for r in recs], dtype=np.int64), np.array([r[2] for r in recs], dtype=np.int32)


def test_equals_the_oracle_on_every_fuzz_case(tmp_path):
    """All 66 seeds of tests/passfuzz.py (alphabets of 2 to 200 symbols, duplicate lines, patterns up to 1022 bytes,
    inputs up to 2 MB), over the whole buffer and over its owned range."""
    for s in SEEDS:
        c = Case(s)
        path = c.write_patterns(str(tmp_path / f"p{s}.pat"))
        o = Oracle(path, 1, 1)
        want = o.scan_spec(c.data, None)
        o.close()
        ref = BigRef(path)
        same(ref.scan_spec(c.data), want)
        own = want[0] < c.n_owned
        same(ref.scan_spec(c.data, None, c.n_owned), (want[0][own], want[1][own]))


def test_equals_the_oracle_on_the_dictionary(tmp_path):
    """The 1.4 M-state dictionary over 8 MiB of its own words (about the most the oracle's dense rows hold)."""
    s = BUILDERS["DICT"]()
    path = s.write(tmp_path / "dict.pat")
    data = word_text(s, 8 << 20)
    o = Oracle(path, 1, 1)
    want = o.scan_spec(data)
    o.close()
    got = BigRef(path).scan_spec(data)
    assert got[0].size > 8 << 20
    same(got, want)


@pytest.mark.parametrize("base", [None, 1, 256])
def test_equals_brute_force_on_tiny_cases(base):
    """Random sets over 2 to 4 symbols with duplicate lines, owned ranges and windows cut by the end of the buffer.
    base 1 hashes a window to the sum of its bytes (every anagram collides) and base 256 to its last 8 bytes: the
    byte-for-byte check alone keeps those exact."""
    rng = np.random.default_rng(11)
    kw = {} if base is None else {"base": base}
    for trial in range(150):
        sym = np.frombuffer(b"abcd", dtype=np.uint8)[: int(rng.integers(2, 5))]
        lines = [sym[rng.integers(0, sym.size, int(rng.integers(1, 13)))].tobytes() for _ in range(int(rng.integers(1, 30)))]
        lines += [lines[int(i)] for i in rng.integers(0, len(lines), int(rng.integers(0, 3)))]
        data = sym[rng.integers(0, sym.size, int(rng.integers(0, 400)))]
        n_owned = int(rng.integers(0, data.size + 1))
        ref = BigRef(b"\n".join(lines) + b"\n", **kw)
        same(ref.scan_spec(data), brute(lines, data))
        same(ref.scan_spec(data, None, n_owned), brute(lines, data, n_owned))


@pytest.mark.parametrize("base", [1, 256])
def test_weak_hashes_stay_exact_at_size(base, tmp_path):
    """A weak hash on a real case (2 600 dictionary words, 200 kB): base 256 keeps the last 8 bytes only, so words
    that share them collide; base 1 makes anagrams collide."""
    c = Case(5)
    path = c.write_patterns(str(tmp_path / "p.pat"))
    o = Oracle(path, 1, 1)
    want = o.scan_spec(c.data)
    o.close()
    same(BigRef(path, base=base, filter_bits=8).scan_spec(c.data), want)


def test_text_formatter_equals_the_host_emitter(tmp_path):
    rng = np.random.default_rng(3)
    pos = np.sort(rng.integers(0, 10**9, 5000))
    ids = rng.integers(1, 10**7, 5000).astype(np.int32)
    rec = np.zeros(pos.size, dtype=[("pos", np.uint32), ("state", np.uint32)])
    rec["pos"], rec["state"] = pos, np.arange(pos.size)
    emit_records(str(tmp_path / "o.txt"), rec, ids, base=7)
    assert (tmp_path / "o.txt").read_bytes() == format_lines(pos, ids, base=7)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_sets_hit_their_statistics(name, tmp_path):
    s = BUILDERS[name]()
    s.check(PfacTable.from_file(s.write(tmp_path / "p.pat"), 256))


def test_one_byte_past_the_size_limit_is_refused(tmp_path):
    """NEAR_LIMIT sits exactly on the builder's limit (lines + 2 + pattern bytes = (2^31 - 1) / 256); one byte more is
    PFAC_E_PATTERN, through both readers, and nothing else breaks."""
    s = near_limit_set()
    assert len(s.lines) + 2 + sum(len(p) for p in s.lines) == LIMIT
    (tmp_path / "over.pat").write_bytes(over_limit(s))
    for build in (lambda: PfacTable.from_file(str(tmp_path / "over.pat"), 256), lambda: PfacTable.from_bytes(over_limit(s), 256)):
        with pytest.raises(PfacError) as e:
            build()
        assert e.value.status == PFAC_E_PATTERN and "too large" in str(e.value)
    t = PfacTable.from_bytes(s.image(), 256)
    assert t.num_final == len(s.lines)
