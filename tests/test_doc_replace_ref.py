"""The per-document host reference of selection and find-and-replace (tests/docreplref.py) against Python `re` applied to
every document on its own.  CPU only."""
import numpy as np
import pytest

from docref import random_offsets
from docreplref import per_doc
from llref import line_lengths
from orc import Oracle
from replref import re_replace, rep_table


def write_patterns(tmp_path, pats):
    f = tmp_path / "p.pat"
    f.write_bytes(b"".join(p + b"\n" for p in pats))
    return str(f)


@pytest.mark.parametrize("seed", range(12))
def test_per_document_reference_agrees_with_re(seed, tmp_path):
    rng = np.random.default_rng([seed, 71])
    alpha = b"abc"[: int(rng.integers(2, 4))]
    pats = [bytes(rng.choice(list(alpha), int(rng.integers(1, 6)))) for _ in range(int(rng.integers(1, 12)))]
    if seed % 3 == 0:
        pats.append(pats[0])                                   # a duplicate line
    reps = [bytes(rng.choice(list(b"XYZ"), int(rng.integers(0, 9)))) for _ in pats]
    data = np.frombuffer(bytes(rng.choice(list(alpha + b"d"), int(rng.integers(0, 600)))), dtype=np.uint8)
    off = random_offsets(rng, data.size, int(rng.integers(1, 30)), empties=int(rng.integers(0, 4)))
    path = write_patterns(tmp_path, pats)
    o = Oracle(path, 1, 1)
    first, pos, ids, out_off, out = per_doc(o, data, off, line_lengths(path), rep_table(reps))
    o.close()
    assert first[-1] == pos.size and out_off[-1] == out.size
    for d in range(off.size - 1):
        a, b = int(off[d]), int(off[d + 1])
        want, ex = re_replace(pats, reps, data[a:b], 0, b - a)
        assert ex == 0
        assert bytes(out[int(out_off[d]):int(out_off[d + 1])]) == bytes(want)
        assert (pos[int(first[d]):int(first[d + 1])] < b - a).all()


def test_worked_example(tmp_path):
    """Patterns abc and cd, documents xab and cdy, redaction with '*': xab + **y per document, x***dy as one text."""
    pats = [b"abc", b"cd"]
    reps = [b"***", b"**"]
    path = write_patterns(tmp_path, pats)
    data = np.frombuffer(b"xabcdy", dtype=np.uint8)
    off = np.array([0, 3, 6], dtype=np.uint64)
    o = Oracle(path, 1, 1)
    first, pos, ids, out_off, out = per_doc(o, data, off, line_lengths(path), rep_table(reps))
    o.close()
    assert bytes(out) == b"xab**y" and list(out_off) == [0, 3, 6]
    assert list(first) == [0, 0, 1] and list(pos) == [0] and list(ids) == [2]
    assert bytes(re_replace(pats, reps, data, 0, data.size)[0]) == b"x***dy"
