"""Host reference for the whole-word filter (the checker, never the product), written from the rule in include/pfac.h:

    W(b)   = bit b of word_set (uint64[4]: byte b at bit b & 63 of word b >> 6; None = [0-9A-Za-z_])
    in[i]  = buf[i] for 0 <= i < n; in[-1] = prev, in[n] = next (-1: no byte there)
    cut(i) = in[i-1] and in[i] both exist and are word bytes, and (with documents) i is not one of the offsets
    keep   = not (edges & LEFT and cut(pos)) and not (edges & RIGHT and cut(pos + len))

`filter_words` returns the boolean keep mask over the records (pos, lens) of a scan of `buf`; the records come from a
CPU matcher, their lengths from the pattern file's own lines."""
import numpy as np

LEFT, RIGHT, BOTH = 1, 2, 3
DEFAULT_WORD = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ_abcdefghijklmnopqrstuvwxyz"


def word_table(word_set=None):
    """bool[257]: [b + 1] = W(b) for b in -1..255 (no byte: never a word byte)."""
    tab = np.zeros(257, dtype=bool)
    if word_set is None:
        tab[np.frombuffer(DEFAULT_WORD, dtype=np.uint8).astype(np.int64) + 1] = True
    else:
        ws = [int(x) for x in np.asarray(word_set, dtype=np.uint64)]
        assert len(ws) == 4
        for b in range(256):
            tab[b + 1] = (ws[b >> 6] >> (b & 63)) & 1
    return tab


def cuts(buf, word_set=None, prev=-1, next=-1, off=None):
    """bool[n + 1]: cut(i) for 0 <= i <= n."""
    buf = np.asarray(buf, dtype=np.uint8)
    assert -1 <= prev <= 255 and -1 <= next <= 255
    ext = np.concatenate(([prev], buf.astype(np.int64), [next]))         # ext[i + 1] = in[i]
    isw = word_table(word_set)[ext + 1]
    cut = isw[:-1] & isw[1:]                                               # in[i - 1] and in[i]
    if off is not None:
        cut[np.asarray(off, dtype=np.int64)] = False
    return cut


def filter_words(buf, pos, lens, word_set=None, edges=BOTH, prev=-1, next=-1, off=None):
    assert edges in (LEFT, RIGHT, BOTH)
    pos = np.asarray(pos, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    n = int(np.asarray(buf).size)
    assert pos.size == 0 or (int((pos + lens).max()) <= n and int(lens.min()) >= 1)
    cut = cuts(buf, word_set, prev, next, off)
    keep = np.ones(pos.size, dtype=bool)
    if edges & LEFT:
        keep &= ~cut[pos]
    if edges & RIGHT:
        keep &= ~cut[pos + lens]
    return keep


def filter_words_loop(buf, pos, lens, word_set=None, edges=BOTH, prev=-1, next=-1, off=None):
    """The same rule record by record in plain Python (pins the vectorised form in the CPU tests)."""
    buf = bytes(np.asarray(buf, dtype=np.uint8))
    tab = word_table(word_set)
    offs = set(int(x) for x in off) if off is not None else set()
    n = len(buf)

    def at(i):
        return prev if i < 0 else (next if i >= n else buf[i])

    def cut(i):
        return bool(tab[at(i - 1) + 1]) and bool(tab[at(i) + 1]) and i not in offs

    return np.array([not ((edges & LEFT) and cut(int(p))) and not ((edges & RIGHT) and cut(int(p) + int(l)))
                     for p, l in zip(pos, lens)], dtype=bool)
