"""An exact multi-pattern matcher that builds no trie (the checker, never the product), for automata too large for the
CPU oracle's dense 256-entry rows (tests/orc.py) or for oracle/ac_serial.c.

It works one pattern length L at a time: a 64-bit polynomial hash of every window of length L, kept in one array and
extended by one byte per length (h_L = h_{L-1} * B + data[p + L - 1], mod 2^64); a bit-table filter on a mix of the
hash and L; an exact lookup among the sorted hashes of the patterns of length L; and a byte-for-byte check of every
candidate against every pattern with that hash, so a hash collision can never make a record.  Memory is O(n + pattern
bytes) and independent of the number of states.

The rules are the reference's (tests/orc.py ``Oracle.scan_spec``): ids are 1-based line numbers, the later of identical
lines wins, a record (pos, L) is kept for pos < n_owned and pos + L <= n_avail, and the output is ordered by (position,
pattern length)."""
import numpy as np

MIX = np.uint64(0x9E3779B97F4A7C15)
SALT = np.uint64(0xD6E8FEB86659FD93)
BASE = 0xA0761D6478BD642F                # any odd 64-bit number; tests pass weak ones to show the byte check at work
CHUNK = 1 << 22                          # positions per filter pass (bounds the temporaries)


def read_lines(patterns):
    """Lines of a pattern file (path) or image (bytes), as the product's reader splits them."""
    img = patterns if isinstance(patterns, (bytes, bytearray)) else open(patterns, "rb").read()
    if not img.endswith(b"\n"):
        raise ValueError("pattern file must end with a newline")
    return bytes(img[:-1]).split(b"\n")


def format_lines(pos, ids, base=0):
    """The reference's text, "At position %4d, match pattern %d\\n" per record, formatted in Python."""
    return "".join(f"At position {p:4d}, match pattern {i}\n"
                   for p, i in zip((np.asarray(pos, dtype=np.int64) + base).tolist(), np.asarray(ids).tolist())).encode()


class BigRef:
    """``BigRef(pattern file or image)``; ``scan_spec`` has ``Oracle.scan_spec``'s interface."""

    def __init__(self, patterns, base=BASE, filter_bits=24):
        winner = {}
        for i, p in enumerate(read_lines(patterns), start=1):
            if not p:
                raise ValueError(f"pattern {i} is empty")
            winner[p] = i                                       # the last of identical lines wins
        by_len = {}
        for p, i in winner.items():
            by_len.setdefault(len(p), []).append((p, i))
        self.base = np.uint64(base)
        self.shift = np.uint64(64 - filter_bits)
        self.filter = np.zeros(1 << filter_bits, dtype=bool)
        self.groups = {}                        # L -> (sorted hashes, patterns [k, L], ids, whether two hashes are equal)
        for L, items in by_len.items():
            pats = np.frombuffer(b"".join(p for p, _ in items), dtype=np.uint8).reshape(len(items), L)
            ids = np.array([i for _, i in items], dtype=np.int32)
            h = np.zeros(len(items), dtype=np.uint64)
            with np.errstate(over="ignore"):
                for j in range(L):
                    h = h * self.base + pats[:, j]
                self.filter[self._key(h, L)] = True
            o = np.argsort(h, kind="stable")
            h = h[o]
            self.groups[L] = (h, pats[o], ids[o], bool((h[1:] == h[:-1]).any()))
        self.max_len = max(self.groups) if self.groups else 0

    def _key(self, h, L):
        with np.errstate(over="ignore"):
            return ((h ^ (np.uint64(L) * SALT)) * MIX) >> self.shift

    def _length(self, buf, h, L, cnt):
        """(positions, ids) of the patterns of length L at positions [0, cnt), h[p] = hash of buf[p : p + L]."""
        gh, gp, gid, shared = self.groups[L]
        cand = [c0 + np.flatnonzero(self.filter[self._key(h[c0:min(c0 + CHUNK, cnt)], L)])
                for c0 in range(0, cnt, CHUNK)]
        cand = np.concatenate(cand) if cand else np.empty(0, dtype=np.int64)
        ch = h[cand]
        lo = np.searchsorted(gh, ch, side="left")
        if shared:                                              # some patterns of this length share a hash
            k = np.searchsorted(gh, ch, side="right") - lo
        else:
            k = (gh[np.minimum(lo, gh.size - 1)] == ch).astype(np.int64)
        keep = k > 0
        cand, lo, k = cand[keep], lo[keep], k[keep]
        # every (window, pattern with the window's hash) pair, checked byte for byte
        rep = np.repeat(np.arange(cand.size), k)
        pidx = lo[rep] + (np.arange(rep.size) - (np.cumsum(k) - k)[rep])
        at = cand[rep]
        ok = np.ones(rep.size, dtype=bool)
        for j in range(L):
            ok &= buf[at + j] == gp[pidx, j]
        return at[ok], gid[pidx[ok]]

    def scan_spec(self, data, n=None, n_owned=None):
        """(pos int64[], id int32[]) of every pattern occurrence in data[:n] that starts before n_owned (default n),
        ordered by (position, pattern length)."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
        n_avail = buf.size if n is None else min(int(n), buf.size)
        n_owned = n_avail if n_owned is None else min(int(n_owned), n_avail)
        buf = np.ascontiguousarray(buf[:n_avail])
        h = np.zeros(n_avail, dtype=np.uint64)
        pos, lens, ids = [], [], []
        for L in range(1, self.max_len + 1):
            m = n_avail - L + 1
            if m <= 0:
                break
            hv = h[:m]
            with np.errstate(over="ignore"):
                np.multiply(hv, self.base, out=hv)
                np.add(hv, buf[L - 1:L - 1 + m], out=hv, casting="unsafe")
            cnt = min(n_owned, m)
            if L in self.groups and cnt > 0:
                p, i = self._length(buf, h, L, cnt)
                pos.append(p)
                ids.append(i)
                lens.append(np.full(p.size, L, dtype=np.int32))
        if not pos:
            return np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int32)
        pos, lens, ids = np.concatenate(pos).astype(np.int64), np.concatenate(lens), np.concatenate(ids)
        o = np.lexsort((lens, pos))
        return pos[o], ids[o].astype(np.int32)

    def close(self):
        pass
