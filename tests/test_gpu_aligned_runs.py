"""16-bit records leave the scan as whole 16-byte blocks: the record heap gives every tile's run space for its count
rounded up to 8 records, so every run starts on a 16-byte boundary of the record array, while the tile index keeps the
exact count.  Consumers walk the tile index, so the gaps between runs never show (GPU tests, -m gpu on an MI355X)."""
import hashlib
import json
import os

import numpy as np
import pytest

from heapguard import GuardedBuffer
from orc import Oracle, match_checksum
from phfpfac_amd import GpuMatcher, PfacTable
from phfpfac_amd.dist import packed_to_records

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FP = json.load(open(os.path.join(HERE, "golden", "fingerprints.json")))


def runs_of(tix):
    cnt = (tix >> np.uint64(40)).astype(np.int64)
    first = (tix & np.uint64((1 << 40) - 1)).astype(np.int64)
    return first, cnt


def check_heap(words, tix, used, capacity, n):
    first, cnt = runs_of(tix)
    live = cnt > 0
    assert int(cnt.sum()) == n
    assert (first[live] % 8 == 0).all(), "a tile's run does not start on a 16-byte boundary"
    spans = sorted(zip(first[live].tolist(), (first[live] + cnt[live]).tolist()))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "tile runs overlap in the heap"
    assert spans[-1][1] <= used <= capacity and words.size == used
    assert used >= int(((cnt + 7) & ~7).sum())          # every run owns its padding


def test_headline_runs_aligned_in_chunked_placement(resolve):
    """The headline's table over 64 MiB of the tiled text, record array large enough for chunked placement (chunks of
    >= 1024 records per workgroup): every run starts on a multiple of 8 records, runs never overlap, and the compact
    form read through the tile index equals the expanded records."""
    import torch
    table = PfacTable.from_file(resolve("experimentpattern"), 256)
    para = open(resolve("paragraph402"), "rb").read()
    N = 64 << 20
    cap = N // 4
    buf = torch.empty(N + 4096, dtype=torch.uint8, device="cuda:0")
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.fill_tiled(buf, N, para)
        g.reserve(0, 0, cap)
        for _ in range(2):                                 # (the staging layout may adapt after the first scan)
            n = g.scan_resident(N, N, d_input=buf)
            rb, n_tiles, used = g.scan_format(0)
            assert rb == 2 and n_tiles == N // 4096
            words, tix = g.packed_to_host(0)
            check_heap(words, tix, used, cap, n)
            rec = g.records_to_host(n)
            got = packed_to_records(words, tix, 2)
            np.testing.assert_array_equal(got["pos"], rec["pos"])
            np.testing.assert_array_equal(got["state"], rec["state"])
            assert g.checksum(n) == match_checksum(rec["pos"], table.idmap[rec["state"]])
    # the per-period match count of the oracle, as in the whole-buffer test of the parity suite
    o = Oracle(resolve("experimentpattern"), 1, 1)
    from phfpfac_amd.matcher import tiled_bytes
    pos, _ = o.scan_spec(tiled_bytes(402 * 8, para))
    full, tail = divmod(N, 402)
    lpos, _ = o.scan_spec(tiled_bytes(tail, para))
    o.close()
    assert n == int(((pos >= 402) & (pos < 804)).sum()) * full + lpos.size


def test_golden_through_aligned_runs(resolve):
    """exp_x_1M_s1_w256: expanded records, checksum and the GPU text emitter against the golden output and the oracle."""
    c = FP["cases"]["exp_x_1M_s1_w256"]
    table = PfacTable.from_file(resolve(c["pattern"]), c["width"])
    data = np.frombuffer(open(resolve(c["input"]), "rb").read()[:-1], dtype=np.uint8)
    o = Oracle(resolve(c["pattern"]), 1, 1)
    opos, oids = o.scan_spec(data)
    o.close()
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        for _ in range(2):
            rec = g.scan_bytes(data)
            n = rec.size
            rb, _, used = g.scan_format(0)
            words, tix = g.packed_to_host(0)
            assert rb == 2 and n == c["lines"] == opos.size
            check_heap(words, tix, used, max(data.size // 8, 4096), n)
            np.testing.assert_array_equal(rec["pos"].astype(np.int64), opos)
            np.testing.assert_array_equal(table.idmap[rec["state"]], oids)
            assert g.checksum(n) == match_checksum(opos, oids)
            text = g.text_to_host(g.emit_text_device(0))
            assert len(text) == c["bytes"] and hashlib.md5(text).hexdigest() == c["md5"]


def test_capacity_limit(resolve):
    """Near the capacity limit: a record array of capacity_hint() records fits the scan (same matches), one with fewer
    records than matches reports overflow and still the exact count.  The record array is exactly `cap` 16-bit records
    inside guard bytes (tests/heapguard.py), so a store past the capacity shows."""
    import torch
    c = FP["cases"]["exp_x_1M_s1_w256"]
    table = PfacTable.from_file(resolve(c["pattern"]), c["width"])
    data = np.frombuffer(open(resolve(c["input"]), "rb").read()[:-1], dtype=np.uint8)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        want = g.scan_bytes(data)
        hint = g.capacity_hint(0)
        d_in = torch.from_numpy(np.concatenate([data, np.zeros(64, np.uint8)])).to("cuda:0")
        for cap, over_expected in ((hint, False), (want.size - 1, True), (want.size // 2, True)):
            d_rec = GuardedBuffer(cap * 2)                                             # cap 16-bit records, no more
            g.scan_async(data.size, data.size, d_input=d_in, d_records=d_rec.ptr, capacity=cap)
            n, over = g.scan_finish(0, allow_overflow=True)
            assert n == want.size and over == over_expected, (cap, n, over)
            if not over:
                rb, _, used = g.scan_format(0)
                assert rb == 2 and used <= cap
                got = g.records_to_host(n, d_records=d_rec.ptr)
                np.testing.assert_array_equal(got["pos"], want["pos"])
                np.testing.assert_array_equal(got["state"], want["state"])
            d_rec.check(what=f"the record array of capacity {cap}")
