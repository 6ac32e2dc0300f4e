"""How a scan reports that it has ended and how long it took: the dispatch carries no completion signal and no
timestamps; the kernel's last workgroup stores a DONE word behind its result words, which pfac_scan_finish polls, and
pfac_scan_elapsed_ms is first workgroup in -> last workgroup out by the kernel's own clock.  A stale DONE word, result
words of one slot read for another, or a wait that never returns would show here: back-to-back scans of two slots on
one stream, one slot reused at once, scans finished out of order, stream swaps, and the bounds of the elapsed time
under both clocks (GPU tests, -m gpu on an MI355X)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":                               # the child process of the PFAC_EVENT_TIMING test: no conftest
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    os.environ.setdefault("PFAC_ENABLE_KNOBS", "1")

from orc import Oracle, ac_whole_shard
from phfpfac_amd import GpuMatcher, PfacTable

pytestmark = pytest.mark.gpu

NC = 15                     # compute waves per workgroup of the headline kernel (tables in LDS)
TILE = 4096
SIZES = [0, 1, TILE, (NC - 1) * TILE, NC * TILE, (NC + 1) * TILE, (1 << 20) + 17]
N_TIMED = 64 << 20
PEAK_BYTES_PER_MS = 8e12 / 1e3      # HBM peak of the MI355X: no kernel moves its bytes faster
DATA = os.path.join(HERE, "golden", "data")
PAT = os.path.join(DATA, "experimentpattern")


def host_text(n):
    para = open(os.path.join(DATA, "paragraph402"), "rb").read()
    return para, np.frombuffer(para * (n // len(para) + 1), dtype=np.uint8)[:n].copy()


@pytest.fixture(scope="module")
def world():
    """The device buffer (64 MiB of the tiled paragraph), the table, and the oracle's records of every size in SIZES."""
    import torch
    para, host = host_text(SIZES[-1])
    buf = torch.empty(N_TIMED + 4096, dtype=torch.uint8, device="cuda:0")
    table = PfacTable.from_file(PAT, 256)
    with GpuMatcher(0, 1) as g:
        g.fill_tiled(buf, N_TIMED, para)
    o = Oracle(PAT, 1, 1)
    exp = {n: o.scan_spec(host[:n]) if n else (np.empty(0, np.int64), np.empty(0, np.int32)) for n in SIZES}
    o.close()
    return buf, table, exp


def matcher(table, n_slots, shared=True):
    g = GpuMatcher(0, n_slots)
    if shared:
        for s in range(1, n_slots):
            g.set_stream(s, g.stream_handle(0))
    g.load_table(table)
    for s in range(n_slots):
        g.reserve(s, 0, N_TIMED // 8)
    return g


def check(g, table, exp, n, slot, records=True):
    cnt, over = g.scan_finish(slot)
    pos, ids = exp[n]
    assert not over and cnt == pos.size, (n, slot, cnt, pos.size)
    if records and n < (1 << 20):
        rec = g.records_to_host(cnt, slot=slot)
        assert (rec["pos"].astype(np.int64) == pos).all() and (table.idmap[rec["state"]] == ids).all(), (n, slot)


def test_back_to_back_scans_on_a_shared_stream(world):
    """Two slots on one stream, 200 alternating scans of sizes drawn from SIZES, each finished one scan behind the
    launches (as bench.py does): every count exact, the records of every scan below 1 MiB the oracle's."""
    buf, table, exp = world
    rng = np.random.default_rng(20261019)
    seq = [SIZES[i] for i in rng.integers(0, len(SIZES), 200)]
    seq[:len(SIZES)] = SIZES                              # every size at least once, ...
    seq[-2:] = [SIZES[-1], 0]                             # ... and an empty scan finished last, behind a long one
    with matcher(table, 2) as g:
        inflight = []
        for k, n in enumerate(seq):
            g.scan_async(n, n, d_input=buf, slot=k & 1)
            inflight.append((k & 1, n))
            if len(inflight) == 2:
                sl, m = inflight.pop(0)
                check(g, table, exp, m, sl)
        for sl, m in inflight:
            check(g, table, exp, m, sl)


def test_immediate_reuse_of_one_slot(world):
    """200 rounds of scan_async -> scan_finish -> scan_async on one slot, the size changing every time: the count of
    every round is its own, so DONE is cleared per scan and never read from the scan before."""
    buf, table, exp = world
    rng = np.random.default_rng(7)
    with matcher(table, 1) as g:
        last = None
        for _ in range(200):
            n = SIZES[int(rng.integers(0, len(SIZES)))]
            if n == last:
                n = SIZES[(SIZES.index(n) + 1) % len(SIZES)]
            last = n
            g.scan_async(n, n, d_input=buf)
            check(g, table, exp, n, 0, records=False)


@pytest.mark.parametrize("shared", [True, False])
def test_finishing_out_of_order(shared, world):
    """Both scans enqueued, slot 1 finished before slot 0 (on one stream slot 1's scan runs behind slot 0's long one)."""
    buf, table, exp = world
    big, small = SIZES[-1], SIZES[3]
    with matcher(table, 2, shared) as g:
        for _ in range(4):
            g.scan_async(big, big, d_input=buf, slot=0)
            g.scan_async(small, small, d_input=buf, slot=1)
            check(g, table, exp, small, 1)
            check(g, table, exp, big, 0)


def timed_scan(g, buf, st):
    """elapsed_ms of one 64 MiB scan on torch stream st, its count, and the time between two torch events around it."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    g.scan_async(N_TIMED, N_TIMED, d_input=buf)
    e1.record(st)
    cnt, _ = g.scan_finish(0)
    ms = g.elapsed_ms(0)
    e1.synchronize()
    return ms, cnt, e0.elapsed_time(e1)


def elapsed_figures(buf, table):
    import torch
    st = torch.cuda.Stream()
    with GpuMatcher(0, 1) as g:
        g.set_stream(0, st.cuda_stream)
        g.load_table(table)
        g.reserve(0, 0, N_TIMED // 8)
        g.scan_resident(N_TIMED, N_TIMED, d_input=buf)    # (the first launch on a fresh context is not the one to time)
        ms, cnt, bracket = timed_scan(g, buf, st)
        g.scan_async(0, 0, d_input=buf)
        g.scan_finish(0)
        empty = g.elapsed_ms(0)
    return {"elapsed_ms": ms, "bracket_ms": bracket, "empty_ms": empty, "count": cnt}


def check_elapsed(f, count):
    print(f)
    assert f["count"] == count
    assert f["elapsed_ms"] >= N_TIMED / PEAK_BYTES_PER_MS, f      # 64 MiB at 8 TB/s: 8.4 us
    assert f["elapsed_ms"] <= f["bracket_ms"], f                  # the kernel lies inside its own dispatch
    assert f["empty_ms"] == 0, f


@pytest.fixture(scope="module")
def timed_count(world):
    buf = world[0]
    return ac_whole_shard(PAT, buf[:N_TIMED].cpu().numpy())[0]


def test_elapsed_ms_bounds(world, timed_count):
    """The kernel's own clock: no shorter than 64 MiB take at the HBM peak, no longer than the time between two events
    recorded around the launch on its stream; an empty scan takes no time."""
    buf, table, _ = world
    check_elapsed(elapsed_figures(buf, table), timed_count)


def test_elapsed_ms_bounds_with_event_timing(timed_count):
    """PFAC_EVENT_TIMING=1 (read when a context is created: a fresh process) puts the events back on the dispatch; the
    same bounds hold for their figure."""
    env = dict(os.environ, PFAC_ENABLE_KNOBS="1", PFAC_EVENT_TIMING="1")
    flags = ["-s"] if sys.flags.no_user_site else []
    out = subprocess.run([sys.executable, *flags, os.path.abspath(__file__)], env=env, check=True, capture_output=True,
                         text=True, timeout=300).stdout
    check_elapsed(json.loads(out.strip().splitlines()[-1]), timed_count)


def test_stream_swap_behind_a_finished_and_an_unfinished_scan(world):
    """set_stream after a finished scan, with an unfinished one that is then finished, and with an unfinished one that the
    next scan follows at once: the next scan's records are the oracle's every time."""
    import torch
    buf, table, exp = world
    streams = [torch.cuda.Stream() for _ in range(3)]
    big, small = SIZES[-1], SIZES[5]
    with matcher(table, 1) as g:
        g.scan_async(big, big, d_input=buf)
        check(g, table, exp, big, 0)
        g.set_stream(0, streams[0].cuda_stream)           # behind a finished scan
        g.scan_async(small, small, d_input=buf)
        check(g, table, exp, small, 0)
        g.scan_async(big, big, d_input=buf)
        g.set_stream(0, streams[1].cuda_stream)           # behind an unfinished one, ...
        check(g, table, exp, big, 0)                      # ... which still finishes with its own count
        g.scan_async(small, small, d_input=buf)
        check(g, table, exp, small, 0)
        g.scan_async(big, big, d_input=buf)
        g.set_stream(0, streams[2].cuda_stream)           # ... and one that is never finished
        g.scan_async(SIZES[4], SIZES[4], d_input=buf)
        check(g, table, exp, SIZES[4], 0)
        g.set_stream(0, 0)                                # back to the slot's own stream
        g.scan_async(small, small, d_input=buf)
        check(g, table, exp, small, 0)


if __name__ == "__main__":
    import torch
    para, _ = host_text(1)
    buf = torch.empty(N_TIMED + 4096, dtype=torch.uint8, device="cuda:0")
    table = PfacTable.from_file(PAT, 256)
    with GpuMatcher(0, 1) as g:
        g.fill_tiled(buf, N_TIMED, para)
    print(json.dumps(elapsed_figures(buf, table)))
