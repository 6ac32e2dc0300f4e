"""How the scan hands out its tiles and how it ends: every workgroup takes batches of NC tiles (one per compute wave) by
ticket from TICKET_WAYS counters, the last batch is partial, and the last workgroup to leave reports the totals.  Every
tile must be scanned exactly once at every size around those edges, under every ticket-counter count and kernel kind,
and back to back on one stream, where each scan zeroes the other slot's control header (GPU tests, -m gpu on an
MI355X)."""
import functools
import os

import numpy as np
import pytest

from orc import Oracle, ac_whole_shard
from phfpfac_amd import GpuMatcher, PfacTable

pytestmark = pytest.mark.gpu

NC = 15                     # compute waves per workgroup of the headline kernel (tables in LDS)
TILE = 4096
N_BIG = 1 << 30


def sizes(grid):
    """Byte sizes at the edges of the dispensing: one tile, one batch (NC tiles) +- 1, one round of the whole grid
    (grid * NC tiles, one batch per workgroup) +- 1, two rounds +- 1, and ragged last tiles."""
    tiles = [1, NC - 1, NC, NC + 1, grid * NC - 1, grid * NC, grid * NC + 1, 2 * grid * NC - 1, 2 * grid * NC, 2 * grid * NC + 1]
    return [t * TILE for t in tiles] + [1, 3 * TILE + 1, (grid * NC + 7) * TILE + 123, (2 * grid * NC + 5) * TILE - 1000]


@functools.lru_cache(maxsize=None)
def host_text(n, para):
    reps = n // len(para) + 1
    return np.frombuffer(para * reps, dtype=np.uint8)[:n].copy()


def check_scan(g, pat, idmap, host, n, slot=0, records=False, expect=None):
    """Finish the slot's scan of n bytes and compare (count, checksum) with one serial Aho-Corasick pass over
    the same bytes; small scans also record by record with the oracle's PFAC walk."""
    cnt, over = g.scan_finish(slot)
    assert not over
    chk = g.checksum(cnt, slot=slot)
    exp = expect if expect is not None else ac_whole_shard(pat, host[:n])
    assert (cnt, chk) == exp, (n, cnt, chk, exp)
    if records:
        o = Oracle(pat, 1, 1)
        pos, ids = o.scan_spec(host[:n])
        o.close()
        rec = g.records_to_host(cnt, slot=slot)
        assert (rec["pos"].astype(np.int64) == pos).all() and (idmap[rec["state"]] == ids).all(), n
    return cnt


def run_sizes(g, table, buf, pat, host, sz):
    for n in sz:
        g.scan_async(n, n, d_input=buf)
        check_scan(g, pat, table.idmap, host, n, records=n <= (1 << 20))


@pytest.fixture(scope="module")
def text_buf():
    import torch
    para = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data", "paragraph402"), "rb").read()
    n = 2 * 256 * NC * TILE + 64 * TILE                  # every size of sizes() on a chip of up to 256 CUs
    buf = torch.empty(N_BIG + 4096, dtype=torch.uint8, device="cuda:0")
    return buf, para, host_text(n, para)


def fresh(table, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = GpuMatcher(0, 1)
    g.load_table(table)                                   # knobs are read when a table is installed
    return g


@pytest.mark.parametrize("ways", ["1", "2", "4"])
def test_every_tile_once_at_the_dispensing_edges(ways, text_buf, resolve, monkeypatch):
    """The headline kernel (tables in LDS) at 1 tile, NC +- 1 tiles, grid*NC and 2*grid*NC +- 1 tile and ragged last
    tiles, under 1, 2 and 4 ticket counters."""
    buf, para, host = text_buf
    pat = resolve("experimentpattern")
    table = PfacTable.from_file(pat, 256)
    g = fresh(table, monkeypatch, {"PFAC_TICKET_WAYS": ways})
    try:
        assert g.info()["variant"] == "tables_in_lds"
        sz = sizes(g.info()["grid_blocks"])
        g.fill_tiled(buf, host.size, para)
        g.reserve(0, 0, host.size // 4)
        run_sizes(g, table, buf, pat, host, sz)
    finally:
        g.close()


@pytest.mark.parametrize("env,patname", [({"PFAC_FORCE_L2": "1"}, "experimentpattern"),
                                         ({"PFAC_DENSE": "1"}, "experimentpattern"),
                                         ({"PFAC_FORCE_L2": "1", "PFAC_DENSE": "1"}, "xaa+xab+xac+xad"),
                                         ({"PFAC_FORCE_L2": "1", "PFAC_DENSE": "1", "PFAC_NO_DENSE2": "1"}, "xaa+xab+xac+xad"),
                                         ({"PFAC_LAG": "1"}, "experimentpattern")])
def test_every_tile_once_in_the_other_kernels(env, patname, text_buf, resolve, monkeypatch):
    """The same edges through the L2-table kernel, dense mode (both forms, with the dictionary) and the two-buffer
    layout: their compute-wave counts differ, so the batch boundaries fall elsewhere in the tile space."""
    buf, para, host = text_buf
    pat = resolve(patname)
    table = PfacTable.from_file(pat, 256)
    g = fresh(table, monkeypatch, env)
    try:
        sz = sizes(g.info()["grid_blocks"])
        g.fill_tiled(buf, host.size, para)
        g.reserve(0, 0, host.size // 2)
        run_sizes(g, table, buf, pat, host, [n for n in sz if n <= 2 * host.size // 3] + [host.size])
    finally:
        g.close()


def test_large_scans_count_and_checksum(text_buf, resolve):
    """64 MiB and 1 GiB of the tiled text (the headline's size): the whole shard's count and checksum."""
    buf, para, _ = text_buf
    pat = resolve("experimentpattern")
    table = PfacTable.from_file(pat, 256)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        g.fill_tiled(buf, N_BIG, para)
        g.reserve(0, 0, N_BIG // 8)
        for n in (64 << 20, N_BIG):
            g.scan_resident(n, n, d_input=buf)
            host = buf[:n].cpu().numpy()
            g.scan_async(n, n, d_input=buf)
            check_scan(g, pat, table.idmap, host, n)
            del host


def test_two_slots_back_to_back_alternating_sizes(text_buf, resolve):
    """Two slots on ONE stream, the next scan enqueued while the last runs, sizes alternating between large and small
    (and across the batch and round edges): each scan zeroes the other slot's control header for its next scan."""
    buf, para, host = text_buf
    pat = resolve("experimentpattern")
    table = PfacTable.from_file(pat, 256)
    with GpuMatcher(0, 2) as g:
        g.set_stream(1, g.stream_handle(0))
        g.load_table(table)
        g.fill_tiled(buf, host.size, para)
        g.reserve(0, 0, host.size // 4)
        g.reserve(1, 0, host.size // 4)
        sz = sizes(g.info()["grid_blocks"])
        big = host.size - 3 * TILE - 5
        seq = [x for n in sz for x in (big, n)] + [big, big, 1, 1]
        exp = {n: ac_whole_shard(pat, host[:n]) for n in set(seq)}
        inflight = []
        for k, n in enumerate(seq):
            g.scan_async(n, n, d_input=buf, slot=k & 1)
            inflight.append((k & 1, n))
            if len(inflight) == 2:
                sl, m = inflight.pop(0)
                check_scan(g, pat, table.idmap, host, m, slot=sl, expect=exp[m])
        for sl, m in inflight:
            check_scan(g, pat, table.idmap, host, m, slot=sl, expect=exp[m])
