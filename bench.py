#!/usr/bin/env python3
"""bench.py -- input GB/s scanned by the PFAC hot path on N MI355X (BASELINE.json's metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload NAME] [--bytes-per-gpu B] [--dump-outputs DIR] [--full]

N > 1 works from a bare command line (the parent spawns one fresh process per GPU before anything touches a GPU) and
under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` (RANK/LOCAL_RANK/WORLD_SIZE are
then already set and nothing is spawned).

A "step" is one pass of the hot path over one batch of synthetic input that is ALREADY RESIDENT in HBM: run the scan
kernel over this rank's shard (owned bytes + max_pat_len-1 bytes of halo) and read back the exact match count.  With
N > 1 the per-rank counts of the K steps are all-gathered once, inside the timed region (the one exchange the sharded
path needs).  Weak scaling: every rank owns the same number of bytes (default 1 GiB at N = 1 = BASELINE.json
configs[1]; 4 GiB per GPU at N > 1 = configs[3]'s shard size).  Workload = pattern file `experimentpattern`, input =
the reference's `1M` text (402-byte period) tiled to the shard size, 1 stream per GPU, PHF width 256.  Rank 0 builds
the table on the host (C) and broadcasts its image with RCCL.

Before the W warm-up steps an untimed settling phase scans (64 to 192 launches) until eight consecutive launches agree
within 1.5 % and sit within 2 % of the fastest launch seen (a cold GPU's first launches run up to 20 % slower while the
clocks ramp, with intermediate plateaus); its length and the cold figure are reported in `config` (`settle_launches`,
`cold_first20_gbs`).  On the headline workload the sustained run (below) follows, still untimed, and the W + K steps come
after it: on some boxes the governor needs longer than the settling launches, and the K timed steps should see the clock
state a long job runs in, not the tail of the ramp.

A plain run does only what the headline figure needs: set up (table, resident input, record buffers, and the settling
launches and sustained run that bring the card to the clock state the steps are timed in), the W warm-up and K timed
steps, --dump-outputs if given, and the JSON line with `value`, `ms_per_step`, `roofline` (from the timed steps' own HIP
events) and `sustained`.  --full adds everything else, each part outside the timed region: the parity check, the consumer
costs (`config.*_ms`), `other_workloads`, `end_to_end` and the CPU baselines; --no-extra, --no-end-to-end,
--no-cpu-baseline and --cpu-threads trim a --full run.

Parity (--full), outside the timed region, for EVERY workload timed and on every rank: the GPU's (match count, record
checksum) of the whole resident shard == one serial Aho-Corasick pass over the bytes copied back from HBM (tests/orc.py:
ac_whole_shard), plus the records of the first 1 MiB one by one, in order, against the oracle's PFAC walk.

--dump-outputs DIR writes, after the timed steps, what the last of them computed: its match count, the checksum of all its
records and a seeded sample of the records, as float64 .npy files (dump_outputs, at most 24 MiB).  The inputs are the same
from run to run, so the files of two builds can be compared one for one.

One JSON line is printed by rank 0 (contract in the task statement) with extra objects:
  roofline         algorithmic bytes (1 B per input byte) / kernel time measured with HIP events on the stream the kernel
                   runs on, against the 8 TB/s HBM3E peak; `traffic` = HBM bytes per launch from the committed rocprofv3
                   PMC passes when they were taken from this very kernel source (else null), `traffic_model` = input +
                   records + tile index bytes computed from this run
  sustained        the same scan back to back for --sustain-seconds (default 2.5 s, ~11 000 launches): mean / p5 / p50 / p95 of
                   the per-launch kernel rate and the wall-clock rate -- what a long job sees, next to the K-step `value`
                   (run before the W + K steps, see above)
  end_to_end       (--full) BASELINE configs[2], PCIe inclusive: 4 GiB in pinned host memory -> four slots on four streams
                   (hipMemcpyAsync H2D || scan) -> counts (N = 1 only; never reported as `value`)
  config.*_ms      (--full) what an ordered / host / text consumer pays on top of the scan, each outside the timed region: expand_ms
                   (heap -> sorted 8-byte records on the device), readback_ms (compact form D2H), emit_text_ms (GPU-side text
                   emitter), gather_ms (N > 1: compact records to rank 0 over RCCL)
  cpu_baseline     (--full) serial Aho-Corasick (oracle/ac_serial.c, the CHECKER, kind "port") on ONE host core, bounded sample;
                   cpu_baseline_pfac (the oracle's PFAC-on-CPU walk, one core) and cpu_baseline_threads (serial AC on
                   all the cores this process may use) next to it (N = 1 only)
  other_workloads  (--full) short passes of the other BASELINE configurations' pattern sets / inputs (N = 1 only)
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

DATA = os.path.join(REPO, "tests", "golden", "data")
KERNEL_SRC = os.path.join(REPO, "phfpfac_amd", "csrc", "pfac_hip.hip")
PROFILE = os.path.join(REPO, "profiles", "r3_pmc_per_launch.json")
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
GIB = 1 << 30
DUMP_RECORDS = 1 << 20         # --dump-outputs: records sampled from the last timed step, over all ranks (24 MiB as float64)
DUMP_WINDOW = 1 << 14          # ... in windows of this many consecutive records
DUMP_SEED = 0x44554D50

WORKLOADS = {
    # name: (pattern fixture, input kind, description)
    "text1g_experimentpattern": ("experimentpattern", "text", "experimentpattern (4 patterns) x reference 1M text tiled to {size}/GPU"),
    "text1g_bytefile10000": ("bytefile_10000byte", "text", "bytefile/10000byte (1376 patterns) x reference 1M text tiled to {size}/GPU"),
    "rand1g_experimentpattern": ("experimentpattern", "rand", "experimentpattern x splitmix64 random bytes, {size}/GPU"),
    "text1g_dictionary": ("xaa+xab+xac+xad", "text", "7989-word dictionary (xaa..xad) x reference 1M text tiled to {size}/GPU"),
    "rand1g_snort75k": ("bytefile_1000000byte.gz", "rand", "bytefile/1000000byte (75840 patterns, 542732 states, tables via L2) x splitmix64 random bytes, {size}/GPU"),
    "text1g_snort75k": ("bytefile_1000000byte.gz", "text", "bytefile/1000000byte (75840 patterns, 542732 states, tables via L2) x reference 1M text tiled to {size}/GPU"),
}
HEADLINE = "text1g_experimentpattern"


def spawn_ranks(n, argv, extra_env=None):
    """Run `argv` as n fresh child processes, one per GPU, with the torch.distributed environment of a single node
    (RANK, LOCAL_RANK, WORLD_SIZE, MASTER_ADDR=127.0.0.1, a free MASTER_PORT).  The parent never touches a GPU.
    Rank 0's stdout is passed through; returns the worst exit code."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for rank in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(n), "MASTER_ADDR": "127.0.0.1",
                    "MASTER_PORT": str(port), "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")})
        env.update(extra_env or {})
        procs.append(subprocess.Popen(argv, env=env, stdout=None if rank == 0 else subprocess.DEVNULL))
    worst = 0
    for p in procs:
        rc = p.wait()
        worst = worst or rc
    return worst


def pattern_path(name, tmpdir):
    if name.endswith(".gz"):
        import gzip
        p = os.path.join(tmpdir, name[:-3])
        with gzip.open(os.path.join(DATA, name), "rb") as g, open(p, "wb") as f:
            f.write(g.read())
        return p
    if "+" not in name:
        return os.path.join(DATA, name)
    p = os.path.join(tmpdir, "all.pat")
    with open(p, "wb") as f:
        for part in name.split("+"):
            f.write(open(os.path.join(DATA, part), "rb").read())
    return p


def usable_cores():
    try:
        return len(os.sched_getaffinity(0))
    except AttributeError:
        return os.cpu_count() or 1


def cpu_baseline_threads(pat_path, kind, para, n_threads, seconds=6.0):
    """The same serial Aho-Corasick scan on n_threads host threads, each over its own 32 MiB slice (plus halo) of
    the workload, repeated for a few seconds -- the all-cores figure next to the one-core baseline."""
    import ctypes as C
    import threading
    from orc import Oracle, lib
    from phfpfac_amd.matcher import splitmix64_bytes, tiled_bytes
    L = lib()
    o = Oracle(pat_path, 1, 1)
    ac = L.ac_build(o.m)
    piece = 32 << 20
    buf = tiled_bytes(piece + 1024, para) if kind == "text" else splitmix64_bytes(piece + 1024, 0x5048465046414331)
    done = [0] * n_threads
    stop = time.perf_counter() + seconds

    def work(i):
        chk = C.c_uint64(0)
        while time.perf_counter() < stop:
            L.ac_scan_count(ac, buf.ctypes.data, piece, C.byref(chk))      # ctypes releases the GIL during the call
            done[i] += 1

    t0 = time.perf_counter()
    th = [threading.Thread(target=work, args=(i,)) for i in range(n_threads)]
    [t.start() for t in th]
    [t.join() for t in th]
    dt = time.perf_counter() - t0
    L.ac_free(ac)
    o.close()
    return {"value": round(sum(done) * piece / dt / 1e9, 3), "unit": "GB/s", "cores": n_threads, "kind": "port",
            "sample": f"{sum(done)} scans of a 32 MiB slice on {n_threads} threads ({dt:.1f} s), serial Aho-Corasick full-DFA per thread"}


def cpu_baseline(pat_path, kind, para, seconds=10.0):
    """Serial Aho-Corasick on ONE host core over a bounded sample of the same workload."""
    import ctypes as C
    from orc import Oracle, lib
    from phfpfac_amd.matcher import splitmix64_bytes, tiled_bytes
    L = lib()
    o = Oracle(pat_path, 1, 1)
    ac = L.ac_build(o.m)
    sample = 256 << 20
    buf = tiled_bytes(sample, para) if kind == "text" else splitmix64_bytes(sample, 0x5048465046414331)
    chk = C.c_uint64(0)
    L.ac_scan_count(ac, buf.ctypes.data, 1 << 20, C.byref(chk))          # warm the DFA
    passes, t0, matches = 0, time.perf_counter(), 0
    while True:
        matches = L.ac_scan_count(ac, buf.ctypes.data, sample, C.byref(chk))
        passes += 1
        dt = time.perf_counter() - t0
        if dt >= seconds or passes >= 64:
            break
    L.ac_free(ac)
    o.close()
    gbs = passes * sample / dt / 1e9
    return {"value": round(gbs, 4), "unit": "GB/s", "cores": 1, "kind": "port",
            "sample": f"{passes} pass(es) over the first 256 MiB of the workload ({dt:.1f} s), serial Aho-Corasick "
                      f"full-DFA, {matches} matches/pass; host has {os.cpu_count()} logical cores"}


def cpu_baseline_pfac(pat_path, kind, para, seconds=6.0):
    """BASELINE.md's second CPU figure: PFAC itself on one core -- the oracle's walk from every start offset over the
    dense trie (the bit-exact emitter the GPU records are checked against)."""
    from orc import Oracle
    from phfpfac_amd.matcher import splitmix64_bytes, tiled_bytes
    o = Oracle(pat_path, 1, 1)
    sample = 32 << 20
    buf = tiled_bytes(sample, para) if kind == "text" else splitmix64_bytes(sample, 0x5048465046414331)
    passes, t0, n = 0, time.perf_counter(), 0
    while True:
        pos, _ = o.scan_spec(buf, None)
        n = int(pos.size)
        passes += 1
        dt = time.perf_counter() - t0
        if dt >= seconds or passes >= 64:
            break
    o.close()
    return {"value": round(passes * sample / dt / 1e9, 4), "unit": "GB/s", "cores": 1, "kind": "port",
            "sample": f"{passes} pass(es) over the first 32 MiB of the workload ({dt:.1f} s), PFAC walk from every offset "
                      f"over the dense trie (oracle/pfac_oracle.c), records materialised, {n} matches/pass"}


def config3_end_to_end(ppath, para, local_rank, chunk=GIB, k_slots=4):
    """BASELINE configs[2] on one GPU, PCIe INCLUSIVE (reported next to the kernel-resident value, never as it): 4 GiB
    of the text workload in pinned host memory -> four pipeline slots on four HIP streams (hipMemcpyAsync H2D || scan) ->
    exact counts.  Everything is enqueued before anything is waited for; the clock runs from the first H2D call to the
    last count.  The total is checked against the input's period (oracle over a few periods, as the -m gpu test does)."""
    import numpy as np
    import torch
    from orc import Oracle
    from phfpfac_amd import GpuMatcher, PfacTable
    from phfpfac_amd.matcher import tiled_bytes
    table = PfacTable.from_file(ppath, 256)
    n_total = chunk * k_slots
    period = len(para)
    host = torch.empty(chunk + period + table.halo + 64, dtype=torch.uint8).pin_memory()
    host.numpy()[:] = tiled_bytes(host.numel(), para)
    hv = host.numpy()
    o = Oracle(ppath, 1, 1)
    pos, _ = o.scan_spec(tiled_bytes(period * 8, para), None)
    per_period = int(((pos >= period) & (pos < 2 * period)).sum())
    full, tail = divmod(n_total, period)
    lpos, _ = o.scan_spec(tiled_bytes(tail, para), None)
    o.close()
    expect = per_period * full + int(lpos.size)
    best, counts = None, []
    with GpuMatcher(local_rank, k_slots) as g:
        g.load_table(table)
        for s in range(k_slots):
            g.reserve(s, chunk + table.halo, chunk // 8)
        for rep in range(3):                       # first pass warms buffers and clocks; best of the other two
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(k_slots):
                lo = s * chunk
                n_avail = min(n_total, lo + chunk + table.halo) - lo
                ph = lo % period
                g.h2d(hv[ph: ph + n_avail], slot=s)
                g.scan_async(chunk, n_avail, slot=s)
            counts = [g.scan_finish(s)[0] for s in range(k_slots)]
            dt = time.perf_counter() - t0
            if rep and (best is None or dt < best):
                best = dt
        kern = sum(g.elapsed_ms(s) for s in range(k_slots))
    if sum(counts) != expect:
        raise SystemExit(f"config-3 end-to-end run: {sum(counts)} matches, expected {expect}")
    return {"value": round(n_total / best / 1e9, 2), "unit": "GB/s", "bytes": n_total, "ms": round(best * 1e3, 2),
            "slots": k_slots, "streams": k_slots, "kernel_ms_sum": round(kern, 3), "matches": sum(counts),
            "note": "PCIe-inclusive (H2D from pinned host memory || scan, counts read back); bound by the host link, "
                    "reported beside the HBM-resident value, never as it"}


def committed_traffic():
    """HBM bytes per headline launch from the committed rocprofv3 --pmc passes -- only when they were taken from this
    very kernel source (tools/summarize_prof.py stores its sha256)."""
    try:
        prof = json.load(open(PROFILE))
        src = hashlib.sha256(open(KERNEL_SRC, "rb").read()).hexdigest()
        if prof.get("kernel_source_sha256") == src:
            return prof.get("derived_hbm_bytes"), "rocprofv3 --pmc FETCH_SIZE x2 (gfx950 correction) + WRITE_SIZE per launch, profiles/r3_pmc_per_launch.json (same kernel source)"
        return None, "profiles/r3_pmc_per_launch.json was taken from a different kernel source: not reported"
    except (OSError, ValueError):
        return None, "no committed PMC profile"


def dump_outputs(out_dir, g, table, slot, n, base, rank, world):
    """--dump-outputs: what the last timed step computed, as a caller of the scan receives it, as float64 .npy files in
    `out_dir` (suffix _rank<r> when N > 1): match_count, records_checksum (the order-independent checksum of ALL its
    records with global positions, low and high 32 bits) and a fixed sample of the records in output order -- windows of
    DUMP_WINDOW consecutive records, the first and the last always included, the others drawn with DUMP_SEED -- as
    record_index, record_pos (global start position) and record_pattern_id."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    sfx = "" if world == 1 else "_rank%d" % rank
    chk = g.checksum(n, base=base, slot=slot)
    idx, pos, pid = [], [], []
    if n:
        n_blocks = -(-n // DUMP_WINDOW)
        want = max(DUMP_RECORDS // world // DUMP_WINDOW, 2)
        rest = np.arange(1, n_blocks - 1)
        pick = np.random.default_rng(DUMP_SEED).choice(rest, size=min(want - 2, rest.size), replace=False)
        for b in np.unique(np.concatenate([[0, n_blocks - 1], pick])):
            first = int(b) * DUMP_WINDOW
            rec = g.records_to_host(min(DUMP_WINDOW, n - first), slot=slot, first=first)
            idx.append(np.arange(first, first + rec.size))
            pos.append(rec["pos"].astype(np.int64) + base)
            pid.append(table.idmap[rec["state"]])
    cat = lambda parts: np.concatenate(parts or [np.empty(0)]).astype(np.float64)      # noqa: E731
    arrays = {"match_count": np.array([n], dtype=np.float64),
              "records_checksum": np.array([chk & 0xFFFFFFFF, chk >> 32], dtype=np.float64),
              "record_index": cat(idx), "record_pos": cat(pos), "record_pattern_id": cat(pid)}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + sfx + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default=HEADLINE, choices=sorted(WORKLOADS))
    ap.add_argument("--bytes-per-gpu", type=int, default=0, help="default: 1 GiB at --gpus 1, 4 GiB per GPU otherwise")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: parity, consumer costs, other workloads, end to end, CPU baselines")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baselines")
    ap.add_argument("--extra", action="store_true", help="(default of --full at --gpus 1) also time the other workloads (short)")
    ap.add_argument("--no-extra", action="store_true", help="--full without the other workloads")
    ap.add_argument("--sustain-seconds", type=float, default=2.5, help="length of the sustained back-to-back run reported beside the K-step value (0: skip)")
    ap.add_argument("--no-end-to-end", action="store_true", help="--full without the PCIe-inclusive config-3 run (4 GiB pinned host -> 4 slots)")
    ap.add_argument("--cpu-threads", type=int, default=-1, help="threads of the --full all-cores CPU baseline (default: usable cores, at most 32; 0: skip)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (float64, see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1 and args.gpus > 1:
        # bare `python bench.py --gpus N`: one fresh process per GPU, started before this one has touched a GPU
        sys.exit(spawn_ranks(args.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]))
    if os.environ.get("PFAC_BENCH_SPAWN_TEST"):            # tests/test_dist_cpu.py: the spawner alone, no GPU
        me = {"rank": os.environ["RANK"], "local_rank": os.environ["LOCAL_RANK"], "world": os.environ["WORLD_SIZE"],
              "master": os.environ["MASTER_ADDR"] + ":" + os.environ["MASTER_PORT"], "argv": sys.argv[1:]}
        with open(os.path.join(os.environ["PFAC_BENCH_SPAWN_TEST"], "rank%s.json" % me["rank"]), "w") as f:
            json.dump(me, f)
        print(json.dumps(me), flush=True)
        return

    import numpy as np
    import torch
    from phfpfac_amd import GpuMatcher, PfacTable
    from phfpfac_amd import dist as pdist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU: the PFAC scan has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # PFAC_BENCH_FORCE_DIST=1 runs the RCCL code path (table broadcast, count all-gather, record gather) even with one rank
    use_dist = world > 1 or os.environ.get("PFAC_BENCH_FORCE_DIST") == "1"
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    import tempfile
    tmpdir = tempfile.mkdtemp()
    para = open(os.path.join(DATA, "paragraph402"), "rb").read()
    per = args.bytes_per_gpu or (GIB if world == 1 else 4 * GIB)
    n_total = per * world

    sustain_s = args.sustain_seconds if world == 1 else min(args.sustain_seconds, 1.0)

    def run_workload(name, steps, warmup, headline):
        pat_name, kind, desc = WORKLOADS[name]
        desc = desc.format(size=("%d GiB" % (per >> 30)) if per % GIB == 0 else ("%d bytes" % per))
        ppath = pattern_path(pat_name, tmpdir)
        g = GpuMatcher(local_rank, 2)          # two buffer sets (slots) ...
        g.set_stream(1, g.stream_handle(0))    # ... on ONE HIP stream: step k+1 is enqueued while step k runs
        if use_dist:
            table = PfacTable.from_file(ppath, 256) if rank == 0 else None
            blob, table = pdist.broadcast_table(table, dev, 0)             # RCCL broadcast of the table image
            torch.cuda.synchronize()
            g.load_table_device(blob, blob.numel(), 0, host_table=table)
        else:
            table = PfacTable.from_file(ppath, 256)
            g.load_table(table)
        lo, hi, end = pdist.shard_read_range(n_total, rank, world, table.halo)
        n_owned, n_avail = hi - lo, end - lo
        buf = torch.empty(n_avail + 4096, dtype=torch.uint8, device=dev)
        if kind == "text":
            g.fill_tiled(buf, n_avail, para, phase=lo % len(para))
        else:
            g.fill_random(buf, (n_avail + 7) // 8 * 8, 0x5048465046414331 + lo // 8)
        cap = max(n_owned // 8, 1 << 20)
        g.reserve(0, 0, cap)
        n = g.scan_resident(n_owned, n_avail, d_input=buf)                 # sizes the record heap, warms up
        _, _, used = g.scan_format(0)
        g.reserve(1, 0, max(cap, used + used // 8))
        assert g.scan_resident(n_owned, n_avail, d_input=buf, slot=1) == n
        t_par = None
        if args.full:
            # Parity (outside the timed region), on the FULL-SIZE launch itself: the GPU's (match count, order-independent
            # record checksum) of the WHOLE shard against one serial Aho-Corasick pass (oracle/ac_serial.c, the CHECKER) over
            # the very bytes the kernel read, copied back from HBM -- every record of the shard enters the comparison.  The
            # checksum cannot see order, so the records of the first 1 MiB are also compared one by one, in order, with the
            # oracle's PFAC walk (in (position, length) order they are a prefix of the record sequence).
            from orc import Oracle, ac_whole_shard
            chk = g.checksum(n, base=lo, slot=1)
            host = buf[:n_avail].cpu().numpy()
            t_par = time.perf_counter()
            cnt_o, chk_o = ac_whole_shard(ppath, host, n_owned=n_owned, base=lo)
            t_par = time.perf_counter() - t_par
            if (n, chk) != (cnt_o, chk_o):
                raise SystemExit(f"rank {rank}: PARITY FAILURE on workload {name}: GPU (count, checksum) = ({n}, {chk:#x}), "
                                 f"serial Aho-Corasick over the same {n_avail} bytes = ({cnt_o}, {chk_o:#x})")
            m = min(1 << 20, n_owned)
            o = Oracle(ppath, 1, 1)
            opos, oids = o.scan_spec(host[: min(n_avail, m + table.halo)], None)
            keep = opos < m
            opos, oids = opos[keep], oids[keep]
            o.close()
            del host
            k = int(opos.size)
            rec = g.records_to_host(min(n, k + 1), slot=1)
            ok = n >= k and np.array_equal(rec["pos"][:k].astype(np.int64), opos) and \
                np.array_equal(table.idmap[rec["state"][:k]], oids) and (n == k or int(rec["pos"][k]) >= m)
            if not ok:
                raise SystemExit(f"rank {rank}: PARITY FAILURE on workload {name}: first {k} records differ from the oracle")

        pending = []
        inflight = []                          # slots with an enqueued, not yet finished scan (depth <= 2)
        kern_ms = []

        def finish_oldest():
            sl = inflight.pop(0)
            cnt, _ = g.scan_finish(sl)
            kern_ms.append(g.elapsed_ms(sl))
            pending.append(cnt)
            return cnt

        def step(k):
            """One pass of the hot path over the resident shard.  The launch of step k overlaps the run of step
            k-1 (same stream, alternate control/record buffers); every step's count is read back."""
            sl = k & 1
            g.scan_async(n_owned, n_avail, d_input=buf, slot=sl)
            inflight.append(sl)
            return finish_oldest() if len(inflight) == 2 else None

        def drain(exchange=True):
            cnt = None
            while inflight:
                cnt = finish_oldest()
            if use_dist and pending and exchange:
                # the one exchange the sharded path needs -- every rank learns every shard's match count of
                # every scan, i.e. where its records go in the global stream -- done once for the batch of scans
                mine = torch.tensor(pending, dtype=torch.int64, device=dev)
                allc = torch.empty(world * len(pending), dtype=torch.int64, device=dev)
                dist.all_gather_into_tensor(allc, mine)
                assert int(allc.view(world, -1)[rank, -1].item()) == pending[-1]
            pending.clear()
            return cnt

        # Clock settling (untimed, part of the setup): the first ~40 back-to-back launches on a cold GPU run up to 20 %
        # slower than the steady state -- the governor ramping (with intermediate plateaus), not the kernel.  Keep scanning
        # (at least 64, at most 192 launches) until eight consecutive launches agree within 1.5 % AND sit within 2 % of the
        # fastest launch seen, so that W warm-up + K timed steps measure the steady state a long-running job sees.
        # Both the number of launches and the cold figure go into the JSON.
        settle = 0
        while settle < 192:
            step(settle)
            settle += 1
            if settle >= 64 and len(kern_ms) >= 8:     # at least 64 launches (~20 ms): the ramp has intermediate plateaus
                last = kern_ms[-8:]
                if max(last) <= 1.015 * min(last) and float(np.mean(last)) <= 1.02 * min(kern_ms):
                    break
        drain(exchange=False)                  # (ranks settle after different numbers of launches: no collective here)
        cold_ms = float(np.mean(kern_ms[:20]))
        sus_ms = None
        if headline and sustain_s > 0:
            # SUSTAINED figure: back-to-back launches for >= sustain_s seconds (thousands of them), every launch timed by
            # its own HIP event pair -- what a long job sees.  It runs BEFORE the W + K steps: the card's governor needs
            # longer than the settling launches above on some boxes (intermediate plateaus of tens of milliseconds), and
            # the K timed steps should see the state a long job runs in, not the tail of the ramp
            kern_ms.clear()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            k = 0
            while time.perf_counter() - t1 < sustain_s:
                step(k)
                k += 1
            drain(exchange=False)
            sus_wall, sus_ms, sus_k = time.perf_counter() - t1, list(kern_ms), k      # (statistics after the timed steps: no idle gap here)
        for k in range(warmup):
            step(k)
        drain()
        kern_ms.clear()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            step(k)
        cnt = drain()                          # all K scans finished, every count exchange completed
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        dt = time.perf_counter() - t0
        if use_dist:
            t = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
            tot = torch.tensor([cnt], dtype=torch.int64, device=dev)
            dist.all_reduce(tot)
            cnt_all = int(tot.item())
        else:
            cnt_all = cnt
        if headline and args.dump_outputs:
            dump_outputs(args.dump_outputs, g, table, (steps - 1) & 1, cnt, lo, rank, world)
        res = {"name": name, "desc": desc, "ppath": ppath, "kind": kind, "dt": dt, "kernel_ms": float(np.mean(kern_ms)),
               "kernel_ms_min": float(np.min(kern_ms)), "matches": cnt_all, "matches_rank": cnt, "table": table,
               "n_owned": n_owned, "n_avail": n_avail, "settle": settle, "cold_ms": cold_ms, "parity_s": t_par}
        if sus_ms is not None:
            wall, k = sus_wall, sus_k
            gbs = n_owned / (np.array(sus_ms) * 1e-3) / 1e9
            sustained = {"seconds": round(wall, 2), "launches": k,
                         "kernel_gbs_mean": round(float(n_owned / (np.mean(sus_ms) * 1e-3) / 1e9), 1),
                         "kernel_gbs_p5": round(float(np.percentile(gbs, 5)), 1),
                         "kernel_gbs_p50": round(float(np.percentile(gbs, 50)), 1),
                         "kernel_gbs_p95": round(float(np.percentile(gbs, 95)), 1),
                         "wall_gbs": round(n_owned * k / wall / 1e9, 1),
                         "frac_of_hbm_peak_mean": round(float(n_owned / (np.mean(sus_ms) * 1e-3) / 1e9 / HBM_PEAK_GBS), 4),
                         "note": "back-to-back launches of the same resident shard, each timed by its HIP event pair; "
                                 "the card's power/clock state over seconds is part of this figure"}
            res["sustained"] = sustained
        if headline:
            rec_b, n_tiles, used = g.scan_format(1)
            res.update(rec_bytes=rec_b, heap_used=used, n_tiles=n_tiles)
        if headline and args.full:
            # What a consumer of ONE ordered record stream pays on top of the scan, reported next to the timed value:
            # heap -> sorted 8-byte records on the device (expand), and (N > 1) their ordered gather on rank 0.
            wide = torch.empty(max(cnt, 1), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            g.expand_records(cnt, wide, slot=1)
            g.sync(1)
            res["expand_ms"] = (time.perf_counter() - t1) * 1e3
            del wide
            # D2H of the compact form itself (heap words + tile index into pinned host memory): what the CLI's emitter
            # and any host consumer reads back -- the counterpart of the reference's dense D2H (master_kernel.cu:428)
            words_h = torch.empty(max(used * rec_b, 1), dtype=torch.uint8).pin_memory()
            tix_h = torch.empty(max(n_tiles, 1), dtype=torch.int64).pin_memory()
            for _ in range(2):                               # (first pass: pages the pinned buffers in)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                g.packed_to_host_into(words_h, tix_h, slot=1)
                res["readback_ms"] = (time.perf_counter() - t1) * 1e3
            res["readback_bytes"] = used * rec_b + n_tiles * 8
            del words_h, tix_h
            if world == 1:
                # the GPU-side text emitter (main.cc:335-350 on the device): the same records -> finished lines of
                # GPU_match_result.txt in a device buffer (size pass, prefix sum, format); twice: the first call allocates
                for _ in range(2):
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    res["emit_text_bytes"] = g.emit_text_device(lo, slot=1)
                    g.sync(1)
                    res["emit_text_ms"] = (time.perf_counter() - t1) * 1e3
            if use_dist:
                dist.barrier()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                parts = pdist.gather_packed(g, dev, slot=1, dst=0)          # the COMPACT form travels: 2 B (4 B) per match
                torch.cuda.synchronize()
                dist.barrier()
                res["gather_ms"] = (time.perf_counter() - t1) * 1e3
                if rank == 0:
                    res["gather_records"] = sum(p["n_matches"] for p in parts)
                    res["gather_bytes"] = sum(p["words"].numel() + 8 * p["tix"].numel() for p in parts)
                del parts
        res["info"] = g.info()
        g.close()
        del buf
        torch.cuda.empty_cache()
        return res

    res = run_workload(args.workload, args.steps, args.warmup, True)
    value = n_total * args.steps / res["dt"] / 1e9
    achieved = res["n_owned"] / (res["kernel_ms"] * 1e-3) / 1e9
    traffic, traffic_note = (None, "measured for the headline workload at 1 GiB only")
    if args.workload == HEADLINE and per == GIB:
        traffic, traffic_note = committed_traffic()
    rec_bytes = res["rec_bytes"]
    out = {
        "metric": "input GB/s scanned", "value": round(value, 2), "unit": "GB/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(res["dt"] / args.steps * 1e3, 4),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": res["desc"], "bytes_per_gpu": per, "global_bytes": n_total, "streams_per_gpu": 1, "launch_pipeline_depth": 2,
                   "phf_width": 256, "patterns": res["table"].n_patterns, "states": res["table"].state_num,
                   "kernel_variant": res["info"]["variant"], "tile_bytes": res["info"]["tile_bytes"],
                   "grid_blocks": res["info"]["grid_blocks"], "lds_bytes": res["info"]["lds_bytes"],
                   "staging_buffers": res["info"]["staging_buffers"], "staging_records": res["info"]["staging_records"],
                   "parallelism": f"input-sharded x{world}, halo {res['table'].halo} B",
                   "matches_per_step": res["matches"], "record_bytes": rec_bytes,
                   "record_layout": "heap of compact records (pos:12 | final state, as wide as the automaton needs) + ordered tile index (8 B per 4 KiB tile)",
                   "parity": "whole shard: count + checksum == serial AC (every rank, over the bytes copied back from HBM); "
                             "records of the first 1 MiB == CPU oracle in order, bit-exact" if args.full else "not checked (see --full)",
                   "settle_launches": res["settle"], "cold_first20_gbs": round(res["n_owned"] / (res["cold_ms"] * 1e-3) / 1e9, 1),
                   "value_note": "steady state: K steps after the clock-settling launches and the sustained run; `sustained` is the same scan run back to back for seconds, every launch timed",
                   "multi_gpu_note": "N > 1 numbers exist only where the driver ran them (SCALE_rNN.json): the builder's box has one GPU"},
        "roofline": {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_note": traffic_note,
                     "traffic_model": res["n_avail"] + rec_bytes * res["matches_rank"] + 8 * res["n_tiles"],
                     "traffic_model_note": "bytes one launch must move: input incl. halo + record bytes of this run's matches + tile index",
                     "kernel": "pfac_scan_kernel", "kernel_ms_avg": round(res["kernel_ms"], 4),
                     "kernel_ms_min": round(res["kernel_ms_min"], 4),
                     "algorithmic_bytes_per_launch": res["n_owned"]},
    }
    if "sustained" in res:
        out["sustained"] = res["sustained"]
    if "expand_ms" in res:
        out["config"].update({
            "expand_ms": round(res["expand_ms"], 3),
            "expand_note": "heap -> one sorted pfac_record array on the device, outside the timed region (what an ordered consumer pays)",
            "readback_ms": round(res["readback_ms"], 3), "readback_bytes": res["readback_bytes"],
            "readback_note": "D2H of the compact form (record heap + tile index) into pinned host memory, outside the timed region (the reference's dense D2H, master_kernel.cu:428, made compact)"})
    if "emit_text_ms" in res:
        out["config"].update({
            "emit_text_ms": round(res["emit_text_ms"], 3), "emit_text_bytes": res["emit_text_bytes"],
            "emit_text_note": "GPU-side text emitter (pfac_emit_text_device): these records formatted into the lines of GPU_match_result.txt in device memory, outside the timed region"})
    if "gather_ms" in res:
        out["config"]["gather_ms"] = round(res["gather_ms"], 3)
        out["config"]["gather_note"] = (f"ordered gather of {res.get('gather_records')} records to rank 0 in the COMPACT form the scan "
                                        f"wrote ({res.get('gather_bytes')} bytes: heap words + tile index, send/recv over RCCL), outside the timed region")
    if args.full and world == 1 and not args.no_extra:
        out["other_workloads"] = {}
        for name in sorted(WORKLOADS):
            if name == args.workload:
                continue
            k = max(3, args.steps // 4)
            r = run_workload(name, k, 1, False)
            out["other_workloads"][name] = {
                "value_gbs": round(n_total * k / r["dt"] / 1e9, 2),
                "kernel_gbs": round(r["n_owned"] / (r["kernel_ms"] * 1e-3) / 1e9, 2),
                "frac_of_hbm_peak": round(r["n_owned"] / (r["kernel_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "steps": k, "matches_per_step": r["matches"], "kernel_variant": r["info"]["variant"]}
    if args.full and world == 1 and not args.no_end_to_end and args.workload == HEADLINE:
        out["end_to_end"] = config3_end_to_end(res["ppath"], para, local_rank)
    if args.full and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(res["ppath"], res["kind"], para)
        out["cpu_baseline_pfac"] = cpu_baseline_pfac(res["ppath"], res["kind"], para)
        nthr = min(usable_cores(), 32) if args.cpu_threads < 0 else args.cpu_threads
        if nthr > 1:
            out["cpu_baseline_threads"] = cpu_baseline_threads(res["ppath"], res["kind"], para, nthr)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
