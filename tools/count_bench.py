"""GPU measurement of the per-state histogram (pfac_records_count_states) against the checksum of the same scan
(pfac_records_checksum: the same heap bytes, one atomic per wave -- the floor for this access pattern) and against
today's route to the same numbers (pfac_records_expand to 8-byte records, D2H of all of them, numpy.bincount).

For every workload: one resident input of --bytes (default 1 GiB), scanned once.  Each step runs, with HIP events on the
slot's stream around every call:

    count    (the whole call: the memsets, the kernel, the copy of the record count to the host),
    checksum (the whole call, likewise),
    count of the leftmost-longest selection (pfac_selection_count_states) where the table fits the selection;
    and, for --route-steps steps, expand + D2H into pinned memory + numpy.bincount (wall clock: the host does the work).

Medians over --steps steps after --warmup.  Once, before the timed steps, the counts are checked on the device against
torch.bincount of the expand output.  Prints ONE JSON line.  (`rocprofv3 --kernel-trace --stats -- python
tools/count_bench.py` gives the kernels' own times.)

    python tools/count_bench.py [--bytes N] [--steps 10] [--warmup 2] [--route-steps 2] [--workload NAME ...]
"""
import argparse
import gzip
import hashlib
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phfpfac_amd import GpuMatcher, PfacTable  # noqa: E402

DATA = os.path.join(REPO, "tests", "golden", "data")
KERNEL_SRC = os.path.join(REPO, "phfpfac_amd", "csrc", "pfac_hip.hip")
WORKLOADS = [  # name, pattern files, input kind
    ("text_experimentpattern", ("experimentpattern",), "text"),     # bench.py's headline workload: ONE hot state
    ("text_dictionary", ("xaa", "xab", "xac", "xad"), "text"),      # dense: thousands of states, a direct LDS table
    ("rand_snort75k", ("bytefile_1000000byte.gz",), "rand"),        # sparse, 75 840 states: the cache regime
]


def check_once(d_exp, total, counts):
    """On the device: the counts are torch.bincount of the states of the expanded records."""
    want = torch.zeros(counts.size, dtype=torch.int64, device="cuda:0")
    step = 1 << 26
    for lo in range(0, total, step):
        st = d_exp[lo:min(lo + step, total)].view(torch.int32).view(-1, 2)[:, 1].to(torch.int64)
        want += torch.bincount(st, minlength=counts.size)
    if not np.array_equal(want.cpu().numpy().astype(np.uint64), counts):
        raise SystemExit("count_bench: the counts differ from torch.bincount of the expanded records")


def run(name, pats, kind, n, steps, warmup, route_steps, tmpdir):
    path = os.path.join(tmpdir, name + ".pat")
    with open(path, "wb") as f:
        for p in pats:
            src = os.path.join(DATA, p)
            f.write(gzip.open(src, "rb").read() if p.endswith(".gz") else open(src, "rb").read())
    table = PfacTable.from_file(path, 256)
    stream = torch.cuda.Stream()
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        if kind == "text":
            g.fill_tiled(buf, n, open(os.path.join(DATA, "paragraph402"), "rb").read())
        else:
            g.fill_random(buf, n, 0x5048465046414331)
        g.reserve(0, 0, max(n // 8, 1 << 20))
        total = g.scan_resident(n, n, d_input=buf)
        total = g.scan_resident(n, n, d_input=buf)      # (the staging mode has adapted to the workload)
        rec_bytes, n_tiles, used = g.scan_format()
        d_exp = torch.empty(max(total, 1), dtype=torch.int64, device="cuda:0")
        g.expand_records(total, d_exp)
        assert g.count_states() == total
        counts = g.state_counts_to_host()
        check_once(d_exp, total, counts)
        n_sel, _ = g.select_leftmost_longest(0)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        t = {k: [] for k in ("count", "checksum", "count_selection")}
        for step in range(warmup + steps):
            ev[0].record(stream)
            assert g.count_states() == total
            ev[1].record(stream)
            g.checksum(total)
            ev[2].record(stream)
            assert g.count_selection_states() == n_sel
            ev[3].record(stream)
            ev[3].synchronize()
            if step < warmup:
                continue
            t["count"].append(ev[0].elapsed_time(ev[1]))
            t["checksum"].append(ev[1].elapsed_time(ev[2]))
            t["count_selection"].append(ev[2].elapsed_time(ev[3]))
        # today's route: 8-byte records over the link, the histogram on the host
        route, d2h, binc = [], [], []
        if route_steps:
            host = torch.empty(max(total, 1), dtype=torch.int64, pin_memory=True)
            for step in range(route_steps + 1):
                stream.synchronize()
                t0 = time.perf_counter()
                g.expand_records(total, d_exp)
                host.copy_(d_exp, non_blocking=True)
                stream.synchronize()
                t1 = time.perf_counter()
                today = np.bincount(host.numpy().view(np.uint32)[1:2 * total:2], minlength=table.num_final)
                t2 = time.perf_counter()
                if not np.array_equal(today.astype(np.uint64), counts):
                    raise SystemExit("count_bench: the host's bincount differs from the device's counts")
                if step:                                  # (the first pass faults the pinned pages in)
                    route.append((t2 - t0) * 1e3)
                    d2h.append((t1 - t0) * 1e3)
                    binc.append((t2 - t1) * 1e3)
            del host
        del buf, d_exp
    torch.cuda.empty_cache()
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {
        "workload": name, "bytes": n, "record_bytes": rec_bytes, "matches": total, "num_final": int(table.num_final),
        "states_hit": int((counts > 0).sum()), "hottest_state_share": round(float(counts.max()) / max(total, 1), 4),
        "selected": n_sel,
        "count_call_ms": round(med["count"], 3), "count_call_ms_min": round(float(np.min(t["count"])), 3),
        "checksum_call_ms": round(med["checksum"], 3), "checksum_call_ms_min": round(float(np.min(t["checksum"])), 3),
        "count_over_checksum": round(med["count"] / med["checksum"], 3),
        "count_ns_per_record": round(med["count"] * 1e6 / max(total, 1), 5),
        "count_selection_call_ms": round(med["count_selection"], 3),
    }
    if route:
        out.update({"expand_d2h_bincount_ms": round(float(np.median(route)), 1),
                    "expand_d2h_ms": round(float(np.median(d2h)), 1), "host_bincount_ms": round(float(np.median(binc)), 1),
                    "route_over_count": round(float(np.median(route)) / med["count"], 1)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--route-steps", type=int, default=2, help="timed passes of expand + D2H + numpy.bincount (0: skip)")
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    out = {"metric": "per-state histogram (pfac_records_count_states) vs pfac_records_checksum of the same scan, and vs "
                     "expand + D2H + numpy.bincount",
           "kernel_source_sha256": hashlib.sha256(open(KERNEL_SRC, "rb").read()).hexdigest(),
           "library": os.path.basename(os.environ.get("PFAC_HIP_LIB") or "libpfac_hip.so"),
           "steps": args.steps, "warmup": args.warmup, "route_steps": args.route_steps, "workloads": []}
    with tempfile.TemporaryDirectory() as tmpdir:
        for name, pats, kind in WORKLOADS:
            if args.workload and name not in args.workload:
                continue
            if not all(os.path.exists(os.path.join(DATA, p)) for p in pats):
                continue                                   # (rand_snort75k: only where its pattern set is)
            out["workloads"].append(run(name, pats, kind, args.bytes, args.steps, args.warmup, args.route_steps, tmpdir))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
