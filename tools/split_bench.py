"""GPU measurement of the device-side delimiter split (pfac_slot_doc_offsets_split) and of pfac_documents_matching
against (a) the scan of the same buffer and (b) today's host path for the same offsets.

For every workload: one resident input of --bytes (default 1 GiB) of text lines that end in '\\n' (a tiled block of
seeded line lengths around the workload's mean).  Each step scans it, splits it at '\\n', cuts the scan into the lines
(pfac_records_segment) and compacts the ids of the lines that matched (pfac_documents_matching).  HIP events on the
slot's stream time the scan, the split call (count, group sums, prefix, ends, the 16-byte copy back, the write) and the
matching call (count, prefix, the copy back, the write); medians over --steps steps after --warmup.  The host path is
what a caller does without the split: numpy.flatnonzero(buf == delim) over a host copy of the input, then
pfac_slot_doc_offsets (a blocking upload of 8 bytes per line) -- wall clock, median of --host-steps.  The offsets and the
ids are checked against the host's once, before the timed steps.  Prints ONE JSON line.

    python tools/split_bench.py [--bytes N] [--steps 20] [--warmup 3] [--host-steps 5]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phfpfac_amd import GpuMatcher, PfacTable  # noqa: E402

DATA = os.path.join(REPO, "tests", "golden", "data")
DELIM = 10
WORKLOADS = [  # name, mean line bytes (delimiter included)
    ("text_lines100", 100),
    ("text_lines1500", 1500),
    ("text_lines16", 16),
]


def line_block(mean, seed, block=1 << 20):
    """About `block` bytes of lines cut from the paragraph text, lengths uniform in [mean/2, 3 mean/2], each ending in
    the delimiter and holding no other."""
    para = open(os.path.join(DATA, "paragraph402"), "rb").read().replace(b"\n", b" ")
    text = np.frombuffer(para * (block // len(para) + 2), dtype=np.uint8)[:block].copy()
    rng = np.random.default_rng(seed)
    lens = rng.integers(max(mean // 2, 1), mean + mean // 2 + 1, block // max(mean // 2, 1) + 1)
    ends = np.cumsum(lens)
    ends = ends[ends <= block]
    text = text[:int(ends[-1])]
    text[ends - 1] = DELIM
    return text


def run(name, mean, n, steps, warmup, host_steps):
    table = PfacTable.from_file(os.path.join(DATA, "experimentpattern"), 256)
    block = line_block(mean, mean)
    stream = torch.cuda.Stream()                 # (not the null stream: a NULL handle would give the slot its own back)
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)      # the slot's work runs on this stream: its events bracket it
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, block.tobytes())
        g.reserve(0, 0, max(n // 8, 1 << 20))
        total = g.scan_resident(n, n, d_input=buf)
        g.scan_resident(n, n, d_input=buf)        # (the staging mode has adapted to the workload)
        n_docs, tail = g.split_documents(n, DELIM, d_input=buf)
        d_seg = torch.empty(max(total, 1), dtype=torch.int64, device="cuda:0")
        d_first = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
        d_ids = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
        kept = g.segment_records(n_docs, d_out=d_seg, out_cap=total, d_doc_first=d_first)
        n_match = g.matching_documents(n_docs, d_doc_first=d_first, d_out=d_ids, out_cap=n_docs)
        g.sync()
        # (b) the host path, and the check of the device results against it
        host = buf[:n].cpu().numpy()
        host_ms, up_ms = [], []
        for step in range(1 + host_steps):
            t0 = time.perf_counter()
            ends = np.flatnonzero(host == DELIM).astype(np.uint64) + np.uint64(1)
            off = np.concatenate([np.zeros(1, np.uint64), ends, np.full(0 if host[-1] == DELIM else 1, n, np.uint64)])
            t1 = time.perf_counter()
            g.set_doc_offsets(off)
            t2 = time.perf_counter()
            if step:
                host_ms.append((t2 - t0) * 1e3)
                up_ms.append((t2 - t1) * 1e3)
        first = d_first.cpu().numpy().view(np.uint64)
        want_ids = np.flatnonzero(first[1:] > first[:-1])
        want_tail = n if host[-1] == DELIM else int(ends[-1]) if ends.size else 0
        g.split_documents(n, DELIM, d_input=buf)
        if not (off.size == n_docs + 1 and tail == want_tail and np.array_equal(g.doc_offsets_to_host(n_docs), off)
                and n_match == want_ids.size and np.array_equal(d_ids[:n_match].cpu().numpy(), want_ids)):
            raise SystemExit("split_bench: the device offsets or ids differ from the host's")
        del host, ends, off
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        scan_ms, split_ms, seg_ms, match_ms = [], [], [], []
        for step in range(warmup + steps):
            ev[0].record(stream)
            g.scan_async(n, n, d_input=buf)
            ev[1].record(stream)
            assert g.scan_finish(0)[0] == total
            ev[2].record(stream)
            assert g.split_documents(n, DELIM, d_input=buf) == (n_docs, tail)
            ev[3].record(stream)
            assert g.segment_records(n_docs, d_out=d_seg, out_cap=total, d_doc_first=d_first) == kept
            ev[4].record(stream)
            assert g.matching_documents(n_docs, d_doc_first=d_first, d_out=d_ids, out_cap=n_docs) == n_match
            ev[5].record(stream)
            ev[5].synchronize()
            if step < warmup:
                continue
            scan_ms.append(ev[0].elapsed_time(ev[1]))
            split_ms.append(ev[2].elapsed_time(ev[3]))
            seg_ms.append(ev[3].elapsed_time(ev[4]))
            match_ms.append(ev[4].elapsed_time(ev[5]))
        del buf, d_seg, d_first, d_ids
    torch.cuda.empty_cache()
    med = lambda x: float(np.median(x))         # noqa: E731
    scan, split, match, hostp = med(scan_ms), med(split_ms), med(match_ms), med(host_ms)
    split_bytes = 2 * n + (n_docs + 1) * 8       # the input read twice + 8 B per offset written
    match_bytes = 2 * (n_docs + 1) * 8 + n_match * 8
    return {
        "workload": name, "bytes": n, "mean_line_bytes": mean, "n_docs": n_docs, "tail_start": tail, "matches": total,
        "kept": kept, "matching_docs": n_match, "scan_ms": round(scan, 3), "split_ms": round(split, 3),
        "segment_ms": round(med(seg_ms), 3), "matching_ms": round(match, 3),
        "split_over_scan": round(split / scan, 3), "matching_over_scan": round(match / scan, 3),
        "host_path_ms": round(hostp, 1), "host_upload_ms": round(med(up_ms), 1), "host_path_over_split": round(hostp / split, 1),
        "split_gbs": round(split_bytes / (split * 1e-3) / 1e9, 1), "matching_gbs": round(match_bytes / (match * 1e-3) / 1e9, 1),
        "split_ms_min": round(float(np.min(split_ms)), 3), "matching_ms_min": round(float(np.min(match_ms)), 3),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=5, help="timed repetitions of the host path (after one untimed)")
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    args = ap.parse_args()
    if args.steps < 1 or args.host_steps < 1:
        raise SystemExit("--steps and --host-steps must be >= 1")
    out = {"metric": "delimiter split (pfac_slot_doc_offsets_split) and pfac_documents_matching vs the scan of the same buffer "
                     "and vs numpy.flatnonzero + pfac_slot_doc_offsets on the host",
           "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps,
           "split_ms_counts": "the whole call: count, group sums, prefix, ends, the 16-byte copy back, the write (HIP events)",
           "split_gbs_counts": "the input read twice + 8 B per offset written",
           "host_path_ms_counts": "wall clock: flatnonzero over the input in host memory + the blocking upload of the offsets",
           "workloads": []}
    for name, mean in WORKLOADS:
        if args.workload and name not in args.workload:
            continue
        out["workloads"].append(run(name, mean, args.bytes, args.steps, args.warmup, args.host_steps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
