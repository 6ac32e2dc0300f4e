"""GPU measurement of the group-mask pass (pfac_documents_group_masks) and of grep_lines_where against what the same
answer costs without them.

The inputs and the pattern set are those of tools/split_bench.py: for every workload one resident input of --bytes
(default 1 GiB) of text lines that end in '\\n', scanned with experimentpattern; every pattern is in a group of its
own.  Two comparisons, in ONE process:

  mask pass   pfac_documents_group_masks (the memset, the one kernel, the 16-byte copy back) against
              pfac_records_segment + pfac_documents_matching over the same finished scan and the same offsets: both
              end with "which lines hold a match" on the device (for the masks: pfac_documents_matching_groups with
              any_of = ~0, timed apart).  HIP events on the slot's stream, medians over --steps steps after --warmup.
  end to end  GpuMatcher.grep_lines_where(any_of = ~0) against GpuMatcher.grep_lines on the same host buffer: upload,
              scan, split, [segment + matching | masks + predicate], gather, fetch.  Wall clock, median of --e2e-steps
              after one untimed call of each, on --e2e-bytes (default 256 MiB) of the same lines.

The ids of both paths are compared once, before the timed steps.  Prints ONE JSON line and writes it to --out.

    python tools/groups_bench.py [--bytes N] [--steps 20] [--warmup 3] [--e2e-steps 5] [--out profiles/groups_bench.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phfpfac_amd import GpuMatcher, PfacTable  # noqa: E402
from split_bench import DATA, DELIM, WORKLOADS, line_block  # noqa: E402

ALL = (1 << 64) - 1


def run(name, mean, n, steps, warmup, e2e_n, e2e_steps):
    table = PfacTable.from_file(os.path.join(DATA, "experimentpattern"), 256)
    groups = [None] + list(range(int(table.n_patterns)))        # pattern id i in group i - 1
    block = line_block(mean, mean)
    stream = torch.cuda.Stream()                 # (not the null stream: a NULL handle would give the slot its own back)
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)      # the slot's work runs on this stream: its events bracket it
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_pattern_groups(groups)
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, block.tobytes())
        g.reserve(0, 0, max(n // 8, 1 << 20))
        total = g.scan_resident(n, n, d_input=buf)
        g.scan_resident(n, n, d_input=buf)        # (the staging mode has adapted to the workload)
        n_docs, _ = g.split_documents(n, DELIM, d_input=buf)
        d_seg = torch.empty(max(total, 1), dtype=torch.int64, device="cuda:0")
        d_first = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
        d_ids = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
        d_masks = torch.empty(max(n_docs, 1), dtype=torch.int64, device="cuda:0")
        d_ids2 = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
        kept = g.segment_records(n_docs, d_out=d_seg, out_cap=total, d_doc_first=d_first)
        n_match = g.matching_documents(n_docs, d_doc_first=d_first, d_out=d_ids, out_cap=n_docs)
        any_mask = g.document_group_masks(n_docs, d_out=d_masks)
        n_where = g.matching_documents_where(n_docs, any_of=ALL, d_masks=d_masks, d_out=d_ids2, out_cap=n_docs)
        g.sync()
        if not (n_where == n_match and torch.equal(d_ids[:n_match], d_ids2[:n_where])):
            raise SystemExit("groups_bench: the ids of the mask path differ from those of segment + matching")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        seg_ms, match_ms, mask_ms, where_ms = [], [], [], []
        for step in range(warmup + steps):
            ev[0].record(stream)
            assert g.segment_records(n_docs, d_out=d_seg, out_cap=total, d_doc_first=d_first) == kept
            ev[1].record(stream)
            assert g.matching_documents(n_docs, d_doc_first=d_first, d_out=d_ids, out_cap=n_docs) == n_match
            ev[2].record(stream)
            assert g.document_group_masks(n_docs, d_out=d_masks) == any_mask
            ev[3].record(stream)
            assert g.matching_documents_where(n_docs, any_of=ALL, d_masks=d_masks, d_out=d_ids2, out_cap=n_docs) == n_match
            ev[4].record(stream)
            ev[4].synchronize()
            if step < warmup:
                continue
            seg_ms.append(ev[0].elapsed_time(ev[1]))
            match_ms.append(ev[1].elapsed_time(ev[2]))
            mask_ms.append(ev[2].elapsed_time(ev[3]))
            where_ms.append(ev[3].elapsed_time(ev[4]))
        # the slot-owned form: no copy of the masks into a caller's buffer
        own_ms = []
        for step in range(warmup + steps):
            ev[0].record(stream)
            g.document_group_masks(n_docs)
            ev[1].record(stream)
            ev[1].synchronize()
            if step >= warmup:
                own_ms.append(ev[0].elapsed_time(ev[1]))
        # end to end, from a host buffer
        host = buf[:e2e_n].cpu().numpy()
        host[-1] = DELIM
        del buf, d_seg, d_first, d_ids, d_masks, d_ids2
        a = g.grep_lines_where(host, any_of=ALL)
        b = g.grep_lines(host)
        if not all(np.array_equal(x, y) for x, y in zip(a, b)):
            raise SystemExit("groups_bench: grep_lines_where(any_of = ~0) differs from grep_lines")
        e2e_lines, e2e_out = int(a[2].size), int(a[0].size)
        del a, b
        where_wall, grep_wall = [], []
        for step in range(e2e_steps):                           # alternating, so that drift hits both alike
            t0 = time.perf_counter()
            g.grep_lines(host)
            t1 = time.perf_counter()
            g.grep_lines_where(host, any_of=ALL)
            t2 = time.perf_counter()
            grep_wall.append((t1 - t0) * 1e3)
            where_wall.append((t2 - t1) * 1e3)
    torch.cuda.empty_cache()
    med = lambda x: float(np.median(x))         # noqa: E731
    seg, match, mask, where, own = med(seg_ms), med(match_ms), med(mask_ms), med(where_ms), med(own_ms)
    return {
        "workload": name, "bytes": n, "mean_line_bytes": mean, "n_docs": n_docs, "matches": total, "kept": kept,
        "matching_docs": n_match, "any_mask": any_mask,
        "segment_ms": round(seg, 3), "matching_ms": round(match, 3), "group_masks_ms": round(mask, 3),
        "group_masks_slot_owned_ms": round(own, 3), "matching_groups_ms": round(where, 3),
        "group_masks_ms_min": round(float(np.min(mask_ms)), 3), "segment_ms_min": round(float(np.min(seg_ms)), 3),
        "masks_over_segment": round(mask / seg, 3),
        "masks_over_segment_plus_matching": round(mask / (seg + match), 3),
        "mask_path_over_segment_path": round((mask + where) / (seg + match), 3),
        "e2e_bytes": e2e_n, "e2e_lines_out": e2e_lines, "e2e_bytes_out": e2e_out,
        "grep_lines_ms": round(med(grep_wall), 1), "grep_lines_where_ms": round(med(where_wall), 1),
        "grep_lines_where_over_grep_lines": round(med(where_wall) / med(grep_wall), 3),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-bytes", type=int, default=1 << 28)
    ap.add_argument("--e2e-steps", type=int, default=5)
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "groups_bench.json"))
    args = ap.parse_args()
    if args.steps < 1 or args.e2e_steps < 1:
        raise SystemExit("--steps and --e2e-steps must be >= 1")
    out = {"metric": "pfac_documents_group_masks vs pfac_records_segment + pfac_documents_matching on the same scan, and "
                     "grep_lines_where(any_of = ~0) vs grep_lines on the same host buffer",
           "steps": args.steps, "warmup": args.warmup, "e2e_steps": args.e2e_steps,
           "group_masks_ms_counts": "the whole call into a caller's buffer: the memsets, the kernel, the 16-byte copy back, the copy of "
                                    "the masks behind the check (HIP events); _slot_owned_ms: without that copy",
           "segment_ms_counts": "the whole call: count, prefix, the 16-byte copy back, the write of 8 B per kept record (HIP events)",
           "e2e_ms_counts": "wall clock of the whole Python call from a host buffer: upload, scan, split, passes, gather, fetches",
           "workloads": []}
    for name, mean in WORKLOADS:
        if args.workload and name not in args.workload:
            continue
        out["workloads"].append(run(name, mean, args.bytes, args.steps, args.warmup, min(args.e2e_bytes, args.bytes), args.e2e_steps))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
