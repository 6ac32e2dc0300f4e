"""GPU measurement of the document pass (pfac_records_segment) against pfac_records_expand of the same scan.

For every workload: one resident input of --bytes (default 1 GiB), cut into documents of a fixed size; each step scans
it, then cuts the scan into documents (segment) and expands the same scan into one sorted pfac_record array (expand),
in alternating order.  HIP events on the slot's stream time the scan, the segment call (count kernel, group prefix,
the copy of n_kept to the host, write kernel) and the expand call (group sums, prefix, copy kernel); medians over
--steps steps after --warmup.  The segment result is checked against the expand result on the host once, before the
timed steps.  Prints ONE JSON line.

    python tools/doc_bench.py [--bytes N] [--steps 20] [--warmup 3]
"""
import argparse
import gzip
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phfpfac_amd import GpuMatcher, PfacTable  # noqa: E402

DATA = os.path.join(REPO, "tests", "golden", "data")
SEED = 0x5048465046414331
WORKLOADS = [  # name, pattern fixture, input kind, document bytes
    ("text_experimentpattern_doc1500", "experimentpattern", "text", 1500),
    ("rand_snort75k_doc1500", "bytefile_1000000byte.gz", "rand", 1500),
    ("rand_snort75k_doc64", "bytefile_1000000byte.gz", "rand", 64),
]


def pattern_path(name, tmpdir):
    if name.endswith(".gz"):
        p = os.path.join(tmpdir, name[:-3])
        if not os.path.exists(p):
            with gzip.open(os.path.join(DATA, name), "rb") as g, open(p, "wb") as f:
                f.write(g.read())
        return p
    return os.path.join(DATA, name)


def check_once(g, table, n, off, total, kept, d_seg, d_first, d_exp):
    """segment == expand filtered by the document rule (lengths from the table, documents by searchsorted)."""
    whole = d_exp[:total].cpu().numpy().view(np.uint32).reshape(-1, 2)
    got = d_seg[:kept].cpu().numpy().view(np.uint32).reshape(-1, 2)
    first = d_first.cpu().numpy().view(np.uint64)
    pos = whole[:, 0].astype(np.int64)
    lens = table.final_lengths().astype(np.int64)
    o = off.astype(np.int64)
    doc = np.searchsorted(o, pos, side="right") - 1
    keep = pos + lens[whole[:, 1]] <= o[doc + 1]
    ok = (int(keep.sum()) == kept and np.array_equal(got[:, 0].astype(np.int64), (pos - o[doc])[keep])
          and np.array_equal(got[:, 1], whole[keep, 1])
          and np.array_equal(first, np.searchsorted(doc[keep], np.arange(off.size), side="left").astype(np.uint64)))
    if not ok:
        raise SystemExit("doc_bench: segment output differs from the filtered expand output")


def run(name, pat, kind, doc_bytes, n, steps, warmup, tmpdir):
    table = PfacTable.from_file(pattern_path(pat, tmpdir), 256)
    para = open(os.path.join(DATA, "paragraph402"), "rb").read()
    stream = torch.cuda.Stream()                 # (not the null stream: a NULL handle would give the slot its own back)
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)      # the slot's work runs on this stream: its events bracket it
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        if kind == "text":
            g.fill_tiled(buf, n, para)
        else:
            g.fill_random(buf, (n + 7) // 8 * 8, SEED)
        g.reserve(0, 0, max(n // 8, 1 << 20))
        total = g.scan_resident(n, n, d_input=buf)
        g.scan_resident(n, n, d_input=buf)        # (the staging mode has adapted to the workload)
        rec_bytes, n_tiles, used = g.scan_format()
        off = np.append(np.arange(0, n, doc_bytes, dtype=np.uint64), np.uint64(n))
        n_docs = off.size - 1
        g.set_doc_offsets(off)
        d_exp = torch.empty(max(total, 1), dtype=torch.int64, device="cuda:0")
        d_seg = torch.empty(max(total, 1), dtype=torch.int64, device="cuda:0")
        d_first = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
        kept = g.segment_records(n_docs, d_out=d_seg, out_cap=total, d_doc_first=d_first)
        g.expand_records(total, d_exp)
        g.sync()
        check_once(g, table, n, off, total, kept, d_seg, d_first, d_exp)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        scan_ms, seg_ms, exp_ms = [], [], []
        for step in range(warmup + steps):
            ev[0].record(stream)
            g.scan_async(n, n, d_input=buf)
            ev[1].record(stream)
            assert g.scan_finish(0)[0] == total
            ev[2].record(stream)
            if step % 2 == 0:
                assert g.segment_records(n_docs, d_out=d_seg, out_cap=total, d_doc_first=d_first) == kept
                ev[3].record(stream)
                g.expand_records(total, d_exp)
                ev[4].record(stream)
            else:
                g.expand_records(total, d_exp)
                ev[3].record(stream)
                assert g.segment_records(n_docs, d_out=d_seg, out_cap=total, d_doc_first=d_first) == kept
                ev[4].record(stream)
            ev[4].synchronize()
            if step < warmup:
                continue
            scan_ms.append(ev[0].elapsed_time(ev[1]))
            a, b = ev[2].elapsed_time(ev[3]), ev[3].elapsed_time(ev[4])
            seg_ms.append(a if step % 2 == 0 else b)
            exp_ms.append(b if step % 2 == 0 else a)
        del buf, d_exp, d_seg, d_first
    torch.cuda.empty_cache()
    seg, exp, scan = float(np.median(seg_ms)), float(np.median(exp_ms)), float(np.median(scan_ms))
    seg_bytes = total * rec_bytes + kept * 8 + (n_docs + 1) * 8      # heap read once + records and index written
    return {
        "workload": name, "bytes": n, "doc_bytes": doc_bytes, "n_docs": n_docs, "record_bytes": rec_bytes,
        "matches": total, "kept": kept, "scan_ms": round(scan, 3), "segment_ms": round(seg, 3),
        "expand_ms": round(exp, 3), "segment_over_expand": round(seg / exp, 3),
        "segment_gbs": round(seg_bytes / (seg * 1e-3) / 1e9, 1),
        "expand_gbs": round((total * rec_bytes + total * 8) / (exp * 1e-3) / 1e9, 1),
        "segment_ms_min": round(float(np.min(seg_ms)), 3), "expand_ms_min": round(float(np.min(exp_ms)), 3),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    out = {"metric": "document pass (pfac_records_segment) vs pfac_records_expand of the same scan",
           "steps": args.steps, "warmup": args.warmup,
           "segment_gbs_counts": "record heap read once + kept records (8 B) + doc_first (8 B per document) written",
           "workloads": []}
    with tempfile.TemporaryDirectory() as tmpdir:
        for name, pat, kind, doc_bytes in WORKLOADS:
            if args.workload and name not in args.workload:
                continue
            out["workloads"].append(run(name, pat, kind, doc_bytes, args.bytes, args.steps, args.warmup, tmpdir))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
