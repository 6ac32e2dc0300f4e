"""GPU measurement of the term-count pass (pfac_documents_term_counts) against a floor, against torch.unique and against
the host path it replaces.

The inputs and the pattern set are those of tools/score_bench.py: for every workload one resident input of --bytes
(default 1 GiB) of text lines that end in '\\n', scanned with experimentpattern, split at '\\n', cut per line into a
caller's buffers.  Then, in ONE process and over that same cut:

  terms         the whole call into the caller's buffers: the 8-byte read of doc_first[n_docs], the key kernel, the sort
                passes, the heads, the 16-byte copy back, the write, the counts and row_ptr
  segment       pfac_records_segment into the caller's buffers, the pass that feeds it: the floor -- it reads every
                record once and writes every kept one once
  torch_unique  torch.unique(keys, return_counts=True) on the device over the same packed keys doc << sbits | state,
                made by torch beforehand and not timed: what a torch user would write.  It yields the pairs and the
                counts, not row_ptr
  host_path     what a caller did before: segment_to_host, numpy.lexsort by (document, state) and run lengths (wall
                clock, since the host works)

HIP events on the slot's stream around each whole call, medians over --steps steps after --warmup; the device paths
alternate inside one step.  Once, before anything is timed, the pass over a scan of the first 4 MiB is compared with
tests/termref.py, and the pass over the whole input with torch.unique's pairs and counts.  Prints ONE JSON line and
writes it to --out.

    python tools/terms_bench.py [--bytes N] [--steps 20] [--warmup 3] [--host-steps 2] [--out profiles/terms_bench.json]

--host-steps 0 leaves the host path out.  With PFAC_ENABLE_KNOBS=1, PFAC_TERMS_ROWS=n limits the workgroups of a sort pass
to n instead of PFAC_TERMS_SORT_ROWS (the sweep of DESIGN.md section 23); the JSON names the value.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import termref  # noqa: E402
from phfpfac_amd import GpuMatcher, PfacTable  # noqa: E402
from split_bench import DATA, DELIM, WORKLOADS, line_block  # noqa: E402

CHECK_BYTES = 4 << 20


def host_path(g, n_kept, n_docs):
    """Both fetches, a lexsort by (document, state), run lengths."""
    first, rec = g.segment_to_host(n_kept, n_docs)
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(first.astype(np.int64)))
    st = rec["state"]
    order = np.lexsort((st, doc))
    d, s = doc[order], st[order]
    head = np.flatnonzero(np.concatenate([[True], (d[1:] != d[:-1]) | (s[1:] != s[:-1])])) if d.size else np.empty(0, np.int64)
    counts = np.diff(np.concatenate([head, [d.size]]))
    row = np.searchsorted(d[head], np.arange(n_docs + 1))
    return row, s[head], counts


def run(name, mean, n, steps, warmup, host_steps):
    table = PfacTable.from_file(os.path.join(DATA, "experimentpattern"), 256)
    nf = int(table.num_final)
    sbits = termref.state_bits(nf)
    block = line_block(mean, mean)
    stream = torch.cuda.Stream()
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, block.tobytes())
        g.reserve(0, 0, max(n // 8, 1 << 20))
        # once, before anything is timed: the first 4 MiB against the reference
        n4 = min(n, CHECK_BYTES)
        g.scan_resident(n4, n4, d_input=buf)
        nd4, _ = g.split_documents(n4, DELIM, d_input=buf)
        kept4 = g.segment_records(nd4)
        first4, rec4 = g.segment_to_host(kept4, nd4)
        nt4 = g.document_term_counts(nd4)
        termref.check(termref.term_counts(rec4["state"], first4, nf), *g.term_counts_to_host(nd4, nt4), what=f"terms_bench {name}, first 4 MiB")
        total = g.scan_resident(n, n, d_input=buf)
        g.scan_resident(n, n, d_input=buf)        # (the staging mode has adapted to the workload)
        n_docs, _ = g.split_documents(n, DELIM, d_input=buf)
        kept = g.segment_records(n_docs)
        d_rec = torch.empty(2 * max(kept, 1), dtype=torch.int32, device="cuda:0")
        d_first = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
        assert g.segment_records(n_docs, d_out=d_rec, out_cap=kept, d_doc_first=d_first) == kept
        n_terms = g.document_term_counts(n_docs, d_sel=d_rec, d_doc_first=d_first)
        d_row = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
        d_st = torch.empty(max(n_terms, 1), dtype=torch.int32, device="cuda:0")
        d_cnt = torch.empty(max(n_terms, 1), dtype=torch.int32, device="cuda:0")
        assert g.document_term_counts(n_docs, d_sel=d_rec, d_doc_first=d_first, d_row_ptr=d_row, d_states=d_st, d_counts=d_cnt,
                                      out_cap=n_terms) == n_terms
        g.sync()
        # the packed keys a torch user would build, and the whole input's result against torch.unique's
        doc = torch.repeat_interleave(torch.arange(n_docs, dtype=torch.int64, device="cuda:0"), d_first[1:] - d_first[:-1])
        keys = (doc << sbits) | d_rec.view(kept, 2)[:, 1].to(torch.int64)
        del doc
        uniq, ucnt = torch.unique(keys, return_counts=True)
        mine = (torch.repeat_interleave(torch.arange(n_docs, dtype=torch.int64, device="cuda:0"), d_row[1:] - d_row[:-1]) << sbits) | d_st[:n_terms].to(torch.int64)
        if not (uniq.numel() == n_terms and torch.equal(uniq, mine) and torch.equal(ucnt, d_cnt[:n_terms].to(torch.int64))):
            raise SystemExit("terms_bench: the pairs or counts of the pass differ from torch.unique's")
        del uniq, ucnt, mine
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        seg_ms, terms_ms, uniq_ms = [], [], []
        for step in range(warmup + steps):
            ev[0].record(stream)
            assert g.segment_records(n_docs, d_out=d_rec, out_cap=kept, d_doc_first=d_first) == kept
            ev[1].record(stream)
            assert g.document_term_counts(n_docs, d_sel=d_rec, d_doc_first=d_first, d_row_ptr=d_row, d_states=d_st, d_counts=d_cnt,
                                          out_cap=n_terms) == n_terms
            ev[2].record(stream)
            u = torch.unique(keys, return_counts=True)
            ev[3].record(stream)
            ev[3].synchronize()
            del u
            if step < warmup:
                continue
            for lst, k in ((seg_ms, 0), (terms_ms, 1), (uniq_ms, 2)):
                lst.append(ev[k].elapsed_time(ev[k + 1]))
        del keys
        g.segment_records(n_docs)                   # the host path reads the slot-owned cut
        host_wall = []
        for step in range(host_steps):
            t0 = time.perf_counter()
            h = host_path(g, kept, n_docs)
            host_wall.append((time.perf_counter() - t0) * 1e3)
        if host_steps and not (h[1].size == n_terms and np.array_equal(h[0], d_row.cpu().numpy()) and np.array_equal(h[1], d_st[:n_terms].cpu().numpy().view(np.uint32))
                and np.array_equal(h[2], d_cnt[:n_terms].cpu().numpy())):
            raise SystemExit("terms_bench: the host path's result differs from the pass's")
        del buf, d_rec, d_first, d_row, d_st, d_cnt
    torch.cuda.empty_cache()
    med = lambda x: float(np.median(x))         # noqa: E731
    mm = lambda x: [round(float(np.min(x)), 3), round(float(np.max(x)), 3)]      # noqa: E731
    chunks, n_blocks, per = termref.sort_shape(kept, int(os.environ.get("PFAC_TERMS_ROWS") or termref.SORT_ROWS))
    return {
        "workload": name, "bytes": n, "mean_line_bytes": mean, "n_docs": n_docs, "matches": total, "kept": kept, "n_terms": n_terms,
        "num_final": nf, "sort_passes": termref.sort_passes(n_docs, nf), "sort_chunks_per_workgroup": chunks, "sort_workgroups": n_blocks,
        "row_prefix_trips": per,
        "terms_ms": round(med(terms_ms), 3), "terms_ms_min_max": mm(terms_ms),
        "segment_ms": round(med(seg_ms), 3), "segment_ms_min_max": mm(seg_ms),
        "torch_unique_ms": round(med(uniq_ms), 3), "torch_unique_ms_min_max": mm(uniq_ms),
        "host_path_ms": round(med(host_wall), 1) if host_wall else None,
        "terms_over_segment": round(med(terms_ms) / med(seg_ms), 3),
        "terms_over_torch_unique": round(med(terms_ms) / med(uniq_ms), 3),
        "terms_over_host_path": round(med(terms_ms) / med(host_wall), 5) if host_wall else None,
        "terms_ns_per_record_pass": round(med(terms_ms) * 1e6 / max(kept, 1) / max(termref.sort_passes(n_docs, nf), 1), 4),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "terms_bench.json"))
    args = ap.parse_args()
    if args.steps < 1 or args.host_steps < 0:
        raise SystemExit("--steps must be >= 1 and --host-steps >= 0 (0: the host path is not run)")
    out = {"sort_rows_knob": os.environ.get("PFAC_TERMS_ROWS"),
           "metric": "pfac_documents_term_counts vs pfac_records_segment (the floor), vs torch.unique(return_counts=True) over the same "
                     "packed keys, and vs segment_to_host + numpy.lexsort + run lengths",
           "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps,
           "terms_ms_counts": "the whole call into the caller's buffers: the read of doc_first[n_docs], the key kernel, the sort, the "
                              "heads, the 16-byte copy back, the write, the counts, row_ptr (HIP events)",
           "torch_unique_ms_counts": "torch.unique alone; building its keys is not timed, and it yields no row_ptr",
           "host_path_ms_counts": "wall clock: the fetch of the kept records and doc_first, numpy.repeat, numpy.lexsort, the run lengths, "
                                  "numpy.searchsorted",
           "workloads": []}
    for name, mean in WORKLOADS:
        if args.workload and name not in args.workload:
            continue
        out["workloads"].append(run(name, mean, args.bytes, args.steps, args.warmup, args.host_steps))
        print(f"terms_bench: {name} done", file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
