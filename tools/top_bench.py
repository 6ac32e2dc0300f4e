"""GPU measurement of the rank over document scores (pfac_documents_top_scores) against a floor, against torch.topk and
against the host path it replaces.

The inputs, the pattern set and the weights are those of tools/score_bench.py: for every workload one resident input of
--bytes (default 1 GiB) of text lines, scanned with experimentpattern, split at '\\n', scored once into a caller's
buffer.  Then, in ONE process and over those same scores, for k in {10, 1 000, 1 % of n_docs}, by score, largest first:

  top_ranked / top_unranked  the whole call into the caller's buffers (the memset, the eight select passes and their
              picks, the 8-byte copy back, the compaction and, ranked, the sort), no rule: every line is a candidate
  floor       pfac_documents_matching_scores (min_count = 1) over the same scores: ONE count pass and one write pass
              over the same bytes -- what any answer that reads every score costs at least
  torch_topk  torch.topk on a device int64 view of the score column (stride 2) plus the index gather of the pairs
  host_path   what a caller did before: the scores D2H, numpy.argpartition, a sort of the k, the ids H2D (wall clock,
              since the host works)

HIP events on the slot's stream around each whole call, medians over --steps steps after --warmup; the device paths
alternate inside one step.  Once, before anything is timed, the scores of the ranked winners are compared with
torch.topk's values (the ids may differ inside a tie) and the unranked ids with the sorted ranked ones.  Prints ONE JSON
line and writes it to --out.

    python tools/top_bench.py [--bytes N] [--steps 20] [--warmup 3] [--host-steps 2] [--out profiles/top_bench.json]
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


def host_path(d_scores, n_docs, k, stream):
    """Scores D2H, argpartition, a sort of the winners (ties to the smaller id), ids H2D."""
    sc = d_scores.view(n_docs, 2).cpu().numpy()[:, 0]
    part = np.argpartition(-sc, k - 1)[:k] if k < n_docs else np.arange(n_docs)
    ids = part[np.lexsort((part, -sc[part]))].astype(np.int64)
    d_ids = torch.from_numpy(ids).to("cuda:0")
    stream.synchronize()
    return d_ids


def run(name, mean, n, steps, warmup, host_steps):
    table = PfacTable.from_file(os.path.join(DATA, "experimentpattern"), 256)
    n_ids = int(table.n_patterns)
    weights = [0] + [5 * i % 7 - 3 for i in range(1, n_ids + 1)]
    block = line_block(mean, mean)
    stream = torch.cuda.Stream()
    rows = []
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_pattern_weights(weights)
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, block.tobytes())
        g.reserve(0, 0, max(n // 8, 1 << 20))
        g.scan_resident(n, n, d_input=buf)
        n_docs, _ = g.split_documents(n, DELIM, d_input=buf)
        d_scores = torch.empty(2 * max(n_docs, 1), dtype=torch.int64, device="cuda:0")
        g.document_scores(n_docs, d_out=d_scores)
        g.sync()
        del buf
        column = d_scores.view(n_docs, 2)[:, 0]
        d_all = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        for k in (10, 1000, max(n_docs // 100, 1)):
            k = min(k, n_docs)
            d_ids = torch.empty(k, dtype=torch.int64, device="cuda:0")
            d_ids_u = torch.empty(k, dtype=torch.int64, device="cuda:0")
            d_pairs = torch.empty(2 * k, dtype=torch.int64, device="cuda:0")
            # once, untimed: the winners' scores are torch.topk's values, the unranked ids are the ranked ones sorted
            assert g.top_documents(n_docs, k, d_scores=d_scores, d_out=d_ids, out_cap=k, d_top_scores=d_pairs) == k
            assert g.top_documents(n_docs, k, ranked=False, d_scores=d_scores, d_out=d_ids_u, out_cap=k, d_top_scores=d_pairs) == k
            g.sync()
            values = torch.topk(column, k).values
            stream.synchronize()
            if not torch.equal(column[d_ids], values):
                raise SystemExit(f"top_bench: the scores of the ranked winners differ from torch.topk's values (k = {k})")
            if not torch.equal(torch.sort(d_ids).values, d_ids_u):
                raise SystemExit(f"top_bench: the unranked ids are not the ranked ones in document order (k = {k})")
            if not torch.equal(column[host_path(d_scores, n_docs, k, stream)], values):    # (argpartition cuts a tie class anywhere)
                raise SystemExit(f"top_bench: the host path's scores differ from torch.topk's values (k = {k})")
            n_floor = g.matching_documents_scored(n_docs, min_count=1, d_scores=d_scores, d_out=d_all, out_cap=n_docs)
            ranked_ms, unranked_ms, floor_ms, topk_ms = [], [], [], []
            for step in range(warmup + steps):
                ev[0].record(stream)
                g.top_documents(n_docs, k, d_scores=d_scores, d_out=d_ids, out_cap=k, d_top_scores=d_pairs)
                ev[1].record(stream)
                g.top_documents(n_docs, k, ranked=False, d_scores=d_scores, d_out=d_ids_u, out_cap=k, d_top_scores=d_pairs)
                ev[2].record(stream)
                g.matching_documents_scored(n_docs, min_count=1, d_scores=d_scores, d_out=d_all, out_cap=n_docs)
                ev[3].record(stream)
                idx = torch.topk(column, k).indices
                pairs = d_scores.view(n_docs, 2)[idx]
                ev[4].record(stream)
                ev[4].synchronize()
                del idx, pairs
                if step >= warmup:
                    for lst, j in ((ranked_ms, 0), (unranked_ms, 1), (floor_ms, 2), (topk_ms, 3)):
                        lst.append(ev[j].elapsed_time(ev[j + 1]))
            host_wall = []
            for step in range(host_steps):
                t0 = time.perf_counter()
                host_path(d_scores, n_docs, k, stream)
                host_wall.append((time.perf_counter() - t0) * 1e3)
            med = lambda x: float(np.median(x))         # noqa: E731
            ranked, unranked, floor, topk, host = med(ranked_ms), med(unranked_ms), med(floor_ms), med(topk_ms), med(host_wall)
            rows.append({
                "workload": name, "bytes": n, "mean_line_bytes": mean, "n_docs": n_docs, "k": k, "floor_docs": n_floor,
                "top_ranked_ms": round(ranked, 3), "top_unranked_ms": round(unranked, 3), "floor_ms": round(floor, 3),
                "torch_topk_ms": round(topk, 3), "host_path_ms": round(host, 1),
                "top_ranked_ms_min_max": [round(float(np.min(ranked_ms)), 3), round(float(np.max(ranked_ms)), 3)],
                "torch_topk_ms_min_max": [round(float(np.min(topk_ms)), 3), round(float(np.max(topk_ms)), 3)],
                "top_ranked_over_floor": round(ranked / floor, 2), "top_unranked_over_floor": round(unranked / floor, 2),
                "top_ranked_over_torch_topk": round(ranked / topk, 2), "top_ranked_over_host_path": round(ranked / host, 4),
                "scores_bytes_per_ranked_call_GBps": round(n_docs * 16 / (ranked * 1e6), 1),
            })
            del d_ids, d_ids_u, d_pairs
        del d_scores, d_all, column
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "top_bench.json"))
    args = ap.parse_args()
    if args.steps < 1 or args.host_steps < 1:
        raise SystemExit("--steps and --host-steps must be >= 1")
    out = {"metric": "pfac_documents_top_scores (by score, largest first, no rule) vs pfac_documents_matching_scores over the same "
                     "scores, vs torch.topk + index gather, vs scores D2H + numpy.argpartition + sort + ids H2D",
           "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps,
           "top_ms_counts": "the whole call into the caller's buffers (HIP events): memset, select, copy back, compaction, sort",
           "host_path_ms_counts": "wall clock: the scores D2H, numpy.argpartition, numpy.lexsort of the k, the ids H2D",
           "rows": []}
    for name, mean in WORKLOADS:
        if args.workload and name not in args.workload:
            continue
        out["rows"] += run(name, mean, args.bytes, args.steps, args.warmup, args.host_steps)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
