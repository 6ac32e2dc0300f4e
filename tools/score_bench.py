"""GPU measurement of the score pass (pfac_documents_scores) and of its predicate (pfac_documents_matching_scores)
against the nearest existing passes and against the path they replace.

The inputs and the pattern set are those of tools/groups_bench.py: for every workload one resident input of --bytes
(default 1 GiB) of text lines that end in '\\n', scanned with experimentpattern; pattern id i has weight 5 i % 7 - 3 (the
one pattern that English text holds, "a", weighs -2) and is in a group of its own.  In ONE process, on the same finished scan and the same offsets:

  score pass  pfac_documents_scores (the memsets, the one kernel, the 24-byte copy back) against
              pfac_documents_group_masks, which reads what it reads and writes 8 instead of 16 bytes per document, and
              against the host path it replaces: pfac_records_segment, the fetch of the kept records and of doc_first,
              numpy.add.at of the weights and numpy.diff for the counts (wall clock, since the host works).
  predicate   pfac_documents_matching_scores (min_count = 1, and the same with a density of -3 / 1, which every line
              meets: it adds the two loads of the offsets and the 128-bit compare) against
              pfac_documents_matching_groups (any_of = ~0): all three report "the lines that hold a match".

HIP events on the slot's stream, medians over --steps steps after --warmup; the device paths alternate inside one step.
The scores of the device are compared with the host path's once, before the timed steps.  Prints ONE JSON line and
writes it to --out.

    python tools/score_bench.py [--bytes N] [--steps 20] [--warmup 3] [--host-steps 2] [--out profiles/score_bench.json]
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

from phfpfac_amd import SCORE_DTYPE, GpuMatcher, PfacTable  # noqa: E402
from split_bench import DATA, DELIM, WORKLOADS, line_block  # noqa: E402

ALL = (1 << 64) - 1


def host_path(g, table, w_state, n_docs):
    """What a user did before the pass: the document cut, both fetches, the sums on the host."""
    kept = g.segment_records(n_docs)
    first, rec = g.segment_to_host(kept, n_docs)
    out = np.zeros(n_docs, dtype=SCORE_DTYPE)
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(first.astype(np.int64)))
    np.add.at(out["score"], doc, w_state[rec["state"]])
    out["count"] = np.diff(first)
    return out


def run(name, mean, n, steps, warmup, host_steps):
    table = PfacTable.from_file(os.path.join(DATA, "experimentpattern"), 256)
    n_ids = int(table.n_patterns)
    weights = [0] + [5 * i % 7 - 3 for i in range(1, n_ids + 1)]
    groups = [None] + list(range(n_ids))
    w_state = table.state_weights(weights).astype(np.int64)
    block = line_block(mean, mean)
    stream = torch.cuda.Stream()
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_pattern_groups(groups)
        g.set_pattern_weights(weights)
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, block.tobytes())
        g.reserve(0, 0, max(n // 8, 1 << 20))
        total = g.scan_resident(n, n, d_input=buf)
        g.scan_resident(n, n, d_input=buf)        # (the staging mode has adapted to the workload)
        n_docs, _ = g.split_documents(n, DELIM, d_input=buf)
        d_masks = torch.empty(max(n_docs, 1), dtype=torch.int64, device="cuda:0")
        d_scores = torch.empty(2 * max(n_docs, 1), dtype=torch.int64, device="cuda:0")
        d_ids = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
        d_ids2 = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
        # once, before anything is timed: the device's scores are the host path's
        want = host_path(g, table, w_state, n_docs)
        tot = g.document_scores(n_docs)
        got = g.document_scores_to_host(n_docs)
        if not (np.array_equal(got["score"], want["score"]) and np.array_equal(got["count"], want["count"])
                and tot == (int(want["score"].sum()), int(want["count"].sum()))):
            raise SystemExit("score_bench: the scores of the device differ from the host path's")
        any_mask = g.document_group_masks(n_docs, d_out=d_masks)
        assert g.document_scores(n_docs, d_out=d_scores) == tot
        n_match = g.matching_documents_where(n_docs, any_of=ALL, d_masks=d_masks, d_out=d_ids, out_cap=n_docs)
        n_scored = g.matching_documents_scored(n_docs, min_count=1, d_scores=d_scores, d_out=d_ids2, out_cap=n_docs)
        g.sync()
        if not (n_scored == n_match and torch.equal(d_ids[:n_match], d_ids2[:n_scored])):
            raise SystemExit("score_bench: the ids of the score predicate differ from those of the group predicate")
        n_dense = g.matching_documents_scored(n_docs, min_count=1, density=(-3, 1), d_scores=d_scores, d_out=d_ids2, out_cap=n_docs)
        if n_dense != n_match:
            raise SystemExit("score_bench: the density that every line meets changed the ids")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        mask_ms, score_ms, where_ms, scored_ms, dense_ms = [], [], [], [], []
        for step in range(warmup + steps):
            ev[0].record(stream)
            assert g.document_group_masks(n_docs, d_out=d_masks) == any_mask
            ev[1].record(stream)
            assert g.document_scores(n_docs, d_out=d_scores) == tot
            ev[2].record(stream)
            assert g.matching_documents_where(n_docs, any_of=ALL, d_masks=d_masks, d_out=d_ids, out_cap=n_docs) == n_match
            ev[3].record(stream)
            assert g.matching_documents_scored(n_docs, min_count=1, d_scores=d_scores, d_out=d_ids2, out_cap=n_docs) == n_match
            ev[4].record(stream)
            assert g.matching_documents_scored(n_docs, min_count=1, density=(-3, 1), d_scores=d_scores, d_out=d_ids2,
                                               out_cap=n_docs) == n_dense
            ev[5].record(stream)
            ev[5].synchronize()
            if step < warmup:
                continue
            for lst, k in ((mask_ms, 0), (score_ms, 1), (where_ms, 2), (scored_ms, 3), (dense_ms, 4)):
                lst.append(ev[k].elapsed_time(ev[k + 1]))
        # the slot-owned forms: no copy of the result into a caller's buffer
        own_mask, own_score = [], []
        for step in range(warmup + steps):
            ev[0].record(stream)
            g.document_group_masks(n_docs)
            ev[1].record(stream)
            g.document_scores(n_docs)
            ev[2].record(stream)
            ev[2].synchronize()
            if step >= warmup:
                own_mask.append(ev[0].elapsed_time(ev[1]))
                own_score.append(ev[1].elapsed_time(ev[2]))
        host_wall = []
        for step in range(host_steps):                          # (the comparison above was its untimed first run)
            t0 = time.perf_counter()
            host_path(g, table, w_state, n_docs)
            host_wall.append((time.perf_counter() - t0) * 1e3)
        del buf, d_masks, d_scores, d_ids, d_ids2
    torch.cuda.empty_cache()
    med = lambda x: float(np.median(x))         # noqa: E731
    mask, score, where, scored, dense = med(mask_ms), med(score_ms), med(where_ms), med(scored_ms), med(dense_ms)
    return {
        "workload": name, "bytes": n, "mean_line_bytes": mean, "n_docs": n_docs, "matches": total, "kept": tot[1],
        "total_score": tot[0], "matching_docs": n_match, "matching_docs_dense": n_dense,
        "group_masks_ms": round(mask, 3), "scores_ms": round(score, 3),
        "group_masks_ms_min_max": [round(float(np.min(mask_ms)), 3), round(float(np.max(mask_ms)), 3)],
        "scores_ms_min_max": [round(float(np.min(score_ms)), 3), round(float(np.max(score_ms)), 3)],
        "group_masks_slot_owned_ms": round(med(own_mask), 3), "scores_slot_owned_ms": round(med(own_score), 3),
        "host_path_ms": round(med(host_wall), 1),
        "matching_groups_ms": round(where, 3), "matching_scores_ms": round(scored, 3), "matching_scores_density_ms": round(dense, 3),
        "scores_over_group_masks": round(score / mask, 3),
        "scores_slot_owned_over_group_masks_slot_owned": round(med(own_score) / med(own_mask), 3),
        "scores_over_host_path": round(score / med(host_wall), 4),
        "matching_scores_over_matching_groups": round(scored / where, 3),
        "matching_scores_density_over_matching_groups": round(dense / where, 3),
        "scores_written_GBps": round(n_docs * 16 / (med(own_score) * 1e6), 1),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "score_bench.json"))
    args = ap.parse_args()
    if args.steps < 1 or args.host_steps < 1:
        raise SystemExit("--steps and --host-steps must be >= 1")
    out = {"metric": "pfac_documents_scores vs pfac_documents_group_masks on the same scan and vs segment + fetch + numpy.add.at; "
                     "pfac_documents_matching_scores vs pfac_documents_matching_groups",
           "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps,
           "scores_ms_counts": "the whole call into a caller's buffer: the memsets, the kernel, the 24-byte copy back, the copy of the "
                               "scores behind the check (HIP events); _slot_owned_ms: without that copy",
           "host_path_ms_counts": "wall clock: pfac_records_segment, the fetch of the kept records and doc_first, numpy.repeat, "
                                  "numpy.add.at, numpy.diff",
           "workloads": []}
    for name, mean in WORKLOADS:
        if args.workload and name not in args.workload:
            continue
        out["workloads"].append(run(name, mean, args.bytes, args.steps, args.warmup, args.host_steps))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
