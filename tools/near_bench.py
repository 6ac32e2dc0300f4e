"""GPU measurement of the proximity-rule pass (pfac_documents_near) against the project's own yardsticks for "one walk
over the records" and against the host path it replaces.

The inputs are those of tools/groups_bench.py: for every workload one resident input of --bytes
(default 1 GiB) of text lines that end in '\\n'.  The pattern set is --patterns: WORDS16 (default), sixteen short words
and fragments of which the text holds many per line -- groups_bench.py's experimentpattern reaches ONE final state in this
text, so no pair of two classes exists there (profiles/near_bench_experimentpattern.json keeps that run: the pass with
nothing to pair).  The final states that occur are dealt over the 64 groups by frequency.
Rule r of a set of k pairs group r with group 7 r + 1 (modulo the populated groups) within 5, 20, 60 or 200 bytes, every
other rule ordered.  Timed, in
ONE process, for every k of --rule-counts (default 1, 8 and 64 rules):

  pass        pfac_documents_near over the slot-owned result of pfac_records_segment (the rules' upload, the memsets, the
              three kernels, the 16-byte copy back).  HIP events on the slot's stream, medians over --steps after --warmup.
  yardsticks  pfac_records_segment and pfac_documents_group_masks on the same scan and the same offsets, the same way.
  host path   what a caller did before, on --host-bytes (default 32 MiB) of the same lines: pfac_records_segment, the
              fetch of the kept records and doc_first (8 bytes per record across the link), and the rules in numpy -- per
              rule the previous A / previous B index by numpy.maximum.accumulate, clipped at doc_first.  Wall clock (the
              host works), median of --host-steps; the device's masks of the same input are compared with it first.

The clocks the driver reports are recorded before and after (rocm-smi --showclocks, read only; "not available" if the
tool is not there).  Prints ONE JSON line and writes it to --out.

    python tools/near_bench.py [--bytes N] [--steps 20] [--warmup 3] [--host-steps 3] [--out profiles/near_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phfpfac_amd import GpuMatcher, PfacTable, near_rule  # noqa: E402
from split_bench import DATA, DELIM, WORKLOADS, line_block  # noqa: E402

RULE_COUNTS = (1, 8, 64)
WORDS16 = [b"the", b"he", b"th", b"and", b"an", b"in", b"ing", b"ed", b" t", b"er", b"that", b"re", b"at", b"en", b"on", b"with"]


def rule_set(k, n_groups):
    """k rules over the populated groups: rule r pairs group r with group 7 r + 1 (both modulo n_groups)."""
    return np.stack([near_rule(r % n_groups, (7 * r + 1) % n_groups, (5, 20, 60, 200)[r % 4], ordered=bool(r & 1)) for r in range(k)])


def host_near(rec, first, gmask, rules):
    """The rules on the host, vectorised: what the pass replaces."""
    f = first.astype(np.int64)
    n_docs, n = f.size - 1, int(f[-1])
    out = np.zeros(n_docs, dtype=np.uint64)
    if n == 0:
        return out
    g, p = gmask[rec["state"].astype(np.int64)], rec["pos"].astype(np.int64)
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(f))
    start, idx = f[doc], np.arange(n, dtype=np.int64)

    def fires(mine, other, dist):
        prev = np.concatenate([[-1], np.maximum.accumulate(np.where(other, idx, -1))[:-1]])
        return mine & (prev >= start) & (p - p[np.maximum(prev, 0)] <= dist)
    for r, ru in enumerate(rules):
        isa, isb = (g & ru["a_groups"]) != 0, (g & ru["b_groups"]) != 0
        fire = fires(isb, isa, int(ru["max_dist"]))
        if not int(ru["flags"]) & 1:
            fire |= fires(isa, isb, int(ru["max_dist"]))
        hit = np.zeros(n_docs, dtype=bool)
        hit[doc[fire]] = True
        out[hit] |= np.uint64(1) << np.uint64(r)
    return out


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        keep = [" ".join(x.split()) for x in out.splitlines() if "clk" in x.lower() and "GPU[0]" in x]
        return keep or "not available"
    except (OSError, subprocess.SubprocessError):
        return "not available"


def run(name, mean, n, steps, warmup, host_n, host_steps, patterns, counts):
    if patterns == "words16":
        table = PfacTable.from_bytes(b"".join(w + b"\n" for w in WORDS16), 256)
    else:
        table = PfacTable.from_file(os.path.join(DATA, patterns), 256)
    block = line_block(mean, mean)
    stream = torch.cuda.Stream()                 # (not the null stream: a NULL handle would give the slot its own back)
    med = lambda x: float(np.median(x))         # noqa: E731
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)      # the slot's work runs on this stream: its events bracket it
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, block.tobytes())
        g.reserve(0, 0, max(n // 2, 1 << 20))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

        def scan(n_bytes):
            g.scan_resident(n_bytes, n_bytes, d_input=buf)
            total = g.scan_resident(n_bytes, n_bytes, d_input=buf)           # (the staging mode has adapted to the workload)
            n_docs, _ = g.split_documents(n_bytes, DELIM, d_input=buf)
            return total, n_docs

        # the host path first, on the smaller input, and the device's masks held against it
        total, n_docs = scan(host_n)
        # the groups: the final states that occur, by how often, dealt round robin over the 64 groups -- every group
        # holds patterns of the text, so the rules' classes are all populated
        _, rec = g.segment_to_host(g.segment_records(n_docs), n_docs)
        hist = np.bincount(rec["state"], minlength=int(table.num_final))
        order = np.argsort(-hist, kind="stable")[:int(np.count_nonzero(hist))]
        groups = np.zeros(int(table.n_patterns) + 1, dtype=np.uint64)
        groups[np.asarray(table.idmap, dtype=np.int64)[order]] = np.uint64(1) << (np.arange(order.size, dtype=np.uint64) % np.uint64(64))
        g.set_pattern_groups(groups)
        gmask = table.state_group_masks(groups)
        states_seen = int(order.size)
        host = {}
        for k in counts:
            if k not in RULE_COUNTS:                            # (the rule counts between: the pass alone)
                continue
            rules = rule_set(k, min(states_seen, 64))
            wall = []
            for step in range(host_steps):
                t0 = time.perf_counter()
                kept = g.segment_records(n_docs)
                first, rec = g.segment_to_host(kept, n_docs)
                want = host_near(rec, first, gmask, rules)
                wall.append((time.perf_counter() - t0) * 1e3)
            g.document_near_masks(n_docs, rules)
            if not np.array_equal(g.near_masks_to_host(n_docs), want):
                raise SystemExit(f"near_bench: the device's masks differ from the host's ({name}, {k} rules)")
            host[k] = {"host_path_ms": round(med(wall), 1), "docs_fired": int(np.count_nonzero(want)), "kept": int(kept), "n_docs": int(n_docs)}
        total, n_docs = scan(n)
        seg_ms, mask_ms = [], []
        for step in range(warmup + steps):
            ev[0].record(stream)
            kept = g.segment_records(n_docs)
            ev[1].record(stream)
            g.document_group_masks(n_docs)
            ev[2].record(stream)
            ev[2].synchronize()
            if step >= warmup:
                seg_ms.append(ev[0].elapsed_time(ev[1]))
                mask_ms.append(ev[1].elapsed_time(ev[2]))
        per_k = {}
        for k in counts:
            rules = rule_set(k, min(states_seen, 64))
            ms = []
            for step in range(warmup + steps):
                ev[0].record(stream)
                any_mask = g.document_near_masks(n_docs, rules)
                ev[1].record(stream)
                ev[1].synchronize()
                if step >= warmup:
                    ms.append(ev[0].elapsed_time(ev[1]))
            fired = int(np.count_nonzero(g.near_masks_to_host(n_docs)))
            scale = n / host_n
            per_k[str(k)] = {"near_ms": round(med(ms), 3), "near_ms_min": round(float(np.min(ms)), 3), "docs_fired": fired,
                             "rules_fired": bin(any_mask).count("1"), "near_over_segment": round(med(ms) / med(seg_ms), 3),
                             "near_over_group_masks": round(med(ms) / med(mask_ms), 3),
                             "records_per_s": round(kept / (med(ms) * 1e-3))}
            if k in host:
                per_k[str(k)].update({"host": host[k], "host_path_ms_scaled_to_bytes": round(host[k]["host_path_ms"] * scale, 1),
                                      "host_scaled_over_near": round(host[k]["host_path_ms"] * scale / med(ms), 1)})
    torch.cuda.empty_cache()
    ks = sorted(int(k) for k in per_k)
    slopes = {f"{a}_to_{b}": round((per_k[str(b)]["near_ms"] - per_k[str(a)]["near_ms"]) / (b - a), 4) for a, b in zip(ks[:-1], ks[1:])}
    return {"workload": name, "bytes": n, "host_bytes": host_n, "mean_line_bytes": mean, "n_docs": int(n_docs), "matches": int(total),
            "kept": int(kept), "states_in_groups": states_seen, "segment_ms": round(med(seg_ms), 3), "group_masks_ms": round(med(mask_ms), 3), "rules": per_k,
            "ms_per_added_rule": slopes, "most_over_fewest_rules": round(per_k[str(ks[-1])]["near_ms"] / per_k[str(ks[0])]["near_ms"], 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-bytes", type=int, default=1 << 25)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--rule-counts", default="1,8,64", help="rule counts to time (the host path runs at 1, 8 and 64 of them)")
    ap.add_argument("--patterns", default="words16", help="words16, or a pattern file of tests/golden/data")
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "near_bench.json"))
    args = ap.parse_args()
    if args.steps < 1 or args.host_steps < 1:
        raise SystemExit("--steps and --host-steps must be >= 1")
    out = {"metric": "pfac_documents_near with 1, 8 and 64 rules vs pfac_records_segment and pfac_documents_group_masks on the same scan, "
                     "and vs segment + D2H + numpy on a smaller input of the same lines",
           "patterns": args.patterns, "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps,
           "near_ms_counts": "the whole call over the slot-owned segment result into the slot-owned masks: the rules' upload, the memsets, "
                             "the three kernels, the 16-byte copy back (HIP events)",
           "host_path_ms_counts": "wall clock on host_bytes: pfac_records_segment, the fetch of the kept records and doc_first, numpy; "
                                  "_scaled_to_bytes multiplies by bytes / host_bytes (the host path is linear in the records)",
           "clocks_before": clocks(), "workloads": []}
    for name, mean in WORKLOADS:
        if args.workload and name not in args.workload:
            continue
        out["workloads"].append(run(name, mean, args.bytes, args.steps, args.warmup, min(args.host_bytes, args.bytes), args.host_steps, args.patterns,
                                    sorted({int(k) for k in args.rule_counts.split(",")})))
    out["clocks_after"] = clocks()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
