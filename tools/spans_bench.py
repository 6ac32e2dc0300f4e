"""GPU measurement of the span filter (pfac_records_filter_spans) against the two passes that walk the same heap with
the same document lookup: pfac_records_filter_words with documents, and pfac_records_segment.

The inputs are those of tools/split_bench.py: for every workload one resident input of --bytes (default 1 GiB) of text
lines that end in '\\n' (mean 100 / 1 500 / 16 bytes).  Two pattern sets: experimentpattern (at most 64 final states:
lengths and spans in lane registers) and the dictionary xaa+xab+xac+xad (one 16-byte span gather per record).  Every
pattern draws its rule from {none, ^, $, ^$, (5, 25 - L, ANY)}.  Each step runs, with HIP events on the slot's stream
around every call, a fresh scan in front of each (a filter changes the heap it reads):

    scan, filter_words (documents = the lines; both edges, the default word set)
    scan, filter_spans (the drawn rules, delimiter '\\n')
    scan, filter_spans (PFAC_SPANS_LINE: grep -x, no span load)
    scan, segment      (into a caller's buffers)

Medians over --steps steps after --warmup; every figure is the whole call (memsets, the offsets' check, the kernel, the
16-byte copy back), not the kernel alone.  Once, before the timed steps, the span filter's records are checked on the
device against the rule evaluated with torch on the unfiltered records.  Prints ONE JSON line and writes it to --out.

    python tools/spans_bench.py [--bytes N] [--steps 10] [--warmup 2] [--workload NAME ...] [--patterns NAME ...]
"""
import argparse
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phfpfac_amd import GpuMatcher, PfacTable  # noqa: E402
from split_bench import DATA, DELIM, WORKLOADS, line_block  # noqa: E402

PATTERNS = [("experimentpattern", ("experimentpattern",)), ("dictionary", ("xaa", "xab", "xac", "xad"))]
ANY = 0xFFFFFFFF
INF = 1 << 62


def drawn_rules(table, seed=7):
    """One rule per pattern id from {none, ^, $, ^$, (5, 25 - L, ANY)}, L the pattern's length."""
    lens = np.zeros(int(table.n_patterns) + 1, dtype=np.int64)
    lens[np.asarray(table.idmap)] = table.final_lengths()
    pick = np.random.default_rng(seed).integers(0, 5, lens.size)
    return [None] + [(None, "^", "$", "^$", (5, 25 - int(lens[i]), None))[pick[i]] for i in range(1, lens.size)]


def check_once(table, spans, buf, off, d_all, total, d_kept, kept):
    """On the device: the kept records are exactly the unfiltered ones the rule of include/pfac.h admits."""
    lens = torch.from_numpy(table.final_lengths().astype(np.int64)).cuda()
    lo_, hi_, tl_ = (torch.from_numpy(spans[k].astype(np.int64)).cuda() for k in ("min_start", "max_start", "max_tail"))
    off = torch.from_numpy(off.astype(np.int64)).cuda()
    at = 0
    step = 1 << 25
    for lo in range(0, total, step):
        part = d_all[lo:min(lo + step, total)]
        rec = part.view(torch.int32).view(-1, 2).to(torch.int64)
        pos, st = rec[:, 0].contiguous(), rec[:, 1].contiguous()
        d = torch.searchsorted(off, pos, right=True) - 1
        base, end = off[d], off[d + 1]
        cend = end - (buf[end - 1] == DELIM).long()
        pe = pos + lens[st]
        tail = torch.where(pe <= cend, cend - pe, torch.where(pe <= end, torch.zeros_like(pe), torch.full_like(pe, INF)))
        rel = pos - base
        keep = (rel >= lo_[st]) & (rel <= hi_[st]) & ((tl_[st] == ANY) | (tail <= tl_[st]))
        k = int(keep.sum())
        if at + k > kept or not torch.equal(part[keep], d_kept[at:at + k]):
            raise SystemExit("spans_bench: the filtered records differ from the rule applied to the unfiltered ones")
        at += k
    if at != kept:
        raise SystemExit(f"spans_bench: {kept} records kept, the rule keeps {at}")


def run(name, mean, pname, pats, n, steps, warmup, tmpdir):
    path = os.path.join(tmpdir, pname + ".pat")
    with open(path, "wb") as f:
        for p in pats:
            f.write(open(os.path.join(DATA, p), "rb").read())
    table = PfacTable.from_file(path, 256)
    rules = drawn_rules(table)
    block = line_block(mean, mean)
    stream = torch.cuda.Stream()                 # (not the null stream: a NULL handle would give the slot its own back)
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)      # the slot's work runs on this stream: its events bracket it
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_pattern_spans(rules)
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, block.tobytes())
        g.reserve(0, 0, max(n // 8, 1 << 20))
        total = g.scan_resident(n, n, d_input=buf)
        g.scan_resident(n, n, d_input=buf)        # (the staging mode has adapted to the workload)
        rec_bytes = g.scan_format()[0]
        n_docs, _ = g.split_documents(n, DELIM, d_input=buf)
        d_all = torch.empty(max(total, 1), dtype=torch.int64, device="cuda:0")
        g.expand_records(total, d_all)
        kept = g.filter_spans(delimiter=DELIM, n_docs=n_docs, d_input=buf)
        d_kept = torch.empty(max(kept, 1), dtype=torch.int64, device="cuda:0")
        g.expand_records(kept, d_kept)
        g.sync()
        check_once(table, table.state_spans(rules), buf, g.doc_offsets_to_host(n_docs), d_all, total, d_kept, kept)
        del d_kept
        d_first = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")     # (d_all takes the segment's records)

        def rescan():
            g.scan_async(n, n, d_input=buf)
            assert g.scan_finish(0)[0] == total

        ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        t = {k: [] for k in ("words", "spans", "line", "segment")}
        kept_words = kept_line = kept_seg = 0
        for step in range(warmup + steps):
            rescan()
            ev[0].record(stream)
            kept_words = g.filter_whole_words(n_docs=n_docs, d_input=buf)
            ev[1].record(stream)
            rescan()
            ev[2].record(stream)
            assert g.filter_spans(delimiter=DELIM, n_docs=n_docs, d_input=buf) == kept
            ev[3].record(stream)
            rescan()
            ev[4].record(stream)
            kept_line = g.filter_spans(delimiter=DELIM, line_match=True, n_docs=n_docs, d_input=buf)
            ev[5].record(stream)
            rescan()
            ev[6].record(stream)
            kept_seg = g.segment_records(n_docs, d_out=d_all, out_cap=total, d_doc_first=d_first)
            ev[7].record(stream)
            ev[7].synchronize()
            if step < warmup:
                continue
            for k, i in (("words", 0), ("spans", 2), ("line", 4), ("segment", 6)):
                t[k].append(ev[i].elapsed_time(ev[i + 1]))
        del buf, d_all, d_first
    torch.cuda.empty_cache()
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {
        "workload": name, "patterns": pname, "bytes": n, "mean_line_bytes": mean, "n_docs": n_docs, "record_bytes": rec_bytes,
        "num_final": int(table.num_final), "matches": total, "kept_spans": kept, "kept_line": kept_line,
        "kept_words": kept_words, "kept_segment": kept_seg,
        "filter_words_ms": round(med["words"], 3), "filter_spans_ms": round(med["spans"], 3),
        "filter_spans_line_ms": round(med["line"], 3), "segment_ms": round(med["segment"], 3),
        "filter_spans_ms_min": round(float(np.min(t["spans"])), 3), "filter_words_ms_min": round(float(np.min(t["words"])), 3),
        "spans_over_words": round(med["spans"] / med["words"], 3), "spans_over_segment": round(med["spans"] / med["segment"], 3),
        "line_over_words": round(med["line"] / med["words"], 3),
        "filter_spans_ns_per_record": round(med["spans"] * 1e6 / max(total, 1), 4),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    ap.add_argument("--patterns", action="append", default=None, help="only these pattern sets (repeatable)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spans_bench.json"))
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    out = {"metric": "pfac_records_filter_spans vs pfac_records_filter_words (with documents) and pfac_records_segment on the "
                     "same scan and the same line offsets",
           "steps": args.steps, "warmup": args.warmup,
           "ms_counts": "the whole call behind a fresh scan: memsets, the offsets' check, the kernel(s), the 16-byte copy back "
                        "(HIP events on the slot's stream); segment also writes 8 B per kept record into a caller's buffer",
           "rules": "per pattern from {none, ^, $, ^$, (5, 25 - L, ANY)}, seed 7; _line_: PFAC_SPANS_LINE",
           "workloads": []}
    with tempfile.TemporaryDirectory() as tmpdir:
        for name, mean in WORKLOADS:
            if args.workload and name not in args.workload:
                continue
            for pname, pats in PATTERNS:
                if args.patterns and pname not in args.patterns:
                    continue
                out["workloads"].append(run(name, mean, pname, pats, args.bytes, args.steps, args.warmup, tmpdir))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
