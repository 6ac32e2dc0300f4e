"""GPU measurement of the whole-word filter (pfac_records_filter_words) against pfac_records_expand of the same,
unfiltered scan, and of what it does to the passes behind it.

For every workload: one resident input of --bytes (default 1 GiB), redaction replacements.  Each step runs, with HIP
events on the slot's stream around every call:

    scan, expand (the unfiltered scan -> one sorted pfac_record array: the existing reader of the same heap bytes),
    filter (the whole call: the 16-byte memset, the kernel, the copy of the count to the host),
    select + replace over the filtered scan;
    then scan, select + replace without the filter.

Medians over --steps steps after --warmup.  `filter_call_ms` is the whole pfac_records_filter_words call, not the kernel
alone (a `rocprofv3 --kernel-trace --stats -- python tools/words_bench.py` run gives the kernel's own time).  Once, before the timed steps, the filtered records are checked on
the device against the rule evaluated with torch on the unfiltered expand output.  Prints ONE JSON line.

    python tools/words_bench.py [--bytes N] [--steps 10] [--warmup 2] [--workload NAME ...]
"""
import argparse
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
WORKLOADS = [  # name, pattern files
    ("text_dictionary", ("xaa", "xab", "xac", "xad")),
    ("text_experimentpattern", ("experimentpattern",)),       # bench.py's headline workload
]
WORD = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ_abcdefghijklmnopqrstuvwxyz"


def check_once(table, buf, n, d_all, total, d_kept, kept):
    """On the device: the kept records are exactly the unfiltered ones whose ends do not split a word."""
    lens = torch.from_numpy(table.final_lengths().astype(np.int64)).cuda()
    isw = torch.zeros(256, dtype=torch.bool, device="cuda:0")
    isw[torch.from_numpy(np.frombuffer(WORD, dtype=np.uint8).astype(np.int64)).cuda()] = True
    want = 0
    step = 1 << 26
    got = d_kept[:kept]
    at = 0
    for lo in range(0, total, step):
        rec = d_all[lo:min(lo + step, total)].view(torch.int32).view(-1, 2).to(torch.int64)
        pos, st = rec[:, 0], rec[:, 1]
        end = pos + lens[st]
        lcut = (pos > 0) & isw[buf[(pos - 1).clamp(min=0)].long()] & isw[buf[pos].long()]
        rcut = (end < n) & isw[buf[end - 1].long()] & isw[buf[end.clamp(max=n - 1)].long()]
        keep = ~lcut & ~rcut
        k = int(keep.sum())
        if not torch.equal(d_all[lo:min(lo + step, total)][keep], got[at:at + k]):
            raise SystemExit("words_bench: the filtered records differ from the rule applied to the unfiltered ones")
        at += k
        want += k
    if want != kept:
        raise SystemExit(f"words_bench: {kept} records kept, the rule keeps {want}")


def run(name, pats, n, steps, warmup, tmpdir):
    path = os.path.join(tmpdir, name + ".pat")
    with open(path, "wb") as f:
        for p in pats:
            f.write(open(os.path.join(DATA, p), "rb").read())
    table = PfacTable.from_file(path, 256)
    stream = torch.cuda.Stream()
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_redaction(b"*")
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, open(os.path.join(DATA, "paragraph402"), "rb").read())
        g.reserve(0, 0, max(n // 8, 1 << 20))
        total = g.scan_resident(n, n, d_input=buf)
        g.scan_resident(n, n, d_input=buf)        # (the staging mode has adapted to the workload)
        rec_bytes, n_tiles, used = g.scan_format()
        d_exp = torch.empty(max(total, 1), dtype=torch.int64, device="cuda:0")
        g.expand_records(total, d_exp)
        kept = g.filter_whole_words(d_input=buf)
        d_kept = torch.empty(max(kept, 1), dtype=torch.int64, device="cuda:0")
        g.expand_records(kept, d_kept)
        g.sync()
        check_once(table, buf, n, d_exp, total, d_kept, kept)
        del d_kept
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(9)]
        t = {k: [] for k in ("scan", "expand", "filter", "passes_filtered", "with_filter", "passes_plain", "without_filter")}
        sel_f = sel_p = out_f = out_p = 0
        for step in range(warmup + steps):
            ev[0].record(stream)
            g.scan_async(n, n, d_input=buf)
            ev[1].record(stream)
            assert g.scan_finish(0)[0] == total
            ev[2].record(stream)
            g.expand_records(total, d_exp)
            ev[3].record(stream)
            assert g.filter_whole_words(d_input=buf) == kept
            ev[4].record(stream)
            sel_f, _ = g.select_leftmost_longest(0)
            out_f = g.replace_selection(d_input=buf)
            ev[5].record(stream)
            ev[5].synchronize()
            ev[6].record(stream)
            g.scan_async(n, n, d_input=buf)
            assert g.scan_finish(0)[0] == total
            ev[7].record(stream)
            sel_p, _ = g.select_leftmost_longest(0)
            out_p = g.replace_selection(d_input=buf)
            ev[8].record(stream)
            ev[8].synchronize()
            if step < warmup:
                continue
            scan = ev[0].elapsed_time(ev[1])
            t["scan"].append(scan)
            t["expand"].append(ev[2].elapsed_time(ev[3]))
            t["filter"].append(ev[3].elapsed_time(ev[4]))
            t["passes_filtered"].append(ev[4].elapsed_time(ev[5]))
            t["with_filter"].append(scan + ev[3].elapsed_time(ev[5]))
            t["passes_plain"].append(ev[7].elapsed_time(ev[8]))
            t["without_filter"].append(ev[6].elapsed_time(ev[8]))
        del buf, d_exp
    torch.cuda.empty_cache()
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {
        "workload": name, "bytes": n, "record_bytes": rec_bytes, "matches": total, "kept": kept,
        "selected_filtered": sel_f, "selected_plain": sel_p, "out_bytes_filtered": out_f, "out_bytes_plain": out_p,
        "scan_ms": round(med["scan"], 3), "expand_unfiltered_ms": round(med["expand"], 3),
        "filter_call_ms": round(med["filter"], 3), "filter_call_ms_min": round(float(np.min(t["filter"])), 3),
        "filter_over_expand": round(med["filter"] / med["expand"], 3),
        "filter_ns_per_record": round(med["filter"] * 1e6 / max(total, 1), 4),
        "select_replace_after_filter_ms": round(med["passes_filtered"], 3),
        "select_replace_unfiltered_ms": round(med["passes_plain"], 3),
        "scan_filter_select_replace_ms": round(med["with_filter"], 3),
        "scan_select_replace_ms": round(med["without_filter"], 3),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    out = {"metric": "whole-word filter (pfac_records_filter_words) vs pfac_records_expand of the same unfiltered scan; "
                     "scan + filter + selection + replace vs scan + selection + replace",
           "steps": args.steps, "warmup": args.warmup, "workloads": []}
    with tempfile.TemporaryDirectory() as tmpdir:
        for name, pats in WORKLOADS:
            if args.workload and name not in args.workload:
                continue
            out["workloads"].append(run(name, pats, args.bytes, args.steps, args.warmup, tmpdir))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
