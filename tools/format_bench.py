"""GPU measurement of the gather with labels (pfac_documents_gather_format: grep -n, -b, the "--" lines, the final
newline) against the plain gather of the same ids in the same run, and against the host path the call replaces.

For every workload: one resident input of --bytes (default 1 GiB) of text lines that end in '\\n' (the line blocks of
tools/split_bench.py), cut into lines on the device, and for every selection (every 100th line, every other line, every
line) the ascending ids on the device.  HIP events on the slot's stream time the whole call into the caller's buffers
(count and checks, group prefix, the 16-byte copy back, the output offsets, the write) for the plain gather and for three
formats -- "n" (line numbers), "nb" (numbers and byte offsets) and "all" (both, the terminator, the context separator
from a doc_first in which every third line holds a record, and "--\\n" between lines that are not adjacent) -- one after
the other in every step; medians over --steps steps after --warmup.

The host path is what a caller does without the call: the plain gather's bytes, offsets and ids fetched, then one Python
loop that puts the labels in front of every line (b"%d" and b"".join).  It runs on the first --check-bytes of the input
(the loop takes about a microsecond per line and byte-sized work on top; a GiB of 16-byte lines would take minutes), is
timed there, and its time per line is scaled to the selection's line count: host_path_ms is that estimate.  The same
loop's output is the check: every format's device output and offsets on the first --check-bytes are compared with it
byte for byte before anything is timed, and at the full size out_bytes and the offsets are checked against the label
lengths computed with numpy.  Writes ONE JSON document to --out and prints it.

    python tools/format_bench.py [--bytes N] [--steps 20] [--warmup 3] [--check-bytes N] [--out profiles/format_bench.json]
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

from phfpfac_amd import GpuMatcher  # noqa: E402
from split_bench import DELIM, WORKLOADS, line_block  # noqa: E402

SELECTIONS = [("every_100th", 100), ("every_other", 2), ("all", 1)]
FORMATS = [("n", dict(number=True)), ("nb", dict(number=True, byte_offset=True)),
           ("all", dict(number=True, byte_offset=True, terminate=DELIM, context_sep=True, group_sep=b"--\n"))]


def host_format(out, out_off, ids, off, kw):
    """The host path's loop: labels in front of every gathered line.  `off`: the selected lines' offsets in the input."""
    data = out.tobytes()
    number, offset, term, ctx, sep = (kw.get(k) for k in ("number", "byte_offset", "terminate", "context_sep", "group_sep"))
    nl = bytes([term]) if term is not None else b""
    pieces, prev = [], None
    for k, i in enumerate(ids.tolist()):
        line = data[out_off[k]:out_off[k + 1]]
        c = b"-" if ctx and i % 3 else b":"
        s = sep if sep and prev is not None and i != prev + 1 else b""
        if number:
            s += b"%d" % (i + 1) + c
        if offset:
            s += b"%d" % off[k] + c
        s += line
        if nl and not line.endswith(nl):
            s += nl
        pieces.append(s)
        prev = i
    return pieces


POW10 = np.array([10 ** k for k in range(1, 19)], dtype=np.int64)


def ndigits(v):
    return 1 + np.searchsorted(POW10, v, side="right")


def want_offsets(ids, off, n_bytes_last_unterminated, kw):
    """out_off of a format over terminated lines (only the input's last line may lack its newline), with numpy."""
    lo, hi = off[ids], off[ids + 1]
    seg = hi - lo
    if kw.get("number"):
        seg = seg + ndigits(ids + 1) + 1
    if kw.get("byte_offset"):
        seg = seg + ndigits(lo) + 1
    if kw.get("group_sep"):
        seg[1:] += (ids[1:] != ids[:-1] + 1) * len(kw["group_sep"])
    if kw.get("terminate") is not None and n_bytes_last_unterminated and ids.size and ids[-1] == off.size - 2:
        seg[-1] += 1
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(seg)]).astype(np.uint64)


def check_prefix(g, buf, n_chk, name):
    """Every selection and format on the first n_chk bytes against the host loop; -> {selection: {format: seconds per
    line of the host path}} (the plain gather's fetch included)."""
    n_docs, _ = g.split_documents(n_chk, DELIM, d_input=buf)
    off = g.doc_offsets_to_host(n_docs).astype(np.int64)
    d_first = ((torch.arange(0, n_docs + 1, dtype=torch.int64, device="cuda:0") + 2) // 3).contiguous()
    per_line = {}
    for sel, step in SELECTIONS:
        d_ids = torch.arange(0, n_docs, step, dtype=torch.int64, device="cuda:0")
        n_ids = int(d_ids.numel())
        torch.cuda.current_stream().synchronize()
        per_line[sel] = {}
        g.gathered_to_host(g.gather_documents(n_docs, n_ids, n_chk, d_input=buf, d_ids=d_ids))    # (untimed: the buffers grow here)
        for fname, kw in FORMATS:
            t0 = time.perf_counter()
            nb = g.gather_documents(n_docs, n_ids, n_chk, d_input=buf, d_ids=d_ids)
            out, out_off = g.gathered_to_host(nb), g.gathered_offsets_to_host(n_ids).astype(np.int64)
            ids = d_ids.cpu().numpy()
            pieces = host_format(out, out_off.tolist(), ids, off[ids].tolist(), kw)
            want = b"".join(pieces)
            per_line[sel][fname] = (time.perf_counter() - t0) / max(n_ids, 1)
            n = g.gather_documents_formatted(n_docs, n_ids, n_chk, d_input=buf, d_ids=d_ids, d_doc_first=d_first, **kw)
            got, got_off = g.gathered_to_host(n), g.gathered_offsets_to_host(n_ids)
            want_off = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.uint64)
            if not (n == len(want) and np.array_equal(got_off, want_off) and got.tobytes() == want):
                raise SystemExit(f"format_bench: {name} {sel} {fname}: the device output differs from the host's")
        del d_ids
    return per_line


def run(name, mean, n, steps, warmup, n_chk):
    block = line_block(mean, mean)
    stream = torch.cuda.Stream()                 # (not the null stream: a NULL handle would give the slot its own back)
    rows = []
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)      # the slot's work runs on this stream: its events bracket it
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, block.tobytes())
        g.sync()
        per_line = check_prefix(g, buf, min(n, n_chk), name)
        n_docs, tail = g.split_documents(n, DELIM, d_input=buf)
        off = g.doc_offsets_to_host(n_docs).astype(np.int64)
        d_first = ((torch.arange(0, n_docs + 1, dtype=torch.int64, device="cuda:0") + 2) // 3).contiguous()
        for sel, step_ids in SELECTIONS:
            d_ids = torch.arange(0, n_docs, step_ids, dtype=torch.int64, device="cuda:0")
            n_ids = int(d_ids.numel())
            ids = d_ids.cpu().numpy()
            d_off = torch.empty(n_ids + 1, dtype=torch.int64, device="cuda:0")
            stream.synchronize()
            calls = [("plain", None)] + FORMATS
            sizes = {}
            for fname, kw in calls:              # size the outputs, check the counts and the offsets
                common = dict(d_input=buf, d_ids=d_ids, d_out_offsets=d_off)
                if kw is None:
                    sizes[fname] = g.gather_documents(n_docs, n_ids, n, **common)
                else:
                    sizes[fname] = g.gather_documents_formatted(n_docs, n_ids, n, d_doc_first=d_first, **common, **kw)
                g.sync()
                want_off = want_offsets(ids, off, tail < n, kw or {})
                if sizes[fname] != int(want_off[-1]) or not np.array_equal(d_off.cpu().numpy().view(np.uint64), want_off):
                    raise SystemExit(f"format_bench: {name} {sel} {fname}: out_bytes or the offsets differ from the host's")
                del want_off
            d_out = torch.empty(max(sizes.values()) + 16, dtype=torch.uint8, device="cuda:0")
            stream.synchronize()
            ms = {fname: [] for fname, _ in calls}
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * len(calls))]
            for step in range(warmup + steps):
                for j, (fname, kw) in enumerate(calls):
                    args = dict(d_input=buf, d_ids=d_ids, d_out=d_out, out_cap=sizes[fname], d_out_offsets=d_off)
                    ev[2 * j].record(stream)
                    if kw is None:
                        got = g.gather_documents(n_docs, n_ids, n, **args)
                    else:
                        got = g.gather_documents_formatted(n_docs, n_ids, n, d_doc_first=d_first, **args, **kw)
                    ev[2 * j + 1].record(stream)
                    assert got == sizes[fname]
                ev[-1].synchronize()
                if step >= warmup:
                    for j, (fname, _) in enumerate(calls):
                        ms[fname].append(ev[2 * j].elapsed_time(ev[2 * j + 1]))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            row = {"workload": name, "selection": sel, "bytes": n, "mean_line_bytes": mean, "n_docs": n_docs, "n_ids": n_ids,
                   "plain_out_bytes": sizes["plain"], "plain_ms": round(med["plain"], 3),
                   "plain_ms_min": round(float(np.min(ms["plain"])), 3)}
            for fname, _ in FORMATS:
                host_ms = per_line[sel][fname] * n_ids * 1e3
                row.update({
                    f"{fname}_out_bytes": sizes[fname], f"{fname}_ms": round(med[fname], 3),
                    f"{fname}_ms_min": round(float(np.min(ms[fname])), 3),
                    f"{fname}_over_plain": round(med[fname] / med["plain"], 2),
                    f"{fname}_added_bytes_per_line": round((sizes[fname] - sizes["plain"]) / max(n_ids, 1), 2),
                    f"{fname}_gbs": round((sizes["plain"] + sizes[fname] + 24 * n_ids) / (med[fname] * 1e-3) / 1e9, 1),
                    f"{fname}_host_path_ms": round(host_ms, 1), f"{fname}_host_path_over_call": round(host_ms / med[fname], 1),
                })
            rows.append(row)
            del d_ids, d_off, d_out
            torch.cuda.empty_cache()
        del buf
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check-bytes", type=int, default=(4 << 20) + 5, help="the prefix the host loop runs on (checked and timed)")
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "format_bench.json"))
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    out = {"metric": "pfac_documents_gather_format (-n; -n -b; all flags) vs pfac_documents_gather of the same ids in the same run, "
                     "and vs the host path (the plain gather fetched, the labels put in by a Python loop)",
           "steps": args.steps, "warmup": args.warmup, "check_bytes": args.check_bytes,
           "ms_counts": "the whole call into the caller's buffers: count and checks, group prefix, the 16-byte copy back, the "
                        "output offsets, the write (HIP events)",
           "gbs_counts": "(the bodies read + the output written + 24 B per id) / the call's time",
           "host_path_ms_counts": "wall clock on the first check_bytes (the plain gather, its three fetches, the Python loop), per "
                                  "line, times the selection's lines: an estimate, not a run at the full size",
           "rows": []}
    for name, mean in WORKLOADS:
        if args.workload and name not in args.workload:
            continue
        out["rows"] += run(name, mean, args.bytes, args.steps, args.warmup, args.check_bytes)
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
