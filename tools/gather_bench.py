"""GPU measurement of the device-side gather of selected lines (pfac_documents_gather) against (a) a device-to-device
copy of the same out_bytes in the same run and (b) the host path for the same bytes.

For every workload: one resident input of --bytes (default 1 GiB) of text lines that end in '\\n' (the line blocks of
tools/split_bench.py), cut into lines on the device (pfac_slot_doc_offsets_split), and for every selection (every
100th line, every other line, every line: about 1 %, 50 % and 100 % of the lines) the ascending ids on the device.
HIP events on the slot's stream time the whole gather call into the caller's buffers (count and checks, group prefix,
the 16-byte copy back, the output offsets, the write) and a copy of out_bytes bytes between two device buffers; medians
over --steps steps after --warmup.  The gather also reads 16 B of offsets and writes 8 B per id, so its yardstick is
model_ms = (2 x out_bytes + 24 x n_ids) / the copy's rate.  The host path is what a caller does without the gather:
fetch the ids and the offsets, copy the input device-to-host, select the lines' bytes with numpy (a mask from the
selected lines' ends) -- wall clock, median of --host-steps.  The device output and its offsets are checked against the
host's once, before the timed steps.  Writes ONE JSON document to --out and prints it.

    python tools/gather_bench.py [--bytes N] [--steps 20] [--warmup 3] [--host-steps 1] [--out profiles/gather_bench.json]
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


def host_path(g, buf, n, n_docs, d_ids, n_ids):
    """(out, out_off, seconds): ids and offsets fetched, the input copied to the host, the lines selected with numpy."""
    t0 = time.perf_counter()
    ids = d_ids[:n_ids].cpu().numpy()
    off = g.doc_offsets_to_host(n_docs).astype(np.int64)
    host = buf[:n].cpu().numpy()
    marks = np.zeros(n + 1, dtype=np.int8)       # +1 where a selected line starts, -1 where one ends: ascending ids without
    ends = off[ids + 1]                          # repeats over non-empty lines, so neither index list holds a value twice
    marks[off[ids]] = 1
    marks[ends] -= 1                             # (a line's end may be the next one's start: the two cancel)
    out = host[np.cumsum(marks[:-1], dtype=np.int8) > 0]
    out_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(ends - off[ids])]).astype(np.uint64)
    return out, out_off, time.perf_counter() - t0


def run(name, mean, n, steps, warmup, host_steps):
    block = line_block(mean, mean)
    stream = torch.cuda.Stream()                 # (not the null stream: a NULL handle would give the slot its own back)
    rows = []
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)      # the slot's work runs on this stream: its events bracket it
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, block.tobytes())
        n_docs, _ = g.split_documents(n, DELIM, d_input=buf)
        g.sync()
        for sel, step_ids in SELECTIONS:
            d_ids = torch.arange(0, n_docs, step_ids, dtype=torch.int64, device="cuda:0")
            n_ids = int(d_ids.numel())
            d_off = torch.empty(n_ids + 1, dtype=torch.int64, device="cuda:0")
            stream.synchronize()
            out_bytes = g.gather_documents(n_docs, n_ids, n, d_input=buf, d_ids=d_ids, d_out_offsets=d_off)   # (sizes the output)
            d_out = torch.empty(out_bytes + 16, dtype=torch.uint8, device="cuda:0")
            d_src = torch.empty(out_bytes + 16, dtype=torch.uint8, device="cuda:0")
            stream.synchronize()
            args = dict(d_input=buf, d_ids=d_ids, d_out=d_out, out_cap=out_bytes, d_out_offsets=d_off)
            assert g.gather_documents(n_docs, n_ids, n, **args) == out_bytes
            g.sync()
            host_s = []
            for step in range(host_steps):
                want, want_off, s = host_path(g, buf, n, n_docs, d_ids, n_ids)
                host_s.append(s)
            if not (want.size == out_bytes and np.array_equal(d_off.cpu().numpy().view(np.uint64), want_off)
                    and np.array_equal(d_out[:out_bytes].cpu().numpy(), want)):
                raise SystemExit(f"gather_bench: {name} {sel}: the device output differs from the host's")
            del want, want_off
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            gather_ms, copy_ms = [], []
            for step in range(warmup + steps):
                ev[0].record(stream)
                assert g.gather_documents(n_docs, n_ids, n, **args) == out_bytes
                ev[1].record(stream)
                ev[2].record(stream)
                d_src[:out_bytes].copy_(d_out[:out_bytes])
                ev[3].record(stream)
                ev[3].synchronize()
                if step >= warmup:
                    gather_ms.append(ev[0].elapsed_time(ev[1]))
                    copy_ms.append(ev[2].elapsed_time(ev[3]))
            med = lambda x: float(np.median(x))  # noqa: E731
            ga, cp, hs = med(gather_ms), med(copy_ms), med(host_s) * 1e3
            copy_rate = 2 * out_bytes / (cp * 1e-3)                      # bytes moved per second by the copy (read + write)
            model = (2 * out_bytes + 24 * n_ids) / copy_rate * 1e3
            rows.append({
                "workload": name, "selection": sel, "bytes": n, "mean_line_bytes": mean, "n_docs": n_docs, "n_ids": n_ids,
                "out_bytes": out_bytes, "gather_ms": round(ga, 3), "gather_ms_min": round(float(np.min(gather_ms)), 3),
                "copy_ms": round(cp, 3), "copy_gbs": round(copy_rate / 1e9, 1), "model_ms": round(model, 3),
                "gather_over_copy": round(ga / cp, 2), "gather_over_model": round(ga / model, 2),
                "gather_gbs": round((2 * out_bytes + 24 * n_ids) / (ga * 1e-3) / 1e9, 1),
                "host_path_ms": round(hs, 1), "host_path_over_gather": round(hs / ga, 1),
            })
            del d_ids, d_off, d_out, d_src
            torch.cuda.empty_cache()
        del buf
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=1, help="timed repetitions of the host path")
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gather_bench.json"))
    args = ap.parse_args()
    if args.steps < 1 or args.host_steps < 1:
        raise SystemExit("--steps and --host-steps must be >= 1")
    out = {"metric": "pfac_documents_gather vs a device-to-device copy of out_bytes in the same run, and vs the host path "
                     "(ids, offsets and the input fetched, the lines selected with numpy)",
           "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps,
           "gather_ms_counts": "the whole call into the caller's buffers: count and checks, group prefix, the 16-byte copy back, "
                               "the output offsets, the write (HIP events)",
           "model_ms_counts": "(2 x out_bytes + 24 x n_ids) / the copy's rate: the bytes read and written, 16 B of offsets read and "
                              "8 B written per id",
           "host_path_ms_counts": "wall clock: D2H of the ids, the offsets and the input, a numpy mask over the input",
           "rows": []}
    for name, mean in WORKLOADS:
        if args.workload and name not in args.workload:
            continue
        out["rows"] += run(name, mean, args.bytes, args.steps, args.warmup, args.host_steps)
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
