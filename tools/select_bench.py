"""GPU measurement of leftmost-longest selection (pfac_records_leftmost_longest) against pfac_records_expand of the same
scan.

For every workload: one resident input of --bytes (default 1 GiB); each step scans it, then selects the leftmost-longest
non-overlapping matches (select) and expands the same scan into one sorted pfac_record array (expand), in alternating
order.  HIP events on the slot's stream time the scan, the whole select call (tile functions, group composition,
marking, group prefix, the copy of the count and exit to the host, write) and the expand call (group sums, prefix,
copy); medians over --steps steps after --warmup.  Once, before the timed steps, the selection is checked on the device
to be ascending, non-overlapping and a subset of the expand output.  Prints ONE JSON line.

    python tools/select_bench.py [--bytes N] [--steps 20] [--warmup 3] [--workload NAME ...]
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
LONG_SEED = 20261016
WORKLOADS = [  # name, pattern source, input kind
    ("text_experimentpattern", "experimentpattern", "text"),
    ("rand_snort75k", "bytefile_1000000byte.gz", "rand"),
    ("aa_runs", "aa", "runs"),
    ("long_m1000", "long", "long"),
]


def long_base():
    """A random 65 521-byte string over a..d; the long-pattern set is cut from it and the input tiled from it."""
    return np.random.default_rng(LONG_SEED).integers(97, 101, 65521).astype(np.uint8)


def pattern_path(name, tmpdir):
    if name.endswith(".gz"):
        p = os.path.join(tmpdir, name[:-3])
        if not os.path.exists(p):
            with gzip.open(os.path.join(DATA, name), "rb") as g, open(p, "wb") as f:
                f.write(g.read())
        return p
    if name == "aa":
        p = os.path.join(tmpdir, "aa.pat")
        open(p, "wb").write(b"aa\n")
        return p
    if name == "long":                                      # 64 patterns of 900 to 1 000 bytes: max_pat_len near 1 000
        base, rng = long_base(), np.random.default_rng(LONG_SEED + 1)
        lines = []
        for _ in range(64):
            L = int(rng.integers(900, 1001))
            s = int(rng.integers(0, base.size - L))
            lines.append(base[s:s + L].tobytes() + b"\n")
        p = os.path.join(tmpdir, "long.pat")
        open(p, "wb").write(b"".join(lines))
        return p
    return os.path.join(DATA, name)


def fill(g, buf, n, kind):
    if kind == "text":
        g.fill_tiled(buf, n, open(os.path.join(DATA, "paragraph402"), "rb").read())
    elif kind == "rand":
        g.fill_random(buf, (n + 7) // 8 * 8, SEED)
    elif kind == "runs":                                    # runs of 100 003 `a`, one `b` between them
        g.fill_tiled(buf, n, b"a" * 100003 + b"b")
    else:
        g.fill_tiled(buf, n, long_base().tobytes())


def check_once(table, total, n_sel, d_sel, d_exp):
    """On the device: the selection ascends, does not overlap, and every pick is a record of the scan."""
    sel = d_sel[:n_sel].view(torch.int32).view(-1, 2).to(torch.int64)
    lens = torch.from_numpy(table.final_lengths().astype(np.int64)).cuda()
    pos, st = sel[:, 0], sel[:, 1]
    ok = bool((pos[1:] >= pos[:-1] + lens[st[:-1]]).all()) if n_sel > 1 else True
    whole = d_exp[:total].view(torch.int32).view(-1, 2).to(torch.int64)
    key = whole[:, 0] * (1 << 24) + whole[:, 1]
    skey = pos * (1 << 24) + st
    at = torch.searchsorted(key, skey).clamp(max=max(total - 1, 0))
    ok = ok and bool((key[at] == skey).all())
    if not ok:
        raise SystemExit("select_bench: the selection is not an ascending non-overlapping subset of the scan")


def run(name, pat, kind, n, steps, warmup, tmpdir):
    table = PfacTable.from_file(pattern_path(pat, tmpdir), 256)
    stream = torch.cuda.Stream()                 # (not the null stream: a NULL handle would give the slot its own back)
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)      # the slot's work runs on this stream: its events bracket it
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        fill(g, buf, n, kind)
        g.reserve(0, 0, max(n // 8, 1 << 20) if kind != "runs" else n + n // 8)
        total = g.scan_resident(n, n, d_input=buf)
        g.scan_resident(n, n, d_input=buf)        # (the staging mode has adapted to the workload)
        rec_bytes, n_tiles, used = g.scan_format()
        d_exp = torch.empty(max(total, 1), dtype=torch.int64, device="cuda:0")
        d_sel = torch.empty(max(total, 1), dtype=torch.int64, device="cuda:0")
        n_sel, ex = g.select_leftmost_longest(0, d_out=d_sel, out_cap=total)
        g.expand_records(total, d_exp)
        g.sync()
        check_once(table, total, n_sel, d_sel, d_exp)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        scan_ms, sel_ms, exp_ms = [], [], []
        for step in range(warmup + steps):
            ev[0].record(stream)
            g.scan_async(n, n, d_input=buf)
            ev[1].record(stream)
            assert g.scan_finish(0)[0] == total
            ev[2].record(stream)
            if step % 2 == 0:
                assert g.select_leftmost_longest(0, d_out=d_sel, out_cap=total) == (n_sel, ex)
                ev[3].record(stream)
                g.expand_records(total, d_exp)
                ev[4].record(stream)
            else:
                g.expand_records(total, d_exp)
                ev[3].record(stream)
                assert g.select_leftmost_longest(0, d_out=d_sel, out_cap=total) == (n_sel, ex)
                ev[4].record(stream)
            ev[4].synchronize()
            if step < warmup:
                continue
            scan_ms.append(ev[0].elapsed_time(ev[1]))
            a, b = ev[2].elapsed_time(ev[3]), ev[3].elapsed_time(ev[4])
            sel_ms.append(a if step % 2 == 0 else b)
            exp_ms.append(b if step % 2 == 0 else a)
        del buf, d_exp, d_sel
    torch.cuda.empty_cache()
    sel, exp, scan = float(np.median(sel_ms)), float(np.median(exp_ms)), float(np.median(scan_ms))
    return {
        "workload": name, "bytes": n, "max_pat_len": table.max_pat_len, "record_bytes": rec_bytes,
        "matches": total, "selected": n_sel, "exit": ex, "scan_ms": round(scan, 3), "select_ms": round(sel, 3),
        "expand_ms": round(exp, 3), "select_over_expand": round(sel / exp, 3),
        "select_ns_per_record": round(sel * 1e6 / max(total, 1), 4),
        "select_ms_min": round(float(np.min(sel_ms)), 3), "expand_ms_min": round(float(np.min(exp_ms)), 3),
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
    out = {"metric": "leftmost-longest selection (pfac_records_leftmost_longest) vs pfac_records_expand of the same scan",
           "steps": args.steps, "warmup": args.warmup, "workloads": []}
    with tempfile.TemporaryDirectory() as tmpdir:
        for name, pat, kind in WORKLOADS:
            if args.workload and name not in args.workload:
                continue
            out["workloads"].append(run(name, pat, kind, args.bytes, args.steps, args.warmup, tmpdir))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
