"""GPU measurement of find-and-replace over the leftmost-longest selection (pfac_replace_leftmost_longest) against a
plain device-to-device copy of the same input.

For every workload: one resident input of --bytes (default 1 GiB); each step scans it, selects the leftmost-longest
matches (select), rewrites the input with every pick replaced (replace: the count kernel, the group prefix, the copy of
the output length to the host and the write kernel) and copies the n_owned input bytes to the output buffer with one
D2D copy on the same stream (the floor for the same read and write traffic).  HIP events on the slot's stream time each
part; medians over --steps steps after --warmup.  Once, before the timed steps, the head of the output is checked on
the host against tests/replref.splice of the device's selection.  Prints ONE JSON line.

    python tools/replace_bench.py [--bytes N] [--steps 20] [--warmup 3] [--workload NAME ...]
"""
import argparse
import gzip
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phfpfac_amd import GpuMatcher, PfacError, PfacTable  # noqa: E402
from replref import rep_table, splice  # noqa: E402

DATA = os.path.join(REPO, "tests", "golden", "data")
SEED = 0x5048465046414331
WORKLOADS = [  # name, pattern source, input kind, replacements
    ("text_experimentpattern", "experimentpattern", "text", "random"),
    ("rand_snort75k", "bytefile_1000000byte.gz", "rand", "random"),
    ("aa_runs_delete", "aa", "runs", "delete"),
    ("text_no_match", "nomatch", "text", "random"),
]
CHECK_BYTES = 64 << 20


def pattern_path(name, tmpdir):
    if name.endswith(".gz"):
        p = os.path.join(tmpdir, name[:-3])
        if not os.path.exists(p):
            with gzip.open(os.path.join(DATA, name), "rb") as g, open(p, "wb") as f:
                f.write(g.read())
        return p
    if name in ("aa", "nomatch"):
        p = os.path.join(tmpdir, name + ".pat")
        open(p, "wb").write(b"aa\n" if name == "aa" else b"\x01\x02\x03\n")
        return p
    return os.path.join(DATA, name)


def fill(g, buf, n, kind):
    if kind == "text":
        g.fill_tiled(buf, n, open(os.path.join(DATA, "paragraph402"), "rb").read())
    elif kind == "rand":
        g.fill_random(buf, (n + 7) // 8 * 8, SEED)
    else:                                                   # runs of 100 003 `a`, one `b` between them
        g.fill_tiled(buf, n, b"a" * 100003 + b"b")


def replacements(table, path, how):
    n_ids = sum(1 for _ in open(path, "rb"))
    if how == "delete":
        return {i: b"" for i in range(1, n_ids + 1)}
    rng = np.random.default_rng(SEED & 0xFFFFFFFF)
    return {i: bytes(rng.integers(0x41, 0x5B, int(rng.integers(0, 17))).astype(np.uint8)) for i in range(1, n_ids + 1)}


def check_once(table, reps, buf, n, n_sel, d_sel, d_out, n_out):
    """The output's head against the host splice of the device's selection: the picks before the first one at or after
    CHECK_BYTES (m: that pick's position) give exactly the output of input[0, m)."""
    pos_dev = d_sel[:n_sel].view(torch.int32).view(-1, 2)[:, 0].to(torch.int64)
    j = int(torch.searchsorted(pos_dev, torch.tensor([CHECK_BYTES], device=pos_dev.device))[0]) if n_sel else 0
    m = int(pos_dev[j]) if j < n_sel else n
    sel = d_sel[:j].view(torch.int32).view(-1, 2).cpu().numpy().astype(np.int64)
    lens = table.final_lengths().astype(np.int64)
    pos, st = sel[:, 0], sel[:, 1]
    want = splice(buf[:m].cpu().numpy(), 0, m, pos, lens[st], table.idmap[st].astype(np.int64), rep_table(reps))
    if want.size > n_out or not np.array_equal(d_out[:want.size].cpu().numpy(), want):
        raise SystemExit("replace_bench: the output differs from the host splice of the selection")


def run(name, pat, kind, how, n, steps, warmup, tmpdir):
    path = pattern_path(pat, tmpdir)
    table = PfacTable.from_file(path, 256)
    reps = replacements(table, path, how)
    stream = torch.cuda.Stream()                 # (not the null stream: a NULL handle would give the slot its own back)
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_replacements(reps)
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        fill(g, buf, n, kind)
        g.reserve(0, 0, max(n // 8, 1 << 20) if kind != "runs" else n + n // 8)
        total = g.scan_resident(n, n, d_input=buf)
        g.scan_resident(n, n, d_input=buf)        # (the staging mode has adapted to the workload)
        d_sel = torch.empty(max(total, 1), dtype=torch.int64, device="cuda:0")
        n_sel, ex = g.select_leftmost_longest(0, d_out=d_sel, out_cap=total)
        try:
            n_out = g.replace_selection(d_input=buf, d_sel=d_sel, d_out=buf, out_cap=0)
        except PfacError as e:                   # (a zero out_cap only asks for the length)
            n_out = e.out_bytes
        d_out = torch.empty(max(n_out, n) + 4096, dtype=torch.uint8, device="cuda:0")
        assert g.replace_selection(d_input=buf, d_sel=d_sel, d_out=d_out, out_cap=d_out.numel()) == n_out
        g.sync()
        check_once(table, reps, buf, n, n_sel, d_sel, d_out, n_out)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        scan_ms, sel_ms, rep_ms, copy_ms = [], [], [], []
        for step in range(warmup + steps):
            ev[0].record(stream)
            g.scan_async(n, n, d_input=buf)
            assert g.scan_finish(0)[0] == total
            ev[1].record(stream)
            assert g.select_leftmost_longest(0, d_out=d_sel, out_cap=total) == (n_sel, ex)
            ev[2].record(stream)
            assert g.replace_selection(d_input=buf, d_sel=d_sel, d_out=d_out, out_cap=d_out.numel()) == n_out
            ev[3].record(stream)
            d_out[:n].copy_(buf[:n])
            ev[4].record(stream)
            ev[4].synchronize()
            if step < warmup:
                continue
            scan_ms.append(ev[0].elapsed_time(ev[1]))
            sel_ms.append(ev[1].elapsed_time(ev[2]))
            rep_ms.append(ev[2].elapsed_time(ev[3]))
            copy_ms.append(ev[3].elapsed_time(ev[4]))
        del buf, d_sel, d_out
    torch.cuda.empty_cache()
    rep, cp = float(np.median(rep_ms)), float(np.median(copy_ms))
    return {
        "workload": name, "bytes": n, "matches": total, "selected": n_sel, "out_bytes": n_out,
        "scan_ms": round(float(np.median(scan_ms)), 3), "select_ms": round(float(np.median(sel_ms)), 3),
        "replace_ms": round(rep, 3), "d2d_copy_ms": round(cp, 3), "replace_over_copy": round(rep / cp, 3),
        "replace_ns_per_pick": round(rep * 1e6 / n_sel, 4) if n_sel else None,
        "replace_ms_min": round(float(np.min(rep_ms)), 3), "d2d_copy_ms_min": round(float(np.min(copy_ms)), 3),
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
    out = {"metric": "find-and-replace over the leftmost-longest selection (pfac_replace_leftmost_longest) vs a D2D copy "
                     "of the input", "steps": args.steps, "warmup": args.warmup, "workloads": []}
    with tempfile.TemporaryDirectory() as tmpdir:
        for name, pat, kind, how in WORKLOADS:
            if args.workload and name not in args.workload:
                continue
            out["workloads"].append(run(name, pat, kind, how, args.bytes, args.steps, args.warmup, tmpdir))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
