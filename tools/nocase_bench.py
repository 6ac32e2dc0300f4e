"""GPU measurement of the case-insensitive scan (pfac_table_set_case_fold): what the fold inside the scan kernel costs,
and what the alternatives a user had before it cost.

For every workload: one resident input of --bytes (default 1 GiB) and the table of the FOLDED patterns
(PfacTable.from_file(..., ignore_case=True)).  In one process, alternating step by step, on the same device buffer:

    folded     the scan with the fold on            (kernel time from the kernel's own clock, pfac_scan_elapsed_ms)
    exact      the same scan with the fold off      (what the fold-off path of the same build costs)
    lower      a torch byte-wise lower-casing of the buffer into a second buffer (HIP events around it) + the exact scan
               of that copy: the device-side form of "lower-case the input first"; it needs a second buffer of the
               input's size and hands every later pass the folded bytes
    classes    the exact scan with the table built through character classes ([aA][bB]...): pfac_table_build_mem_charclass
               over the same patterns, every letter written as a two-member class

Medians over --steps steps after --warmup.  Once, before the timed steps, the folded scan's count and checksum are
checked against the exact scan of the lower-cased copy.  Prints ONE JSON line.

    python tools/nocase_bench.py [--bytes N] [--steps 20] [--warmup 3] [--workload NAME ...]
"""
import argparse
import gzip
import json
import os
import sys

os.environ.setdefault("PFAC_ENABLE_KNOBS", "1")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phfpfac_amd import GpuMatcher, PfacTable  # noqa: E402

DATA = os.path.join(REPO, "tests", "golden", "data")
WORKLOADS = [  # name, pattern fixtures (None: a set that matches nothing), input -- the workloads of tools/series.py
    ("text_experimentpattern", ("experimentpattern",), "text"),       # bench.py's headline workload
    ("rand_experimentpattern", ("experimentpattern",), "rand"),
    ("rand_snort75k", ("bytefile_1000000byte.gz",), "rand"),
    ("text_dictionary", ("xaa", "xab", "xac", "xad"), "text"),
    ("text_no_match", None, "text"),
]


def pattern_image(pats):
    if pats is None:
        return b"\x01\x02\n"
    return b"".join(gzip.open(os.path.join(DATA, p), "rb").read() if p.endswith(".gz") else open(os.path.join(DATA, p), "rb").read()
                    for p in pats)


def class_image(img):
    """The same patterns for the character-class reader, case-insensitive by hand: a letter is a two-member class,
    every other byte an escape (the reader is escape-aware, and '[' must not open a class)."""
    out = bytearray()
    for b in img:
        if b == 0x0A:
            out += b"\n"
        elif 0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A:
            out += b"[%c%c]" % (b | 0x20, b & 0xDF)
        else:
            out += b"\\x%02x" % b
    return bytes(out)


def lower_into(dst, src, n):
    up = (src[:n] >= 0x41) & (src[:n] <= 0x5A)
    torch.where(up, src[:n] | 0x20, src[:n], out=dst[:n])


def run(name, pats, kind, n, steps, warmup):
    img = pattern_image(pats)
    table = PfacTable.from_bytes(img, 256, ignore_case=True)
    ctable = PfacTable.from_charclass(class_image(img), 256)
    stream = torch.cuda.Stream()
    with GpuMatcher(0, 1) as g, GpuMatcher(0, 1) as gc, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)
        gc.set_stream(0, stream.cuda_stream)
        g.load_table(table)
        gc.load_table(ctable)
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        low = torch.zeros(n + 4096, dtype=torch.uint8, device="cuda:0")
        if kind == "rand":
            g.fill_random(buf, n, 0x5048465046414331)
        else:
            g.fill_tiled(buf, n, open(os.path.join(DATA, "paragraph402"), "rb").read())
        cap = n // 2 if pats and len(pats) > 1 else n // 8
        g.reserve(0, 0, cap)
        gc.reserve(0, 0, cap)
        g.sync()
        # the check: folded scan of the buffer == exact scan of the lower-cased copy
        lower_into(low, buf, n)
        stream.synchronize()
        g.set_case_fold(True)
        folded = g.scan_resident(n, n, d_input=buf)
        sum_f = g.checksum(folded)
        g.set_case_fold(False)
        exact_low = g.scan_resident(n, n, d_input=low)
        if (folded, sum_f) != (exact_low, g.checksum(exact_low)):
            raise SystemExit(f"nocase_bench: {name}: the folded scan differs from the exact scan of the lower-cased input")
        exact = g.scan_resident(n, n, d_input=buf)
        classes = gc.scan_resident(n, n, d_input=buf)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        t = {k: [] for k in ("folded", "exact", "lower", "lower_scan", "classes")}
        for step in range(warmup + steps):
            g.set_case_fold(True)
            g.scan_async(n, n, d_input=buf)
            assert g.scan_finish(0)[0] == folded
            ms_f = g.elapsed_ms(0)
            g.set_case_fold(False)
            g.scan_async(n, n, d_input=buf)
            assert g.scan_finish(0)[0] == exact
            ms_e = g.elapsed_ms(0)
            ev[0].record(stream)
            lower_into(low, buf, n)
            ev[1].record(stream)
            ev[1].synchronize()
            g.scan_async(n, n, d_input=low)
            assert g.scan_finish(0)[0] == folded
            ms_l = g.elapsed_ms(0)
            gc.scan_async(n, n, d_input=buf)
            gc.scan_finish(0, allow_overflow=True)
            ms_c = gc.elapsed_ms(0)
            if step >= warmup:
                t["folded"].append(ms_f)
                t["exact"].append(ms_e)
                t["lower"].append(ev[0].elapsed_time(ev[1]))
                t["lower_scan"].append(ms_l)
                t["classes"].append(ms_c)
        info, cinfo = g.info(), gc.info()
        del buf, low
    torch.cuda.empty_cache()
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {
        "workload": name, "bytes": n, "matches_folded": folded, "matches_exact": exact, "matches_class_table": classes,
        "states": table.state_num, "states_class_table": ctable.state_num, "keys": table.n_keys, "keys_class_table": ctable.n_keys,
        "placement": info["variant"], "placement_class_table": cinfo["variant"],
        "scan_folded_ms": round(med["folded"], 4), "scan_exact_ms": round(med["exact"], 4),
        "folded_over_exact": round(med["folded"] / med["exact"], 4),
        "scan_folded_gbs": round(n / med["folded"] / 1e6, 1), "scan_exact_gbs": round(n / med["exact"] / 1e6, 1),
        "scan_folded_ms_min": round(float(np.min(t["folded"])), 4), "scan_exact_ms_min": round(float(np.min(t["exact"])), 4),
        "torch_lower_ms": round(med["lower"], 4), "scan_of_lowered_ms": round(med["lower_scan"], 4),
        "lower_then_scan_ms": round(med["lower"] + med["lower_scan"], 4),
        "lower_then_scan_over_folded": round((med["lower"] + med["lower_scan"]) / med["folded"], 3),
        "scan_class_table_ms": round(med["classes"], 4), "class_table_over_folded": round(med["classes"] / med["folded"], 3),
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
    out = {"metric": "scan with the case fold on vs off (same build, same table of folded patterns, same buffer); "
                     "vs torch lower-casing + exact scan; vs the exact scan of a character-class table",
           "steps": args.steps, "warmup": args.warmup, "workloads": []}
    for name, pats, kind in WORKLOADS:
        if args.workload and name not in args.workload:
            continue
        out["workloads"].append(run(name, pats, kind, args.bytes, args.steps, args.warmup))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
