"""GPU measurement of the per-document selection and find-and-replace (pfac_records_leftmost_longest_documents,
pfac_replace_documents) against the whole-stream calls of the same scan (pfac_records_leftmost_longest,
pfac_replace_leftmost_longest).

For every workload: one resident input of --bytes (default 1 GiB), cut into documents of a fixed size; each step scans
it, then runs the whole-stream selection and replace and the per-document selection and replace, the two pairs in
alternating order.  HIP events on the slot's stream time the scan and each call (every call includes its host round
trip); medians over --steps steps after --warmup.  Once, before the timed steps, the documents in front of CHECK_BYTES
are checked on the host: every pick inside its document, the output against tests/replref.splice of the picks and the
output offsets against a cumulative sum.  Prints ONE JSON line.  The time of the per-document offsets kernels comes from
a `rocprofv3 --kernel-trace --stats` run of this tool.

    python tools/doc_replace_bench.py [--bytes N] [--steps 20] [--warmup 3] [--workload NAME ...]
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
WORKLOADS = [  # name, pattern fixture, input kind, document bytes
    ("text_experimentpattern_doc1500", "experimentpattern", "text", 1500),
    ("rand_snort75k_doc1500", "bytefile_1000000byte.gz", "rand", 1500),
    ("rand_snort75k_doc64", "bytefile_1000000byte.gz", "rand", 64),
]
CHECK_BYTES = 32 << 20


def pattern_path(name, tmpdir):
    if name.endswith(".gz"):
        p = os.path.join(tmpdir, name[:-3])
        if not os.path.exists(p):
            with gzip.open(os.path.join(DATA, name), "rb") as g, open(p, "wb") as f:
                f.write(g.read())
        return p
    return os.path.join(DATA, name)


def replacements(path):
    n_ids = sum(1 for _ in open(path, "rb"))
    rng = np.random.default_rng(SEED & 0xFFFFFFFF)
    return {i: bytes(rng.integers(0x41, 0x5B, int(rng.integers(0, 17))).astype(np.uint8)) for i in range(1, n_ids + 1)}


def check_once(table, reps, buf, off, d_sel, d_first, d_out, d_ooff):
    first = d_first.cpu().numpy().view(np.uint64).astype(np.int64)
    o64 = off.astype(np.int64)
    nd = int(np.searchsorted(o64, min(CHECK_BYTES, int(o64[-1])), side="right")) - 1    # documents [0, nd)
    k = int(first[nd])
    sel = d_sel[:k].view(torch.int32).view(-1, 2).cpu().numpy().astype(np.int64)
    lens = table.final_lengths().astype(np.int64)
    pos, st = sel[:, 0], sel[:, 1]
    doc = np.repeat(np.arange(nd), np.diff(first[:nd + 1]))
    if not ((pos >= o64[doc]).all() and (pos + lens[st] <= o64[doc + 1]).all() and (np.diff(pos) > 0).all()):
        raise SystemExit("doc_replace_bench: a pick leaves its document")
    m = int(o64[nd])
    ids = table.idmap[st].astype(np.int64)
    roff, rb = rep_table(reps)
    want = splice(buf[:m].cpu().numpy(), 0, m, pos, lens[st], ids, (roff, rb))
    ooff = d_ooff.cpu().numpy().view(np.uint64).astype(np.int64)
    delta = np.concatenate([[0], np.cumsum(roff[ids + 1] - roff[ids] - lens[st])])
    if (not np.array_equal(d_out[:want.size].cpu().numpy(), want) or ooff[nd] != want.size
            or not np.array_equal(ooff[:nd + 1], o64[:nd + 1] + delta[first[:nd + 1]])):
        raise SystemExit("doc_replace_bench: the output differs from the host splice of the selection")


def run(name, pat, kind, doc_bytes, n, steps, warmup, tmpdir):
    path = pattern_path(pat, tmpdir)
    table = PfacTable.from_file(path, 256)
    reps = replacements(path)
    para = open(os.path.join(DATA, "paragraph402"), "rb").read()
    stream = torch.cuda.Stream()                 # (not the null stream: a NULL handle would give the slot its own back)
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)      # the slot's work runs on this stream: its events bracket it
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        g.set_replacements(reps)
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        if kind == "text":
            g.fill_tiled(buf, n, para)
        else:
            g.fill_random(buf, (n + 7) // 8 * 8, SEED)
        g.reserve(0, 0, max(n // 8, 1 << 20))
        total = g.scan_resident(n, n, d_input=buf)
        g.scan_resident(n, n, d_input=buf)        # (the staging mode has adapted to the workload)
        off = np.append(np.arange(0, n, doc_bytes, dtype=np.uint64), np.uint64(n))
        n_docs = off.size - 1
        d_off = torch.from_numpy(off.view(np.int64)).to("cuda:0")
        d_sel = torch.empty(max(total, 1), dtype=torch.int64, device="cuda:0")
        d_dsel = torch.empty(max(total, 1), dtype=torch.int64, device="cuda:0")
        d_first = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
        d_ooff = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")

        def select(docs):
            if docs:
                return g.select_leftmost_longest_documents(n_docs, d_doc_offsets=d_off, d_out=d_dsel, out_cap=total,
                                                           d_doc_first=d_first)
            return g.select_leftmost_longest(0, d_out=d_sel, out_cap=total)[0]

        def replace(docs, out, cap):
            if docs:
                return g.replace_selection_documents(d_input=buf, d_sel=d_dsel, d_out=out, out_cap=cap, d_out_offsets=d_ooff,
                                                     d_doc_offsets=d_off, d_doc_first=d_first)
            return g.replace_selection(d_input=buf, d_sel=d_sel, d_out=out, out_cap=cap)

        cap = 0
        for docs in (False, True):               # (a zero out_cap only asks for the length)
            select(docs)
            try:
                replace(docs, buf, 0)
            except PfacError as e:
                cap = max(cap, e.out_bytes)
        d_out = torch.empty(cap + 4096, dtype=torch.uint8, device="cuda:0")
        got = {}
        for docs in (False, True):
            got[docs] = (select(docs), replace(docs, d_out, d_out.numel()))
        g.sync()
        check_once(table, reps, buf, off, d_dsel, d_first, d_out, d_ooff)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
        scan_ms, t_ms = [], {False: ([], []), True: ([], [])}
        for step in range(warmup + steps):
            ev[0].record(stream)
            g.scan_async(n, n, d_input=buf)
            assert g.scan_finish(0)[0] == total
            ev[1].record(stream)
            order = (False, True) if step % 2 == 0 else (True, False)
            for j, docs in enumerate(order):     # pair j: select from ev[1 + 3j] to ev[2 + 3j], replace to ev[3 + 3j]
                if j == 1:
                    ev[4].record(stream)
                n_sel = select(docs)
                ev[2 + 3 * j].record(stream)
                assert (n_sel, replace(docs, d_out, d_out.numel())) == got[docs]
                ev[3 + 3 * j].record(stream)
            ev[6].synchronize()
            if step < warmup:
                continue
            scan_ms.append(ev[0].elapsed_time(ev[1]))
            for j, docs in enumerate(order):
                t_ms[docs][0].append(ev[1 + 3 * j].elapsed_time(ev[2 + 3 * j]))
                t_ms[docs][1].append(ev[2 + 3 * j].elapsed_time(ev[3 + 3 * j]))
        del buf, d_sel, d_dsel, d_first, d_ooff, d_out, d_off
    torch.cuda.empty_cache()
    med = lambda x: float(np.median(x))             # noqa: E731
    sel, rep = med(t_ms[False][0]), med(t_ms[False][1])
    dsel, drep = med(t_ms[True][0]), med(t_ms[True][1])
    return {
        "workload": name, "bytes": n, "doc_bytes": doc_bytes, "n_docs": n_docs, "matches": total,
        "selected": got[False][0], "doc_selected": got[True][0], "out_bytes": got[False][1], "doc_out_bytes": got[True][1],
        "scan_ms": round(med(scan_ms), 3), "select_ms": round(sel, 3), "doc_select_ms": round(dsel, 3),
        "replace_ms": round(rep, 3), "doc_replace_ms": round(drep, 3),
        "doc_select_over_select": round(dsel / sel, 3), "doc_replace_over_replace": round(drep / rep, 3),
        "select_ms_min": round(float(np.min(t_ms[False][0])), 3), "doc_select_ms_min": round(float(np.min(t_ms[True][0])), 3),
        "replace_ms_min": round(float(np.min(t_ms[False][1])), 3), "doc_replace_ms_min": round(float(np.min(t_ms[True][1])), 3),
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
    out = {"metric": "per-document selection and replace (pfac_records_leftmost_longest_documents, pfac_replace_documents) "
                     "vs the whole-stream calls of the same scan", "steps": args.steps, "warmup": args.warmup,
           "workloads": []}
    with tempfile.TemporaryDirectory() as tmpdir:
        for name, pat, kind, doc_bytes in WORKLOADS:
            if args.workload and name not in args.workload:
                continue
            out["workloads"].append(run(name, pat, kind, doc_bytes, args.bytes, args.steps, args.warmup, tmpdir))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
