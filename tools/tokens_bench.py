"""GPU measurement of the tokenize pass (pfac_tokenize_leftmost_longest) against the selection that feeds it, the plain
replace of the same selection and the host path it replaces.

For every workload: one resident input of --bytes (default 1 GiB), scanned once.  Vocabulary token of pattern id i is
i, a byte b outside every pick is n_patterns + 1 + b, whitespace emits nothing.  Before the timed steps the device's
tokens with positions below --check-bytes (4 MiB) are compared with tests/tokref.py's numpy form of the rule over the
picks that start there.  Then, in ONE process, the paths alternating step by step, each timed with HIP events around the
whole call on the slot's stream, medians over --steps steps after --warmup:

  (i)   the tokenize pass into the caller's ids (no positions), and (i+) the same with positions
  (ii)  the leftmost-longest selection that feeds it: the floor
  (iii) the plain replace of the same selection (every pattern replaced by itself: the sibling that moves similar bytes)
  (iv)  the host path (i) replaces: the selection D2H, numpy assembly, ids H2D, on the picks of the first --host-bytes
        of the input (wall clock; the input itself is taken to be on the host already)

Bytes moved by (i) are counted as n_owned read twice + n_picks x 8 read + n_tokens x 4 written.  Prints ONE JSON line.

    python tools/tokens_bench.py [--bytes N] [--steps 10] [--warmup 2] [--workload NAME ...]
"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phfpfac_amd import GpuMatcher, PfacError, PfacTable  # noqa: E402
from tokref import by_numpy  # noqa: E402

DATA = os.path.join(REPO, "tests", "golden", "data")
WORKLOADS = [("text_experimentpattern", ["experimentpattern"]), ("text_dictionary", ["xaa", "xab", "xac", "xad"])]
WHITESPACE = b" \n\t\r"
REC = np.dtype([("pos", "<u4"), ("state", "<u4")])


def event_ms(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return round(float(np.median(ms)), 3), [round(float(np.min(ms)), 3), round(float(np.max(ms)), 3)]


def run(name, files, n, steps, warmup, host_bytes, check_bytes, tmpdir):
    path = os.path.join(tmpdir, name + ".pat")
    with open(path, "wb") as f:
        for p in files:
            f.write(open(os.path.join(DATA, p), "rb").read())
    lines = open(path, "rb").read().split(b"\n")[:-1]
    table = PfacTable.from_file(path, 256)
    lens = table.final_lengths()
    idmap = np.asarray(table.idmap, dtype=np.int64)
    tok_by_id = np.arange(len(lines) + 1, dtype=np.int32)
    tok_by_id[0] = -1
    btok = (len(lines) + 1 + np.arange(256)).astype(np.int32)
    btok[np.frombuffer(WHITESPACE, dtype=np.uint8)] = -1
    stream = torch.cuda.Stream()
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)
        g.load_table(table)
        g.set_final_lengths(lens)
        g.set_token_ids({i: i for i in range(1, len(lines) + 1)}, byte_ids=btok)
        g.set_replacements({i: p for i, p in enumerate(lines, start=1)})
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, open(os.path.join(DATA, "paragraph402"), "rb").read())
        g.reserve(0, 0, max(n // 8, 1 << 20))
        total = g.scan_resident(n, n, d_input=buf)
        n_sel, _ = g.select_leftmost_longest(0)
        d_sel = torch.empty(max(n_sel, 1), dtype=torch.int64, device="cuda:0")

        def select():
            return g.select_leftmost_longest(0, d_out=d_sel, out_cap=n_sel)[0]
        assert select() == n_sel
        try:
            n_tok = g.tokenize_selection(d_input=buf, d_sel=d_sel, d_ids=buf, out_cap=0)
        except PfacError as e:                      # (a zero out_cap only asks for the count)
            n_tok = e.n_tokens
        d_ids = torch.empty(max(n_tok, 4), dtype=torch.int32, device="cuda:0")
        d_pos = torch.empty(max(n_tok, 4), dtype=torch.int32, device="cuda:0")
        out = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")

        def tokenize():
            return g.tokenize_selection(d_input=buf, d_sel=d_sel, d_ids=d_ids, out_cap=n_tok)

        def tokenize_pos():
            return g.tokenize_selection(d_input=buf, d_sel=d_sel, d_ids=d_ids, out_cap=n_tok, d_pos=d_pos)

        def replace():
            return g.replace_selection(d_input=buf, d_sel=d_sel, d_out=out, out_cap=out.numel())
        # the check: tokens below check_bytes against the reference over the picks that start there
        assert tokenize_pos() == n_tok
        g.sync()
        cb = min(check_bytes, n)
        pos_dev = d_sel[:n_sel].view(torch.int32).view(-1, 2)[:, 0].to(torch.int64)
        k = int(torch.searchsorted(pos_dev, torch.tensor([cb], device=pos_dev.device))[0]) if n_sel else 0
        sel = d_sel[:k].cpu().numpy().view(REC)
        head = buf[:cb].cpu().numpy()
        want = by_numpy(head, 0, cb, sel["pos"], lens[sel["state"]], idmap[sel["state"]], tok_by_id, btok)
        m = int(torch.searchsorted(d_pos[:n_tok].to(torch.int64), torch.tensor([cb], device="cuda:0"))[0])
        if m != want[0].size or not np.array_equal(d_ids[:m].cpu().numpy(), want[0]) or \
                not np.array_equal(d_pos[:m].cpu().numpy().view(np.uint32), want[1]):
            raise SystemExit(f"tokens_bench: the tokens of the first {cb} bytes differ from the reference's")
        assert tokenize() == n_tok and replace() == n                    # (every pattern replaced by itself)
        # the timed steps, paths alternating
        ms = {"tokenize": [], "tokenize_pos": [], "select": [], "replace": []}
        for step in range(warmup + steps):
            t = {"tokenize": event_ms(stream, tokenize), "tokenize_pos": event_ms(stream, tokenize_pos),
                 "select": event_ms(stream, select), "replace": event_ms(stream, replace)}
            if step >= warmup:
                for key, v in t.items():
                    ms[key].append(v)
        # the host path on the head of the input
        kh = int(torch.searchsorted(pos_dev, torch.tensor([host_bytes], device=pos_dev.device))[0]) if n_sel else 0
        hb = min(n, host_bytes)
        host_in = buf[:hb].cpu().numpy()
        host_ms, host_tokens = [], 0
        for _ in range(3):
            t0 = time.perf_counter()
            hsel = d_sel[:kh].cpu().numpy().view(REC)
            ids = by_numpy(host_in, 0, hb, hsel["pos"], lens[hsel["state"]], idmap[hsel["state"]], tok_by_id, btok)[0]
            d_host_ids = torch.from_numpy(ids).to("cuda:0")
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
            host_tokens = int(d_host_ids.numel())
        del buf, d_sel, d_ids, d_pos, out
    torch.cuda.empty_cache()
    tk, tp, sl, rp = stats(ms["tokenize"]), stats(ms["tokenize_pos"]), stats(ms["select"]), stats(ms["replace"])
    moved = 2 * n + 8 * n_sel + 4 * n_tok
    return {"workload": name, "bytes": n, "matches": total, "selected": n_sel, "tokens": n_tok, "checked_bytes": cb, "checked_tokens": m,
            "tokenize_ms": tk[0], "tokenize_ms_min_max": tk[1], "tokenize_with_positions_ms": tp[0],
            "tokenize_with_positions_ms_min_max": tp[1], "select_ms": sl[0], "select_ms_min_max": sl[1],
            "replace_ms": rp[0], "replace_ms_min_max": rp[1],
            "tokenize_over_select": round(tk[0] / sl[0], 3), "tokenize_over_replace": round(tk[0] / rp[0], 3),
            "counted_bytes_moved": moved, "tokenize_gb_per_s": round(moved / tk[0] / 1e6, 1),
            "host_path_picks": kh, "host_path_input_bytes": hb, "host_path_tokens": host_tokens,
            "host_path_ms": round(float(np.median(host_ms)), 3),
            "tokenize_ms_scaled_to_host_bytes": round(tk[0] * hb / n, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-bytes", type=int, default=64 << 20)
    ap.add_argument("--check-bytes", type=int, default=4 << 20)
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    out = {"metric": "tokenize pass vs the selection that feeds it, the plain replace of the same selection and the host path",
           "steps": args.steps, "warmup": args.warmup, "workloads": []}
    with tempfile.TemporaryDirectory() as tmpdir:
        for name, files in WORKLOADS:
            if args.workload and name not in args.workload:
                continue
            out["workloads"].append(run(name, files, args.bytes, args.steps, args.warmup, args.host_bytes, args.check_bytes, tmpdir))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
