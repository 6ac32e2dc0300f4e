"""GPU measurement of replacement templates and match extraction (pfac_table_set_replacement_templates,
pfac_extract_leftmost_longest) against the plain replace that writes the same bytes.

For every workload: one resident input of --bytes (default 1 GiB), scanned and selected once; then, each timed with HIP
events around the whole call on the slot's stream, medians over --steps steps after --warmup:

  (i)   the plain replace with the fixed replacements prefix + pattern + suffix (exact-case literals: the same bytes)
  (ii)  the templated replace with (prefix, suffix) on every state; its output is compared with (i)'s on the device
  (iii) the extraction with the template (b"", b"\\n") -- grep -o
  (iv)  one D2D copy of (iii)'s output bytes
  (v)   the host path for (iii): the selection D2H plus numpy slicing of the input, on the picks of the first
        --host-bytes of the input (wall clock; the input itself is taken to be on the host already)

The extraction is checked once against (v)'s bytes.  Prints ONE JSON line.

    python tools/template_bench.py [--bytes N] [--steps 10] [--warmup 2] [--workload NAME ...]
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
from replref import _gather_ranges  # noqa: E402

DATA = os.path.join(REPO, "tests", "golden", "data")
WORKLOADS = [("text_experimentpattern", ["experimentpattern"]), ("text_dictionary", ["xaa", "xab", "xac", "xad"])]
PREFIX, SUFFIX = b"<mark>", b"</mark>"


def timed(stream, steps, warmup, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for step in range(warmup + steps):
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        if step >= warmup:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def length_of(call):
    try:
        return call(0)
    except PfacError as e:                       # (a zero out_cap only asks for the length)
        return e.out_bytes


def host_extract(host_in, sel, lens):
    """(v): the picks' bytes, each followed by a newline, by numpy slicing."""
    pos, L = sel["pos"].astype(np.int64), lens[sel["state"]].astype(np.int64)
    out = np.full(int(L.sum()) + pos.size, 0x0A, dtype=np.uint8)
    o = np.concatenate(([0], np.cumsum(L + 1)[:-1])) if pos.size else np.empty(0, dtype=np.int64)
    out[_gather_ranges(o, L)] = host_in[_gather_ranges(pos, L)]
    return out


def run(name, files, n, steps, warmup, host_bytes, tmpdir):
    path = os.path.join(tmpdir, name + ".pat")
    with open(path, "wb") as f:
        for p in files:
            f.write(open(os.path.join(DATA, p), "rb").read())
    lines = open(path, "rb").read().split(b"\n")[:-1]
    table = PfacTable.from_file(path, 256)
    lens = table.final_lengths()
    stream = torch.cuda.Stream()
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)
        g.load_table(table)
        g.set_final_lengths(lens)
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, open(os.path.join(DATA, "paragraph402"), "rb").read())
        g.reserve(0, 0, max(n // 8, 1 << 20))
        total = g.scan_resident(n, n, d_input=buf)
        n_sel, _ = g.select_leftmost_longest(0)
        d_sel = torch.empty(max(n_sel, 1), dtype=torch.int64, device="cuda:0")
        assert g.select_leftmost_longest(0, d_out=d_sel, out_cap=n_sel)[0] == n_sel

        def replace_into(d_out):
            return lambda cap=None: g.replace_selection(d_input=buf, d_sel=d_sel, d_out=d_out, out_cap=d_out.numel() if cap is None else cap)
        # (i) fixed replacements that spell the match out
        g.set_replacements({i: PREFIX + p + SUFFIX for i, p in enumerate(lines, start=1)})
        n_out = length_of(replace_into(buf))
        out_i = torch.empty(n_out + 4096, dtype=torch.uint8, device="cuda:0")
        assert replace_into(out_i)() == n_out
        plain = timed(stream, steps, warmup, replace_into(out_i))
        # (ii) the template
        g.set_highlight(PREFIX, SUFFIX)
        out_ii = torch.empty(n_out + 4096, dtype=torch.uint8, device="cuda:0")
        assert replace_into(out_ii)() == n_out
        g.sync()
        if not torch.equal(out_i[:n_out], out_ii[:n_out]):
            raise SystemExit("template_bench: the templated replace differs from the plain one")
        tpl = timed(stream, steps, warmup, replace_into(out_ii))
        del out_i, out_ii
        # (iii) grep -o, (iv) a copy of its bytes
        g.set_highlight(b"", b"\n")
        d_off = torch.empty(n_sel + 1, dtype=torch.int64, device="cuda:0")

        def extract_into(d_out):
            return lambda cap=None: g.extract_selection(d_input=buf, d_sel=d_sel, d_out=d_out, d_pick_offsets=d_off,
                                                        out_cap=d_out.numel() if cap is None else cap)
        n_ext = length_of(extract_into(buf))
        ext = torch.empty(n_ext + 4096, dtype=torch.uint8, device="cuda:0")
        other = torch.empty(n_ext + 4096, dtype=torch.uint8, device="cuda:0")
        assert extract_into(ext)() == n_ext
        extract = timed(stream, steps, warmup, extract_into(ext))
        copy = timed(stream, steps, warmup, lambda: other[:n_ext].copy_(ext[:n_ext]))
        # (v) the host path on the head of the input, and the check of (iii) against it
        pos_dev = d_sel[:n_sel].view(torch.int32).view(-1, 2)[:, 0].to(torch.int64)
        k = int(torch.searchsorted(pos_dev, torch.tensor([host_bytes], device=pos_dev.device))[0]) if n_sel else 0
        host_in = buf[:min(n, host_bytes + 4096)].cpu().numpy()
        rec = np.dtype([("pos", "<u4"), ("state", "<u4")])
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            sel = d_sel[:k].cpu().numpy().view(rec)
            got = host_extract(host_in, sel, lens)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        head = int(d_off[k].item())
        if got.size != head or not np.array_equal(ext[:head].cpu().numpy(), got):
            raise SystemExit("template_bench: the extraction differs from the host's slicing")
        del buf, d_sel, ext, other, d_off
    torch.cuda.empty_cache()
    r3 = lambda x: round(x, 3)                                              # noqa: E731
    return {"workload": name, "bytes": n, "matches": total, "selected": n_sel, "replace_out_bytes": n_out, "extract_out_bytes": n_ext,
            "plain_replace_ms": r3(plain[0]), "plain_replace_ms_min_max": [r3(plain[1]), r3(plain[2])],
            "template_replace_ms": r3(tpl[0]), "template_replace_ms_min_max": [r3(tpl[1]), r3(tpl[2])],
            "template_over_plain": r3(tpl[0] / plain[0]),
            "extract_ms": r3(extract[0]), "extract_ms_min_max": [r3(extract[1]), r3(extract[2])],
            "d2d_copy_of_extract_ms": r3(copy[0]), "extract_over_copy": r3(extract[0] / copy[0]),
            "host_path_picks": k, "host_path_input_bytes": min(n, host_bytes), "host_path_out_bytes": head,
            "host_path_ms": r3(float(np.median(host_ms))),
            "extract_ms_scaled_to_host_picks": r3(extract[0] * k / n_sel) if n_sel else None}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-bytes", type=int, default=64 << 20)
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    out = {"metric": "templated replace vs the plain replace of the same bytes; match extraction vs a D2D copy and the host path",
           "steps": args.steps, "warmup": args.warmup, "prefix": PREFIX.decode(), "suffix": SUFFIX.decode(), "workloads": []}
    with tempfile.TemporaryDirectory() as tmpdir:
        for name, files in WORKLOADS:
            if args.workload and name not in args.workload:
                continue
            out["workloads"].append(run(name, files, args.bytes, args.steps, args.warmup, args.host_bytes, tmpdir))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
