"""GPU measurement of the rule-set pass (pfac_documents_rules) against the pass that feeds it, against torch's sparse
product and against the host path it replaces.

For every workload of tools/terms_bench.py (text lines of three lengths that end in '\\n', --bytes of them, default
1 GiB) the input is scanned with --patterns (default: the dictionary xaa+xab+xac+xad, whose text reaches many final
states; WORDS16: the sixteen words of tools/near_bench.py), split at '\\n', cut per line, and turned into the
document-term matrix.  Then, for 1, 64, 4096 and 65536 seeded rules of 2 to 4 terms over ALL final states (a rule base
most of whose patterns are rare: tests/ruleref.py makes them) and for 1 and 64 rules over the states this text REACHES
(every term common), over that one matrix:

  rules         the whole call into the caller's buffers: the 8-byte read of row_ptr[n_docs], the count kernel and its
                prefix, the 16-byte copy back, the expand, the sort passes, the fired tails, the copy back of the total,
                the write and row_ptr.  The pass refuses an expansion of 2^32 keys or more, and its sort holds 16 bytes per
                key: it runs over the longest PREFIX of the documents whose keys stay within --max-keys (default 2^30),
                and the JSON names the documents and the keys E of that prefix
  terms         pfac_documents_term_counts of the whole input, the pass that feeds it
  torch_sparse  presence (the term matrix, float32 CSR) @ positive and @ negative (CSR, states x rules) with
                torch.sparse.mm, then the two compares -- where torch on this build can do it; the JSON holds the error
                text where it cannot.  Over the prefix of --side-keys keys (default 2^24)
  host_path     what a caller did before: the CSR to the host, numpy (tests/ruleref.fired: the expansion, numpy.unique,
                two bincounts), the ids not returned.  Over the same --side-keys prefix, wall clock

HIP events on the slot's stream around each whole call, medians over --steps steps after --warmup.  Before anything is
timed the pass over a prefix of 2^22 keys is compared with tests/ruleref.py.  Prints ONE JSON line and writes it to --out.

    python tools/rules_bench.py [--bytes N] [--patterns dictionary|WORDS16] [--steps 10] [--warmup 2] [--out profiles/rules_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ruleref  # noqa: E402
from phfpfac_amd import GpuMatcher, PfacError, PfacTable  # noqa: E402
from near_bench import WORDS16  # noqa: E402
from split_bench import DATA, DELIM, WORKLOADS, line_block  # noqa: E402

RULE_SETS = ((1, "reached"), (64, "reached"), (1, "all"), (64, "all"), (4096, "all"), (65536, "all"))
CHECK_KEYS = 1 << 22


def load_table(patterns):
    if patterns == "WORDS16":
        return PfacTable.from_bytes(b"".join(w + b"\n" for w in WORDS16), 256)
    with tempfile.NamedTemporaryFile(suffix=".pat") as f:
        for p in ("xaa", "xab", "xac", "xad"):
            f.write(open(os.path.join(DATA, p), "rb").read())
        f.flush()
        return PfacTable.from_file(f.name, 256)


def prefix(keys_before_doc, limit):
    """The most documents whose keys number `limit` at the most."""
    return int(np.searchsorted(keys_before_doc, limit, side="right")) - 1


def torch_route(d_row, d_st, n_docs, n_pairs, rules, nf):
    """(ms, fired) or (None, the error): presence @ positive >= need and presence @ negative == 0, sparse in, sparse out."""
    try:
        dev = d_row.device
        ptr = rules.rule_ptr.astype(np.int64)
        t = rules.terms.astype(np.int64)
        rule = np.repeat(np.arange(rules.n_rules), np.diff(ptr))
        mats = []
        for neg in (0, 1):
            m = (t >> 31) == neg
            coo = torch.sparse_coo_tensor(torch.tensor(np.stack([t[m] & 0x7FFFFFFF, rule[m]]), device=dev),
                                          torch.ones(int(m.sum()), device=dev), size=(nf, rules.n_rules))
            mats.append(coo.coalesce().to_sparse_csr())
        need = torch.tensor(rules.need.astype(np.float32), device=dev)
        a = torch.sparse_csr_tensor(d_row[: n_docs + 1], d_st[:n_pairs].to(torch.int64), torch.ones(n_pairs, device=dev), size=(n_docs, nf))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ms = []
        for _ in range(3):
            ev[0].record()
            pos = torch.sparse.mm(a, mats[0]).to_sparse_coo().coalesce()
            hit = pos.values() >= need[pos.indices()[1]]
            cand = pos.indices()[:, hit]
            n_fired = int(cand.shape[1])
            if mats[1]._nnz():
                bad = torch.sparse.mm(a, mats[1]).to_sparse_coo().coalesce().indices()
                ck, bk = cand[0] * rules.n_rules + cand[1], bad[0] * rules.n_rules + bad[1]
                n_fired = int((~torch.isin(ck, bk)).sum())
            ev[1].record()
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        return float(np.median(ms)), n_fired
    except Exception as e:      # noqa: BLE001 -- the JSON reports what torch said
        return None, f"{type(e).__name__}: {str(e).splitlines()[0][:200]}"


def run(name, mean, n, patterns, steps, warmup, max_keys, side_keys):
    table = load_table(patterns)
    nf = int(table.num_final)
    block = line_block(mean, mean)
    stream = torch.cuda.Stream()
    out = {"workload": name, "bytes": n, "mean_line_bytes": mean, "patterns": patterns, "num_final": nf, "rules": []}
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)
        g.load_table(table)
        g.set_final_lengths(table.final_lengths())
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, block.tobytes())
        g.reserve(0, 0, max(n // 2, 1 << 20))
        g.scan_resident(n, n, d_input=buf)
        total = g.scan_resident(n, n, d_input=buf)        # (the staging mode has adapted to the workload)
        n_docs, _ = g.split_documents(n, DELIM, d_input=buf)
        kept = g.segment_records(n_docs)
        n_terms = g.document_term_counts(n_docs)
        d_row = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
        d_st = torch.empty(max(n_terms, 1), dtype=torch.int32, device="cuda:0")
        d_cnt = torch.empty(max(n_terms, 1), dtype=torch.int32, device="cuda:0")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        terms_ms = []
        for step in range(warmup + steps):
            ev[0].record(stream)
            assert g.document_term_counts(n_docs, d_row_ptr=d_row, d_states=d_st, d_counts=d_cnt, out_cap=n_terms) == n_terms
            ev[1].record(stream)
            ev[1].synchronize()
            if step >= warmup:
                terms_ms.append(ev[0].elapsed_time(ev[1]))
        del d_cnt, buf
        row = d_row.cpu().numpy().astype(np.int64)
        st = d_st[:n_terms].cpu().numpy().astype(np.int64)
        out.update(n_docs=n_docs, matches=total, kept=kept, n_terms=n_terms, states_reached=int(np.unique(st).size),
                   terms_ms=round(float(np.median(terms_ms)), 3))
        reached = np.unique(st)
        for n_rules, over in RULE_SETS:
            rules = ruleref.random_rules(np.random.default_rng([0x62656E63, n_rules]), n_rules, nf,
                                         spare=np.setdiff1d(np.arange(nf), reached) if over == "reached" else ())
            g.set_rules((rules.rule_ptr, rules.terms, rules.need))
            before = np.concatenate([[0], np.cumsum(rules.degree()[st])])[row]       # keys in front of document d
            # once, before anything is timed: a prefix against the reference
            nd = prefix(before, CHECK_KEYS)
            nf_ = g.document_rules(nd, d_row_ptr=d_row, d_states=d_st)
            ruleref.check(ruleref.fired(row[: nd + 1], st[: row[nd]], rules), *g.rules_to_host(nd, nf_), what=f"rules_bench {name}, {n_rules} rules over {over} states")
            nd = prefix(before, min(max_keys, (1 << 32) - 1))
            E = int(before[nd])
            n_fired = g.document_rules(nd, d_row_ptr=d_row, d_states=d_st)
            d_out_row = torch.empty(nd + 1, dtype=torch.int64, device="cuda:0")
            d_out = torch.empty(max(n_fired, 1), dtype=torch.int32, device="cuda:0")
            ms = []
            for step in range(warmup + steps):
                ev[0].record(stream)
                assert g.document_rules(nd, d_row_ptr=d_row, d_states=d_st, d_row_ptr_out=d_out_row, d_rules=d_out, out_cap=n_fired) == n_fired
                ev[1].record(stream)
                ev[1].synchronize()
                if step >= warmup:
                    ms.append(ev[0].elapsed_time(ev[1]))
            del d_out_row, d_out
            if nd < n_docs:                                     # the refusal of the whole input, where it expands too far
                try:
                    g.document_rules(n_docs, d_row_ptr=d_row, d_states=d_st)
                    whole = "accepted"
                except PfacError as e:
                    whole = f"refused (status {e.status})" if int(before[n_docs]) >= 1 << 32 else f"not run: {e}"
            else:
                whole = "measured"
            ns = prefix(before, side_keys)
            t_ms, t_res = torch_route(d_row, d_st, ns, int(row[ns]), rules, nf)
            t0 = time.perf_counter()
            h_row, h_st = d_row[: ns + 1].cpu().numpy(), d_st[: int(row[ns])].cpu().numpy()
            h = ruleref.fired(h_row, h_st, rules)
            host_ms = (time.perf_counter() - t0) * 1e3
            med = float(np.median(ms))
            out["rules"].append({
                "n_rules": n_rules, "terms_over": over, "terms": int(rules.terms.size), "docs_measured": nd, "pairs_measured": int(row[nd]), "E": E,
                "E_of_whole_input": int(before[n_docs]), "whole_input": whole, "sort_passes": ruleref.sort_passes(nd, n_rules),
                "n_fired": n_fired, "rules_ms": round(med, 3), "rules_ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
                "rules_ns_per_key": round(med * 1e6 / E, 4) if E else None, "rules_over_terms": round(med / float(np.median(terms_ms)), 3),
                "side_docs": ns, "side_E": int(before[ns]), "side_n_fired": int(h[1].size),
                "torch_sparse_ms": None if t_ms is None else round(t_ms, 3),
                "torch_sparse_result": t_res if t_ms is None else ("agrees" if t_res == h[1].size else f"{t_res} fired, the reference has {h[1].size}"),
                "host_path_ms": round(host_ms, 1),
            })
            print(f"rules_bench: {name}, {n_rules} rules over {over} states done", file=sys.stderr, flush=True)
        del d_row, d_st
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--patterns", choices=("dictionary", "WORDS16"), default="dictionary")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-keys", type=int, default=1 << 30)
    ap.add_argument("--side-keys", type=int, default=1 << 24)
    ap.add_argument("--workload", action="append", default=None, help="only these (repeatable)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rules_bench.json"))
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    out = {"metric": "pfac_documents_rules vs pfac_documents_term_counts (the pass that feeds it), vs torch.sparse.mm over the term matrix, "
                     "and vs the CSR fetched to the host + numpy",
           "steps": args.steps, "warmup": args.warmup, "max_keys": args.max_keys, "side_keys": args.side_keys,
           "rules_ms_counts": "the whole call into the caller's buffers over the prefix of docs_measured documents (HIP events)",
           "terms_ms_counts": "pfac_documents_term_counts of the WHOLE input from the slot-owned cut into the caller's buffers (HIP events)",
           "torch_sparse_ms_counts": "two torch.sparse.mm, the compares and torch.isin over the prefix of side_docs documents; building the "
                                     "operands is not timed",
           "host_path_ms_counts": "wall clock over the same prefix: the fetch of row_ptr and states, numpy.repeat, numpy.unique, two bincounts",
           "workloads": []}
    for name, mean in WORKLOADS:
        if args.workload and name not in args.workload:
            continue
        out["workloads"].append(run(name, mean, args.bytes, args.patterns, args.steps, args.warmup, args.max_keys, args.side_keys))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
