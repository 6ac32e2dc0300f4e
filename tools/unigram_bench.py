"""GPU measurement of the Unigram pass against the WordPiece pipeline it stands beside and the host path it replaces.

One resident input of --bytes (default 1 GiB) of the tiled paragraph; the vocabulary is the dictionary (xaa..xad), every
other word as a continuation piece, the rest as `▁` pieces, with seeded scores in [-12, -2); words are runs of
[0-9A-Za-z_], punctuation bytes have ids of their own, whitespace emits nothing; a run of byte edges is one unk.  Before
the timed steps the tokens of the first --check-bytes (4 MiB, moved to a word boundary) are compared with
tests/uniref.py's forward DP over the records of a scan of that prefix, and with the head of the full run.  Then, in ONE
process, the paths alternating step by step, each timed with HIP events around the whole calls on the slot's stream,
medians over --steps steps after --warmup, every path on a fresh scan of the same input (the scan is outside the events):

  (i)   pfac_unigram_records, into the caller's ids without positions
  (ii)  the WordPiece pipeline over the same buffer and vocabulary: pfac_records_filter_roles, then
        pfac_records_leftmost_longest, then pfac_wordpiece_leftmost_longest
  (iii) the host path: tokenizers' Unigram behind a Metaspace pre-tokenizer on the first --host-bytes of the input (wall
        clock), if that package is importable

Bytes moved by the Unigram pass are counted as n_owned read twice + the records read twice + n_tiles x 1.5 KiB written
and read (the kept bitmaps) + n_tiles x 1 KiB (the emit bitmap and its prefixes, written and read) + 18 bytes gathered
per record (length and piece entry) + n_tokens x 4 written.  Prints ONE JSON line and, for the default --bytes, writes
it to profiles/unigram_bench.json.

    python tools/unigram_bench.py [--bytes N] [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phfpfac_amd import GpuMatcher, PfacError, unigram_table  # noqa: E402
import uniref  # noqa: E402

DATA = os.path.join(REPO, "tests", "golden", "data")
DICTIONARY = ["xaa", "xab", "xac", "xad"]
PUNCT = b".,;:!?'\"()-"
WORD = uniref.CASE_WORD


def event_ms(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return round(float(np.median(ms)), 3), [round(float(np.min(ms)), 3), round(float(np.max(ms)), 3)]


def vocabulary(seed=5):
    words = []
    for p in DICTIONARY:
        words += open(os.path.join(DATA, p), "rb").read().split(b"\n")
    words = sorted(set(w for w in words if w and all(b in WORD for b in w)))
    rng = np.random.default_rng(seed)
    scores = -(2.0 + 10.0 * rng.random(len(words)))
    scores = np.round(scores * 65536) / 65536
    return [(b"<unk>", 0.0)] + [((w if k & 1 else uniref.PREFIX + w), float(s)) for k, (w, s) in enumerate(zip(words, scores))]


def host_path(entries, text):
    try:
        from tokenizers import Tokenizer, pre_tokenizers
        from tokenizers.models import Unigram
        tok = Tokenizer(Unigram([(e.decode("latin-1") if not e.startswith(uniref.PREFIX) else "▁" + e[3:].decode("latin-1"), s)
                                 for e, s in entries], unk_id=0, byte_fallback=False))
        tok.pre_tokenizer = pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="always", split=True)
        s = text.decode("latin-1")
        t0 = time.perf_counter()
        n = len(tok.encode(s).ids)
        return {"host_path_ms": round((time.perf_counter() - t0) * 1e3, 3), "host_path_input_bytes": len(text), "host_path_tokens": n}
    except ImportError:
        return None


def run(n, steps, warmup, host_bytes, check_bytes):
    entries = vocabulary()
    table, pieces, scale, skipped = unigram_table(entries, word_bytes=WORD, max_word_bytes=100)
    ints = [(e, int(round(s * scale))) for e, s in entries]
    byte_ids = np.full(256, -1, dtype=np.int32)
    byte_ids[np.frombuffer(PUNCT, dtype=np.uint8)] = len(entries) + np.arange(len(PUNCT))
    bscore = int(-20 * scale)
    v = uniref.Vocab(ints, 0, 100, WORD, False, byte_ids, bscore)
    lens = table.final_lengths()
    stream = torch.cuda.Stream()
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)
        g.load_table(table)
        g.set_final_lengths(lens)
        g.set_unigram(pieces, byte_ids, bscore, unk_id=0, word_bytes=WORD, max_word_bytes=100)
        g.set_wordpiece(pieces["first_id"], pieces["cont_id"], byte_ids, unk_id=0, word_bytes=WORD, max_word_bytes=100)
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, open(os.path.join(DATA, "paragraph402"), "rb").read())
        g.reserve(0, 0, max(n // 2, 1 << 20))
        # the check: a scan of the prefix alone, its records through the reference's forward DP
        head = buf[:min(check_bytes + 4096, n)].cpu().numpy()
        cb = uniref.wpref.to_boundary(head, head.size, min(check_bytes, n), v)
        n_rec = g.scan_resident(cb, head.size, d_input=buf)
        rec = g.records_to_host(n_rec)
        n_head = g.unigram_records(d_input=buf, positions=True)
        ids_head, pos_head = g.tokens_to_host(n_head, True)
        index = {p: i for i, p in enumerate(v.pieces)}
        rpos = rec["pos"].astype(np.int64)
        rlen = lens[rec["state"]].astype(np.int64)
        ridx = np.array([index[bytes(head[int(p):int(p) + int(L)])] for p, L in zip(rpos, rlen)], dtype=np.int64)
        want = uniref.by_records(head, cb, rpos, rlen, ridx, v)
        if n_head != want[0].size or not np.array_equal(ids_head, want[0]) or not np.array_equal(pos_head, want[1]):
            raise SystemExit(f"unigram_bench: the tokens of the first {cb} bytes differ from the reference's")
        greedy = uniref.greedy_words(head, cb, v)

        def scan():
            return g.scan_resident(n, n, d_input=buf)
        total = scan()
        try:
            n_tok = g.unigram_records(d_input=buf, d_ids=buf, out_cap=0)
        except PfacError as e:                      # (a zero out_cap only asks for the count)
            n_tok = e.n_tokens
        d_ids = torch.empty(max(n_tok + n_tok // 2, 4), dtype=torch.int32, device="cuda:0")
        cap = int(d_ids.numel())
        assert g.unigram_records(d_input=buf, d_ids=d_ids, out_cap=cap) == n_tok
        g.sync()
        if not np.array_equal(d_ids[:n_head].cpu().numpy(), want[0]):
            raise SystemExit("unigram_bench: the head of the full run differs from the run over the prefix")

        def pipeline():
            g.filter_roles(0, d_input=buf)
            g.select_leftmost_longest(0)
            return g.wordpiece_selection(d_input=buf, d_ids=d_ids, out_cap=cap)
        ms = {"unigram": [], "pipeline": []}
        kept = 0
        for step in range(warmup + steps):
            scan()
            t = {"unigram": event_ms(stream, lambda: g.unigram_records(d_input=buf, d_ids=d_ids, out_cap=cap))}
            scan()
            t["pipeline"] = event_ms(stream, pipeline)
            kept = g.last_count()
            if step >= warmup:
                for key, val in t.items():
                    ms[key].append(val)
        text = bytes(buf[:min(n, host_bytes)].cpu().numpy())
        rb = g.scan_format()[0]
        del buf, d_ids
    torch.cuda.empty_cache()
    ug, pl = stats(ms["unigram"]), stats(ms["pipeline"])
    n_tiles = (n + 4095) // 4096
    moved = 2 * n + 2 * total * rb + 2 * 1536 * n_tiles + 2 * 1024 * n_tiles + 18 * total + 4 * n_tok
    out = {"bytes": n, "vocabulary_entries": len(entries), "skipped_entries": len(skipped), "scale": scale, "record_bytes": rb,
           "matches": total, "kept_by_roles": kept, "tokens": n_tok, "checked_bytes": cb, "checked_tokens": n_head,
           "checked_unk_tokens": int((want[0] == 0).sum()), "checked_tokens_greedy": int(greedy[0].size),
           "checked_greedy_differs": bool(greedy[0].size != want[0].size or not np.array_equal(greedy[0], want[0])),
           "unigram_ms": ug[0], "unigram_ms_min_max": ug[1], "wordpiece_pipeline_ms": pl[0], "wordpiece_pipeline_ms_min_max": pl[1],
           "unigram_over_pipeline": round(ug[0] / pl[0], 3), "unigram_counted_bytes": moved,
           "unigram_gb_per_s": round(moved / ug[0] / 1e6, 1), "unigram_input_gb_per_s": round(n / ug[0] / 1e6, 1)}
    host = host_path(entries, text)
    if host is not None:
        out.update(host)
        out["unigram_ms_scaled_to_host_bytes"] = round(ug[0] * len(text) / n, 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-bytes", type=int, default=64 << 20)
    ap.add_argument("--check-bytes", type=int, default=4 << 20)
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    out = {"metric": "Unigram pass over the record heap vs role filter + selection + WordPiece pass on the same buffer; host path",
           "steps": args.steps, "warmup": args.warmup}
    out.update(run(args.bytes, args.steps, args.warmup, args.host_bytes, args.check_bytes))
    line = json.dumps(out)
    if args.bytes == 1 << 30:                       # the recorded run is the default input
        with open(os.path.join(REPO, "profiles", "unigram_bench.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
