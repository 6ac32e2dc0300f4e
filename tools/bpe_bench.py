"""GPU measurement of the BPE pass beside the Unigram pass over the same record heap, the scan that feeds both, and the
host library.

One resident input of --bytes (default 1 GiB) of the tiled paragraph.  The vocabulary is trained here, on the host, from
that paragraph with `tokenizers`' BpeTrainer behind a ByteLevel pre-tokenizer (nothing is fetched) and goes through
`bpe_table(byte_level=True)`: words are runs of non-whitespace with their one leading space, the cap is 64 bytes.  The
Unigram attachment sits on the SAME table -- the same strings, the same scan, the same records: every string's score is
-(its merge rank + 1), a byte edge scores below all of them.  Before the timed steps the tokens of the first
--check-bytes (4 MiB, moved out of a word) are compared with tests/bperef.py's by_strings, which never sees a record,
and with the head of the full run.  Then, in ONE process, the paths alternating step by step, each timed with HIP
events around the whole call on the slot's stream, medians over --steps steps after --warmup with min and max:

  (i)   the scan (it feeds both passes; every pass below runs on a fresh one)
  (ii)  pfac_bpe_records, into the caller's ids without positions
  (iii) pfac_unigram_records on the same buffer and table
  (iv)  the host path: the trained tokenizer's `encode` of the first --host-bytes of the input (wall clock)

Bytes counted for the BPE pass: the input read 2.125 times (the solve pass reads its region, the write pass the tile) +
the records read 2.125 times in their width + n_tiles x 1 KiB written and read (the kept maps V, P) + n_tiles x 1 KiB
(the emit bitmap and its prefixes, written and read) + n_tokens x 4 written.  The gathers of a lookup (2 bytes of length
and 16 bytes of piece per record walked) depend on the merges and are NOT counted.  Prints ONE JSON line and, for the
default --bytes, writes it to profiles/bpe_bench.json.

    python tools/bpe_bench.py [--bytes N] [--steps 10] [--warmup 2]
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

from phfpfac_amd import GpuMatcher, PfacError, bpe_byte_alphabet, bpe_table  # noqa: E402
import bperef  # noqa: E402

DATA = os.path.join(REPO, "tests", "golden", "data")
CAP = 64


def event_ms(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return round(float(np.median(ms)), 3), [round(float(np.min(ms)), 3), round(float(np.max(ms)), 3)]


def train(paragraph, vocab_size):
    """-> (tokenizer, vocab, merges) trained on the paragraph alone"""
    from tokenizers import Tokenizer, pre_tokenizers
    from tokenizers.models import BPE
    from tokenizers.trainers import BpeTrainer
    tok = Tokenizer(BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.train_from_iterator([paragraph.decode("latin-1")] * 4,
                            BpeTrainer(vocab_size=vocab_size, initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False))
    model = json.loads(tok.to_str())["model"]
    return tok, model["vocab"], model["merges"]


def reference_vocab(vocab, merges):
    back = {c: b for b, c in bpe_byte_alphabet().items()}
    enc = lambda t: bytes(back[c] for c in t)                   # noqa: E731
    pairs = [m.split(" ") if isinstance(m, str) else m for m in merges]
    return bperef.Vocab({enc(t): i for t, i in vocab.items()}, [(enc(l), enc(r)) for l, r in pairs], lead=0x20, max_word=CAP,
                        word=bperef.DEFAULT_WORD)


def run(n, steps, warmup, host_bytes, check_bytes, vocab_size):
    paragraph = open(os.path.join(DATA, "paragraph402"), "rb").read()
    tok, vocab, merges = train(paragraph, vocab_size)
    table, pieces, byte_ids, skipped = bpe_table(vocab, merges, byte_level=True, max_word_bytes=CAP)
    v = reference_vocab(vocab, merges)
    nf = int(table.num_final)
    ug = np.zeros((nf, 4), dtype=np.int32)                      # the same strings as a Unigram vocabulary
    ug[:, 0] = ug[:, 1] = pieces["id"]
    ug[:, 2] = ug[:, 3] = -(pieces["rank"] + 1)
    ug_byte_score = -(len(merges) + 10)
    lens = table.final_lengths()
    stream = torch.cuda.Stream()
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)
        g.load_table(table)
        g.set_final_lengths(lens)
        g.set_bpe(pieces, byte_ids, lead=0x20, max_word_bytes=CAP)
        g.set_unigram(ug, byte_ids, ug_byte_score, unk_id=-1, max_word_bytes=CAP)
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, paragraph)
        # the check: the prefix alone, against the form of the rule that never sees a record
        head = buf[:min(check_bytes + 4096, n)].cpu().numpy()
        cb = bperef.to_boundary(head, head.size, min(check_bytes, n), v)
        g.reserve(0, 0, 8 * head.size)              # (nested strings: a few records per byte)
        n_rec_head = g.scan_resident(cb, head.size, d_input=buf)
        n_head = g.bpe_records(d_input=buf, positions=True)
        ids_head, pos_head = g.tokens_to_host(n_head, True)
        g.reserve(0, 0, int(n_rec_head / max(cb, 1) * n * 1.25) + (1 << 20))     # the heap of the full run, from the prefix's density
        st = {}
        want = bperef.by_strings(head, cb, v, None, st)
        if n_head != want[0].size or not np.array_equal(ids_head, want[0]) or not np.array_equal(pos_head, want[1]):
            raise SystemExit(f"bpe_bench: the tokens of the first {cb} bytes differ from the reference's")
        greedy = bperef.greedy(head, cb, v)

        def scan():
            return g.scan_resident(n, n, d_input=buf)
        total = scan()
        try:
            n_tok = g.bpe_records(d_input=buf, d_ids=buf, out_cap=0)
        except PfacError as e:                      # (a zero out_cap only asks for the count)
            n_tok = e.n_tokens
        try:
            n_ug = g.unigram_records(d_input=buf, d_ids=buf, out_cap=0)
        except PfacError as e:
            n_ug = e.n_tokens
        cap = int(max(n_tok, n_ug) * 3 // 2 + 4)
        d_ids = torch.empty(cap, dtype=torch.int32, device="cuda:0")
        assert g.bpe_records(d_input=buf, d_ids=d_ids, out_cap=cap) == n_tok
        g.sync()
        if not np.array_equal(d_ids[:n_head].cpu().numpy(), want[0]):
            raise SystemExit("bpe_bench: the head of the full run differs from the run over the prefix")
        ms = {"scan": [], "bpe": [], "unigram": []}
        for step in range(warmup + steps):
            t = {"scan": event_ms(stream, scan)}
            t["bpe"] = event_ms(stream, lambda: g.bpe_records(d_input=buf, d_ids=d_ids, out_cap=cap))
            scan()
            t["unigram"] = event_ms(stream, lambda: g.unigram_records(d_input=buf, d_ids=d_ids, out_cap=cap))
            if step >= warmup:
                for key, val in t.items():
                    ms[key].append(val)
        text = bytes(buf[:min(n, host_bytes)].cpu().numpy())
        rb = g.scan_format()[0]
        del buf, d_ids
    torch.cuda.empty_cache()
    sc, bp, un = stats(ms["scan"]), stats(ms["bpe"]), stats(ms["unigram"])
    n_tiles = (n + 4095) // 4096
    moved = int(2.125 * n + 2.125 * total * rb) + 2 * 1024 * n_tiles + 2 * 1024 * n_tiles + 4 * n_tok
    out = {"bytes": n, "vocabulary_tokens": len(vocab), "merges": len(merges), "patterns": int(len(v.strings)),
           "skipped_entries": len(skipped), "max_word_bytes": CAP, "record_bytes": rb, "matches": total, "tokens": n_tok,
           "unigram_tokens": n_ug, "checked_bytes": cb, "checked_tokens": n_head, "checked_words_with_lead": int(st["lead"]),
           "checked_words_over_cap": int(st["over"]), "checked_tie_steps": int(st["ties"]),
           "checked_greedy_differs": bool(greedy[0].size != want[0].size or not np.array_equal(greedy[0], want[0])),
           "scan_ms": sc[0], "scan_ms_min_max": sc[1], "bpe_ms": bp[0], "bpe_ms_min_max": bp[1], "unigram_ms": un[0],
           "unigram_ms_min_max": un[1], "bpe_over_unigram": round(bp[0] / un[0], 3), "bpe_over_scan": round(bp[0] / sc[0], 3),
           "bpe_counted_bytes": moved, "bpe_counted_gb_per_s": round(moved / bp[0] / 1e6, 1), "bpe_input_gb_per_s": round(n / bp[0] / 1e6, 1)}
    s = text.decode("latin-1")
    t0 = time.perf_counter()
    n_host = len(tok.encode(s).ids)
    out.update({"host_encode_ms": round((time.perf_counter() - t0) * 1e3, 3), "host_encode_input_bytes": len(text), "host_encode_tokens": n_host,
                "bpe_ms_scaled_to_host_bytes": round(bp[0] * len(text) / n, 3)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-bytes", type=int, default=64 << 20)
    ap.add_argument("--check-bytes", type=int, default=4 << 20)
    ap.add_argument("--vocab-size", type=int, default=1000)
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    out = {"metric": "BPE pass over the record heap vs the Unigram pass on the same buffer, table and records; the scan; host encode",
           "steps": args.steps, "warmup": args.warmup}
    out.update(run(args.bytes, args.steps, args.warmup, args.host_bytes, args.check_bytes, args.vocab_size))
    line = json.dumps(out)
    if args.bytes == 1 << 30:                       # the recorded run is the default input
        with open(os.path.join(REPO, "profiles", "bpe_bench.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
