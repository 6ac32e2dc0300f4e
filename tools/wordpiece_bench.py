"""GPU measurement of the WordPiece passes against their nearest siblings and the host path they replace.

One resident input of --bytes (default 1 GiB) of the tiled paragraph; the vocabulary is the dictionary (xaa..xad), every
other word as a `##` piece, the rest as word-initial pieces, plus [UNK]; punctuation bytes have ids of their own,
whitespace emits nothing.  Before the timed steps the device's tokens with positions below --check-bytes (4 MiB, moved
to a word boundary) are compared with tests/wpref.py's numpy form of the rule over the picks that start there.  Then, in
ONE process, the paths alternating step by step, each timed with HIP events around the whole call on the slot's stream,
medians over --steps steps after --warmup:

  (i)   pfac_records_filter_roles against pfac_records_filter_words (default set, both edges), each on a fresh scan of
        the same input (the scan itself is outside the events)
  (ii)  pfac_wordpiece_leftmost_longest against pfac_tokenize_leftmost_longest over the SAME selection (made from the
        role-filtered scan), both into the caller's ids without positions
  (iii) the host path: tokenizers' WordPiece behind its Whitespace pre-tokenizer on the first --host-bytes of the input
        (wall clock), if that package is importable

Bytes moved by the token pass are counted as n_owned read twice + n_picks x 8 read + n_tiles x 2 KiB written and read
(the kept bitmaps) + n_tokens x 4 written; by the filter as the records read + the kept ones written + 2 bytes and 8
bytes gathered per record.  Prints ONE JSON line.

    python tools/wordpiece_bench.py [--bytes N] [--steps 10] [--warmup 2]
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

from phfpfac_amd import GpuMatcher, PfacError, wordpiece_table  # noqa: E402
import wpref  # noqa: E402

DATA = os.path.join(REPO, "tests", "golden", "data")
DICTIONARY = ["xaa", "xab", "xac", "xad"]
PUNCT = b".,;:!?'\"()-"
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


def vocabulary():
    words = []
    for p in DICTIONARY:
        words += open(os.path.join(DATA, p), "rb").read().split(b"\n")
    words = sorted(set(w for w in words if w))
    entries = [b"[UNK]"] + [(b"##" + w if k & 1 else w) for k, w in enumerate(words)] + [bytes([b]) for b in PUNCT]
    return entries


def host_path(entries, text):
    try:
        from tokenizers import Tokenizer, pre_tokenizers
        from tokenizers.models import WordPiece
    except ImportError:
        return None
    vocab = {}
    for k, e in enumerate(entries):
        vocab.setdefault(e.decode("latin-1"), k)
    tok = Tokenizer(WordPiece(vocab=vocab, unk_token="[UNK]", max_input_chars_per_word=100, continuing_subword_prefix="##"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    s = text.decode("latin-1")
    t0 = time.perf_counter()
    n = len(tok.encode(s).ids)
    return {"host_path_ms": round((time.perf_counter() - t0) * 1e3, 3), "host_path_input_bytes": len(text), "host_path_tokens": n}


def run(n, steps, warmup, host_bytes, check_bytes):
    entries = vocabulary()
    table, first, cont, byte_ids, skipped = wordpiece_table(entries)
    v = wpref.Vocab(entries, b"[UNK]")
    lens = table.final_lengths()
    plain = np.where(first >= 0, first, cont).astype(np.int32)         # the plain tokenizer's ids over the same states
    stream = torch.cuda.Stream()
    with GpuMatcher(0, 1) as g, torch.cuda.stream(stream):
        g.set_stream(0, stream.cuda_stream)
        g.load_table(table)
        g.set_final_lengths(lens)
        g.set_wordpiece(first, cont, byte_ids, unk_id=0, max_word_bytes=100)
        g._check(g._L.pfac_table_set_token_ids(g._ctx, plain.ctypes.data, plain.size, byte_ids.ctypes.data))
        buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
        g.fill_tiled(buf, n, open(os.path.join(DATA, "paragraph402"), "rb").read())
        g.reserve(0, 0, max(n // 8, 1 << 20))

        def scan():
            return g.scan_resident(n, n, d_input=buf)
        total = scan()
        kept = g.filter_roles(0, d_input=buf)
        n_sel, _ = g.select_leftmost_longest(0)
        d_sel = torch.empty(max(n_sel, 1), dtype=torch.int64, device="cuda:0")
        assert g.select_leftmost_longest(0, d_out=d_sel, out_cap=n_sel)[0] == n_sel
        counts = {}
        for name, fn in (("wordpiece", g.wordpiece_selection), ("tokenize", g.tokenize_selection)):
            try:
                counts[name] = fn(d_input=buf, d_sel=d_sel, d_ids=buf, out_cap=0)
            except PfacError as e:                  # (a zero out_cap only asks for the count)
                counts[name] = e.n_tokens
        n_tok = counts["wordpiece"]
        cap = max(counts.values())
        d_ids = torch.empty(max(cap, 4), dtype=torch.int32, device="cuda:0")
        d_pos = torch.empty(max(cap, 4), dtype=torch.int32, device="cuda:0")

        def wordpiece():
            return g.wordpiece_selection(d_input=buf, d_sel=d_sel, d_ids=d_ids, out_cap=cap)

        def tokenize():
            return g.tokenize_selection(d_input=buf, d_sel=d_sel, d_ids=d_ids, out_cap=cap)
        # the check: tokens below cb against the reference over the picks that start there
        assert g.wordpiece_selection(d_input=buf, d_sel=d_sel, d_ids=d_ids, out_cap=cap, d_pos=d_pos) == n_tok
        g.sync()
        head = buf[:min(check_bytes + 4096, n)].cpu().numpy()
        cb = wpref.to_boundary(head, head.size, min(check_bytes, n), v)
        pos_dev = d_sel[:n_sel].view(torch.int32).view(-1, 2)[:, 0].to(torch.int64)
        k = int(torch.searchsorted(pos_dev, torch.tensor([cb], device=pos_dev.device))[0]) if n_sel else 0
        sel = d_sel[:k].cpu().numpy().view(REC)
        index = {p: i for i, p in enumerate(v.pieces)}
        plen = lens[sel["state"]].astype(np.int64)
        pidx = np.array([index[bytes(head[int(p):int(p) + int(L)])] for p, L in zip(sel["pos"], plen)], dtype=np.int64)
        want = wpref.by_bitmaps(head, cb, sel["pos"], plen, pidx, v)
        m = int(torch.searchsorted(d_pos[:n_tok].to(torch.int64), torch.tensor([cb], device="cuda:0"))[0])
        if m != want[0].size or not np.array_equal(d_ids[:m].cpu().numpy(), want[0]) or \
                not np.array_equal(d_pos[:m].cpu().numpy().view(np.uint32), want[1]):
            raise SystemExit(f"wordpiece_bench: the tokens of the first {cb} bytes differ from the reference's")
        ms = {"filter_roles": [], "filter_words": [], "wordpiece": [], "tokenize": []}
        kept_words = 0
        for step in range(warmup + steps):
            t = {"wordpiece": event_ms(stream, wordpiece), "tokenize": event_ms(stream, tokenize)}
            scan()
            t["filter_words"] = event_ms(stream, lambda: g.filter_whole_words(0, d_input=buf))
            kept_words = g.last_count()
            scan()
            t["filter_roles"] = event_ms(stream, lambda: g.filter_roles(0, d_input=buf))
            assert g.last_count() == kept
            assert g.select_leftmost_longest(0, d_out=d_sel, out_cap=n_sel)[0] == n_sel    # (the token passes' selection again)
            if step >= warmup:
                for key, val in t.items():
                    ms[key].append(val)
        text = bytes(buf[:min(n, host_bytes)].cpu().numpy())
        rb = g.scan_format()[0]
        del buf, d_sel, d_ids, d_pos
    torch.cuda.empty_cache()
    fr, fw, wp, tk = stats(ms["filter_roles"]), stats(ms["filter_words"]), stats(ms["wordpiece"]), stats(ms["tokenize"])
    n_tiles = (n + 4095) // 4096
    moved = 2 * n + 8 * n_sel + 2 * 2048 * n_tiles + 4 * n_tok
    fmoved = total * rb + kept * rb + total * 10
    out = {"bytes": n, "vocabulary_entries": len(entries), "skipped_entries": len(skipped), "matches": total, "kept_by_roles": kept,
           "kept_by_whole_words": kept_words, "selected": n_sel, "tokens": n_tok, "unk_tokens_checked": int((want[0] == 0).sum()),
           "plain_tokens": counts["tokenize"], "checked_bytes": cb, "checked_tokens": m,
           "filter_roles_ms": fr[0], "filter_roles_ms_min_max": fr[1], "filter_words_ms": fw[0], "filter_words_ms_min_max": fw[1],
           "filter_roles_over_words": round(fr[0] / fw[0], 3), "filter_counted_bytes": fmoved,
           "filter_roles_gb_per_s": round(fmoved / fr[0] / 1e6, 1),
           "wordpiece_ms": wp[0], "wordpiece_ms_min_max": wp[1], "tokenize_ms": tk[0], "tokenize_ms_min_max": tk[1],
           "wordpiece_over_tokenize": round(wp[0] / tk[0], 3), "wordpiece_counted_bytes": moved,
           "wordpiece_gb_per_s": round(moved / wp[0] / 1e6, 1)}
    host = host_path(entries, text)
    if host is not None:
        out.update(host)
        out["wordpiece_ms_scaled_to_host_bytes"] = round(wp[0] * len(text) / n, 3)
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
    out = {"metric": "role filter vs whole-word filter; WordPiece token pass vs the plain tokenize of the same selection; host path",
           "steps": args.steps, "warmup": args.warmup}
    out.update(run(args.bytes, args.steps, args.warmup, args.host_bytes, args.check_bytes))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
