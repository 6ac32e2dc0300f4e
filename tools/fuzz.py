"""GPU differential fuzz: random pattern sets x random inputs, random kernel knobs; every record of the scan, the
documents pass, the leftmost-longest selection and the find-and-replace output compared with the CPU references.
The cases and checks are tests/passfuzz.py's (the suite runs a fixed list of its seeds).
usage: fuzz.py [seconds] [seed]
       fuzz.py session [seconds] [seed]     random SESSIONS instead: one context per plan driven through about 60 calls
                                            in random order (tests/session.py: the model, plans and executor of the suite);
                                            the plans rotate through the four families: plain, with the whole-word filter
                                            among the calls (plan(seed, words=True): filtered scans read by every pass and
                                            reader, results fetched across a filter), and with the per-pattern counts as well
                                            (plan(seed, counts=True): counts accumulated and fetched late, count knobs),
                                            and with the line path as well (plan(seed, lines=True): the delimiter split,
                                            matching documents with context lines, and the gather of their bytes)
       fuzz.py verdict [seconds] [seed]     random VERDICT sessions instead (tests/verdictsession.py): one context per plan driven
                                            through about 160 calls of the pattern groups, the document scores, the rank and both
                                            gathers in random order, results fetched late behind scans, uploads, filters, reserves,
                                            new offsets and stream changes -- plan(seed) for seeds past the suite's.  One child
                                            process per plan under a time limit; the first child that fails, ends by a signal or
                                            runs over stops the tool
       fuzz.py class [seconds] [seed]       character-class and escaped-file cases instead (tests/classfuzz.py), against the
                                            brute-force matcher oracle/charclass_oracle.py and the escape-aware CPU oracle
       fuzz.py guard [seconds] [seed]       the capacity contract instead (tests/heapguard.py): the scan of random cases into
                                            guarded record heaps of random capacities -- count, overflow flag, hint, records,
                                            heap layout, guards.  Every case runs in a child process of its own under a time
                                            limit; the first failure (or a child that dies or runs over) stops the tool
       fuzz.py words [seconds] [seed]       the whole-word filter instead (tests/wordfuzz.py): random word / phrase sets,
                                            edges, word sets, neighbour bytes and document cuts -- the filtered records,
                                            the selection and the replacement or the document cut behind the filter,
                                            against tests/wordref.py over the CPU oracle's records.  One child process
                                            per case under a time limit, as `guard`
       fuzz.py late [seconds] [seed]        the passes behind those instead (tests/latefuzz.py): the span filter, the group
                                            masks with their predicate and the gather, the per-document selection, replacement
                                            templates and match extraction per document and over the whole stream, the plain
                                            replace on the same selection -- exact and case-folded tables, lines cut on the
                                            device or explicit offsets, every step against the host references over the CPU
                                            oracle's records.  One child process per case under a time limit, as `guard`
       fuzz.py rank [seconds] [seed]        the passes behind those instead (tests/rankfuzz.py): document scores behind a drawn
                                            filter (none, whole words, spans), the score rule and the gather, three top draws
                                            and the formatted gather of a ranked one, the context path (segment, matching
                                            documents with context, the formatted gather under context_sep), the selection's
                                            scores and their rank, every fourth case again into the caller's buffers -- document
                                            counts from 1 to about 40 000, every step against the host references over the CPU
                                            oracle's records.  One child process per case under a time limit, as `guard`"""
import os, sys, tempfile, time
os.environ.setdefault("PFAC_ENABLE_KNOBS", "1")     # tuning / test knobs of libpfac_hip.so are opt-in
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from phfpfac_amd import GpuMatcher, PfacTable
from orc import Oracle
from passfuzz import KNOB_NAMES, KNOBS, Case, knob_label, run_case

if len(sys.argv) > 1 and sys.argv[1] == "session":
    import session as S
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    t0 = t_last = time.time(); plans = 0; tot = {"ops": 0, "errors": 0, "compared": 0, "filters": 0, "counts": 0, "splits": 0, "matchings": 0, "gathers": 0, "ids": 0}; widths = set(); staging = set()
    regimes = set()
    while time.time() - t0 < seconds:
        plan_seed = (seed << 20) + len(S.SEEDS) + plans // 4   # (beyond the suite's seeds; the four families in turn)
        family = ("", "words", "counts", "lines")[plans % 4]
        with GpuMatcher(0, S.N_SLOTS) as g:
            try:
                st = S.run(g, S.plan(plan_seed, words=family == "words", counts=family == "counts", lines=family == "lines"), S.Model(),
                           seed=f"{plan_seed} ({family})" if family else plan_seed)
            except AssertionError as e:
                raise SystemExit(f"MISMATCH in plan {plans}: {e}")
        for k in tot: tot[k] += st.get(k, 0)
        widths |= st["widths"]; staging |= st["staging"]; regimes |= st["regimes"]; plans += 1
        if time.time() - t_last > 30:
            t_last = time.time(); print(f"  ... {plans} plans, {tot['ops']} operations, {tot['compared']} records and bytes compared, {t_last - t0:.0f} s", flush=True)
    print(f"session fuzz ok: {plans} plans in {time.time() - t0:.0f} s (seed {seed}), {tot['ops']} operations of which {tot['errors']} "
          f"documented errors, {tot['filters']} whole-word filters, {tot['counts']} counts, {tot['splits']} splits, {tot['matchings']} matching calls and {tot['gathers']} "
          f"gathers, {tot['compared']} records and bytes and {tot['ids']} document ids and offsets compared")
    print(f"record widths {sorted(widths)}, staging layouts (buffers, records) {sorted(staging)}, count regimes (overlay, regime) {sorted(regimes)}")
    raise SystemExit(0)
if len(sys.argv) > 1 and sys.argv[1] == "verdict-plan":        # one plan on the GPU (the child of `verdict` below)
    import verdictsession as V
    plan_seed = int(sys.argv[2])
    with GpuMatcher(0, V.N_SLOTS) as g:
        try:
            st = V.run(g, V.plan(plan_seed), V.Model(), seed=plan_seed)
        except AssertionError as e:
            raise SystemExit(f"MISMATCH: {e}")
    print(f"{st['ops']} {st['verdict']} {st['errors']} {st['docs']} {st['bytes']} " + ",".join(f"{r}:{n}" for r, n in st["rules"].items()))
    raise SystemExit(0)
if len(sys.argv) > 1 and sys.argv[1] == "verdict":
    import subprocess
    import verdictsession as V
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    STEP_LIMIT = 300                                           # seconds one plan may take (the references of a 130-tile input, 160 calls)
    t0 = t_last = time.time(); plans = 0; tot = [0, 0, 0, 0, 0]; rules = {r: 0 for r in V.RULES}
    while time.time() - t0 < seconds:
        plan_seed = (seed << 20) + len(V.SEEDS) + plans        # (beyond the suite's seeds)
        try:                                                   # (this process never opens the GPU: every plan is a fresh child)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "verdict-plan", str(plan_seed)], capture_output=True,
                               text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"TIME LIMIT: plan {plans} (fuzz.py verdict-plan {plan_seed}) ran over {STEP_LIMIT} s; stopping")
        if r.returncode:
            how = f"signal {-r.returncode}" if r.returncode < 0 else f"exit status {r.returncode}"
            raise SystemExit(f"FAILED plan {plans} (fuzz.py verdict-plan {plan_seed}), {how}; stopping\n" + r.stdout[-2000:] + r.stderr[-4000:])
        *nums, seen = r.stdout.strip().split("\n")[-1].split(" ")
        tot = [a + int(b) for a, b in zip(tot, nums)]
        for item in seen.split(","):
            rules[item.split(":")[0]] += int(item.split(":")[1])
        plans += 1
        if time.time() - t_last > 30:
            t_last = time.time(); print(f"  ... {plans} plans, {tot[0]} operations, {t_last - t0:.0f} s", flush=True)
    print(f"verdict fuzz ok: {plans} plans in {time.time() - t0:.0f} s (seed {seed}), {tot[0]} operations of which {tot[1]} verdict operations and "
          f"{tot[2]} documented errors, {tot[3]} document entries and {tot[4]} bytes compared")
    print("operations in which a rule decided the outcome: " + ", ".join(f"{r} {n}" for r, n in rules.items()))
    raise SystemExit(0)
if len(sys.argv) > 1 and sys.argv[1] == "class":
    import classfuzz as F
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    rng = np.random.default_rng(seed)
    tmp = tempfile.mkdtemp()
    t0 = t_last = time.time(); cases = 0; recs = 0; per_knob = {}; kinds = {}
    while time.time() - t0 < seconds:
        case_seed = (seed << 32) + len(F.SEEDS) + cases        # (beyond the suite's seeds)
        knobs = KNOBS[int(rng.integers(0, len(KNOBS)))]
        c = F.ClassCase(case_seed, knobs)
        for k in KNOB_NAMES: os.environ.pop(k, None)
        os.environ.update(knobs)
        try:
            recs += F.run_class_case(lambda: GpuMatcher(0, 1), c, tmp)
        except AssertionError as e:
            raise SystemExit(f"MISMATCH case {cases} (ClassCase({case_seed}, {knobs})): {e}")
        per_knob[knob_label(knobs)] = per_knob.get(knob_label(knobs), 0) + 1
        kinds[c.kind] = kinds.get(c.kind, 0) + 1
        cases += 1
        if time.time() - t_last > 30:
            t_last = time.time(); print(f"  ... {cases} cases, {recs} records compared, {t_last - t0:.0f} s", flush=True)
    print(f"class fuzz ok: {cases} cases in {time.time() - t0:.0f} s (seed {seed}; {', '.join(f'{v} {k}' for k, v in sorted(kinds.items()))}), "
          f"{recs} records compared (scan x2, documents, selection, replace, outputs lists, GPU text)")
    print("cases per knob set: " + ", ".join(f"{k} {v}" for k, v in sorted(per_knob.items())))
    raise SystemExit(0)
if len(sys.argv) > 1 and sys.argv[1] == "guard-case":         # one case on the GPU (the child of `guard` below)
    import torch
    import heapguard as H
    from passfuzz import record_width
    case_seed = int(sys.argv[2])
    rng = np.random.default_rng([case_seed, 0x4755415244])
    knobs = KNOBS[int(rng.integers(0, len(KNOBS)))]
    c = Case(case_seed, knobs)
    for k in KNOB_NAMES: os.environ.pop(k, None)
    os.environ.update(knobs)
    pf = c.write_patterns(os.path.join(tempfile.mkdtemp(), "guard.pat"))
    o = Oracle(pf, 1, 1); want = H.oracle_want(o, c.data, c.n_owned, c.n); o.close()
    table = PfacTable.from_file(pf, c.width)
    rb = record_width(table.num_final, knobs)
    P = want.padded(rb)
    d_in = torch.from_numpy(np.concatenate([c.data, np.zeros(2 * H.TILE, np.uint8)])).to("cuda:0")
    scans = 0
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        hints = []
        first = H.verdict(g, table, want, d_in, c.n_owned, c.n, 0, rb, H.FILLS[0], hints, c.describe())
        ladder = H.capacity_ladder(want.n, P, first["hint"])
        caps = [int(x) for x in rng.choice(ladder, min(len(ladder), 12), replace=False)] + \
               [int(x) for x in rng.integers(0, 4 * first["hint"] + 1, 6)] + [int(x) for x in rng.integers(max(P - 64, 0), P + 65, 6)]
        for k, cap in enumerate(caps):
            H.verdict(g, table, want, d_in, c.n_owned, c.n, cap, rb, H.FILLS[k % 2], hints, c.describe())
            scans += 1
    print(f"{scans} {want.n} {knob_label(knobs)}")
    raise SystemExit(0)
if len(sys.argv) > 1 and sys.argv[1] == "guard":
    import subprocess
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    STEP_LIMIT = 300                                           # seconds one case may take (oracle + some twenty scans)
    t0 = t_last = time.time(); cases = 0; scans = 0; recs = 0; per_knob = {}
    while time.time() - t0 < seconds:
        case_seed = (seed << 32) + cases
        try:                                                   # (this process never opens the GPU: every step is a fresh child)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "guard-case", str(case_seed)], capture_output=True,
                               text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"TIME LIMIT: case {cases} (fuzz.py guard-case {case_seed}) ran over {STEP_LIMIT} s; stopping")
        if r.returncode:
            raise SystemExit(f"FAILED case {cases} (fuzz.py guard-case {case_seed}), exit status {r.returncode}; stopping\n"
                             + r.stdout[-2000:] + r.stderr[-4000:])
        k, n, label = r.stdout.strip().split("\n")[-1].split(" ", 2)
        scans += int(k); recs += int(n) ; per_knob[label] = per_knob.get(label, 0) + 1; cases += 1
        if time.time() - t_last > 30:
            t_last = time.time(); print(f"  ... {cases} cases, {scans} guarded scans, {t_last - t0:.0f} s", flush=True)
    print(f"guard fuzz ok: {cases} cases in {time.time() - t0:.0f} s (seed {seed}), {scans} scans into guarded heaps, "
          f"{recs} matches per ladder in all")
    print("cases per knob set: " + ", ".join(f"{k} {v}" for k, v in sorted(per_knob.items())))
    raise SystemExit(0)
if len(sys.argv) > 1 and sys.argv[1] == "words-case":         # one case on the GPU (the child of `words` below)
    import wordfuzz as W
    case_seed = int(sys.argv[2])
    c = W.WordCase(case_seed, W.KNOBS[int(np.random.default_rng([case_seed, 0x4B4E4F42]).integers(0, len(W.KNOBS)))])
    for k in set(KNOB_NAMES) | set(W.KNOB_NAMES): os.environ.pop(k, None)
    os.environ.update(c.knobs)
    try:
        n = W.run_word_case(lambda: GpuMatcher(0, 1), c, tempfile.mkdtemp())
    except AssertionError as e:
        raise SystemExit(f"MISMATCH: {e}")
    print(f"{n} {knob_label(c.knobs)}")
    raise SystemExit(0)
if len(sys.argv) > 1 and sys.argv[1] == "words":
    import subprocess
    import wordfuzz as W
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    STEP_LIMIT = 120                                           # seconds one case may take
    t0 = t_last = time.time(); cases = 0; recs = 0; per_knob = {}
    while time.time() - t0 < seconds:
        case_seed = (seed << 32) + len(W.SEEDS) + cases        # (beyond the suite's seeds)
        try:                                                   # (this process never opens the GPU: every case is a fresh child)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "words-case", str(case_seed)], capture_output=True,
                               text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"TIME LIMIT: case {cases} (fuzz.py words-case {case_seed}) ran over {STEP_LIMIT} s; stopping")
        if r.returncode:
            raise SystemExit(f"FAILED case {cases} (fuzz.py words-case {case_seed}), exit status {r.returncode}; stopping\n"
                             + r.stdout[-2000:] + r.stderr[-4000:])
        n, label = r.stdout.strip().split("\n")[-1].split(" ", 1)
        recs += int(n); per_knob[label] = per_knob.get(label, 0) + 1; cases += 1
        if time.time() - t_last > 30:
            t_last = time.time(); print(f"  ... {cases} cases, {recs} records compared, {t_last - t0:.0f} s", flush=True)
    print(f"words fuzz ok: {cases} cases in {time.time() - t0:.0f} s (seed {seed}), {recs} records compared (scan, filter, "
          f"selection + replace or documents)")
    print("cases per knob set: " + ", ".join(f"{k} {v}" for k, v in sorted(per_knob.items())))
    raise SystemExit(0)
if len(sys.argv) > 1 and sys.argv[1] == "late-case":          # one case on the GPU (the child of `late` below)
    import latefuzz as LF
    case_seed = int(sys.argv[2])
    c = LF.LateCase(case_seed, LF.KNOBS[int(np.random.default_rng([case_seed, 0x4B4E4F42]).integers(0, len(LF.KNOBS)))])
    for k in set(KNOB_NAMES) | set(LF.KNOB_NAMES): os.environ.pop(k, None)
    os.environ.update(c.knobs)
    try:
        n_rec, n_bytes = LF.run_late_case(lambda: GpuMatcher(0, 1), c, tempfile.mkdtemp())
    except AssertionError as e:
        raise SystemExit(f"MISMATCH: {e}")
    print(f"{n_rec} {n_bytes} {knob_label(c.knobs)}")
    raise SystemExit(0)
if len(sys.argv) > 1 and sys.argv[1] == "late":
    import subprocess
    import latefuzz as LF
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    STEP_LIMIT = 120                                           # seconds one case may take
    t0 = t_last = time.time(); cases = 0; recs = 0; nbytes = 0; per_knob = {}
    while time.time() - t0 < seconds:
        case_seed = (seed << 32) + len(LF.SEEDS) + cases       # (beyond the suite's seeds)
        try:                                                   # (this process never opens the GPU: every case is a fresh child)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "late-case", str(case_seed)], capture_output=True,
                               text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"TIME LIMIT: case {cases} (fuzz.py late-case {case_seed}) ran over {STEP_LIMIT} s; stopping")
        if r.returncode:
            raise SystemExit(f"FAILED case {cases} (fuzz.py late-case {case_seed}), exit status {r.returncode}; stopping\n"
                             + r.stdout[-2000:] + r.stderr[-4000:])
        n, b, label = r.stdout.strip().split("\n")[-1].split(" ", 2)
        recs += int(n); nbytes += int(b); per_knob[label] = per_knob.get(label, 0) + 1; cases += 1
        if time.time() - t_last > 30:
            t_last = time.time(); print(f"  ... {cases} cases, {recs} records and {nbytes} bytes compared, {t_last - t0:.0f} s", flush=True)
    print(f"late fuzz ok: {cases} cases in {time.time() - t0:.0f} s (seed {seed}), {recs} records and {nbytes} bytes compared (scan, "
          f"span filter, group masks + gather, selections, templated replace + extraction, plain replace)")
    print("cases per knob set: " + ", ".join(f"{k} {v}" for k, v in sorted(per_knob.items())))
    raise SystemExit(0)
if len(sys.argv) > 1 and sys.argv[1] == "rank-case":          # one case on the GPU (the child of `rank` below)
    import rankfuzz as RF
    case_seed = int(sys.argv[2])
    c = RF.RankCase(case_seed, RF.KNOBS[int(np.random.default_rng([case_seed, 0x4B4E4F42]).integers(0, len(RF.KNOBS)))])
    for k in set(KNOB_NAMES) | set(RF.KNOB_NAMES): os.environ.pop(k, None)
    os.environ.update(c.knobs)
    try:
        n_rec, n_doc, n_bytes = RF.run_rank_case(lambda: GpuMatcher(0, 1), c, tempfile.mkdtemp())
    except AssertionError as e:
        raise SystemExit(f"MISMATCH: {e}")
    print(f"{n_rec} {n_doc} {n_bytes} {knob_label(c.knobs)}")
    raise SystemExit(0)
if len(sys.argv) > 1 and sys.argv[1] == "rank":
    import subprocess
    import rankfuzz as RF
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    STEP_LIMIT = 120                                           # seconds one case may take
    t0 = t_last = time.time(); cases = 0; recs = 0; ndocs = 0; nbytes = 0; per_knob = {}
    while time.time() - t0 < seconds:
        case_seed = (seed << 32) + len(RF.SEEDS) + cases       # (beyond the suite's seeds)
        try:                                                   # (this process never opens the GPU: every case is a fresh child)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "rank-case", str(case_seed)], capture_output=True,
                               text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"TIME LIMIT: case {cases} (fuzz.py rank-case {case_seed}) ran over {STEP_LIMIT} s; stopping")
        if r.returncode:
            raise SystemExit(f"FAILED case {cases} (fuzz.py rank-case {case_seed}), exit status {r.returncode}; stopping\n"
                             + r.stdout[-2000:] + r.stderr[-4000:])
        n, d, b, label = r.stdout.strip().split("\n")[-1].split(" ", 3)
        recs += int(n); ndocs += int(d); nbytes += int(b); per_knob[label] = per_knob.get(label, 0) + 1; cases += 1
        if time.time() - t_last > 30:
            t_last = time.time(); print(f"  ... {cases} cases, {recs} records, {ndocs} document entries and {nbytes} bytes compared, {t_last - t0:.0f} s", flush=True)
    print(f"rank fuzz ok: {cases} cases in {time.time() - t0:.0f} s (seed {seed}), {recs} records, {ndocs} document entries and {nbytes} "
          f"bytes compared (scan, filter, scores x2 + rule + gather, three ranks + formatted gather, context path, selection scores)")
    print("cases per knob set: " + ", ".join(f"{k} {v}" for k, v in sorted(per_knob.items())))
    raise SystemExit(0)
seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = np.random.default_rng(seed)
tmp = tempfile.mkdtemp()
t0 = t_last = time.time(); cases = 0; recs = 0; per_knob = {}
while time.time() - t0 < seconds:
    case_seed = (seed << 32) + cases
    knobs = KNOBS[int(rng.integers(0, len(KNOBS)))]
    c = Case(case_seed, knobs)
    for k in KNOB_NAMES: os.environ.pop(k, None)
    os.environ.update(knobs)
    try:
        recs += run_case(lambda: GpuMatcher(0, 1), c, tmp)
    except AssertionError as e:
        raise SystemExit(f"MISMATCH case {cases} (Case({case_seed}, {knobs})): {e}")
    per_knob[knob_label(knobs)] = per_knob.get(knob_label(knobs), 0) + 1
    if c.n_owned and rng.random() < 0.5:                   # the GPU-side text emitter against lines formatted here
        pf = c.write_patterns(os.path.join(tmp, "text.pat"))
        o = Oracle(pf, 1, 1); pos, ids = o.scan_spec(c.data, None); o.close()
        own = pos < c.n_owned
        pos, ids = pos[own], ids[own]
        if pos.size < 400000:
            with GpuMatcher(0, 1) as g:
                g.load_table(PfacTable.from_file(pf, c.width))
                g.scan_bytes(c.data, c.n_owned)
                base = int(rng.choice([0, 999_999_990, 3 << 32]))
                text = g.text_to_host(g.emit_text_device(base))
            want = "".join("At position %4d, match pattern %d\n" % (p + base, i) for p, i in zip(pos.tolist(), ids.tolist())).encode()
            if text != want:
                raise SystemExit(f"TEXT MISMATCH case {cases}: {c.describe()} base {base}: {len(text)} bytes, want {len(want)}")
    cases += 1
    if time.time() - t_last > 30:
        t_last = time.time(); print(f"  ... {cases} cases, {recs} records compared, {t_last - t0:.0f} s", flush=True)
print(f"fuzz ok: {cases} cases in {time.time() - t0:.0f} s (seed {seed}), {recs} records compared (scan x2, documents, "
      f"selection, replace)")
print("cases per knob set: " + ", ".join(f"{k} {v}" for k, v in sorted(per_knob.items())))
