"""Verdict sessions: ONE GpuMatcher context driven through long sequences of the calls behind the scan that hold the most
state -- pattern groups and their masks, document scores, the rank and both gathers (tests/verdictsession.py) -- every
result compared bit for bit with what include/pfac.h promises for that history.  The random plans are the suite's 24
seeds; the named sessions are histories random plans reach rarely.  Run with -m gpu on an MI355X.  Expectations come
from the CPU oracle, wordref, llref, groupref, scoreref, topref, gatherref, fmtref and splitref, never from the device.
No session aims at a fault: they provoke the errors the header documents, nothing else."""
import pytest

import verdictsession as V
from phfpfac_amd import GpuMatcher
from verdictsession import E_ARG, E_OVERFLOW, E_STATE, OK, U64_MAX

pytestmark = pytest.mark.gpu

X = V.pool()


def run(steps):
    """The operations on one fresh context.  `steps`: operations, or (operation, status) where the header refuses the
    call; the model must agree before anything runs."""
    ops = [s[0] if isinstance(s, tuple) else s for s in steps]
    want = [s[1] if isinstance(s, tuple) else OK for s in steps]
    probe = V.Model()
    got = [probe.apply(op).status for op in ops]
    assert got == want, [(k, V.fmt(op), V.STATUS_NAMES[g], V.STATUS_NAMES[w]) for k, (op, g, w) in enumerate(zip(ops, got, want)) if g != w]
    with GpuMatcher(0, V.N_SLOTS) as g:
        return V.run(g, ops, V.Model(), seed="named")


def load(tab, gkey="g0", wkey="w0", knob=None):
    return [dict(op="load_table", tab=tab, knob=V.VTABLES[tab][0] if knob is None else knob), dict(op="set_flen"),
            dict(op="set_groups", key=gkey, ns="ok"), dict(op="set_weights", key=wkey, ns="ok")]


def scan(inp, slot=0, no="all"):
    return dict(op="scan", slot=slot, inp=inp, no=no)


def split(slot=0):
    return dict(op="split", slot=slot)


def doc(tab, inp, form, slot=0):
    return dict(op="set_doc", slot=slot, tab=tab, inp=inp, form=form)


def masks(slot=0, out="own", heap="own", nd="ok"):
    return dict(op="masks", slot=slot, out=out, heap=heap, nd=nd)


def scores(slot=0, out="own", heap="own", nd="ok"):
    return dict(op="scores", slot=slot, out=out, heap=heap, nd=nd)


def top(k, flags=V.topref.RANKED, slot=0, src="own", rule=0, out="own"):
    return dict(op="top", slot=slot, src=src, rule=rule, k=k, flags=flags, nd="ok", out=out)


def match_scores(rule=1, slot=0, src="own", out="own"):
    return dict(op="match_scores", slot=slot, src=src, rule=rule, nd="ok", out=out)


def match_groups(pred=0, slot=0, src="own", out="own"):
    return dict(op="match_groups", slot=slot, src=src, pred=pred, nd="ok", out=out)


def gather(slot=0, ids="own", out="own", f=None):
    op = dict(op="gather" if f is None else "gather_format", slot=slot, ids=ids, ni="ok", out=out)
    return op if f is None else dict(op, f=f)


def fetch(kind, slot=0, first=0, n=None):
    return dict(op=kind, slot=slot) if n is None else dict(op=kind, slot=slot, first=first, n=n)


def whole(ops, kind, slot=0):
    """The fetch of the whole slot-owned result that `ops` leaves for `kind`."""
    m = V.Model()
    for op in ops:
        m.apply(op[0] if isinstance(op, tuple) else op)
    r = getattr(m.slots[slot], "ga" if kind == "ga_fetch" else kind[:-6])
    return fetch(kind, slot, 0, r["n"])


@pytest.mark.parametrize("seed", V.SEEDS)
def test_session(seed):
    """One random plan on one context."""
    ops = V.plan(seed)
    with GpuMatcher(0, V.N_SLOTS) as g:
        st = V.run(g, ops, V.Model(), seed=seed)
    print(f"verdict session {seed}: {st['ops']} operations ({st['verdict']} verdict operations, {st['errors']} documented errors), "
          f"{st['docs']} document entries and {st['bytes']} bytes compared, record widths {sorted(st['widths'])}, rules observed "
          f"{ {r: n for r, n in st['rules'].items() if n} }, {len(st['late'])} (result, event) pairs of R9")


def test_a_matching_call_behind_the_rank_leaves_the_pairs_and_hands_its_own_ids_on():
    """R1, R2, R3: rank, then matching(min_count=1): top_fetch is still the rank's pairs, gather(NULL) takes the
    matching's ids, ids_fetch returns them."""
    ops = load("abc2") + [scan(0), split(), scores(), top(65), match_scores(1)]
    ops += [fetch("top_fetch", 0, 0, 65), gather(), whole(ops + [gather()], "ga_fetch"), fetch("gaoff_fetch"), fetch("ids_fetch")]
    st = run(ops)
    assert st["rules"]["R3"] and st["rules"]["R2"] >= 2


def test_a_call_into_the_callers_buffer_leaves_no_slot_owned_scores_or_masks():
    """R4, R5: scores (slot), scores (caller's guarded buffer): matching_scores(NULL) and the fetch are PFAC_E_STATE."""
    ops = load("mid4") + [scan(0), doc("mid4", 0, "host"), scores(), fetch("scores_fetch", 0, 0, 5), scores(out="caller"),
                          (match_scores(1), E_STATE), (fetch("scores_fetch", 0, 0, 1), E_STATE), (top(5), E_STATE), match_scores(1, src="caller"),
                          masks(), fetch("masks_fetch", 0, 3, 7), masks(out="caller"), (match_groups(0), E_STATE),
                          (fetch("masks_fetch", 0, 0, 1), E_STATE), match_groups(2, src="caller"), fetch("ids_fetch")]
    run(ops)


def test_a_failed_formatted_gather_discards_the_plain_gathers_result():
    """R6: gather, then a gather_format refused for a bad id: both fetches are PFAC_E_STATE; then a good format; then
    the all-zero format is byte for byte the plain gather."""
    base = load("cclass") + [scan(0), split(), masks(), match_groups(0), gather()]
    ops = base + [whole(base, "ga_fetch"), (gather(ids="bad_id", f=1), E_ARG), (fetch("ga_fetch", 0, 0, 1), E_STATE), (fetch("gaoff_fetch"), E_STATE),
                  fetch("ids_fetch"), gather(f=1)]
    ops += [whole(ops, "ga_fetch"), fetch("gaoff_fetch"), gather(f=0)]
    ops += [whole(ops, "ga_fetch"), fetch("gaoff_fetch"), gather()]
    ops += [whole(ops, "ga_fetch"), fetch("gaoff_fetch"), gather(out="caller", f=0), (fetch("gaoff_fetch"), E_STATE)]
    run(ops)


def test_a_queued_pass_keeps_the_weights_and_groups_it_was_launched_with():
    """R7: scores queued, set_state_weights at once, no sync: the fetch returns the old weights' sums, a second pass the
    new ones; a setter with the wrong n_states changes nothing.  The same for the groups."""
    base = load("abc2", "g0", "w0") + [scan(1), split(), scores(), dict(op="set_weights", key="w1", ns="ok")]
    ops = base + [whole(base, "scores_fetch"), scores()]
    ops += [whole(ops, "scores_fetch"), (dict(op="set_weights", key="w0", ns="wrong"), E_ARG), scores()]
    ops += [whole(ops, "scores_fetch"), masks(), dict(op="set_groups", key="g1", ns="ok")]
    ops += [whole(ops, "masks_fetch"), masks()]
    ops += [whole(ops, "masks_fetch"), (dict(op="set_groups", key="g0", ns="wrong"), E_ARG), masks()]
    ops += [whole(ops, "masks_fetch")]
    st = run(ops)
    assert st["rules"]["R7"] >= 8


def test_every_result_of_a_large_input_outlives_everything_behind_it():
    """R9: masks, scores, ids, pairs and the formatted text of a 130-tile input, fetched behind an upload of another
    table, a scan of a 3-tile input under another record width, a whole-word filter, a reserve that replaces the input and
    record buffers and new offsets."""
    base = load("abc2") + [scan(2), split(), masks(), scores(), top(U64_MAX, rule=1), gather(f=4)]
    ops = base + load("cclass") + [scan(0), dict(op="filter", slot=0), dict(op="reserve_grow", slot=0, k=1), doc("cclass", 0, "one")]
    ops += [whole(base, k) for k in ("masks_fetch", "scores_fetch", "top_fetch", "ga_fetch")] + [fetch("ids_fetch"), fetch("gaoff_fetch")]
    st = run(ops)
    assert {e for _, e in st["late"]} >= {"upload", "scan", "filter", "reserve", "offsets"} and {r for r, _ in st["late"]} == set(V.RESULTS)
    assert st["widths"] == {2, 8}


def test_large_then_tiny_then_large_behind_a_queued_formatted_gather():
    """The sort's two buffers, the histograms and the id buffer shrink and regrow (n_docs above 16 384, then 1, then
    above 16 384; n_top above 1 024, then 1, then above 1 024) behind a formatted gather that is still reading the ids."""
    t = "abc2"
    base = load(t) + [scan(2), split(), scores(), top(U64_MAX, rule=1), gather(f=1)]
    assert X.n_docs((t, 2, "split")) > 16384
    tiny = base + [doc(t, 2, "one"), scores(), top(1)]
    ops = tiny + [whole(base, "ga_fetch"), fetch("gaoff_fetch"), fetch("top_fetch", 0, 0, 1), gather(f=4)]
    ops += [whole(ops, "ga_fetch"), split(), scores(), top(U64_MAX, flags=V.topref.RANKED | V.topref.BY_COUNT), gather(f=3), doc(t, 2, "one"), scores(), top(1)]
    ops += [whole(ops[:-3], "ga_fetch"), fetch("gaoff_fetch"), fetch("ids_fetch")]
    st = run(ops)
    assert st["docs"] > 30000


def test_a_stream_change_between_a_producer_and_its_consumer():
    """Slot 1 moves to slot 0's stream between top_scores and the gather_format that consumes its ids, and back between
    the scores and top_scores(NULL)."""
    base = load("mid4") + [scan(1, slot=1), split(1), scores(1), dict(op="set_stream", slot=1, share=True), top(V.SORT_BLOCK + 1, slot=1),
                           dict(op="set_stream", slot=1, share=False), gather(1, f=1)]
    ops = base + [whole(base, "ga_fetch", 1), scores(1), dict(op="set_stream", slot=1, share=True), top(65, slot=1, flags=V.topref.RANKED | V.topref.LOWEST),
                  fetch("ids_fetch", 1), fetch("top_fetch", 1, 0, 65)]
    run(ops)


@pytest.mark.parametrize("share", [True, False], ids=["shared-stream", "own-streams"])
def test_two_slots_rank_and_gather_side_by_side(share):
    """One slot ranks while the other uploads its input and scans; both then gather: neither slot's ids, pairs or text
    show the other's."""
    base = ([dict(op="set_stream", slot=1, share=True)] if share else []) + load("abc2")
    base += [scan(1, 0), split(0), scores(0), scan(0, 1), top(V.SORT_BLOCK - 1, slot=0), split(1), scores(1), top(64, slot=1, flags=V.topref.RANKED | V.topref.BY_COUNT),
             gather(0, f=1), gather(1)]
    ops = base + [whole(base, "ga_fetch", 0), whole(base, "ga_fetch", 1), fetch("ids_fetch", 0), fetch("ids_fetch", 1),
                  whole(base, "top_fetch", 0), whole(base, "top_fetch", 1), fetch("gaoff_fetch", 1), fetch("gaoff_fetch", 0)]
    run(ops)


def test_the_scores_of_the_slots_own_selection():
    """R10: selection_document_scores(NULL, NULL) behind a per-document selection, with top_scores(NULL) over it; behind a
    later scan and behind a selection into the caller's buffers it is PFAC_E_STATE; one pointer NULL is PFAC_E_ARG."""
    sel = lambda out="own": dict(op="select_docs", slot=0, out=out)                   # noqa: E731
    ss = lambda src="own", out="own": dict(op="sel_scores", slot=0, src=src, out=out)   # noqa: E731
    base = load("cclass") + [scan(0), split(), sel(), ss()]
    ops = base + [whole(base, "scores_fetch"), top(65), fetch("ids_fetch"), (ss("half"), E_ARG), (fetch("scores_fetch", 0, 0, 1), E_STATE),
                  ss(), scan(0), (ss(), E_STATE), sel("caller"), (ss(), E_STATE), ss("caller"), top(3, rule=1), ss("caller", "caller"),
                  (top(3), E_STATE), sel(), dict(op="filter", slot=0), (ss(), E_STATE)]
    st = run(ops)
    assert st["rules"]["R10"] >= 8


def test_the_error_ladder_of_the_mask_and_score_passes_one_rung_at_a_time():
    """R8: PFAC_E_STATE (a scan of an earlier table, no lengths, no groups or weights, an n_docs that is not the
    offsets'), then PFAC_E_OVERFLOW, then PFAC_E_ARG (offsets that break the rules, a foreign heap, a misaligned buffer);
    every refused call leaves its guarded buffer untouched and the slot's earlier masks or scores discarded."""
    t = "mid4"
    gone_m, gone_s = (fetch("masks_fetch", 0, 0, 1), E_STATE), (fetch("scores_fetch", 0, 0, 1), E_STATE)
    up = dict(op="load_table", tab=t, knob=V.VTABLES[t][1])
    ops = [(masks(out="caller"), E_STATE)] + load(t) + [(scores(out="caller"), E_STATE), scan(0), (masks(out="caller", nd="more"), E_STATE),
                                                        split(), masks(), scores(),
                                                        up, (masks(out="caller"), E_STATE), gone_m, scan(0), (scores(out="caller"), E_STATE), gone_s,
                                                        dict(op="set_flen"), (masks(out="caller"), E_STATE), (scores(out="odd"), E_STATE),
                                                        dict(op="set_groups", key="g1", ns="ok"), dict(op="set_weights", key="w1", ns="ok"),
                                                        (masks(out="caller", nd="more"), E_STATE), masks(), scores(),
                                                        dict(op="scan_over", slot=0, inp=0), (masks(out="caller"), E_OVERFLOW), gone_m,
                                                        doc(t, 0, "bad_end"), (scores(out="odd"), E_OVERFLOW), gone_s,
                                                        scan(0), (masks(out="caller"), E_ARG), (scores(out="caller"), E_ARG),
                                                        doc(t, 0, "bad_order"), (masks(out="caller"), E_ARG), doc(t, 0, "host"), masks(), scores(),
                                                        (masks(out="caller", heap="foreign"), E_ARG), gone_m, (scores(out="odd"), E_ARG), gone_s,
                                                        masks(out="caller"), scores(out="caller"), masks(), scores()]
    ops += [whole(ops, "masks_fetch"), whole(ops, "scores_fetch")]
    st = run(ops)
    assert st["rules"]["R8"] >= 15
