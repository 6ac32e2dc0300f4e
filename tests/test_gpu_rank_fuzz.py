"""Document scores (pfac_documents_scores, pfac_selection_document_scores, pfac_documents_matching_scores), the rank
(pfac_documents_top_scores) and the formatted gather (pfac_documents_gather_format) behind a real scan, a real filter and
each other, on the seeded random cases of tests/rankfuzz.py under the knob sets that change the record form or the heap
layout; then eight of the cases in a row on ONE context.  Run with -m gpu on an MI355X.  Expectations come from the CPU
oracle and the host references alone (tests/test_rankfuzz_cases.py pins them, and what the inputs reach, without a
GPU).  Bit-exact."""
import numpy as np
import pytest

from phfpfac_amd import GpuMatcher, PfacError, _ffi
from rankfuzz import KNOB_NAMES, SEEDS, RankCase, case_id, expectation, record_width, run_rank_case

pytestmark = pytest.mark.gpu


def set_knobs(monkeypatch, knobs):
    for k in KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("seed", SEEDS, ids=[case_id(s) for s in SEEDS])
def test_rank_fuzz(seed, monkeypatch, tmp_path):
    """One random case (tests/rankfuzz.py): scan, offsets, the drawn filter, the scores twice, the score rule and the
    gather, three top draws and the formatted gather of a ranked one, the context path, the selection's scores and
    their rank; for seed % 4 == 3 the scores and the rank again into the caller's buffers."""
    case = RankCase(seed)
    set_knobs(monkeypatch, case.knobs)
    n_rec, n_doc, n_bytes = run_rank_case(lambda: GpuMatcher(0, 1), case, str(tmp_path))
    print(f"case {case.describe()}: {n_rec} records, {n_doc} document entries and {n_bytes} bytes compared")


# large -> tiny -> large -> 1 document, twice; the table's record width changes at every step
CHAIN = (19, 3, 39, 31, 42, 12, 27, 14)


def test_one_context_through_a_chain(monkeypatch, tmp_path):
    """Eight cases in a row on one long-lived context, nothing closed in between: `reserve` and `load_table` again for
    each, so the slot-owned scores, matching ids, top pairs, group sums and the sort's two buffers are reused at a
    smaller and then a larger size (16 454 -> 63 -> 39 917 -> 1 -> 40 179 -> 65 -> 12 293 -> 1 documents; n_top above
    2 048 -> below 64 -> above 1 024 -> 1 -> ...), under a record width that differs between neighbours.  The knobs
    are read once per table install (read_knobs in the library), not per context, so every case keeps its own knob
    set.  Behind each upload, in front of set_pattern_weights, document_scores is refused with PFAC_E_STATE: the
    weights belong to the uploaded table.  Then every step of run_rank_case passes on that context."""
    tmp = str(tmp_path)
    want = [expectation(s, tmp) for s in CHAIN]
    docs = [w.n_docs for _, w in want]
    tops = [max(t.n_top for t in w.tops) for _, w in want]
    widths = [record_width(c.table(f"{tmp}/rank_{c.seed}.pat").num_final, c.knobs) for c, _ in want]
    assert docs[0] > 16384 and docs[1] < 64 and docs[2] > 32768 and docs[3] == 1, docs
    assert docs[4] > 32768 and docs[5] < 4096 and docs[6] > 4096 and docs[7] == 1, docs
    assert tops[0] > 2048 and tops[1] < 64 and tops[2] > 1024 and tops[4] > 2048 and tops[5] < 64 and tops[6] > 1024, tops
    assert all(a != b for a, b in zip(widths, widths[1:])) and set(widths) == {2, 4, 8}, widths

    def refused(g, nd):
        with pytest.raises(PfacError) as e:
            g.document_scores(nd)
        assert e.value.status == _ffi.PFAC_E_STATE and "weights" in str(e.value), f"document_scores before the weights: {e.value}"

    tot = np.zeros(3, dtype=np.int64)
    with GpuMatcher(0, 1) as g:
        for c, w in want:
            set_knobs(monkeypatch, c.knobs)
            tot += run_rank_case(None, c, tmp, want=w, g=g, before_weights=refused)
    print(f"chain {CHAIN}: documents {docs}, largest n_top {tops}, record widths {widths}; {tot[0]} records, {tot[1]} document "
          f"entries and {tot[2]} bytes compared")
