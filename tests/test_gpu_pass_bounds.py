"""The passes' caller-owned DEVICE outputs at exact capacity, between guard bands (run with -m gpu on an MI355X): one
test per call of the ABI that writes into a caller's device buffer, each over the three record widths and the cases of
tests/passguard.py, each with both fills.  Every buffer is exactly as long as include/pfac.h asks for and lies between
4 KiB of known bytes; passguard.exact_call drives the capacity one too small (PFAC_E_OVERFLOW, the exact count, nothing
written), rule-breaking document offsets (PFAC_E_ARG, nothing written) and the exact capacity (payloads equal to the
CPU's, guards intact, read back).  Expectations come from passguard.Cpu alone -- tests/test_passguard_cases.py checks
them, and the preconditions of every case, without a GPU.  One context per record width serves the whole module; a scan
is repeated only when a test needs another one."""
import pytest

from heapguard import FILLS, GUARD
from passguard import DOC_SHAPES, FILTERED, LADDER, SEL_COUNTS, SIZE_CASES, WIDTHS, Device, cpu

pytestmark = pytest.mark.gpu

SCANS = SIZE_CASES + (FILTERED,)        # every input size, the halo, the scan without a record, and one filtered scan
WINDOWS = ("t130", "t130+words")
PACKED_VARIANTS = ("null", "heap", "zero")


def _ids(pairs):
    return [f"w{p[0]}-" + "-".join(str(v) for v in p[1:]) for p in pairs]


def _pairs(*names):
    return [(W, n) for W in WIDTHS for group in names for n in group]


@pytest.fixture(scope="module")
def device():
    made = {}

    def get(W):
        if W not in made:
            made[W] = Device(W)
        return made[W]
    yield get
    for d in made.values():
        d.close()


def _key(case):
    x = cpu()
    if case == "t130+words":
        return x.size_key("t130")[:3] + (True,)
    return x.size_key(case)


P_EXPAND = _pairs(SCANS) + [(W, "windows", s) for W in WIDTHS for s in WINDOWS]


@pytest.mark.parametrize("case", P_EXPAND, ids=_ids(P_EXPAND))
def test_expand(device, case):
    """pfac_records_expand: d_out of exactly n x 8 bytes.  Every scan whole (and the window one past its end refused);
    on the 130-tile scan, plain and filtered, windows that start and end at a tile's and at a 64-tile group's first
    and last record."""
    d = device(case[0])
    x = cpu()
    for fill in FILLS:
        if case[1] == "windows":
            key = _key(case[2])
            windows, (_, _, T) = x.windows(d.W, key)
            for first, n in windows:
                d.expand(key, first, n, fill, refuse_past_end=first + n == T)
        else:
            key = _key(case[1])
            T = int(x.scan(d.W, key)[0].size)
            d.expand(key, 0, T, fill, refuse_past_end=True)
            d.expand(key, T // 3, T // 2, fill)


P_PACKED = _pairs(SCANS) + [(W, "t65", v) for W in (2, 4) for v in PACKED_VARIANTS]


@pytest.mark.parametrize("case", P_PACKED, ids=_ids(P_PACKED))
def test_packed_device(device, case):
    """pfac_records_packed_device: d_words_out of exactly used x record_bytes, d_tile_index_out of exactly n_tiles x 8,
    decoded and compared with the oracle; d_words_out NULL or the heap itself, and n_words = 0, copy the index only; a scan
    of 8-byte records is refused (PFAC_E_STATE) with both buffers untouched."""
    d = device(case[0])
    for fill in FILLS:
        d.packed(_key(case[1]), fill, case[2] if len(case) > 2 else "both")


P_DOCS = [(W, n, "rand") for W in WIDTHS for n in SCANS] + [(W, "docs", s) for W in WIDTHS for s in DOC_SHAPES]


def _doc_case(case):
    x = cpu()
    return (x.doc_key(case[2]), case[2]) if case[1] == "docs" else (_key(case[1]), "rand")


@pytest.mark.parametrize("case", P_DOCS, ids=_ids(P_DOCS))
def test_segment(device, case):
    """pfac_records_segment: d_out of exactly n_kept x 8 bytes, d_doc_first of exactly (n_docs + 1) x 8."""
    d = device(case[0])
    key, shape = _doc_case(case)
    for fill in FILLS:
        d.segment(key, shape, fill)


P_SELECT = _pairs(SCANS) + [(W, "picks", c) for W in WIDTHS for c in SEL_COUNTS]


def _sel_key(d, case):
    return cpu().sel_key(d.W, case[2]) if case[1] == "picks" else _key(case[1])


@pytest.mark.parametrize("case", P_SELECT, ids=_ids(P_SELECT))
def test_leftmost_longest(device, case):
    """pfac_records_leftmost_longest: d_out of exactly n_selected x 8 bytes."""
    d = device(case[0])
    for fill in FILLS:
        d.select(_sel_key(d, case), fill)


@pytest.mark.parametrize("case", P_DOCS, ids=_ids(P_DOCS))
def test_leftmost_longest_documents(device, case):
    """pfac_records_leftmost_longest_documents: d_out of exactly n_selected x 8 bytes, d_doc_first of (n_docs + 1) x 8."""
    d = device(case[0])
    key, shape = _doc_case(case)
    for fill in FILLS:
        d.select_docs(key, shape, fill)


P_REPLACE = P_SELECT + [(2, "ladder", name, front) for name in LADDER for front in (GUARD, GUARD + 16)]


@pytest.mark.parametrize("case", P_REPLACE, ids=_ids(P_REPLACE))
def test_replace(device, case):
    """pfac_replace_leftmost_longest: d_out of exactly out_bytes bytes (the back guard begins inside the last 16-byte
    block), d_sel the exact guarded d_out of the selection.  The ladder: every residue of out_bytes mod 16, outputs
    below 16 bytes, of no byte, at the 1 KiB window and the 4 KiB workgroup edge, blocks of picks that vanish, an entry
    with an exit; the payload at its tensor's natural start and 16 bytes further."""
    d = device(case[0])
    x = cpu()
    for fill in FILLS:
        if case[1] == "ladder":
            key, entry = x.ladder_key(d.W, case[2])
            d.replace(key, fill, entry, front=case[3])
        else:
            d.replace(_sel_key(d, case), fill)


@pytest.mark.parametrize("case", P_DOCS, ids=_ids(P_DOCS))
def test_replace_documents(device, case):
    """pfac_replace_documents: d_out of exactly out_bytes bytes, d_out_offsets of exactly (n_docs + 1) x 8; d_sel,
    d_doc_offsets and d_doc_first the exact guarded buffers of the selection."""
    d = device(case[0])
    key, shape = _doc_case(case)
    for fill in FILLS:
        d.replace_docs(key, shape, fill)
