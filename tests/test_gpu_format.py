"""The gather with labels on the GPU (run with -m gpu on an MI355X): pfac_documents_gather_format against tests/fmtref.py
(the rule of include/pfac.h in numpy, pinned to a b"%d"-and-join form and to the system grep by
tests/test_format_ref.py), into guard bands of exactly out_bytes and (n_ids + 1) x 8 bytes driven through
passguard.exact_call, its errors (each one answered by the host or by the first pass -- none provokes a fault), the
result it shares with pfac_documents_gather, chunked numbering, and GpuMatcher.grep_text against a grep in Python.
Integer work: bit-exact.  No expectation comes from the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import fmtref
from fmtref import (BIG_PERIODS, LOG_PATTERNS, NL, Fmt, FormatCase, all_format_cases, assert_format, big_case, chain_cuts,
                    format_ref, grep_fmt, make_log, python_grep)
from gatherref import assert_gather, count_cases as plain_count_cases
from heapguard import FILLS, GuardedBuffer
from passguard import Want, exact_call
from phfpfac_amd import GpuMatcher, PfacError, PfacTable
from phfpfac_amd import _ffi

pytestmark = pytest.mark.gpu

CASES = all_format_cases()
SHIFT = 48                                  # a caller's input starts here in its allocation: 16-B aligned, not 256
PADS = (NL, 0xA5)                           # what the bytes from n_bytes to the next tile hold: the terminator, then another byte


@pytest.fixture(scope="module")
def g():
    with GpuMatcher(0, 1) as m:
        yield m


def status_of(fn):
    with pytest.raises(PfacError) as e:
        fn()
    return e.value.status


def device_bytes(host, shift=0):
    """A device tensor holding `host` from byte `shift` on; -> (tensor, pointer of the first byte of `host`)."""
    t = torch.zeros(shift + host.size + 16, dtype=torch.uint8, device="cuda:0")
    t[shift:shift + host.size] = torch.from_numpy(host)
    torch.cuda.synchronize()                # (the slot's stream is not torch's)
    return t, int(t.data_ptr()) + shift


def device_u64(a):
    """A device copy of uint64 values (one spare entry, so that an empty array still has an address)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    t = torch.from_numpy(np.append(a, np.uint64(0)).view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def place_input(g, case, pad, source):
    """The case's bytes in the slot's input buffer or in a caller's buffer; -> (keep-alive, d_input)."""
    storage = case.storage(pad)
    if source == "slot":
        g.reserve(0, storage.size)
        g.h2d(storage)
        return None, None
    keep, ptr = device_bytes(storage, SHIFT)
    assert ptr % 16 == 0 and ptr % 256 != 0
    return keep, ptr


def call_status(fn):
    """(status, out_bytes) of a formatted gather, as passguard.exact_call wants it."""
    try:
        return 0, fn()
    except PfacError as e:
        return e.status, getattr(e, "out_bytes", None)


def run_exact(g, case, d_in, d_ids, fill, what, refusals=(), d_first=None):
    """One case through passguard.exact_call: one byte short (PFAC_E_OVERFLOW, the exact count, nothing written), the
    rule-breaking variants `refusals` (keyword overrides; PFAC_E_ARG, nothing written), the exact capacity (every byte
    and offset the reference's, guards intact).  -> the output bytes."""
    want, want_off = case.want()
    buf = {"d_out": GuardedBuffer(want.size, fill=fill), "d_out_offsets": GuardedBuffer((case.n_ids + 1) * 8, fill=fill)}
    if d_first is None and case.doc_first is not None:
        d_first = device_u64(case.doc_first)

    def call(cap, bad=None):
        kw = dict(d_input=d_in, d_ids=d_ids, d_doc_first=d_first, d_out=buf["d_out"].ptr, out_cap=cap,
                  d_out_offsets=buf["d_out_offsets"].ptr, **case.fmt.kwargs())
        if bad is not None:
            kw.update(refusals[bad])
        return call_status(lambda: g.gather_documents_formatted(case.n_docs, case.n_ids, case.n, **kw))
    exact_call(g, call, Want(want.size, {"d_out": want, "d_out_offsets": want_off}, bad=len(refusals)), buf, fill,
               f"pfac_documents_gather_format {case.name} {what}")
    whole = buf["d_out"].tensor[buf["d_out"].front:].cpu().numpy()      # the payload and the back guard behind it
    assert_format(case, want.size, buf["d_out_offsets"].host().view(np.uint64), whole, fill=fill, what=what)
    return whole[:want.size].copy()


# ---------------------------------------------------------------------------
# every named case

@pytest.mark.parametrize("case", CASES, ids=repr)
def test_format_equals_reference(g, case):
    """Every named case into buffers of exactly out_bytes and (n_ids + 1) x 8 bytes, once from the slot's input with the
    terminator byte behind n_bytes and once from a caller's buffer (16-B aligned, not 256) with another byte there:
    identical output; then the slot-owned form."""
    g.set_doc_offsets(case.offsets)
    d_ids = device_u64(case.ids)
    seen = []
    for pad, source, fill in zip(PADS, ("slot", "caller"), FILLS):
        keep, d_in = place_input(g, case, pad, source)
        seen.append(run_exact(g, case, d_in, d_ids, fill, f"({source}, padding 0x{pad:02x})"))
        assert status_of(lambda: g.gathered_to_host(0)) == _ffi.PFAC_E_STATE          # both went to the caller's buffers
    first = device_u64(case.doc_first) if case.doc_first is not None else None
    n = g.gather_documents_formatted(case.n_docs, case.n_ids, case.n, d_input=d_in, d_ids=d_ids, d_doc_first=first,
                                     **case.fmt.kwargs())
    assert_format(case, n, g.gathered_offsets_to_host(case.n_ids), g.gathered_to_host(n), what="slot-owned")
    del keep
    assert np.array_equal(seen[0], seen[1]), "the bytes behind n_bytes changed the output"


def named(name):
    return next(c for c in CASES if c.name == name)


def test_refused_calls_write_nothing(g):
    """An id >= n_docs and descending offsets of a selected document: PFAC_E_ARG from the first pass, every buffer
    untouched (with the overflow and the exact capacity around them, through exact_call, under both fills)."""
    case = named("ids1025_all")
    past = case.ids.copy()
    past[1024] = case.n_docs
    k = int(case.ids[700])
    desc = case.offsets.copy()
    assert desc[k] > 0
    desc[k + 1] = desc[k] - np.uint64(1)
    d_past, d_desc = device_u64(past), device_u64(desc)
    g.set_doc_offsets(case.offsets)
    keep, d_in = place_input(g, case, 0, "caller")
    for fill in FILLS:
        run_exact(g, case, d_in, device_u64(case.ids), fill, "refusals", refusals=[dict(d_ids=d_past), dict(d_doc_offsets=d_desc)])
    del keep


def test_exact_capacity_through_every_output_residue(g):
    """n_ids chosen so that out_bytes takes every residue mod 16: the guards right behind the last partial 16 bytes."""
    base = named("terminate_all_labels")
    by_res = {}
    for n in range(1, base.n_ids + 1):
        c = FormatCase(f"residue_n{n}", base.data, base.offsets, base.ids[:n], base.fmt)
        by_res.setdefault(int(c.want()[0].size) % 16, c)
    assert sorted(by_res) == list(range(16))
    g.set_doc_offsets(base.offsets)
    place_input(g, base, 0, "slot")
    for r, c in sorted(by_res.items()):
        run_exact(g, c, None, device_u64(c.ids), FILLS[r & 1], f"out_bytes = {r} mod 16")


# ---------------------------------------------------------------------------
# the plain gather's result

def raw_format(g, case, fmt_ptr, d_ids, d_out=None, out_cap=0, d_off=None, d_first=None):
    n = C.c_uint64(0)
    rc = g._L.pfac_documents_gather_format(g._ctx, 0, None, case.n, None, case.n_docs, int(d_ids.data_ptr()), case.n_ids, d_first,
                                           fmt_ptr, d_out, out_cap, d_off, C.byref(n))
    return rc, n.value


@pytest.mark.parametrize("case", [c for c in plain_count_cases() if c.n_ids in (0, 65, 1025)], ids=repr)
def test_null_and_zero_format_are_the_plain_gather(g, case):
    g.set_doc_offsets(case.offsets)
    place_input(g, case, 0, "slot")
    d_ids = device_u64(case.ids)
    zero = _ffi.CLineFormat()
    zero.sep_match, zero.sep_context, zero.terminator, zero.number_base = 58, 45, 10, 1      # (no flag reads them)
    for what, fmt in (("fmt NULL", None), ("the all-zero format", C.byref(zero))):
        rc, n = raw_format(g, case, fmt, d_ids)
        assert rc == 0, what
        assert_gather(case, n, g.gathered_offsets_to_host(case.n_ids), g.gathered_to_host(n), what=what)


def test_shared_result(g):
    """One slot-owned result for both gathers: the formatted one is fetched through pfac_documents_gather_d2h (windows
    too), a failing plain gather discards it, and two identical calls give identical bytes."""
    case = named("ids1025_all")
    want, want_off = case.want()
    g.set_doc_offsets(case.offsets)
    place_input(g, case, 0, "slot")
    d_ids, d_first = device_u64(case.ids), device_u64(case.doc_first)
    kw = dict(d_ids=d_ids, d_doc_first=d_first, **case.fmt.kwargs())
    n = g.gather_documents_formatted(case.n_docs, case.n_ids, case.n, **kw)
    one = g.gathered_to_host(n)
    assert_format(case, n, g.gathered_offsets_to_host(case.n_ids), one)
    assert np.array_equal(g.gathered_to_host(17, first=n - 17), want[n - 17:])
    assert g.gather_documents_formatted(case.n_docs, case.n_ids, case.n, **kw) == n
    assert np.array_equal(g.gathered_to_host(n), one)
    assert status_of(lambda: g.gather_documents(case.n_docs + 1, case.n_ids, case.n, d_ids=d_ids)) == _ffi.PFAC_E_STATE
    assert status_of(lambda: g.gathered_to_host(0)) == _ffi.PFAC_E_STATE
    assert status_of(lambda: g.gathered_offsets_to_host(case.n_ids)) == _ffi.PFAC_E_STATE
    plain = g.gather_documents(case.n_docs, case.n_ids, case.n, d_ids=d_ids)         # ... and the other way round
    assert plain < n
    assert status_of(lambda: g.gather_documents_formatted(case.n_docs + 1, case.n_ids, case.n, **kw)) == _ffi.PFAC_E_STATE
    assert status_of(lambda: g.gathered_to_host(0)) == _ffi.PFAC_E_STATE


def test_argument_errors(g):
    """group_sep_len = 9, an unknown flag, bases past the bound: PFAC_E_ARG, the slot-owned result discarded, the
    caller's buffers untouched.  The bases AT the bound pass."""
    case = named("ids65_number")
    want, _ = case.want()
    g.set_doc_offsets(case.offsets)
    place_input(g, case, 0, "slot")
    d_ids = device_u64(case.ids)
    gb, go = GuardedBuffer(want.size), GuardedBuffer((case.n_ids + 1) * 8, fill=0x3C)

    def fmt(**kw):
        f = _ffi.CLineFormat()
        f.flags, f.sep_match, f.sep_context, f.terminator, f.number_base = _ffi.PFAC_LINE_NUMBER, 58, 45, 10, 1
        for k, v in kw.items():
            setattr(f, k, v)
        return f
    limit = fmtref.LIMIT
    errors = [("group_sep_len = 9", fmt(group_sep_len=9)), ("an unknown flag", fmt(flags=32)), ("every bit set", fmt(flags=0xFFFFFFFF)),
              ("number_base + n_docs past 10^18", fmt(number_base=limit - case.n_docs + 1)),
              ("number_base that wraps", fmt(number_base=2 ** 64 - 1)),
              ("offset_base + n_bytes past 10^18", fmt(flags=_ffi.PFAC_LINE_OFFSET, offset_base=limit - case.n + 1)),
              ("offset_base that wraps", fmt(offset_base=2 ** 64 - 2))]
    for name, f in errors:
        n = g.gather_documents_formatted(case.n_docs, case.n_ids, case.n, d_ids=d_ids, number=True)      # a result to lose
        assert n == want.size
        rc, _ = raw_format(g, case, C.byref(f), d_ids, gb.ptr, want.size, go.ptr)
        assert rc == _ffi.PFAC_E_ARG, name
        g.sync()
        gb.check(payload_untouched=True, what=f"d_out after {name}")
        go.check(payload_untouched=True, what=f"d_out_offsets after {name}")
        assert status_of(lambda: g.gathered_to_host(0)) == _ffi.PFAC_E_STATE, name
    at = FormatCase("bases_at_the_bound", case.data, case.offsets, case.ids,
                    Fmt(number=True, byte_offset=True, number_base=limit - case.n_docs, offset_base=limit - case.n))
    n = g.gather_documents_formatted(case.n_docs, case.n_ids, case.n, d_ids=d_ids, **at.fmt.kwargs())
    assert_format(at, n, g.gathered_offsets_to_host(case.n_ids), g.gathered_to_host(n))
    with pytest.raises(ValueError):
        g.gather_documents_formatted(case.n_docs, case.n_ids, case.n, d_ids=d_ids, group_sep=b"123456789")


# ---------------------------------------------------------------------------
# the large output

def test_large_output_past_64_mib(g):
    """write_grid's wins = 4 regime: the ids of one period, BIG_PERIODS times, over a small input.  Every period prints
    the same odd number of bytes (the 16-byte phase rotates), checked against format_ref on the period."""
    case = big_case()
    piece, piece_off = case.want()
    k = BIG_PERIODS
    assert piece.size * k > 64 << 20
    g.set_doc_offsets(case.offsets)
    place_input(g, case, 0, "slot")
    d_ids = device_u64(np.tile(case.ids, k))
    d_first = device_u64(case.doc_first)
    n = g.gather_documents_formatted(case.n_docs, case.n_ids * k, case.n, d_ids=d_ids, d_doc_first=d_first, **case.fmt.kwargs())
    assert n == piece.size * k
    got = torch.from_numpy(g.gathered_to_host(n))
    assert torch.equal(got, torch.from_numpy(piece.copy()).repeat(k))
    off = g.gathered_offsets_to_host(case.n_ids * k)
    want_off = (np.arange(k, dtype=np.uint64)[:, None] * np.uint64(piece.size) + piece_off[None, :-1]).ravel()
    assert np.array_equal(off[:-1], want_off) and int(off[-1]) == n


# ---------------------------------------------------------------------------
# chunks

def test_chaining_equals_one_shot(g):
    """A buffer cut at three document boundaries (what a reader that carries the split's tail_start over does): every
    chunk formatted with number_base, offset_base and SEP_FIRST set from what the chunks before it printed; the
    concatenation is the one-shot output."""
    base = named("terminate_all_labels")
    rng = np.random.default_rng(31)
    sel = np.flatnonzero(rng.random(base.n_docs) < 0.6).astype(np.uint64)
    fmt = Fmt(number=True, byte_offset=True, terminate=NL, context_sep=True, group_sep=b"--\n")
    first = fmtref.seeded_first(base.n_docs, 32)
    whole, _ = format_ref(base.data, base.offsets, sel, fmt, first)
    cuts = [0] + chain_cuts(base.offsets) + [base.n]
    off = base.offsets.astype(np.int64)
    parts, last_printed = [], None
    for a, b in zip(cuts[:-1], cuts[1:]):
        d0, d1 = int(np.searchsorted(off, a)), int(np.searchsorted(off, b))       # the chunk's documents [d0, d1)
        assert off[d0] == a and off[d1] == b
        ids = sel[(sel >= d0) & (sel < d1)] - np.uint64(d0)
        chunk = FormatCase(f"chunk_{a}", base.data[a:b], off[d0:d1 + 1] - a, ids, Fmt(
            **{**fmt.kwargs(), "number_base": 1 + d0, "offset_base": a,
               "sep_first": bool(ids.size) and last_printed is not None and int(ids[0]) + d0 != last_printed + 1}), first[d0:d1 + 1])
        g.set_doc_offsets(chunk.offsets)
        place_input(g, chunk, 0, "slot")
        n = g.gather_documents_formatted(chunk.n_docs, chunk.n_ids, chunk.n, d_ids=device_u64(ids),
                                         d_doc_first=device_u64(chunk.doc_first), **chunk.fmt.kwargs())
        got = g.gathered_to_host(n)
        assert_format(chunk, n, g.gathered_offsets_to_host(chunk.n_ids), got)
        parts.append(got)
        if ids.size:
            last_printed = int(ids[-1]) + d0
    assert len(parts) == 4 and all(p.size for p in parts)
    assert bytes(np.concatenate(parts)) == bytes(whole)


# ---------------------------------------------------------------------------
# the context separator over a real segment pass, and grep_text

@pytest.fixture(scope="module")
def log():
    data = make_log()
    pats = b"".join(p + b"\n" for p in LOG_PATTERNS)
    return {"data": data, "buf": np.frombuffer(data, dtype=np.uint8), "table": PfacTable.from_bytes(pats, 256),
            "folded": PfacTable.from_bytes(pats, 256, ignore_case=True)}


def scanned_lines(m, log):
    m.load_table(log["table"])
    _, n_docs = m._scan_lines(log["buf"], b"\n", 0, fetch_offsets=False)
    return n_docs


@pytest.mark.parametrize("window", [(0, 0), (1, 0), (0, 1), (2, 3)], ids=lambda w: f"B{w[0]}_A{w[1]}")
def test_context_separator_over_a_segment_pass(log, window):
    """Scan, split, cut, context ids and the formatted gather with every default NULL: the label separator comes from
    the slot's doc_first.  The expectation is a grep in Python."""
    before, after = window
    off, ids, first, n_lines = python_grep(log["data"], LOG_PATTERNS, before, after)
    fmt = Fmt(number=True, byte_offset=True, terminate=NL, context_sep=True, group_sep=b"--\n")
    case = FormatCase(f"log_B{before}_A{after}", log["buf"], off, ids, fmt, first)
    want, _ = case.want()
    assert (b"-" in bytes(want).replace(b"--\n", b"")) == bool(before or after)
    with GpuMatcher(0, 1) as m:
        n_docs = scanned_lines(m, log)
        assert n_docs == n_lines
        assert status_of(lambda: m.gather_documents_formatted(n_docs, 0, case.n, d_ids=device_u64(ids), **fmt.kwargs())) == _ffi.PFAC_E_STATE
        m.segment_records(n_docs)
        k = m.matching_documents(n_docs, before=before, after=after)
        assert k == ids.size
        n = m.gather_documents_formatted(n_docs, k, case.n, **fmt.kwargs())
        assert_format(case, n, m.gathered_offsets_to_host(k), m.gathered_to_host(n))
        # a doc_first of another n_docs is not the slot's; a caller's is taken as it is
        m.set_doc_offsets(off[:-1])
        assert status_of(lambda: m.gather_documents_formatted(n_docs - 1, 0, int(off[-2]), d_ids=device_u64(ids), **fmt.kwargs())) == _ffi.PFAC_E_ARG
        m.set_doc_offsets(off)
        n = m.gather_documents_formatted(n_docs, k, case.n, d_ids=device_u64(ids), d_doc_first=device_u64(first), **fmt.kwargs())
        assert_format(case, n, m.gathered_offsets_to_host(k), m.gathered_to_host(n), what="a caller's doc_first")


GREP_TEXT = [dict(), dict(number=True), dict(byte_offset=True), dict(number=True, byte_offset=True),
             dict(number=True, before=1, after=1), dict(byte_offset=True, before=2, after=2), dict(number=True, before=2),
             dict(number=True, invert=True), dict(number=True, ignore_case=True, after=1), dict(number=True, whole_words=True),
             dict(number=True, byte_offset=True, line_match=True), dict(number=True, number_base=1000, offset_base=10 ** 9 - 5, sep_first=True, after=1)]


@pytest.mark.parametrize("kw", GREP_TEXT, ids=lambda kw: "_".join(f"{k}{'' if v is True else v}" for k, v in kw.items()) or "plain")
def test_grep_text(log, kw):
    kw = dict(kw)
    fold = kw.pop("ignore_case", False)
    sel = {k: kw[k] for k in ("invert", "whole_words", "line_match") if k in kw}
    before, after = kw.get("before", 0), kw.get("after", 0)
    off, ids, first, n_lines = python_grep(log["data"], LOG_PATTERNS, before, after, ignore_case=fold, **sel)
    assert 0 < ids.size < n_lines
    labels = {k: kw[k] for k in ("number", "byte_offset", "number_base", "offset_base", "sep_first") if k in kw}
    case = FormatCase("grep_text", log["buf"], off, ids, grep_fmt(labels, before, after), first)
    with GpuMatcher(0, 1) as m:
        m.load_table(log["folded" if fold else "table"])
        if fold:
            m.set_case_fold(True)
        text, out_off, got_ids = m.grep_text(log["data"], **kw)
    assert got_ids.tolist() == ids.tolist()
    assert_format(case, text.size, out_off, text)
    if fold:
        assert b"ERROR" in bytes(text)                              # the lines come back as written
