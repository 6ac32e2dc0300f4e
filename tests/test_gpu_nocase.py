"""Case-insensitive scans on the GPU (run with -m gpu on an MI355X): the scan kernel folds A-Z of its input on the way
into LDS (pfac_table_set_case_fold), the caller's bytes stay as they are.  Every expectation is tests/nocaseref.py's --
the CPU oracle on the folded pattern file and the folded input -- and every input is one of its named cases, which
tests/test_nocase_ref.py holds against a second matcher without a GPU.  Integer work: the bar is bit-exact."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import countref
import docref
import gatherref
import llref
import nocaseref
import replref
import splitref
import wordref
from heapguard import GuardedBuffer
from phfpfac_amd import GpuMatcher, PfacError, PfacTable, emit_records
from phfpfac_amd._ffi import PFAC_E_ARG, PFAC_E_STATE

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FP = json.load(open(os.path.join(HERE, "golden", "fingerprints.json")))
TILE = 4096

# the environment list of test_gpu_parity.py::test_golden_under_every_kernel_variant
VARIANT_ENVS = [{"PFAC_FORCE_L2": "1"}, {"PFAC_FORCE_L2": "1", "PFAC_DENSE": "1"},
                {"PFAC_FORCE_L2": "1", "PFAC_NO_D1": "1", "PFAC_DENSE": "1"},
                {"PFAC_FORCE_L2": "1", "PFAC_NO_FUSE": "1"}, {"PFAC_NWB": "5", "PFAC_DENSE": "1"},
                {"PFAC_NWB": "3"}, {"PFAC_NO_D1": "1"},
                {"PFAC_WIDE": "1"},
                {"PFAC_REC_BYTES": "4"},
                {"PFAC_WIDE": "1", "PFAC_FORCE_L2": "1", "PFAC_DENSE": "1"},
                {"PFAC_LAG": "1"}, {"PFAC_LAG": "2"},
                {"PFAC_LAG": "2", "PFAC_REC_BYTES": "4"},
                {"PFAC_L2F": "0"}, {"PFAC_L2F": "2"},
                {"PFAC_L2F": "2", "PFAC_FORCE_L2": "1"}, {"PFAC_NO_SECF": "1", "PFAC_FORCE_L2": "1"},
                {"PFAC_NO_D1PACK": "1", "PFAC_FORCE_L2": "1"}]


def _env_id(env):
    return ",".join(f"{k[5:]}={v}" for k, v in env.items()) or "default"


def nocase_table(case, width=None):
    return PfacTable.from_bytes(case.patterns, width or case.width, ignore_case=True)


def folded_records(case, width=None):
    table = nocase_table(case, width)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        assert g.case_fold
        return table, g.scan_bytes(case.data, case.n_owned)


def text_of(pos, ids):
    return "".join("At position %4d, match pattern %d\n" % (p, i) for p, i in zip(pos.tolist(), ids.tolist())).encode()


def assert_records(table, rec, pos, ids, tmp_path=None):
    assert rec.size == pos.size, f"match count {rec.size} != reference {pos.size}"
    np.testing.assert_array_equal(rec["pos"].astype(np.int64), pos)
    np.testing.assert_array_equal(table.idmap[rec["state"]], ids)
    if tmp_path is not None:
        out = tmp_path / "GPU_match_result.txt"
        emit_records(str(out), rec, table.idmap)
        assert out.read_bytes() == text_of(pos, ids)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", nocaseref.parity_cases(), ids=repr)
def test_folded_scan_equals_the_reference(case, tmp_path):
    """Mixed-case text and the cycle of all 256 byte values, under the four-line set and the set with @ [ ` {, digits and
    bytes >= 0x80 next to letters, at three PHF widths: the records and their text."""
    table, rec = folded_records(case)
    assert_records(table, rec, *case.want, tmp_path=tmp_path)


@pytest.mark.parametrize("env", VARIANT_ENVS, ids=_env_id)
@pytest.mark.parametrize("case", nocaseref.variant_cases(), ids=repr)
def test_folded_scan_under_every_kernel_variant(case, env, monkeypatch):
    """The fold sits in front of everything that reads input bytes: tables in LDS, through L2, fused; two and four
    walks, dense staging; no dense rows, unpacked dense rows; every form of the level-2 filter; both lags; every record
    form."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    table, rec = folded_records(case)
    assert_records(table, rec, *case.want)


@pytest.mark.parametrize("width,env", [(256, {}), (64, {}), (256, {"PFAC_NO_DENSE2": "1"}), (4096, {"PFAC_NO_NW4": "1"}),
                                       (256, {"PFAC_D2_LOGCAP": "64"})])
def test_folded_dictionary_dense_mode_kernels(width, env, monkeypatch):
    """The 2 600-word dictionary on fused L2 tables in dense mode (dense2_tile, its fallback pass, the classic four-walk
    and the unfused two-walk kernels) over a few hundred KiB of mixed-case text."""
    monkeypatch.setenv("PFAC_DENSE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = nocaseref.dictionary_case()
    table, rec = folded_records(case, width)
    assert_records(table, rec, *case.want)


@pytest.mark.parametrize("env", [{}, {"PFAC_FORCE_L2": "1"}, {"PFAC_L2F": "0"}, {"PFAC_L2F": "2"}], ids=_env_id)
@pytest.mark.parametrize("case", nocaseref.root1_cases(), ids=repr)
def test_one_edge_root_sees_folded_bytes(case, env, monkeypatch):
    """ROOT == 1 compares every input byte with the one root byte, and l2f_mode 1 the next byte with one or two child
    bytes: the input has all of them in upper case only."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    table, rec = folded_records(case)
    assert_records(table, rec, *case.want)


@pytest.mark.parametrize("case", nocaseref.placement_cases(), ids=repr)
def test_fold_reaches_halo_owned_end_ragged_tail_and_every_length(case, tmp_path):
    """A match whose tail comes from the halo registers; one that starts in the last 15 owned bytes and ends past
    n_owned; input lengths 1, 7 and 15 (mod 16) with an upper-case match ending in the last, byte-patched, byte;
    max_pat_len 1, 2, 17 and 1022."""
    table, rec = folded_records(case)
    assert_records(table, rec, *case.want, tmp_path=tmp_path)


# ---------------------------------------------------------------------------
def slot_input_back(g, n, slot=0):
    """The first n bytes of the slot's input buffer, through the gather of the one document [0, n)."""
    import torch
    g.set_doc_offsets(np.array([0, n], dtype=np.uint64), slot)
    ids = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert g.gather_documents(1, 1, n, d_ids=ids, slot=slot) == n
    return g.gathered_to_host(n, slot)


def test_the_input_is_never_written():
    import torch
    case = nocaseref.placement_cases()[4]                  # a ragged tail: the byte-wise patch runs too
    assert case.name.startswith("ragged-tail")
    table = nocase_table(case)
    n = case.data.size
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        rec = g.scan_bytes(case.data)
        assert_records(table, rec, *case.want)
        np.testing.assert_array_equal(slot_input_back(g, n), case.data)
        # a caller's buffer of exactly n bytes between guard bands
        for fill in (0xA5, 0x3C):
            gb = GuardedBuffer(n, fill=fill)
            gb.payload().copy_(torch.from_numpy(case.data.copy()))
            torch.cuda.synchronize()
            g.scan_async(n, n, d_input=gb.ptr)
            cnt, over = g.scan_finish()
            assert not over
            assert_records(table, g.records_to_host(cnt), *case.want)
            gb.check()
            np.testing.assert_array_equal(gb.host(), case.data)


# ---------------------------------------------------------------------------
def test_the_settings_life():
    case = nocaseref.variant_cases()[1]
    data = case.data
    n = data.size
    table = nocase_table(case)
    plain = PfacTable.from_bytes(nocaseref.fold_bytes(case.patterns), 256)          # the same table without the flag
    fpos, fids = case.want
    epos, eids = nocaseref.exact(nocaseref.fold_bytes(case.patterns), data)        # lower-case occurrences only
    assert 0 < epos.size < fpos.size
    with GpuMatcher(0, 2) as g:
        with pytest.raises(PfacError) as e:
            g.set_case_fold(True)                                                   # no table yet
        assert e.value.status == PFAC_E_STATE
        g.load_table(plain)
        assert not g.case_fold                                                      # off after a table without the flag
        assert_records(plain, g.scan_bytes(data), epos, eids)
        # on, off, on between scans, on both slots
        for k, on in enumerate((True, False, True, True, False)):
            g.set_case_fold(on)
            assert g.case_fold == on
            assert_records(plain, g.scan_bytes(data, slot=k & 1), *((fpos, fids) if on else (epos, eids)))
        # a scan queued before the toggle keeps its mode
        big = nocaseref.tiled(130 * TILE, data.tobytes())
        bf, be = nocaseref.expected(case.patterns, big), nocaseref.exact(nocaseref.fold_bytes(case.patterns), big)
        for slot in (0, 1):
            g.reserve(slot, big.size, big.size // 2)
            g.h2d(big, slot)
        g.set_case_fold(True)
        g.scan_async(big.size, slot=0)
        g.set_case_fold(False)
        g.scan_async(big.size, slot=1)
        g.set_case_fold(True)
        n0, _ = g.scan_finish(0)
        n1, _ = g.scan_finish(1)
        assert_records(plain, g.records_to_host(n0, 0), *bf)
        assert_records(plain, g.records_to_host(n1, 1), *be)
        # other modes: PFAC_E_ARG, and nothing changes
        for mode in (2, 0xFFFFFFFF):
            assert g._L.pfac_table_set_case_fold(g._ctx, mode) == PFAC_E_ARG
            assert g.case_fold
        # a new upload resets it -- unless the table says otherwise
        g.load_table(plain.blob())
        assert not g.case_fold
        assert_records(plain, g.scan_bytes(data), epos, eids)
        g.load_table(table)
        assert g.case_fold
        assert_records(table, g.scan_bytes(data), fpos, fids)
        import torch
        blob = torch.from_numpy(table.blob()).to("cuda:0")
        torch.cuda.synchronize()
        g.load_table_device(blob, blob.numel())
        assert not g.case_fold
        g.load_table_device(blob, blob.numel(), host_table=table)
        assert g.case_fold


# ---------------------------------------------------------------------------
# behind the scan: every pass against its own CPU reference, fed the reference's records and the ORIGINAL bytes

@pytest.fixture(scope="module")
def passes():
    case = nocaseref.passes_case()
    table = nocase_table(case)
    lines = case.patterns[:-1].split(b"\n")
    line_len = np.array([0] + [len(l) for l in lines], dtype=np.int64)
    pos, ids = case.want
    g = GpuMatcher(0, 1)
    g.load_table(table)
    yield g, table, case, pos, ids, line_len[ids], len(lines)
    g.close()


def test_count_patterns_behind_a_folded_scan(passes):
    g, table, case, pos, ids, lens, n_lines = passes
    got = g.count_patterns(case.data)
    np.testing.assert_array_equal(got[: n_lines + 1], countref.pattern_counts(ids, n_lines))
    assert int(got.sum()) == pos.size


def test_leftmost_longest_behind_a_folded_scan(passes):
    g, table, case, pos, ids, lens, _ = passes
    rec, ex = g.scan_leftmost_longest(case.data)
    sel, want_ex = llref.greedy(pos, lens, 0, case.data.size)
    assert sel.size > 100 and ex == want_ex
    assert_records(table, rec, pos[sel], ids[sel])
    assert llref.check_greedy(pos, lens, (rec["pos"], lens[sel]), 0, case.data.size) == ex


def test_redaction_keeps_the_original_case_outside_the_picks(passes):
    g, table, case, pos, ids, lens, n_lines = passes
    g.set_redaction(b"*")
    out, ex = g.replace(case.data)
    reps = {i: b"*" * len(l) for i, l in enumerate(case.patterns[:-1].split(b"\n"), start=1)}
    want, want_ex = replref.greedy_replace(case.data, 0, case.data.size, pos, lens, ids, replref.rep_table(reps))
    assert ex == want_ex
    np.testing.assert_array_equal(out, want)
    outside = out != ord("*")
    assert out.size == case.data.size and 0 < outside.sum() < out.size
    np.testing.assert_array_equal(out[outside], case.data[outside])
    assert ((out >= 0x41) & (out <= 0x5A)).sum() > 1000            # upper case came through


def test_scan_documents_behind_a_folded_scan(passes):
    g, table, case, pos, ids, lens, _ = passes
    off = docref.random_offsets(np.random.default_rng(3), case.data.size, 90, empties=4)
    first, rec = g.scan_documents((case.data, off))
    with nocaseref.FoldedOracle(case.patterns) as o:
        wfirst, wpos, wids = docref.oracle_per_doc(o, nocaseref.fold(case.data), off)
    np.testing.assert_array_equal(first, wfirst)
    assert_records(table, rec, wpos, wids)


def test_grep_lines_returns_the_original_lines(passes):
    g, table, case, pos, ids, lens, _ = passes
    out, out_off, line_ids = g.grep_lines(case.data, before=1, after=1)
    off, n_docs, _ = splitref.split_offsets(case.data, 0x0A)
    with nocaseref.FoldedOracle(case.patterns) as o:
        first, _, _ = docref.oracle_per_doc(o, nocaseref.fold(case.data), off)
    want_ids = gatherref.context_ids(first, 1, 1)
    want, want_off = gatherref.gather_ref(case.data, off, want_ids)
    assert 0 < want_ids.size
    np.testing.assert_array_equal(line_ids, want_ids)
    np.testing.assert_array_equal(out_off, want_off)
    np.testing.assert_array_equal(out, want)
    assert ((out >= 0x41) & (out <= 0x5A)).sum() > 1000
    # grep -i without context: fewer lines with the fold off
    ids_on = g.grep_lines(case.data)[2]
    g.set_case_fold(False)
    ids_off = g.grep_lines(case.data)[2]
    g.set_case_fold(True)
    assert ids_off.size < ids_on.size and np.isin(ids_off, ids_on).all()


def test_whole_words_are_judged_on_the_original_bytes(passes):
    g, table, case, pos, ids, lens, _ = passes
    rec = g.scan_bytes(case.data, whole_words=True)
    keep = wordref.filter_words(case.data, pos, lens)
    assert 0 < keep.sum() < keep.size
    assert_records(table, rec, pos[keep], ids[keep])
    # a word set that separates the cases sees the case the input was written in: only lower-case letters are word bytes
    lower = bytes(range(0x61, 0x7B))
    rec = g.scan_bytes(case.data, whole_words=lower)
    from phfpfac_amd import word_set
    keep_l = wordref.filter_words(case.data, pos, lens, word_set=word_set(lower))
    assert keep_l.sum() != wordref.filter_words(nocaseref.fold(case.data), pos, lens, word_set=word_set(lower)).sum()
    assert_records(table, rec, pos[keep_l], ids[keep_l])


# ---------------------------------------------------------------------------
def test_gphf_ignore_case(tmp_path):
    """The CLI: PFAC_IGNORE_CASE=1 with two workers and 1 MiB chunks gives the oracle's text for the folded case; without
    it the golden file comes out as ever."""
    exe = os.path.join(os.path.dirname(HERE), "phfpfac_amd", "bin", "gphf")
    data_dir = os.path.join(HERE, "golden", "data")
    pats = open(os.path.join(data_dir, "xaa"), "rb").read().title()
    pf = tmp_path / "Title.pat"
    pf.write_bytes(pats)
    n = 3 * (1 << 20) + 12345
    text = nocaseref.mixed_text(n + 1, seed=9)                   # + the byte the CLI drops
    big = tmp_path / "mixed.txt"
    big.write_bytes(text.tobytes())
    env = dict(os.environ, PFAC_CHUNK_MB="1", PFAC_WORKERS_PER_GPU="2", PFAC_IGNORE_CASE="1")
    out = subprocess.run([exe, str(pf), "2", "256", str(big)], cwd=tmp_path, env=env, capture_output=True, text=True,
                         check=True).stdout
    assert "(2 worker(s);" in out
    exp = tmp_path / "expected.txt"
    with nocaseref.FoldedOracle(pats) as o:
        cnt, _ = o.emit(nocaseref.fold(text[:n]), str(exp), spec=True)
    got = (tmp_path / "GPU_match_result.txt").read_bytes()
    assert cnt > 100_000 and got == exp.read_bytes()
    # without the switch: title-case patterns find next to nothing in this text, and the golden case is what it was
    env.pop("PFAC_IGNORE_CASE")
    subprocess.check_call([exe, str(pf), "2", "256", str(big)], cwd=tmp_path, env=env, stdout=subprocess.DEVNULL)
    assert len((tmp_path / "GPU_match_result.txt").read_bytes()) < len(got) // 2
    one_m = tmp_path / "1M"
    para = nocaseref.paragraph()
    one_m.write_bytes((para * (1048576 // 402 + 1))[:1048576])
    subprocess.check_call([exe, os.path.join(data_dir, "experimentpattern"), "2", "256", str(one_m)], cwd=tmp_path, env=env,
                          stdout=subprocess.DEVNULL)
    assert hashlib.md5((tmp_path / "GPU_match_result.txt").read_bytes()).hexdigest() == FP["cases"]["exp_x_1M_s1_w256"]["md5"]
