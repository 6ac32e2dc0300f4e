"""Automata at the bit-width limits of the scan's packed words (tests/bigsets.py), scanned on the GPU and compared
record for record with the trie-free matcher of tests/bigref.py.

Every scan runs twice (the staging layout adapts after the first), on three inputs per set: text made of the set's own
words, random symbols with patterns planted, and the greatest pattern (final state F - 1) at tile offsets 0 and 4095,
on the last owned byte, across the owned end and in the halo.  Each checks positions and idmap[state], the device
checksum and the record width.

Knob sets per pattern set (width 256 unless named):
- every set: default; PFAC_DENSE=1, where F65535, S2^20 and N2048 must run dense mode's second form and their +1 twins
  must not;
- F65535, F65536, S2^20, S2^20+1, N2048, N2049: also PFAC_DENSE=1 + PFAC_NO_D1 and width 64 (unfused);
- F2^20, F2^20+1 and DICT: also width 64, PFAC_NO_FUSE, PFAC_L2F=0, PFAC_L2F=2, PFAC_NO_SECF and PFAC_TICKET_WAYS=1;
  F2^20 and F2^20+1 also PFAC_NO_D1.
The consumers run on F2^20+1 (8-byte records, 7-digit ids) and DICT (1.4 M states and more): the GPU text emitter,
the host emitters, documents / selection / replace / chained selection (tests/passfuzz.py's checks), pattern-partition
mode in 2 and 3 parts, and the gphf CLI (F2^20+1 only) with either emitter and two workers."""
import os
import subprocess

import numpy as np
import pytest

from bigref import BigRef, format_lines
from bigsets import BUILDERS, BigCase, adversarial, planted_random, word_text
from orc import match_checksum
from passfuzz import record_width, run_case
from phfpfac_amd import GpuMatcher, PfacTable, emit_packed, emit_records

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SECOND_FORM = {"F65535": True, "F65536": False, "S2^20": True, "S2^20+1": False, "N2048": True, "N2049": False}
GATES = list(SECOND_FORM)
WIDE = ["F2^20", "F2^20+1", "DICT"]
PLAN = ([(s, 256, {}) for s in BUILDERS] + [(s, 256, {"PFAC_DENSE": "1"}) for s in BUILDERS]
        + [(s, 256, {"PFAC_DENSE": "1", "PFAC_NO_D1": "1"}) for s in GATES] + [(s, 64, {}) for s in GATES + WIDE]
        + [(s, 256, k) for s in WIDE for k in ({"PFAC_NO_FUSE": "1"}, {"PFAC_L2F": "0"}, {"PFAC_L2F": "2"},
                                               {"PFAC_NO_SECF": "1"}, {"PFAC_TICKET_WAYS": "1"})]
        + [(s, 256, {"PFAC_NO_D1": "1"}) for s in ("F2^20", "F2^20+1")])
_CACHE = {}


def label(p):
    s, w, k = p
    return f"{s}-w{w}-" + ("+".join(f"{a[5:]}={b}" for a, b in sorted(k.items())) or "default")


class Big:
    """One set with its file, tables by width, matcher and inputs with their expectations, built once."""

    def __init__(self, name, d):
        self.name = name
        self.s = BUILDERS[name]()
        self.path = self.s.write(os.path.join(d, "p.pat"))
        self.tables = {}
        self.ref = BigRef(self.path)
        big = name in ("DICT",)
        self.inputs = {"text": (word_text(self.s, (6 << 20) + 11 if big else (2 << 20) + 5), None),
                       "planted": (planted_random(self.s, (2 << 20) - 3), None),
                       "edges": adversarial(self.s, (1 << 20) + 4096 * 3 + 77)}
        self.want = {}

    def table(self, width):
        if width not in self.tables:
            t = PfacTable.from_file(self.path, width)
            self.s.check(t)
            self.tables[width] = t
        return self.tables[width]

    def expect(self, kind):
        if kind not in self.want:
            data, n_owned = self.inputs[kind]
            self.want[kind] = self.ref.scan_spec(data, None, n_owned)
        return self.want[kind]


def big(name, tmp_path_factory):
    if name not in _CACHE:
        _CACHE[name] = Big(name, str(tmp_path_factory.mktemp(name.replace("^", "p").replace("+", "x"))))
    return _CACHE[name]


def knobs_env(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def check_scans(g, table, data, n_owned, want, knobs, where):
    wpos, wids = want
    for rep in range(2):
        rec = g.scan_bytes(data, n_owned)
        assert rec.size == wpos.size, f"{where} scan {rep}: {rec.size} records, want {wpos.size}"
        np.testing.assert_array_equal(rec["pos"].astype(np.int64), wpos, err_msg=f"{where} scan {rep}: positions")
        assert int(rec["state"].max(initial=0)) < table.num_final, f"{where} scan {rep}: a state past the final states"
        np.testing.assert_array_equal(table.idmap[rec["state"]], wids, err_msg=f"{where} scan {rep}: pattern ids")
        assert g.checksum(rec.size) == match_checksum(wpos, wids), f"{where} scan {rep}: checksum"
    assert g.scan_format()[0] == record_width(table.num_final, knobs), f"{where}: record width"
    return rec


@pytest.mark.parametrize("plan", sorted(PLAN, key=lambda p: list(BUILDERS).index(p[0])), ids=label)
def test_scans_equal_the_trie_free_matcher(plan, tmp_path_factory, monkeypatch):
    name, width, knobs = plan
    b = big(name, tmp_path_factory)
    knobs_env(monkeypatch, knobs)
    table = b.table(width)
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        for kind, (data, n_owned) in b.inputs.items():
            check_scans(g, table, data, n_owned, b.expect(kind), knobs, f"{label(plan)} {kind}")
            if knobs == {"PFAC_DENSE": "1"} and name in SECOND_FORM:
                info = g.info()
                form2 = info["staging_buffers"] == 1 and info["staging_records"] == 4096
                assert form2 == SECOND_FORM[name], f"{label(plan)} {kind}: dense mode's second form {info}"
    wpos, wids = b.expect("edges")
    top = wids == table.idmap[table.num_final - 1]                          # records of final state F - 1
    assert ((wpos % 4096 == 0) & top).any() and ((wpos % 4096 == 4095) & top).any()
    if name == "F2^20":                                                      # the 4-byte record word 0xFFFFFFFF
        assert table.idmap[(1 << 20) - 1] == 1 << 20
    if name == "F2^20+1":                                                    # state 2^20 in an 8-byte record
        assert table.idmap[1 << 20] == (1 << 20) + 1


@pytest.mark.parametrize("name", ["F2^20+1", "DICT"])
def test_emitters(name, tmp_path_factory, tmp_path):
    """The GPU text emitter (7-digit ids on F2^20+1) at two bases, the host emitter from records and, for the compact
    4-byte form of DICT, the host emitter straight from the record heap -- each against lines formatted in Python."""
    b = big(name, tmp_path_factory)
    table = b.table(256)
    data, n_owned = b.inputs["edges"] if name != "DICT" else (b.inputs["text"][0][: 1 << 20], None)
    pos, ids = b.ref.scan_spec(data, None, n_owned)
    if name == "F2^20+1":
        assert ids.max() >= 10**6
    with GpuMatcher(0, 1) as g:
        g.load_table(table)
        rec = g.scan_bytes(data, n_owned)
        for base in (0, 999_999_000):
            text = g.text_to_host(g.emit_text_device(base))
            assert text == format_lines(pos, ids, base), f"GPU text emitter, base {base}"
        emit_records(str(tmp_path / "h.txt"), rec, table.idmap)
        assert (tmp_path / "h.txt").read_bytes() == format_lines(pos, ids)
        if g.scan_format()[0] < 8:
            words, tix = g.packed_to_host()
            emit_packed(str(tmp_path / "p.txt"), words, tix, table.idmap, threads=3)
            assert (tmp_path / "p.txt").read_bytes() == format_lines(pos, ids)
        else:
            assert name == "F2^20+1"


@pytest.mark.parametrize("name,kind", [("F2^20+1", "planted"), ("F2^20+1", "edges"), ("DICT", "text")])
def test_documents_selection_replace(name, kind, tmp_path_factory, tmp_path):
    """tests/passfuzz.py's checks of the post-scan passes with the trie-free matcher's expectations: final-length and
    replacement tables of more than 2^20 states on the device."""
    b = big(name, tmp_path_factory)
    data, n_owned = b.inputs[kind]
    data = data[: 2 << 20]
    c = BigCase(b.s, data, data.size if n_owned is None else min(n_owned, data.size), seed=len(kind))
    assert run_case(lambda: GpuMatcher(0, 1), c, str(tmp_path), matcher=b.ref) > 0


@pytest.mark.parametrize("name", ["F2^20+1", "DICT"])
def test_pattern_partitions(name, tmp_path_factory):
    b = big(name, tmp_path_factory)
    data, _ = b.inputs["planted"]
    pos, ids = b.ref.scan_spec(data)
    for n_parts in (2, 3):
        tabs = [PfacTable.from_file_part(b.path, 256, k, n_parts) for k in range(n_parts)]
        assert sum(t.num_final for t in tabs) == b.s.want["num_final"]
        with GpuMatcher(0, 1) as g:
            merged = g.scan_partitioned(tabs, data)
        np.testing.assert_array_equal(merged["pos"].astype(np.int64), pos)
        np.testing.assert_array_equal(merged["state"].astype(np.int32), ids)


@pytest.mark.parametrize("emit", ["host", "device"])
def test_gphf_8_byte_records(emit, tmp_path_factory, tmp_path):
    """The CLI on F2^20+1 (8-byte records through its chunk pipeline), two workers, 1 MiB chunks: byte-identical to
    the reference text of the input without its last byte (main.cc:138)."""
    b = big("F2^20+1", tmp_path_factory)
    data = np.concatenate([b.inputs["planted"][0], b.inputs["edges"][0]])
    (tmp_path / "in.txt").write_bytes(data.tobytes())
    exe = os.path.join(os.path.dirname(HERE), "phfpfac_amd", "bin", "gphf")
    env = dict(os.environ, PFAC_CHUNK_MB="1", PFAC_WORKERS_PER_GPU="2", PFAC_EMIT=emit)
    subprocess.run([exe, b.path, "1", "256", str(tmp_path / "in.txt")], cwd=tmp_path, env=env, check=True,
                   stdout=subprocess.DEVNULL, timeout=600)
    pos, ids = b.ref.scan_spec(data[:-1])
    assert (tmp_path / "GPU_match_result.txt").read_bytes() == format_lines(pos, ids)
