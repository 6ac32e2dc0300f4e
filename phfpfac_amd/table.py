"""Host-side table build: pattern file -> PHF-compressed PFAC transition table.

Thin wrapper over ``libpfac_host.so`` (``csrc/pfac_table.c``), i.e. over the
replacement of the reference's ``create_PFAC_table_reorder()`` + ``FFDM()``
(main.cc:108,125).  All arithmetic happens in the C library.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._ffi import PFAC_NEAR_ANY_DIST, PFAC_NEAR_ORDERED, PFAC_SPAN_ANY, CTable, PfacError, host_lib
from ._ffi import NEAR_RULE_DTYPE as _NEAR_RULE_FIELDS
from ._ffi import SCORE_DTYPE as _SCORE_FIELDS
from ._ffi import SPAN_DTYPE as _SPAN_FIELDS

RECORD_DTYPE = np.dtype([("pos", np.uint32), ("state", np.uint32)])
SPAN_DTYPE = np.dtype(_SPAN_FIELDS)         # struct pfac_state_span
SCORE_DTYPE = np.dtype(_SCORE_FIELDS)       # struct pfac_doc_score
NEAR_RULE_DTYPE = np.dtype(_NEAR_RULE_FIELDS)       # struct pfac_near_rule


def _group_mask(groups) -> int:
    """A group index 0..63, an iterable of indices, or a ready mask (numpy.uint64) -> the 64-bit mask."""
    if isinstance(groups, np.uint64):
        return int(groups)
    mask = 0
    for g in ((groups,) if isinstance(groups, (int, np.integer)) else groups):
        if not 0 <= int(g) < 64:
            raise ValueError(f"group {int(g)} is outside 0..63")
        mask |= 1 << int(g)
    return mask


def near_rule(a, b, within=None, ordered: bool = False) -> np.ndarray:
    """One proximity rule of ``GpuMatcher.document_near_masks`` (``struct pfac_near_rule``, a ``NEAR_RULE_DTYPE``
    scalar array of shape ()): a record of the groups ``a`` and a record of the groups ``b`` whose starts are at most
    ``within`` bytes apart (None: anywhere in the same document), ``ordered``: the ``a`` record first.  ``a`` / ``b``
    are a group index, an iterable of indices, or a ready mask (``numpy.uint64``).  Stack several with ``numpy.stack``
    or pass a list of them."""
    dist = PFAC_NEAR_ANY_DIST if within is None else int(within)
    if not 0 <= dist <= PFAC_NEAR_ANY_DIST:
        raise ValueError("within is a distance in bytes, 0..2^32 - 1")
    out = np.zeros((), dtype=NEAR_RULE_DTYPE)
    out["a_groups"], out["b_groups"] = _group_mask(a), _group_mask(b)
    out["max_dist"], out["flags"] = dist, PFAC_NEAR_ORDERED if ordered else 0
    return out


class PfacTable:
    """One automaton over the whole pattern file, in the reference's table terms.

    Attributes mirror ``struct thread_data`` (main.cc:19-32): ``s0`` (root row),
    ``r``, ``HT``, ``val`` (the perfect hash), ``width``, ``ht_size`` (HTSize),
    ``state_num``, ``num_final`` (final_state_num), ``max_pat_len``; ``idmap``
    is ``patternIdMaps`` (final state -> 1-based pattern line number).

    ``ignore_case``: the table was built from folded patterns (``ignore_case=True`` of a constructor) and is meant
    for folded scans; ``GpuMatcher.load_table`` sets the scan's case fold from it.  The blob does not carry it.
    """

    def __init__(self, ptr, ignore_case: bool = False):
        self._ptr = ptr
        self.ignore_case = bool(ignore_case)
        t = ptr.contents
        for name in ("width", "width_bit", "n_patterns", "num_final", "state_num", "max_pat_len", "max_row",
                     "ht_size", "n_keys"):
            setattr(self, name, int(getattr(t, name)))
        self.s0 = np.ctypeslib.as_array(t.s0, (256,))
        self.r = np.ctypeslib.as_array(t.r, (self.max_row,))
        self.HT = np.ctypeslib.as_array(t.HT, (self.ht_size,))
        self.val = np.ctypeslib.as_array(t.val, (self.ht_size,))
        self.idmap = np.ctypeslib.as_array(t.idmap, (max(self.num_final, 1),))[: self.num_final]

    # -- construction -----------------------------------------------------
    @classmethod
    def from_file(cls, pattern_file: str, width: int = 256, escapes: bool = False, ignore_case: bool = False) -> "PfacTable":
        """``escapes=True`` reads the file like the reference's ``read_pattern_ext`` (backslash escapes).
        ``ignore_case=True`` folds the patterns (A-Z -> a-z, after escape decoding) before they are sorted."""
        L = host_lib()
        ptr = C.POINTER(CTable)()
        err = C.create_string_buffer(256)
        if ignore_case:
            rc = L.pfac_table_build_file_nocase(os.fsencode(pattern_file), int(width), int(bool(escapes)), C.byref(ptr), err, 256)
        else:
            fn = L.pfac_table_build_file_escaped if escapes else L.pfac_table_build_file
            rc = fn(os.fsencode(pattern_file), int(width), C.byref(ptr), err, 256)
        if rc:
            raise PfacError(rc, err.value.decode(errors="replace"))
        return cls(ptr, ignore_case)

    @classmethod
    def from_bytes(cls, patterns: bytes, width: int = 256, part: int = 0, n_parts: int = 1,
                   ignore_case: bool = False) -> "PfacTable":
        L = host_lib()
        ptr = C.POINTER(CTable)()
        err = C.create_string_buffer(256)
        buf = C.create_string_buffer(patterns, len(patterns))
        fn = L.pfac_table_build_mem_nocase if ignore_case else L.pfac_table_build_mem_part
        rc = fn(buf, len(patterns), int(width), int(part), int(n_parts), C.byref(ptr), err, 256)
        if rc:
            raise PfacError(rc, err.value.decode(errors="replace"))
        return cls(ptr, ignore_case)

    @classmethod
    def from_file_part(cls, pattern_file: str, width: int, part: int, n_parts: int, ignore_case: bool = False) -> "PfacTable":
        """Partition ``part`` of ``n_parts`` of the sorted pattern list -- the reference's pattern partitioning
        (create_table_reorder.c:217-247): every partition scans the whole input, ``merge_partitions`` merges.
        ``ignore_case=True``: the cuts are those of the folded, sorted list."""
        if ignore_case:
            with open(pattern_file, "rb") as f:
                return cls.from_bytes(f.read(), width, part, n_parts, ignore_case=True)
        L = host_lib()
        ptr = C.POINTER(CTable)()
        err = C.create_string_buffer(256)
        rc = L.pfac_table_build_file_part(os.fsencode(pattern_file), int(width), int(part), int(n_parts), C.byref(ptr),
                                          err, 256)
        if rc:
            raise PfacError(rc, err.value.decode(errors="replace"))
        return cls(ptr)

    @classmethod
    def from_charclass(cls, patterns, width: int = 256, ignore_case: bool = False) -> "PfacTable":
        """Character-class pattern file (path) or image (bytes): single characters and ``[...]`` / ``[^...]`` classes
        with ``l-r`` ranges, escape-aware (charset_table_reorder.c:45-168).  The table's final states can stand for
        several patterns: ``out_first`` / ``out_ids`` list them (``idmap`` holds the first); print with
        ``emit_records_multi``.  ``ignore_case=True`` folds single characters and the listed set of every class;
        ``[^...]`` complements the folded set."""
        from ._ffi import COutputs
        L = host_lib()
        ptr, optr = C.POINTER(CTable)(), C.POINTER(COutputs)()
        err = C.create_string_buffer(256)
        if isinstance(patterns, (bytes, bytearray)):
            buf = C.create_string_buffer(bytes(patterns), len(patterns))
            fn = L.pfac_table_build_mem_charclass_nocase if ignore_case else L.pfac_table_build_mem_charclass
            rc = fn(buf, len(patterns), int(width), C.byref(ptr), C.byref(optr), err, 256)
        else:
            fn = L.pfac_table_build_file_charclass_nocase if ignore_case else L.pfac_table_build_file_charclass
            rc = fn(os.fsencode(patterns), int(width), C.byref(ptr), C.byref(optr), err, 256)
        if rc:
            raise PfacError(rc, err.value.decode(errors="replace"))
        t = cls(ptr, ignore_case)
        o = optr.contents
        t.out_first = np.ctypeslib.as_array(o.first, (o.n_states + 1,)).copy()
        t.out_ids = np.ctypeslib.as_array(o.ids, (max(int(t.out_first[-1]), 1),))[: int(t.out_first[-1])].copy()
        L.pfac_outputs_free(optr)
        return t

    @classmethod
    def from_blob(cls, blob: np.ndarray, ignore_case: bool = False) -> "PfacTable":
        """``ignore_case``: what the table's builder was told -- the image does not carry it."""
        L = host_lib()
        blob = np.ascontiguousarray(blob, dtype=np.int32)
        ptr = C.POINTER(CTable)()
        rc = L.pfac_table_from_blob(blob.ctypes.data, blob.size, C.byref(ptr))
        if rc:
            raise PfacError(rc, "bad table image")
        return cls(ptr, ignore_case)

    @classmethod
    def from_reference_arrays(cls, s0, r, HT, val, idmap, width, state_num, num_final, ht_size, max_pat_len):
        """Wrap arrays produced by the reference's own FFDM() (main.cc:72-76,125)."""
        L = host_lib()
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (s0, r, HT, val, idmap)]
        ptr = C.POINTER(CTable)()
        rc = L.pfac_table_from_reference_arrays(*[a.ctypes.data for a in arrs], int(width), int(state_num),
                                                int(num_final), int(ht_size), int(max_pat_len), C.byref(ptr))
        if rc:
            raise PfacError(rc, "bad reference arrays")
        return cls(ptr)

    # -- use --------------------------------------------------------------
    def lookup(self, state: int, ch: int) -> int:
        """The device lookup (master_kernel.cu:52-63) evaluated on the host."""
        return int(host_lib().pfac_table_lookup(self._ptr, int(state), int(ch)))

    def final_lengths(self) -> np.ndarray:
        """int32[num_final]: bytes of the pattern(s) ending in each final state (its depth in the trie / DFA), -1 for
        a final state no input reaches (the state of a duplicate line).  Computed from the table alone."""
        out = np.empty(max(self.num_final, 1), dtype=np.int32)
        rc = host_lib().pfac_table_final_lengths(self._ptr, out.ctypes.data, out.size)
        if rc:
            raise PfacError(rc, "pfac_table_final_lengths")
        return out[: self.num_final]

    def blob(self) -> np.ndarray:
        """Flat int32 image (what gets uploaded / broadcast between ranks)."""
        L = host_lib()
        n = int(L.pfac_table_blob_words(self._ptr))
        out = np.empty(n, dtype=np.int32)
        rc = L.pfac_table_to_blob(self._ptr, out.ctypes.data, n)
        if rc:
            raise PfacError(rc, "pfac_table_to_blob")
        return out

    @property
    def halo(self) -> int:
        """Bytes a shard must be able to read past its owned range."""
        return max(self.max_pat_len - 1, 0)

    def pattern_ids(self, records: np.ndarray) -> np.ndarray:
        return self.idmap[records["state"]]

    def states_to_patterns(self, states) -> np.ndarray:
        """The 1-based pattern id of every final state of ``states`` (the column indices of
        ``GpuMatcher.term_counts_to_host``): ``idmap[state]``.  Only for a table with one id per final state: a
        character-class table whose states stand for several patterns raises ValueError -- read its ``outputs``
        (``out_first`` / ``out_ids``) instead."""
        first = getattr(self, "out_first", None)
        if first is not None and np.any(np.diff(np.asarray(first, dtype=np.int64)) != 1):
            raise ValueError("a final state of this character-class table stands for several patterns: take them from "
                             "its outputs (out_ids[out_first[s]:out_first[s + 1]])")
        st = np.asarray(states, dtype=np.int64)
        if st.size and (int(st.min()) < 0 or int(st.max()) >= self.num_final):
            raise ValueError(f"a state outside [0, num_final = {self.num_final})")
        return np.asarray(self.idmap, dtype=np.int64)[st]

    def counts_by_pattern(self, state_counts) -> np.ndarray:
        """Counts per final state (``GpuMatcher.state_counts_to_host``) -> uint64 counts indexed by the 1-based pattern
        id (entry 0 is unused), long enough for every id the table can report.  A literal table puts ``counts[s]`` at
        ``idmap[s]``: of duplicate lines the one that wins has the matches, the others 0.  A character-class table adds
        ``counts[s]`` to every pattern that ends in state s (``out_ids[out_first[s]:out_first[s + 1]]``)."""
        counts = np.asarray(state_counts, dtype=np.uint64).ravel()
        if counts.size != self.num_final:
            raise ValueError(f"need one count per final state ({self.num_final}), got {counts.size}")
        first = getattr(self, "out_first", None)
        if first is None:
            ids = np.asarray(self.idmap, dtype=np.int64)
        else:
            ids = np.asarray(self.out_ids, dtype=np.int64)
            counts = np.repeat(counts, np.diff(np.asarray(first, dtype=np.int64)))
        out = np.zeros(max(int(self.n_patterns), int(ids.max()) if ids.size else 0) + 1, dtype=np.uint64)
        np.add.at(out, ids, counts)
        return out

    def state_group_masks(self, groups) -> np.ndarray:
        """Pattern groups -> uint64[num_final] for ``pfac_table_set_state_groups``: bit g of ``masks[s]`` is set iff a
        pattern that ends in final state s belongs to group g (0..63).  ``groups`` is indexed by the 1-based pattern
        id (entry 0 is unused), one entry per id the table can report, as ``counts_by_pattern`` returns them: a group
        index, an iterable of indices, or None for a pattern in no group; a uint64 array holds ready masks.  A literal
        table takes ``masks[s]`` from ``idmap[s]``: of duplicate lines the winning line's groups.  A character-class
        table ORs the groups of every pattern that ends in state s (``out_ids[out_first[s]:out_first[s + 1]]``)."""
        first = getattr(self, "out_first", None)
        ids = np.asarray(self.idmap if first is None else self.out_ids, dtype=np.int64)
        need = max(int(self.n_patterns), int(ids.max()) if ids.size else 0) + 1
        if isinstance(groups, np.ndarray) and groups.dtype == np.uint64:
            by_id = groups.ravel()
        else:
            entries = list(groups)
            by_id = np.zeros(len(entries), dtype=np.uint64)
            for i, e in enumerate(entries[1:], 1):
                for g in (() if e is None else (e,) if isinstance(e, (int, np.integer)) else e):
                    if not 0 <= int(g) < 64:
                        raise ValueError(f"group {int(g)} of pattern id {i} is outside 0..63")
                    by_id[i] |= np.uint64(1) << np.uint64(int(g))
        if by_id.size != need:
            raise ValueError(f"need one entry per pattern id and the unused entry 0 ({need}), got {by_id.size}")
        per = by_id[ids]
        if first is None:
            return np.ascontiguousarray(per[: self.num_final], dtype=np.uint64)
        out = np.zeros(int(self.num_final), dtype=np.uint64)
        np.bitwise_or.at(out, np.repeat(np.arange(int(self.num_final)), np.diff(np.asarray(first, dtype=np.int64))), per)
        return out

    def _states_of_patterns(self):
        """{1-based pattern id: [final states an input can reach that report it]}: the inverse of ``idmap`` (of the
        outputs of a character-class table).  The state of a line that lost to a duplicate is reached by no input
        (``final_lengths`` -1) and is left out, so such an id has no entry."""
        first = getattr(self, "out_first", None)
        live = self.final_lengths() >= 0
        out = {}
        if first is None:
            for s, i in enumerate(np.asarray(self.idmap, dtype=np.int64).tolist()):
                if live[s]:
                    out.setdefault(i, []).append(s)
        else:
            first = np.asarray(first, dtype=np.int64)
            ids = np.asarray(self.out_ids, dtype=np.int64).tolist()
            for s in range(int(self.num_final)):
                if live[s]:
                    for i in ids[first[s]:first[s + 1]]:
                        out.setdefault(i, []).append(s)
        return out

    def rule_table(self, rules):
        """Rules over patterns -> ``(rule_ptr uint64[n_rules + 1], terms uint32[], need uint32[n_rules])`` for
        ``pfac_table_set_rules`` (``GpuMatcher.set_rules``).  ``rules`` is a list; an item is an iterable of 1-based
        pattern ids (all of them must occur), a dict ``{"all_of" | "any_of": ids, "none_of": ids, "need": k}``
        (``all_of``: every id; ``any_of``: one of them; ``need``: at least k of them; ``none_of``: none of these may
        occur), or a ready ``(positive states, negated states, need)`` triple of final states.  Pattern ids become
        states through the inverse of ``idmap``; two ids of one rule that end in one state are merged, and a default
        ``need`` counts distinct states.  ValueError, naming the id, for an id that lost to a duplicate line, a pattern
        of a character-class table that ends in several states, a negated term on a state that is also positive, and an
        explicit ``need`` above the distinct positive states."""
        from ._ffi import PFAC_RULE_NOT
        by_id, top = None, 0
        ptr, terms, need = [0], [], []

        def states(ids, r):
            nonlocal by_id, top
            if by_id is None:
                by_id = self._states_of_patterns()
                top = max(int(self.n_patterns), max(by_id, default=0))
            out = []
            for i in ids:
                st = by_id.get(int(i))
                if not 1 <= int(i) <= top:
                    raise ValueError(f"rule {r}: pattern id {int(i)} is outside 1..{top}")
                if not st:
                    raise ValueError(f"rule {r}: pattern id {int(i)} lost to a duplicate line: no input reaches its state")
                if len(st) > 1:
                    raise ValueError(f"rule {r}: pattern id {int(i)} ends in several final states ({st[0]}, {st[1]}, ...)")
                out.append((st[0], int(i)))
            return out

        for r, item in enumerate(rules):
            k = None
            if isinstance(item, tuple) and len(item) == 3 and not isinstance(item[0], (int, np.integer)):
                pos = [(int(s), None) for s in item[0]]
                neg = [(int(s), None) for s in item[1]]
                k = int(item[2])
                for s, _ in pos + neg:
                    if not 0 <= s < self.num_final:
                        raise ValueError(f"rule {r}: state {s} is outside [0, num_final = {self.num_final})")
            elif isinstance(item, dict):
                unknown = set(item) - {"all_of", "any_of", "none_of", "need"}
                if unknown or ("all_of" in item) == ("any_of" in item):
                    raise ValueError(f"rule {r}: a rule names all_of or any_of (one of them), none_of and need")
                pos = states(item.get("all_of", item.get("any_of")), r)
                neg = states(item.get("none_of", ()), r)
                k = int(item["need"]) if "need" in item else (1 if "any_of" in item else None)
            else:
                pos, neg = states(item, r), []
            named = lambda t: f"state {t[0]}" if t[1] is None else f"pattern id {t[1]}"     # noqa: E731
            p_states = {}
            for t in pos:
                p_states.setdefault(t[0], t)
            n_states = {}
            for t in neg:
                if t[0] in p_states:
                    raise ValueError(f"rule {r}: the negated {named(t)} ends in state {t[0]}, which {named(p_states[t[0]])} makes positive")
                n_states.setdefault(t[0], t)
            if not p_states:
                raise ValueError(f"rule {r}: a rule needs a positive term")
            if k is None:
                k = len(p_states)
            if not 1 <= k <= len(p_states):
                raise ValueError(f"rule {r}: need {k} is outside 1..{len(p_states)}, its distinct positive states")
            terms += sorted(p_states) + [s | PFAC_RULE_NOT for s in sorted(n_states)]
            need.append(k)
            ptr.append(len(terms))
        return (np.array(ptr, dtype=np.uint64), np.array(terms, dtype=np.uint32), np.array(need, dtype=np.uint32))

    def state_weights(self, weights) -> np.ndarray:
        """Pattern weights -> int32[num_final] for ``pfac_table_set_state_weights``.  ``weights`` is indexed by the
        1-based pattern id (entry 0 is unused), one integer per id the table can report, as in
        ``state_group_masks``.  A literal table takes ``weights[idmap[s]]``: of duplicate lines the winning line's
        weight.  A character-class table SUMS the weights of every pattern that ends in state s
        (``out_ids[out_first[s]:out_first[s + 1]]``), because every one of them matched there.  ValueError if a
        weight or a sum leaves int32."""
        first = getattr(self, "out_first", None)
        ids = np.asarray(self.idmap if first is None else self.out_ids, dtype=np.int64)
        need = max(int(self.n_patterns), int(ids.max()) if ids.size else 0) + 1
        given = list(weights)
        if len(given) != need:
            raise ValueError(f"need one entry per pattern id and the unused entry 0 ({need}), got {len(given)}")
        entries = [0] + [int(w) for w in given[1:]]
        lo, hi = -(2 ** 31), 2 ** 31 - 1
        for i, w in enumerate(entries):
            if not lo <= w <= hi:
                raise ValueError(f"weight {w} of pattern id {i} is outside int32")
        per = np.array(entries, dtype=np.int64)[ids]
        if first is None:
            out = per[: self.num_final]
        else:
            out = np.zeros(int(self.num_final), dtype=np.int64)
            np.add.at(out, np.repeat(np.arange(int(self.num_final)), np.diff(np.asarray(first, dtype=np.int64))), per)
            over = np.flatnonzero((out < lo) | (out > hi))
            if over.size:
                raise ValueError(f"the weights of the patterns that end in final state {int(over[0])} sum to {int(out[over[0]])}, outside int32")
        return np.ascontiguousarray(out, dtype=np.int32)

    def state_spans(self, rules) -> np.ndarray:
        """Anchors and offsets of the patterns -> ``SPAN_DTYPE[num_final]`` for ``pfac_table_set_state_spans``.
        ``rules`` is indexed by the 1-based pattern id (entry 0 is unused), one entry per id the table can report, as in
        ``state_group_masks``.  An entry is None (anywhere), ``"^"`` (at its line's start), ``"$"`` (at its end, in
        front of the delimiter), ``"^$"`` (the whole line), or ``(min_start, max_start, max_tail)`` with None for a
        bound that is not judged -- Snort's ``offset`` o and ``depth`` d of a pattern of length L are ``(o, o + d - L,
        None)``; a negative ``max_start`` (a depth shorter than the pattern) admits no start.  A literal table takes the
        rule of ``idmap[s]``: of duplicate lines the winning line's.  On a character-class table the ids that share a
        final state must carry the same rule: ValueError names them."""
        first = getattr(self, "out_first", None)
        ids = np.asarray(self.idmap if first is None else self.out_ids, dtype=np.int64)
        need = max(int(self.n_patterns), int(ids.max()) if ids.size else 0) + 1
        entries = list(rules)
        if len(entries) != need:
            raise ValueError(f"need one entry per pattern id and the unused entry 0 ({need}), got {len(entries)}")
        by_id = np.zeros(need, dtype=SPAN_DTYPE)
        by_id["max_start"] = by_id["max_tail"] = PFAC_SPAN_ANY
        for i, e in enumerate(entries[1:], 1):
            by_id[i] = _span_of(e, i)
        per = by_id[ids]
        if first is None:
            return np.ascontiguousarray(per[: self.num_final])
        first = np.asarray(first, dtype=np.int64)
        out = np.zeros(int(self.num_final), dtype=SPAN_DTYPE)
        out["max_start"] = out["max_tail"] = PFAC_SPAN_ANY          # (a state no pattern ends in)
        for s in range(int(self.num_final)):
            mine = per[first[s]:first[s + 1]]
            if mine.size:
                odd = np.flatnonzero(mine != mine[0])
                if odd.size:
                    a, b = int(ids[first[s]]), int(ids[first[s] + odd[0]])
                    raise ValueError(f"pattern ids {a} and {b} end in one final state ({s}) but carry different span rules")
                out[s] = mine[0]
        return out

    def __del__(self):
        ptr = getattr(self, "_ptr", None)
        if ptr is not None:
            try:
                host_lib().pfac_table_free(ptr)
            except Exception:
                pass
            self._ptr = None


_ANCHORS = {"^": (0, 0, None), "$": (0, None, 0), "^$": (0, 0, 0)}


def _span_of(rule, pattern_id: int) -> tuple:
    """One entry of ``PfacTable.state_spans`` -> (min_start, max_start, max_tail, 0) in the struct's terms."""
    if rule is None:
        return (0, PFAC_SPAN_ANY, PFAC_SPAN_ANY, 0)
    if isinstance(rule, str):
        if rule not in _ANCHORS:
            raise ValueError(f"the rule of pattern id {pattern_id} must be one of {sorted(_ANCHORS)}, a tuple or None")
        rule = _ANCHORS[rule]
    lo, hi, tail = rule
    lo = 0 if lo is None else int(lo)
    hi = PFAC_SPAN_ANY if hi is None else int(hi)
    tail = PFAC_SPAN_ANY if tail is None else int(tail)
    if hi < 0:                              # no admissible start: min_start > max_start
        lo, hi = 1, 0
    if not (0 <= lo <= PFAC_SPAN_ANY and hi <= PFAC_SPAN_ANY and 0 <= tail <= PFAC_SPAN_ANY):
        raise ValueError(f"the rule of pattern id {pattern_id} is outside 0..2^32 - 1")
    return (lo, hi, tail, 0)


def strip_anchors(lines) -> tuple:
    """Pattern lines with grep's anchors -> (lines, rules): a leading ``^`` and a trailing ``$`` are taken off every
    line (bytes) and become the line's rule for ``PfacTable.state_spans`` (``rules[0]`` is the unused entry 0, line k
    has pattern id k + 1).  Escapes are not handled: a caller whose patterns hold a literal ``^`` or ``$`` there passes
    the rules itself.  Two lines that differ only in their anchors become duplicate lines: one final state, and the
    winning line's rule.  A line that is empty after stripping raises ValueError."""
    out, rules = [], [None]
    for k, line in enumerate(lines):
        line = bytes(line)
        head, tail = line.startswith(b"^"), line.endswith(b"$") and len(line) > (1 if line.startswith(b"^") else 0)
        body = line[1 if head else 0:len(line) - (1 if tail else 0)]
        if not body:
            raise ValueError(f"pattern line {k + 1} is empty once its anchors are stripped")
        out.append(body)
        rules.append(("^" if head else "") + ("$" if tail else "") or None)
    return out, rules


def fold_ascii(data) -> np.ndarray:
    """The case fold of an ``ignore_case`` scan, on the host (``pfac_fold_ascii``): a uint8 copy of ``data`` (bytes or a
    uint8 array) with A-Z turned into a-z and every other byte, all of 0x80..0xFF included, unchanged."""
    src = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview))
                               else np.asarray(data, dtype=np.uint8))
    out = np.empty_like(src)
    rc = host_lib().pfac_fold_ascii(out.ctypes.data, src.ctypes.data, src.size)
    if rc:
        raise PfacError(rc, "pfac_fold_ascii")
    return out


MAX_REPLACEMENT = 65536              # bytes of one replacement (PFAC_MAX_REPLACEMENT)


def _state_lengths(table: "PfacTable") -> np.ndarray:
    lens = getattr(table, "_final_lengths", None)
    if lens is None:
        lens = table.final_lengths()
        table._final_lengths = lens          # once per table
    return lens


def replacement_table(table: "PfacTable", replacements) -> tuple:
    """-> (offsets uint32[num_final + 1], bytes): the replacement of every final state, for
    ``pfac_table_set_replacements``.  ``replacements`` is a dict {pattern id: bytes} or a sequence with one entry per
    line of the pattern file, in file order (``replacements[id - 1]``; None = none given).  A state gets the
    replacement of ``idmap[s]``: the winning line of duplicates, the first (lowest) id of a character-class state.
    Unreachable states get an empty one.  Every reachable state must be covered: ValueError names the smallest id
    that is missing."""
    lens = _state_lengths(table)
    ids = np.asarray(table.idmap, dtype=np.int64)
    if isinstance(replacements, dict):
        get = replacements.get
    else:
        seq = list(replacements)
        get = lambda i: seq[i - 1] if 1 <= i <= len(seq) else None   # noqa: E731
    offsets = np.zeros(int(table.num_final) + 1, dtype=np.uint32)
    parts, missing, at = [], [], 0
    for s in range(int(table.num_final)):
        if lens[s] >= 1:
            r = get(int(ids[s]))
            if r is None:
                missing.append(int(ids[s]))
            else:
                r = bytes(r)
                if len(r) > MAX_REPLACEMENT:
                    raise ValueError(f"the replacement of pattern id {int(ids[s])} is longer than {MAX_REPLACEMENT} bytes")
                parts.append(r)
                at += len(r)
        offsets[s + 1] = at
    if missing:
        raise ValueError(f"no replacement for pattern id {min(missing)}")
    return offsets, b"".join(parts)


TOKEN_DROP = -1                      # PFAC_TOKEN_DROP: the state (or byte) emits no token


def token_table(table: "PfacTable", ids) -> np.ndarray:
    """-> int32[num_final]: the token id of every final state, for ``pfac_table_set_token_ids``.  ``ids`` is a dict
    {pattern id: token id} or a sequence with one entry per line of the pattern file, in file order (``ids[id - 1]``;
    None = none given).  A state gets the token of ``idmap[s]`` exactly as ``replacement_table`` maps a replacement:
    the winning line of duplicates, the first (lowest) id of a character-class state.  Patterns that are not named, and
    unreachable states, are TOKEN_DROP.  A token id is >= 0 or TOKEN_DROP (else ValueError) and fits int32."""
    lens = _state_lengths(table)
    idmap = np.asarray(table.idmap, dtype=np.int64)
    if isinstance(ids, dict):
        get = ids.get
    else:
        seq = list(ids)
        get = lambda i: seq[i - 1] if 1 <= i <= len(seq) else None   # noqa: E731
    out = np.full(int(table.num_final), TOKEN_DROP, dtype=np.int32)
    for s in range(int(table.num_final)):
        if lens[s] >= 1:
            t = get(int(idmap[s]))
            if t is not None:
                t = int(t)
                if t < TOKEN_DROP or t >= 2**31:
                    raise ValueError(f"the token id of pattern id {int(idmap[s])} is neither in [0, 2^31) nor TOKEN_DROP")
                out[s] = t
    return out


WORD_BYTES = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ_abcdefghijklmnopqrstuvwxyz"    # the default word set of the filters


def wordpiece_table(vocab, prefix: bytes = b"##", word_bytes=None, ignore_case: bool = False) -> tuple:
    """A WordPiece vocabulary as ONE automaton with two ids per final state, for ``pfac_table_set_wordpiece``.
    ``vocab`` is a sequence of entries (bytes or str; entry k has token id k, as in a BERT ``vocab.txt``) or the path of
    such a file, one entry per line.  ``word_bytes``: the bytes that make up words (None = ``[0-9A-Za-z_]``).
    Returns (table, first_ids int32[num_final], cont_ids int32[num_final], byte_ids int32[256], skipped):

    - the patterns are the distinct stripped strings (``##ing`` is inserted as ``ing``) made of word bytes only, folded
      under ``ignore_case``; a state's first id is the id of the plain entry, its continuation id that of the
      ``prefix`` entry, TOKEN_DROP where the vocabulary has none;
    - an entry of one non-word byte gives that byte's id in ``byte_ids`` (TOKEN_DROP elsewhere);
    - ``skipped`` lists (id, entry) of everything the rule can never produce: ``[CLS]``, a ``##`` piece with a non-word
      byte, an empty string, an entry that holds a newline, a pattern of 1024 bytes or more, and the later of two
      entries that are the same piece.

    The states take their ids as ``token_table`` maps them (``idmap[s]``)."""
    if isinstance(vocab, (str, os.PathLike)):
        with open(vocab, "rb") as f:
            lines = f.read().split(b"\n")
        if lines and lines[-1] == b"":
            lines.pop()
        entries = [e[:-1] if e.endswith(b"\r") else e for e in lines]
    else:
        entries = [e.encode() if isinstance(e, str) else bytes(e) for e in vocab]
    prefix = bytes(prefix)
    words = set(WORD_BYTES if word_bytes is None else bytes(word_bytes))
    byte_ids = np.full(256, TOKEN_DROP, dtype=np.int32)
    lines, ids, skipped = [], {}, []           # pattern lines in order; piece -> [first id, continuation id]
    for k, e in enumerate(entries):
        cont = len(prefix) > 0 and e.startswith(prefix) and len(e) > len(prefix)
        piece = e[len(prefix):] if cont else e
        if ignore_case:
            piece = bytes(fold_ascii(piece)) if piece else piece
        if piece and len(piece) < 1024 and b"\n" not in piece and all(b in words for b in piece):
            pair = ids.get(piece)
            if pair is None:
                pair = ids[piece] = [TOKEN_DROP, TOKEN_DROP]
                lines.append(piece)
            if pair[cont] == TOKEN_DROP:
                pair[cont] = k
                continue
        elif not cont and len(e) == 1 and e[0] not in words and e != b"\n" and byte_ids[e[0]] == TOKEN_DROP:
            byte_ids[e[0]] = k
            continue
        skipped.append((k, e))
    if not lines:
        raise ValueError("the vocabulary holds no piece made of word bytes")
    table = PfacTable.from_bytes(b"".join(p + b"\n" for p in lines), 256, ignore_case=ignore_case)
    first = token_table(table, [ids[p][0] for p in lines])
    cont = token_table(table, [ids[p][1] for p in lines])
    return table, first, cont, byte_ids, skipped


UNIGRAM_PIECE_DTYPE = np.dtype([("first_id", "<i4"), ("cont_id", "<i4"), ("first_score", "<i4"), ("cont_score", "<i4")])   # pfac_unigram_piece
UNIGRAM_SPACE = bytes(b for b in range(256) if b not in b"\t\n\v\f\r ")      # the default word set: SentencePiece splits at whitespace


def unigram_scale_fits(score: int, max_word_bytes: int) -> bool:
    """The bound of ``pfac_table_set_unigram``: sums of at most max_word_bytes + 1 such scores stay in int32."""
    return abs(int(score)) * (int(max_word_bytes) + 1) < 2**31


def unigram_table(vocab, prefix="▁", word_bytes=None, max_word_bytes: int = 100, scale=None, ignore_case: bool = False) -> tuple:
    """A Unigram (SentencePiece-style) vocabulary as ONE automaton with a pair of (id, score) per final state, for
    ``pfac_table_set_unigram``.  ``vocab`` is a sequence of (piece, score): piece bytes or str, score the piece's
    log-probability as a float; entry k has token id k.  ``word_bytes``: the bytes that make up words (None = every
    byte but ``\\t\\n\\v\\f\\r`` and space).  Scores become integers, ``round(score * scale)``; ``scale=None`` picks the
    largest power of two <= 2^16 under which every score keeps ``|score| * (max_word_bytes + 1) < 2^31``; a given
    ``scale`` that breaks the bound is a ValueError (the runtime would answer PFAC_E_ARG).
    Returns (table, pieces UNIGRAM_PIECE_DTYPE[num_final], scale, skipped):

    - the patterns are the distinct stripped strings (``▁the`` is inserted as ``the``) made of word bytes only, folded
      under ``ignore_case``; ``▁the`` gives its state's first id and score, a plain ``the`` the continuation ones;
      TOKEN_DROP (score 0) where the vocabulary has none;
    - ``skipped`` lists (id, entry) of everything the rule can never produce: the bare prefix, a piece with the prefix
      inside it, a piece with a non-word byte, an empty entry, a pattern of 1024 bytes or more, the later of two
      entries that are the same piece, and control entries (``<unk>``, ``<s>``, ``<0x0A>``: anything in angle
      brackets).  Byte-fallback ids are the caller's to pass as ``byte_ids``."""
    prefix = prefix.encode() if isinstance(prefix, str) else bytes(prefix)
    words = set(UNIGRAM_SPACE if word_bytes is None else bytes(word_bytes))
    entries = [((e.encode() if isinstance(e, str) else bytes(e)), float(sc)) for e, sc in vocab]
    lines, slots, skipped = [], {}, []          # pattern lines in order; piece -> [first entry, continuation entry]
    for k, (e, _) in enumerate(entries):
        first = len(prefix) > 0 and e.startswith(prefix)
        piece = e[len(prefix):] if first else e
        if ignore_case and piece:
            piece = bytes(fold_ascii(piece))
        control = len(e) >= 2 and e.startswith(b"<") and e.endswith(b">")
        if (piece and not control and len(piece) < 1024 and (not prefix or prefix not in piece) and b"\n" not in piece
                and all(b in words for b in piece)):
            pair = slots.get(piece)
            if pair is None:
                pair = slots[piece] = [None, None]
                lines.append(piece)
            if pair[0 if first else 1] is None:
                pair[0 if first else 1] = k
                continue
        skipped.append((k, e))
    if not lines:
        raise ValueError("the vocabulary holds no piece made of word bytes")
    kept = [k for pair in slots.values() for k in pair if k is not None]
    top = max(abs(entries[k][1]) for k in kept)
    if scale is None:
        scale = 2.0**16
        while scale > 2.0**-40 and not unigram_scale_fits(round(top * scale), max_word_bytes):
            scale /= 2.0
    scale = float(scale)
    if not unigram_scale_fits(round(top * scale), max_word_bytes):
        raise ValueError(f"a score of {top} times the scale {scale} breaks |score| * (max_word_bytes + 1) < 2^31")
    table = PfacTable.from_bytes(b"".join(p + b"\n" for p in lines), 256, ignore_case=ignore_case)
    line_of = token_table(table, list(range(len(lines))))
    pieces = np.zeros(int(table.num_final), dtype=UNIGRAM_PIECE_DTYPE)
    pieces["first_id"] = pieces["cont_id"] = TOKEN_DROP
    for s, ln in enumerate(line_of):
        if ln < 0:
            continue
        for half, k in zip(("first", "cont"), slots[lines[ln]]):
            if k is not None:
                pieces[half + "_id"][s] = k
                pieces[half + "_score"][s] = int(round(entries[k][1] * scale))
    return table, pieces, scale, skipped


BPE_PIECE_DTYPE = np.dtype([("id", "<i4"), ("rank", "<i4"), ("split", "<u4"), ("reserved", "<u4")])   # pfac_bpe_piece


def bpe_byte_alphabet() -> dict:
    """The printable alphabet of byte-level BPE vocabularies (GPT-2's): a byte whose Latin-1 character is printable
    and not a space stands for itself, every other byte takes the code points 256, 257, ... in ascending order (so the
    space is ``Ġ`` and the newline ``Ċ``).  Returns byte -> character."""
    import unicodedata
    out, spare = {}, 256
    for b in range(256):
        if unicodedata.category(chr(b))[0] in "CZ":
            out[b] = chr(spare)
            spare += 1
        else:
            out[b] = chr(b)
    return out


def bpe_table(vocab, merges, byte_level: bool = True, lead=b" ", word_bytes=None, max_word_bytes: int = 64,
              any_split: bool = False, ignore_case: bool = False) -> tuple:
    """A byte-pair-encoding vocabulary as it ships (``vocab.json`` plus ``merges.txt``, or the ``model`` part of a
    ``tokenizer.json``) as ONE automaton with an (id, rank, split) per final state, for ``pfac_table_set_bpe``.
    ``vocab`` maps token -> id; ``merges`` is the ordered list of pairs (two-element sequences, or ``"left right"``).
    ``byte_level``: the tokens are written in the printable byte alphabet (``bpe_byte_alphabet``) and are mapped back
    to bytes; else a token is its bytes (str: UTF-8).  ``lead``: the one byte outside words that a word takes from in
    front of it (None: none); ``word_bytes`` as for ``unigram_table``; ``any_split``: every split 0 (the rank belongs
    to the string, ``tiktoken``'s form); ``max_word_bytes`` is checked against 1..255 and is otherwise the caller's to
    pass to ``set_bpe``.  Returns (table, pieces BPE_PIECE_DTYPE[num_final], byte_ids int32[256], skipped):

    - the patterns are the distinct merged strings of at least 2 bytes, folded under ``ignore_case``; merge k gives its
      string rank k and split ``len(left)``; the id is the vocabulary's;
    - ``byte_ids`` holds the ids of the single-byte tokens, TOKEN_DROP where there is none;
    - ``skipped`` lists (merge index, (left, right), reason) or (id, token, reason) of what the rule can never produce:
      a non-word byte other than a lead at offset 0 (``"non-word byte"``), a lead anywhere else (``"lead inside"``),
      ``"newline"``, 1 024 bytes or more (``"too long"``), a merge whose result is ``"not in vocab"``, the later of two
      merges that make the same string (``"ambiguous"``), a token outside the byte alphabet (``"not byte-level"``) and
      a token of two or more bytes that no merge makes (``"no merge"``)."""
    if not 1 <= int(max_word_bytes) <= 255:
        raise ValueError("max_word_bytes must lie in 1..255")
    if lead is None or (isinstance(lead, int) and lead < 0):
        lead_b = -1
    else:
        lead_b = int(lead) if isinstance(lead, int) else bytes(lead)[0]
    words = set(UNIGRAM_SPACE if word_bytes is None else bytes(word_bytes))
    if lead_b in words:
        raise ValueError("the lead byte is a word byte")
    back = {c: b for b, c in bpe_byte_alphabet().items()} if byte_level else None

    def raw(tok):
        if isinstance(tok, (bytes, bytearray)):
            return bytes(tok)
        if back is None:
            return tok.encode()
        try:
            return bytes(back[c] for c in tok)
        except KeyError:
            return None

    def refuses(s):
        if b"\n" in s:
            return "newline"
        if len(s) >= 1024:
            return "too long"
        for j, b in enumerate(s):
            if b not in words:
                if b != lead_b:
                    return "non-word byte"
                if j:
                    return "lead inside"
        return None
    ids, skipped = {}, []
    byte_ids = np.full(256, TOKEN_DROP, dtype=np.int32)
    for tok, i in vocab.items():
        b = raw(tok)
        if b is None:
            skipped.append((int(i), tok, "not byte-level"))
        elif len(b) == 1:
            byte_ids[b[0]] = int(i)
        elif b:
            ids.setdefault(b, (int(i), tok))
    lines, made = [], {}
    for k, m in enumerate(merges):
        l, r = m.split(" ") if isinstance(m, str) else m
        lb, rb = raw(l), raw(r)
        if lb is None or rb is None:
            skipped.append((k, (l, r), "not byte-level"))
            continue
        s = lb + rb
        why = refuses(bytes(fold_ascii(s)) if ignore_case else s)
        if why is None and s not in ids:
            why = "not in vocab"
        key = bytes(fold_ascii(s)) if ignore_case else s
        if why is None and key in made:
            why = "ambiguous"
        if why is not None:
            skipped.append((k, (l, r), why))
            continue
        made[key] = (ids[s][0], k, 0 if any_split else len(lb))
        lines.append(key)
    if not lines:
        raise ValueError("no merge makes a string of word bytes that the vocabulary holds")
    for s, (i, tok) in ids.items():
        if (bytes(fold_ascii(s)) if ignore_case else s) not in made:
            skipped.append((i, tok, "no merge"))
    table = PfacTable.from_bytes(b"".join(p + b"\n" for p in lines), 256, ignore_case=ignore_case)
    line_of = token_table(table, list(range(len(lines))))
    pieces = np.zeros(int(table.num_final), dtype=BPE_PIECE_DTYPE)
    pieces["id"] = TOKEN_DROP
    for s, ln in enumerate(line_of):
        if ln >= 0:
            pieces["id"][s], pieces["rank"][s], pieces["split"][s] = made[lines[ln]]
    return table, pieces, byte_ids, skipped


TEMPLATE_PLAIN = 0xFFFFFFFF          # PFAC_TEMPLATE_PLAIN: the state's replacement does not quote the match


def _template_of(t, pattern_id: int) -> tuple:
    """One template -> (replacement bytes, split): bytes = plain, (prefix, suffix) = the match quoted between them."""
    if isinstance(t, (bytes, bytearray, memoryview, np.ndarray)):
        r, split = bytes(t), TEMPLATE_PLAIN
    else:
        try:
            prefix, suffix = t
        except (TypeError, ValueError):
            raise ValueError(f"the template of pattern id {pattern_id} must be bytes or a (prefix, suffix) pair") from None
        prefix, suffix = bytes(prefix), bytes(suffix)
        r, split = prefix + suffix, len(prefix)
    if len(r) > MAX_REPLACEMENT:
        raise ValueError(f"the template of pattern id {pattern_id} is longer than {MAX_REPLACEMENT} bytes")
    return r, split


def template_table(table: "PfacTable", templates) -> tuple:
    """-> (offsets uint32[num_final + 1], splits uint32[num_final], bytes): the replacement template of every final
    state, for ``pfac_table_set_replacement_templates``.  ``templates`` is a dict {pattern id: template} or a sequence
    with one entry per line of the pattern file, resolved through ``idmap`` exactly as ``replacement_table`` does.  A
    template is bytes (a plain replacement) or a pair (prefix, suffix): the pick becomes prefix + the matched bytes as
    they stand in the input + suffix.  Unreachable states get an empty plain one; every reachable state must be
    covered.  On a character-class table the ids that share a final state must carry the same template: ValueError
    names them, as ``state_spans`` does."""
    lens = _state_lengths(table)
    ids = np.asarray(table.idmap, dtype=np.int64)
    first = getattr(table, "out_first", None)
    if isinstance(templates, dict):
        get = templates.get
    else:
        seq = list(templates)
        get = lambda i: seq[i - 1] if 1 <= i <= len(seq) else None   # noqa: E731
    n_states = int(table.num_final)
    offsets = np.zeros(n_states + 1, dtype=np.uint32)
    splits = np.full(n_states, TEMPLATE_PLAIN, dtype=np.uint32)
    parts, missing, at = [], [], 0
    for s in range(n_states):
        if lens[s] >= 1:
            i = int(ids[s])
            t = get(i)
            if t is None:
                missing.append(i)
            else:
                r, splits[s] = _template_of(t, i)
                if first is not None:
                    for j in table.out_ids[int(first[s]):int(first[s + 1])]:
                        other = get(int(j))
                        if other is None or _template_of(other, int(j)) != (r, int(splits[s])):
                            raise ValueError(f"pattern ids {i} and {int(j)} end in one final state ({s}) but carry different templates")
                parts.append(r)
                at += len(r)
        offsets[s + 1] = at
    if missing:
        raise ValueError(f"no template for pattern id {min(missing)}")
    return offsets, splits, b"".join(parts)


def redaction_table(table: "PfacTable", fill: bytes = b"*") -> tuple:
    """``replacement_table`` of a redaction: every reachable state gets ``fill`` repeated to its pattern length."""
    lens = _state_lengths(table)
    fill = bytes(fill)
    reps = [fill * int(n) if n >= 1 else b"" for n in lens]
    offsets = np.zeros(int(table.num_final) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(r) for r in reps], dtype=np.uint64)
    return offsets, b"".join(reps)


def merge_partitions(record_lists, idmaps=None) -> np.ndarray:
    """The reference's host merge (main.cc:304-324) on compact records: ``record_lists[k]`` are the position-sorted
    records of pattern partition k; returns one array ordered by (position, partition) whose ``state`` field holds
    the PATTERN ID (``idmaps[k]`` applied; None = the lists already hold ids)."""
    L = host_lib()
    lists = [np.ascontiguousarray(r, dtype=RECORD_DTYPE) for r in record_lists]
    k = len(lists)
    maps = [None if idmaps is None or m is None else np.ascontiguousarray(m, dtype=np.int32) for m in (idmaps or [None] * k)]
    ptrs = (C.c_void_p * max(k, 1))(*[r.ctypes.data if r.size else None for r in lists])
    counts = (C.c_uint64 * max(k, 1))(*[r.size for r in lists])
    mptrs = (C.c_void_p * max(k, 1))(*[None if m is None else m.ctypes.data for m in maps])
    total = sum(r.size for r in lists)
    out = np.empty(total, dtype=RECORD_DTYPE)
    n = L.pfac_merge_partitions(ptrs, counts, mptrs, k, out.ctypes.data, total)
    if n != total:
        raise PfacError(int(n), "pfac_merge_partitions")
    return out


def emit_records(path_or_file, records: np.ndarray, idmap, base: int = 0, append: bool = False,
                 threads: int = 1) -> int:
    """Write ``At position %4d, match pattern %d`` lines (main.cc:335-350).  Returns bytes written.
    ``threads`` > 1 uses the parallel emitter (same bytes).  ``idmap`` None: ``records["state"]`` already holds
    pattern ids (the output of ``merge_partitions``)."""
    L = host_lib()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    idmap = None if idmap is None else np.ascontiguousarray(idmap, dtype=np.int32)
    idmap_ptr = None if idmap is None else idmap.ctypes.data
    libc.fseek.argtypes = [C.c_void_p, C.c_long, C.c_int]
    # append = open for update and seek to the end (an "a" stream is O_APPEND, which defeats positioned writes)
    f = libc.fopen(os.fsencode(path_or_file), b"r+b" if append and os.path.exists(path_or_file) else b"wb")
    if not f:
        raise PfacError(-2, f"cannot open {path_or_file}")
    if append:
        libc.fseek(f, 0, 2)
    try:
        if threads > 1:
            n = L.pfac_emit_records_mt(f, records.ctypes.data, records.size, int(base), idmap_ptr, int(threads))
        else:
            n = L.pfac_emit_records(f, records.ctypes.data, records.size, int(base), idmap_ptr)
    finally:
        libc.fclose(f)
    if n < 0:
        raise PfacError(int(n), "pfac_emit_records")
    return int(n)


def emit_packed(path, words: np.ndarray, tile_index: np.ndarray, idmap, base: int = 0, threads: int = 1) -> int:
    """The same text straight from the compact device form (``GpuMatcher.packed_to_host``): record heap + ordered tile
    index (include/pfac.h).  Returns bytes written."""
    L = host_lib()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    words = np.ascontiguousarray(words)
    if words.dtype not in (np.uint16, np.uint32):
        raise TypeError("compact records are uint16 or uint32 words")
    tix = np.ascontiguousarray(tile_index, dtype=np.uint64)
    idmap = None if idmap is None else np.ascontiguousarray(idmap, dtype=np.int32)
    f = libc.fopen(os.fsencode(path), b"wb")
    if not f:
        raise PfacError(-2, f"cannot open {path}")
    try:
        n = L.pfac_emit_packed(f, words.ctypes.data, int(words.size), int(words.dtype.itemsize), tix.ctypes.data, tix.size, int(base),
                               None if idmap is None else idmap.ctypes.data, int(threads))
    finally:
        libc.fclose(f)
    if n < 0:
        raise PfacError(int(n), "pfac_emit_packed")
    return int(n)


def emit_records_multi(path, records: np.ndarray, table: "PfacTable", base: int = 0) -> int:
    """Text for a character-class table: one line per (record, pattern that ends in the record's final state)."""
    from ._ffi import COutputs
    L = host_lib()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    first = np.ascontiguousarray(table.out_first, dtype=np.int32)
    ids = np.ascontiguousarray(table.out_ids if table.out_ids.size else np.zeros(1, np.int32), dtype=np.int32)
    o = COutputs(int(first.size - 1), first.ctypes.data_as(C.POINTER(C.c_int32)), ids.ctypes.data_as(C.POINTER(C.c_int32)))
    f = libc.fopen(os.fsencode(path), b"wb")
    if not f:
        raise PfacError(-2, f"cannot open {path}")
    try:
        n = L.pfac_emit_records_multi(f, records.ctypes.data, records.size, int(base), C.byref(o))
    finally:
        libc.fclose(f)
    if n < 0:
        raise PfacError(int(n), "pfac_emit_records_multi")
    return int(n)
