"""The rule-set reference against itself, without a GPU: tests/ruleref.py holds the rule three times and makes the cases
of tests/test_gpu_rules.py; here the three agree, every case has the property it is named for, the checker refuses
wrong results of five kinds, and PfacTable.rule_table maps pattern ids to states and refuses what it must.  (The host
validation of pfac_table_set_rules needs a context, and a context needs a device: it is in the GPU file.)"""
import numpy as np
import pytest

import ruleref
from phfpfac_amd import PFAC_RULE_NOT, PfacTable
from ruleref import BLOCK, EDGES, GROUP, SORT_BLOCK, Rules, cases, check, dense, fired, fired_dense, fired_sets, from_docs, seeded

SMALL = 1 << 20                                 # cells of a dense form that is still built


def all_cases():
    return [c for W in (2, 4) for c in cases(W).values()]


def test_names_are_the_cases():
    for W in (2, 4):
        assert list(cases(W)) == ruleref.names(W)


def test_the_three_references_agree_on_the_named_cases():
    n_sets = n_dense = 0
    for c in all_cases():
        want = c.want()
        if c.E <= 500000:
            check(want, *fired_sets(c.row, c.states, c.rules), what=f"{c.name}: the sets")
            n_sets += 1
        nr = c.rules.n_rules
        if c.n_docs and max(c.n_docs * c.num_final, c.num_final * nr, c.n_docs * nr) <= SMALL:
            np.testing.assert_array_equal(dense(*want, nr), fired_dense(c.row, c.states, c.rules), err_msg=c.name)
            n_dense += 1
    assert n_sets >= len(all_cases()) - 1 and n_dense >= 40


def test_the_three_references_agree_on_seeded_cases():
    dull = 0
    for seed in range(64):
        c = seeded(seed)
        want = c.want()
        check(want, *fired_sets(c.row, c.states, c.rules), what=c.name)
        m = fired_dense(c.row, c.states, c.rules)
        np.testing.assert_array_equal(dense(*want, c.rules.n_rules), m, err_msg=c.name)
        dull += int(m.sum() == 0 or m.all())
    assert dull <= 8, f"{dull} of 64 seeded cases fire nothing or everything"


def test_sizes():
    by = cases(2)
    for E in ruleref.SIZES:
        assert by[f"E{E}"].E == E
    assert by["big"].E == ruleref.BIG_E and -(-by["big"].E // GROUP) > 1024
    assert by["E0"].n > 0 and by["E0"].want()[1].size == 0              # pairs, but every state in no rule
    for c in (by["nodocs"], by["nopairs"]):
        assert c.n == 0 and c.E == 0 and c.want()[1].size == 0
    assert by["nodocs"].n_docs == 0 and by["nopairs"].n_docs == 100
    assert cases(4)["E4097"].num_final > 1000


def test_every_firing_case_sets_something_and_leaves_something_clear():
    for c in all_cases():
        n = c.want()[1].size
        if c.name in ("E0", "nodocs", "nopairs", "nothing"):
            continue
        if c.name.startswith("passes-") and (c.rules.n_rules == 1 or c.n_docs * c.rules.n_rules <= 4):       # (one rule, or two cells)
            assert n > 0, c.name
            continue
        if c.name == "allfire":
            assert n == c.n_docs * c.rules.n_rules > 0
            continue
        assert 0 < n < c.n_docs * c.rules.n_rules, c.name
    assert cases(2)["nothing"].E > 1000 and cases(2)["nothing"].want()[1].size == 0


def test_run_positions():
    for edge in EDGES:
        assert cases(2)[f"edge{edge}"].reaches_back_over(edge) >= 1
    assert cases(2)["edge4096"].reaches_back_over(BLOCK) >= 1 and cases(2)["edge4096"].reaches_back_over(SORT_BLOCK) >= 1
    big = cases(2)["big"]
    assert all(big.reaches_back_over(e) > 0 for e in EDGES)


def test_neighbouring_documents():
    c = cases(2)["neighbours"]
    k = c.sorted_keys()
    assert (k >> 1).tolist() == [0, 1, 1, 2, 3, 3, 3] and int(c.rules.need[0]) == 2      # entry 0: t < need - 1
    row, rules = c.want()
    assert row.tolist() == [0, 0, 1, 1, 2] and rules.tolist() == [0, 0]


def test_negated_terms_and_need():
    c = cases(2)["negated"]
    a, b, cc = 0, 1, 2
    assert [set(c.states[int(x):int(y)].tolist()) for x, y in zip(c.row[:-1], c.row[1:])] == [{a, b}, {a}, {b}, {a, cc}, {b, cc}, set()]
    row, rules = c.want()
    got = [rules[int(x):int(y)].tolist() for x, y in zip(row[:-1], row[1:])]
    # rule 0 = a and not b; rule 1 = (a or c) and not b; rule 2 = c and not a and not b.  Document 2 holds b alone: runs of
    # negated entries only
    assert got == [[], [0, 1], [], [0, 1], [], []]
    k = c.sorted_keys()
    runs = {}
    for key in k.tolist():
        runs.setdefault(key >> 1, []).append(key & 1)
    assert any(all(v) for v in runs.values()) and any(not any(v) for v in runs.values()) and any(0 in v and 1 in v for v in runs.values())
    n = cases(2)["need"]
    assert n.rules.need.tolist() == [1, 2, 3, 4]
    m = dense(*n.want(), 4)
    assert m.sum(axis=0).tolist() == [15, 11, 5, 1]                 # subsets of four with at least 1, 2, 3, 4 members


def test_fan_out_and_empty_documents():
    c = cases(2)["fan3000"]
    deg = c.rules.degree()
    assert deg[5] == ruleref.FAN > 256 * 8 and deg[9] == 0 and (c.states == 9).sum() >= 2 and (c.states == 5).sum() >= 3
    for run in ruleref.EMPTY_RUNS:
        e = cases(2)[f"empty{run}"]
        runs = e.empty_runs()
        assert len(runs) == 4 and all(ln == run for _, ln in runs)
        assert runs[0][0] == 0 and runs[3][0] + run == e.n_docs
        assert int(e.row[runs[2][0]]) % BLOCK == 0 and 0 < int(e.row[runs[1][0]]) % BLOCK


def test_sort_passes_one_to_five():
    by = cases(2)
    got = {(nr, nd): by[f"passes-r{nr}-d{nd}"].passes for nr in ruleref.PASS_RULES for nd in ruleref.PASS_DOCS}
    assert set(got.values()) == {1, 2, 3, 4, 5}
    assert got[(64, 2)] == 1 and got[(65, 2)] == 2                  # 8 and 9 key bits
    assert got[(2, 2049)] == 2 and got[(2 ** 15 + 1, 1)] == 3       # 14 and 17
    assert got[(2, 524289)] == 3 and got[(64, 524289)] == 4         # 22 and 27
    assert got[(2 ** 15 + 1, 2049)] == 4 and got[(2 ** 15 + 1, 524289)] == 5      # 29 and 37
    for (nr, nd), p in got.items():
        c = by[f"passes-r{nr}-d{nd}"]
        assert c.rules.n_rules == nr and c.n_docs == nd and c.E > 0
    assert sum(by[f"passes-r{nr}-d524289"].E > SORT_BLOCK for nr in ruleref.PASS_RULES) >= 3      # the many-block sort too


# ---------------------------------------------------------------------------
# the checker refuses wrong results

def refused(c, row, rules, words):
    assert not (np.array_equal(row, c.want()[0]) and np.array_equal(rules, c.want()[1])), f"{c.name}: the seeded result is not wrong"
    with pytest.raises(AssertionError, match=words):
        check(c.want(), row, rules, what=c.name)


def test_checker_refuses_a_run_merged_across_a_document_edge():
    c = cases(2)["neighbours"]
    refused(c, *fired(c.row, c.states, c.rules, bug="merge"), "row_ptr|fired rules")


def test_checker_refuses_an_ignored_negation_and_a_need_off_by_one():
    c = cases(2)["negated"]
    refused(c, *fired(c.row, c.states, c.rules, bug="noneg"), "fired rules, want")
    c = cases(2)["need"]
    refused(c, *fired(c.row, c.states, c.rules, bug="need"), "fired rules, want")
    c = cases(2)["random"]
    for bug in ("noneg", "need", "merge"):
        refused(c, *fired(c.row, c.states, c.rules, bug=bug), "fired rules, want|row_ptr")


def test_checker_refuses_unsorted_ids_and_a_short_row_ptr():
    c = cases(2)["allfire"]
    row, rules = (a.copy() for a in c.want())
    rules[[0, 1]] = rules[[1, 0]]
    refused(c, row, rules, "strictly ascend")
    # row_ptr without the first group's sum: the documents whose first key lies past the first 4096 keys
    c = cases(2)["E12293"]
    row, rules = (a.copy() for a in c.want())
    tails, _ = c.firing_tails()
    first_key = np.searchsorted(c.sorted_keys() >> (ruleref.bit_width(c.rules.n_rules - 1) + 1), np.arange(c.n_docs + 1))
    in_group0 = int((tails < GROUP).sum())
    assert in_group0 > 0
    row[first_key >= GROUP] -= np.uint64(in_group0)
    refused(c, row, rules, "row_ptr")


# ---------------------------------------------------------------------------
# PfacTable.rule_table

PATTERNS = b"he\nshe\nhers\nhis\n"                              # ids 1, 2, 3, 4


def state_of(table):
    return {int(i): s for s, i in enumerate(table.idmap)}


def test_rule_table_maps_pattern_ids_to_states():
    t = PfacTable.from_bytes(PATTERNS, 256)
    s = state_of(t)
    ptr, terms, need = t.rule_table([[1, 2], {"any_of": [3, 4, 1]}, {"all_of": [1, 2, 3], "need": 2, "none_of": [4]},
                                     ([s[1]], [s[2], s[3]], 1), {"all_of": (2,), "none_of": (1,)}])
    assert ptr.dtype == np.uint64 and terms.dtype == np.uint32 and need.dtype == np.uint32
    assert ptr.tolist() == [0, 2, 5, 9, 12, 14] and need.tolist() == [2, 1, 2, 1, 1]
    rules = Rules.from_arrays(ptr, terms, need, t.num_final).as_sets()
    assert rules == [({s[1], s[2]}, set(), 2), ({s[3], s[4], s[1]}, set(), 1), ({s[1], s[2], s[3]}, {s[4]}, 2),
                     ({s[1]}, {s[2], s[3]}, 1), ({s[2]}, {s[1]}, 1)]
    for r in range(5):                                          # positives in front, both halves ascending
        mine = terms[int(ptr[r]):int(ptr[r + 1])].astype(np.int64)
        assert (np.diff(mine) > 0).all() and (mine[mine >= PFAC_RULE_NOT] - PFAC_RULE_NOT < t.num_final).all()
    assert [a.size for a in t.rule_table([])] == [1, 0, 0]


def test_rule_table_refuses():
    t = PfacTable.from_bytes(PATTERNS, 256)
    s = state_of(t)
    with pytest.raises(ValueError, match="pattern id 2"):
        t.rule_table([{"all_of": [1, 2], "none_of": [2]}])       # negated and positive
    with pytest.raises(ValueError, match="need 3"):
        t.rule_table([{"all_of": [1, 2], "need": 3}])
    with pytest.raises(ValueError, match="need 0"):
        t.rule_table([{"any_of": [1, 2], "need": 0}])
    with pytest.raises(ValueError, match="pattern id 5"):
        t.rule_table([[1, 5]])
    with pytest.raises(ValueError, match="positive term"):
        t.rule_table([{"all_of": [], "none_of": [1]}])
    with pytest.raises(ValueError, match="state 99"):
        t.rule_table([([99], [], 1)])
    with pytest.raises(ValueError, match=f"state {s[1]}"):
        t.rule_table([([s[1]], [s[1]], 1)])
    dup = PfacTable.from_bytes(b"abc\nab\nabc\n", 256)          # of identical lines the last one wins
    assert [a.tolist() for a in dup.rule_table([[3, 2]])][2] == [2]
    with pytest.raises(ValueError, match="pattern id 1 lost to a duplicate"):
        dup.rule_table([[1, 2]])
    folded = PfacTable.from_bytes(b"He\nhe\nshe\n", 256, ignore_case=True)     # "He" and "he" are one line once folded
    with pytest.raises(ValueError, match="pattern id 1 lost to a duplicate"):
        folded.rule_table([[1, 3]])


def test_rule_table_of_a_class_table():
    t = PfacTable.from_charclass(b"ac\n[a]c\nad\n[ab]d\n", 256)
    by = t._states_of_patterns()
    assert by[1] == by[2] and len(by[1]) == 1 and len(by[4]) == 2       # two ids on one state; a pattern in two states
    ptr, terms, need = t.rule_table([[1, 2], {"any_of": [2, 1], "need": 1}])
    assert ptr.tolist() == [0, 1, 2] and terms.tolist() == [by[1][0]] * 2 and need.tolist() == [1, 1]    # merged; need counts states
    with pytest.raises(ValueError, match="need 2"):
        t.rule_table([{"all_of": [1, 2], "need": 2}])
    with pytest.raises(ValueError, match="pattern id 4 ends in several"):
        t.rule_table([[1, 4]])


def test_from_docs_and_rules_reject_malformed_input():
    with pytest.raises(AssertionError):
        Rules([([1], [1], 1)], 16)
    with pytest.raises(AssertionError):
        Rules([([1, 2], [], 3)], 16)
    c = from_docs("x", 2, [[3, 1, 3], []], Rules([([1, 3], [], 2)], 16))
    assert c.states.tolist() == [1, 3] and c.want()[1].tolist() == [0]
