"""Proximity rules without a GPU: the two references of tests/nearref.py held against one another on every case of
tests/test_gpu_near.py, the preconditions that make the named cases test what they are named for, the condition on the
seeded cases (few of them all-zero or all-ones), and the Python side of a rule (near_rule, the dtype, the symbols)."""
import numpy as np
import pytest

import nearref
from nearref import ALL, BLOCK, NAMES, N_SEEDS, case, near_brute, near_masks
from phfpfac_amd import NEAR_RULE_DTYPE, PFAC_NEAR_ANY_DIST, PFAC_NEAR_ORDERED, _ffi, near_rule


def test_the_names_are_the_cases():
    assert tuple(nearref.by_name()) == NAMES and len(set(ALL)) == len(NAMES) + N_SEEDS


@pytest.mark.parametrize("name", ALL)
def test_the_two_references_agree(name):
    c = case(name)
    a, b = c.want(), near_brute(c.states, c.pos, c.first, c.rules)
    assert a.dtype == b.dtype == np.uint64 and a.size == b.size == c.n_docs
    nearref.check(a, b, what=name)
    assert c.rules.size == 64 or int(a.max(initial=0)) >> c.rules.size == 0


@pytest.mark.parametrize("name", NAMES)
def test_preconditions(name):
    c = case(name)
    c.precondition()
    w = c.want()
    bits = int(c.n_docs * c.rules.size)
    set_ = sum(bin(int(m)).count("1") for m in w)
    if c.fires:                                                 # a bit set and a bit clear: neither a kernel that writes nothing
        assert 0 < set_ < bits, f"{set_} of {bits} bits"        # nor one that fires everywhere passes
    else:
        assert set_ == 0


def test_the_named_cases_cover_the_kernels_edges():
    sizes = {n: case(n).n for n in NAMES}
    assert max(sizes.values()) == 3 * BLOCK and sizes["no-records"] == 0
    assert any(BLOCK < s < 2 * BLOCK for s in sizes.values())
    assert case("rules-0").rules.size == 0 and case("rules-1").rules.size == 1 and case("rules-64").rules.size == 64
    assert np.array_equal(case("rules-64").want() >> np.uint64(63), case("rules-1").want())     # the same rule, as bit 63 and as bit 0


def test_few_seeded_cases_are_all_zero_or_all_ones():
    """A condition on the inputs, judged with the brute-force reference: at most one case in eight is trivial."""
    trivial, blocks = 0, 0
    for s in range(N_SEEDS):
        c = case(f"seed{s}")
        w = near_brute(c.states, c.pos, c.first, c.rules)
        full = np.uint64((1 << c.rules.size) - 1)
        trivial += bool((w == 0).all() or (w == full).all())
        blocks += c.n > BLOCK
    assert trivial * 8 <= N_SEEDS, f"{trivial} of {N_SEEDS} seeded cases are all zero or all ones"
    assert blocks >= 2, "some seeded cases lie across a block edge"


def test_the_references_refuse_what_they_must():
    c = case("distance-exact")
    pos = c.pos.copy()
    pos[1] = 50                                                 # a position that decreases inside a document
    with pytest.raises(AssertionError, match="decreases"):
        near_masks(c.states, pos, c.first, c.rules)
    with pytest.raises(AssertionError):
        nearref.check(c.want(), c.want()[::-1].copy())


def test_near_rule_and_the_bindings():
    assert NEAR_RULE_DTYPE == nearref.RULE and NEAR_RULE_DTYPE.itemsize == 32
    r = near_rule(0, [1, 63], 60, ordered=True)
    assert r.dtype == NEAR_RULE_DTYPE and r.shape == ()
    assert (int(r["a_groups"]), int(r["b_groups"]), int(r["max_dist"]), int(r["flags"]), int(r["reserved"])) == (1, 2 | 1 << 63, 60, PFAC_NEAR_ORDERED, 0)
    r = near_rule(np.uint64(5), 2)
    assert (int(r["a_groups"]), int(r["b_groups"]), int(r["max_dist"]), int(r["flags"])) == (5, 4, PFAC_NEAR_ANY_DIST, 0)
    assert r.tobytes() == nearref.rule(5, 4, nearref.ANY_DIST).tobytes()
    for bad in (lambda: near_rule(64, 0, 1), lambda: near_rule(0, -1, 1), lambda: near_rule(0, 1, -1), lambda: near_rule(0, 1, 2 ** 32)):
        with pytest.raises(ValueError):
            bad()
    assert {"pfac_documents_near", "pfac_near_masks_d2h", "pfac_slot_near_masks"} <= set(_ffi.HIP_SYMBOLS)
    assert (nearref.ORDERED, nearref.ANY_DIST, nearref.MAX_RULES) == (_ffi.PFAC_NEAR_ORDERED, _ffi.PFAC_NEAR_ANY_DIST, _ffi.PFAC_NEAR_MAX_RULES)
    from phfpfac_amd.matcher import _near_rules
    arr = _near_rules([near_rule(0, 1, 3), near_rule(1, 0, None, True)])
    assert arr.dtype == NEAR_RULE_DTYPE and arr.shape == (2,) and arr.flags.c_contiguous
    assert arr.tobytes() == nearref.rules_array([nearref.rule(1, 2, 3), nearref.rule(2, 1, nearref.ANY_DIST, True)]).tobytes()
    assert _near_rules([]).size == 0 and _near_rules(arr) is not None
