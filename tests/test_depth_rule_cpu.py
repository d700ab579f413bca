"""The numpy model of the depth rule (tests/depth_rule_cases.py) against the reference's own find_most_likely_depth, recorded over its
whole domain (tests/golden/depth_rule.npz), and what the recorded cases can tell apart: each plausible mistake of a kernel -- in the
rule's float / double steps or in the integer rules around it -- must change at least one cell of at least one case, or stand in
INDISTINGUISHABLE by name.  tests/test_gpu_depth_rule.py holds the device kernels to this model."""
import functools

import numpy as np
import pytest

import depth_rule_cases as D

# mutants that no average and no interval can expose (none: c / upper in float is exposed by the case ave12.0_5_19next)
INDISTINGUISHABLE = ()


@functools.lru_cache(maxsize=None)
def _rows():
    return D.rows()


def test_the_recorded_cases_are_the_listed_ones_with_the_reference_s_own_intervals():
    g = D.golden()
    assert list(g) == D.CASE_NAMES
    for name, ave, interval in D.CASES:
        got_ave, lower, upper, table = g[name]
        assert got_ave.view(np.uint32) == np.float32(ave).view(np.uint32), name
        assert table.shape == (D.H_MAX + 1, D.N_C, D.N_F) and table.dtype == np.uint8
        assert (lower, upper) == (tuple(interval) if interval is not None else D.poisson_interval(ave)), (name, lower, upper)
    _, lower, upper, _ = g["ave23.5_14_33"]
    assert (lower, upper) == (14.0, 33.0)
    _, lower, upper, _ = g["ave23.5"]
    assert 13 < lower < 14 and 33 < upper < 34      # the integer interval of ave = 23.5 is the explicit case's


def test_model_equals_the_reference_in_every_cell_of_every_case():
    for name, (ave, lower, upper, table) in D.golden().items():
        model = D.depth_table(ave, upper)
        bad = np.argwhere(model != table)
        assert bad.size == 0, (name, len(bad), [(int(h), int(c), int(f) + 1, int(model[h, c, f]), int(table[h, c, f])) for h, c, f in bad[:5]])


def test_every_mutant_of_the_depth_rule_differs_from_the_model_somewhere():
    """cells of the (h, c, f) table, per case"""
    g = D.golden()
    model = {name: D.depth_table(ave, upper) for name, (ave, _, upper, _) in g.items()}
    print()
    for mutant in D.TABLE_MUTANTS:
        counts = {name: int(np.count_nonzero(D.depth_table(ave, upper, mutant) != model[name])) for name, (ave, _, upper, _) in g.items()}
        print(f"depth rule mutant {mutant}: differing cells per case {counts}, in all {sum(counts.values())}")
        if mutant in INDISTINGUISHABLE:
            assert sum(counts.values()) == 0, (mutant, "is told apart after all: take it off the list")
        else:
            assert sum(counts.values()) > 0, mutant


def test_every_mutant_of_the_rules_around_it_differs_from_the_model_somewhere():
    """rows of the device test at ploidy 2 whose picked terms or flag byte change, per case"""
    g, r = D.golden(), _rows()
    model = {name: D.expected(r, 2, table, lower, upper) for name, (_, lower, upper, table) in g.items()}
    print()
    for mutant in D.RULE_MUTANTS:
        counts = {}
        for name, (ave, lower, upper, table) in g.items():
            idx, kept, flags = model[name]
            m_idx, m_kept, m_flags = D.expected(r, 2, table, lower, upper, mutant)
            counts[name] = int(np.count_nonzero((idx != m_idx).any(axis=1) | (flags != m_flags) | (kept != m_kept)))
        print(f"rule mutant {mutant}: differing rows per case {counts}, in all {sum(counts.values())}")
        if mutant in INDISTINGUISHABLE:
            assert sum(counts.values()) == 0, (mutant, "is told apart after all: take it off the list")
        else:
            assert sum(counts.values()) > 0, mutant


def test_indistinguishable_mutants_are_mutants():
    assert set(INDISTINGUISHABLE) <= set(D.TABLE_MUTANTS) | set(D.RULE_MUTANTS)


@pytest.mark.parametrize("ploidy", sorted({f.ploidy for f in D.FAMILIES}))
def test_the_rows_pick_every_term_the_rule_can_name(ploidy):
    """per case and per h 0 .. ploidy: every h * 256 + cc the recorded table holds at that h is picked by some genotype of some row, and
    nothing else is"""
    r, total = _rows(), 0
    for name, (ave, lower, upper, table) in D.golden().items():
        idx, _, _ = D.expected(r, ploidy, table, lower, upper)
        picked = np.unique(idx)
        assert picked.min() >= 0 and picked.max() < 256 * (ploidy + 1)
        for h in range(ploidy + 1):
            can = np.unique(table[h]).astype(np.int64) + 256 * h
            got = picked[(picked >> 8) == h]
            assert np.array_equal(got, can), (name, h, np.setxor1d(got, can)[:8].tolist())
        total += picked.size
    print(f"\nploidy {ploidy}: {total} distinct (case, h, cc) terms picked, every one the tables hold")


def test_rows_are_the_whole_domain_once():
    r = _rows()
    key = ((r.carrier.astype(np.int64) * 2 + r.flag) * 256 + r.c) * 256 + r.f
    assert r.c.size == D.N_ROWS == 261120 and np.unique(key).size == D.N_ROWS and r.f.min() == 1 and r.f.max() == 255
    fam = D.FAMILIES[0]
    x = D.family_inputs(fam, r)
    bit = lambda i: (x["words"] >> np.uint64(16 + i)) & np.uint64(1)
    assert np.array_equal(bit(fam.id0), 1 - r.carrier) and np.array_equal(bit(fam.id_off), r.carrier) and np.array_equal(bit(47), r.flag)
    assert np.array_equal((x["words"] >> np.uint64(8)) & np.uint64(0xFF), r.f) and not bit(fam.id1).any()
