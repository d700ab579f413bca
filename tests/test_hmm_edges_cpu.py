"""The constructed rows of hmm_edge_rows.py discriminate, shown without a GPU.  The numpy model with the recursion kernels' skip rules
written in (true x87 sums, terms left out at the kernels' thresholds) equals the plain model on every constructed row; a rule that cuts
one binade too early does not.  test_gpu_hmm_edges.py holds the kernels to the plain model on the same rows.

Every threshold is tight.  In the term loop `+ 1` for `+ 2` and `> 63` for `> 64` each must differ on the rows whose product is a denormal
that rounds up a binade (its exponent is the operands' sum + 2); rows with a normal product cannot tell those two (their products lie at
most one above the sum) and catch the next cut, `+ 0` or both at once.  In the total loop `> 63` must differ."""
import numpy as np
import pytest

import hmm_edge_rows as er

LD = np.longdouble
BUILDERS = {"term": er.term_rule_rows, "denormal_product": er.denormal_product_rows, "total": er.total_rule_rows, "denormal": er.denormal_rows}


@pytest.fixture(scope="module")
def built():
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    out = {}
    for name, make in BUILDERS.items():
        rows = make(5)
        out[name] = (rows, rows.model())
    return out


def _differing_steps(rows, plain, **rules):
    return np.flatnonzero((rows.model(**rules) != plain).any(axis=1))


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_the_kernels_rules_leave_every_constructed_row_as_x87_has_it(built, name):
    rows, plain = built[name]
    assert _differing_steps(rows, plain, term_rule=(2, 64), total_rule=64).size == 0
    assert np.isfinite(plain.astype(np.float64)).all()


def test_the_rows_reach_what_they_are_for(built):
    rows, plain = built["denormal"]
    keep, obs, row, restart, pows, uniform, chains = rows.arrays()
    tiny = np.finfo(LD).tiny
    assert ((obs > 0) & (obs < tiny)).all(axis=1).any()                     # a whole row of denormal scores
    fallback = [s for s in range(len(row)) if not restart[s] and (plain[s] == uniform).all() and (obs[row[s]] > 0).all()]
    assert fallback                                                         # non-zero scores, zero total, on a continuing step
    rows, plain = built["term"]
    assert (plain[1::2, 3] > 0).all() and (plain[1::2, 4] > 0).all()


def _last_bit(x):
    return int.from_bytes(LD(x).tobytes()[:8], "little") & 1


@pytest.mark.parametrize("rule", [(1, 64), (2, 63)])
def test_a_bound_or_a_cut_one_binade_too_eager_shows_on_a_denormal_product(built, rule):
    """+ 1 for + 2, > 63 for > 64: a denormal product two binades above the operands' sum, half an ulp of the running sum or just above"""
    rows, plain = built["denormal_product"]
    steps = _differing_steps(rows, plain, term_rule=rule)
    assert steps.size > 0
    assert {rows.what[s][4] for s in steps} == {64}                              # only at the threshold
    assert {rows.what[s][5] for s in steps} == set(er.DENORMAL_SUMS)             # at every exponent sum tried
    assert {rows.what[s][1] for s in steps} == {er.ALL, er.ALL - 1}
    # the running sum of lane 3 before the probe (leading term + 63-binades term) has an odd last bit in some caught rows and an even one in others
    keep, obs, row, restart, pows, uniform, chains = rows.arrays()
    bits = set()
    for s in steps:
        score = obs[row[s]][3]
        bits.add(_last_bit((LD(0.5) * pows[s, 0, 0]) * score + (LD(0.25) * pows[s, 0, 1]) * score))
    assert bits == {0, 1}


@pytest.mark.parametrize("rule", [(1, 63), (0, 64)])
def test_a_term_cut_one_binade_too_early_shows(built, rule):
    rows, plain = built["term"]
    steps = _differing_steps(rows, plain, term_rule=rule)
    assert steps.size > 0
    caught = {rows.what[s][1] for s in steps}
    assert er.ALL - 1 in caught or (3 << 62) in caught, caught      # the product one binade above the operands' exponents: where the bound bites
    assert {rows.what[s][4] for s in steps} <= {64, 65}              # and only next to the threshold
    assert {rows.what[s][2] & 1 for s in steps} == {0, 1} or {rows.what[s][3] for s in steps} == {True, False}   # sums of either last bit


def test_a_total_cut_one_binade_too_early_shows(built):
    rows, plain = built["total"]
    assert _differing_steps(rows, plain, total_rule=63).size > 0
    assert _differing_steps(rows, plain, total_rule=65).size == 0
