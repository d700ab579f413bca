"""The `-m rec` recursion kernels and the posterior kernels (vgmi_hmm.hip) where their layouts change and on operands the random rows of
test_gpu_hmm.py never contain, against the same computations in x87 long double (_host_chain, _host_posterior), bit for bit.

  sizes      n_gt = 1 .. 128 under two and four wavefronts (a lane per genotype), 129 (the kernel switches), 256 / 257 (a lane's stride in
             the big kernel), 512 / 513 and 1 024 / 1 025 (genotypes per lane change), 2 048 (VGMI_HMM_MAX_GT); the last genotype carries
             weight in every row, so a lane or slot that is dropped shows
  operands   the constructed rows of hmm_edge_rows.py: terms and entries 60 to 70 binades below a sum with either last bit (the two skip
             rules at their thresholds; the term's product normal, and a denormal that rounds up a binade), rows of denormal scores, totals
             at the border of the normal range, products that all underflow;
             test_hmm_edges_cpu.py shows without a GPU that a rule one binade too eager changes these rows
  ties       equal posteriors and equal sums of genotype strings: the first in string order and the first entry win"""
import functools

import numpy as np
import pytest

import hmm_edge_rows as er
from test_gpu_hmm import _host_chain, _host_posterior
from varigraph_amd import vgmi

pytestmark = pytest.mark.gpu
LD = np.longdouble


# ---- sizes ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _size_case(n, ploidy):
    """inputs of Context.hmm_calls and what x87 makes of them, computed once per size (the wavefront count does not enter)"""
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    rng = np.random.default_rng(n * 10 + ploidy)
    n_windows, per_window = 2, (5 if n <= 1024 else 3)          # (the numpy model is O(rows n) vector operations: fewer rows, not fewer sizes)
    keep = rng.integers(0, ploidy + 1, size=(n_windows, n, n), dtype=np.uint8)
    keep = np.triu(keep) + np.triu(keep, 1).transpose(0, 2, 1)              # any symmetric one
    idx = np.arange(n)
    keep[:, idx, idx] = rng.integers(1, ploidy + 1, size=(n_windows, n), dtype=np.uint8)
    n_rows = n_windows * per_window
    expo = rng.choice([0, -20, -300, -2000, -4800, -4940, -4960], size=(n_rows, n), p=[.15, .2, .25, .2, .1, .05, .05])
    obs = (rng.random((n_rows, n)).astype(LD) + LD(0.01)) * np.power(LD(10), expo.astype(LD))
    obs[rng.random((n_rows, n)) < 0.02] = 0
    obs[:, n - 1] = rng.random(n_rows).astype(LD) + LD(0.01)               # the last genotype carries weight in every row
    obs[3] = 0                                                               # but one: the uniform fallback
    row, restart, pows, chains = [], [], [], []
    fwd = np.zeros(n_rows, dtype=np.uint64)
    bwd = np.zeros(n_rows, dtype=np.uint64)
    for w in range(n_windows):
        for direction in (1, -1):
            rows = list(range(w * per_window, (w + 1) * per_window))[::direction]
            first = len(row)
            for i, r in enumerate(rows):
                (fwd if direction == 1 else bwd)[r] = len(row)
                row.append(r)
                restart.append(1 if i == 0 or (i == per_window // 2 and w == 1 and direction == 1) else 0)     # one restart in mid-chain
                d = LD(rng.integers(1, 50_000))
                recomb = (LD(1) - np.exp(-d / LD(30))) * (LD(1) / LD(30))
                no_recomb = np.exp(-d / LD(30)) + recomb
                pows.append([[no_recomb ** LD(k) for k in range(ploidy + 1)], [recomb ** LD(k) for k in range(ploidy + 1)]])
            chains.append((first, len(rows), w))
    pows = np.array(pows, dtype=LD)
    uniform = LD(1) / LD(n)
    n_ids = min(n, 128) if n <= 128 else min(n, 255)
    gid = (rng.permutation(n) % n_ids).astype(np.uint8).reshape(1, n).repeat(n_rows, axis=0)
    for r in range(n_rows):
        gid[r] = np.roll(gid[r], r)
    order = np.full((n_rows, n), 0xFF, dtype=np.uint8)
    order[:, :n_ids] = np.arange(n_ids)[::-1] if n_ids < 3 else np.roll(np.arange(n_ids)[::-1], 1)      # not the identity
    assert n == 1 or not np.array_equal(order[0, :n_ids], np.arange(n_ids))
    want_ab = np.zeros((len(row), n), dtype=LD)
    for first, count, w in chains:
        want_ab[first:first + count] = _host_chain(keep[w], [obs[r] for r in row[first:first + count]], restart[first:first + count],
                                                   pows[first:first + count], uniform, ploidy)
    want_post = [_host_posterior(want_ab[fwd[r]], want_ab[bwd[r]], gid[r], order[r]) for r in range(n_rows)]
    for a in (keep, obs, pows, gid, order, fwd, bwd, want_ab):
        a.setflags(write=False)
    return (keep, obs, row, restart, pows, uniform, chains, ploidy, gid, order, fwd, bwd), want_ab, want_post


def _check_size(n, ploidy):
    args, want_ab, want_post = _size_case(n, ploidy)
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        prob, winner, ab = ctx.hmm_calls(*args)
    finally:
        ctx.close()
    assert np.array_equal(ab, want_ab), (n, ploidy, int(np.argmax((ab != want_ab).any(axis=1))), np.flatnonzero((ab != want_ab).any(axis=0))[:8])
    assert (ab[:, n - 1] > 0).all()
    n_called = 0
    for r, (best, win) in enumerate(want_post):
        if best is None:
            assert winner[r] == 0xFFFFFFFF, r
            continue
        assert winner[r] == win and prob[r] == best, r
        n_called += 1
    assert n_called >= len(want_post) - 2


@pytest.mark.parametrize("waves", [2, 4])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128])
def test_a_lane_per_genotype_at_the_edges_of_its_wavefronts(n, waves, monkeypatch):
    monkeypatch.setenv("VGMI_HMM_WAVES", str(waves))
    _check_size(n, 2)


@pytest.mark.parametrize("n", [129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048])
def test_several_genotypes_per_lane_at_the_edges_of_their_layouts(n):
    _check_size(n, 2)


@pytest.mark.parametrize("ploidy", [1, 4])
@pytest.mark.parametrize("n,waves", [(128, 2), (128, 4), (129, None), (2048, None)])
def test_the_kernels_switch_and_the_largest_list_at_other_ploidies(n, waves, ploidy, monkeypatch):
    if waves:
        monkeypatch.setenv("VGMI_HMM_WAVES", str(waves))
    _check_size(n, ploidy)


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operand_case(name, n):
    rows = {"term": er.term_rule_rows, "denormal_product": er.denormal_product_rows, "total": er.total_rule_rows, "denormal": er.denormal_rows}[name](n)
    keep, obs, row, restart, pows, uniform, chains = rows.arrays()
    want = np.zeros((len(row), n), dtype=LD)
    for first, count, w in chains:
        want[first:first + count] = _host_chain(keep[w], [obs[r] for r in row[first:first + count]], restart[first:first + count],
                                                pows[first:first + count], uniform, rows.ploidy)
    assert np.array_equal(want, rows.model())        # the model test_hmm_edges_cpu.py mutates is the one the kernels are held to
    return rows, want


@pytest.mark.parametrize("name", ["term", "denormal_product", "total", "denormal"])
@pytest.mark.parametrize("n,waves", [(5, 2), (5, 4), (130, None)])
def test_constructed_operands_equal_x87(name, n, waves, monkeypatch):
    """(5, waves): the lane kernel under two and four wavefronts; 130: the same rows as the first genotypes of a list for the big kernel"""
    if waves:
        monkeypatch.setenv("VGMI_HMM_WAVES", str(waves))
    rows, want = _operand_case(name, n)
    keep, obs, row, restart, pows, uniform, chains = rows.arrays()
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        got = ctx.hmm_recursion(keep, obs, row, restart, pows, uniform, chains, rows.ploidy)
    finally:
        ctx.close()
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (name, n, waves, bad[:5], [rows.what[s] for s in bad[:5]])


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------
def _tie_case(n):
    """-> (arguments of hmm_calls, {name: row})"""
    ploidy = 2
    keep = np.ones((2, n, n), dtype=np.uint8)
    keep[1] = 2 * np.eye(n, dtype=np.uint8)          # window 1: a genotype follows itself only (the tables below: nothing moves)
    names, obs, gids, orders = {}, [], [], []

    def add(name, scores, gid, order):
        o = np.zeros(n, dtype=LD)
        o[:len(scores)] = scores
        g = np.full(n, gid[-1], dtype=np.uint8)
        g[:len(gid)] = gid
        od = np.full(n, 0xFF, dtype=np.uint8)
        od[:len(order)] = order
        names[name] = len(obs)
        obs.append(o)
        gids.append(g)
        orders.append(od)

    s = [LD(x) / LD(16) for x in range(17)]
    generic = (np.arange(n) % 7 + 1).astype(LD)
    add("generic", generic, [g % 4 for g in range(n)] if n >= 4 else [0] * n, [1, 3, 0, 2] if n >= 4 else [0])
    if n >= 6:
        # strings 3 and 1 hold the same posteriors in the same entry order; 3 stands before 1 in `order`: neither the lower id nor the later one
        add("two_strings", [s[5], s[5], s[3], s[3], s[1], s[2]], [3, 1, 3, 1, 0, 2], [2, 3, 1, 0])
        # the winning string 2 has its largest posterior twice (entries 2 and 4) after a smaller one: the first of the two
        add("inside_string", [s[4], s[2], s[6], s[1], s[6], s[1]], [0, 2, 2, 1, 2, 1], [1, 0, 2])
        # string 4 has nothing but zeros and stands first
        add("zero_string_first", [0, s[3], 0, s[5], s[2], 0], [4, 0, 4, 1, 0, 4], [4, 1, 0])
    add("all_equal", [s[2]] * n, [g % 3 for g in range(n)] if n >= 3 else [0] * n, [2, 0, 1] if n >= 3 else [0])
    # a denormal denominator (window 1): alpha has its weight on entry 0, beta on entry 1, every product is a denormal
    tiny, mid = er.ld(er.ONE, -16400), er.ld(er.ONE, -8200)
    if n >= 2:
        add("alpha", [LD(1), tiny] + [mid] * (n - 2), [0] * n, [0])
        add("beta", [tiny, LD(1)] + [mid] * (n - 2), [0] * n, [0])
        add("denormal_denominator", [LD(1)] * n, [g % 2 for g in range(n)], [1, 0])
    obs, gid, order = np.array(obs, dtype=LD), np.array(gids), np.array(orders)
    n_rows = len(obs)
    row, restart, chains = [], [], []
    fwd = np.zeros(n_rows, dtype=np.uint64)
    bwd = np.zeros(n_rows, dtype=np.uint64)
    plain = [r for name, r in names.items() if name not in ("alpha", "beta", "denormal_denominator")]
    for direction, where in ((1, fwd), (-1, bwd)):          # window 0: the generic row, then the tie rows, forward and backward
        rows = [plain[0]] + plain[1:][::direction]
        chains.append((len(row), len(rows), 0))
        for i, r in enumerate(rows):
            where[r] = len(row)
            row.append(r)
            restart.append(1 if i == 0 else 0)
    if n >= 2:
        for first_row, where in ((names["alpha"], fwd), (names["beta"], bwd)):
            chains.append((len(row), 2, 1))
            fwd[first_row] = bwd[first_row] = len(row)
            where[names["denormal_denominator"]] = len(row) + 1
            row += [first_row, names["denormal_denominator"]]
            restart += [1, 0]
    pows = np.zeros((len(row), 2, ploidy + 1), dtype=LD)
    pows[:, 0] = [LD(0), LD(0), LD(1)]          # keep_pow: all of a genotype's weight stays (window 1), a constant sum (window 0: k = 1 ...)
    pows[:, 1] = LD(1)
    pows[:, 0, 1] = LD(1) / LD(3)               # ... times a third
    return (keep, obs, row, restart, pows, LD(1) / LD(n), chains, ploidy, gid, order, fwd, bwd), names


@pytest.mark.parametrize("n", [1, 12, 128, 130])
def test_posterior_ties_go_to_the_first_string_and_the_first_entry(n):
    """n up to 128: hmm_posterior_kernel; 130: hmm_posterior_big_kernel"""
    args, names = _tie_case(n)
    keep, obs, row, restart, pows, uniform, chains, ploidy, gid, order, fwd, bwd = args
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        prob, winner, ab = ctx.hmm_calls(*args)
    finally:
        ctx.close()
    for first, count, w in chains:
        want = _host_chain(keep[w], [obs[r] for r in row[first:first + count]], restart[first:first + count], pows[first:first + count], uniform, ploidy)
        assert np.array_equal(ab[first:first + count], want), (n, first)
    for name, r in names.items():
        best, win = _host_posterior(ab[fwd[r]], ab[bwd[r]], gid[r], order[r])
        assert best is not None and winner[r] == win and prob[r] == best, (n, name, winner[r], win)
    post = {name: ab[fwd[r]] * ab[bwd[r]] for name, r in names.items()}
    if n >= 6:
        p = post["two_strings"]
        r = names["two_strings"]
        assert p[0] == p[1] and p[2] == p[3] and winner[r] == 0        # string 3's first entry, not string 1's:
        assert gid[r, 0] == 3 and gid[r, 1] == 1 and list(order[r]).index(3) < list(order[r]).index(1)     # the higher id, the earlier in order
        p = post["inside_string"]
        assert p[2] == p[4] > p[1] and winner[names["inside_string"]] == 2
        assert winner[names["zero_string_first"]] == 3 and gid[names["zero_string_first"], 3] == 1
    assert (post["all_equal"] == post["all_equal"][0]).all()
    if n == 12:         # three strings of four entries each: three equal sums, and string 2 stands first
        assert winner[names["all_equal"]] == 2
    if n >= 2:
        p = post["denormal_denominator"]
        den = LD(0)
        for x in p:
            den = den + x
        assert 0 < den < np.finfo(LD).tiny and (p > 0).all()
    if n == 1:
        assert winner[names["all_equal"]] == 0 and prob[names["all_equal"]] == 1
