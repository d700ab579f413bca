"""The HMM on the device for samples of ploidy 5 to 8 under `-m rec`: the recursion (strides 6 to 9 of both kernels), the emission scores
of the whole panel and with a genotype list per window (term tables of (ploidy + 1) x 256 entries, copy numbers summed over `ploidy`
places), the refusals at ploidy 0 and 9, and the command line against the deterministic build of the reference.  The kernels against the
same computations spelled out in numpy.longdouble (the x87 format), bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

from varigraph_amd import vgmi
from test_gpu_hmm import _host_chain, _keep_matrix
from test_gpu_hmm_select import AVE, LD, LOWER, UPPER, _mld, _panel
from test_gpu_hmm_select_ploidy import _blocks, _model

pytestmark = pytest.mark.gpu

PLOIDIES = [5, 6, 7, 8]


# ---- the recursion ------------------------------------------------------------------------------------------------------------------------
def _recursion_case(rng, ploidy, n):
    """n genotypes of `ploidy` haplotypes out of 12 -- the first all haplotype 0, the second haplotypes 1 .. ploidy, so that the keep matrix
    holds 0 and `ploidy` -- one window, 12 rows walked forward and backward with a restart in the middle, scores over 300 decades, row 3
    all zero (the uniform fallback)."""
    n_hap, n_rows = 12, 12
    genotypes = [(0,) * ploidy, tuple(range(1, ploidy + 1))][:n]
    while len(genotypes) < n:
        genotypes.append(tuple(sorted(int(x) for x in rng.integers(0, n_hap, size=ploidy))))
    keep = _keep_matrix(genotypes, n_hap + 1)[None]
    assert np.array_equal(keep[0], keep[0].T) and (keep == ploidy).any() and (n == 1 or (keep == 0).any())
    obs = (rng.random((n_rows, n)).astype(LD) + LD(0.01)) * np.power(LD(10), rng.integers(-300, 1, size=(n_rows, n)).astype(LD))
    obs[rng.random((n_rows, n)) < 0.03] = 0
    obs[3] = 0
    row, restart, pows, chains = [], [], [], []
    for direction in (1, -1):
        first = len(row)
        for i, r in enumerate(range(n_rows)[::direction]):
            row.append(r)
            restart.append(1 if i in (0, 6) else 0)
            d = LD(rng.integers(1, 50_000))
            recomb = (LD(1) - np.exp(-d / LD(30))) * (LD(1) / LD(30))
            no_recomb = np.exp(-d / LD(30)) + recomb
            pows.append([[no_recomb ** LD(k) for k in range(ploidy + 1)], [recomb ** LD(k) for k in range(ploidy + 1)]])
        chains.append((first, n_rows, 0))
    return keep, obs, row, restart, np.array(pows, dtype=LD), LD(1) / LD(n), chains


def _check_recursion(got, keep, obs, row, restart, pows, uniform, chains, ploidy):
    for first, count, w in chains:
        want = _host_chain(keep[w], [obs[r] for r in row[first:first + count]], restart[first:first + count], pows[first:first + count], uniform, ploidy)
        g = got[first:first + count]
        assert np.array_equal(g, want), (ploidy, keep.shape[1], int(np.argmax((g != want).any(axis=1))))
    at = row.index(3)      # the all-zero node: 1 / n for everyone
    assert (got[at] == uniform).all()
    assert (got > 0).any()


@pytest.mark.parametrize("waves", [2, 4])
@pytest.mark.parametrize("ploidy", PLOIDIES)
def test_recursion_of_ploidy_5_to_8_equals_x87(ploidy, waves, monkeypatch):
    """hmm_recursion_kernel<6 .. 9, waves> with 1, 3, 16, 65 and 128 genotypes (one lane, part of a wavefront, more than one wavefront, the
    full width): two chains of 12 steps each."""
    monkeypatch.setenv("VGMI_HMM_WAVES", str(waves))
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        for n in (1, 3, 16, 65, 128):
            case = _recursion_case(np.random.default_rng(1000 * ploidy + n), ploidy, n)
            got = ctx.hmm_recursion(*case, ploidy)
            _check_recursion(got, *case, ploidy)
    finally:
        ctx.close()


def test_recursion_of_ploidy_8_beyond_128_genotypes_equals_x87():
    """hmm_recursion_big_kernel<9, 2>: 129 genotypes of eight haplotypes."""
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    case = _recursion_case(np.random.default_rng(8129), 8, 129)
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        got = ctx.hmm_recursion(*case, 8)
    finally:
        ctx.close()
    _check_recursion(got, *case, 8)


# ---- emission scores of the whole panel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ploidy", PLOIDIES)
def test_emission_scores_of_the_whole_panel_for_ploidy_5_to_8(ploidy):
    """vgmi_hmm_emissions_ploidy over 16 used haplotypes (the reference and 15 more): the genotypes are the all-zero block and the blocks of
    `ploidy` consecutive haplotypes, the last one truncated (haplotype 0 stands in the places beyond the panel; 15 is a multiple of 5, so
    ploidy 5 gets a truncated block by hand).
    Entries that every haplotype carries and entries that one haplotype outside a block carries give copy numbers 0 and `ploidy`; the
    coverages lie on both sides of the interval's bounds and at 255.  A row with a carried under-covered multi-copy k-mer is flagged and
    scored again with a fix that takes a block's haplotypes off that entry."""
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    rng = np.random.default_rng(5800 + ploidy)
    n_hap, bit_len = 16, 3
    used = np.arange(n_hap, dtype=np.uint8)
    blocks = [list(b) for b in _blocks(range(n_hap), ploidy, n_hap - 1)]
    if (n_hap - 1) % ploidy == 0:      # (ploidy 5: 11 .. 15 is a whole block; a truncated one as a panel of 14 haplotypes would have it)
        blocks.append([11, 12, 13] + [0] * (ploidy - 3))
    assert [0] * ploidy in blocks and any(0 in b and max(b) > 0 for b in blocks)
    pos = np.array(blocks, dtype=np.uint8)
    n_gt = pos.shape[0]
    top_mask = (1 << n_hap) - 1
    tables = (rng.random((ploidy + 1) * 256).astype(LD) + LD(0.05)) * np.power(LD(10), rng.integers(-200, 1, size=(ploidy + 1) * 256).astype(LD))
    n_rows, flag_row = 40, 11
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, n_rows, density=0.4, fixed={flag_row: 25, 5: 0})
    n_entries = f.size
    bits[rng.random(n_entries) < 0.1] |= np.uint64(top_mask)              # carried by every haplotype
    alone = rng.random(n_entries) < 0.1                                   # carried by haplotype 1 alone
    bits[alone] = (bits[alone] & ~np.uint64(top_mask)) | np.uint64(2)
    none = (bits & np.uint64(top_mask)) == 0
    bits[none] |= np.uint64(4)                                            # (the whole-list path does not prune: every entry has a carrier)
    cov[rng.random(n_entries) < 0.05] = 255
    gt0 = rng.integers(0, 1 << n_hap, size=n_rows).astype(np.uint16)
    # the flagged row: entry 2 is under-covered, multi-copy and carried by the second block's haplotypes; the fix takes them off
    jf = int(entry_begin[flag_row]) + 2
    second = blocks[2]
    cov[jf], f[jf] = 1, 2
    bits[jf] = np.uint64(sum(1 << h for h in set(second)))
    fix_mask = sum(1 << h for h in set(second) if h)
    entries = (f << np.uint64(8)) | (bits << np.uint64(16))

    def model(fixes=None):
        obs = np.ones((n_rows, n_gt), dtype=LD)
        flags = np.zeros(n_rows, dtype=np.uint8)
        seen = set()
        for r in range(n_rows):
            prod = np.ones(n_gt, dtype=LD)
            for jj in range(int(counts[r])):
                j = int(entry_begin[r]) + jj
                c, ff, b = int(cov[j]), int(f[j]), int(bits[j])
                last = (b >> (8 * bit_len - 1)) & 1
                in_interval = last == 1 and LOWER <= c <= UPPER
                one = [1 if (in_interval and (int(gt0[r]) >> p) & 1) else (b >> p) & 1 for p in range(n_hap)]
                if c < LOWER and ff >= 2 and any(one):
                    flags[r] |= 1
                if fixes and (r, jj) in fixes:
                    one = [0 if (fixes[(r, jj)] >> p) & 1 else o for p, o in enumerate(one)]
                fj = 2 if (last == 1 and ff == 1) else ff
                hs = [sum(one[p] for p in blk) for blk in blocks]      # a place that stands several times counts each time
                seen.update(hs)
                prod = prod * np.array([tables[h * 256 + _mld(h, c, fj)] for h in hs], dtype=LD)
            obs[r] = prod
        return obs, flags, seen

    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        obs, n_kept, flags = ctx.hmm_emissions(entries, cov, used, None, None, top_mask, bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, gt0, pos=pos)
        obs_f, n_kept_f, flags_f = ctx.hmm_emissions(entries, cov, used, None, None, top_mask, bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, gt0,
                                                     pos=pos, fixes=([flag_row], [0, 1], [2], [fix_mask]))
    finally:
        ctx.close()
    want, want_flags, seen = model()
    assert seen == set(range(ploidy + 1)), seen
    assert np.array_equal(n_kept, counts) and np.array_equal(flags, want_flags) and flags[flag_row] & 1 and not (flags & 2).any()
    for r in range(n_rows):
        assert np.array_equal(obs[r], want[r]), (r, int(np.argmax(obs[r] != want[r])))
    assert (obs[5] == 1).all() and (obs > 0).any()
    want_f, _, _ = model({(flag_row, 2): fix_mask})
    assert np.array_equal(n_kept_f, counts) and np.array_equal(flags_f, want_flags)
    for r in range(n_rows):
        assert np.array_equal(obs_f[r], want_f[r]), (r, int(np.argmax(obs_f[r] != want_f[r])))
    assert not np.array_equal(obs_f[flag_row], obs[flag_row]) and np.array_equal(np.delete(obs_f, flag_row, axis=0), np.delete(obs, flag_row, axis=0))


# ---- emission scores with a genotype list per window --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_drawn", [1, 5, 15])
@pytest.mark.parametrize("bit_len,n_hap", [(2, 15), (6, 47)])
@pytest.mark.parametrize("ploidy", PLOIDIES)
def test_emissions_with_a_genotype_list_per_window_for_ploidy_5_to_8(ploidy, bit_len, n_hap, n_drawn):
    """vgmi_hmm_emissions_select_ploidy against the numpy model -- scores, n_kept, flags, alive bytes -- in one call over six windows: a
    random draw, a draw with haplotype 0 (the all-zero block: haplotype 0 counted `ploidy` times), a draw with the last haplotype (its
    block is truncated, haplotype 0 repeated in it, wherever the last id is no multiple of the ploidy: everywhere but ploidy 7 over 15
    haplotypes, whose last block 8 .. 14 is whole), two drawn haplotypes in one block, a single drawn haplotype (one genotype), a second
    random draw.  20 rows per window of 0 .. 70 entries: a row of no entries, a row that loses every entry, a row half of whose entries are
    dead on entry, a flagged row that a second launch scores again with a fix that clears the panel's last haplotype (id 46 with six bytes
    of bits).  A further call with other draws scores the lists the first one pruned."""
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    rng = np.random.default_rng(1000 * ploidy + 10 * bit_len + n_drawn)
    max_hap = n_hap - 1
    assert max_hap == 8 * bit_len - 2
    truncated = max_hap % ploidy != 0
    assert truncated or (ploidy, n_hap) == (7, 15)
    per_window = 20

    def draws():
        def some(k, must=()):
            pool = [h for h in range(n_hap) if h not in must]
            return sorted(list(must) + [int(x) for x in rng.choice(pool, size=max(0, k - len(must)), replace=False)])
        return [some(n_drawn), some(n_drawn, (0,)), some(n_drawn, (max_hap,)), some(n_drawn, (1, 2) if n_drawn > 1 else (1,)), [5], some(n_drawn)]

    def windows(tops):
        lists = [_blocks(t, ploidy, max_hap) for t in tops]
        n_gt = max(len(x) for x in lists)
        win_haps = np.zeros((len(tops), n_gt, ploidy), dtype=np.uint8)
        for w, x in enumerate(lists):
            win_haps[w, :len(x)] = np.array(x, dtype=np.uint8)
        return (np.array([len(x) for x in lists], dtype=np.uint32), win_haps, np.array([sum(1 << h for h in t) for t in tops], dtype=np.uint64), lists)

    tops = draws()
    n_windows = len(tops)
    n_rows = n_windows * per_window
    win_n, win_haps, win_top, lists = windows(tops)
    assert (0,) * ploidy in lists[1] and win_n[4] == 1 and win_n[3] < max(n_drawn, 2)
    last_block = next(gt for gt in lists[2] if max_hap in gt)
    assert (0 in last_block) == truncated
    zero_row, lost_row, dead_row, flag_row = 2, per_window + 3, 3 * per_window + 5, 2 * per_window + 7
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, n_rows, fixed={zero_row: 0, lost_row: 20, dead_row: 30, flag_row: 25})
    row_win = np.repeat(np.arange(n_windows), per_window).astype(np.uint32)
    gt0 = rng.integers(0, 1 << n_hap, size=n_rows, dtype=np.uint64)
    tables = (rng.random(256 * (ploidy + 1)).astype(LD) + LD(0.05)) * np.power(LD(10), rng.integers(-300, 1, size=256 * (ploidy + 1)).astype(LD))
    counts_l = counts.tolist()
    e_lost = slice(int(entry_begin[lost_row]), int(entry_begin[lost_row]) + counts_l[lost_row])
    bits[e_lost] &= ~win_top[1]
    alive0 = (rng.random(f.size) < 0.9).astype(np.uint8)
    alive0[int(entry_begin[dead_row]):int(entry_begin[dead_row]) + counts_l[dead_row]:2] = 0
    alive0[int(entry_begin[dead_row]) + 1] = 1      # (one of the living is carried by the window's draw for certain)
    bits[int(entry_begin[dead_row]) + 1] |= win_top[3]
    # the flagged row (window 2, whose draw holds the last haplotype): entry 2 is under-covered, multi-copy and carried by the last
    # haplotype alone among those of its block; the sequence check takes it off
    jf = int(entry_begin[flag_row]) + 2
    alive0[jf] = 1
    cov[jf], f[jf] = 1, 2
    bits[jf] &= ~np.uint64(sum(1 << h for h in set(last_block)))
    bits[jf] |= np.uint64(1) << np.uint64(max_hap)
    gt0[flag_row] = 0
    # an entry every haplotype of the panel carries, in a row of the all-zero block's window: copy number `ploidy` from one id
    j_all = int(entry_begin[per_window + 5])
    if counts_l[per_window + 5]:
        alive0[j_all] = 1
        bits[j_all] |= np.uint64((1 << n_hap) - 1)
    entries = (f << np.uint64(8)) | (bits << np.uint64(16))
    fixes = {(flag_row, 2): 1 << max_hap}
    tops2 = draws()
    win_n2, win_haps2, win_top2, _ = windows(tops2)

    def call(ctx, wn, wh, wt, fx=None):
        return ctx.hmm_emissions_select_ploidy(ploidy, wn, wh, wt, bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0, fixes=fx)

    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        ctx.hmm_entries_upload(entries, cov, alive0)
        obs, n_kept, flags = call(ctx, win_n, win_haps, win_top)
        alive1 = ctx.hmm_alive_fetch()
        obs_f, n_kept_f, flags_f = call(ctx, win_n, win_haps, win_top, ([flag_row], [0, 1], [2], [fixes[(flag_row, 2)]]))
        alive1b = ctx.hmm_alive_fetch()
        obs2, n_kept2, flags2 = call(ctx, win_n2, win_haps2, win_top2)
        alive2 = ctx.hmm_alive_fetch()
    finally:
        ctx.close()

    m_alive = alive0.copy()
    want, want_kept, want_flags = _model(f, bits, cov, m_alive, bit_len, win_n, win_haps, win_top, tables, entry_begin, counts, row_win, gt0)
    assert np.array_equal(n_kept, want_kept) and np.array_equal(flags, want_flags)
    for r in range(n_rows):
        assert np.array_equal(obs[r], want[r]), (r, int(np.argmax(obs[r] != want[r])))
    assert np.array_equal(alive1, m_alive)
    assert n_kept[zero_row] == 0 and (obs[zero_row, :win_n[0]] == 1).all()
    assert n_kept[lost_row] == 0 and not alive1[e_lost].any() and (obs[lost_row, :win_n[1]] == 1).all()
    assert 0 < n_kept[dead_row] <= counts_l[dead_row] // 2
    assert flags[flag_row] & 1 and not (flags & 2).any()
    for w in range(n_windows):      # lanes beyond a window's count: zero scores
        assert not obs[row_win == w][:, win_n[w]:].any()
    assert 0 < (alive0 != alive1).sum() and (n_kept > 0).sum() > n_rows // 2 and (obs > 0).any()

    # the same lists once more with the flagged row scored again: nothing further dies, the other rows keep their scores
    want_f, _, _ = _model(f, bits, cov, m_alive, bit_len, win_n, win_haps, win_top, tables, entry_begin, counts, row_win, gt0, fixes=fixes)
    assert np.array_equal(alive1b, alive1) and np.array_equal(n_kept_f, n_kept) and np.array_equal(flags_f, flags)
    for r in range(n_rows):
        assert np.array_equal(obs_f[r], want_f[r]), r
    assert not np.array_equal(obs_f[flag_row], obs[flag_row]) and np.array_equal(np.delete(obs_f, flag_row, axis=0), np.delete(obs, flag_row, axis=0))

    # other draws: the lists as the first call left them
    want2, want_kept2, want_flags2 = _model(f, bits, cov, m_alive, bit_len, win_n2, win_haps2, win_top2, tables, entry_begin, counts, row_win, gt0)
    assert np.array_equal(n_kept2, want_kept2) and np.array_equal(flags2, want_flags2)
    for r in range(n_rows):
        assert np.array_equal(obs2[r], want2[r]), (r, int(np.argmax(obs2[r] != want2[r])))
    killed = (alive0 == 1) & (alive1 == 0)
    assert np.array_equal(alive2, m_alive) and not alive2[killed].any() and n_kept2[lost_row] == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_ploidy_0_and_9_are_refused_and_the_context_serves_on():
    """Every widened call answers VGMI_E_INVALID to ploidy 0 and to ploidy 9 -- vgmi_hmm_recursion, _calls, _calls_part, _emissions_ploidy with
    _part_calls and _plan_create behind it, _emissions_select_ploidy -- and a valid call of ploidy 5 goes through after each."""
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    rng = np.random.default_rng(59)
    ploidy, n = 5, 3
    keep, obs, row, restart, pows, uniform, chains = _recursion_case(rng, ploidy, n)
    want = np.concatenate([_host_chain(keep[0], [obs[r] for r in row[a:a + c]], restart[a:a + c], pows[a:a + c], uniform, ploidy) for a, c, _ in chains])
    n_rows = obs.shape[0]
    gid = np.zeros((n_rows, n), dtype=np.uint8)
    order = np.full((n_rows, n), 0xFF, dtype=np.uint8)
    order[:, 0] = 0
    fwd = np.arange(n_rows, dtype=np.uint64)
    bwd = (2 * n_rows - 1 - np.arange(n_rows)).astype(np.uint64)
    row_a, restart_a = np.array(row, dtype=np.uint32), np.array(restart, dtype=np.uint8)

    def pw(p):      # tables of the width a call of ploidy p would read
        return np.ones((len(row), 2, p + 1), dtype=LD)

    # emissions: three rows of four entries over seven haplotypes
    n_hap, bit_len = 7, 1
    entries = ((np.uint64(1) << np.uint64(8)) | (rng.integers(1, 1 << n_hap, size=12).astype(np.uint64) << np.uint64(16)))
    cov = rng.integers(0, 40, size=12).astype(np.uint8)
    e_begin, e_count = np.array([0, 4, 8], dtype=np.uint64), np.array([4, 4, 4], dtype=np.uint32)
    used = np.arange(n_hap, dtype=np.uint8)

    def emit_args(p):
        pos = np.array([[0] * p, [min(q + 1, n_hap - 1) for q in range(p)]], dtype=np.uint8) if p else np.zeros((2, 0), dtype=np.uint8)
        return dict(pos=pos, tables=np.full((p + 1) * 256, LD(0.5), dtype=LD))

    def emit(p, calls=None):
        a = emit_args(p)
        return ctx.hmm_emissions(entries, cov, used, None, None, (1 << n_hap) - 1, bit_len, AVE, LOWER, UPPER, a["tables"], e_begin, e_count,
                                 np.zeros(3, dtype=np.uint16), pos=a["pos"], calls=calls)

    def emit_lists(p):
        a = emit_args(p)
        haps = a["pos"][None]
        return ctx.hmm_emissions_select_ploidy(p, [2], haps, [(1 << n_hap) - 1], bit_len, AVE, LOWER, UPPER, a["tables"], e_begin, e_count, [0, 0, 0],
                                               np.zeros(3, dtype=np.uint64))

    def part_calls(p):      # a part of ploidy 5 whose recursion is asked for with ploidy p: vgmi_hmm_part_calls, then _plan_create
        k2 = np.full((1, 2, 2), 1, dtype=np.uint8)
        return dict(ploidy=p, keep=k2, row=[0, 1, 2, 2, 1, 0], restart=[1, 0, 0, 1, 0, 0], pow=np.ones((6, 2, p + 1), dtype=LD), uniform=LD(0.5),
                    chains=[(0, 3, 0), (3, 3, 0)], gid=np.zeros((3, 2), dtype=np.uint8), order=np.array([[0, 0xFF]] * 3, dtype=np.uint8), fwd=[0, 1, 2], bwd=[5, 4, 3])

    def refused(fn):
        with pytest.raises(vgmi.VgmiError) as e:
            fn()
        assert e.value.code == vgmi.E_INVALID
        assert np.array_equal(ctx.hmm_recursion(keep, obs, row, restart, pows, uniform, chains, ploidy), want)

    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        good = emit(5, calls=part_calls(5))
        assert len(good) == 4 and (good[0] > 0).all()
        good_lists = emit_lists(5)
        for bad in (0, 9):
            refused(lambda: ctx.hmm_recursion(keep, obs, row, restart, pw(bad), uniform, chains, bad))
            refused(lambda: ctx.hmm_calls(keep, obs, row, restart, pw(bad), uniform, chains, bad, gid, order, fwd, bwd))
            prob, winner = np.zeros(n_rows, dtype=LD), np.zeros(n_rows, dtype=np.uint32)
            refused(lambda: ctx.hmm_calls_part(keep, obs, row_a, restart_a, pw(bad), uniform, chains, bad, gid, order, fwd, bwd, (0, n_rows), (0, len(row)),
                                               prob, winner))
            refused(lambda: emit(bad))
            refused(lambda: emit(5, calls=part_calls(bad)))      # vgmi_hmm_part_calls refuses (and would before _plan_create is reached)
            refused(lambda: emit_lists(bad))
            ctx.hmm_entries_upload(entries, cov)      # (the emission calls of this wrapper upload; the lists' call reads the context's)
            again = emit_lists(5)
            assert all(np.array_equal(x, y) for x, y in zip(again, good_lists))
        # beyond 128 genotypes a node's step table must fit the workgroup's local memory: 12 x n_gt x (ploidy + 2) bytes of 160 KiB
        wide = 1365
        refused(lambda: ctx.hmm_recursion(np.zeros((1, wide, wide), dtype=np.uint8), np.ones((n_rows, wide), dtype=LD), row, restart, pw(8), LD(1) / LD(wide),
                                          chains, 8))
        # vgmi_hmm_plan_create on its own: the wrapper reaches it only behind a good _part_calls, so straight at the C ABI
        import ctypes as C
        from varigraph_amd.vgmi import _ptr
        a = part_calls(5)
        ch = np.zeros((2, 3), dtype=np.uint64)
        ch[0], ch[1] = (0, 3, 0), (3, 3, 0)
        arrs = dict(keep=a["keep"], row=np.array(a["row"], dtype=np.uint32), restart=np.array(a["restart"], dtype=np.uint8), uni=np.array([a["uniform"]], dtype=LD),
                    gid=a["gid"], order=a["order"], fwd=np.array(a["fwd"], dtype=np.uint64), bwd=np.array(a["bwd"], dtype=np.uint64))
        for p, want_rc in ((0, vgmi.E_INVALID), (9, vgmi.E_INVALID), (8, 0)):
            plan = C.c_void_p()
            pw_p = np.ones((6, 2, p + 1), dtype=LD)
            rc = ctx._l.vgmi_hmm_plan_create(ctx._h, 2, p, _ptr(arrs["keep"]), 1, 3, _ptr(arrs["row"]), _ptr(arrs["restart"]), _ptr(pw_p), 6, _ptr(arrs["uni"]),
                                             _ptr(ch), 2, _ptr(arrs["gid"]), _ptr(arrs["order"]), _ptr(arrs["fwd"]), _ptr(arrs["bwd"]), C.byref(plan))
            assert rc == want_rc, (p, rc)
            if rc == 0:
                ctx._l.vgmi_hmm_plan_free(plan)
            assert np.array_equal(ctx.hmm_recursion(keep, obs, row, restart, pows, uniform, chains, ploidy), want)
    finally:
        ctx.close()


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def _cohort(tmp_path_factory, name, length, n_sites, n_samples, who, n_pairs, seed):
    import shutil
    from test_gpu_configs import CLI, ENV, _need_binaries, _write_fastq
    from varigraph_amd import synth
    _need_binaries()
    work = str(tmp_path_factory.mktemp(name))
    ref = synth.make_reference(length)
    variants, gts = synth.make_cohort(ref, n_sites, n_samples=n_samples, ploidy=6, seed=seed, indel_frac=0.1, sv_frac=0.4)
    fa, vcf = os.path.join(work, "ref.fa"), os.path.join(work, "in.vcf")
    synth.write_fasta(fa, "chr1", ref)
    synth.write_vcf(vcf, "chr1", len(ref), variants, gts, n_samples, 6)
    graph = os.path.join(work, "graph.bin")
    r = subprocess.run([CLI, "construct", "-r", fa, "-v", vcf, "--save-graph", graph, "-t", "16", "--gpu", "0", "--vcf-ploidy", "6"], cwd=work,
                       capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    cfg = ""
    for i, ind in enumerate(who):
        fq = _write_fastq(os.path.join(work, f"s{i}"), synth.sample_haplotypes(ref, variants, gts, ind, 6), n_pairs, seed=570 + i)
        cfg += f"ind{i} " + " ".join(fq) + "\n"
    return work, graph, cfg, lambda: shutil.rmtree(work, ignore_errors=True)


@pytest.fixture(scope="module")
def hexaploid_cohort(tmp_path_factory):
    """120 kb, 800 sites (one in ten a short indel, four in ten an insertion of 60 .. 300 bp), `--vcf-ploidy 6`, four samples: 25 haplotypes
    with the reference.  Reads of three individuals, three samples in one samples.cfg: the second and third see pruned lists."""
    work, graph, cfg, done = _cohort(tmp_path_factory, "ploidy8_cli", 120_000, 800, 4, (0, 1, 3), 16_000, 23)
    yield work, graph, cfg
    done()


@pytest.fixture(scope="module")
def hexaploid_panel(tmp_path_factory):
    """60 kb, 400 sites, two hexaploid samples: 13 haplotypes, so `-n` (15) selects them all and the whole panel's emissions are scored."""
    work, graph, cfg, done = _cohort(tmp_path_factory, "ploidy8_panel_cli", 60_000, 400, 2, (0, 1), 8_000, 29)
    yield work, graph, cfg
    done()


SELECT_LINE = r"HMM emissions on the device: .*haplotypes selected per window for (\d+) of (\d+) windows"
POOL_LINE = r"HMM part \d+ \(windows (\d+)-(\d+)\): on the device from"
PANEL_LINE = r"HMM part \d+ \(windows (\d+)-(\d+)\): emissions, recursion and posterior on the device from"
TALLY_LINE = r"HMM tallies on the device"
DEVICE_LINE = r"HMM (?:part \d+|emissions|recursion|tallies|transitions by haplotype frequency)[^\n]* on the device"      # any of the HMM's own lines
SUMMARY_LINE = r"genotyping [\d.]+ s \(HMM [\d.]+ with (\d+) of (\d+) windows on the device"


def _nothing_on_the_device(log, n_samples):
    seen = re.findall(SUMMARY_LINE, log)
    assert not re.search(DEVICE_LINE, log) and len(seen) == n_samples and all(a == "0" for a, _ in seen), seen


def _legs(work, graph, cfg, opts, legs, n_samples):
    """`genotype` once per leg (name, executable, more options, environment): ({name: the samples' VCFs}, {name: stderr})"""
    from test_gpu_configs import _run, _vcf
    tag = "_".join(o.strip("-") for o in opts)
    outs, logs = {}, {}
    for name, exe, more, env in legs:
        d = os.path.join(work, f"{name}_{tag}")
        os.makedirs(d, exist_ok=True)
        open(os.path.join(d, "samples.cfg"), "w").write(cfg)
        r = _run([exe, "genotype", "--load-graph", graph, "-s", "samples.cfg", "-t", "6"] + opts + ["--use-depth", "--granularity", "0.01"] + more, cwd=d,
                 capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        outs[name] = [_vcf(d, f"ind{i}") for i in range(n_samples)]
        logs[name] = r.stderr
    lines = [v.count(b"\n") for v in outs["cpu"]]
    print(f"{' '.join(opts)}: reference VCF lines {lines}")
    assert min(lines) >= 50, lines
    for name in outs:
        for i in range(n_samples):
            assert outs[name][i] == outs["cpu"][i], (opts, name, i)
    return outs, logs


def _windows_on_the_device(line, log, n_samples):
    """the windows a log's part lines cover, which must be the same whole range for every sample; returns that number"""
    spans = [(int(a), int(b)) for a, b in re.findall(line, log)]
    total = sum(b - a + 1 for a, b in spans)
    n_windows = max(b for _, b in spans) + 1 if spans else 0
    assert spans and min(a for a, _ in spans) == 0 and total == n_samples * n_windows, spans
    return n_windows


@pytest.mark.parametrize("opts", [["--sample-ploidy", "6", "-n", "5"], ["--sample-ploidy", "8", "-n", "4"], ["--sample-ploidy", "5", "-n", "5", "--sv"],
                                  ["--sample-ploidy", "6", "-n", "40"]], ids=["p6n5", "p8n4", "p5n5sv", "p6n40"])
def test_command_line_ploidy_5_to_8_on_the_device_equals_the_reference(opts, hexaploid_cohort):
    """`varigraph-mi genotype --sample-ploidy P -n N --use-depth` over a 25-haplotype graph, three samples in one run: every VCF is the
    deterministic reference build's byte for byte (at least 50 lines each), with the device and with VGH_HMM_DEVICE=0 (the host's whole HMM,
    which says nothing of a device), and for `-n` below the panel with VGH_HMM_SELECT_DEVICE=0 as well.  The VGH_TIMING log names the device
    for every window of every sample -- the list-per-window path under `-n` 4 and 5, the recursion alone (the pool) under `-n 40`, where
    nothing is selected and the panel is wider than 16 haplotypes -- and never the device's tallies: a call of five to eight haplotypes is
    tallied by the host's walk."""
    from test_gpu_configs import CLI, ENV, REF
    work, graph, cfg = hexaploid_cohort
    selection = opts[opts.index("-n") + 1] != "40"
    timing = dict(ENV, VGH_TIMING="1")
    legs = [("cpu", REF, [], ENV), ("native", CLI, ["--gpu", "0"], timing), ("host", CLI, ["--gpu", "0"], dict(timing, VGH_HMM_DEVICE="0"))]
    if selection:
        legs.append(("host_select", CLI, ["--gpu", "0"], dict(timing, VGH_HMM_SELECT_DEVICE="0")))
    outs, logs = _legs(work, graph, cfg, opts, legs, 3)
    assert outs["cpu"][0] != outs["cpu"][1] != outs["cpu"][2] and outs["cpu"][0] != outs["cpu"][2]
    if selection:
        seen = re.findall(SELECT_LINE, logs["native"])
        assert len(seen) == 3 and all(a == b and int(b) >= 12 for a, b in seen), seen
        assert "haplotypes selected per window" not in logs["host_select"]
    else:
        assert _windows_on_the_device(POOL_LINE, logs["native"], 3) >= 12
        assert len(re.findall(r"HMM recursion on the device: ", logs["native"])) == 3
    assert not re.search(TALLY_LINE, logs["native"])
    _nothing_on_the_device(logs["host"], 3)


def test_command_line_hexaploid_whole_panel_on_the_device_equals_the_reference(hexaploid_panel):
    """`--sample-ploidy 6` over a 13-haplotype graph: every haplotype is selected, so the emissions of the whole panel, the recursion and the
    posterior run on the device, part by part, for every window of both samples; VGH_HMM_EMIT_DEVICE=0 (the host's scores, the device's
    recursion) and VGH_HMM_DEVICE=0 write the same bytes as the reference.  No tallies on the device."""
    from test_gpu_configs import CLI, ENV, REF
    work, graph, cfg = hexaploid_panel
    timing = dict(ENV, VGH_TIMING="1")
    legs = [("cpu", REF, [], ENV), ("native", CLI, ["--gpu", "0"], timing), ("host", CLI, ["--gpu", "0"], dict(timing, VGH_HMM_DEVICE="0")),
            ("host_emit", CLI, ["--gpu", "0"], dict(timing, VGH_HMM_EMIT_DEVICE="0"))]
    outs, logs = _legs(work, graph, cfg, ["--sample-ploidy", "6"], legs, 2)
    assert outs["cpu"][0] != outs["cpu"][1]
    assert _windows_on_the_device(PANEL_LINE, logs["native"], 2) >= 6
    assert len(re.findall(r"HMM emissions on the device: \d+ parts", logs["native"])) == 2
    assert not re.search(TALLY_LINE, logs["native"])
    _nothing_on_the_device(logs["host"], 2)
    assert not re.search(PANEL_LINE, logs["host_emit"]) and _windows_on_the_device(POOL_LINE, logs["host_emit"], 2) >= 6


def test_command_line_hexaploid_by_haplotype_frequency_stays_on_the_host(hexaploid_panel):
    """`-m fre --sample-ploidy 6`: the recursion by haplotype frequency takes genotypes of 2 .. 4 haplotypes, so this sample keeps the host's
    HMM -- the reference's bytes, and no word of a device in the log."""
    from test_gpu_configs import CLI, ENV, REF
    work, graph, cfg = hexaploid_panel
    legs = [("cpu", REF, [], ENV), ("native", CLI, ["--gpu", "0"], dict(ENV, VGH_TIMING="1"))]
    outs, logs = _legs(work, graph, cfg, ["--sample-ploidy", "6", "-m", "fre"], legs, 2)
    _nothing_on_the_device(logs["native"], 2)
