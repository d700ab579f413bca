"""A diploid sample over a panel of 48 to 254 haplotypes on the device (vgmi_hmm_*_wide: 7 to 32 bytes of haplotype bits per entry, W = 1, 2
or 4 words on the device): the support sums, the emission scores with the prune, the alive bytes and the calls' tallies against the same
computation spelled out in numpy / Python integers (products in numpy.longdouble, the x87 format, bit for bit); the wide calls against the
packed ones on data both take; every refusal; and the command line over a 53- and a 67-haplotype graph against the deterministic build of
the reference, byte for byte, with the log saying which path ran."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from varigraph_amd import vgmi
from test_gpu_hmm_select import AVE, LOWER, UPPER, _model_emissions

pytestmark = pytest.mark.gpu
LD = np.longdouble
N_WINDOWS, PER_WINDOW = 3, 40


def _words(bit_len):
    return 1 if bit_len <= 8 else 2 if bit_len <= 16 else 4


def _masks(win_used, bit_len):
    """(n_windows, W) uint64: word i of a window holds its haplotypes 64 i .. 64 i + 63"""
    m = np.zeros((len(win_used), _words(bit_len)), dtype=np.uint64)
    for w, used in enumerate(win_used):
        for h in used:
            m[w, int(h) >> 6] |= np.uint64(1) << np.uint64(int(h) & 63)
    return m


def _bytes_of(bits, bit_len):
    """the entries' bit vectors as they stand in a graph: (n_entries, bit_len) uint8 from Python integers"""
    return np.frombuffer(b"".join(int(b).to_bytes(bit_len, "little") for b in bits), dtype=np.uint8).reshape(len(bits), bit_len)


def _panel(rng, n_hap, bit_len, n_rows, fixed):
    """counts, entry_begin, f, bits (Python integers: any width), cov"""
    counts = rng.integers(0, 71, size=n_rows)
    for r, n in fixed.items():
        counts[r] = n
    entry_begin = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    n_entries = int(counts.sum())
    f = rng.choice([1, 1, 1, 2, 3, 4], size=n_entries).astype(np.uint8)
    carried = rng.random((n_entries, n_hap)) < 12.0 / n_hap        # a dozen carriers per entry whatever the panel's size
    last = rng.integers(0, 2, size=n_entries)
    bits = [sum(1 << int(h) for h in np.flatnonzero(carried[j])) | (int(last[j]) << (8 * bit_len - 1)) for j in range(n_entries)]
    cov = rng.choice([0, 1, 2, 5, 14, 15, 20, 23, 24, 30, 33, 34, 60, 255], size=n_entries).astype(np.uint8)
    return counts, entry_begin, f, bits, cov


def _model_support(f, bits, cov, alive, n_hap, n_windows, entry_begin, counts, row_win):
    want = np.zeros((n_windows, n_hap), dtype=np.uint64)
    for r in range(len(counts)):
        for j in range(int(entry_begin[r]), int(entry_begin[r]) + int(counts[r])):
            if alive[j] and cov[j] > 1 and f[j] <= 1:
                for h in range(n_hap):
                    if (bits[j] >> h) & 1:
                        want[row_win[r], h] += int(cov[j])
    return want


def _model_tallies(f, bits, cov, alive, pairs, win_used, entry_begin, counts, row_win, winner):
    out = np.zeros((len(counts), 4), dtype=np.uint32)
    uniq = np.zeros(len(counts), dtype=np.uint8)
    for r in range(len(counts)):
        if winner[r] >= len(pairs):
            continue
        ha, hb = (int(win_used[row_win[r]][p]) for p in pairs[winner[r]])
        u = 0
        for j in range(int(entry_begin[r]), int(entry_begin[r]) + int(counts[r])):
            if not alive[j]:
                continue
            if f[j] <= 1 and u < 255:
                u += 1
            if (bits[j] >> ha) & 1:
                out[r, 0] += 1
                out[r, 1] += int(cov[j])
            if (bits[j] >> hb) & 1:
                out[r, 2] += 1
                out[r, 3] += int(cov[j])
        uniq[r] = u
    return out, uniq


# bit_len -> (haplotypes, ids the first window's selection must hold)
WIDTHS = {7: (53, [52]), 8: (63, [62]), 9: (71, [63, 64, 70]), 12: (95, [63, 64, 94]), 17: (135, [127, 128, 134]), 32: (255, [0, 127, 128, 253])}


@pytest.mark.parametrize("n_used", [5, 15])
@pytest.mark.parametrize("bit_len", sorted(WIDTHS))
def test_wide_kernels_equal_the_host_arithmetic_at_every_width(bit_len, n_used):
    """Support, emissions (with the prune, a fixed row, a second sample on the pruned lists), alive bytes and tallies of the _wide calls against
    the model, array_equal throughout, at the widths where the kernels can go wrong: 7 bytes (53 haplotypes, the first width past the packed
    word), 8 (W = 1, the last bit at bit 63, id 62 selected), 9 (W = 2, ids 63 and 64 both selected, the last bit at bit 71), 12 (95
    haplotypes), 17 (W = 4, the words beyond byte 17 are padding) and 32 (ids 0, 127, 128 and 253 selected, the last bit at 255); 5 and 15
    selected haplotypes (15 and 120 genotypes).  120 rows in three windows: an empty row, a row that dies in the prune, a row with dead
    entries on entry, an entry only a haplotype of the top word carries (it stays), an entry whose only set bit is the last bit (it leaves
    the list: the last bit is no haplotype) and a flagged row scored again with a fix."""
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    n_hap, must = WIDTHS[bit_len]
    W = _words(bit_len)
    assert n_hap <= 8 * bit_len - 1 and max(must) <= 8 * bit_len - 2
    rng = np.random.default_rng(100 * bit_len + n_used)
    n_rows = N_WINDOWS * PER_WINDOW
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, n_rows, fixed={3: 20, 5: 0, 50: 30, 60: 6, 90: 25})
    row_win = np.repeat(np.arange(N_WINDOWS), PER_WINDOW).astype(np.uint32)

    def selection(first):
        sel = []
        for w in range(N_WINDOWS):      # every window holds a haplotype of the top word
            base = list(first) if w == 0 else [n_hap - 1 - w]
            others = [h for h in range(n_hap) if h not in base]
            sel.append(sorted(base + [int(h) for h in rng.choice(others, size=n_used - len(base), replace=False)]))
        return np.array(sel, dtype=np.uint8)
    win_used = selection(must)
    assert all(h in win_used[0] for h in must) and (win_used >> 6 == (n_hap - 1) >> 6).any(axis=1).all()
    masks = _masks(win_used, bit_len)
    assert masks.shape == (N_WINDOWS, W) and (W == 1 or masks[:, (n_hap - 1) >> 6].all())
    int_mask = [sum(1 << int(h) for h in u) for u in win_used]
    pairs = list(itertools.combinations_with_replacement(range(n_used), 2))
    assert len(pairs) == (15 if n_used == 5 else 120)
    gt0 = rng.integers(0, 1 << n_used, size=n_rows).astype(np.uint16)
    tables = (rng.random(768).astype(LD) + LD(0.05)) * np.power(LD(10), rng.integers(-300, 1, size=768).astype(LD))
    last_bit = 1 << (8 * bit_len - 1)
    e = [int(x) for x in entry_begin]
    # row 3: no entry carries a haplotype of its window; row 50: half its entries dead on entry; row 60 (window 1): entry 0 is carried by the
    # window's top-word haplotype alone, entry 1 has the last bit alone, entry 2 the last bit and haplotypes outside the selection; row 90:
    # entry 2 is an under-covered multi-copy k-mer that the window's first two haplotypes carry
    for j in range(e[3], e[3] + 20):
        bits[j] &= ~int_mask[0]
    alive0 = (rng.random(len(bits)) < 0.9).astype(np.uint8)
    alive0[e[50]:e[50] + 30:2] = 0
    top_hap = int(win_used[1].max())
    assert top_hap >> 6 == (n_hap - 1) >> 6
    outside = [h for h in range(n_hap) if h not in win_used[1]][:3]
    bits[e[60]], bits[e[60] + 1], bits[e[60] + 2] = 1 << top_hap, last_bit, last_bit | sum(1 << h for h in outside)
    alive0[e[60]:e[60] + 3] = 1
    cov[e[60]:e[60] + 3] = 23
    j90 = e[90] + 2
    alive0[j90] = 1
    cov[j90], f[j90] = 1, 2
    bits[j90] |= (1 << int(win_used[2][0])) | (1 << int(win_used[2][1]))
    gt0[90] = 0
    fixes = {(90, 2): 0b01}
    win_used2 = selection([n_hap - 1])
    masks2 = _masks(win_used2, bit_len)
    winner = rng.integers(0, len(pairs), size=n_rows).astype(np.uint32)
    winner[::9] = 0xFFFFFFFF
    pa, pb = [a for a, _ in pairs], [b for _, b in pairs]

    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        ctx.hmm_entries_upload_wide(f, _bytes_of(bits, bit_len), bit_len, cov, alive0)
        support = ctx.hmm_support_wide(bit_len, n_hap, N_WINDOWS, entry_begin, counts, row_win)
        obs, n_kept, flags = ctx.hmm_emissions_select_wide(pa, pb, win_used, masks, bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0)
        alive1 = ctx.hmm_alive_fetch()
        support1 = ctx.hmm_support_wide(bit_len, n_hap, N_WINDOWS, entry_begin, counts, row_win)
        tally, uniq = ctx.hmm_tallies_select_wide(bit_len, entry_begin, counts, row_win, winner, pa, pb, win_used)
        # the same selection once more with the flagged row scored again: nothing further dies, the other rows keep their scores
        obs_f, n_kept_f, flags_f = ctx.hmm_emissions_select_wide(pa, pb, win_used, masks, bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win,
                                                                 gt0, fixes=([90], [0, 1], [2], [fixes[(90, 2)]]))
        alive1b = ctx.hmm_alive_fetch()
        # the next sample: other haplotypes per window, the lists as the first sample left them
        obs2, n_kept2, flags2 = ctx.hmm_emissions_select_wide(pa, pb, win_used2, masks2, bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0)
        alive2 = ctx.hmm_alive_fetch()
        tally2, uniq2 = ctx.hmm_tallies_select_wide(bit_len, entry_begin, counts, row_win, winner, pa, pb, win_used2)
    finally:
        ctx.close()

    assert np.array_equal(support.astype(np.uint64), _model_support(f, bits, cov, alive0, n_hap, N_WINDOWS, entry_begin, counts, row_win))
    assert support[:, n_hap - 1].all() and support[0, must].all()
    m_alive = alive0.copy()
    want, want_kept, want_flags = _model_emissions(f, bits, cov, m_alive, bit_len, pairs, win_used, tables, entry_begin, counts, row_win, gt0)
    assert np.array_equal(n_kept, want_kept) and np.array_equal(flags, want_flags)
    for r in range(n_rows):
        assert np.array_equal(obs[r], want[r]), (r, int(np.argmax(obs[r] != want[r])))
    assert np.array_equal(alive1, m_alive)
    assert n_kept[3] == 0 and not alive1[e[3]:e[3] + 20].any() and (obs[3] == 1).all()
    assert n_kept[5] == 0 and (obs[5] == 1).all()
    assert alive1[e[60]] == 1 and alive1[e[60] + 1] == 0 and alive1[e[60] + 2] == 0
    assert flags[90] & 1 and not (flags & 2).any()
    assert 0 < (alive0 != alive1).sum() and (n_kept > 0).sum() > n_rows // 2 and (obs > 0).any()
    assert np.array_equal(support1.astype(np.uint64), _model_support(f, bits, cov, alive1, n_hap, N_WINDOWS, entry_begin, counts, row_win))
    want_t, want_u = _model_tallies(f, bits, cov, alive1, pairs, win_used, entry_begin, counts, row_win, winner)
    assert np.array_equal(tally, want_t) and np.array_equal(uniq, want_u)
    assert not tally[::9].any() and tally[1::9].any() and tally[:, 0].any() and tally[:, 2].any()

    want_f, _, _ = _model_emissions(f, bits, cov, m_alive, bit_len, pairs, win_used, tables, entry_begin, counts, row_win, gt0, fixes=fixes)
    assert np.array_equal(alive1b, alive1) and np.array_equal(n_kept_f, n_kept) and np.array_equal(flags_f, flags)
    for r in range(n_rows):
        assert np.array_equal(obs_f[r], want_f[r]), r
    assert not np.array_equal(obs_f[90], obs[90]) and np.array_equal(np.delete(obs_f, 90, axis=0), np.delete(obs, 90, axis=0))

    killed = (alive0 == 1) & (alive1 == 0)
    int_mask2 = [sum(1 << int(h) for h in u) for u in win_used2]
    assert any(bits[j] & int_mask2[row_win[np.searchsorted(entry_begin, j, side="right") - 1]] for j in np.flatnonzero(killed)), \
        "no entry would tell a persistent prune from a fresh one"
    want2, want_kept2, want_flags2 = _model_emissions(f, bits, cov, m_alive, bit_len, pairs, win_used2, tables, entry_begin, counts, row_win, gt0)
    assert np.array_equal(n_kept2, want_kept2) and np.array_equal(flags2, want_flags2)
    for r in range(n_rows):
        assert np.array_equal(obs2[r], want2[r]), (r, int(np.argmax(obs2[r] != want2[r])))
    assert np.array_equal(alive2, m_alive) and not alive2[killed].any() and n_kept2[3] == 0
    want_t2, want_u2 = _model_tallies(f, bits, cov, alive2, pairs, win_used2, entry_begin, counts, row_win, winner)
    assert np.array_equal(tally2, want_t2) and np.array_equal(uniq2, want_u2)


@pytest.mark.parametrize("bit_len,n_hap", [(3, 23), (6, 47)])
def test_wide_calls_return_the_packed_calls_bytes(bit_len, n_hap):
    """On data both forms take -- 3 and 6 bytes of haplotype bits -- hmm_support_wide / hmm_emissions_select_wide (with a fixed row) /
    hmm_tallies_select_wide return exactly what hmm_support / hmm_emissions_select / hmm_tallies_select return, alive bytes included."""
    rng = np.random.default_rng(77 + bit_len)
    n_used, n_rows = 5, N_WINDOWS * PER_WINDOW
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, n_rows, fixed={3: 20, 90: 25})
    row_win = np.repeat(np.arange(N_WINDOWS), PER_WINDOW).astype(np.uint32)
    win_used = np.array([sorted([n_hap - 1 - w] + [int(h) for h in rng.choice(n_hap - 4, size=n_used - 1, replace=False)]) for w in range(N_WINDOWS)], dtype=np.uint8)
    pairs = list(itertools.combinations_with_replacement(range(n_used), 2))
    pa, pb = [a for a, _ in pairs], [b for _, b in pairs]
    gt0 = rng.integers(0, 1 << n_used, size=n_rows).astype(np.uint16)
    tables = (rng.random(768).astype(LD) + LD(0.05)) * np.power(LD(10), rng.integers(-300, 1, size=768).astype(LD))
    alive0 = (rng.random(len(bits)) < 0.9).astype(np.uint8)
    j90 = int(entry_begin[90]) + 2
    alive0[j90], cov[j90], f[j90] = 1, 1, 2
    bits[j90] |= (1 << int(win_used[2][0])) | (1 << int(win_used[2][1]))
    gt0[90] = 0
    fix = ([90], [0, 1], [2], [0b10])
    winner = rng.integers(0, len(pairs), size=n_rows).astype(np.uint32)
    winner[::7] = 0xFFFFFFFF
    entries = (f.astype(np.uint64) << np.uint64(8)) | (np.array(bits, dtype=np.uint64) << np.uint64(16))
    got = {}
    for form in ("packed", "wide"):
        ctx = vgmi.Context(0, buffer_mib=16)
        try:
            if form == "packed":
                ctx.hmm_entries_upload(entries, cov, alive0)
                sup = ctx.hmm_support(n_hap, N_WINDOWS, entry_begin, counts, row_win)
                emit = ctx.hmm_emissions_select(pa, pb, win_used, _masks(win_used, bit_len)[:, 0], bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0)
                alive = ctx.hmm_alive_fetch()
                fixed = ctx.hmm_emissions_select(pa, pb, win_used, _masks(win_used, bit_len)[:, 0], bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win,
                                                 gt0, fixes=fix)
                tal = ctx.hmm_tallies_select(entry_begin, counts, row_win, winner, pa, pb, win_used)
            else:
                ctx.hmm_entries_upload_wide(f, _bytes_of(bits, bit_len), bit_len, cov, alive0)
                sup = ctx.hmm_support_wide(bit_len, n_hap, N_WINDOWS, entry_begin, counts, row_win)
                emit = ctx.hmm_emissions_select_wide(pa, pb, win_used, _masks(win_used, bit_len), bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0)
                alive = ctx.hmm_alive_fetch()
                fixed = ctx.hmm_emissions_select_wide(pa, pb, win_used, _masks(win_used, bit_len), bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win,
                                                      gt0, fixes=fix)
                tal = ctx.hmm_tallies_select_wide(bit_len, entry_begin, counts, row_win, winner, pa, pb, win_used)
            got[form] = [sup, *emit, alive, *fixed, *tal, ctx.hmm_alive_fetch()]
        finally:
            ctx.close()
    assert len(got["packed"]) == len(got["wide"]) == 11
    for i, (a, b) in enumerate(zip(got["packed"], got["wide"])):
        assert a.dtype == b.dtype and np.array_equal(a, b), i
    sup, obs, n_kept, flags, alive, obs_f = got["wide"][:6]
    assert sup.any() and (obs > 0).any() and (n_kept > 0).sum() > n_rows // 2 and flags[90] & 1 and (alive != alive0).any() and not np.array_equal(obs_f[90], obs[90])


def test_wide_calls_refuse_what_they_cannot_take_and_serve_on():
    """Every refusal of the _wide entry points -- VGMI_E_INVALID: bit_len 0 and 33, more haplotypes than 8 bit_len - 1, a selected id at
    8 bit_len - 1, n_used 0 and 17, n_gt 0 and 129, a genotype outside the list, a row outside the entries, a row in a window that does not
    exist; VGMI_E_STATE: a _wide call on packed entries or on none, a packed call on _wide entries, a _wide call with another bit_len than
    the upload's -- and after each of them a valid call that returns what it returned before."""
    rng = np.random.default_rng(5)
    bit_len, n_hap, n_used, n_rows = 9, 71, 5, 30
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, n_rows, fixed={})
    row_win = np.repeat(np.arange(3), 10).astype(np.uint32)
    win_used = np.array([[0, 5, 63, 64, 70], [1, 2, 3, 62, 69], [4, 6, 8, 65, 68]], dtype=np.uint8)
    masks = _masks(win_used, bit_len)
    pairs = list(itertools.combinations_with_replacement(range(n_used), 2))
    pa, pb = [a for a, _ in pairs], [b for _, b in pairs]
    gt0 = np.zeros(n_rows, dtype=np.uint16)
    tables = rng.random(768).astype(LD) + LD(0.05)
    winner = np.zeros(n_rows, dtype=np.uint32)
    raw = _bytes_of(bits, bit_len)
    n_entries = len(bits)
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        def emit(c=ctx, **kw):
            a = dict(pos_a=pa, pos_b=pb, win_used=win_used, win_top_mask=masks, bit_len=bit_len, ave=AVE, lower=LOWER, upper=UPPER, tables=tables,
                     entry_begin=entry_begin, entry_count=counts, row_win=row_win, gt0=gt0)
            a.update(kw)
            return c.hmm_emissions_select_wide(**a)

        def tally(**kw):
            a = dict(bit_len=bit_len, entry_begin=entry_begin, entry_count=counts, row_win=row_win, winner=winner, pos_a=pa, pos_b=pb, win_used=win_used)
            a.update(kw)
            return ctx.hmm_tallies_select_wide(**a)

        def support(**kw):
            a = dict(bit_len=bit_len, n_hap=n_hap, n_windows=3, entry_begin=entry_begin, entry_count=counts, row_win=row_win)
            a.update(kw)
            return ctx.hmm_support_wide(**a)

        # nothing uploaded yet: a state error, not a fault
        with pytest.raises(vgmi.VgmiError) as err:
            support()
        assert err.value.code == vgmi.E_STATE
        ctx.hmm_entries_upload_wide(f, raw, bit_len, cov)
        emit()      # (the selection prunes the lists once; from here on every valid call finds the state it left)
        good = support()
        good_obs = emit()
        good_tally = tally()

        def serves_on():
            assert np.array_equal(support(), good)
            again = emit()
            assert all(np.array_equal(a, b) for a, b in zip(again, good_obs))
            assert all(np.array_equal(a, b) for a, b in zip(tally(), good_tally))

        def refused(code, call):
            with pytest.raises(vgmi.VgmiError) as err:
                call()
            assert err.value.code == code, (err.value.code, str(err.value))
            serves_on()

        beyond = entry_begin.copy()
        beyond[-1] = n_entries
        counts_beyond = counts.copy()
        counts_beyond[-1] = 1
        bad_win = row_win.copy()
        bad_win[4] = 3
        at_flag = win_used.copy()
        at_flag[1, 4] = 8 * bit_len - 1
        pairs129 = (pairs * 9)[:129]
        for code, call in [
                (vgmi.E_INVALID, lambda: support(n_hap=8 * bit_len)),
                (vgmi.E_INVALID, lambda: support(n_hap=0)),
                (vgmi.E_INVALID, lambda: support(bit_len=0)),
                (vgmi.E_INVALID, lambda: support(bit_len=33)),
                (vgmi.E_STATE, lambda: support(bit_len=10)),
                (vgmi.E_INVALID, lambda: support(entry_begin=beyond, entry_count=counts_beyond)),
                (vgmi.E_INVALID, lambda: support(row_win=bad_win)),
                (vgmi.E_INVALID, lambda: emit(win_used=at_flag)),
                (vgmi.E_INVALID, lambda: emit(win_used=np.zeros((3, 0), dtype=np.uint8))),
                (vgmi.E_INVALID, lambda: emit(win_used=np.tile(np.arange(17, dtype=np.uint8), (3, 1)))),
                (vgmi.E_INVALID, lambda: emit(pos_a=[], pos_b=[])),
                (vgmi.E_INVALID, lambda: emit(pos_a=[a for a, _ in pairs129], pos_b=[b for _, b in pairs129])),
                (vgmi.E_INVALID, lambda: emit(pos_a=[n_used] + pa[1:])),
                (vgmi.E_INVALID, lambda: emit(bit_len=0)),
                (vgmi.E_INVALID, lambda: emit(bit_len=33)),
                (vgmi.E_STATE, lambda: emit(bit_len=12)),
                (vgmi.E_INVALID, lambda: emit(entry_begin=beyond, entry_count=counts_beyond)),
                (vgmi.E_INVALID, lambda: emit(row_win=bad_win)),
                (vgmi.E_INVALID, lambda: tally(win_used=at_flag)),
                (vgmi.E_INVALID, lambda: tally(win_used=np.zeros((3, 0), dtype=np.uint8))),
                (vgmi.E_INVALID, lambda: tally(win_used=np.tile(np.arange(17, dtype=np.uint8), (3, 1)))),
                (vgmi.E_INVALID, lambda: tally(pos_a=[], pos_b=[])),
                (vgmi.E_INVALID, lambda: tally(pos_a=[a for a, _ in pairs129], pos_b=[b for _, b in pairs129])),
                (vgmi.E_INVALID, lambda: tally(bit_len=33)),
                (vgmi.E_STATE, lambda: tally(bit_len=8)),
                (vgmi.E_INVALID, lambda: tally(entry_begin=beyond, entry_count=counts_beyond)),
                (vgmi.E_INVALID, lambda: tally(row_win=bad_win)),
                # the packed calls on entries uploaded as bytes
                (vgmi.E_STATE, lambda: ctx.hmm_support(47, 3, entry_begin, counts, row_win)),
                (vgmi.E_STATE, lambda: ctx.hmm_emissions_select(pa, pb, win_used % 40, masks[:, 0], 6, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0)),
                (vgmi.E_STATE, lambda: ctx.hmm_tallies_select(entry_begin, counts, row_win, winner, pa, pb, win_used % 40))]:
            refused(code, call)
        # an upload that is refused leaves the context's entries as they were
        for bad_len in (0, 33):
            refused(vgmi.E_INVALID, lambda: ctx.hmm_entries_upload_wide(f, np.zeros((n_entries, max(bad_len, 1)), dtype=np.uint8), bad_len))
        # a replaced table, either way: packed entries refuse the _wide calls, and the reverse again
        ctx.hmm_entries_upload(np.zeros(n_entries, dtype=np.uint64), cov)
        for call in (support, emit, tally):
            with pytest.raises(vgmi.VgmiError) as err:
                call()
            assert err.value.code == vgmi.E_STATE
        assert not ctx.hmm_support(47, 3, entry_begin, counts, row_win).any()
        ctx.hmm_entries_upload_wide(f, raw, bit_len, cov)
        emit()      # (every entry is alive again: the selection prunes once more)
        serves_on()
    finally:
        ctx.close()


# ---- the command line: a cohort of 26 diploid samples (53 haplotypes, seven bytes of haplotype bits per entry) -------------------------
SELECTED = r"HMM emissions on the device: .*haplotypes selected per window for (\d+) of (\d+) windows"
BITS = r"HMM haplotype bits on the device: (\d+) bytes per entry"


def _cohort(work, n_samples, whos, sv_frac):
    from test_gpu_configs import CLI, ENV, _need_binaries, _write_fastq
    from varigraph_amd import synth
    _need_binaries()
    ref = synth.make_reference(150_000)
    variants, gts = synth.make_cohort(ref, 250, n_samples=n_samples, ploidy=2, seed=4, indel_frac=0.1, sv_frac=sv_frac)
    fa, vcf = os.path.join(work, "ref.fa"), os.path.join(work, "in.vcf")
    synth.write_fasta(fa, "chr1", ref)
    synth.write_vcf(vcf, "chr1", len(ref), variants, gts, n_samples, 2)
    graph = os.path.join(work, "graph.bin")
    r = subprocess.run([CLI, "construct", "-r", fa, "-v", vcf, "--save-graph", graph, "-t", "16", "--gpu", "0"], cwd=work, capture_output=True, text=True,
                       env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    cfg = []
    for i, who in enumerate(whos):
        fq = _write_fastq(os.path.join(work, f"s{i}"), synth.sample_haplotypes(ref, variants, gts, who, 2), 25_000, seed=8 + i)
        cfg.append(f"ind{i} " + " ".join(fq) + "\n")
    return graph, cfg


@pytest.fixture(scope="module")
def wide_cohort(tmp_path_factory):
    """150 kb, 250 sites, 26 diploid samples, seed 4, 25 000 read pairs per sample: the parameters test_wide_panel_of_53_haplotypes_identical
    holds to more than 100 VCF lines -- but four sites in ten are insertions of 60..300 bp, not one in a hundred: with two or three such
    sites `--sv` has nothing to compare (12 VCF lines)."""
    work = str(tmp_path_factory.mktemp("wide_cli"))
    graph, cfg = _cohort(work, 26, (3, 7, 11), 0.4)
    yield work, graph, cfg
    shutil.rmtree(work, ignore_errors=True)


def _genotype(work, graph, cfg, tag, exe, opts, env):
    from test_gpu_configs import REF, _run, _vcf
    d = os.path.join(work, tag)
    os.makedirs(d, exist_ok=True)
    open(os.path.join(d, "samples.cfg"), "w").write("".join(cfg))
    more = [] if exe == REF else ["--gpu", "0"]
    r = _run([exe, "genotype", "--load-graph", graph, "-s", "samples.cfg", "-t", "6"] + opts + more, cwd=d, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (tag, r.stderr[-2000:])
    return [_vcf(d, f"ind{i}") for i in range(len(cfg))], r.stderr


CASES = {"n15": (["-n", "15"], 1), "n5_depth_3_samples": (["-n", "5", "--use-depth"], 3), "n5_sv": (["-n", "5", "--sv"], 1),
         "n5_hom": (["-n", "5", "-g", "hom"], 1), "fre_n5": (["-m", "fre", "-n", "5"], 1)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_command_line_over_53_haplotypes_on_the_selected_path_equals_the_reference(case, wide_cohort):
    """`varigraph-mi genotype` over the 53-haplotype graph, byte for byte the deterministic reference build's VCFs: -n 15; -n 5 --use-depth with
    three samples in one run (the pruned lists carry over); -n 5 --sv; -n 5 -g hom; -m fre -n 5 -- each also with VGH_HMM_WIDE_DEVICE=0 (the
    parent's path), VGH_HMM_SELECT_DEVICE=0, VGH_DEVICE_TALLIES=0, VGH_HMM_FIX_DEVICE=0 (flagged rows scored by the host's hidden_states,
    which reads the bit vectors) and VGH_HMM_FAKE_NOMEM=1 (the first sample takes the pool, the next ones start from the host's lists).  The default run's log carries the selected-path line for every window of every sample and the
    `haplotype bits on the device: 7 bytes` line once; with VGH_HMM_WIDE_DEVICE=0 it carries neither.
    Reference VCF lines, counted on the CPU with the host twin of the read generator before these parameters were fixed: -n 15: 197;
    -n 5 --use-depth: 197, 197, 205; -n 5 --sv: 89; -n 5 -g hom: 164; -m fre -n 5: 197 (at least 50 each: the comparison must not be of
    empty files)."""
    from test_gpu_configs import CLI, ENV, REF
    work, graph, cfg = wide_cohort
    opts, n = CASES[case]
    opts = opts + ["--granularity", "0.04"]      # windows of 40 kb: four of them
    timing = dict(ENV, VGH_TIMING="1")
    want, _ = _genotype(work, graph, cfg[:n], f"{case}_cpu", REF, opts, ENV)
    lines = [v.count(b"\n") for v in want]
    print(f"{case}: reference VCF lines {lines}")
    assert min(lines) >= 50, lines
    logs = {}
    for name, env in (("native", timing), ("parent_path", dict(timing, VGH_HMM_WIDE_DEVICE="0")), ("host_select", dict(timing, VGH_HMM_SELECT_DEVICE="0")),
                      ("host_tallies", dict(timing, VGH_DEVICE_TALLIES="0")), ("host_fixes", dict(timing, VGH_HMM_FIX_DEVICE="0")),
                      ("fake_nomem", dict(timing, VGH_HMM_FAKE_NOMEM="1"))):
        got, logs[name] = _genotype(work, graph, cfg[:n], f"{case}_{name}", CLI, opts, env)
        for i in range(n):
            assert got[i] == want[i], (case, name, i)
    for name in ("native", "host_tallies", "host_fixes"):
        seen = re.findall(SELECTED, logs[name])
        assert len(seen) == n and all(a == b and int(b) >= 4 for a, b in seen), (name, seen)
        assert re.findall(BITS, logs[name]) == ["7"], name
    for name in ("parent_path", "host_select"):
        assert not re.search(SELECTED, logs[name]) and not re.search(BITS, logs[name]), name
    # as if the device had no room for the first sample: it takes the pool, the others the selected path on the host's lists
    assert len(re.findall(SELECTED, logs["fake_nomem"])) == n - 1 and len(re.findall(BITS, logs["fake_nomem"])) == min(1, n - 1)


def test_command_line_over_67_haplotypes_takes_two_words_per_entry(tmp_path_factory):
    """A cohort of 33 diploid samples -- 67 haplotypes, nine bytes of haplotype bits, W = 2 on the device -- with -n 5 --use-depth: the
    reference's VCF byte for byte (194 lines when counted on the CPU), the selected path for every window, `9 bytes per entry` once."""
    from test_gpu_configs import CLI, ENV, REF
    work = str(tmp_path_factory.mktemp("wide_cli_67"))
    try:
        graph, cfg = _cohort(work, 33, (3,), 0.01)
        opts = ["-n", "5", "--use-depth", "--granularity", "0.04"]
        want, _ = _genotype(work, graph, cfg, "cpu", REF, opts, ENV)
        assert want[0].count(b"\n") >= 50, want[0].count(b"\n")
        got, log = _genotype(work, graph, cfg, "native", CLI, opts, dict(ENV, VGH_TIMING="1"))
        assert got[0] == want[0]
        seen = re.findall(SELECTED, log)
        assert len(seen) == 1 and seen[0][0] == seen[0][1] and int(seen[0][1]) >= 4, seen
        assert re.findall(BITS, log) == ["9"]
    finally:
        shutil.rmtree(work, ignore_errors=True)


@pytest.mark.parametrize("opts", [["-n", "28"], ["--sample-ploidy", "4", "-n", "5"]], ids=["n28", "tetraploid_n5"])
def test_what_stays_out_of_scope_keeps_the_pool(opts, wide_cohort):
    """-n above 16 and a polyploid sample over the 53-haplotype graph keep the parent's path, the pool: the host prepares every window (the
    `HMM thread-seconds` line without the `host thread-seconds around the device` line that only the two emission paths print), no
    selected-path line, no haplotype bits on the device.  With -n 28 every window has the announced 406 genotypes and the pool's parts run
    their recursion on the device (`HMM part ... on the device from`); a tetraploid sample's windows have lists of 1 .. 5 blocks, and the
    pool hands over only those whose length is the announced one -- possibly none, so that line is not asked of it."""
    from test_gpu_configs import CLI, ENV
    work, graph, cfg = wide_cohort
    _, log = _genotype(work, graph, cfg[:1], "pool_" + "_".join(o.strip("-") for o in opts), CLI, opts + ["--granularity", "0.04"], dict(ENV, VGH_TIMING="1"))
    assert not re.search(SELECTED, log) and not re.search(BITS, log)
    assert "HMM thread-seconds: selection" in log and "host thread-seconds around the device" not in log
    if opts[0] == "-n":
        assert re.search(r"HMM part \d+ \(windows \d+-\d+\): on the device from", log)
