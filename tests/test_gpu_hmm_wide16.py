"""A diploid sample over a panel of 255 to 511 haplotypes on the device (vgmi_hmm_*_wide16: 33 to 64 bytes of haplotype bits per entry, eight
words on the device, the drawn haplotypes of a window as 16-bit ids): support, emission scores with the prune, alive bytes and tallies
against the same computation spelled out in Python integers (products in numpy.longdouble, the x87 format, bit for bit); ids that differ
only above bit 8; more support counters than a workgroup has lanes; the _wide16 calls against the _wide ones on a panel both can hold; and
every refusal, with the table replaced in each direction."""
import itertools

import numpy as np
import pytest

from varigraph_amd import vgmi
from test_gpu_hmm_select import AVE, LOWER, UPPER, _model_emissions
from test_gpu_hmm_wide import _bytes_of, _model_support, _model_tallies, _panel
from test_gpu_hmm_wide import _masks as _masks_wide

pytestmark = pytest.mark.gpu
LD = np.longdouble
N_WINDOWS, PER_WINDOW = 3, 40
W = 8


def _masks(win_used):
    """(n_windows, 8) uint64: word i of a window holds its haplotypes 64 i .. 64 i + 63"""
    m = np.zeros((len(win_used), W), dtype=np.uint64)
    for w, used in enumerate(win_used):
        for h in used:
            m[w, int(h) >> 6] |= np.uint64(1) << np.uint64(int(h) & 63)
    return m


def _tables(rng):
    return (rng.random(768).astype(LD) + LD(0.05)) * np.power(LD(10), rng.integers(-300, 1, size=768).astype(LD))


def _pairs(n_used):
    pairs = list(itertools.combinations_with_replacement(range(n_used), 2))
    return pairs, [a for a, _ in pairs], [b for _, b in pairs]


# bit_len -> (haplotypes, ids the selections must hold)
WIDTHS = {33: (263, [255, 256, 262]), 40: (319, [63, 64, 318]), 41: (327, [319, 320, 326]), 56: (447, [383, 384, 446]),
          64: (511, [0, 255, 256, 447, 448, 510])}


@pytest.mark.parametrize("n_used", [5, 15])
@pytest.mark.parametrize("bit_len", sorted(WIDTHS))
def test_wide16_kernels_equal_the_host_arithmetic_at_every_width(bit_len, n_used):
    """Support, emissions (with the prune, a fixed row, a second sample on the pruned lists), alive bytes and tallies of the _wide16 calls
    against the model, array_equal throughout: 33 bytes (263 haplotypes: ids 255 and 256, the first that no byte holds, and 262), 40 (ids 63,
    64, 318; five whole words), 41 (319, 320, 326: the first byte of the sixth word), 56 (383, 384, 446) and 64 (0, 255, 256, 447, 448, 510;
    the flag at bit 511); 5 and 15 selected haplotypes (15 and 120 genotypes).  The listed ids stand in the first window's selection -- at 64
    bytes with 5 selected the sixth of them, 510, in the second window's.  120 rows in three windows: an empty row, a row that dies in the
    prune, a row with dead entries on entry, an entry only a haplotype of word 4 carries and one only the panel's top word's haplotype carries
    (word 7 at 64 bytes; both stay), an entry whose only set bit is the last bit (it leaves the list: the last bit is no haplotype) and a
    flagged row scored again with a fix."""
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    n_hap, must = WIDTHS[bit_len]
    assert n_hap <= 8 * bit_len - 1 and max(must) <= 8 * bit_len - 2
    top_word = (n_hap - 1) >> 6
    assert top_word >= 4 and (bit_len != 64 or top_word == 7)
    rng = np.random.default_rng(100 * bit_len + n_used)
    n_rows = N_WINDOWS * PER_WINDOW
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, n_rows, fixed={3: 20, 5: 0, 50: 30, 60: 6, 90: 25})
    row_win = np.repeat(np.arange(N_WINDOWS), PER_WINDOW).astype(np.uint32)

    def selection(first):
        sel = []
        for w in range(N_WINDOWS):      # every window holds a haplotype of the top word and one of word 4
            base = list(first[:n_used]) if w == 0 else list(first[n_used:]) * (w == 1) + [n_hap - 1 - w, 256 + w]
            others = [h for h in range(n_hap) if h not in base]
            sel.append(sorted(base + [int(h) for h in rng.choice(others, size=n_used - len(base), replace=False)]))
        return np.array(sel, dtype=np.uint16)
    win_used = selection(must)
    assert all((win_used == h).any() for h in must) and (win_used >> 6 == top_word).any(axis=1)[1:].all() and (win_used >> 6 == 4).any(axis=1)[1:].all()
    assert (win_used > 255).any(axis=1).all()
    masks = _masks(win_used)
    int_mask = [sum(1 << int(h) for h in u) for u in win_used]
    pairs, pa, pb = _pairs(n_used)
    assert len(pairs) == (15 if n_used == 5 else 120)
    gt0 = rng.integers(0, 1 << n_used, size=n_rows).astype(np.uint16)
    tables = _tables(rng)
    last_bit = 1 << (8 * bit_len - 1)
    e = [int(x) for x in entry_begin]
    # row 3: no entry carries a haplotype of its window; row 50: half its entries dead on entry; row 60 (window 1): entry 0 is carried by the
    # window's top-word haplotype alone, entry 1 has the last bit alone, entry 2 the last bit and haplotypes outside the selection, entry 3
    # is carried by the window's haplotype of word 4 alone; row 90: entry 2 is an under-covered multi-copy k-mer that the window's first two
    # haplotypes carry
    for j in range(e[3], e[3] + 20):
        bits[j] &= ~int_mask[0]
    alive0 = (rng.random(len(bits)) < 0.9).astype(np.uint8)
    alive0[e[50]:e[50] + 30:2] = 0
    top_hap = int(win_used[1].max())
    assert top_hap >> 6 == top_word
    outside = [h for h in range(n_hap) if h not in win_used[1]][:3]
    bits[e[60]], bits[e[60] + 1], bits[e[60] + 2], bits[e[60] + 3] = 1 << top_hap, last_bit, last_bit | sum(1 << h for h in outside), 1 << 257
    assert 257 in win_used[1]
    alive0[e[60]:e[60] + 4] = 1
    cov[e[60]:e[60] + 4] = 23
    j90 = e[90] + 2
    alive0[j90] = 1
    cov[j90], f[j90] = 1, 2
    bits[j90] |= (1 << int(win_used[2][0])) | (1 << int(win_used[2][1]))
    gt0[90] = 0
    fixes = {(90, 2): 0b01}
    win_used2 = selection([n_hap - 1, 256])
    masks2 = _masks(win_used2)
    winner = rng.integers(0, len(pairs), size=n_rows).astype(np.uint32)
    winner[::9] = 0xFFFFFFFF

    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        ctx.hmm_entries_upload_wide16(f, _bytes_of(bits, bit_len), bit_len, cov, alive0)
        support = ctx.hmm_support_wide16(bit_len, n_hap, N_WINDOWS, entry_begin, counts, row_win)
        obs, n_kept, flags = ctx.hmm_emissions_select_wide16(pa, pb, win_used, masks, bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0)
        alive1 = ctx.hmm_alive_fetch()
        support1 = ctx.hmm_support_wide16(bit_len, n_hap, N_WINDOWS, entry_begin, counts, row_win)
        tally, uniq = ctx.hmm_tallies_select_wide16(bit_len, entry_begin, counts, row_win, winner, pa, pb, win_used)
        # the same selection once more with the flagged row scored again: nothing further dies, the other rows keep their scores
        obs_f, n_kept_f, flags_f = ctx.hmm_emissions_select_wide16(pa, pb, win_used, masks, bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win,
                                                                   gt0, fixes=([90], [0, 1], [2], [fixes[(90, 2)]]))
        alive1b = ctx.hmm_alive_fetch()
        # the next sample: other haplotypes per window, the lists as the first sample left them
        obs2, n_kept2, flags2 = ctx.hmm_emissions_select_wide16(pa, pb, win_used2, masks2, bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0)
        alive2 = ctx.hmm_alive_fetch()
        tally2, uniq2 = ctx.hmm_tallies_select_wide16(bit_len, entry_begin, counts, row_win, winner, pa, pb, win_used2)
    finally:
        ctx.close()

    assert np.array_equal(support.astype(np.uint64), _model_support(f, bits, cov, alive0, n_hap, N_WINDOWS, entry_begin, counts, row_win))
    assert support[:, n_hap - 1].all() and support[0, [h for h in must if h in win_used[0]]].all() and support[:, 256:].any(axis=1).all()
    m_alive = alive0.copy()
    want, want_kept, want_flags = _model_emissions(f, bits, cov, m_alive, bit_len, pairs, win_used, tables, entry_begin, counts, row_win, gt0)
    assert np.array_equal(n_kept, want_kept) and np.array_equal(flags, want_flags)
    for r in range(n_rows):
        assert np.array_equal(obs[r], want[r]), (r, int(np.argmax(obs[r] != want[r])))
    assert np.array_equal(alive1, m_alive)
    assert n_kept[3] == 0 and not alive1[e[3]:e[3] + 20].any() and (obs[3] == 1).all()
    assert n_kept[5] == 0 and (obs[5] == 1).all()
    assert alive1[e[60]] == 1 and alive1[e[60] + 1] == 0 and alive1[e[60] + 2] == 0 and alive1[e[60] + 3] == 1
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


def test_wide16_ids_that_differ_only_above_bit_8_are_told_apart():
    """Window 0 draws haplotype 256 and not 0, window 1 draws 0 and not 256 (the other three ids are the same in both), and every entry carries
    haplotype 0 alone or haplotype 256 alone.  Support, kept counts, observations, alive bytes and tallies equal the model -- and the model
    with the ids cut to a byte gives other numbers for each of them, so a kernel that read win_used through a byte would be seen."""
    rng = np.random.default_rng(256)
    bit_len, n_hap, n_rows = 33, 263, 24
    counts = np.full(n_rows, 12, dtype=np.uint32)
    entry_begin = (np.arange(n_rows) * 12).astype(np.uint64)
    n_entries = n_rows * 12
    only0 = rng.random(n_entries) < 0.5
    bits = [1 if z else 1 << 256 for z in only0]
    f = np.ones(n_entries, dtype=np.uint8)
    cov = rng.choice([14, 20, 23, 30], size=n_entries).astype(np.uint8)
    alive0 = np.ones(n_entries, dtype=np.uint8)
    row_win = np.repeat(np.arange(2), n_rows // 2).astype(np.uint32)
    win_used = np.array([[7, 100, 256, 260], [0, 7, 100, 260]], dtype=np.uint16)
    pairs, pa, pb = _pairs(4)
    gt0 = np.zeros(n_rows, dtype=np.uint16)
    tables = _tables(rng)
    winner = np.array([pairs.index((2, 2)) if w == 0 else pairs.index((0, 0)) for w in row_win], dtype=np.uint32)      # the called pair: (256, 256) or (0, 0)
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        ctx.hmm_entries_upload_wide16(f, _bytes_of(bits, bit_len), bit_len, cov, alive0)
        support = ctx.hmm_support_wide16(bit_len, n_hap, 2, entry_begin, counts, row_win)
        obs, n_kept, flags = ctx.hmm_emissions_select_wide16(pa, pb, win_used, _masks(win_used), bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0)
        alive1 = ctx.hmm_alive_fetch()
        tally, uniq = ctx.hmm_tallies_select_wide16(bit_len, entry_begin, counts, row_win, winner, pa, pb, win_used)
    finally:
        ctx.close()
    assert np.array_equal(support.astype(np.uint64), _model_support(f, bits, cov, alive0, n_hap, 2, entry_begin, counts, row_win))
    assert support[:, 0].all() and support[:, 256].all() and not np.array_equal(support[:, 0], support[:, 256]) and not np.delete(support, [0, 256], axis=1).any()
    m_alive = alive0.copy()
    want, want_kept, want_flags = _model_emissions(f, bits, cov, m_alive, bit_len, pairs, win_used, tables, entry_begin, counts, row_win, gt0)
    assert np.array_equal(n_kept, want_kept) and np.array_equal(flags, want_flags) and np.array_equal(obs, want) and np.array_equal(alive1, m_alive)
    # window 0 keeps exactly the entries of haplotype 256, window 1 those of haplotype 0
    for r in range(n_rows):
        mine = ~only0[12 * r:12 * r + 12] if row_win[r] == 0 else only0[12 * r:12 * r + 12]
        assert n_kept[r] == mine.sum() and np.array_equal(alive1[12 * r:12 * r + 12], mine.astype(np.uint8))
    want_t, want_u = _model_tallies(f, bits, cov, alive1, pairs, win_used, entry_begin, counts, row_win, winner)
    assert np.array_equal(tally, want_t) and np.array_equal(uniq, want_u) and np.array_equal(tally[:, 0], n_kept) and tally[:, 1].all()
    # what ids cut to a byte would have given: 256 reads as 0 (and 260 as 4) -- the observations and the tallies differ (the prune is by the mask)
    cut = (win_used & 0xFF).astype(np.uint16)
    cut_obs, _, _ = _model_emissions(f, bits, cov, alive0.copy(), bit_len, pairs, cut, tables, entry_begin, counts, row_win, gt0, prune=False)
    cut_t, _ = _model_tallies(f, bits, cov, alive1, pairs, cut, entry_begin, counts, row_win, winner)
    assert not np.array_equal(cut_obs[row_win == 0], obs[row_win == 0]) and not np.array_equal(cut_t[row_win == 0], tally[row_win == 0])


@pytest.mark.parametrize("bit_len,n_hap", [(33, 261), (64, 511)])
def test_wide16_support_beyond_256_counters(bit_len, n_hap):
    """More counters than the workgroup has lanes: 261 and 511 haplotypes with coverage on ids 256 to 510 (every id of the panel is carried
    somewhere).  100 rows, windows changing at rows 30 and 70: two windows meet inside each 64-row workgroup, so its counters are zeroed and
    written out twice."""
    rng = np.random.default_rng(bit_len)
    n_rows = 100
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, n_rows, fixed={})
    f[:] = 1
    cov[:] = rng.integers(2, 60, size=len(bits))
    for h in range(n_hap):      # every haplotype in every window
        for lo, hi in ((0, 30), (30, 70), (70, 100)):
            r = int(rng.integers(lo, hi))
            while counts[r] == 0:
                r = lo + (r + 1 - lo) % (hi - lo)
            bits[int(entry_begin[r]) + int(rng.integers(0, counts[r]))] |= 1 << h
    alive = (rng.random(len(bits)) < 0.95).astype(np.uint8)
    row_win = np.array([0] * 30 + [1] * 40 + [2] * 30, dtype=np.uint32)
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        ctx.hmm_entries_upload_wide16(f, _bytes_of(bits, bit_len), bit_len, cov, alive)
        support = ctx.hmm_support_wide16(bit_len, n_hap, 3, entry_begin, counts, row_win)
    finally:
        ctx.close()
    assert support.shape == (3, n_hap)
    assert np.array_equal(support.astype(np.uint64), _model_support(f, bits, cov, alive, n_hap, 3, entry_begin, counts, row_win))
    assert (support[:, 256:] > 0).mean() > 0.8 and support[:, n_hap - 1].any()


def test_wide16_calls_return_the_wide_calls_bytes_on_a_panel_both_hold():
    """A 17-byte panel of 135 haplotypes, and the same entries in 40-byte vectors: the same haplotype bits, the flag moved from bit 135 to bit
    319.  The _wide16 calls return the _wide calls' bytes: support over 135 haplotypes, n_kept, flags, the part's scores (with a fixed row),
    alive bytes and tallies."""
    rng = np.random.default_rng(1740)
    n_hap, n_used, n_rows = 135, 5, N_WINDOWS * PER_WINDOW
    counts, entry_begin, f, bits17, cov = _panel(rng, n_hap, 17, n_rows, fixed={3: 20, 90: 25})
    row_win = np.repeat(np.arange(N_WINDOWS), PER_WINDOW).astype(np.uint32)
    win_used = np.array([sorted([n_hap - 1 - w] + [int(h) for h in rng.choice(n_hap - 4, size=n_used - 1, replace=False)]) for w in range(N_WINDOWS)])
    pairs, pa, pb = _pairs(n_used)
    gt0 = rng.integers(0, 1 << n_used, size=n_rows).astype(np.uint16)
    tables = _tables(rng)
    alive0 = (rng.random(len(bits17)) < 0.9).astype(np.uint8)
    j90 = int(entry_begin[90]) + 2
    alive0[j90], cov[j90], f[j90] = 1, 1, 2
    bits17[j90] |= (1 << int(win_used[2][0])) | (1 << int(win_used[2][1]))
    gt0[90] = 0
    fix = ([90], [0, 1], [2], [0b10])
    winner = rng.integers(0, len(pairs), size=n_rows).astype(np.uint32)
    winner[::7] = 0xFFFFFFFF
    flag17, flag40 = 1 << 135, 1 << 319
    bits40 = [(b & ~flag17) | (flag40 if b & flag17 else 0) for b in bits17]
    assert any(b & flag17 for b in bits17) and all(b >> 135 in (0, 1) for b in bits17)
    got = {}
    for form in ("wide", "wide16"):
        ctx = vgmi.Context(0, buffer_mib=16)
        try:
            if form == "wide":
                m = _masks_wide(win_used, 17)
                ctx.hmm_entries_upload_wide(f, _bytes_of(bits17, 17), 17, cov, alive0)
                sup = ctx.hmm_support_wide(17, n_hap, N_WINDOWS, entry_begin, counts, row_win)
                emit = ctx.hmm_emissions_select_wide(pa, pb, win_used, m, 17, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0)
                alive = ctx.hmm_alive_fetch()
                fixed = ctx.hmm_emissions_select_wide(pa, pb, win_used, m, 17, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0, fixes=fix)
                tal = ctx.hmm_tallies_select_wide(17, entry_begin, counts, row_win, winner, pa, pb, win_used)
            else:
                m = _masks(win_used)
                ctx.hmm_entries_upload_wide16(f, _bytes_of(bits40, 40), 40, cov, alive0)
                sup = ctx.hmm_support_wide16(40, n_hap, N_WINDOWS, entry_begin, counts, row_win)
                emit = ctx.hmm_emissions_select_wide16(pa, pb, win_used, m, 40, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0)
                alive = ctx.hmm_alive_fetch()
                fixed = ctx.hmm_emissions_select_wide16(pa, pb, win_used, m, 40, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0, fixes=fix)
                tal = ctx.hmm_tallies_select_wide16(40, entry_begin, counts, row_win, winner, pa, pb, win_used)
            got[form] = [sup, *emit, alive, *fixed, *tal, ctx.hmm_alive_fetch()]
        finally:
            ctx.close()
    assert len(got["wide"]) == len(got["wide16"]) == 11
    for i, (a, b) in enumerate(zip(got["wide"], got["wide16"])):
        assert a.dtype == b.dtype and np.array_equal(a, b), i
    sup, obs, n_kept, flags, alive, obs_f = got["wide16"][:6]
    assert sup.any() and (obs > 0).any() and (n_kept > 0).sum() > n_rows // 2 and flags[90] & 1 and (alive != alive0).any() and not np.array_equal(obs_f[90], obs[90])


def test_wide16_calls_refuse_what_they_cannot_take_and_serve_on():
    """Every refusal of the _wide16 entry points -- VGMI_E_INVALID: bit_len 32 and 65, n_hap 0 and 8 bit_len, a selected id at 8 bit_len - 1,
    n_used 0 and 17, n_gt 0 and 129, a genotype outside the list, a row outside the entries, a row in a window that does not exist;
    VGMI_E_STATE: a _wide16 call on packed entries, on _wide entries or on none, a _wide or packed call on _wide16 entries, a _wide16 call with
    another bit_len than the upload's -- and after each of them a valid call that returns what it returned before.  A refused upload leaves
    the entries as they were; the table is replaced in each direction between packed, _wide and _wide16."""
    rng = np.random.default_rng(16)
    bit_len, n_hap, n_used, n_rows = 41, 327, 5, 30
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, n_rows, fixed={})
    row_win = np.repeat(np.arange(3), 10).astype(np.uint32)
    win_used = np.array([[0, 5, 255, 256, 326], [1, 2, 3, 319, 320], [4, 6, 8, 300, 325]], dtype=np.uint16)
    masks = _masks(win_used)
    pairs, pa, pb = _pairs(n_used)
    gt0 = np.zeros(n_rows, dtype=np.uint16)
    tables = rng.random(768).astype(LD) + LD(0.05)
    winner = np.zeros(n_rows, dtype=np.uint32)
    raw = _bytes_of(bits, bit_len)
    n_entries = len(bits)
    # a 9-byte panel over the same rows for the _wide family
    used9 = np.array([[0, 5, 63, 64, 70], [1, 2, 3, 62, 69], [4, 6, 8, 65, 68]], dtype=np.uint8)
    raw9 = _bytes_of([b & ((1 << 71) - 1) for b in bits], 9)
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        def emit(**kw):
            a = dict(pos_a=pa, pos_b=pb, win_used=win_used, win_top_mask=masks, bit_len=bit_len, ave=AVE, lower=LOWER, upper=UPPER, tables=tables,
                     entry_begin=entry_begin, entry_count=counts, row_win=row_win, gt0=gt0)
            a.update(kw)
            return ctx.hmm_emissions_select_wide16(**a)

        def tally(**kw):
            a = dict(bit_len=bit_len, entry_begin=entry_begin, entry_count=counts, row_win=row_win, winner=winner, pos_a=pa, pos_b=pb, win_used=win_used)
            a.update(kw)
            return ctx.hmm_tallies_select_wide16(**a)

        def support(**kw):
            a = dict(bit_len=bit_len, n_hap=n_hap, n_windows=3, entry_begin=entry_begin, entry_count=counts, row_win=row_win)
            a.update(kw)
            return ctx.hmm_support_wide16(**a)

        def wide_calls():      # the _wide family on a 9-byte table
            m9 = _masks_wide(used9, 9)
            return (lambda: ctx.hmm_support_wide(9, 71, 3, entry_begin, counts, row_win),
                    lambda: ctx.hmm_emissions_select_wide(pa, pb, used9, m9, 9, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0),
                    lambda: ctx.hmm_tallies_select_wide(9, entry_begin, counts, row_win, winner, pa, pb, used9))

        def packed_calls():
            return (lambda: ctx.hmm_support(47, 3, entry_begin, counts, row_win),
                    lambda: ctx.hmm_emissions_select(pa, pb, used9 % 40, np.zeros(3, dtype=np.uint64), 6, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0),
                    lambda: ctx.hmm_tallies_select(entry_begin, counts, row_win, winner, pa, pb, used9 % 40))

        def all_state_errors(calls):
            for call in calls:
                with pytest.raises(vgmi.VgmiError) as err:
                    call()
                assert err.value.code == vgmi.E_STATE, (err.value.code, str(err.value))

        all_state_errors((support, emit, tally))      # nothing uploaded yet: a state error, not a fault
        ctx.hmm_entries_upload_wide16(f, raw, bit_len, cov)
        fresh = support()      # (every entry alive)
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
        wide17 = np.zeros((3, 4), dtype=np.uint64)
        for code, call in [
                (vgmi.E_INVALID, lambda: support(n_hap=8 * bit_len)),
                (vgmi.E_INVALID, lambda: support(n_hap=0)),
                (vgmi.E_INVALID, lambda: support(bit_len=32)),
                (vgmi.E_INVALID, lambda: support(bit_len=65)),
                (vgmi.E_STATE, lambda: support(bit_len=42)),
                (vgmi.E_INVALID, lambda: support(entry_begin=beyond, entry_count=counts_beyond)),
                (vgmi.E_INVALID, lambda: support(row_win=bad_win)),
                (vgmi.E_INVALID, lambda: emit(win_used=at_flag)),
                (vgmi.E_INVALID, lambda: emit(win_used=np.zeros((3, 0), dtype=np.uint16))),
                (vgmi.E_INVALID, lambda: emit(win_used=np.tile(np.arange(17, dtype=np.uint16), (3, 1)))),
                (vgmi.E_INVALID, lambda: emit(pos_a=[], pos_b=[])),
                (vgmi.E_INVALID, lambda: emit(pos_a=[a for a, _ in pairs129], pos_b=[b for _, b in pairs129])),
                (vgmi.E_INVALID, lambda: emit(pos_a=[n_used] + pa[1:])),
                (vgmi.E_INVALID, lambda: emit(bit_len=32)),
                (vgmi.E_INVALID, lambda: emit(bit_len=65)),
                (vgmi.E_STATE, lambda: emit(bit_len=48)),
                (vgmi.E_INVALID, lambda: emit(entry_begin=beyond, entry_count=counts_beyond)),
                (vgmi.E_INVALID, lambda: emit(row_win=bad_win)),
                (vgmi.E_INVALID, lambda: tally(win_used=at_flag)),
                (vgmi.E_INVALID, lambda: tally(win_used=np.zeros((3, 0), dtype=np.uint16))),
                (vgmi.E_INVALID, lambda: tally(win_used=np.tile(np.arange(17, dtype=np.uint16), (3, 1)))),
                (vgmi.E_INVALID, lambda: tally(pos_a=[], pos_b=[])),
                (vgmi.E_INVALID, lambda: tally(pos_a=[a for a, _ in pairs129], pos_b=[b for _, b in pairs129])),
                (vgmi.E_INVALID, lambda: tally(bit_len=65)),
                (vgmi.E_STATE, lambda: tally(bit_len=33)),
                (vgmi.E_INVALID, lambda: tally(entry_begin=beyond, entry_count=counts_beyond)),
                (vgmi.E_INVALID, lambda: tally(row_win=bad_win)),
                # the _wide calls with a width of theirs, and the packed calls, on entries of the _wide16 upload
                (vgmi.E_STATE, lambda: ctx.hmm_emissions_select_wide(pa, pb, used9, wide17, 17, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0)),
                *[(vgmi.E_STATE, call) for call in wide_calls()],
                *[(vgmi.E_STATE, call) for call in packed_calls()]]:
            refused(code, call)
        # an upload that is refused leaves the context's entries as they were -- the _wide16 upload's and the _wide upload's bounds alike
        for bad_len in (32, 65):
            refused(vgmi.E_INVALID, lambda: ctx.hmm_entries_upload_wide16(f, np.zeros((n_entries, bad_len), dtype=np.uint8), bad_len))
        refused(vgmi.E_INVALID, lambda: ctx.hmm_entries_upload_wide(f, np.zeros((n_entries, 33), dtype=np.uint8), 33))
        # a replaced table in each direction: _wide16 -> packed -> _wide16 -> _wide -> packed -> _wide -> _wide16
        def now_wide16():
            ctx.hmm_entries_upload_wide16(f, raw, bit_len, cov)
            emit()      # (every entry is alive again: the selection prunes once more)
            serves_on()
            all_state_errors(wide_calls() + packed_calls())

        def now_packed():
            ctx.hmm_entries_upload(np.zeros(n_entries, dtype=np.uint64), cov)
            all_state_errors((support, emit, tally) + wide_calls())
            assert not ctx.hmm_support(47, 3, entry_begin, counts, row_win).any()

        def now_wide():
            ctx.hmm_entries_upload_wide(f, raw9, 9, cov)
            all_state_errors((support, emit, tally) + packed_calls())
            sup9 = ctx.hmm_support_wide(9, 71, 3, entry_begin, counts, row_win)
            assert np.array_equal(sup9, fresh[:, :71]) and sup9.any()      # (the same haplotype bits below 71, every entry alive again)

        for step in (now_packed, now_wide16, now_wide, now_packed, now_wide, now_wide16):
            step()
    finally:
        ctx.close()
