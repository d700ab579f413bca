"""A POLYPLOID sample over a panel of 48 to 254 haplotypes on the device (vgmi_hmm_emissions_select_ploidy_wide, its second launch
vgmi_hmm_part_fix_rows_ploidy_wide and vgmi_hmm_tallies_ploidy_wide: a genotype list per window by haplotype id, every mask over ids W = 1,
2 or 4 words): the kernels against the packed calls' numpy models fed Python integers of 8 * bit_len bits (products in numpy.longdouble, the
x87 format, bit for bit), the new calls against the packed ones on data both take, every refusal, and the command line over a 53- and a
69-haplotype tetraploid cohort against the deterministic build of the reference, byte for byte, with the log saying which path ran."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from varigraph_amd import vgmi
from test_gpu_hmm_select import AVE, LD, LOWER, UPPER
from test_gpu_hmm_select_ploidy import _blocks, _model
from test_gpu_hmm_wide import BITS, SELECTED, _bytes_of, _panel, _words

pytestmark = pytest.mark.gpu
PER_WINDOW = 35
TALLY_LINE = r"HMM tallies on the device: (\d+) rows, ploidy (\d+)"


def _split(x, W):
    """a Python integer as W 64-bit words, little-endian"""
    return [(int(x) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(W)]


def _word_rows(xs, W):
    return np.array([_split(x, W) for x in xs], dtype=np.uint64).reshape(len(xs), W)


def _mask_of(ids):
    m = 0
    for h in ids:
        m |= 1 << int(h)
    return m


def _max_hap(bit_len, ploidy):
    """the last haplotype: the largest id the width holds that is no multiple of the ploidy (its block is truncated); 254 at 32 bytes"""
    h = 8 * bit_len - 2
    while h % ploidy == 0:
        h -= 1
    return h


def _straddle(ploidy, max_hap):
    """haplotypes whose block(s) lie on both sides of a word boundary: a block that holds ids 64 b - 1 and 64 b where the ploidy has one (61 ..
    64 at ploidy 4, 127 .. 129 at ploidy 3), else the two blocks that meet at id 64; one word only: the middle of the panel"""
    for b in (64, 128, 192):
        first = ((b - 1 + ploidy - 1) // ploidy - 1) * ploidy + 1      # the block of id b - 1
        if first <= b - 1 and first + ploidy - 1 >= b and first + ploidy - 1 <= max_hap:
            return [b - 1]
    return [63, 64] if max_hap >= 64 else [max_hap // 2]


def _emission_case(ploidy, bit_len, n_drawn):
    """the data of one emissions test: eight windows of 35 rows"""
    rng = np.random.default_rng(1000 * ploidy + 10 * bit_len + n_drawn)
    W = _words(bit_len)
    max_hap = _max_hap(bit_len, ploidy)
    n_hap = max_hap + 1
    assert max_hap % ploidy != 0 and max_hap <= 8 * bit_len - 2 and (bit_len != 32 or n_hap == 255)
    high = 64 if W > 1 else max_hap // 2      # (one word: no id of 64 and above; the upper half of the panel)
    straddle = _straddle(ploidy, max_hap)

    def draws():
        def some(k, must=(), lo=0):
            must = list(must)[:max(k, 1)]
            pool = [h for h in range(lo, n_hap) if h not in must]
            return sorted(must + [int(x) for x in rng.choice(pool, size=max(0, k - len(must)), replace=False)])
        return [some(n_drawn), some(n_drawn, (0,)), some(n_drawn, (max_hap,)), some(n_drawn, (1, 2) if n_drawn > 1 else (1,)), [5], some(n_drawn),
                some(min(n_drawn, n_hap - high), lo=high), some(max(n_drawn, len(straddle)), straddle)]

    def windows(tops):
        lists = [_blocks(t, ploidy, max_hap) for t in tops]
        n_gt = max(len(x) for x in lists)
        win_haps = np.zeros((len(tops), n_gt, ploidy), dtype=np.uint8)
        for w, x in enumerate(lists):
            win_haps[w, :len(x)] = np.array(x, dtype=np.uint8)
        return np.array([len(x) for x in lists], dtype=np.uint32), win_haps, [_mask_of(t) for t in tops], lists

    tops = draws()
    n_windows = len(tops)
    n_rows = n_windows * PER_WINDOW
    win_n, win_haps, win_top, lists = windows(tops)
    assert (0,) * ploidy in lists[1] and any(0 in gt and max_hap in gt for gt in lists[2]) and win_n[4] == 1
    assert tops[6] and min(tops[6]) >= high
    if W > 1:      # a block, or two that meet, on both sides of a word boundary
        ids = sorted({h for gt in lists[7] for h in gt})
        assert any(a + 1 == b and (b & 63) == 0 for a, b in zip(ids, ids[1:])), ids
    rows = dict(zero=2, lost=PER_WINDOW + 3, dead=3 * PER_WINDOW + 5, flag=2 * PER_WINDOW + 7, top_only=2 * PER_WINDOW + 9, last_bit=4, gt0_all=7 * PER_WINDOW + 1)
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, n_rows,
                                               fixed={rows["zero"]: 0, rows["lost"]: 20, rows["dead"]: 30, rows["flag"]: 25, rows["top_only"]: 12,
                                                      rows["last_bit"]: 12, rows["gt0_all"]: 40})
    counts_l = counts.tolist()
    row_win = np.repeat(np.arange(n_windows), PER_WINDOW).astype(np.uint32)
    gt0 = [int.from_bytes(rng.bytes(bit_len), "little") & ((1 << n_hap) - 1) for _ in range(n_rows)]
    tables = (rng.random(256 * (ploidy + 1)).astype(LD) + LD(0.05)) * np.power(LD(10), rng.integers(-300, 1, size=256 * (ploidy + 1)).astype(LD))
    e = {k: int(entry_begin[r]) for k, r in rows.items()}
    for j in range(e["lost"], e["lost"] + counts_l[rows["lost"]]):      # no drawn haplotype of its window carries any entry of this row
        bits[j] &= ~win_top[1]
    alive0 = (rng.random(len(bits)) < 0.9).astype(np.uint8)
    alive0[e["dead"]:e["dead"] + counts_l[rows["dead"]]:2] = 0
    alive0[e["dead"] + 1] = 1      # (one of the living is carried by the window's draw for certain)
    bits[e["dead"] + 1] |= win_top[3]
    # the flagged row (window 2, whose draw holds the last haplotype): entry 2 is under-covered, multi-copy and carried by the last haplotype
    # alone among those of its block; the sequence check takes it off -- an id of 64 or above wherever the width has one
    jf = e["flag"] + 2
    alive0[jf] = 1
    cov[jf], f[jf] = 1, 2
    last_block = next(gt for gt in lists[2] if max_hap in gt)
    bits[jf] = (bits[jf] & ~_mask_of(set(last_block))) | (1 << max_hap)
    gt0[rows["flag"]] = 0
    assert W == 1 or max_hap >= 64
    # an entry that only the last haplotype carries -- a haplotype of the top word -- in the window that drew it: it stays
    jt = e["top_only"] + 3
    alive0[jt], bits[jt], cov[jt] = 1, 1 << max_hap, 20
    # an entry whose only set bit is the last bit (at nine bytes bit 7 of word 1), never a haplotype: it leaves the list
    jl = e["last_bit"] + 5
    alive0[jl], bits[jl] = 1, 1 << (8 * bit_len - 1)
    # a row whose reference-allele mask has bits in every word, under entries with the last bit set and a coverage inside the interval
    gt0[rows["gt0_all"]] = _mask_of([h for h in (1, 65, 129, 193) if h < n_hap] + [max_hap]) | gt0[rows["gt0_all"]]
    for j in range(e["gt0_all"], e["gt0_all"] + 40, 3):
        bits[j] |= 1 << (8 * bit_len - 1)
        cov[j] = 23
    fixes = {(rows["flag"], 2): 1 << max_hap}
    tops2 = draws()
    win_n2, win_haps2, win_top2, _ = windows(tops2)
    return dict(W=W, n_hap=n_hap, max_hap=max_hap, n_rows=n_rows, n_windows=n_windows, rows=rows, e=e, win=(win_n, win_haps, win_top), win2=(win_n2, win_haps2, win_top2),
                counts=counts, entry_begin=entry_begin, f=f, bits=bits, cov=cov, row_win=row_win, gt0=gt0, tables=tables, alive0=alive0, fixes=fixes, jt=jt, jl=jl)


@pytest.mark.parametrize("n_drawn", [1, 5, 15])
@pytest.mark.parametrize("bit_len", [7, 9, 16, 17, 32])
@pytest.mark.parametrize("ploidy", [3, 4, 6, 8])
def test_emissions_with_a_genotype_list_per_window_over_a_wide_panel_equal_the_host_arithmetic(ploidy, bit_len, n_drawn):
    """vgmi_hmm_emissions_select_ploidy_wide against test_gpu_hmm_select_ploidy's numpy model on Python integers, bit for bit -- scores,
    n_kept, flags, alive bytes -- in ONE call over eight windows: the six of the packed test (a random draw, one with haplotype 0, one with
    the last haplotype -- no multiple of the ploidy, a truncated block; 254 at 32 bytes --, two draws in one block, a single draw, a second
    random draw), one whose drawn haplotypes all lie at ids of 64 and above (seven bytes have one word: the upper half of the panel), and
    one with a block -- at ploidy 3 below 127 haplotypes two blocks -- on both sides of a word boundary.  35 rows each of 0..70 entries: a
    row of zero entries, a row that dies in the prune, a row half dead on entry, an entry only a top-word haplotype carries, an entry whose
    only set bit is the last bit, a row whose gt0 has bits in every word that holds haplotypes, and a flagged row that a second launch scores again with a fix
    that clears the last haplotype (an id of 64 or above from nine bytes on).  A second call sees the first call's prune; a third, with
    other draws, scores what is left.  Ploidy 3 and 4 run the MAXP = 4 kernels, 6 and 8 the MAXP = 8 ones; 15 draws at ploidy 8 name more
    than 64 haplotypes, which the ABI takes."""
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    c = _emission_case(ploidy, bit_len, n_drawn)
    W, n_rows, rows, e = c["W"], c["n_rows"], c["rows"], c["e"]
    win_n, win_haps, win_top = c["win"]
    win_n2, win_haps2, win_top2 = c["win2"]
    counts, entry_begin, row_win, gt0, tables, alive0, fixes = c["counts"], c["entry_begin"], c["row_win"], c["gt0"], c["tables"], c["alive0"], c["fixes"]
    f, bits, cov = c["f"], c["bits"], c["cov"]
    flag_row = rows["flag"]

    def call(ctx, wn, wh, wt, fx=None):
        return ctx.hmm_emissions_select_ploidy_wide(ploidy, wn, wh, _word_rows(wt, W), bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win,
                                                    _word_rows(gt0, W), fixes=fx)

    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        ctx.hmm_entries_upload_wide(f, _bytes_of(bits, bit_len), bit_len, cov, alive0)
        obs, n_kept, flags = call(ctx, win_n, win_haps, win_top)
        alive1 = ctx.hmm_alive_fetch()
        obs_f, n_kept_f, flags_f = call(ctx, win_n, win_haps, win_top, ([flag_row], [0, 1], [2], _word_rows([fixes[(flag_row, 2)]], W)))
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
    assert n_kept[rows["zero"]] == 0 and (obs[rows["zero"], :win_n[0]] == 1).all()
    lost = slice(e["lost"], e["lost"] + int(counts[rows["lost"]]))
    assert n_kept[rows["lost"]] == 0 and not alive1[lost].any() and (obs[rows["lost"], :win_n[1]] == 1).all()
    assert 0 < n_kept[rows["dead"]] <= int(counts[rows["dead"]]) // 2
    assert flags[flag_row] & 1 and not (flags & 2).any()
    assert alive1[c["jt"]] == 1 and alive0[c["jl"]] == 1 and alive1[c["jl"]] == 0
    for w in range(c["n_windows"]):      # lanes beyond a window's count: zero scores
        assert not obs[row_win == w][:, win_n[w]:].any()
    assert 0 < (alive0 != alive1).sum() and (n_kept > 0).sum() > n_rows // 2 and (obs > 0).any()
    assert all(x != 0 for x in _split(gt0[rows["gt0_all"]], W)[:(c["n_hap"] + 63) // 64])      # (17 bytes: four words, haplotypes in three)

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
    assert np.array_equal(alive2, m_alive) and not alive2[killed].any() and n_kept2[rows["lost"]] == 0


# ---- the tallies ----------------------------------------------------------------------------------------------------------------------------
N_GT = 6
WIN_N_GT = [1, 3, 6, 6]


def _model_tallies(ploidy, bit_len, f, bits, cov, alive, win_n_gt, win_haps, win_sel, entry_begin, counts, row_win, winner):
    """test_gpu_hmm_tallies_ploidy's model over Python integers: a place counts if its id is a haplotype (below 8 bit_len - 1) of the window's
    mask; alive None: every entry counts"""
    n_rows = len(counts)
    out = np.zeros((n_rows, 2 * ploidy), dtype=np.uint32)
    uniq = np.zeros(n_rows, dtype=np.uint8)
    for r in range(n_rows):
        w, g = int(row_win[r]), int(winner[r])
        if g >= win_n_gt[w]:
            continue
        ids = [int(h) for h in win_haps[w][g]]
        ok = [h < 8 * bit_len - 1 and (win_sel[w] >> h) & 1 == 1 for h in ids]
        u = 0
        for j in range(int(entry_begin[r]), int(entry_begin[r]) + int(counts[r])):
            if alive is not None and not alive[j]:
                continue
            if f[j] <= 1 and u < 255:
                u += 1
            for q in range(ploidy):
                if ok[q] and (bits[j] >> ids[q]) & 1:
                    out[r, 2 * q] += 1
                    out[r, 2 * q + 1] += int(cov[j])
        uniq[r] = u
    return out, uniq


def _tally_case(ploidy, bit_len):
    """four windows of 70 rows with 1, 3, 6 and 6 genotypes over 8 bit_len - 1 haplotypes"""
    rng = np.random.default_rng(5200 + 10 * bit_len + ploidy)
    n_hap = 8 * bit_len - 1
    last = n_hap - 1                                         # 8 bit_len - 2
    n_windows, per_window = len(WIN_N_GT), 70
    n_rows = n_windows * per_window
    counts = rng.integers(0, 71, size=n_rows)
    counts[[3, 4, 75, 279]] = 0
    counts[7] = 400
    counts[10], counts[11] = 64, 65
    special = [71, 73, 141, 142, 143, 146, 211]                   # rows whose genotype is set below: none a multiple of 9
    counts[special] = rng.integers(20, 71, size=len(special))
    entry_begin = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    n_entries = int(counts.sum())
    f = rng.choice([0, 1, 1, 2, 3], size=n_entries).astype(np.uint8)
    raw = rng.integers(0, 256, size=(n_entries, bit_len), dtype=np.uint8) | rng.integers(0, 256, size=(n_entries, bit_len), dtype=np.uint8)
    bits = [int.from_bytes(raw[j].tobytes(), "little") for j in range(n_entries)]      # three bits in four set, the last bit as well
    cov = rng.integers(0, 256, size=n_entries).astype(np.uint8)
    alive = (rng.random(n_entries) < 0.7).astype(np.uint8)
    lo = int(entry_begin[7])
    f[lo:lo + 400], cov[lo:lo + 400], alive[lo:lo + 400] = 1, 255, 1
    for j in range(lo, lo + 400):
        bits[j] |= 1                                         # haplotype 0 carries all 400
    row_win = np.repeat(np.arange(n_windows), per_window).astype(np.uint32)

    def blk(a):
        return tuple(min(x, last) for x in range(a, a + ploidy))
    zero, rep = (0,) * ploidy, (0,) * (ploidy - 1) + (last,)
    edge = tuple(h if h <= last else 0 for h in (63, 64, last))      # 63, 64 where the width has them, 8 bit_len - 2 ...
    if ploidy == 4:
        edge += (8 * bit_len - 1,)                           # ... and the last BIT, which most entries have set and the masks below hold: no haplotype
    lists = [[zero, blk(20), blk(24), blk(28), blk(32), blk(36)],
             [rep, blk(5), blk(9), blk(13), blk(36), blk(40)],
             [blk(1), blk(13), blk(17), blk(last - ploidy + 1), zero, edge],
             [blk(last - ploidy + 1), blk(33), rep, blk(1), blk(9), edge]]
    win_haps = np.array(lists, dtype=np.uint8)
    assert win_haps.shape == (n_windows, N_GT, ploidy)
    masks = []
    for w in range(n_windows):
        masks.append(_mask_of(h for g in range(WIN_N_GT[w]) for h in lists[w][g] if h <= last))
    masks[2] |= 1 << (8 * bit_len - 1)
    masks[3] |= 1 << (8 * bit_len - 1)
    masks[2] &= ~(1 << 18)                                   # window 2, genotype 2 = 17, 18, 19 ..: 18 was not drawn
    winner = rng.integers(0, N_GT, size=n_rows).astype(np.uint32)      # (windows 0 and 1 have fewer: those rows read zeros)
    winner[::9] = 0xFFFFFFFF
    winner[7] = 0
    winner[10], winner[11] = 0, 0
    winner[71], winner[73] = 0, 4                            # window 1: (0, .., 0, last); 4 < n_gt but >= the window's 3
    winner[141], winner[142], winner[143], winner[146] = 2, 3, 4, 5      # window 2: an id outside the mask; the last haplotype; the all-zero block; 63, 64, last
    winner[211] = 5
    return dict(f=f, bits=bits, cov=cov, alive=alive, entry_begin=entry_begin, counts=counts, row_win=row_win, win_haps=win_haps, masks=masks, winner=winner,
                last=last, edge=edge)


@pytest.mark.parametrize("bit_len", [7, 9, 32])
@pytest.mark.parametrize("ploidy", [3, 4])
def test_tallies_of_a_polyploid_call_over_a_wide_panel_equal_the_host_walk(ploidy, bit_len):
    """vgmi_hmm_tallies_ploidy_wide, every number of every row against the model: rows without entries, of 64 and of 65 entries, 400
    single-copy k-mers of coverage 255 (unique stops at 255, the sum is 102 000), 30 % dead entries, rows without a call, a winner beyond
    its window's count, the genotypes (0, .., 0) and (0, .., 0, last), an id that was not drawn, the ids 63, 64 and 8 bit_len - 2 in one
    genotype (at ploidy 4 with the id of the last bit, which is no haplotype and reads zeros).  Then the whole-lists form: one window, every
    haplotype selected, no alive bytes -- the dead entries count."""
    c = _tally_case(ploidy, bit_len)
    W, n_rows, last = _words(bit_len), len(c["counts"]), c["last"]
    sel = _word_rows(c["masks"], W)
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        ctx.hmm_entries_upload_wide(c["f"], _bytes_of(c["bits"], bit_len), bit_len, c["cov"], c["alive"])
        out, uniq = ctx.hmm_tallies_ploidy_wide(bit_len, ploidy, c["win_haps"], sel, c["entry_begin"], c["counts"], c["winner"], row_win=c["row_win"],
                                                win_n_gt=WIN_N_GT, use_alive=True)
        panel_haps = c["win_haps"][2:3]
        all_haps = [(1 << (last + 1)) - 1]
        out_p, uniq_p = ctx.hmm_tallies_ploidy_wide(bit_len, ploidy, panel_haps, _word_rows(all_haps, W), c["entry_begin"], c["counts"], c["winner"], use_alive=False)
    finally:
        ctx.close()
    assert out.shape == (n_rows, 2 * ploidy) and out.dtype == np.uint32 and uniq.shape == (n_rows,) and uniq.dtype == np.uint8
    want, want_u = _model_tallies(ploidy, bit_len, c["f"], c["bits"], c["cov"], c["alive"], WIN_N_GT, c["win_haps"], c["masks"], c["entry_begin"], c["counts"],
                                  c["row_win"], c["winner"])
    bad = np.flatnonzero((out != want).any(axis=1) | (uniq != want_u))
    assert bad.size == 0, (bad[:10], out[bad[:3]], want[bad[:3]], uniq[bad[:3]], want_u[bad[:3]])
    assert uniq[7] == 255 and out[7].tolist() == [400, 102_000] * ploidy
    assert c["counts"][10] == 64 and c["counts"][11] == 65 and out[10].any() and out[11].any()
    assert not out[::9].any() and not uniq[::9].any() and out[1::9].any()
    assert not out[73].any() and uniq[73] == 0 and c["winner"][73] < N_GT
    assert len(set(out[71, 0:2 * ploidy - 2:2])) == 1 and out[71, 0] > 0 and out[71, 2 * ploidy - 2] > 0         # (0, .., 0, last): every place tallied
    assert out[141, 0] > 0 and out[141, 2:4].tolist() == [0, 0] and out[141, 4] > 0                                   # 18 was not drawn
    assert out[142, 2 * ploidy - 2] > 0                                                                               # the last haplotype
    assert len(set(out[143, 0::2])) == 1 and len(set(out[143, 1::2])) == 1 and out[143, 0] > 0                         # the all-zero block
    assert (out[146, 0:6:2] > 0).all() and out[211, 4] > 0                                                            # 63, 64 (or 0), 8 bit_len - 2
    if ploidy == 4:
        assert c["edge"][3] == 8 * bit_len - 1 and out[146, 6:8].tolist() == [0, 0]                                   # the last bit is no haplotype
    dead = c["alive"] == 0
    assert 0.25 < dead.mean() < 0.35
    want_p, want_pu = _model_tallies(ploidy, bit_len, c["f"], c["bits"], c["cov"], None, [N_GT], panel_haps, all_haps, c["entry_begin"], c["counts"],
                                     np.zeros(n_rows, dtype=np.uint32), c["winner"])
    assert np.array_equal(out_p, want_p) and np.array_equal(uniq_p, want_pu)
    alive_only, _ = _model_tallies(ploidy, bit_len, c["f"], c["bits"], c["cov"], c["alive"], [N_GT], panel_haps, all_haps, c["entry_begin"], c["counts"],
                                   np.zeros(n_rows, dtype=np.uint32), c["winner"])
    assert int(out_p[:, 0::2].sum()) > int(alive_only[:, 0::2].sum()) and not out_p[::9].any()


# ---- narrow widths: the packed calls' bytes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit_len,n_hap", [(2, 15), (6, 47)])
def test_wide_ploidy_calls_return_the_packed_calls_bytes(bit_len, n_hap):
    """At 2 and 6 bytes of haplotype bits, after hmm_entries_upload_wide, hmm_emissions_select_ploidy_wide (with a fixed row) and
    hmm_tallies_ploidy_wide return exactly the bytes hmm_emissions_select_ploidy / hmm_tallies_ploidy return after hmm_entries_upload on the
    same data, alive bytes included."""
    ploidy, n_windows = 4, 3
    rng = np.random.default_rng(300 + bit_len)
    max_hap = n_hap - 1
    n_rows = n_windows * PER_WINDOW
    tops = [sorted(int(x) for x in rng.choice(n_hap, size=5, replace=False)) for _ in range(n_windows - 1)] + [[0, 3, max_hap]]
    lists = [_blocks(t, ploidy, max_hap) for t in tops]
    n_gt = max(len(x) for x in lists)
    win_haps = np.zeros((n_windows, n_gt, ploidy), dtype=np.uint8)
    for w, x in enumerate(lists):
        win_haps[w, :len(x)] = np.array(x, dtype=np.uint8)
    win_n = np.array([len(x) for x in lists], dtype=np.uint32)
    win_top = np.array([_mask_of(t) for t in tops], dtype=np.uint64)
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, n_rows, fixed={3: 20, 90: 25})
    row_win = np.repeat(np.arange(n_windows), PER_WINDOW).astype(np.uint32)
    gt0 = rng.integers(0, 1 << n_hap, size=n_rows, dtype=np.uint64)
    tables = (rng.random(256 * (ploidy + 1)).astype(LD) + LD(0.05)) * np.power(LD(10), rng.integers(-300, 1, size=256 * (ploidy + 1)).astype(LD))
    alive0 = (rng.random(len(bits)) < 0.9).astype(np.uint8)
    j90 = int(entry_begin[90]) + 2      # row 90 (the last window): flagged, and fixed in a second launch
    alive0[j90], cov[j90], f[j90] = 1, 1, 2
    bits[j90] |= 1 << max_hap
    gt0[90] = 0
    fix = ([90], [0, 1], [2], [1 << max_hap])
    winner = rng.integers(0, n_gt, size=n_rows).astype(np.uint32)
    winner[::7] = 0xFFFFFFFF
    entries = (f.astype(np.uint64) << np.uint64(8)) | (np.array(bits, dtype=np.uint64) << np.uint64(16))
    got = {}
    for form in ("packed", "wide"):
        ctx = vgmi.Context(0, buffer_mib=16)
        try:
            if form == "packed":
                ctx.hmm_entries_upload(entries, cov, alive0)
                a = (ploidy, win_n, win_haps, win_top, bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0)
                emit = ctx.hmm_emissions_select_ploidy(*a)
                alive = ctx.hmm_alive_fetch()
                fixed = ctx.hmm_emissions_select_ploidy(*a, fixes=fix)
                tal = ctx.hmm_tallies_ploidy(ploidy, win_haps, win_top, entry_begin, counts, winner, row_win=row_win, win_n_gt=win_n)
                tal_whole = ctx.hmm_tallies_ploidy(ploidy, win_haps[:1], win_top[:1], entry_begin, counts, winner, use_alive=False)
            else:
                ctx.hmm_entries_upload_wide(f, _bytes_of(bits, bit_len), bit_len, cov, alive0)
                a = (ploidy, win_n, win_haps, win_top.reshape(-1, 1), bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0.reshape(-1, 1))
                emit = ctx.hmm_emissions_select_ploidy_wide(*a)
                alive = ctx.hmm_alive_fetch()
                fixed = ctx.hmm_emissions_select_ploidy_wide(*a, fixes=fix)
                tal = ctx.hmm_tallies_ploidy_wide(bit_len, ploidy, win_haps, win_top.reshape(-1, 1), entry_begin, counts, winner, row_win=row_win, win_n_gt=win_n)
                tal_whole = ctx.hmm_tallies_ploidy_wide(bit_len, ploidy, win_haps[:1], win_top[:1].reshape(-1, 1), entry_begin, counts, winner, use_alive=False)
            got[form] = [*emit, alive, *fixed, *tal, *tal_whole, ctx.hmm_alive_fetch()]
        finally:
            ctx.close()
    assert len(got["packed"]) == len(got["wide"]) == 12
    for i, (a, b) in enumerate(zip(got["packed"], got["wide"])):
        assert a.dtype == b.dtype and np.array_equal(a, b), i
    obs, n_kept, flags, alive, obs_f = got["wide"][:5]
    assert (obs > 0).any() and (n_kept > 0).sum() > n_rows // 2 and flags[90] & 1 and (alive != alive0).any() and not np.array_equal(obs_f[90], obs[90])
    assert got["wide"][7].any() and got["wide"][9].any()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_wide_ploidy_calls_refuse_what_they_cannot_take_and_serve_on():
    """Every refusal of the three entry points, and after each a valid call that returns what it returned before.  VGMI_E_INVALID: bit_len 0
    and 33, an id in win_haps at 8 bit_len - 1, a drawn haplotype at 8 bit_len - 1, ploidy 1 and 9 (emissions) and 1 and 5 (tallies), n_gt 0,
    65 (emissions) and 129 (tallies), a window's count of 0 and of n_gt + 1, a row outside the entries, a row in a window that does not
    exist.  VGMI_E_STATE: no entries at all (so neither coverage nor alive bytes), entries of the packed upload, another bit_len than the
    upload's, the packed parts' two fix launches on such a part and this part's fix launch on a packed part."""
    rng = np.random.default_rng(9)
    bit_len, n_hap, ploidy, n_rows = 9, 71, 4, 30
    W = _words(bit_len)
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, n_rows, fixed={})
    row_win = np.repeat(np.arange(3), 10).astype(np.uint32)
    tops = [[0, 5, 63, 64, 70], [1, 2, 3, 62, 69], [4, 6, 8, 65, 68]]
    lists = [_blocks(t, ploidy, n_hap - 1) for t in tops]
    n_gt = max(len(x) for x in lists)
    win_haps = np.zeros((3, n_gt, ploidy), dtype=np.uint8)
    for w, x in enumerate(lists):
        win_haps[w, :len(x)] = np.array(x, dtype=np.uint8)
    win_n = np.array([len(x) for x in lists], dtype=np.uint32)
    masks = _word_rows([_mask_of(t) for t in tops], W)
    gt0 = np.zeros((n_rows, W), dtype=np.uint64)
    tables = rng.random(256 * (ploidy + 1)).astype(LD) + LD(0.05)
    winner = np.zeros(n_rows, dtype=np.uint32)
    raw = _bytes_of(bits, bit_len)
    n_entries = len(bits)
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        def emit(**kw):
            a = dict(ploidy=ploidy, win_n_gt=win_n, win_haps=win_haps, win_top_mask=masks, bit_len=bit_len, ave=AVE, lower=LOWER, upper=UPPER, tables=tables,
                     entry_begin=entry_begin, entry_count=counts, row_win=row_win, gt0=gt0)
            a.update(kw)
            return ctx.hmm_emissions_select_ploidy_wide(**a)

        def tally(**kw):
            a = dict(bit_len=bit_len, ploidy=ploidy, win_haps=win_haps, win_sel_mask=masks, entry_begin=entry_begin, entry_count=counts, winner=winner,
                     row_win=row_win, win_n_gt=win_n)
            a.update(kw)
            return ctx.hmm_tallies_ploidy_wide(**a)

        wide_args = (ploidy, win_n, win_haps, masks, bit_len, tables, entry_begin, counts, row_win, gt0)
        for call in (emit, tally):      # nothing uploaded yet: a state error, not a fault
            with pytest.raises(vgmi.VgmiError) as err:
                call()
            assert err.value.code == vgmi.E_STATE
        ctx.hmm_entries_upload_wide(f, raw, bit_len, cov)
        emit()      # (the selection prunes the lists once; from here on every valid call finds the state it left)
        good_obs = emit()
        good_tally = tally()
        assert (good_obs[0] > 0).any() and good_tally[0].any()

        def serves_on():
            assert all(np.array_equal(a, b) for a, b in zip(emit(), good_obs))
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
        at_flag = win_haps.copy()
        at_flag[1, 0, 1] = 8 * bit_len - 1
        drawn_flag = masks.copy()
        drawn_flag[2, 1] |= np.uint64(1) << np.uint64(7)      # bit 71 = 8 bit_len - 1
        drawn_pad = masks.copy()
        drawn_pad[0, 1] |= np.uint64(1) << np.uint64(40)      # beyond the nine bytes
        t2, t10 = (rng.random(256 * (p + 1)).astype(LD) for p in (1, 9))

        def haps(n, p):
            return np.zeros((3, n, p), dtype=np.uint8)
        for code, call in [
                (vgmi.E_INVALID, lambda: emit(bit_len=0)),
                (vgmi.E_INVALID, lambda: emit(bit_len=33)),
                (vgmi.E_STATE, lambda: emit(bit_len=12)),
                (vgmi.E_STATE, lambda: emit(bit_len=8, win_top_mask=masks[:, :1], gt0=gt0[:, :1])),
                (vgmi.E_INVALID, lambda: emit(win_haps=at_flag)),
                (vgmi.E_INVALID, lambda: emit(win_top_mask=drawn_flag)),
                (vgmi.E_INVALID, lambda: emit(win_top_mask=drawn_pad)),
                (vgmi.E_INVALID, lambda: emit(ploidy=1, win_haps=haps(n_gt, 1), tables=t2)),
                (vgmi.E_INVALID, lambda: emit(ploidy=9, win_haps=haps(n_gt, 9), tables=t10)),
                (vgmi.E_INVALID, lambda: emit(win_haps=haps(0, ploidy))),
                (vgmi.E_INVALID, lambda: emit(win_haps=haps(65, ploidy))),
                (vgmi.E_INVALID, lambda: emit(win_n_gt=[0, 1, 1])),
                (vgmi.E_INVALID, lambda: emit(win_n_gt=[1, n_gt + 1, 1])),
                (vgmi.E_INVALID, lambda: emit(entry_begin=beyond, entry_count=counts_beyond)),
                (vgmi.E_INVALID, lambda: emit(row_win=bad_win)),
                (vgmi.E_INVALID, lambda: tally(bit_len=0)),
                (vgmi.E_INVALID, lambda: tally(bit_len=33)),
                (vgmi.E_STATE, lambda: tally(bit_len=10)),
                (vgmi.E_INVALID, lambda: tally(ploidy=1, win_haps=haps(n_gt, 1))),
                (vgmi.E_INVALID, lambda: tally(ploidy=5, win_haps=haps(n_gt, 5))),
                (vgmi.E_INVALID, lambda: tally(win_haps=haps(0, ploidy))),
                (vgmi.E_INVALID, lambda: tally(win_haps=haps(129, ploidy))),
                (vgmi.E_INVALID, lambda: tally(win_n_gt=[1, n_gt + 1, 1])),
                (vgmi.E_INVALID, lambda: tally(entry_begin=beyond, entry_count=counts_beyond)),
                (vgmi.E_INVALID, lambda: tally(row_win=bad_win)),
                # the packed parts' fix launches on a part of this call
                (vgmi.E_STATE, lambda: _fix_with(ctx, "vgmi_hmm_part_fix_rows", np.uint16, "vgmi_hmm_emissions_select_ploidy_wide", wide_args)),
                (vgmi.E_STATE, lambda: _fix_with(ctx, "vgmi_hmm_part_fix_rows_wide", np.uint64, "vgmi_hmm_emissions_select_ploidy_wide", wide_args))]:
            refused(code, call)
        # packed entries: the new calls refuse them, a packed part refuses the new fix launch, and the reverse again
        ctx.hmm_entries_upload(np.zeros(n_entries, dtype=np.uint64), cov)
        for call in (emit, tally):
            with pytest.raises(vgmi.VgmiError) as err:
                call()
            assert err.value.code == vgmi.E_STATE
        packed_args = (ploidy, win_n, win_haps % 40, np.full(3, 0b111, dtype=np.uint64), 6, tables, entry_begin, counts, row_win, gt0[:, 0])
        _fix_with(ctx, "vgmi_hmm_part_fix_rows_wide", np.uint64, "vgmi_hmm_emissions_select_ploidy", packed_args)      # (its own launch: taken)
        with pytest.raises(vgmi.VgmiError) as err:
            _fix_with(ctx, "vgmi_hmm_part_fix_rows_ploidy_wide", np.uint64, "vgmi_hmm_emissions_select_ploidy", packed_args)
        assert err.value.code == vgmi.E_STATE
        ctx.hmm_entries_upload_wide(f, raw, bit_len, cov)
        emit()      # (every entry is alive again: the selection prunes once more)
        serves_on()
    finally:
        ctx.close()


def _fix_with(ctx, fix_name, mask_type, emit_name, args):
    """a part straight from the C ABI (the Python wrappers pick the right fix launch themselves), handed to the fix launch `fix_name` with one
    fix that takes nothing off entry 0 of the first row that has an entry; raises what the launch answers"""
    import ctypes as C
    from varigraph_amd.vgmi import _ptr
    ploidy, win_n, win_haps, win_top, bit_len, tables, entry_begin, counts, row_win, gt0 = args
    arrs = [np.ascontiguousarray(a, dtype=t) for a, t in ((win_n, np.uint32), (win_haps, np.uint8), (win_top, np.uint64), (tables, np.longdouble),
                                                         (entry_begin, np.uint64), (counts, np.uint32), (row_win, np.uint32), (gt0, np.uint64))]
    n_rows = arrs[4].size
    n_kept, flags = np.zeros(n_rows, dtype=np.uint32), np.zeros(n_rows, dtype=np.uint8)
    part = C.c_void_p()
    ctx._chk(getattr(ctx._l, emit_name)(ctx._h, arrs[1].shape[1], ploidy, arrs[1].shape[0], _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), bit_len, float(AVE),
                                        float(LOWER), float(UPPER), _ptr(arrs[3]), n_rows, _ptr(arrs[4]), _ptr(arrs[5]), _ptr(arrs[6]), _ptr(arrs[7]), _ptr(n_kept),
                                        _ptr(flags), C.byref(part)))
    try:
        row = int(np.flatnonzero(arrs[5])[0])
        rows, off, j, m = np.array([row], dtype=np.uint64), np.array([0, 1], dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.zeros(4, dtype=mask_type)
        ctx._chk(getattr(ctx._l, fix_name)(part, 1, _ptr(rows), _ptr(off), _ptr(j), _ptr(m)))
    finally:
        ctx._l.vgmi_hmm_part_free(part)


# ---- the command line: cohorts of 13 and 17 tetraploid samples (53 and 69 haplotypes: seven and nine bytes of haplotype bits) -------------------
def _ploidy_cohort(work, n_samples):
    """test_gpu_hmm_select_ploidy's cohort with more samples: 200 kb, 1 500 sites (one in ten a short indel, four in ten an insertion of 60 ..
    300 bp), `--vcf-ploidy 4`, seed 19; reads of individuals 0, 1 and 3, 20 000 pairs each, seeds 170 + i, three samples in one samples.cfg"""
    from test_gpu_configs import CLI, ENV, _need_binaries, _write_fastq
    from varigraph_amd import synth
    _need_binaries()
    ref = synth.make_reference(200_000)
    variants, gts = synth.make_cohort(ref, 1500, n_samples=n_samples, ploidy=4, seed=19, indel_frac=0.1, sv_frac=0.4)
    fa, vcf = os.path.join(work, "ref.fa"), os.path.join(work, "in.vcf")
    synth.write_fasta(fa, "chr1", ref)
    synth.write_vcf(vcf, "chr1", len(ref), variants, gts, n_samples, 4)
    graph = os.path.join(work, "graph.bin")
    r = subprocess.run([CLI, "construct", "-r", fa, "-v", vcf, "--save-graph", graph, "-t", "16", "--gpu", "0", "--vcf-ploidy", "4"], cwd=work,
                       capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    cfg = ""
    for i, who in enumerate((0, 1, 3)):
        fq = _write_fastq(os.path.join(work, f"s{i}"), synth.sample_haplotypes(ref, variants, gts, who, 4), 20_000, seed=170 + i)
        cfg += f"ind{i} " + " ".join(fq) + "\n"
    return graph, cfg


@pytest.fixture(scope="module")
def cohort_53(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("wide_ploidy_cli"))
    graph, cfg = _ploidy_cohort(work, 13)
    yield work, graph, cfg
    shutil.rmtree(work, ignore_errors=True)


def _genotype(work, graph, cfg, tag, exe, opts, env):
    from test_gpu_configs import REF, _run, _vcf
    d = os.path.join(work, tag)
    os.makedirs(d, exist_ok=True)
    open(os.path.join(d, "samples.cfg"), "w").write(cfg)
    more = [] if exe == REF else ["--gpu", "0"]
    r = _run([exe, "genotype", "--load-graph", graph, "-s", "samples.cfg", "-t", "6"] + opts + ["--use-depth", "--granularity", "0.01"] + more, cwd=d,
             capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (tag, r.stderr[-2000:])
    return [_vcf(d, f"ind{i}") for i in range(3)], r.stderr


def _reference(work, graph, cfg, tag, opts):
    """the deterministic reference build's three VCFs; at least 100 lines each and no two alike: the comparison is not of empty files"""
    from test_gpu_configs import ENV, REF
    want, _ = _genotype(work, graph, cfg, f"{tag}_cpu", REF, opts, ENV)
    lines = [v.count(b"\n") for v in want]
    print(f"{tag}: reference VCF lines {lines}")
    assert min(lines) >= 100, lines
    assert want[0] != want[1] and want[1] != want[2] and want[0] != want[2]
    return want


CASES = {"p4n5": ["--sample-ploidy", "4", "-n", "5"], "p3n4": ["--sample-ploidy", "3", "-n", "4"], "p4n5sv": ["--sample-ploidy", "4", "-n", "5", "--sv"],
         "p4n5hom": ["--sample-ploidy", "4", "-n", "5", "-g", "hom"], "p4n15": ["--sample-ploidy", "4", "-n", "15"], "p6n5": ["--sample-ploidy", "6", "-n", "5"],
         "p8n8": ["--sample-ploidy", "8", "-n", "8"]}


@pytest.mark.parametrize("case", list(CASES))
def test_command_line_polyploid_over_53_haplotypes_on_the_selected_path_equals_the_reference(case, cohort_53):
    """`varigraph-mi genotype --sample-ploidy P -n N --use-depth` over the 53-haplotype graph (13 tetraploid samples: seven bytes, W = 1), 20
    windows of 10 kb, three samples in one run, VGH_HMM_WIDE_PLOIDY_DEVICE=1: every VCF is the deterministic reference build's byte for byte;
    so are they with VGH_HMM_SELECT_DEVICE=0, VGH_HMM_FIX_DEVICE=0, VGH_DEVICE_TALLIES=0, VGH_HMM_FAKE_NOMEM=1 and with the knob unset.  The
    log of the knob-on runs carries the selected-path line for every window of all three samples and `7 bytes per entry` once, the tallies
    line for ploidy 3 and 4 and not for 6 and 8; with VGH_HMM_FAKE_NOMEM=1 the first sample takes the pool and two take the selected path;
    with the knob unset or VGH_HMM_SELECT_DEVICE=0 there is no selected-path line and the pool's `HMM thread-seconds: selection` line.
    -n 8 at ploidy 8 is 64 places, the bound.  Reference VCF lines, counted on the CPU with the read generator's host twin: p4 n5 1509 / 1427 /
    1420, p3 n4 1509 / 1486 / 1437, p4 n5 --sv 613 / 580 / 576, p4 n5 -g hom 1509 / 1427 / 1420, p4 n15 1509 / 1427 / 1414, p6 n5 1509 / 1505 /
    1486, p8 n8 1509 / 1506 / 1505."""
    from test_gpu_configs import CLI, ENV
    work, graph, cfg = cohort_53
    opts = CASES[case]
    ploidy = opts[1]
    want = _reference(work, graph, cfg, case, opts)
    on = dict(ENV, VGH_TIMING="1", VGH_HMM_WIDE_PLOIDY_DEVICE="1")
    logs = {}
    for name, env in (("native", on), ("host_select", dict(on, VGH_HMM_SELECT_DEVICE="0")), ("host_fixes", dict(on, VGH_HMM_FIX_DEVICE="0")),
                      ("host_tallies", dict(on, VGH_DEVICE_TALLIES="0")), ("fake_nomem", dict(on, VGH_HMM_FAKE_NOMEM="1")), ("knob_unset", dict(ENV, VGH_TIMING="1"))):
        got, logs[name] = _genotype(work, graph, cfg, f"{case}_{name}", CLI, opts, env)
        for i in range(3):
            assert got[i] == want[i], (case, name, i)
    for name in ("native", "host_fixes", "host_tallies"):
        seen = re.findall(SELECTED, logs[name])
        assert len(seen) == 3 and all(a == b and int(b) >= 20 for a, b in seen), (name, seen)
        assert re.findall(BITS, logs[name]) == ["7"], name
    tallied = re.findall(TALLY_LINE, logs["native"])
    if ploidy in ("3", "4"):
        assert len(tallied) == 3 and all(int(rows) > 0 and p == ploidy for rows, p in tallied), tallied
        assert len(re.findall(TALLY_LINE, logs["fake_nomem"])) == 2
    else:
        assert tallied == []
    assert re.findall(TALLY_LINE, logs["host_tallies"]) == []
    assert len(re.findall(SELECTED, logs["fake_nomem"])) == 2 and re.findall(BITS, logs["fake_nomem"]) == ["7"]
    for name in ("knob_unset", "host_select"):      # the pool
        assert not re.search(SELECTED, logs[name]) and not re.search(BITS, logs[name]), name
        assert "HMM thread-seconds: selection" in logs[name], name
    scored = {name: [tuple(map(int, m)) for m in re.findall(r"(\d+) nodes scored by the host, (\d+) scored again on the device", logs[name])]
              for name in ("native", "host_fixes")}
    print(f"{case}: nodes scored by the host / again on the device, per sample: {scored}")


def test_command_line_polyploid_beyond_64_places_keeps_the_pool(cohort_53):
    """--sample-ploidy 6 -n 15 names up to 90 haplotypes per window, more than the host's 64-bit masks over places hold: with the knob set the
    sample keeps the pool and equals the reference (1509 / 1505 / 1486 lines at -n 5; here whatever the reference writes, at least 100)."""
    from test_gpu_configs import CLI, ENV
    work, graph, cfg = cohort_53
    opts = ["--sample-ploidy", "6", "-n", "15"]
    want = _reference(work, graph, cfg, "p6n15", opts)
    got, log = _genotype(work, graph, cfg, "p6n15_native", CLI, opts, dict(ENV, VGH_TIMING="1", VGH_HMM_WIDE_PLOIDY_DEVICE="1"))
    for i in range(3):
        assert got[i] == want[i], i
    assert not re.search(SELECTED, log) and not re.search(BITS, log) and "HMM thread-seconds: selection" in log


def test_command_line_polyploid_over_69_haplotypes_takes_two_words_per_entry(tmp_path_factory):
    """A cohort of 17 tetraploid samples -- 69 haplotypes, nine bytes of haplotype bits, W = 2 on the device -- with --sample-ploidy 4 -n 5: the
    reference's VCFs byte for byte (1509 / 1399 / 1394 lines when counted on the CPU), the selected path for every window of all three samples,
    `9 bytes per entry` once, the tallies on the device."""
    from test_gpu_configs import CLI, ENV
    work = str(tmp_path_factory.mktemp("wide_ploidy_cli_69"))
    try:
        graph, cfg = _ploidy_cohort(work, 17)
        opts = ["--sample-ploidy", "4", "-n", "5"]
        want = _reference(work, graph, cfg, "p4n5_69", opts)
        got, log = _genotype(work, graph, cfg, "p4n5_69_native", CLI, opts, dict(ENV, VGH_TIMING="1", VGH_HMM_WIDE_PLOIDY_DEVICE="1"))
        for i in range(3):
            assert got[i] == want[i], i
        seen = re.findall(SELECTED, log)
        assert len(seen) == 3 and all(a == b and int(b) >= 20 for a, b in seen), seen
        assert re.findall(BITS, log) == ["9"]
        assert len(re.findall(TALLY_LINE, log)) == 3
    finally:
        shutil.rmtree(work, ignore_errors=True)
