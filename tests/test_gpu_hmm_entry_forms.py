"""The two storage forms of the node-list entries under one kernel body, one launcher and one C-ABI implementation per family
(vgmi_hmm.hip: HmmPackedEntries, HmmWideEntries<W>; the polyploid tally keeps two kernels behind its one launcher): what shared code could
get wrong in one form only.  The same entries uploaded packed and wide (one word) must give every output array of
all five families -- support, emissions by places, emissions by genotype lists, tallies of a pair, tallies of a polyploid call -- byte for
byte, and both the numpy / host-arithmetic models of the neighbouring test files; two and four words against the models alone.  One
geometry for all: 65 rows in 3 windows whose boundaries lie inside a workgroup's rows (16 rows a workgroup in the list and polyploid-tally
kernels, 64 in the support kernel; row 64 starts a second one), rows of 0, 1, 63, 64, 65 and 130 entries (the tallies' turns of 64), an
entry dead on entry, one the prune kills, one that raises flag bit 0, one inside the interval with the last bit set, and two flagged rows
scored again with fixes on their first and last entries."""
import ctypes as C
import functools

import numpy as np
import pytest

from varigraph_amd import vgmi
from varigraph_amd.vgmi import _ptr
from test_gpu_hmm_select import AVE, LD, LOWER, UPPER, _model_emissions
from test_gpu_hmm_select_ploidy import _blocks, _model as _model_lists
from test_gpu_hmm_wide import _bytes_of, _masks, _model_support, _model_tallies, _panel, _words
from test_gpu_hmm_wide_ploidy import _fix_with, _mask_of, _model_tallies as _model_tallies_ploidy, _word_rows

pytestmark = pytest.mark.gpu

ROW_WIN = np.array([0] * 20 + [1] * 25 + [2] * 20, dtype=np.uint32)      # both boundaries inside rows 16 .. 31 and 32 .. 47
N_ROWS, N_WINDOWS = 65, 3
SIZES = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 130}                       # rows of window 0
CRAFTED, FIX_ROWS = 3, (4, 5)
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
PLOIDIES = (3, 4, 5, 8)                                                  # MAXP = 4 twice, MAXP = 8 twice
TALLY_PLOIDY = 4


def _tables(rng, ploidy):
    """terms of up to twenty decimal orders below one: the product of a row of 130 entries is still a number"""
    return (rng.random(256 * (ploidy + 1)).astype(LD) + LD(0.05)) * np.power(LD(10), rng.integers(-20, 1, size=256 * (ploidy + 1)).astype(LD))


@functools.lru_cache(maxsize=None)
def _case(bit_len):
    """the data of one width, made once: 8 bit_len - 1 haplotypes, the flag bit directly above them"""
    rng = np.random.default_rng(7100 + bit_len)
    n_hap = 8 * bit_len - 1
    last, flag_bit = n_hap - 1, 8 * bit_len - 1
    sizes = {r: int(x) for r, x in enumerate(rng.integers(0, 31, size=N_ROWS))}
    sizes.update(SIZES)
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, N_ROWS, fixed=sizes)
    if n_hap < 24:      # (a dozen carriers per entry would be all of them: a third each)
        bits = [sum(1 << int(h) for h in np.flatnonzero(rng.random(n_hap) < 0.33)) | (b & (1 << flag_bit)) for b in bits]
    # every window selects three haplotypes: the first and the last one (the first and the last word), the ids 63, 64 and bl8 - 2 where the
    # width has them
    used = [[0, n_hap // 2, last], sorted(int(x) for x in rng.choice(n_hap, size=3, replace=False)), [63, 64, last] if n_hap > 64 else [1, 2, last - 1]]
    win_top = [_mask_of(u) for u in used]
    alive0 = (rng.random(len(bits)) < 0.9).astype(np.uint8)
    e = [int(x) for x in entry_begin]
    j = e[CRAFTED]
    alive0[j] = 0                                                          # dead on entry
    alive0[j + 1], bits[j + 1] = 1, (bits[j + 1] & ~win_top[0]) | 2        # no selected haplotype of window 0 carries it: the prune kills it
    alive0[j + 2], cov[j + 2], f[j + 2] = 1, 1, 2                          # under-covered, multi-copy, carried: flag bit 0
    bits[j + 2] |= 1
    alive0[j + 3], cov[j + 3], f[j + 3] = 1, 23, 1                         # inside the interval with the last bit set
    bits[j + 3] |= (1 << flag_bit) | (1 << last)
    assert LOWER <= 23 <= UPPER and not (2 & win_top[0])
    for r in FIX_ROWS:      # the first and the last entry of both rows: alive, flagged, carried by the last haplotype
        for jj in (0, int(counts[r]) - 1):
            alive0[e[r] + jj], cov[e[r] + jj], f[e[r] + jj] = 1, 1, 2
            bits[e[r] + jj] |= 1 << last
    gt0_places = rng.integers(0, 8, size=N_ROWS).astype(np.uint16)
    gt0_ids = [int.from_bytes(rng.bytes(bit_len), "little") & ((1 << n_hap) - 1) for _ in range(N_ROWS)]
    fix_j = [0, int(counts[4]) - 1, 0, int(counts[5]) - 1]
    fix_at = [(4, fix_j[0]), (4, fix_j[1]), (5, fix_j[2]), (5, fix_j[3])]
    lists = {}
    for p in PLOIDIES:
        per_win = [_blocks(u, p, last) for u in used]
        win_haps = np.zeros((N_WINDOWS, max(len(x) for x in per_win), p), dtype=np.uint8)
        for w, x in enumerate(per_win):
            win_haps[w, :len(x)] = np.array(x, dtype=np.uint8)
        lists[p] = (np.array([len(x) for x in per_win], dtype=np.uint32), win_haps, _tables(rng, p))
    winner_pair = rng.integers(0, len(PAIRS), size=N_ROWS).astype(np.uint32)
    winner_pair[::7] = 0xFFFFFFFF
    winner_list = rng.integers(0, lists[TALLY_PLOIDY][1].shape[1], size=N_ROWS).astype(np.uint32)      # (beyond a window's count: zeros)
    winner_list[::7] = 0xFFFFFFFF
    winner_pair[list(SIZES)] = 1
    winner_list[list(SIZES)] = 0
    return dict(bit_len=bit_len, n_hap=n_hap, last=last, counts=counts, entry_begin=entry_begin, f=f, bits=bits, cov=cov, alive0=alive0, used=used, win_top=win_top,
                gt0_places=gt0_places, gt0_ids=gt0_ids, tables2=_tables(rng, 2), lists=lists, winner_pair=winner_pair, winner_list=winner_list,
                fix=([4, 5], [0, 2, 4], fix_j), fix_places=dict(zip(fix_at, (0b100, 0b101, 0b100, 0b110))), fix_ids=dict(zip(fix_at, [1 << last] * 4)), crafted=j)


@functools.lru_cache(maxsize=None)
def _expected(bit_len):
    """what the models say, in the order _run returns it"""
    c = _case(bit_len)
    f, bits, cov, counts, eb = c["f"], c["bits"], c["cov"], c["counts"], c["entry_begin"]
    want = [_model_support(f, bits, cov, c["alive0"], c["n_hap"], N_WINDOWS, eb, counts, ROW_WIN).astype(np.uint32)]
    alive = c["alive0"].copy()
    want += list(_model_emissions(f, bits, cov, alive, bit_len, PAIRS, c["used"], c["tables2"], eb, counts, ROW_WIN, c["gt0_places"]))
    want += [alive.copy()]
    want += list(_model_emissions(f, bits, cov, alive, bit_len, PAIRS, c["used"], c["tables2"], eb, counts, ROW_WIN, c["gt0_places"], fixes=c["fix_places"]))
    want += [alive.copy()]
    want += list(_model_tallies(f, bits, cov, alive, PAIRS, c["used"], eb, counts, ROW_WIN, c["winner_pair"]))
    for p in PLOIDIES:
        win_n, win_haps, tables = c["lists"][p]
        alive = c["alive0"].copy()
        want += list(_model_lists(f, bits, cov, alive, bit_len, win_n, win_haps, c["win_top"], tables, eb, counts, ROW_WIN, c["gt0_ids"]))
        want += [alive.copy()]
        want += list(_model_lists(f, bits, cov, alive, bit_len, win_n, win_haps, c["win_top"], tables, eb, counts, ROW_WIN, c["gt0_ids"], fixes=c["fix_ids"]))
        want += [alive.copy()]
        if p == TALLY_PLOIDY:
            want += list(_model_tallies_ploidy(p, bit_len, f, bits, cov, alive, win_n, win_haps, c["win_top"], eb, counts, ROW_WIN, c["winner_list"]))
    return want


def _run(bit_len, form):
    """every family once on one context: support, emissions by places (and their fix launch), the pair's tallies on the pruned lists, then per
    ploidy -- the alive bytes uploaded afresh -- emissions by genotype lists, their fix launch, and at ploidy 4 the call's tallies"""
    c = _case(bit_len)
    W = _words(bit_len)
    wide = form == "wide"
    counts, eb = c["counts"], c["entry_begin"]
    pos_a, pos_b = [a for a, _ in PAIRS], [b for _, b in PAIRS]
    rows, off, fj = c["fix"]
    fix_places = (rows, off, fj, list(c["fix_places"].values()))
    ids = list(c["fix_ids"].values())
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        if wide:
            ctx.hmm_entries_upload_wide(c["f"], _bytes_of(c["bits"], bit_len), bit_len, c["cov"], c["alive0"])
            top, gt0, fix_ids = _word_rows(c["win_top"], W), _word_rows(c["gt0_ids"], W), (rows, off, fj, _word_rows(ids, W))
            place = lambda **kw: ctx.hmm_emissions_select_wide(pos_a, pos_b, c["used"], _masks(c["used"], bit_len), bit_len, AVE, LOWER, UPPER, c["tables2"], eb,
                                                               counts, ROW_WIN, c["gt0_places"], **kw)
            got = [ctx.hmm_support_wide(bit_len, c["n_hap"], N_WINDOWS, eb, counts, ROW_WIN)]
        else:
            entries = (c["f"].astype(np.uint64) << np.uint64(8)) | (np.array(c["bits"], dtype=np.uint64) << np.uint64(16))
            ctx.hmm_entries_upload(entries, c["cov"], c["alive0"])
            top, gt0, fix_ids = np.array(c["win_top"], dtype=np.uint64), np.array(c["gt0_ids"], dtype=np.uint64), (rows, off, fj, ids)
            place = lambda **kw: ctx.hmm_emissions_select(pos_a, pos_b, c["used"], top, bit_len, AVE, LOWER, UPPER, c["tables2"], eb, counts, ROW_WIN,
                                                          c["gt0_places"], **kw)
            got = [ctx.hmm_support(c["n_hap"], N_WINDOWS, eb, counts, ROW_WIN)]
        got += [*place(), ctx.hmm_alive_fetch(), *place(fixes=fix_places), ctx.hmm_alive_fetch()]
        if wide:
            got += list(ctx.hmm_tallies_select_wide(bit_len, eb, counts, ROW_WIN, c["winner_pair"], pos_a, pos_b, c["used"]))
        else:
            got += list(ctx.hmm_tallies_select(eb, counts, ROW_WIN, c["winner_pair"], pos_a, pos_b, c["used"]))
        for p in PLOIDIES:
            win_n, win_haps, tables = c["lists"][p]
            ctx.hmm_alive_upload(c["alive0"])
            emit = ctx.hmm_emissions_select_ploidy_wide if wide else ctx.hmm_emissions_select_ploidy
            a = (p, win_n, win_haps, top, bit_len, AVE, LOWER, UPPER, tables, eb, counts, ROW_WIN, gt0)
            got += [*emit(*a), ctx.hmm_alive_fetch(), *emit(*a, fixes=fix_ids), ctx.hmm_alive_fetch()]
            if p == TALLY_PLOIDY and wide:
                got += list(ctx.hmm_tallies_ploidy_wide(bit_len, p, win_haps, top, eb, counts, c["winner_list"], row_win=ROW_WIN, win_n_gt=win_n))
            elif p == TALLY_PLOIDY:
                got += list(ctx.hmm_tallies_ploidy(p, win_haps, top, eb, counts, c["winner_list"], row_win=ROW_WIN, win_n_gt=win_n))
    finally:
        ctx.close()
    return got


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), (what, i, np.argwhere(a != b)[:5].tolist())      # every row, every entry's alive byte


def _the_case_bites(bit_len, got):
    """the geometry's special entries did what they are there for"""
    c = _case(bit_len)
    j, alive0 = c["crafted"], c["alive0"]
    support, obs, n_kept, flags, alive1, obs_f, n_kept_f, flags_f, alive1f, tally, uniq = got[:11]
    assert support.any() and (obs > 0).any() and tally.any() and uniq.any()
    assert alive0[j] == 0 and alive0[j + 1] == 1 and alive1[j + 1] == 0 and alive1[j + 2] == 1 and alive1[j + 3] == 1
    assert flags[CRAFTED] & 1 and all(flags[r] & 1 for r in FIX_ROWS) and n_kept[0] == 0 and (obs[0] == 1).all()
    assert np.array_equal(alive1f, alive1) and np.array_equal(n_kept_f, n_kept) and np.array_equal(flags_f, flags)
    changed = np.flatnonzero((obs_f != obs).any(axis=1))
    assert changed.tolist() == list(FIX_ROWS)
    assert tally[2].any() and tally[3].any() and tally[4].any() and tally[5].any()      # 63, 64, 65 and 130 entries


@pytest.mark.parametrize("bit_len", [1, 2, 6])
def test_packed_and_wide_entries_give_the_same_bytes_and_the_models_numbers(bit_len):
    """1, 2 and 6 bytes of haplotype bits (7 haplotypes with the flag bit directly above them; 15; 47): everything the five families return,
    the alive bytes after every prune and every fix launch included, is the same after hmm_entries_upload and after hmm_entries_upload_wide,
    and is what the models compute.  Genotype lists of ploidy 3, 4, 5 and 8: both MAXP instantiations of the list kernel in both forms."""
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    packed, wide = _run(bit_len, "packed"), _run(bit_len, "wide")
    _same(wide, packed, "wide against packed")
    _same(packed, _expected(bit_len), "packed against the models")
    _the_case_bites(bit_len, packed)


@pytest.mark.parametrize("bit_len", [9, 32])
def test_entries_of_two_and_four_words_equal_the_models(bit_len):
    """9 and 32 bytes (W = 2 and 4): the same geometry with selected haplotypes in the first and in the last word and at 63, 64 and bl8 - 2"""
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    c = _case(bit_len)
    assert c["used"][2] == [63, 64, 8 * bit_len - 2] and c["used"][0][0] == 0 and c["used"][0][2] >> 6 == _words(bit_len) - 1
    got = _run(bit_len, "wide")
    _same(got, _expected(bit_len), "wide against the models")
    _the_case_bites(bit_len, got)


# ---- a part of the wrong kind at each of the three fix launches ------------------------------------------------------------------------------
def _place_part_fix(ctx, wide, fix_name, mask_type, bit_len, c):
    """a part of vgmi_hmm_emissions_select(_wide) straight from the C ABI, handed to the fix launch `fix_name`; raises what it answers"""
    pos_a, pos_b = (np.array(x, dtype=np.uint8) for x in zip(*PAIRS))
    used = np.array(c["used"], dtype=np.uint8)
    top = _masks(c["used"], bit_len) if wide else np.array(c["win_top"], dtype=np.uint64)
    tables = np.ascontiguousarray(c["tables2"], dtype=np.longdouble)
    eb, counts = np.ascontiguousarray(c["entry_begin"], dtype=np.uint64), np.ascontiguousarray(c["counts"], dtype=np.uint32)
    n_kept, flags = np.zeros(N_ROWS, dtype=np.uint32), np.zeros(N_ROWS, dtype=np.uint8)
    part = C.c_void_p()
    emit = ctx._l.vgmi_hmm_emissions_select_wide if wide else ctx._l.vgmi_hmm_emissions_select
    ctx._chk(emit(ctx._h, len(PAIRS), 3, _ptr(pos_a), _ptr(pos_b), N_WINDOWS, _ptr(used), _ptr(top), bit_len, float(AVE), float(LOWER), float(UPPER), _ptr(tables),
                  N_ROWS, _ptr(eb), _ptr(counts), _ptr(ROW_WIN), _ptr(c["gt0_places"]), _ptr(n_kept), _ptr(flags), C.byref(part)))
    try:
        rows, off, j, m = np.array([1], dtype=np.uint64), np.array([0, 1], dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.zeros(4, dtype=mask_type)
        ctx._chk(getattr(ctx._l, fix_name)(part, 1, _ptr(rows), _ptr(off), _ptr(j), _ptr(m)))
    finally:
        ctx._l.vgmi_hmm_part_free(part)


def test_each_fix_launch_takes_its_own_kind_of_part_and_refuses_the_other_three():
    """Four kinds of part -- by places or by genotype lists, over packed or wide entries -- and three fix launches: vgmi_hmm_part_fix_rows serves
    both parts by places, vgmi_hmm_part_fix_rows_wide the packed part by lists, vgmi_hmm_part_fix_rows_ploidy_wide the wide part by lists; every
    other pairing is refused with the code it has always had, and the context serves on."""
    bit_len = 6
    c = _case(bit_len)
    win_n, win_haps, tables = c["lists"][4]
    common = (tables, c["entry_begin"], c["counts"], ROW_WIN)
    lists_packed = (4, win_n, win_haps, np.array(c["win_top"], dtype=np.uint64), bit_len, *common, np.array(c["gt0_ids"], dtype=np.uint64))
    lists_wide = (4, win_n, win_haps, _word_rows(c["win_top"], 1), bit_len, *common, _word_rows(c["gt0_ids"], 1))
    fix_launches = [("vgmi_hmm_part_fix_rows", np.uint16), ("vgmi_hmm_part_fix_rows_wide", np.uint64), ("vgmi_hmm_part_fix_rows_ploidy_wide", np.uint64)]
    #            kind of part -> what each of the three launches answers (None: served)
    answers = {("places", False): (None, vgmi.E_INVALID, vgmi.E_STATE), ("places", True): (None, vgmi.E_INVALID, vgmi.E_STATE),
               ("lists", False): (vgmi.E_INVALID, None, vgmi.E_STATE), ("lists", True): (vgmi.E_STATE, vgmi.E_STATE, None)}
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        for wide in (False, True):
            if wide:
                ctx.hmm_entries_upload_wide(c["f"], _bytes_of(c["bits"], bit_len), bit_len, c["cov"], c["alive0"])
            else:
                ctx.hmm_entries_upload((c["f"].astype(np.uint64) << np.uint64(8)) | (np.array(c["bits"], dtype=np.uint64) << np.uint64(16)), c["cov"], c["alive0"])
            for kind in ("places", "lists"):
                for (fix_name, mask_type), code in zip(fix_launches, answers[(kind, wide)]):
                    def launch():
                        if kind == "places":
                            _place_part_fix(ctx, wide, fix_name, mask_type, bit_len, c)
                        else:
                            _fix_with(ctx, fix_name, mask_type, "vgmi_hmm_emissions_select_ploidy" + ("_wide" if wide else ""), lists_wide if wide else lists_packed)
                    if code is None:
                        launch()
                    else:
                        with pytest.raises(vgmi.VgmiError) as err:
                            launch()
                        assert err.value.code == code, (kind, wide, fix_name, err.value.code, str(err.value))
    finally:
        ctx.close()


# ---- the packed polyploid tally's own rule for an id ---------------------------------------------------------------------------------------------
def test_packed_polyploid_tally_takes_any_id_below_64_that_the_mask_holds():
    """vgmi_hmm_tallies_ploidy does not know bit_len: an id counts if it is below 64 and in the window's mask.  So at two bytes of haplotype
    bits (flag bit 15) a called genotype of the ids 47, 50, 15 and 3 with 47, 50 and 15 in the mask reads: 47 and 50 zero bits (the packed word
    holds 48 bits and these entries have 16), 15 THE FLAG BIT like any other -- the entries that have it set and their coverages -- and 3,
    which the mask does not hold, (0, 0).  A winner at and beyond the window's count reads zeros.  These are the values the packed kernel has
    always returned (recorded from the parent commit's library on an MI355X); vgmi_hmm_tallies_ploidy_wide, which knows bit_len, reads (0, 0)
    for the id 15 = bl8 - 1 on the same entries."""
    bit_len, ploidy = 2, 4
    c = _case(bit_len)
    f, bits, cov, alive0, counts, eb = c["f"], c["bits"], c["cov"], c["alive0"], c["counts"], c["entry_begin"]
    win_haps = np.zeros((N_WINDOWS, 3, ploidy), dtype=np.uint8)
    win_haps[:, 0] = [47, 50, 15, 3]
    win_haps[:, 1] = [0, 1, 2, 14]
    win_n = np.array([2, 1, 2], dtype=np.uint32)
    sel = [(1 << 47) | (1 << 50) | (1 << 15) | 0b111 | (1 << 14)] * N_WINDOWS      # (3 is not in it)
    winner = np.zeros(N_ROWS, dtype=np.uint32)
    winner[1::2] = 1                # window 1 has one genotype: its odd rows name a winner AT the count
    winner[30] = 2                  # ... and this one beyond it (window 1)
    winner[6] = 0xFFFFFFFF
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        ctx.hmm_entries_upload((f.astype(np.uint64) << np.uint64(8)) | (np.array(bits, dtype=np.uint64) << np.uint64(16)), cov, alive0)
        out, uniq = ctx.hmm_tallies_ploidy(ploidy, win_haps, np.array(sel, dtype=np.uint64), eb, counts, winner, row_win=ROW_WIN, win_n_gt=win_n)
        ctx.hmm_entries_upload_wide(f, _bytes_of(bits, bit_len), bit_len, cov, alive0)
        out_w, uniq_w = ctx.hmm_tallies_ploidy_wide(bit_len, ploidy, win_haps, _word_rows(sel, 1), eb, counts, winner, row_win=ROW_WIN, win_n_gt=win_n)
    finally:
        ctx.close()
    want = np.zeros((N_ROWS, 2 * ploidy), dtype=np.uint32)
    want_w = np.zeros_like(want)
    want_u = np.zeros(N_ROWS, dtype=np.uint8)
    for r in range(N_ROWS):
        g = int(winner[r])
        if g >= win_n[ROW_WIN[r]]:
            continue
        for j in range(int(eb[r]), int(eb[r]) + int(counts[r])):
            if not alive0[j]:
                continue
            want_u[r] += f[j] <= 1
            for q, h in enumerate(int(x) for x in win_haps[0, g]):
                if (sel[0] >> h) & 1 and (bits[j] >> h) & 1:      # (the entries' integers have 16 bits: ids 47 and 50 find none)
                    for w_, counted in ((want, True), (want_w, h < 8 * bit_len - 1)):
                        if counted:
                            w_[r, 2 * q] += 1
                            w_[r, 2 * q + 1] += int(cov[j])
    assert np.array_equal(out, want) and np.array_equal(uniq, want_u)
    assert np.array_equal(out_w, want_w) and np.array_equal(uniq_w, want_u)
    zero = winner == 0
    assert not out[zero][:, 0:4].any() and out[zero, 4].any() and not out[zero][:, 6:8].any() and not out_w[zero].any()      # 47, 50: zeros; 15: the flag bit; 3: not held
    assert out[winner == 1][:, 0].any() and not out[ROW_WIN == 1][1::2].any() and not out[30].any() and not out[6].any() and uniq[6] == 0
