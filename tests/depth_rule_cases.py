"""The depth rule of the emission scores over its whole domain: what tests/test_depth_rule_cpu.py and tests/test_gpu_depth_rule.py share.

The reference's find_most_likely_depth (src/genotype.cpp:1136-1158) takes a k-mer's copy number h in a genotype (0 .. 8), its coverage c (a
byte), its multiplicity f (a byte, never 0), the sample's average coverage (a float) and the upper end of its Poisson interval (a
double), and answers the coverage the k-mer is scored at.  The device restates it as hmm_most_likely_depth (vgmi_hmm.hip).  Here:

  CASES            the averages and intervals the golden tables were recorded at (tests/golden/make_depth_rule_golden.py runs the
                   reference's own function through oracle/ref_harness.cpp's `depthrule`; tests/golden/depth_rule.npz)
  depth_table      the rule as a numpy model, [h, c, f - 1] -> the scored coverage; with `mutant`, one plausible mistake of a kernel
  rows             the rows of the device test: one entry each, every (c, f, flag bit, carrier)
  expected         which term of the (ploidy + 1) x 256 table every genotype of every row must pick, n_kept and the flag byte; with
                   `mutant`, one plausible mistake in the integer rules around the depth rule
  FAMILIES, family_inputs   the device calls and the arrays of each over those rows

The rules around the depth rule, as the reference's hidden_states has them (src/genotype.cpp:697-718) and both emission kernels restate
them: a haplotype counts as carrying an entry if the entry's bit says so, or -- when the entry's last bit (the flag bit) is set and
lower <= c <= upper -- if the row's gt0 names it; the multiplicity 1 of an entry with the flag bit set is scored as 2; a row is flagged
(bit 0) when an entry with c < lower and f >= 2 is carried by any haplotype of the genotypes."""
import collections
import os

import numpy as np

GOLDEN_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_rule.npz")

H_MAX, N_C, N_F = 8, 256, 255      # h 0 .. 8, c 0 .. 255, f 1 .. 255

# (name, average as float32, (lower, upper) or None: the average's own interval)
CASES = [(f"ave{a}", np.float32(a), None) for a in ("0.0", "0.4", "1.0", "7.3", "12.0", "23.5", "33.333332", "42.5", "85.0", "127.5", "200.0", "300.0")]
CASES += [
    ("ave23.5_14_33", np.float32(23.5), (14.0, 33.0)),      # both <= of the interval and the < of flag 1 at c = 14 met with equality
    ("ave12.0_5_19", np.float32(12.0), (5.0, 19.0)),
    # c / upper: 19 f / upper is just below f in double and exactly f in float, for f = 2 .. 13 (h = 0, c = 19 f > ave).  An interval of
    # its own because no plain average tried shows a c / upper taken in float: none of the twelve above, and none of the 4 296 float
    # averages k / 8 (to 256), k / 10 (to 256) and k / 3 (to 100) with their own intervals
    ("ave12.0_5_19next", np.float32(12.0), (5.0, float(np.nextafter(np.float64(19.0), np.inf)))),
]
CASE_NAMES = [name for name, _, _ in CASES]


def poisson_interval(ave):
    """GENOTYPE::calculate_poisson_interval (src/genotype.cpp:932-941) of a float average, in double as observable_states calls it"""
    lam = np.float64(np.float32(ave))
    sd = np.sqrt(lam)
    return float(lam - np.float64(1.96) * sd), float(lam + np.float64(1.96) * sd)


_golden = None


def golden():
    """name -> (ave float32, lower, upper, table (9, 256, 255) uint8) as recorded from the reference"""
    global _golden
    if _golden is None:
        z = np.load(GOLDEN_NPZ)
        names = [str(n) for n in z["names"]]
        ave = z["ave_bits"].astype(np.uint32).view(np.float32)
        _golden = {n: (ave[i], float(z["lower"][i]), float(z["upper"][i]), z["tables"][i]) for i, n in enumerate(names)}
    return _golden


TABLE_MUTANTS = ("ave_h_in_double", "reciprocal_multiply", "round_to_nearest", "c_ge_ave_at_h0", "c_over_upper_in_float")
RULE_MUTANTS = ("interval_lower_lt", "interval_upper_lt", "flag1_f_gt_2", "fj_left_at_1")


def depth_table(ave, upper, mutant=None):
    """find_most_likely_depth for every (h, c, f): (9, 256, 255) uint8, [h, c, f - 1].  c, f, h and ave * h are float32, c / upper is
    float64, float -> byte conversions truncate, the branches stand in the reference's order with f == 1 first."""
    assert mutant is None or mutant in TABLE_MUTANTS
    F32, F64 = np.float32, np.float64
    ave = F32(ave)
    shape = (H_MAX + 1, N_C, N_F)
    h = np.broadcast_to(np.arange(H_MAX + 1, dtype=F32)[:, None, None], shape)
    c = np.broadcast_to(np.arange(N_C, dtype=F32)[None, :, None], shape)
    f = np.broadcast_to(np.arange(1, N_F + 1, dtype=F32)[None, None, :], shape)
    to_byte = np.rint if mutant == "round_to_nearest" else np.trunc
    with np.errstate(divide="ignore", invalid="ignore"):      # (upper = 0 at ave = 0: c / 0 is inf or nan, as in C)
        ah = ave * h                                           # float32
        assert ah.dtype == F32
        if mutant == "ave_h_in_double":
            ah = F64(ave) * h.astype(F64)
        first = (h > 0) & (c > ah)
        # where the first branch is taken ave * h < c <= 255: the conversion to a byte is in range and the device's & 0xFF never acts
        assert np.all(ah[first] < 256)
        above = (c >= ave) if mutant == "c_ge_ave_at_h0" else (c > ave)
        second = ~first & (h == 0) & above
        third = ~first & (h == 0) & ~above
        q = c * (F32(1) / f) if mutant == "reciprocal_multiply" else c / f
        assert q.dtype == F32
        if mutant == "c_over_upper_in_float":
            none = f > c / F32(upper)
        else:
            none = f.astype(F64) > c.astype(F64) / F64(upper)
        out = np.where(first, to_byte(ah), np.where(second, np.where(none, 0, to_byte(q)), np.where(third, to_byte(q), c)))
    out = np.where(f == 1, c, out)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


# ---- the device test's rows ---------------------------------------------------------------------------------------------------------------
Rows = collections.namedtuple("Rows", "c f flag carrier")      # each (n_rows,): carrier 0 = place 0, 1 = a haplotype on no genotype
N_ROWS = 2 * 2 * N_C * N_F


def rows():
    """every (carrier, flag bit, c, f), f fastest: 261 120 rows of one entry each"""
    carrier, flag, c, f = np.meshgrid(np.arange(2), np.arange(2), np.arange(N_C), np.arange(1, N_F + 1), indexing="ij")
    r = Rows(*(x.reshape(-1).astype(np.uint8) for x in (c, f, flag, carrier)))
    assert r.c.size == N_ROWS
    return r


def expected(r, ploidy, table, lower, upper, mutant=None):
    """(index (n_rows, ploidy + 1) int64, n_kept (n_rows,) uint32, flags (n_rows,) uint8) of rows `r` for genotypes j = 0 .. ploidy, where
    genotype j holds j copies of place 0 and ploidy - j copies of place 1, the entry is carried by place 0 or by a haplotype on no
    genotype, and gt0 names place 1: outside the interval place 0 alone carries (h = j, or 0 for the other carrier), inside it place 1
    carries as well (h = ploidy, or ploidy - j)."""
    assert mutant is None or mutant in RULE_MUTANTS
    c, f = r.c.astype(np.float64), r.f.astype(np.int64)
    flagged, on0 = r.flag == 1, r.carrier == 0
    above_lower = (c > lower) if mutant == "interval_lower_lt" else (c >= lower)
    below_upper = (c < upper) if mutant == "interval_upper_lt" else (c <= upper)
    inside = flagged & above_lower & below_upper
    j = np.arange(ploidy + 1, dtype=np.int64)
    h = on0[:, None] * j[None, :] + inside[:, None] * (ploidy - j)[None, :]
    fj = f if mutant == "fj_left_at_1" else np.where(flagged & (f == 1), 2, f)
    cc = table[h, r.c.astype(np.int64)[:, None], (fj - 1)[:, None]].astype(np.int64)
    carried = on0 | inside
    multi = (f > 2) if mutant == "flag1_f_gt_2" else (f >= 2)
    flags = ((c < lower) & multi & carried).astype(np.uint8)
    return h * 256 + cc, np.ones(c.size, dtype=np.uint32), flags


# ---- the device calls ------------------------------------------------------------------------------------------------------------------------
# kind: the vgmi.Context wrapper; ids: the haplotypes at place 0, at place 1 and the one on no genotype
Family = collections.namedtuple("Family", "name kind ploidy bit_len id0 id1 id_off")
FAMILIES = [
    Family("emissions_diploid", "emissions", 2, 6, 3, 20, 31),                              # hmm_emissions_kernel<packed, false, 4>
    Family("emissions_ploidy4", "emissions_pos", 4, 6, 3, 20, 31),
    Family("emissions_ploidy8", "emissions_pos", 8, 6, 3, 20, 31),                          # <packed, false, 8>
    Family("select_packed", "select", 2, 6, 46, 45, 44),                                    # <packed, true, 4>: the carrier directly below the flag bit 47
    Family("select_wide_8", "select_wide", 2, 8, 61, 5, 62),                                # <wide 1, true, 4>
    Family("select_wide_9", "select_wide", 2, 9, 63, 64, 70),                               # <wide 2, true, 4>: the places either side of the word boundary
    Family("select_wide_32", "select_wide", 2, 32, 63, 64, 254),                            # <wide 4, true, 4>
    Family("select_ploidy3", "lists", 3, 6, 46, 45, 44),                                    # hmm_emissions_win_kernel<packed, 4>
    Family("select_ploidy8", "lists", 8, 6, 46, 45, 44),                                    # <packed, 8>
    Family("select_ploidy4_wide_9", "lists_wide", 4, 9, 63, 64, 70),                        # <wide 2, 4>
    Family("select_ploidy8_wide_32", "lists_wide", 8, 32, 63, 64, 254),                     # <wide 4, 8>
    Family("select_ploidy3_wide_8", "lists_wide", 3, 8, 61, 5, 62),                         # <wide 1, 4>: the list kernel's other four
    Family("select_ploidy5_wide_8", "lists_wide", 5, 8, 61, 5, 62),                         # <wide 1, 8>
    Family("select_ploidy5_wide_9", "lists_wide", 5, 9, 63, 64, 70),                        # <wide 2, 8>
    Family("select_ploidy3_wide_32", "lists_wide", 3, 32, 63, 64, 254),                     # <wide 4, 4>
]


def words_of(bit_len):
    return 1 if bit_len <= 8 else 2 if bit_len <= 16 else 4


def _id_words(ids, W):
    m = np.zeros(W, dtype=np.uint64)
    for i in ids:
        m[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return m


def term_tables(ploidy):
    """tables[i] = i + 1: exact and distinct in a long double, so a score of one entry, 1.0L * tables[i], names the term it picked"""
    return np.arange(1, 256 * (ploidy + 1) + 1).astype(np.longdouble)


def family_inputs(fam, r):
    """the arrays of family `fam` over rows `r`, whatever the case: the entries (bits as (n, bit_len) bytes and, for the packed forms, as
    words), the coverages, the row arrays, the genotypes by places and by ids, the masks"""
    n, W, flag_bit = r.c.size, words_of(fam.bit_len), 8 * fam.bit_len - 1
    assert len({fam.id0, fam.id1, fam.id_off}) == 3 and max(fam.id0, fam.id1, fam.id_off) < flag_bit
    bits = np.zeros((n, fam.bit_len), dtype=np.uint8)
    carrier_id = np.where(r.carrier == 0, fam.id0, fam.id_off)
    bits[np.arange(n), carrier_id >> 3] |= (1 << (carrier_id & 7)).astype(np.uint8)
    bits[:, flag_bit >> 3] |= (r.flag << (flag_bit & 7)).astype(np.uint8)
    x = dict(bits=bits, f=r.f.copy(), cov=r.c.copy(), entry_begin=np.arange(n, dtype=np.uint64), entry_count=np.ones(n, dtype=np.uint32),
             row_win=np.zeros(n, dtype=np.uint32), used=[fam.id0, fam.id1])
    if fam.bit_len <= 6:
        padded = np.zeros((n, 8), dtype=np.uint8)
        padded[:, :fam.bit_len] = bits
        x["words"] = (r.f.astype(np.uint64) << np.uint64(8)) | (padded.view("<u8").reshape(n) << np.uint64(16))
    x["pos"] = np.array([[0] * j + [1] * (fam.ploidy - j) for j in range(fam.ploidy + 1)], dtype=np.uint8)
    x["gt0_places"] = np.full(n, 0b10, dtype=np.uint16)
    x["win_haps"] = np.array([[[fam.id0] * j + [fam.id1] * (fam.ploidy - j) for j in range(fam.ploidy + 1)]], dtype=np.uint8)
    x["win_n_gt"] = np.array([fam.ploidy + 1], dtype=np.uint32)
    x["top_words"] = _id_words([fam.id0, fam.id1, fam.id_off], W).reshape(1, W)
    x["gt0_words"] = np.tile(_id_words([fam.id1], W), (n, 1))
    return x
