"""The model of the read filter by length and read quality (genotype --min-read-length / --max-read-length / --min-read-quality /
--max-low-quality, vgmi_fastq_set_read_filter; the rule of csrc/vgmi_read_filter.h) and the read files its tests use
(test_read_filter_cpu.py, test_gpu_read_filter.py, test_gpu_read_filter_cli.py).  No device involved.

The rule, all in integers:

    q of a base    FASTQ: clamp(byte - 33, 0, 93) on the unsigned byte      BAM: min(QUAL, 93); QUAL[0] == 0xff: the record has none
    E10[t]       = round_half_even(10^(-t/100) * 2^30), t = 0 .. 930          (computed here with decimal)      E[q] = E10[10 q]
    1 short         len < min_len
    2 long          max_len and len > max_len
    3 low fraction  lowq_below and cnt(q < lowq_below) * 100 > lowq_max_pct * len
    4 low mean      min_mean_q and sum E[q_i] > E10[min_mean_q] * len
    the first test that fails is the read's class; a read without qualities takes the length tests only.

A dropped read is not a read.  So counting file G with the rule equals counting G' with the option off, where G' is G with exactly
the failing reads removed: the builders below give G and G'.  A FASTQ record is (name, seq, qual[, shape]) as in quality_mask_cases.py."""
from decimal import ROUND_HALF_EVEN, Decimal, getcontext

import numpy as np

import bam_py as B
import quality_mask_cases as Q
import subsample_cases as S

PASS, SHORT, LONG_, LOW_FRACTION, LOW_MEAN = 0, 1, 2, 3, 4
CLASS_NAMES = ("pass", "short", "long", "low fraction", "low mean")


def _e10():
    getcontext().prec = 80
    return [int((Decimal(10) ** (Decimal(-t) / Decimal(100)) * Decimal(2 ** 30)).quantize(Decimal(1), rounding=ROUND_HALF_EVEN)) for t in range(931)]


E10 = _e10()
E10_NP = np.array(E10, dtype=np.uint64)


def q_fastq(byte):
    return min(max(byte - 33, 0), 93)


def q_bam(byte):
    return min(byte, 93)


class Rule:
    def __init__(self, min_len=0, max_len=0, min_mean_q=0, lowq_below=0, lowq_max_pct=0):
        self.min_len, self.max_len, self.min_mean_q, self.lowq_below, self.lowq_max_pct = min_len, max_len, min_mean_q, lowq_below, lowq_max_pct

    def dict(self):
        return dict(min_len=self.min_len, max_len=self.max_len, min_mean_q=self.min_mean_q, lowq_below=self.lowq_below, lowq_max_pct=self.lowq_max_pct)

    def line(self):
        return "%d %d %d %d %d" % (self.min_len, self.max_len, self.min_mean_q, self.lowq_below, self.lowq_max_pct)

    @property
    def quality(self):
        return bool(self.min_mean_q or self.lowq_below)

    def __repr__(self):
        return "Rule(%s)" % self.line()

    # the tests, each its own method so that a mutated rule replaces one
    def is_short(self, n):
        return n < self.min_len

    def is_long(self, n):
        return bool(self.max_len) and n > self.max_len

    def q_of(self, byte, bam):
        return q_bam(byte) if bam else q_fastq(byte)

    def weight(self, q):
        return E10[10 * q]

    def is_low_fraction(self, n, n_low):
        return bool(self.lowq_below) and n_low * 100 > self.lowq_max_pct * n

    def is_low_mean(self, n, sum_e, qs):
        return bool(self.min_mean_q) and sum_e > E10[self.min_mean_q] * n

    def classify(self, n, qual=None, bam=False):
        """(class, n_low, sum_e) of a read of n bases; qual: its quality bytes as stored, or None (FASTA).  The sums are 0 where no
        quality test evaluated them."""
        if self.is_short(n):
            return SHORT, 0, 0
        if self.is_long(n):
            return LONG_, 0, 0
        if not self.quality or qual is None or n == 0 or (bam and qual[0] == 0xFF):
            return PASS, 0, 0
        qs = [self.q_of(b, bam) for b in qual]
        n_low = sum(1 for q in qs if q < self.lowq_below)
        sum_e = sum(self.weight(q) for q in qs)
        if self.is_low_fraction(n, n_low):
            return LOW_FRACTION, n_low, sum_e
        if self.is_low_mean(n, sum_e, qs):
            return LOW_MEAN, n_low, sum_e
        return PASS, n_low, sum_e

    def cls(self, n, qual=None, bam=False):
        return self.classify(n, qual, bam)[0]


# ---- the mutated rules: each must change a verdict on the case set --------------------------------------------------------------------
class MeanGreaterEqual(Rule):      # >= for > in the mean test
    def is_low_mean(self, n, sum_e, qs):
        return bool(self.min_mean_q) and sum_e >= E10[self.min_mean_q] * n


class MeanOfPhred(Rule):           # the mean of the Phred values
    def is_low_mean(self, n, sum_e, qs):
        return bool(self.min_mean_q) and sum(qs) * 10 < self.min_mean_q * n


class NoClamp(Rule):               # byte - 33 / QUAL as they are
    def q_of(self, byte, bam):
        return byte if bam else byte - 33

    _w = {}

    def weight(self, q):
        if q not in self._w:
            getcontext().prec = 80
            self._w[q] = int((Decimal(10) ** (Decimal(-q) / Decimal(10)) * Decimal(2 ** 30)).quantize(Decimal(1), rounding=ROUND_HALF_EVEN))
        return self._w[q]


class FractionIntegerDivision(Rule):
    def is_low_fraction(self, n, n_low):
        return bool(self.lowq_below) and n_low * 100 // n > self.lowq_max_pct


class ShortLessEqual(Rule):        # len <= min_len
    def is_short(self, n):
        return n <= self.min_len


MUTATIONS = (MeanGreaterEqual, MeanOfPhred, NoClamp, FractionIntegerDivision, ShortLessEqual)

# ---- the parameters --------------------------------------------------------------------------------------------------------------------
MIN_LEN, MAX_LEN, MEAN_Q, LOW_Q, LOW_PCT = 40, 20000, 150, 15, 40
LONG = 20000
RULES = {
    "short": Rule(min_len=MIN_LEN),
    "long": Rule(max_len=MAX_LEN),
    "lengths": Rule(min_len=MIN_LEN, max_len=MAX_LEN),
    "fraction": Rule(lowq_below=LOW_Q, lowq_max_pct=LOW_PCT),
    "mean": Rule(min_mean_q=MEAN_Q),
    "all": Rule(MIN_LEN, MAX_LEN, MEAN_Q, LOW_Q, LOW_PCT),
}
ALL = RULES["all"]


# ---- the reads -------------------------------------------------------------------------------------------------------------------------
def _ph(values):
    """Phred values -> FASTQ quality bytes"""
    return bytes(v + 33 for v in values)


def special_fastq(d):
    """the named cases as FASTQ records (d: a _Draw of subsample_cases); the comments give the class under ALL"""
    uq = MEAN_Q // 10
    good = lambda n: _ph([40] * n)
    r = []
    for n in (MIN_LEN - 1, MIN_LEN, 1, 63, 64, 65):                                        # short below MIN_LEN, else pass
        r.append((b"len%d" % n, d.seq(n), good(n)))
    r.append((b"uniform", d.seq(100), _ph([uq] * 100)))                                     # the mean equals the bound: pass
    r.append((b"uniform_one_lower", d.seq(100), _ph([uq] * 99 + [uq - 1])))                 # low mean
    r.append((b"phred_mean_passes", d.seq(100), _ph(([40] * 9 + [2]) * 10)))                # mean Phred 36.2, mean error 0.063: low mean
    r.append((b"fraction_equal", d.seq(100), _ph(([LOW_Q - 1] * 2 + [40] * 3) * 20)))       # 40 of 100 low: pass
    r.append((b"fraction_one_more", d.seq(100), _ph([LOW_Q - 1] * 41 + [40] * 59)))         # low fraction
    r.append((b"fraction_half_percent", d.seq(200), _ph([LOW_Q - 1] * 81 + [40] * 119)))    # 40.5 %: low fraction (integer division keeps it)
    r.append((b"bang_tilde", d.seq(100), b"!" * 3 + b"~" * 97))                             # q 0 and q 93: mean error 0.03: pass
    r.append((b"below33_above126", d.seq(100), b"\x20\x1f\x01" + b"\x7f\xff\x80" + b"I" * 94))   # q 0 x 3, q 93 x 3: pass; unclamped: low mean
    r.append((b"all_bang", d.seq(64), b"!" * 64))                                            # low fraction (and low mean: the first is its class)
    r.append((b"short_and_low", d.seq(10), b"!" * 10))                                       # short (and low fraction, low mean)
    r.append((b"max_len_plus_1", d.seq(MAX_LEN + 1), good(MAX_LEN + 1)))                    # long
    return r


def drawn_quality(rng, n, kind):
    """Phred values of a drawn read: 0 good (20..41, a few percent low), 1 poor (3..17), 2 half of its bases low, 3 noisy tail, 4 a
    noisy third (36 % of its bases at Q1: below a 40 % bound of the fraction test, a mean error of 0.29)"""
    if kind == 0:
        ql = rng.integers(20, 42, size=n)
        pick = rng.random(n) < 0.04
        ql[pick] = rng.integers(2, 20, size=int(pick.sum()))
    elif kind == 1:
        ql = rng.integers(3, 18, size=n)
    elif kind == 2:
        ql = rng.integers(25, 41, size=n)
        ql[rng.random(n) < 0.5] = 14
    elif kind == 3:
        ql = rng.integers(30, 41, size=n)
        ql[n - n // 10:] = 3
    else:
        ql = rng.integers(30, 41, size=n)
        ql[:n * 36 // 100] = 1
    return [int(v) for v in ql]


def fastq_records(haps=None, n=600, seed=3):
    """n records: the named cases in front, then drawn reads (lengths 1 .. 150 among the first 40 of them, else 151; qualities of
    four kinds), the records at n // 4 and n // 2 of 20 000 bases -- = MAX_LEN: the first good, the second with a mean error above
    the bound"""
    d = S._Draw(haps, 11000 + seed)
    rng = np.random.default_rng(12000 + seed)
    recs = special_fastq(d)
    first = len(recs)
    for i in range(first, n):
        if i == n // 4:
            recs.append((b"long_kept", d.seq(LONG), _ph(drawn_quality(rng, LONG, 0))))
            continue
        if i == n // 2:
            recs.append((b"long_dropped", d.seq(LONG), _ph(drawn_quality(rng, LONG, 3))))
            continue
        j = i - first
        ln = 1 + (j * 37) % 150 if j < 40 else 151
        kind = (0, 0, 0, 1, 0, 2, 0, 3)[i % 8]
        recs.append((b"r%d" % i, d.seq(ln), _ph(drawn_quality(rng, ln, kind))))
    return recs


def fastq_classes(recs, rule):
    return [rule.cls(len(r[1]), r[2]) for r in recs]


def fastq_text(recs, final_newline=True):
    return Q.fastq_text(recs, final_newline)


def class_counts(classes):
    """(evaluated, short, long, low fraction, low mean): what the stats entries report"""
    return (len(classes),) + tuple(sum(1 for c in classes if c == k) for k in (SHORT, LONG_, LOW_FRACTION, LOW_MEAN))


def bam_records(haps=None, n=300, seed=3):
    """n reads as BAM records with secondary, supplementary and SEQ '*' records in between: the FASTQ cases' lengths and quality shapes
    (QUAL = the Phred values), and what only BAM has: QUAL 0, 93, 94 and 254, and records whose QUAL[0] is 0xff"""
    d = S._Draw(haps, 13000 + seed)
    rng = np.random.default_rng(14000 + seed)
    recs = []
    for name, seq, qual in special_fastq(d):
        if len(seq) > 1000:
            continue                      # (a BAM record of 20 000 bases: its own case below, shorter than the 64 KiB chunks of the test)
        recs.append(B.Rec(name, seq, flag=4, qual=bytes(q_fastq(b) for b in qual)))
    recs.append(B.Rec(b"qual_0_93_94_254", d.seq(100), flag=4, qual=bytes([0] * 3 + [93, 94, 254] * 10 + [40] * 67)))      # pass, as bang_tilde
    recs.append(B.Rec(b"qual_254_low_half", d.seq(100), flag=16, qual=bytes([254] * 59 + [0] * 41)))                      # low fraction
    recs.append(B.Rec(b"no_qual", d.seq(77), flag=4, qual=b"\xff" + bytes(76)))                    # zeros behind 0xff: passes both quality tests
    recs.append(B.Rec(b"no_qual_short", d.seq(10), flag=4, qual=b"\xff" * 10))                     # short
    recs.append(B.Rec(b"long_20000", d.seq(LONG), flag=4, qual=bytes(drawn_quality(rng, LONG, 0))))
    recs.append(B.Rec(b"long_20001", d.seq(LONG + 1), flag=4, qual=bytes(drawn_quality(rng, LONG + 1, 0))))     # long
    turn = 0
    i = sum(1 for r in recs if r.kept)
    while i < n:
        ln = 1 + (i * 37) % 150 if i < 60 else 101 + i % 50
        kind = (0, 0, 0, 1, 0, 2, 0, 3)[i % 8]
        recs.append(B.Rec(b"r%d" % i, d.seq(ln), flag=4 if i % 3 else 16, qual=bytes(drawn_quality(rng, ln, kind))))
        i += 1
        if i % 2:
            k = turn % 3
            turn += 1
            # non-reads of low quality and of a length the rule would drop: they have no number and are not evaluated
            recs.append(B.Rec(b"sec%d" % i, d.seq(30), flag=0x100, qual=bytes(30)) if k == 0 else
                        B.Rec(b"sup%d" % i, d.seq(77), flag=0x800, qual=bytes(77)) if k == 1 else B.Rec(b"star%d" % i, b"", flag=4))
    return recs


def bam_class(r, rule):
    return rule.cls(len(r.seq), r.qual, bam=True)


def bam_filtered(recs, rule, sub=None, first=0):
    """(G': the records without the reads that subsampling (sub = (F, S) or None) or the rule drops -- the non-reads stay --, the
    classes of the evaluated reads, the reads numbered)"""
    out, classes, i = [], [], first
    for r in recs:
        if not r.kept:
            out.append(r)
            continue
        keep = sub is None or S.keep(i, sub[1], sub[0])
        i += 1
        if not keep:
            continue
        c = bam_class(r, rule)
        classes.append(c)
        if c == PASS:
            out.append(r)
    return out, classes, i - first


def fastq_filtered(recs, rule, sub=None, first=0):
    """(the records of G', the classes of the evaluated records)"""
    out, classes = [], []
    for i, r in enumerate(recs):
        if sub is not None and not S.keep(first + i, sub[1], sub[0]):
            continue
        c = rule.cls(len(r[1]), r[2]) if len(r) < 4 or r[3] != "fasta" else rule.cls(len(r[1]))
        classes.append(c)
        if c == PASS:
            out.append(r)
    return out, classes


def fasta_filtered(recs, rule):
    """FASTA: the length tests alone"""
    out, classes = [], []
    for r in recs:
        c = rule.cls(len(r[1]))
        classes.append(c)
        if c == PASS:
            out.append(r)
    return out, classes


def filtered_fastq_text(text, rule):
    """(G', classes) of a four-line FASTQ text G"""
    lines = text.split(b"\n")
    n = (len(lines) - 1) // 4
    classes = [rule.cls(len(lines[4 * i + 1]), lines[4 * i + 3]) for i in range(n)]
    return b"".join(b"\n".join(lines[4 * i:4 * i + 4]) + b"\n" for i in range(n) if classes[i] == PASS), classes


def check_file_lines(rule, items):
    """the input of tests/native/read_filter_check.cpp `classify`: items = ('F' | 'B', quality bytes) or ('N', length)"""
    out = [rule.line()]
    for kind, v in items:
        out.append("N %d" % v if kind == "N" else "%s %s" % (kind, bytes(v).hex()))
    return "\n".join(out) + "\n"
