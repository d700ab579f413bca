"""Constructed inputs for the HMM recursion kernels (vgmi_hmm.hip) -- operands the random rows of test_gpu_hmm.py never contain -- and the
numpy.longdouble model they are held against, with the kernels' two skip rules written in as an option.  Shared by test_hmm_edges_cpu.py
(the rules and their mutants against the plain model, no GPU) and test_gpu_hmm_edges.py (the kernels against the plain model).

How a term is placed.  A restart row of powers of two whose sum is a power of two normalises exactly (0.5, 0.25, 0.25 stay what they
are), the `pow` tables of a step are arbitrary long doubles, and genotype g's term p is  ((prev_p * keep_pow[k]) * change_pow[ploidy - k])
* obs_g  with k = keep[g, p].  With change_pow = 1 and prev_p a power of two the term is  keep_pow[k] * obs_g  scaled exactly: a keep
matrix that gives a lane the values k = 0, 1, 2 for the previous entries 0, 1, 2 lets a step's table set the lane's three terms.

The skip rules (vgmi_hmm.hip).  Term loop: a lane calls a term nothing when  r.e - (st.e + o.e - BIAS + 2) > 64  (exponents of the
normalised values), and the term is left out when a whole wavefront does.  A term 65 binades below the sum is below half an ulp and
changes nothing; one 64 binades down is at least half an ulp and does.  The product's exponent is  st.e + o.e - BIAS  plus 0, 1 or 2: the
significands' product reaches 2, or rounds up to it -- at 64 bits never both, but a DENORMAL product is rounded at fewer bits, and there
it does both ((2^64 - 1)^2 at exponent -2 is the denormal 2^62, exponent 0).  So `+ 2` is tight: term_rule_rows probes a normal product
(exponent + 0 and + 1), denormal_product_rows the `+ 2`.  Total loop: an entry is left out when  total.e - t.e > 64."""
import numpy as np

LD = np.longdouble
BIAS = 16383
ONE = 1 << 63
ALL = (1 << 64) - 1


def ld(m, e):
    """significand m (an integer below 2^64) with bit 63 at 2^e: m * 2^(e - 63), exactly (denormals included, as far as the bits fit)"""
    return np.ldexp(LD(m >> 32) * LD(1 << 32) + LD(m & 0xFFFFFFFF), e - 63)


def den(m):
    """the denormal with significand field m"""
    return ld(m, 63 - 16445)


def n80_exp(x):
    """VgN80.e of a long double (array): the exponent field its leading bit would have, below 1 for a denormal; 0 for zero"""
    return np.frexp(x)[1].astype(np.int64) + (BIAS - 1)


def chain_model(keep, obs_rows, restart, pows, uniform, ploidy, term_rule=None, total_rule=None):
    """_host_chain of test_gpu_hmm.py (the recursion in x87 long double, the reference's order of operations), with the kernels' skip
    rules as an option: term_rule = (bound, cut) leaves a lane's term out when  r.e - (st.e + o.e - BIAS + bound) > cut  (the kernels: (2,
    64)) -- per lane, without the ballot: the strictest reading; total_rule = cut leaves an entry out of the total when  total.e - t.e >
    cut  (the kernels: 64).  True x87 sums otherwise."""
    n = keep.shape[0]
    out = np.zeros((len(obs_rows), n), dtype=LD)
    prev = None
    for s, o in enumerate(obs_rows):
        if restart[s] or prev is None:
            r = LD(0) + o
        else:
            pk, pc = pows[s, 0], pows[s, 1]
            step = np.zeros((n, ploidy + 1), dtype=LD)
            for k in range(ploidy + 1):
                step[:, k] = (prev * pk[k]) * pc[ploidy - k]
            r = np.zeros(n, dtype=LD)
            for p in range(n):
                if not step[p].any():
                    continue                        # every term is + 0
                st = step[p, keep[:, p]]
                new = r + st * o
                if term_rule is not None:
                    bound, cut = term_rule
                    nothing = (st == 0) | (o == 0) | ((r != 0) & (n80_exp(r) - (n80_exp(st) + n80_exp(o) - BIAS + bound) > cut))
                    new = np.where(nothing, r, new)
                r = new
        total = LD(0)
        for g in range(n):
            t = r[g]
            if total_rule is not None and (t == 0 or (total != 0 and int(n80_exp(total)) - int(n80_exp(t)) > total_rule)):
                continue
            total = total + t
        out[s] = r / total if total > 0 else uniform
        prev = out[s]
    return out


class Rows:
    """what Context.hmm_recursion takes, built step by step"""

    def __init__(self, n, ploidy, keep):
        self.n, self.ploidy, self.keep = n, ploidy, np.ascontiguousarray(keep, dtype=np.uint8)
        self.obs, self.row, self.restart, self.pows, self.chains, self.what = [], [], [], [], [], []
        self.uniform = LD(1) / LD(n)

    def add_row(self, values):
        o = np.zeros(self.n, dtype=LD)
        o[:len(values)] = values
        self.obs.append(o)
        return len(self.obs) - 1

    def chain(self, steps, window=0, what=None):
        """steps: (row, restart, keep_pow or None) -- change_pow is 1 throughout, keep_pow None is 1 as well"""
        first = len(self.row)
        for row, restart, kp in steps:
            self.row.append(row)
            self.restart.append(1 if restart else 0)
            t = np.ones((2, self.ploidy + 1), dtype=LD)
            if kp is not None:
                t[0] = kp
            self.pows.append(t)
            self.what.append(what)
        self.chains.append((first, len(steps), window))

    def arrays(self):
        return self.keep, np.array(self.obs, dtype=LD), self.row, self.restart, np.array(self.pows, dtype=LD), self.uniform, self.chains

    def model(self, **rules):
        keep, obs, row, restart, pows, uniform, chains = self.arrays()
        out = np.zeros((len(row), self.n), dtype=LD)
        for first, count, w in chains:
            out[first:first + count] = chain_model(keep[w], [obs[r] for r in row[first:first + count]], restart[first:first + count],
                                                   pows[first:first + count], uniform, self.ploidy, **rules)
        return out


# ---- the term loop ------------------------------------------------------------------------------------------------------------------
# Five live genotypes, ploidy 3 (four table values a step).  The previous node is 0.5, 0.25, 0.25, 0, 0 (and zero beyond): three terms a lane.
#   lanes 0, 1   k = 3, 3, 2: a leading term 256 times the targets' first, so the probe is nothing to them long before it is to a target
#   lane 2       scores zero: every term is nothing to it
#   lane 3       k = 0, 1, 2: the leading term, a term exactly 63 binades below it (the sum's last bit), the probe
#   lane 4       k = 0, 2, 1: the leading term, the probe, the 63-binades term
# Two wavefronts hold lanes {0, 1, 2} {3, 4}, four {0, 1} {2, 3} {4}; the big kernel has all of them in one.  Whether the wavefront of a
# target computes the probe is the target's decision alone: 64 to 66 binades down "only one genotype needs it", from 67 on nobody does.
LEADS = (ONE, ONE | 1)
PROBES = (ONE, ONE | 1, ALL, 3 << 62)
SCORES = (ONE, ALL - 1, 3 << 62)        # times a probe: below 2; (2^63 + 1)(2^64 - 2) rounds up to 2; 2 or above
DISTANCES = range(60, 71)


def term_rule_rows(n):
    assert n >= 5
    keep = np.ones((1, n, n), dtype=np.uint8)
    k = keep[0]
    k[:2, :2] = 3
    k[:2, 2] = k[2, :2] = 2
    k[2, 2] = 3
    k[3, :3] = k[:3, 3] = [0, 1, 2]
    k[4, :3] = k[:3, 4] = [0, 2, 1]
    k[3, 3] = k[4, 4] = 3
    assert np.array_equal(k, k.T)
    rows = Rows(n, 3, keep)
    start = rows.add_row([ld(ONE, -1), ld(ONE, -2), ld(ONE, -2)])
    lead_e = -100
    for score in SCORES:
        scored = rows.add_row([ld(score, 0), ld(score, 0), 0, ld(score, 0), ld(score, 0)])
        for lead in LEADS:
            for second in (True, False):            # with it the sum's last bit is the other one
                for d in DISTANCES:
                    for probe in PROBES:
                        kp = [ld(lead, lead_e + 1), ld(ONE, lead_e - 63 + 2) if second else LD(0), ld(probe, lead_e - d + 2), ld(ONE, lead_e + 9)]
                        rows.chain([(start, True, None), (scored, False, kp)], what=("term", score, lead, second, d, probe))
    return rows


# ---- the term loop, a denormal product ------------------------------------------------------------------------------------------------
# The same five lanes.  Score and probe have significands of all ones (or all ones but one) and exponents whose sum is -2, -3 or -18: the
# product, rounded at a denormal's precision, lies TWO binades above that sum -- the case the bound's `+ 2` is there for.  The leading term
# puts the running sum 62 to 67 binades above the rounded product, with either last bit (four leading significands, with and without the
# 63-binades term).  At 64 the probe is half an ulp or just above: `+ 1` for `+ 2`, or `> 63` for `> 64`, calls it nothing and is wrong.
DENORMAL_SUMS = (-2, -3, -18)


def denormal_product_rows(n):
    assert n >= 5
    rows = Rows(n, 3, term_rule_rows(n).keep)
    start = rows.add_row([ld(ONE, -1), ld(ONE, -2), ld(ONE, -2)])
    carried = 0
    for score_m in (ALL, ALL - 1):
        score = ld(score_m, -8192)                                          # exponent field 8191
        scored = rows.add_row([score, score, 0, score, score])
        for base in DENORMAL_SUMS:
            probe = ld(ALL, base + BIAS - 8191 - BIAS)                      # field: base + BIAS - 8191
            product = probe * score
            assert 0 < product < np.finfo(LD).tiny
            if n80_exp(product) != base + 2:        # (2^64 - 2)(2^64 - 1) at -2 stays one binade lower: not a case
                continue
            carried += 1
            for lead in (ONE, ONE | 1, ALL, ONE | 2):
                unit = int(n80_exp(ld(lead, 0) * score))
                for second in (True, False):
                    for d in range(62, 68):
                        want = base + 2 + d                                  # the leading term's exponent field
                        lead_e = want - unit                                 # of the table value's leading bit, before the previous entry's 2^-1
                        kp = [ld(lead, lead_e + 1), ld(ONE, lead_e - 63 + 2) if second else LD(0), probe * LD(4), ld(lead, lead_e + 9)]
                        rows.chain([(start, True, None), (scored, False, kp)], what=("denormal product", score_m, lead, second, d, base))
    assert carried == 5
    return rows


# ---- the total ------------------------------------------------------------------------------------------------------------------------
# restart rows: r is the row itself.  A leading entry, an entry 63 binades below it (or none), the probe 62 to 67 binades below, and once
# more half an ulp of the leading entry.
def total_rule_rows(n):
    assert n >= 5
    rows = Rows(n, 2, np.ones((1, n, n), dtype=np.uint8))
    steps = []
    for lead in LEADS:
        for second in (True, False):
            for d in range(62, 68):
                for probe in (ONE, ONE | 1, ALL):
                    r = rows.add_row([ld(lead, -50), ld(ONE, -113) if second else 0, ld(probe, -50 - d), ld(ONE, -114), 0])
                    steps.append((r, True, None))
    rows.chain(steps, what="total")
    return rows


# ---- rows of denormals --------------------------------------------------------------------------------------------------------------
def denormal_rows(n):
    assert n >= 5
    keep = np.ones((2, n, n), dtype=np.uint8)
    keep[1] = 2 * np.eye(n, dtype=np.uint8)          # window 1: a genotype keeps everything of itself and nothing of the others
    rows = Rows(n, 2, keep)
    halves = rows.add_row([ld(ONE, -1), ld(ONE, -2), ld(ONE, -2)])
    quarters = rows.add_row([ld(ONE, -2)] * 4)
    all_den = rows.add_row([den(((g + 1) * 0x9E3779B97F4A7C15 % (1 << 54)) | 1) for g in range(n)])      # n <= 256: the sum stays a denormal
    few_den = rows.add_row([den(0x0123456789ABCDEF), den(1), den((1 << 62) + 12345), den(3), den(0x7FFFFFFF)])
    smallest_normal = rows.add_row([den(1 << 62), den(1 << 62)])
    largest_denormal = rows.add_row([den(1 << 62), den((1 << 62) - 1)])
    ones = rows.add_row([den(1)] * n)
    d = LD(1234)
    recomb = (LD(1) - np.exp(-d / LD(30))) * (LD(1) / LD(30))
    no_recomb = np.exp(-d / LD(30)) + recomb
    real = [no_recomb ** LD(k) for k in range(3)]
    for w in (0, 1):
        rows.chain([(halves, True, None), (all_den, False, None), (few_den, False, real),      # denormal scores on a continuing step
                    (all_den, True, None), (all_den, False, real), (few_den, True, None), (few_den, False, None),     # ... and on a restart step
                    (smallest_normal, True, None), (few_den, False, real), (largest_denormal, True, None), (all_den, False, real),
                    (quarters, True, None), (ones, False, None),       # every product underflows to zero: the uniform fallback, not at a restart
                    (all_den, False, real)], window=w, what="denormal")
    return rows
