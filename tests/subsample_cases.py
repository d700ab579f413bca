"""The model of subsampling (genotype --subsample F --subsample-seed S, vgmi_fastq_set_subsample) and the read files its tests use
(test_subsample_cpu.py, test_gpu_subsample.py).  No device involved.

The rule: a file's reads are numbered i = 0, 1, 2, ... in file order -- FASTQ and FASTA: the records; BAM: the records that pass the read
filter (flag & 0x900 == 0 and l_seq > 0; the others have no number) -- and read i is kept iff z(i, S) < T, all arithmetic mod 2^64:

    T = int(F * 2**64)
    x = (i + 1) * 0x9E3779B97F4A7C15 + S
    x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9
    x ^= x >> 27;  x *= 0x94D049BB133111EB
    x ^= x >> 31;  z = x

A dropped read is not a read.  So counting file G with (F, S) equals counting G' with the option off, where G' is G with exactly the
dropped reads removed: the builders below give G and G'.

A FASTQ record is (name, seq, qual[, shape]) as in quality_mask_cases.py, whose fastq_text writes it."""
import numpy as np

import bam_py as B
import quality_mask_cases as Q

M64 = (1 << 64) - 1
FRACTIONS = (0.5, 0.02, 0.9)
SEEDS = (11, 7)                      # the option's default and another: what the GPU tests use

# Known answers (the issue's tables): z(i, S) for i down and S across, the thresholds, and the reads kept among the first 4 000 at S = 11
KNOWN_S = (11, 0, M64)
KNOWN_Z = {
    0: (0x50f5647d2380309d, 0xe220a8397b1dcdaf, 0xe4d971771b652c20),
    1: (0x432a5cd27a6b13a1, 0x6e789e6aa1b965f4, 0xe99ff867dbf682c9),
    2: (0xa356be306e9b126d, 0x06c45d188009454f, 0x382ff84cb27281e9),
    1 << 32: (0x6f1848d17c7a49ca, 0x46093cf9861ec2e4, 0xc5aa1d1d7e827744),
    M64 - 1: (0x64edd2139b64e0d6, 0x336503c6b835bec0, 0xde0a564cbcd060c4),
}
KNOWN_T = {0.5: 0x8000000000000000, 0.02: 0x051eb851eb851ec0, 0.9: 0xe666666666666800}
KNOWN_4000 = {0.5: (2017, (0, 1, 4, 6, 8, 10), 15), 0.02: (70, (41, 69, 123), 274), 0.9: (3611, (), 3)}   # kept, first kept, longest dropped run


def z(i, seed):
    x = ((i + 1) * 0x9E3779B97F4A7C15 + seed) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def threshold(f):
    return int(f * 2 ** 64)


def keep(i, seed, f):
    """read i is kept (f == 1: the option is off, everything is)"""
    return f >= 1.0 or z(i, seed) < threshold(f)


def kept_mask(n, f, seed, first=0):
    """bool per read first .. first + n - 1: numpy's uint64 arithmetic wraps as the rule's does"""
    if f >= 1.0:
        return np.ones(n, dtype=bool)
    with np.errstate(over="ignore"):
        x = (np.arange(first, first + n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x < np.uint64(threshold(f))


def longest_dropped_run(mask):
    best = run = 0
    for k in mask:
        run = 0 if k else run + 1
        best = max(best, run)
    return best


def kept_of(items, f, seed, first=0):
    """the items whose number (first + position) the rule keeps"""
    m = kept_mask(len(items), f, seed, first)
    return [x for x, k in zip(items, m) if k]


# ---- read files ------------------------------------------------------------------------------------------------------------------------
class _Draw:
    def __init__(self, haps, seed):
        self.rng = np.random.default_rng(seed)
        self.haps = haps

    def seq(self, n):
        if self.haps is None:
            return np.frombuffer(b"ACGT", dtype=np.uint8)[self.rng.integers(0, 4, size=n)].tobytes()
        h = self.haps[int(self.rng.integers(0, len(self.haps)))]
        s0 = int(self.rng.integers(0, len(h) - n))
        return h[s0:s0 + n].tobytes().upper()

    def qual(self, n):
        """Phred+33 bytes in 20..41, a few percent in 2..19: --min-base-quality 20 masks some bases of most reads"""
        ql = self.rng.integers(20, 42, size=n, dtype=np.uint8)
        pick = self.rng.random(n) < 0.04
        ql[pick] = self.rng.integers(2, 20, size=int(pick.sum()), dtype=np.uint8)
        return (ql + 33).astype(np.uint8).tobytes()


LONG = 20000                         # a record carried across chunks of 4 KiB


def long_positions(seed, n):
    """where the two 20 000-base records go: the first number >= n // 4 that F = 0.5 keeps under `seed`, the first >= n // 2 it drops"""
    m = kept_mask(n, 0.5, seed)
    return (next(i for i in range(n // 4, n) if m[i]), next(i for i in range(n // 2, n) if not m[i]))


def fastq_records(haps=None, n=600, seed=3, long_at=()):
    """n reads of 151 bases (lengths 1 .. 150 among the first 40, so that records of every residue of the wavefront's 64 lanes are
    dropped and kept), the records at long_at of 20 000 bases"""
    d = _Draw(haps, 7000 + seed)
    recs = []
    for i in range(n):
        ln = LONG if i in long_at else (1 + (i * 37) % 150 if i < 40 else 151)
        recs.append((b"r%d" % i, d.seq(ln), d.qual(ln)))
    return recs


def fastq_text(recs, final_newline=True):
    return Q.fastq_text(recs, final_newline)


def fasta_text(recs, width=None):
    """single-line records, or wrapped at `width` bases"""
    out = []
    for name, seq, *_ in recs:
        out.append(b">" + name + b" x\n")
        w = width or max(len(seq), 1)
        out += [seq[a:a + w] + b"\n" for a in range(0, len(seq), w)]
    return b"".join(out)


def end_of_record(recs, i):
    """bytes of fastq_text(recs) up to and including record i: a commit of this size ends a chunk right behind it"""
    return len(fastq_text(recs[:i + 1]))


def bam_records(haps=None, n=300, seed=3):
    """n reads with secondary, supplementary and SEQ '*' records in between (one after every second read, in turn), so that a read's
    number is not its record's: the non-reads have no number"""
    d = _Draw(haps, 9000 + seed)
    recs, turn = [], 0
    for i in range(n):
        ln = 1 + (i * 37) % 150 if i < 40 else 101 + i % 50
        recs.append(B.Rec(b"r%d" % i, d.seq(ln), flag=4 if i % 3 else 16, qual=bytes(c - 33 for c in d.qual(ln))))
        if i % 2:
            kind = turn % 3
            turn += 1
            if kind == 0:
                recs.append(B.Rec(b"sec%d" % i, d.seq(77), flag=0x100, qual=bytes(77)))
            elif kind == 1:
                recs.append(B.Rec(b"sup%d" % i, d.seq(77), flag=0x800, qual=bytes(77)))
            else:
                recs.append(B.Rec(b"star%d" % i, b"", flag=4))
    return recs


def bam_filtered(recs, f, seed, first=0):
    """(G': the records without the dropped reads -- the non-reads stay where they are --, the file's reads)"""
    out, i = [], first
    for r in recs:
        if not r.kept:
            out.append(r)
            continue
        if keep(i, seed, f):
            out.append(r)
        i += 1
    return out, i - first


def filtered_fastq_text(text, f, seed):
    """(G', kept, seen) of a four-line FASTQ text G"""
    lines = text.split(b"\n")
    n = (len(lines) - 1) // 4
    m = kept_mask(n, f, seed)
    out = [b"\n".join(lines[4 * i:4 * i + 4]) + b"\n" for i in range(n) if m[i]]
    return b"".join(out), int(m.sum()), n
