"""The model of the minimum base quality (genotype --min-base-quality, vgmi_fastq_set_min_quality) and the read files its tests use
(test_quality_mask_cpu.py, test_gpu_quality_mask.py).  No device involved.

The rule: with Q > 0, base i of a FASTQ record is masked -- counted as N -- when quality byte i, as an unsigned byte, is < 33 + Q; base i
of a BAM record when QUAL[i] < Q, except that a record whose QUAL[0] is 0xff stores no qualities and is not masked; base and quality pair
in record order.  Everything else stays.  So counting file F with Q equals counting F' with the option off, where F' is F with exactly
those bases written as N: the builders below give F, F' and the number of masked bases for every Q.

A record is (name, seq, qual[, shape]): qual holds the FASTQ bytes (Phred+33); shape is how the text writes it -- "plain" four lines,
"crlf" four lines ending in \\r\\n, "wrapped" sequence and quality over two lines each (quality lines are joined before pairing)."""
import numpy as np

import bam_py as B

QS = (1, 2, 20, 41, 93)
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 151, 20000)
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def mask(seq, qual, q, offset=33):
    """the sequence with N where the quality byte is < offset + q, and how many: the rule (q == 0: off)"""
    if q == 0:
        return bytes(seq), 0
    assert len(seq) == len(qual)
    s = np.frombuffer(bytes(seq), dtype=np.uint8).copy()
    low = np.frombuffer(bytes(qual), dtype=np.uint8) < offset + q
    s[low] = ord("N")
    return s.tobytes(), int(low.sum())


def mask_bam(seq, qual, q):
    """the same for a BAM record (raw Phred bytes; QUAL[0] == 0xff: no qualities stored, nothing masked)"""
    if len(qual) and qual[0] == 0xFF:
        return bytes(seq), 0
    return mask(seq, qual, q, offset=0)


def windows(seq, k):
    """k-mer windows of seq that hold no N: what a read contributes at all"""
    return sum(1 for i in range(len(seq) - k + 1) if b"N" not in seq[i:i + k])


class _Draw:
    def __init__(self, haps, seed):
        self.rng = np.random.default_rng(seed)
        self.haps = haps

    def seq(self, n):
        if self.haps is None:
            return _ACGT[self.rng.integers(0, 4, size=n)].tobytes()
        h = self.haps[int(self.rng.integers(0, len(self.haps)))]
        s0 = int(self.rng.integers(0, len(h) - n))
        return h[s0:s0 + n].tobytes().upper()


def fastq_records(k, q, haps=None, seed=7, bulk=400):
    """The case set for bound q (>= 1) at k-mer length k: record lengths around the wavefront's 64 lanes and one of 20 000; the values
    33 + q - 1, 33 + q, 33 + q + 1 side by side; '!' and '~'; quality lines that start with '@', '+', '>'; a record masked whole and one
    not at all; k - 1 and k good bases between two masked ones; then `bulk` reads of 151 with qualities drawn in 2..41, a few percent
    below 20 (varied qualities also keep the text from compressing past what the device's gzip decoder takes)."""
    d = _Draw(haps, seed * 1000 + q)
    rng = d.rng
    at = 33 + q
    lo, hi = at - 1, min(at + 1, 126)

    def good(n):
        return rng.integers(at, min(at + 30, 126) + 1, size=n, dtype=np.uint8)

    def low(n):
        return rng.integers(33, lo + 1, size=n, dtype=np.uint8)

    recs = []
    for n in LENGTHS:
        ql = good(n)
        pick = rng.random(n) < 0.1
        ql[pick] = low(int(pick.sum()))
        ql[n - 1] = lo                      # the byte-granular tail of the wavefront's last round
        if n > 2:
            ql[0] = lo
        recs.append((b"len%d" % n, d.seq(n), ql.tobytes()))
    ql = good(151)
    for p in (10, 62, 63, 64, 126, 127, 128):
        ql[p - 1:p + 2] = (lo, at, hi)
    recs.append((b"edge", d.seq(151), ql.tobytes()))
    ql = good(151)
    ql[5::7] = ord("!")
    ql[3::11] = ord("~")
    recs.append((b"bang_tilde", d.seq(151), ql.tobytes()))
    for c in b"@+>":
        ql = good(100)
        ql[0] = c
        ql[50] = lo
        recs.append((b"starts_%d" % c, d.seq(100), ql.tobytes()))
    recs.append((b"all_masked", d.seq(151), low(151).tobytes()))
    recs.append((b"none_masked", d.seq(151), good(151).tobytes()))
    for name, n_good in ((b"k_minus_1", k - 1), (b"k_exact", k)):
        ql = good(n_good + 2)
        ql[0] = ql[-1] = lo
        recs.append((name, d.seq(n_good + 2), ql.tobytes()))
    for i in range(bulk):
        ql = rng.integers(20, 42, size=151, dtype=np.uint8)
        pick = rng.random(151) < 0.04
        ql[pick] = rng.integers(2, 20, size=int(pick.sum()), dtype=np.uint8)
        recs.append((b"bulk%d" % i, d.seq(151), (ql + 33).astype(np.uint8).tobytes()))
    return recs


def masked_records(recs, q):
    """(the records of F', masked bases)"""
    out, total = [], 0
    for r in recs:
        s, n = mask(r[1], r[2], q)
        out.append((r[0], s, r[2]) + tuple(r[3:]))
        total += n
    return out, total


def fastq_text(recs, final_newline=True):
    parts = []
    for r in recs:
        name, seq, qual = r[:3]
        shape = r[3] if len(r) > 3 else "plain"
        if shape == "crlf":
            parts.append(b"@" + name + b"\r\n" + seq + b"\r\n+\r\n" + qual + b"\r\n")
        elif shape == "wrapped":
            h = len(seq) // 2
            parts.append(b"@" + name + b"\n" + seq[:h] + b"\n" + seq[h:] + b"\n+\n" + qual[:h + 3] + b"\n" + qual[h + 3:] + b"\n")
        else:
            parts.append(b"@" + name + b" x\n" + seq + b"\n+\n" + qual + b"\n")
    text = b"".join(parts)
    return text if final_newline else text[:-1]


def line_offsets(recs, i):
    """where record i's sequence line, '+' line and quality line start in fastq_text(recs) (plain records in front of it)"""
    at = len(fastq_text(recs[:i]))
    seq_at = at + len(recs[i][0]) + 4
    plus_at = seq_at + len(recs[i][1]) + 1
    return seq_at, plus_at, plus_at + 2


def fastq_cuts(recs, i):
    """commit sizes that end a chunk behind record i's sequence line, in front of its quality line, and inside it"""
    seq_at, plus_at, qual_at = line_offsets(recs, i)
    return {"behind_sequence_line": plus_at, "quality_line_begins_the_next": qual_at, "inside_quality_line": qual_at + len(recs[i][2]) // 2}


def bam_records(k, q, haps=None, seed=7, bulk=150):
    """The FASTQ case set as BAM records (odd and even l_seq, 1 included), and what only BAM has: a record without qualities
    (QUAL[0] == 0xff, low values behind it) between masked ones, a reverse-strand record, and records the read filter drops
    (secondary, supplementary, SEQ '*') that carry low qualities and must not count."""
    recs = []
    for j, (name, seq, qual) in enumerate(fastq_records(k, q, haps, seed, bulk)):
        ph = bytes(c - 33 for c in qual)
        recs.append(B.Rec(name, seq, flag=4, qual=ph))
        if name == b"edge":
            n = 77
            d = _Draw(haps, seed + 99)
            recs.append(B.Rec(b"no_qual", d.seq(n), flag=4, qual=b"\xff" + bytes(n - 1)))
            recs.append(B.Rec(b"reverse", B.revcomp(d.seq(n)), flag=16, ref=-1, qual=bytes([0] * 5 + [q] * (n - 10) + [max(q - 1, 0)] * 5)))
            recs.append(B.Rec(b"secondary", d.seq(n), flag=256, qual=bytes(n)))
            recs.append(B.Rec(b"supplementary", d.seq(n), flag=2048, qual=bytes(n)))
            recs.append(B.Rec(b"star", b"", flag=4))
    return recs


def masked_bam_records(recs, q):
    out, total = [], 0
    for r in recs:
        s, n = mask_bam(r.seq, r.qual, q) if r.seq else (b"", 0)
        out.append(B.Rec(r.name, s, flag=r.flag, ref=r.ref, qual=r.qual))
        total += n if r.kept else 0
    return out, total


def bam_cuts(recs, i, text=b"@HD\tVN:1.6\tSO:unsorted\n"):
    """decompressed offsets that end a block-gzip member between record i's SEQ and QUAL, and inside its QUAL"""
    _, _, offs = B.raw_bam(recs, text=text)
    r = recs[i]
    seq_at = offs[i] + 36 + len(r.name) + 1 + 4 * len(r.cigar)
    qual_at = seq_at + (len(r.seq) + 1) // 2
    return {"between_seq_and_qual": qual_at, "inside_qual": qual_at + len(r.seq) // 2}


def draw_qualities(text, seed, lo=2, hi=41, frac_low=0.04, below=20):
    """a four-line FASTQ text with its quality lines drawn afresh: values lo..hi, frac_low of them below `below` (the sequences stay)"""
    rng = np.random.default_rng(seed)
    lines = text.split(b"\n")
    for i in range(3, len(lines), 4):
        n = len(lines[i])
        ql = rng.integers(below, hi + 1, size=n, dtype=np.uint8)
        pick = rng.random(n) < frac_low
        ql[pick] = rng.integers(lo, below, size=int(pick.sum()), dtype=np.uint8)
        lines[i] = (ql + 33).astype(np.uint8).tobytes()
    return b"\n".join(lines)


def masked_text(text, q):
    """(F', masked bases) of a four-line FASTQ text F"""
    lines = text.split(b"\n")
    total = 0
    for i in range(1, len(lines) - 2, 4):
        lines[i], n = mask(lines[i], lines[i + 2], q)
        total += n
    return b"\n".join(lines), total


def records_of(text):
    """the records of a four-line FASTQ text as (header line without '@', seq, qual)"""
    lines = text.split(b"\n")
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]
