"""The region test of BAM streams (condition 5 of csrc/vgmi_bam_filter.h) as a Python model, and the records its tests are made of.

The model is the plain definition, no shortcuts: every interval is looked at, the whole CIGAR is summed, in Python's unbounded
integers.  It works on the bytes of a record, never on the code under test.  `verdict_raw` is the whole rule: conditions 1 to 4 of
bam_filter_cases, the region test, then the tag walk of bam_filter_cases.  The oracle of every device test is the model's: the stream
with regions must equal the plain stream of a BAM that holds only the passing records."""
import copy
import struct

import numpy as np

import bam_filter_cases as F
import bam_py as B

READ, DROP, FAULT = F.READ, F.DROP, F.FAULT
WHOLE = 1 << 31
REF_CONSUMING = (0, 2, 3, 7, 8)      # M D N = X
OPS = "MIDNSHP=X"
MUTATIONS = ("closed", "noD", "I", "unmapped_cigar", "sum32")
# the references of every file these cases are written to; the last one has the highest refID
REFS = ((b"chr1", 1 << 28), (b"chr2", WHOLE - 1), (b"HLA-A*01:01:01:01", 3000), (b"chrLast", 1 << 20))
LAST = len(REFS) - 1


# ---- packing ---------------------------------------------------------------------------------------------------------------------------
def record(r):
    """B.record with CIGAR operations given as letters or as codes 0 to 15 (the undefined 9 to 15 among them)"""
    q = copy.copy(r)
    q.cigar = [(n, op if isinstance(op, str) else "P") for n, op in r.cigar]
    raw = bytearray(B.record(q))
    at = 36 + len(r.name) + 1
    for i, (n, op) in enumerate(r.cigar):
        if not isinstance(op, str):
            raw[at + 4 * i:at + 4 * i + 4] = struct.pack("<I", n << 4 | op)
    return bytes(raw)


def raw_bam(recs, refs=REFS):
    """(decompressed stream, header length, offset of every record)"""
    h = B.header(refs=refs)
    parts, offs, pos = [h], [], len(h)
    for r in recs:
        b = record(r)
        offs.append(pos)
        parts.append(b)
        pos += len(b)
    return b"".join(parts), len(h), offs


def write_bam(path, recs, refs=REFS):
    raw, hlen, offs = raw_bam(recs, refs)
    B.bgzf(path, raw)
    return hlen, offs


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def normalise(regions):
    """sorted by (ref, beg), overlapping or touching intervals of one reference merged"""
    out = []
    for ref, beg, end in sorted(regions):
        if out and out[-1][0] == ref and beg <= out[-1][2]:
            out[-1][2] = max(out[-1][2], end)
        else:
            out.append([ref, beg, end])
    return [tuple(x) for x in out]


def placement(raw, o=0):
    """(refID, pos, flag, [(op_len, code)]) of the record at raw[o:]"""
    ref, pos = struct.unpack_from("<ii", raw, o + 4)
    l_rn = raw[o + 12]
    n_cig, flag = struct.unpack_from("<HH", raw, o + 16)
    cig = struct.unpack_from("<%dI" % n_cig, raw, o + 36 + l_rn)
    return ref, pos, flag, [(c >> 4, c & 15) for c in cig]


def endpos(pos, flag, cigar, mutate=None):
    consuming = set(REF_CONSUMING)
    if mutate == "noD":
        consuming.discard(2)
    if mutate == "I":
        consuming.add(1)
    reflen = sum(n for n, code in cigar if code in consuming)
    if mutate == "sum32":
        reflen &= 0xFFFFFFFF
    unmapped = flag & 4 and mutate != "unmapped_cigar"
    return pos + 1 if unmapped or not cigar or reflen == 0 else pos + reflen


def overlaps(raw, regions, unplaced, o=0, mutate=None):
    """condition 5 alone on the record at raw[o:]; regions: any list of (ref, beg, end), normalised or not"""
    ref, pos, flag, cigar = placement(raw, o)
    if ref < 0:
        return bool(unplaced)
    e = endpos(pos, flag, cigar, mutate)
    if mutate == "closed":
        return any(r == ref and pos <= end and e >= beg for r, beg, end in regions)
    return any(r == ref and pos < end and e > beg for r, beg, end in regions)


def verdict_raw(raw, f, regions, unplaced=False, o=0, mutate=None):
    """READ | DROP | FAULT of the whole rule: 1 to 4, the regions (an empty list: no region test), the tag bound"""
    v = F.verdict_raw(raw, F.Filter(f.exclude, f.require, f.min_mapq), o)[0]
    if v != READ:
        return v
    if regions and not overlaps(raw, regions, unplaced, o, mutate):
        return DROP
    return F.verdict_raw(raw, f, o)[0]


def plain(rec):
    """the record as the default rule keeps it: what the oracle's BAM (written by write_bam here, with the same references) holds for a
    passing record"""
    return F.plain(rec)


def apply(recs, f, regions, unplaced=False):
    """-> (the passing records made plain, records examined, reads, index of the first faulted record or None)"""
    out, n = [], 0
    for i, r in enumerate(recs):
        v = verdict_raw(record(r), f, regions, unplaced)
        if v == FAULT:
            return out, n, len(out), i
        n += 1
        if v == READ:
            out.append(plain(r))
    return out, n, len(out), None


# ---- the case set ---------------------------------------------------------------------------------------------------------------------------
# deliberately not normalised: unsorted, two overlapping and two touching intervals.  Normalised: chr1 [100, 200) [300, 400)
# [1000, 1100); chr2 [2^31 - 10, 2^31); chrLast whole
CASE_REGIONS = [(0, 1000, 1100), (LAST, 0, WHOLE), (0, 300, 350), (0, 100, 160), (0, 150, 200), (1, WHOLE - 10, WHOLE), (0, 350, 400)]
BIG = (1 << 28) - 1


def cases(haps=None, seed=21):
    """[(class, Rec)]: every class of the region rule's edges, against CASE_REGIONS"""
    d = F.Draw(seed, haps)
    out = []

    def add(cls, pos, cigar=(), ref=0, flag=0, **kw):
        out.append((cls, d.rec(30, flag=flag, ref=ref, pos=pos, cigar=cigar, **kw)))

    add("pos_end_minus_1", 199, [(1, "M")])
    add("pos_end", 200, [(1, "M")])
    add("endpos_beg", 90, [(10, "M")])
    add("endpos_beg_plus_1", 90, [(11, "M")])
    add("inside", 150, [(10, "M")])
    add("inside", 1050, [(30, "M")])
    add("gap", 220, [(50, "M")])
    add("gap", 200, [(100, "M")])                      # fills the gap exactly: touches both neighbours, overlaps neither
    add("span_gap", 199, [(102, "M")])                 # the last base of one interval to the first of the next
    add("swallow", 50, [(500, "M")])
    add("swallow", 950, [(10, "S"), (400, "M")])
    add("reflen_0", 95, [(20, "S"), (10, "I")])        # endpos = pos + 1 = 96
    add("reflen_0", 99, [(5, "I")])                    # endpos 100 == beg
    add("reflen_0", 100, [(30, "S")])                  # pos inside
    add("no_cigar", 150)
    add("no_cigar", 99)
    add("unmapped_with_cigar", 90, [(50, "M")], flag=4)       # the CIGAR is ignored: endpos 91
    add("unmapped_with_cigar", 150, [(50, "M")], flag=4)
    add("D_reaches", 90, [(5, "M"), (10, "D")])
    add("D_reaches", 90, [(5, "M"), (5, "D")])         # endpos 100: not yet
    add("N_reaches", 90, [(5, "M"), (20, "N"), (5, "M")])
    add("N_reaches", 290, [(11, "N")])
    add("N_reaches", 290, [(10, "N")])                 # endpos 300 == beg
    for op in "ISHP":
        add("ISHP_do_not_reach", 90, [(5, "M"), (100, op), (5, "M")])      # endpos 100
    add("ISHP_do_not_reach", 90, [(5, "M"), (100, "I"), (6, "M")])         # ... and one more M reaches
    add("eq_X", 90, [(6, "="), (6, "X")])
    add("eq_X", 90, [(5, "="), (5, "X")])
    add("code_9", 90, [(5, "M"), (100, 9), (5, "M")])
    add("code_15", 90, [(5, "M"), (100, 15), (5, "M")])
    add("code_15", 90, [(5, "M"), (100, 15), (6, "M")])
    add("placeholder", 50, [(30, "S"), (60, "N")])     # <l_seq>S<reflen>N, the real CIGAR in a CG tag
    add("placeholder", 50, [(30, "S"), (50, "N")])
    add("unplaced", -1, ref=-1, flag=4)
    add("unplaced", -1, ref=-1, flag=4 | 0x1 | 0x8 | 0x40)
    add("pos_minus_1", -1, ref=LAST, flag=4)           # endpos 0: in front of [0, 2^31)
    add("pos_minus_1", -1, ref=0, flag=4)
    add("highest_ref", 5000, [(30, "M")], ref=LAST)
    add("highest_ref", 0, ref=LAST)
    add("sum_wraps_32", 10, [(BIG, "M")] * 17, ref=1)  # 17 * (2^28 - 1) = 2^32 + 2^28 - 17: a 32-bit sum ends far in front
    add("sum_wraps_32", 10, [(BIG, "N")] * 16 + [(30, "M")], ref=1)
    add("sum_wraps_32", 10, [(BIG, "M")] * 7, ref=1)   # 10 + 7 * (2^28 - 1) < 2^31 - 10: does not reach
    add("pos_max", WHOLE - 1, [(1, "M")], ref=1)
    add("pos_max", WHOLE - 1, [(30, "M")], ref=0)
    add("other_ref", 150, [(30, "M")], ref=2)          # a reference without an interval, between two that have some
    # with the other conditions: dropped by 1 to 4 inside a region; kept by them outside
    add("with_flags", 150, [(30, "M")], flag=0x400)
    add("with_flags", 150, [(30, "M")], flag=0x100)
    add("with_flags", 220, [(30, "M")], flag=0x400)
    add("with_mapq", 150, [(30, "M")], mapq=3, aux=F.aux(b"qs", "C", 30))
    add("with_mapq", 150, [(30, "M")], mapq=60, aux=F.aux(b"qs", "C", 30))
    add("with_tag", 150, [(30, "M")], aux=F.aux(b"qs", "C", 30))
    add("with_tag", 150, [(30, "M")], aux=F.aux(b"qs", "C", 3))
    add("with_tag", 220, [(30, "M")], aux=F.aux(b"qs", "C", 30))
    # auxiliary fields that cannot be walked: outside the regions nothing walks them
    add("unwalkable_outside", 220, [(30, "M")], aux=F.aux(b"NM", "C", 1) + F.fault("type"))
    add("unwalkable_outside", -1, ref=-1, flag=4, aux=F.fault("nonul"))
    return out


CLASSES_BOTH_VERDICTS = ("reflen_0", "no_cigar", "unmapped_with_cigar", "D_reaches", "N_reaches", "ISHP_do_not_reach", "eq_X",
                         "code_15", "placeholder", "sum_wraps_32", "pos_max")
CASE_FILTER = F.Filter(exclude=0xF00, min_mapq=20, tag=b"qs", min_value=10)      # for the with_* classes


# ---- interval lists and drawn records ---------------------------------------------------------------------------------------------------------
LIST_SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 1025)


def interval_list(n, several=False, seed=3):
    """n disjoint, non-touching intervals (already merged: n is what the binary search sees), on chr1 alone or dealt over all four
    references, in drawn order"""
    rng = np.random.default_rng(seed + n)
    out = []
    for i in range(n):
        ref = i % len(REFS) if several else 0
        slot = i // len(REFS) if several else i
        beg = 50 + 100 * slot + int(rng.integers(0, 20))
        out.append((ref, beg, beg + int(rng.integers(1, 60))))
    return [out[i] for i in rng.permutation(n)]


def drawn(n=2000, span=None, seed=31, haps=None, unplaced_share=0.05, n_refs=len(REFS)):
    """records with drawn references, positions inside [-1, span) and CIGARs of every operation, a few of them unmapped, unplaced,
    without CIGAR, with flags the default rule drops"""
    d = F.Draw(seed, haps)
    rng = d.rng
    out = []
    for i in range(n):
        u = rng.random()
        if u < unplaced_share:
            out.append(d.rec(flag=4, ref=-1, pos=-1))
            continue
        ref = int(rng.integers(0, n_refs))
        pos = int(rng.integers(-1, span if span else 2600))
        k = int(rng.integers(0, 6))
        cigar = [(int(rng.integers(1, 40)), OPS[int(rng.integers(0, 9))] if rng.random() < 0.95 else int(rng.integers(9, 16))) for _ in range(k)]
        flag = (4 if rng.random() < 0.08 else 0) | (0x100 if rng.random() < 0.05 else 0) | (0x400 if rng.random() < 0.1 else 0)
        out.append(d.rec(0 if i % 101 == 7 else None, flag=flag, ref=ref, pos=pos, cigar=cigar, mapq=int(rng.integers(0, 61)),
                         aux=F.aux(b"qs", "C", int(rng.integers(0, 41)))))
    return out
