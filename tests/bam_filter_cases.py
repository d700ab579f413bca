"""The read filter of BAM streams (csrc/vgmi_bam_filter.h) as a Python model, and the records its tests are made of.

The model works on the bytes of a record as tests/bam_py.py writes them, never on the code under test: `verdict` restates the rule
(l_seq, exclude, require, MAPQ, the first field with the tag), `walk` the auxiliary walk with its fault classes.  `aux` packs a
field of any type.  The oracle of every device test is the model's: the filtered stream must equal the unfiltered stream of a BAM
that holds only the passing records (`plain` turns those into records the default filter keeps)."""
import copy
import math
import struct

import numpy as np

import bam_py as B

READ, DROP, FAULT = 1, 0, -1
INT_TYPES = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
ELEM = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
NUMERIC = "cCsSiIfd"
FAULTS = ("short1", "short2", "type", "subtype", "overrun", "bcount", "bhead", "nonul")


class Filter:
    def __init__(self, exclude=0x900, require=0, min_mapq=0, tag=None, min_value=0.0):
        self.exclude, self.require, self.min_mapq, self.tag, self.min_value = exclude, require, min_mapq, tag, min_value

    @property
    def on(self):
        return (self.exclude, self.require, self.min_mapq, self.tag) != (0x900, 0, 0, None)

    def dict(self):
        return dict(exclude=self.exclude, require=self.require, min_mapq=self.min_mapq, tag=self.tag, min_value=self.min_value)

    def __repr__(self):
        return "F(x%X r%X q%d %s>=%r)" % (self.exclude, self.require, self.min_mapq, self.tag and self.tag.decode(), self.min_value)


# ---- packing ---------------------------------------------------------------------------------------------------------------------------
def aux(tag, typ, value=None, sub=None):
    """one auxiliary field: A (a byte), the integers, f, d, Z / H (bytes without the NUL), B (sub = the subtype, value = the elements)"""
    head = tag + typ.encode()
    if typ == "A":
        return head + (value if isinstance(value, bytes) else bytes([value]))[:1]
    if typ in INT_TYPES:
        return head + struct.pack(INT_TYPES[typ], value)
    if typ == "f":
        return head + (value if isinstance(value, bytes) else struct.pack("<f", value))
    if typ == "d":
        return head + struct.pack("<d", value)
    if typ in "ZH":
        return head + bytes(value) + b"\0"
    assert typ == "B"
    if sub == "C" and isinstance(value, bytes):      # (a long byte array at once)
        return head + b"C" + struct.pack("<I", len(value)) + value
    fmt = "<f" if sub == "f" else INT_TYPES[sub]
    return head + sub.encode() + struct.pack("<I", len(value)) + b"".join(struct.pack(fmt, v) for v in value)


def f32(x):
    """x rounded to a float, as the double the rule compares"""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def f32_below(x):
    """the float just below f32(x) (x > 0)"""
    bits = struct.unpack("<I", struct.pack("<f", x))[0]
    return struct.unpack("<f", struct.pack("<I", bits - 1))[0]


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def walk(a, tag, last=False):
    """the auxiliary bytes `a` of one record -> (READ, value) | (DROP, None) | (FAULT, None).  last: a MUTATED walk, in which the last
    field with the tag decides (it has to pass over every field)"""
    p, end, found = 0, len(a), None
    while p != end:
        if end - p < 3:
            return FAULT, None
        hit, typ = a[p:p + 2] == tag, chr(a[p + 2])
        p += 3
        left = end - p
        if typ in FIXED:
            n = FIXED[typ]
        elif typ in "ZH":
            z = a.find(b"\0", p)
            if z < 0:
                return FAULT, None
            n = z - p + 1
        elif typ == "B":
            if left < 5 or chr(a[p]) not in ELEM:
                return FAULT, None
            n = 5 + int.from_bytes(a[p + 1:p + 5], "little") * ELEM[chr(a[p])]
        else:
            return FAULT, None
        if n > left:
            return FAULT, None
        if hit:
            if typ in INT_TYPES:
                r = (READ, float(struct.unpack(INT_TYPES[typ], a[p:p + n])[0]))
            elif typ == "f":
                r = (READ, struct.unpack("<f", a[p:p + 4])[0])
            elif typ == "d":
                r = (READ, struct.unpack("<d", a[p:p + 8])[0])
            else:
                r = (DROP, None)
            if not last:
                return r
            found = r
        p += n
    return found or (DROP, None)


def fields(raw, o=0):
    """(block_size, l_read_name, mapq, n_cigar_op, flag, l_seq, the auxiliary bytes) of the record at raw[o:]"""
    bs = int.from_bytes(raw[o:o + 4], "little")
    l_rn, mapq = raw[o + 12], raw[o + 13]
    n_cig, flag = raw[o + 16] | raw[o + 17] << 8, raw[o + 18] | raw[o + 19] << 8
    l_seq = int.from_bytes(raw[o + 20:o + 24], "little")
    a = o + 36 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    return bs, l_rn, mapq, n_cig, flag, l_seq, bytes(raw[a:o + 4 + bs])


def verdict_raw(raw, f, o=0, mutate=None):
    """(READ | DROP | FAULT, the tag's value where the walk found a numeric one) of the record at raw[o:].  mutate: a wrong rule --
    "any" (require tested as any bit), "gt" (MAPQ compared with >), "last" (the last field with the tag decides)"""
    _, _, mapq, _, flag, l_seq, a = fields(raw, o)
    req = (flag & f.require) != 0 or not f.require if mutate == "any" else (flag & f.require) == f.require
    mq = mapq > f.min_mapq or not f.min_mapq if mutate == "gt" else mapq >= f.min_mapq
    if l_seq == 0 or flag & f.exclude or not req or not mq:
        return DROP, None
    if f.tag is None:
        return READ, None
    r, v = walk(a, f.tag, last=mutate == "last")
    if r != READ:
        return r, None
    return (READ if v >= f.min_value else DROP), v      # (a NaN compares false)


def verdict(rec, f, mutate=None):
    return verdict_raw(B.record(rec), f, 0, mutate)


def plain(rec):
    """the record as one the default filter keeps: what the oracle's BAM holds for a record that passed a configured filter"""
    r = copy.copy(rec)
    r.flag = rec.flag & ~0x900
    return r


def apply(recs, f):
    """-> (the passing records made plain, records examined, reads, index of the first faulted record or None): the records in front
    of the first walk fault are examined, none at or behind it"""
    out, n = [], 0
    for i, r in enumerate(recs):
        v, _ = verdict(r, f)
        if v == FAULT:
            return out, n, len(out), i
        n += 1
        if v == READ:
            out.append(plain(r))
    return out, n, len(out), None


# ---- walk faults ---------------------------------------------------------------------------------------------------------------------------
def fault(kind):
    """auxiliary bytes that cannot be walked; each is a record's LAST bytes (the record ends where they end)"""
    return {
        "short1": b"X",                                                # one byte left in front of the record's end
        "short2": b"XY",                                               # two
        "type": b"XYq\x01\x02",                                        # an unknown type
        "subtype": b"XYBd" + struct.pack("<I", 1) + bytes(8),          # a B array of doubles: no such subtype
        "overrun": b"XYi\x01\x02",                                     # a 4-byte value, 2 bytes left
        "bcount": b"XYBI" + struct.pack("<I", 0x7FFFFFFF) + bytes(12),  # 2^33 - 4 bytes claimed: 32-bit arithmetic would see -4
        "bhead": b"XYBc\x01\x00",                                      # the data ends inside the count
        "nonul": b"XYZno end",                                         # a string without NUL inside the record
    }[kind]


# ---- records ---------------------------------------------------------------------------------------------------------------------------
class Draw:
    def __init__(self, seed, haps=None):
        self.rng = np.random.default_rng(seed)
        self.haps = haps
        self.i = 0

    def seq(self, n):
        if self.haps is None:
            return np.frombuffer(b"ACGT", dtype=np.uint8)[self.rng.integers(0, 4, size=n)].tobytes()
        h = self.haps[int(self.rng.integers(0, len(self.haps)))]
        s0 = int(self.rng.integers(0, len(h) - n))
        return h[s0:s0 + n].tobytes().upper()

    def qual(self, n):
        """raw Phred bytes in 20..41, a few percent in 2..19"""
        ql = self.rng.integers(20, 42, size=n, dtype=np.uint8)
        pick = self.rng.random(n) < 0.04
        ql[pick] = self.rng.integers(2, 20, size=int(pick.sum()), dtype=np.uint8)
        return ql.tobytes()

    def rec(self, n=None, flag=0, mapq=60, aux=b"", **kw):
        self.i += 1
        n = int(self.rng.integers(140, 161)) if n is None else n
        return B.Rec(b"q%d" % self.i, self.seq(n), flag=flag, mapq=mapq, qual=self.qual(n), aux=aux, **kw)


FLAG_BITS = (0x001, 0x004, 0x010, 0x100, 0x200, 0x400, 0x800)
MAPQS = (0, 1, 19, 20, 21, 59, 60, 254, 255)


def flag_records(n=2000, seed=5, haps=None):
    """records of about 150 bases with drawn flags (every bit of FLAG_BITS set in some and clear in some), MAPQ over MAPQS, SEQ '*'
    among them"""
    d = Draw(seed, haps)
    out = []
    for i in range(n):
        flag = 0
        for b in FLAG_BITS:
            if d.rng.random() < (0.5 if b in (0x001, 0x004, 0x010) else 0.15):
                flag |= b
        mapq = MAPQS[int(d.rng.integers(0, len(MAPQS)))]
        out.append(d.rec(0 if i % 97 == 13 else None, flag=flag, mapq=mapq, aux=b"NMC\x02" if i % 3 else b""))
    return out


FLAG_FILTERS = {
    "exclude_F00": Filter(exclude=0xF00),
    "exclude_400_alone": Filter(exclude=0x400),
    "require_1_exclude_904": Filter(exclude=0x904, require=0x1),
    "mapq_1": Filter(min_mapq=1),
    "mapq_20": Filter(min_mapq=20),
    "mapq_255": Filter(min_mapq=255),
    "all_together": Filter(exclude=0xF04, require=0x1, min_mapq=20),
}

# (type, value) of the wanted tag around the bound 10: below, equal, above in every numeric type
TAG_VALUES = [(t, v) for t in "cCsSiI" for v in (9, 10, 11)] + [("f", 9.5), ("f", 10.0), ("f", 10.5), ("d", 9.999), ("d", 10.0), ("d", 1e300),
                                                                ("c", -128), ("i", -2 ** 31), ("I", 2 ** 32 - 1), ("f", float("nan")),
                                                                ("f", float("inf")), ("f", float("-inf"))]
FRONTS = {
    "none": b"",
    "every_fixed_type": b"".join(aux(b"X" + t.encode(), t, 65 if t == "A" else 1) for t in "AcCsSiIfd"),
    "strings": aux(b"RG", "Z", b"group1") + aux(b"XH", "H", b"1AE301") + aux(b"XE", "Z", b""),
    "arrays": b"".join(aux(b"Y" + s.encode(), "B", [1, 2, 3], s) for s in "cCsSiIf") + aux(b"Y0", "B", [], "i"),
    "b_4k": aux(b"XB", "B", [7] * 4096, "C"),
    "z_300": aux(b"XZ", "Z", b"s" * 300),
}


def tag_records(tag=b"qs", seed=6, haps=None):
    """records carrying `tag` in every numeric type around the bound 10, each behind every FRONTS entry; the tag absent; non-numeric
    (A Z H B); present twice (the first decides); fields behind the tag that could not be walked (not seen)"""
    d = Draw(seed, haps)
    out = []
    for name, front in FRONTS.items():
        for t, v in TAG_VALUES:
            out.append(d.rec(aux=front + aux(tag, t, v) + aux(b"ZZ", "i", 5)))
        out.append(d.rec(aux=front))                                                   # absent
        out.append(d.rec(aux=front + aux(tag, "A", b"9")))
        out.append(d.rec(aux=front + aux(tag, "Z", b"11")))
        out.append(d.rec(aux=front + aux(tag, "H", b"0B")))
        out.append(d.rec(aux=front + aux(tag, "B", [11, 12], "C")))
        out.append(d.rec(aux=front + aux(tag, "C", 11) + aux(tag, "C", 9)))            # twice: the first decides
        out.append(d.rec(aux=front + aux(tag, "C", 9) + aux(tag, "C", 11)))
        out.append(d.rec(aux=front + aux(tag, "C", 11) + fault("type")))               # a fault behind the tag is not seen
        out.append(d.rec(aux=front + aux(tag, "s", 9) + fault("nonul")))
    out.append(d.rec(flag=0x100, aux=fault("type")))                                   # a record that fails 1 to 4 is not walked
    out.append(d.rec(0, aux=fault("short1")))
    return out


def rq_records(n=60, seed=8, haps=None):
    """PacBio-like: rq as f, 0.99f, the float just below, and values drawn around it"""
    d = Draw(seed, haps)
    vals = [f32(0.99), f32_below(0.99), 1.0, 0.0, 0.5] + [float(v) for v in d.rng.uniform(0.97, 1.0, size=n - 5)]
    return [d.rec(flag=4, mapq=255, aux=aux(b"zm", "i", i) + aux(b"rq", "f", v) + aux(b"np", "i", 7)) for i, v in enumerate(vals)]


def faulted(kind, where, seed=9, haps=None, n=24):
    """(records, index of the faulted one): a record whose auxiliary bytes end in fault(kind), first of the stream or in the middle
    with passing records on both sides; the wanted tag is qs and lies BEHIND the fault, so the walk meets the fault first"""
    d = Draw(seed, haps)
    at = 0 if where == "first" else n // 2
    recs = [d.rec(aux=aux(b"qs", "C", 30 if i % 4 else 5)) for i in range(n)]
    recs[at] = d.rec(aux=aux(b"NM", "C", 1) + fault(kind))
    return recs, at
