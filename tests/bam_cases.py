"""Hand-built BAM streams for the device's record kernels (csrc/vgmi_bam.hip), as data: tests/test_bam_cases_cpu.py proves with the
Python model and the host decoder that every case is what it claims, tests/test_gpu_bam_cases.py puts it through the device.

A case is a decompressed stream (tests/bam_py.py), cut into chunks at chosen bytes: every chunk is written as stored block-gzip
members of its own and committed in one call (`piece`), so a device chunk ends exactly where the case wants it.  What the device
must yield comes from the model (bam_py.reads_block over the records in front of the one it stops at), never from the code under
test.

A *fake* is a complete record -- a kept read, flag 0, with a sequence of its own -- planted where arbitrary bytes are legal: a B:C
aux array or the quality bytes of a true record.  Its first byte passes every check of the candidate test, so only the walk from
the chunk's first byte tells it from a record: a chain that enters one changes n_records, n_bases and the counters."""
import struct
import zlib

import numpy as np

import bam_py as B

TAIL_MAX = 1 << 20                    # the carry between chunks (vgmi_fastq_open): a record of block_size <= TAIL_MAX - 4 is the device's
REFS2 = ((b"chr1", 100000), (b"chr2", 5000))
REFS3 = REFS2 + ((b"chrM", 16569),)
TEXT = b"@HD\tVN:1.6\tSO:unsorted\n@PG\tID:cases\tPN:bam_cases\n"
CHAIN_LENS = (1, 2, 3, 4, 5, 255, 256, 257, 1025)
SWEEP = range(-44, 9)                 # first byte of the swept record minus the chunk's end
ERRORS = {"past": "block_size runs past the end of the data", "short": "fixed fields longer than block_size",
          "ref_hi": "refID out of range", "ref_lo": "refID out of range", "next_hi": "next_refID out of range",
          "next_lo": "next_refID out of range", "name0": "l_read_name is 0", "fields": "fields longer than block_size",
          "nul": "read name not NUL-terminated"}
CAP_CHUNK_KB = 64                     # the capacity case: VGMI_FASTQ_CHUNK_KB, the knob test_gpu_bam.py uses for small chunks
CAP_CAND = ((CAP_CHUNK_KB << 10) + TAIL_MAX) // 6 // 4      # cap_cand of such a stream (vgmi_fastq_open, vgmi_fastq_commit_bgzf)
CAP_PERIOD = bytes.fromhex("00000100" "0000000000000000" "01000000")


def SEQ_LENS(k):
    """the decode loop's edges: a lane pass is 128 bases; k - 1 is the longest read without a k-mer"""
    return (1, 2, 3, k - 1, k, k + 1, 127, 128, 129, 255, 256, 257)


def _u32(v):
    return struct.pack("<I", v & 0xFFFFFFFF)


def _ld32(raw, o):
    return int.from_bytes(raw[o:o + 4], "little")


def _s32(raw, o):
    return int.from_bytes(raw[o:o + 4], "little", signed=True)


# ---- the validity rule of vgmi_bam.hip's header comment, restated ------------------------------------------------------------------
def is_record(raw, o, end, n_ref, tail_max=TAIL_MAX):
    """a whole, valid record no longer than the carry starts at byte o of raw[:end]"""
    if end - o < 4:
        return False
    bs = _ld32(raw, o)
    if bs > tail_max - 4 or o + 4 + bs > end:          # block_size inside the data and within the carry
        return False
    if bs < 32:
        return False
    l_rn, n_cig, l_seq = raw[o + 12], raw[o + 16] | raw[o + 17] << 8, _ld32(raw, o + 20)
    if 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
        return False
    if l_rn < 1 or raw[o + 36 + l_rn - 1] != 0:         # a name, ending in NUL
        return False
    return -1 <= _s32(raw, o + 4) < n_ref and -1 <= _s32(raw, o + 24) < n_ref


def candidates(raw, lo, end, n_ref, tail_max=TAIL_MAX):
    """every o in [lo, end) at which is_record holds, in order (numpy only sieves by block_size; the rule is is_record)"""
    if end - lo < 36:
        return []
    a = np.zeros(end - lo + 4, dtype=np.int64)
    a[:end - lo] = np.frombuffer(raw, dtype=np.uint8, count=end - lo, offset=lo)
    n = end - lo
    bs = a[0:n] | a[1:n + 1] << 8 | a[2:n + 2] << 16 | a[3:n + 3] << 24
    o = np.arange(lo, end, dtype=np.int64)
    sieve = o[(bs >= 32) & (bs <= tail_max - 4) & (o + 4 + bs <= end)]
    return [int(x) for x in sieve if is_record(raw, int(x), end, n_ref, tail_max)]


def walk(raw, o, end, n_ref, tail_max=TAIL_MAX):
    """the chain of length prefixes from o while records are valid -> (read block, records kept, first byte not taken)"""
    out, n = [], 0
    while o < end and is_record(raw, o, end, n_ref, tail_max):
        bs, l_rn, n_cig, l_seq = _ld32(raw, o), raw[o + 12], raw[o + 16] | raw[o + 17] << 8, _ld32(raw, o + 20)
        flag = raw[o + 18] | raw[o + 19] << 8
        if not flag & 0x900 and l_seq:
            s = o + 36 + l_rn + 4 * n_cig
            out.append(bytes(B.NT16[raw[s + (i >> 1)] >> (0 if i & 1 else 4) & 15] for i in range(l_seq)) + b"\n")
            n += 1
        o += 4 + bs
    return b"".join(out), n, o


# ---- building blocks ---------------------------------------------------------------------------------------------------------------
class _Gen:
    """random, distinct sequences and ordinary records, the same for a case's name every time"""

    def __init__(self, name):
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.i = 0

    def seq(self, n, alphabet=b"ACGT"):
        al = np.frombuffer(alphabet, dtype=np.uint8)
        return bytes(al[self.rng.integers(0, len(al), size=n)])

    def rec(self, n_ref=2, lo=30, hi=120):
        self.i += 1
        s, name = self.seq(int(self.rng.integers(lo, hi))), b"t%d" % self.i
        kind = self.i % 5 if n_ref else 0
        if kind == 1:
            return B.Rec(name, s, flag=0, ref=0, pos=7, mapq=60, cigar=[(len(s), "M")])
        if kind == 2:
            return B.Rec(name, s, flag=16, ref=n_ref - 1, pos=9, mapq=60, cigar=[(len(s), "M")], next_ref=0)
        if kind == 3:
            return B.Rec(name, s, flag=0x100 if self.i % 2 else 0x800 | 16, ref=0, pos=3, cigar=[(len(s), "M")])    # not a read
        return B.Rec(name, s, flag=4 | (0x400 if kind == 4 else 0))

    def recs(self, n, n_ref=2):
        return [self.rec(n_ref) for _ in range(n)]

    def fake(self, l_seq=30, **kw):
        """-> (the fake as a record of the model, its bytes)"""
        self.i += 1
        r = B.Rec(b"f%d" % self.i, self.seq(l_seq), flag=0, **kw)
        return r, B.record(r)

    def carrier(self, blob, where="aux", flag=0, l_seq=40, **kw):
        """a true record that carries blob in a B:C aux array, or in front of its quality bytes"""
        self.i += 1
        name = b"c%d" % self.i
        if where == "qual":
            s = self.seq(len(blob) + 20)
            return B.Rec(name, s, flag=flag, qual=blob + bytes([30]) * 20, **kw)
        return B.Rec(name, self.seq(l_seq), flag=flag, aux=b"XFBC" + _u32(len(blob)) + blob, **kw)


class Case:
    """raw: the decompressed stream; cuts: the bytes at which a chunk ends (the last chunk ends with the stream); stop: the index of
    the record the device does not take (None: it takes all); tail: that record is carried to the end of the data instead of stopping
    the device; error: the host decoder's reason at that record; fakes: [(bytes of a planted fake, it is a candidate)]"""

    def __init__(self, name, family, recs, refs=REFS2, cuts=(), stop=None, tail=False, error=None, fakes=(), patch=None, inside=None,
                 n_cand=None, extra_reads=(), env=None, text=TEXT):
        self.name, self.family, self.recs, self.n_ref, self.stop, self.error_what = name, family, recs, len(refs), stop, error
        self.env = env or {}
        # the record stopped at is no candidate (malformed, or longer than the carry) unless the stop is about the chunk (capacity)
        self.not_cand = {stop} if stop is not None and not self.env else set()
        raw, self.hlen, self.offs = B.raw_bam(recs, text, refs)
        if patch:
            raw = patch(bytearray(raw), self.offs)
        self.raw = bytes(raw)
        self.cuts = sorted(set(c for c in cuts if 0 < c < len(self.raw)))
        self.fakes = []                                   # (offset, candidate, record of the model)
        for r, b, cand in fakes:
            assert self.raw.count(b) == 1, name
            self.fakes.append((self.raw.find(b), cand, r))
        self.inside = inside or {}                        # {index of a true record: false candidates strictly inside it}
        self.n_cand = n_cand                              # candidates of the (only) chunk, where the case is about their number
        took = recs if stop is None else recs[:stop]
        self.block, self.n_records, self.n_bases = B.reads_block(took)
        self.consumed = len(self.raw) if stop is None else self.offs[stop]
        self.stopped = stop is not None and not tail
        self.tail = self.raw[self.offs[stop]:] if tail else b""
        # every sequence in the file, true or planted: the key table of the GPU test
        self.reads = [r.seq for r in recs if r.seq] + [r.seq for _, _, r in self.fakes] + list(extra_reads)
        self._comp = None

    def error(self, path):
        return f"'{path}': not a valid BAM record at decompressed byte {self.offs[self.stop]} ({self.error_what})" if self.error_what else None

    def chunks(self):
        b = [0] + self.cuts + [len(self.raw)]
        return list(zip(b[:-1], b[1:]))

    def _build(self):
        if self._comp is None:
            sizes, per_commit = [], []
            for a, e in self.chunks():
                m = [B.STORED_MAX] * ((e - a) // B.STORED_MAX) + ([(e - a) % B.STORED_MAX] if (e - a) % B.STORED_MAX else [])
                sizes += m
                per_commit.append(len(m))
            comp, csz = B.bgzf_stored(self.raw, sizes)
            piece, i = [], 0
            for n in per_commit:
                piece.append(sum(csz[i:i + n]))
                i += n
            piece[-1] += csz[-1]                          # the EOF block goes with the last commit
            assert sum(piece) == len(comp) and i == len(sizes)
            self._comp, self.sizes, self._piece = comp, sizes, piece
        return self

    @property
    def comp(self):
        return self._build()._comp

    @property
    def piece(self):
        """compressed bytes per call of Context.bam_bgzf: exactly the members of one chunk each"""
        return self._build()._piece


_BUILDERS = {}       # name -> (family, builder)
_CASES = {}


def _case(family, name=None):
    def deco(fn, name=name):
        name = name or fn.__name__.lstrip("_")
        _BUILDERS[name] = (family, lambda: fn(name, family))
        return fn
    return deco


def names(family=None):
    return [n for n, (f, _) in _BUILDERS.items() if family is None or f == family]


def get(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name][1]()
    return _CASES[name]


def families():
    return sorted({f for f, _ in _BUILDERS.values()})


def _gap(n=3):
    return bytes(n)      # zeros: a block_size of 0 is never a candidate


# ---- planted false candidates ------------------------------------------------------------------------------------------------------
def _planted(name, family, n_fakes, where="aux", last_ends_record=False, adjacent=False, n_after=40, carrier_kw=None, cuts=None):
    g = _Gen(name)
    fk = [g.fake(30 + 2 * i) for i in range(n_fakes)]      # longer than k: a fake entered also changes the counters
    blob = _gap(5)
    for i, (_, b) in enumerate(fk):
        blob += b + (b"" if (adjacent and i + 1 < n_fakes) or (last_ends_record and i + 1 == n_fakes) else _gap())
    assert where == "aux" or not last_ends_record
    c = g.carrier(blob, where, **(carrier_kw or {}))
    recs = g.recs(6) + [c] + g.recs(n_after)
    k = Case(name, family, recs, fakes=[(r, b, True) for r, b in fk], inside={6: n_fakes})
    if cuts:
        k = Case(name, family, recs, fakes=[(r, b, True) for r, b in fk], inside={6: n_fakes}, cuts=cuts(k))
    return k


@_case("planted")
def _one_fake(name, family):
    return _planted(name, family, 1)


@_case("planted")
def _one_fake_in_qualities(name, family):
    return _planted(name, family, 1, where="qual")


@_case("planted")
def _binary_search_6_fakes(name, family):
    return _planted(name, family, 6)


@_case("planted")
def _binary_search_9_fakes_few_behind(name, family):
    return _planted(name, family, 9, n_after=2)


@_case("planted")
def _binary_search_5_fakes_last_record(name, family):
    return _planted(name, family, 5, n_after=0)


@_case("planted")
def _probe_edge_3_fakes(name, family):
    return _planted(name, family, 3)


@_case("planted")
def _probe_edge_4_fakes(name, family):
    return _planted(name, family, 4)


@_case("planted")
def _fake_runs_into_a_true_boundary(name, family):
    return _planted(name, family, 2, last_ends_record=True)


@_case("planted")
def _fake_runs_into_a_fake(name, family):
    return _planted(name, family, 3, adjacent=True)


@_case("planted")
def _fake_past_the_data(name, family):
    g = _Gen(name)
    r, b = g.fake()
    r2, b2 = g.fake()
    b = _u32(5000) + b[4:]                               # claims 5000 bytes; fewer follow
    recs = g.recs(8) + [g.carrier(_gap() + b + _gap() + b2 + _gap())]
    return Case(name, family, recs, fakes=[(r, b, False), (r2, b2, True)], inside={8: 1})


@_case("planted")
def _fakes_in_a_chunks_last_record(name, family):
    return _planted(name, family, 6, cuts=lambda k: [k.offs[7]])


@_case("planted")
def _fakes_in_the_carried_tail(name, family):
    return _planted(name, family, 6, cuts=lambda k: [k.offs[7] - 2])      # every fake whole in the first chunk, the record not


@_case("planted")
def _fakes_in_a_secondary(name, family):
    return _planted(name, family, 5, carrier_kw={"flag": 0x100})


@_case("planted")
def _fakes_in_a_supplementary(name, family):
    return _planted(name, family, 2, carrier_kw={"flag": 0x800 | 16})


@_case("planted")
def _fakes_in_a_record_without_sequence(name, family):
    return _planted(name, family, 5, carrier_kw={"l_seq": 0})


# ---- every alignment of a record against a chunk end ----------------------------------------------------------------------------------
def _sweep(name, family, d, fakes):
    g = _Gen(name)
    recs, fk, inside = g.recs(5), [], {}
    if fakes:      # a fake that runs into the swept record, one in front of it, and two inside the record behind the boundary
        fk = [g.fake() for _ in range(4)]
        recs.append(g.carrier(_gap() + fk[0][1] + _gap() + fk[1][1]))
        inside = {5: 2, 6: 2}
    else:
        recs.append(g.rec())
    blob = _gap() + fk[2][1] + _gap() + fk[3][1] + _gap() if fakes else b""
    aux = b"XFBC" + _u32(len(blob)) + blob if fakes else b""
    recs.append(B.Rec(b"r12", g.seq(51), flag=0, ref=1, pos=77, mapq=60, next_ref=0, aux=aux))      # l_read_name 4: SEQ starts at byte 40
    recs += g.recs(4)
    k = Case(name, family, recs)
    return Case(name, family, recs, cuts=[k.offs[6] - d], fakes=[(r, b, True) for r, b in fk], inside=inside)


for _d in SWEEP:
    for _f in (False, True):
        _case("sweep", "sweep_%s%d%s" % ("m" if _d < 0 else "p", abs(_d), "_fakes" if _f else ""))(
            lambda name, family, d=_d, f=_f: _sweep(name, family, d, f))


def _header(name, family, cuts):
    g = _Gen(name)
    recs = g.recs(6)
    k = Case(name, family, recs)
    return Case(name, family, recs, cuts=cuts(k.hlen))


_case("sweep", "header_ends_with_a_chunk")(lambda n, f: _header(n, f, lambda h: [h]))
_case("sweep", "header_ends_a_byte_short_of_a_chunk")(lambda n, f: _header(n, f, lambda h: [h + 1]))
_case("sweep", "chunk_ends_a_byte_short_of_the_header")(lambda n, f: _header(n, f, lambda h: [h - 1]))
_case("sweep", "header_spans_three_chunks")(lambda n, f: _header(n, f, lambda h: [9, h - 7]))


# ---- sequence lengths ------------------------------------------------------------------------------------------------------------------
def _seqlen(name, family, k):
    g = _Gen(name)
    recs = []
    for flag in (0, 16):
        for n in SEQ_LENS(k):
            recs.append(B.Rec(b"l%d" % n, g.seq(n), flag=flag, ref=0, pos=1, cigar=[(n, "M")]))
        both = g.seq(k) + B.NT16 + b"A" + B.NT16 + g.seq(k)                 # every code in the high and in the low nibble
        recs.append(B.Rec(b"codes", both, flag=flag))
        recs.append(B.Rec(b"pad", g.seq(2 * k + 1), flag=flag, pad=15))     # an odd l_seq whose unused nibble says 'N'
        recs.append(B.Rec(b"", g.seq(k + 2), flag=flag))                    # l_read_name 1: the NUL alone
        recs.append(B.Rec(b"n" * 254, g.seq(k + 3), flag=flag))             # l_read_name 255
        recs.append(B.Rec(b"cig", g.seq(k + 4), flag=flag, ref=1, pos=5, cigar=[(1, "M")] * 65535))
        recs.append(B.Rec(b"aux", g.seq(k + 5), flag=flag, aux=b"RGZgrp1\0" + b"npi\x05\0\0\0"))
        recs.append(B.Rec(b"n-run", g.seq(k) + b"N" + g.seq(k - 1) + b"NN" + g.seq(k), flag=flag))
    assert both[k:k + 16] == B.NT16 and both[k + 17:k + 33] == B.NT16      # 17 apart: opposite nibbles
    k_ = Case(name, family, recs)
    return Case(name, family, recs, cuts=[k_.offs[i] + 38 for i in range(3, len(recs), 4)])


for _k in (27, 11, 22):
    _case("seqlen", "seqlen_k%d" % _k)(lambda n, f, k=_k: _seqlen(n, f, k))


# ---- the carry limit ---------------------------------------------------------------------------------------------------------------------
def _carry(name, family, block_size, split):
    g = _Gen(name)
    fixed = 32 + 4 + (2000 + 1) // 2 + 2000 + 8          # name "big\0", 2000 bases, the aux array's own eight bytes
    big = B.Rec(b"big", g.seq(2000), flag=0, aux=b"XZBC" + _u32(block_size - fixed) + bytes(block_size - fixed))
    recs = g.recs(5) + [big] + g.recs(5)
    took = block_size <= TAIL_MAX - 4
    k = Case(name, family, recs)
    assert _ld32(k.raw, k.offs[5]) == block_size
    return Case(name, family, recs, cuts=[k.offs[5] + 500_000] if split else [], stop=None if took else 5)


for _n, _bs in (("carry_limit_taken", TAIL_MAX - 4), ("carry_limit_refused", TAIL_MAX - 3)):
    for _s in (False, True):
        _case("carry", _n + ("_split" if _s else "_whole"))(lambda n, f, bs=_bs, s=_s: _carry(n, f, bs, s))


# ---- chain lengths -------------------------------------------------------------------------------------------------------------------
def _chain(name, family, n, kept=True, cuts_after=()):
    g = _Gen(name)
    recs = [B.Rec(b"", g.seq(1 + i % 3), flag=0 if kept else (0x100, 0x800, 0x900)[i % 3]) for i in range(n)]
    k = Case(name, family, recs)
    return Case(name, family, recs, n_cand=None if cuts_after else n, cuts=[k.offs[i] for i in cuts_after])


for _n in CHAIN_LENS:
    _case("chain", "chain_%d" % _n)(lambda n, f, c=_n: _chain(n, f, c))
for _n in (1, 4, 257):
    _case("chain", "chain_%d_none_kept" % _n)(lambda n, f, c=_n: _chain(n, f, c, kept=False))
_case("chain", "chain_30000")(lambda n, f: _chain(n, f, 30000))
_case("chain", "chain_chunks_of_1_2_3_4_5")(lambda n, f: _chain(n, f, 15, cuts_after=(1, 3, 6, 10)))
_case("chain", "header_and_no_record")(lambda n, f: Case(n, f, [], n_cand=0))
_case("chain", "only_a_record_without_sequence")(lambda n, f: Case(n, f, [B.Rec(b"s", b"", flag=4)], n_cand=1))


# ---- n_ref ---------------------------------------------------------------------------------------------------------------------------
@_case("nref")
def _unaligned_no_reference(name, family):
    g = _Gen(name)
    r0, b0 = g.fake(ref=0)                               # refID 0 of no reference: not a candidate
    r1, b1 = g.fake(next_ref=0)
    r2, b2 = g.fake()
    recs = g.recs(6, n_ref=0) + [g.carrier(_gap() + b0 + _gap() + b1 + _gap() + b2 + _gap())] + g.recs(6, n_ref=0)
    return Case(name, family, recs, refs=(), fakes=[(r0, b0, False), (r1, b1, False), (r2, b2, True)], inside={6: 1})


@_case("nref")
def _three_references_edges(name, family):
    g = _Gen(name)
    recs = []
    for ref in (-1, 2):
        for nxt in (-1, 2):
            s = g.seq(60)
            recs.append(B.Rec(b"e", s, flag=0, ref=ref, pos=4, next_ref=nxt))
    r3, b3 = g.fake(ref=3)                               # refID n_ref: not a candidate
    r2, b2 = g.fake(ref=2, next_ref=2)
    recs.append(g.carrier(_gap() + b3 + _gap() + b2 + _gap()))
    recs += g.recs(3, n_ref=3)
    return Case(name, family, recs, refs=REFS3, fakes=[(r3, b3, False), (r2, b2, True)], inside={4: 1})


# ---- malformed records -----------------------------------------------------------------------------------------------------------------
def _damage(raw, at, what, n_ref):
    bs, l_rn = _ld32(raw, at), raw[at + 12]
    if what == "past":
        raw[at:at + 4] = _u32(len(raw) - at - 4 + 100)
    elif what == "short":
        raw[at:at + 4] = _u32(31)
    elif what in ("ref_hi", "ref_lo"):
        raw[at + 4:at + 8] = _u32(n_ref if what == "ref_hi" else -2)
    elif what in ("next_hi", "next_lo"):
        raw[at + 24:at + 28] = _u32(n_ref if what == "next_hi" else -2)
    elif what == "name0":
        raw[at + 12] = 0
    elif what == "fields":
        raw[at + 20:at + 24] = _u32(bs)                   # l_seq = block_size
    elif what == "nul":
        raw[at + 36 + l_rn - 1] = ord("x")
    return raw


def _malformed(name, family, what, place, with_fake):
    g = _Gen(name)
    r, b = g.fake()
    at = 0 if place == "first" else 4
    bad = g.carrier(_gap() + (b if with_fake else bytes(len(b))) + _gap(), ref=0, pos=3, next_ref=1)
    recs = g.recs(at) + [bad] + g.recs(4)
    patch = lambda raw, offs: _damage(raw, offs[at], what, 2)
    k = Case(name, family, recs, patch=patch)
    # the fake stays a candidate whatever the damage, and so do the records behind: the chain must end in front of them all the same
    return Case(name, family, recs, patch=patch, stop=at, tail=what == "past", error=ERRORS[what],
                cuts=[k.offs[at] + 20] if place == "later" else [], fakes=[(r, b, True)] if with_fake else [])


for _w in ERRORS:
    for _p in ("first", "middle", "later"):
        for _f in (False, True):
            _case("malformed", "malformed_%s_%s%s" % (_w, _p, "_fake" if _f else ""))(
                lambda n, f, w=_w, p=_p, k=_f: _malformed(n, f, w, p, k))


# ---- capacity ------------------------------------------------------------------------------------------------------------------------
@_case("capacity")
def _more_candidates_than_the_arrays_hold(name, family):
    """A record of the largest size the device takes whose aux array repeats CAP_PERIOD: one candidate per 16 bytes (block_size 65536,
    refID 0, l_read_name 1, l_seq 0 -- no read) wherever 64 KiB + 4 of data follow.  With chunks of CAP_CHUNK_KB the carried front of the
    record grows chunk by chunk until its candidates exceed CAP_CAND: the device takes nothing of that chunk and stops at the record."""
    g = _Gen(name)
    fixed = 32 + 4 + 50 + 100 + 8
    n = TAIL_MAX - 4 - fixed
    blob = (CAP_PERIOD * (n // 16 + 1))[:n]
    recs = g.recs(5) + [B.Rec(b"cap", g.seq(100), flag=0, aux=b"XPBC" + _u32(n) + blob)] + g.recs(5)
    return Case(name, family, recs, stop=5, env={"VGMI_FASTQ_CHUNK_KB": str(CAP_CHUNK_KB)})
