"""A pure-Python BAM writer (SAM spec 4.2) for the tests, and the FASTQ twin of its records: what `samtools fastq` writes from the
same BAM -- one four-line record per record with flag & 0x900 == 0 and a sequence, in file order, reverse-strand reads (0x10)
reverse-complemented back.  The block-gzip layer is synth.bgzf_compress_file: members of a fixed size, so records straddle them;
bgzf_stored writes stored members of chosen sizes, whose compressed sizes are then known."""
import os
import struct
import zlib

from varigraph_amd import synth

NT16 = b"=ACMGRSVTWYHKDBN"
_COMP = bytes.maketrans(b"=ACMGRSVTWYHKDBN", b"=TGKCYSBAWRDMHVN")


class Rec:
    def __init__(self, name, seq, flag=4, ref=-1, pos=-1, mapq=255, cigar=(), next_ref=-1, next_pos=-1, tlen=0, qual=None, aux=b"", pad=0):
        self.name, self.seq, self.flag, self.pad = name, bytes(seq), flag, pad      # pad: the unused low nibble behind an odd l_seq
        self.ref, self.pos, self.mapq, self.cigar = ref, pos, mapq, list(cigar)
        self.next_ref, self.next_pos, self.tlen = next_ref, next_pos, tlen
        self.qual = qual if qual is not None else bytes((30 + i % 10) for i in range(len(self.seq)))
        self.aux = aux

    @property
    def kept(self):
        return not (self.flag & 0x900) and len(self.seq) > 0


def header(text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=()):
    """magic .. the last reference; refs: [(name, length)]"""
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, ln in refs:
        nm = name + b"\0"
        out += [struct.pack("<i", len(nm)), nm, struct.pack("<i", ln)]
    return b"".join(out)


def record(r):
    nm = r.name + b"\0"
    seq = bytearray((len(r.seq) + 1) // 2)
    for i, c in enumerate(r.seq):
        seq[i >> 1] |= NT16.index(c) << (0 if i & 1 else 4)
    if len(r.seq) & 1:
        seq[-1] |= r.pad & 15
    cig = b"".join(struct.pack("<I", n << 4 | "MIDNSHP=X".index(op)) for n, op in r.cigar)
    body = struct.pack("<iiBBHHHiiii", r.ref, r.pos, len(nm), r.mapq, 4680, len(r.cigar), r.flag, len(r.seq), r.next_ref, r.next_pos, r.tlen)
    body += nm + cig + bytes(seq) + (r.qual if r.seq else b"") + r.aux
    return struct.pack("<i", len(body)) + body


def raw_bam(records, text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=()):
    """(decompressed stream, header length, offset of every record in it)"""
    h = header(text, refs)
    parts, offs, pos = [h], [], len(h)
    for r in records:
        b = record(r)
        offs.append(pos)
        parts.append(b)
        pos += len(b)
    return b"".join(parts), len(h), offs


def bgzf(path, raw, level=4, block=0xff00, eof=True):
    """raw (a decompressed BAM stream, well-formed or not) block-gzipped to path"""
    src = str(path) + ".raw"
    with open(src, "wb") as f:
        f.write(raw)
    synth.bgzf_compress_file(src, str(path), level=level, block=block)
    os.unlink(src)
    if not eof:
        data = open(path, "rb").read()
        assert data.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
        open(path, "wb").write(data[:-28])
    return str(path)


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
STORED_MAX = 65536 - 18 - 5 - 8      # text of a stored member: BSIZE counts the header, the stored block's five bytes and the trailer


def bgzf_stored(raw, sizes, eof=True):
    """raw as stored (level 0) block-gzip members of `sizes` decompressed bytes each (what they leave goes into members of STORED_MAX)
    -> (the file's bytes, the compressed size of every member; the EOF block is the last if eof)"""
    sizes = list(sizes)
    assert all(0 < n <= STORED_MAX for n in sizes) and sum(sizes) <= len(raw)
    left = len(raw) - sum(sizes)
    sizes += [STORED_MAX] * (left // STORED_MAX) + ([left % STORED_MAX] if left % STORED_MAX else [])
    out, comp, pos = [], [], 0
    for n in sizes:
        d = raw[pos:pos + n]
        pos += n
        total = 18 + 5 + n + 8
        out.append(bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", total - 1) + b"\1" + struct.pack("<HH", n, n ^ 0xFFFF) + d +
                   struct.pack("<II", zlib.crc32(d), n))
        comp.append(total)
    if eof:
        out.append(BGZF_EOF)
        comp.append(len(BGZF_EOF))
    return b"".join(out), comp


def write_bam(path, records, text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=(), level=4, block=0xff00, eof=True):
    raw, hlen, offs = raw_bam(records, text, refs)
    bgzf(path, raw, level, block, eof)
    return hlen, offs


def reads_block(records):
    """what the BAM decoders must yield: (the '\\n'-joined read block, n_reads, read_base)"""
    kept = [r.seq for r in records if r.kept]
    return b"".join(s + b"\n" for s in kept), len(kept), sum(map(len, kept))


def revcomp(seq):
    return bytes(seq).translate(_COMP)[::-1]


def twin_fastq(path, records):
    with open(path, "wb") as f:
        for r in records:
            if not r.kept:
                continue
            seq, qual = (revcomp(r.seq), r.qual[::-1]) if r.flag & 0x10 else (r.seq, r.qual)
            f.write(b"@" + r.name + b"\n" + seq + b"\n+\n" + bytes(min(q, 93) + 33 for q in qual) + b"\n")
    return str(path)
