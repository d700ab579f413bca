"""The host BAM decoder (vgh_bam_read_all, csrc/host/bam_reader.cpp) against the Python model of tests/bam_py.py: the reads of a
BAM / unaligned BAM file are the records with flag & 0x900 == 0 and a sequence, their 4-bit SEQ decoded as stored, and every
malformed record ends the run naming its decompressed byte."""
import numpy as np
import pytest

import bam_py as B
from varigraph_amd import host


def _seqs(n, seed, lo=1, hi=300, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    al = np.frombuffer(alphabet, dtype=np.uint8)
    return [bytes(al[rng.integers(0, len(al), size=int(rng.integers(lo, hi)))]) for _ in range(n)]


def _check(path, records):
    block, n, rb = host.bam_read_all(path, decode_threads=3)
    want, n_want, rb_want = B.reads_block(records)
    assert block.tobytes() == want
    assert (n, rb) == (n_want, rb_want)


def _ubam(n=3000, seed=1):
    aux = b"RGZgrp1\0" + b"npi\x05\0\0\0"
    return [B.Rec(b"m64011/%d/ccs" % i, s, flag=4 | (0x200 if i % 97 == 0 else 0) | (0x400 if i % 89 == 0 else 0), aux=aux)
            for i, s in enumerate(_seqs(n, seed, 50, 400, b"ACGTN"))]


def _aligned(n=2000, seed=2):
    rng = np.random.default_rng(seed)
    out = []
    for i, s in enumerate(_seqs(n, seed, 1, 251, B.NT16)):
        flag = int(rng.choice([0, 16, 256, 2048, 16 | 2048, 1024, 512, 1 | 64, 1 | 128 | 16, 4]))
        if i % 50 == 7:
            s = b""                                   # SEQ '*'
        ref = -1 if flag & 4 else int(rng.integers(0, 3))
        out.append(B.Rec(b"r%d" % i, s, flag=flag, ref=ref, pos=int(rng.integers(0, 10000)), mapq=60, cigar=[(len(s), "M")] if s else [],
                         next_ref=int(rng.integers(-1, 3)), qual=bytes(int(q) for q in rng.integers(0, 60, size=len(s)))))
    return out


_REFS = [(b"chr1", 1000000), (b"chr2", 500000), (b"chrM", 16569)]


def test_unaligned_bam(tmp_path):
    recs = _ubam()
    p = tmp_path / "u.bam"
    B.write_bam(p, recs)
    _check(str(p), recs)


def test_aligned_bam_with_secondary_supplementary_empty_and_iupac(tmp_path):
    recs = _aligned()
    assert any(r.flag & 0x900 for r in recs) and any(not r.seq for r in recs) and any(len(r.seq) % 2 for r in recs)
    p = tmp_path / "a.bam"
    B.write_bam(p, recs, refs=_REFS)
    _check(str(p), recs)


def test_large_header_and_many_references(tmp_path):
    text = b"".join(b"@CO\tcomment line %06d padding to make the header text large\n" % i for i in range(1100))[: 64 << 10]
    refs = [(b"contig_%05d" % i, 1000 + i) for i in range(3000)]
    recs = [B.Rec(b"x%d" % i, s, flag=0, ref=i % 3000, pos=5, cigar=[(len(s), "M")]) for i, s in enumerate(_seqs(500, 3, 20, 200))]
    p = tmp_path / "h.bam"
    hlen, _ = B.write_bam(p, recs, text=text, refs=refs)
    assert hlen > (64 << 10) + 3000 * 20
    _check(str(p), recs)


def test_a_record_of_3_mib(tmp_path):
    recs = _ubam(40, 4)
    big = _seqs(1, 5, 3 << 20, (3 << 20) + 1)[0]
    recs.insert(20, B.Rec(b"big", big, flag=4))
    p = tmp_path / "big.bam"
    B.write_bam(p, recs)
    _check(str(p), recs)


@pytest.mark.parametrize("level,eof", [(0, True), (0, False), (6, False)])
def test_stored_members_and_a_missing_eof_block(level, eof, tmp_path):
    recs = _aligned(800, 6)
    p = tmp_path / "s.bam"
    B.write_bam(p, recs, refs=_REFS, level=level, eof=eof)
    _check(str(p), recs)


def _corrupt(raw, off, what):
    raw = bytearray(raw)
    l_rn = raw[off + 12]
    if what == "block_size runs past the end of the data":
        raw = raw[: off + 40]
    elif what == "l_read_name is 0":
        raw[off + 12] = 0
    elif what == "read name not NUL-terminated":
        raw[off + 36 + l_rn - 1] = ord("x")
    elif what == "fields longer than block_size":
        bs = int.from_bytes(raw[off:off + 4], "little")
        raw[off + 20:off + 24] = bs.to_bytes(4, "little")     # l_seq = block_size
    elif what == "refID out of range":
        raw[off + 4:off + 8] = (3).to_bytes(4, "little", signed=True)
    elif what == "next_refID out of range":
        raw[off + 24:off + 28] = (-2).to_bytes(4, "little", signed=True)
    return bytes(raw)


@pytest.mark.parametrize("what", ["block_size runs past the end of the data", "l_read_name is 0", "read name not NUL-terminated",
                                  "fields longer than block_size", "refID out of range", "next_refID out of range"])
def test_malformed_records_name_their_byte(what, tmp_path):
    recs = _aligned(600, 7)
    raw, _, offs = B.raw_bam(recs, refs=_REFS)
    at = offs[-1] if what.startswith("block_size") else offs[411]
    p = B.bgzf(tmp_path / "bad.bam", _corrupt(raw, at, what))
    with pytest.raises(RuntimeError) as e:
        host.bam_read_all(p)
    assert str(e.value) == f"'{p}': not a valid BAM record at decompressed byte {at} ({what})"


def test_truncated_header(tmp_path):
    raw, hlen, _ = B.raw_bam(_aligned(10, 8), refs=_REFS)
    p = B.bgzf(tmp_path / "th.bam", raw[: hlen - 5])
    with pytest.raises(RuntimeError, match=r"not a valid BAM record at decompressed byte \d+ \(truncated header\)"):
        host.bam_read_all(p)


def test_not_bam(tmp_path):
    src = tmp_path / "r.fq"
    src.write_bytes(b"@r\nACGT\n+\nIIII\n")
    from varigraph_amd import synth
    p = synth.bgzf_compress_file(str(src), str(tmp_path / "r.fq.gz"))
    with pytest.raises(RuntimeError, match="not a BAM file"):
        host.bam_read_all(p)
