"""bench_bam.py -- a sample's reads through vgh_sample_count as unaligned BAM and as block-gzip FASTQ of the same reads, with the same
member size (0xff00 bytes of text), in one process: reads/s of each, alternating, median of --reps.  Prints one JSON line.

    python tools/bench_bam.py [--reads 20000000] [--reps 3] [--dir DIR] [--only bam|fastq] [--filter [--tags 8]] [--regions]

The reads are 150 bp drawn from the C1 cohort's haplotypes (tests/golden/c1) by the seeded generator; the BAM records are unmapped
(flag 4, refID -1), named, with a quality string and no aux fields -- what a sequencer's uBAM holds.

--filter: the BAM's records carry rq as f (a tenth below 0.99) behind --tags short integer tags (0: a PacBio-like uBAM; 8: an
aligned-style record), a tenth are marked duplicate and 3 % QC-fail; the legs are the BAM with the default read filter, with exclude
0xF00 and with the tag bound rq >= 0.99 (vgh_sample_count_f), reads/s counted over the file's records.

--regions: the BAM is aligned -- 24 references chr1 .. chr22, chrX, chrY of 50 Mb, drawn refID and pos, the CIGAR 5S70M2I3D73M; the legs
are the BAM with the default read filter, with --bam-regions chr20 plus 300 intervals of 1 kb on the other references
(vgh_sample_count_r) and with exclude 0xF00 (no record has those bits: the filter kernel on the same chunks), alternating in this process, records/s counted over the file's records."""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from varigraph_amd import host, synth, vgmi  # noqa: E402

L = 150
MEMBER = 0xff00
PIECE = 1_000_000     # reads generated, laid out and compressed at a time
NT16 = np.frombuffer(b"=ACMGRSVTWYHKDBN", dtype=np.uint8)
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _member(d, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    cd = c.compress(d) + c.flush()
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(cd) + 25) + cd + struct.pack("<II", zlib.crc32(d), len(d))


class BgzfWriter:
    """members of exactly MEMBER bytes of a continuous stream (records straddle them), compressed by threads (zlib drops the GIL)"""

    def __init__(self, path, level, pool):
        self.f, self.level, self.pool, self.carry = open(path, "wb"), level, pool, b""

    def write(self, data):
        data = self.carry + data
        n = len(data) // MEMBER * MEMBER
        self.carry = data[n:]
        for m in self.pool.map(lambda o: _member(data[o:o + MEMBER], self.level), range(0, n, MEMBER)):
            self.f.write(m)

    def close(self):
        if self.carry:
            self.f.write(_member(self.carry, self.level))
        self.f.write(EOF_BLOCK)
        self.f.close()


REF_NAMES = [b"chr%d" % i for i in range(1, 23)] + [b"chrX", b"chrY"]
REF_LEN = 50_000_000
CIGAR = ((5, 4), (70, 0), (2, 1), (3, 2), (73, 0))      # 5S 70M 2I 3D 73M: 150 bases of the read, 146 of the reference


def region_list(n_short=300, seed=7):
    """chr20 whole and n_short intervals of 1 kb on the other references, as --bam-regions takes them"""
    rng = np.random.default_rng(seed)
    items = ["chr20"]
    for _ in range(n_short):
        ref = int(rng.integers(0, 24))
        beg = int(rng.integers(1, REF_LEN - 1000))
        items.append("%s:%d-%d" % (REF_NAMES[ref if ref != 19 else 0].decode(), beg, beg + 999))
    return ",".join(items)


def _records(rows, first, n_tags=None, aligned=False):
    """fixed-layout uBAM records of the reads `rows` (n x 150 ASCII): name 'r%09d', no CIGAR, SEQ, QUAL 30, no aux; n_tags (--filter):
    n_tags fields 'X<d>C' <d>, then rq:f, and drawn duplicate / QC-fail flags"""
    n = rows.shape[0]
    name = 11
    cig = 4 * len(CIGAR) if aligned else 0
    size = 4 + 32 + name + cig + L // 2 + L + (0 if n_tags is None else 4 * n_tags + 7)
    rec = np.zeros((n, size), dtype=np.uint8)
    fixed = struct.pack("<iiiBBHHHiiii", size - 4, -1, -1, name, 60 if aligned else 0, 4680, len(CIGAR) if aligned else 0, 0 if aligned else 4,
                        L, -1, -1, 0)
    rec[:, :36] = np.frombuffer(fixed, dtype=np.uint8)
    if aligned:      # (--regions) drawn refID and pos, one CIGAR
        rng = np.random.default_rng(first + 2)
        rec[:, 4:8] = rng.integers(0, len(REF_NAMES), n).astype("<i4").view(np.uint8).reshape(n, 4)
        rec[:, 8:12] = rng.integers(0, REF_LEN - 200, n).astype("<i4").view(np.uint8).reshape(n, 4)
        rec[:, 36 + name:36 + name + cig] = np.frombuffer(b"".join(struct.pack("<I", ln << 4 | op) for ln, op in CIGAR), dtype=np.uint8)
    idx = np.arange(first, first + n, dtype=np.int64)
    rec[:, 36] = ord("r")
    for d in range(9):
        rec[:, 37 + d] = (idx // 10 ** (8 - d)) % 10 + ord("0")
    code = np.zeros(256, dtype=np.uint8)
    code[NT16] = np.arange(16, dtype=np.uint8)
    c = code[rows]
    rec[:, 36 + name + cig:36 + name + cig + L // 2] = c[:, 0::2] << 4 | c[:, 1::2]
    q0 = 36 + name + cig + L // 2
    rec[:, q0:q0 + L] = 30
    if n_tags is not None:
        rng = np.random.default_rng(first + 1)
        flag = np.full(n, 4, dtype=np.uint16)
        flag[rng.random(n) < 0.1] |= 0x400
        flag[rng.random(n) < 0.03] |= 0x200
        rec[:, 18:20] = flag.view(np.uint8).reshape(n, 2)
        a = q0 + L
        for t in range(n_tags):
            rec[:, a:a + 4] = np.frombuffer(b"X%dC" % (t % 10) + bytes([t]), dtype=np.uint8)
            a += 4
        rec[:, a:a + 3] = np.frombuffer(b"rqf", dtype=np.uint8)
        rq = np.where(rng.random(n) < 0.9, rng.uniform(0.99, 1.0, n), rng.uniform(0.9, 0.99, n)).astype("<f4")
        rec[:, a + 3:a + 7] = rq.view(np.uint8).reshape(n, 4)
    return rec


def _fastq(rows, first):
    n = rows.shape[0]
    m = np.empty((n, 12 + L + 3 + L + 1), dtype=np.uint8)
    idx = np.arange(first, first + n, dtype=np.int64)
    m[:, 0], m[:, 1] = ord("@"), ord("r")
    for d in range(9):
        m[:, 2 + d] = (idx // 10 ** (8 - d)) % 10 + ord("0")
    m[:, 11] = 10
    m[:, 12:12 + L] = rows
    m[:, 12 + L], m[:, 13 + L], m[:, 14 + L] = 10, ord("+"), 10
    m[:, 15 + L:15 + 2 * L] = ord("?")
    m[:, 15 + 2 * L] = 10
    return m


def make_files(d, n_reads, haps, level, n_tags=None, aligned=False):
    bam, fq = os.path.join(d, "reads.bam"), os.path.join(d, "reads.fq.gz")
    with ThreadPoolExecutor(16) as pool:
        wb, wf = BgzfWriter(bam, level, pool), BgzfWriter(fq, level, pool)
        text = b"@HD\tVN:1.6\tSO:unknown\n@RG\tID:bench\tSM:sample0\n"
        refs = b"".join(struct.pack("<i", len(nm) + 1) + nm + b"\0" + struct.pack("<i", REF_LEN) for nm in REF_NAMES) if aligned else b""
        wb.write(b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(REF_NAMES) if aligned else 0) + refs)
        for first in range(0, n_reads, PIECE):
            n = min(PIECE, n_reads - first)
            rows = vgmi.synth_reads_host(4242, first, n, L, haps).reshape(n, L + 1)[:, :L]
            wb.write(_records(rows, first, n_tags, aligned).tobytes())
            wf.write(_fastq(rows, first).tobytes())
        wb.close()
        wf.close()
    return bam, fq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--only", choices=["bam", "fastq"], default=None)
    ap.add_argument("--filter", action="store_true", help="the read-filter legs: default, exclude 0xF00, rq >= 0.99")
    ap.add_argument("--tags", type=int, default=0, help="--filter: short tags in front of rq in every record")
    ap.add_argument("--regions", action="store_true", help="the region legs on an aligned BAM: default filter, --bam-regions chr20 + 300 x 1 kb")
    a = ap.parse_args()
    gdir = os.path.join(ROOT, "tests", "golden", "c1")
    meta = json.load(open(os.path.join(gdir, "meta.json")))
    ref = synth.make_reference(meta["ref_len"], seed=meta["ref_seed"])
    variants, gts = synth.make_cohort(ref, meta["n_var"], n_samples=meta["n_samples"], ploidy=meta["ploidy"], seed=meta["cohort_seed"])
    haps = synth.sample_haplotypes(ref, variants, gts, 0, meta["ploidy"])
    tmp = tempfile.TemporaryDirectory(dir=a.dir)
    t0 = time.perf_counter()
    bam, fq = make_files(tmp.name, a.reads, haps, a.level, a.tags if a.filter else None, a.regions)
    t_make = time.perf_counter() - t0
    g = host.Graph(os.path.join(gdir, "graph.bin.gz"))
    ctx = vgmi.Context(0)
    g.upload(ctx)
    legs = {"bam": bam, "fastq": fq} if a.only is None else {a.only: bam if a.only == "bam" else fq}
    filters = {}
    if a.filter:
        legs = {"bam": bam, "bam_exclude": bam, "bam_tag": bam}
        filters = {"bam_exclude": dict(exclude=0xF00), "bam_tag": dict(tag=b"rq", min_value=0.99)}
    regions = {}
    if a.regions:
        legs = {"bam": bam, "bam_regions": bam, "bam_exclude": bam}      # (the third: 4.23's filter kernel on the same chunks)
        regions = {"bam_regions": region_list()}
        filters = {"bam_exclude": dict(exclude=0xF00)}
    rates, stats = {k: [] for k in legs}, {}
    g.sample_count(ctx, [bam], threads=16, require_depth=False)      # warm-up: code objects, pinned buffers
    for _ in range(a.reps):
        for k, p in legs.items():
            t = time.perf_counter()
            cov, _, hist, st = g.sample_count(ctx, [p], threads=16, require_depth=False, bam_filter=filters.get(k), bam_regions=regions.get(k))
            dt = time.perf_counter() - t
            rates[k].append((a.reads if a.filter or a.regions else st["n_reads"]) / dt)      # (--filter, --regions: the file's records per second)
            stats[k] = (st["n_reads"], st["read_base"], hist.tobytes())
    if len(stats) == 2 and not a.filter and not a.regions:
        assert stats["bam"] == stats["fastq"], "BAM and FASTQ legs count differently"
    out = {"tool": "bench_bam", "reads": a.reads, "read_len": L, "member_text_bytes": MEMBER, "level": a.level,
           "bytes": {k: os.path.getsize(p) for k, p in (("bam", bam), ("fastq", fq))}, "make_s": round(t_make, 1),
           "reads_per_s": {k: float("%.4g" % statistics.median(v)) for k, v in rates.items()},
           "runs": {k: ["%.4g" % x for x in v] for k, v in rates.items()}}
    if a.filter:
        out["filter"] = {"tags": a.tags, "reads_passed": {k: stats[k][0] for k in stats}}
    if a.regions:
        out["regions"] = {"intervals": regions["bam_regions"].count(",") + 1, "reads_passed": {k: stats[k][0] for k in stats},
                          "default_min_max": ["%.4g" % min(rates["bam"]), "%.4g" % max(rates["bam"])]}
    if len(stats) == 2 and not a.filter and not a.regions:
        out["bam_over_fastq"] = round(out["reads_per_s"]["bam"] / out["reads_per_s"]["fastq"], 3)
    print(json.dumps(out))
    ctx.close()
    g.close()
    tmp.cleanup()


if __name__ == "__main__":
    main()
