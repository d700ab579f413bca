"""BAM / unaligned BAM samples on the device (vgmi_fastq_open_bam, csrc/vgmi_bam.hip) against their FASTQ twin -- the FASTQ
`samtools fastq` writes from the same BAM (tests/bam_py.py) -- through today's FASTQ path: counters, per-node counters, the
histogram, n_reads and read_base bit for bit, and the genotype VCF byte for byte against the reference on the twin."""
import os
import shutil

import numpy as np
import pytest

import bam_py as B
import oracle_lib as o
from conftest import get_cohort
from varigraph_amd import host, synth, vgmi

pytestmark = pytest.mark.gpu

_REFS = [(b"chr1", 100000), (b"chr2", 5000)]
_TEXT = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@PG\tID:step%d\tPN:pipeline\tCL:some command line %d\n" % (i, i) for i in range(150))


def _records(haps, n, seed, lo=60, hi=260):
    """reads of `haps` as BAM records: forward and reverse-strand (stored reverse-complemented, as aligners store them), unmapped,
    with secondary / supplementary copies, SEQ '*' records, N and IUPAC codes"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h = haps[int(rng.integers(0, len(haps)))]
        ln = int(rng.integers(lo, hi))
        s0 = int(rng.integers(0, len(h) - ln))
        r = bytearray(h[s0:s0 + ln].tobytes().upper())
        if rng.random() < 0.1:
            r[int(rng.integers(0, ln))] = ord("N")
        if rng.random() < 0.05:
            r[int(rng.integers(0, ln))] = B.NT16[int(rng.integers(0, 16))]
        r = bytes(r)
        kind = rng.random()
        if kind < 0.4:
            out.append(B.Rec(b"r%d" % i, r, flag=0, ref=0, pos=s0, mapq=60, cigar=[(ln, "M")]))
        elif kind < 0.8:
            out.append(B.Rec(b"r%d" % i, B.revcomp(r), flag=16 | (0x400 if i % 13 == 0 else 0), ref=1, pos=s0, mapq=60, cigar=[(ln, "M")],
                             next_ref=0))
        else:
            out.append(B.Rec(b"r%d" % i, r, flag=4 | (0x200 if i % 7 == 0 else 0)))
        if i % 17 == 0:        # alignments of the same read that are not reads
            out.append(B.Rec(b"r%d" % i, r[::-1], flag=256, ref=0, pos=3, cigar=[(ln, "M")]))
            out.append(B.Rec(b"r%d" % i, r[: ln // 2], flag=2048 | 16, ref=1, pos=4, cigar=[(ln // 2, "M")]))
        if i % 101 == 0:
            out.append(B.Rec(b"star%d" % i, b"", flag=4))
    return out


def _graph_ctx(path):
    g = host.Graph(path)
    ctx = vgmi.Context(0, buffer_mib=16)
    g.upload(ctx)
    return g, ctx


@pytest.fixture(scope="module")
def snp():
    cohort = get_cohort("cohort_snp")
    g, ctx = _graph_ctx(os.path.join(cohort.dir, "graph.bin.gz"))
    yield g, ctx, cohort.haplotypes(), cohort
    ctx.close()
    g.close()


@pytest.fixture(scope="module")
def k22():
    cohort = get_cohort("cohort_k22")
    g, ctx = _graph_ctx(os.path.join(cohort.dir, "graph.bin.gz"))
    yield g, ctx, cohort.haplotypes(), cohort
    ctx.close()
    g.close()


@pytest.fixture(scope="module")
def k21(tmp_path_factory):
    """a graph of another odd k, built by `varigraph-mi construct -k 21`"""
    import test_gpu_configs as cfg
    cfg._need_binaries()
    work = str(tmp_path_factory.mktemp("bam_k21"))
    ref = synth.make_reference(80_000)
    variants, gts = synth.make_cohort(ref, 150, n_samples=4, ploidy=2, seed=5)
    fa, vcf, graph = os.path.join(work, "ref.fa"), os.path.join(work, "in.vcf"), os.path.join(work, "graph.bin")
    synth.write_fasta(fa, "chr1", ref)
    synth.write_vcf(vcf, "chr1", len(ref), variants, gts, 4, 2)
    r = cfg._run([cfg.CLI, "construct", "-r", fa, "-v", vcf, "--save-graph", graph, "-t", "16", "--gpu", "0", "-k", "21"], cwd=work,
                 capture_output=True, text=True, env=cfg.ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    g, ctx = _graph_ctx(graph)
    yield g, ctx, synth.sample_haplotypes(ref, variants, gts, 0, 2), None
    ctx.close()
    g.close()
    shutil.rmtree(work, ignore_errors=True)


def _count(g, ctx, paths, monkeypatch, host_parse=False, chunk_kb=None):
    with monkeypatch.context() as m:
        m.setenv("VGH_HOST_PARSE", "1" if host_parse else "0")
        if chunk_kb:
            m.setenv("VGMI_FASTQ_CHUNK_KB", str(chunk_kb))
        else:
            m.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
        cov, node, hist, st = g.sample_count(ctx, [str(p) for p in paths], threads=4, require_depth=False)
    return {"cov": cov, "node": node, "hist": hist, "n_reads": st["n_reads"], "read_base": st["read_base"]}


def _same(a, b):
    assert np.array_equal(a["cov"], b["cov"]) and np.array_equal(a["node"], b["node"]) and np.array_equal(a["hist"], b["hist"])
    assert (a["n_reads"], a["read_base"]) == (b["n_reads"], b["read_base"])


def _files(tmp_path, recs, name="s", **kw):
    bam, twin = tmp_path / (name + ".bam"), tmp_path / (name + ".fq")
    hlen, offs = B.write_bam(bam, recs, text=_TEXT, refs=_REFS, **kw)
    B.twin_fastq(twin, recs)
    return bam, twin, hlen, offs


@pytest.mark.parametrize("which", ["snp", "k21"])
@pytest.mark.parametrize("chunk_kb,block", [(None, 0xff00), (64, 0xff00), (4, 3000)])
def test_device_takes_every_record(which, chunk_kb, block, request, tmp_path, monkeypatch):
    """Ctx.bam_bgzf: every kept record is found and decoded on the device (none left for the host), also when 4 KiB / 64 KiB chunks put
    records, and the header, across chunk and member boundaries; counters equal the twin's through the device FASTQ parser."""
    g, ctx, haps, cohort = request.getfixturevalue(which)
    recs = _records(haps, 1500, 3)
    bam, twin, hlen, _ = _files(tmp_path, recs, block=block)
    raw, _, _ = B.raw_bam(recs, text=_TEXT, refs=_REFS)
    want_block, n_kept, rb = B.reads_block(recs)
    with monkeypatch.context() as m:
        if chunk_kb:
            m.setenv("VGMI_FASTQ_CHUNK_KB", str(chunk_kb))
        ctx.counts_reset()
        r = ctx.bam_bgzf(bam.read_bytes(), hlen, len(_REFS))
        cov, _, _ = ctx.counts_finish()
    assert not r["stopped"] and not r["inflate_failed"] and r["tail"] == b""
    assert (r["n_records"], r["n_bases"], r["consumed"]) == (n_kept, rb, len(raw))
    if cohort is not None:
        t = o.Table(cohort.graph.keys)
        t.count_block(np.frombuffer(want_block, dtype=np.uint8), cohort.k)
        assert np.array_equal(cov, t.counts())
    want = _count(g, ctx, [twin], monkeypatch)
    assert np.array_equal(cov, want["cov"]) and want["n_reads"] == n_kept
    _same(_count(g, ctx, [bam], monkeypatch, chunk_kb=chunk_kb), want)


@pytest.mark.parametrize("which", ["snp", "k22"])
def test_sample_count_bam_equals_twin(which, request, tmp_path, monkeypatch):
    """vgh_sample_count: a BAM listed alone, and next to a FASTQ file of the same sample, equals its twin (odd k: device records;
    even k: the host decoder)."""
    g, ctx, haps, _ = request.getfixturevalue(which)
    recs = _records(haps, 4000, 11)
    bam, twin, _, _ = _files(tmp_path, recs)
    want = _count(g, ctx, [twin], monkeypatch)
    assert want["n_reads"] == B.reads_block(recs)[1]
    _same(_count(g, ctx, [bam], monkeypatch), want)
    _same(_count(g, ctx, [bam], monkeypatch, host_parse=True), want)
    other = _records(haps, 800, 12)
    fq = B.twin_fastq(tmp_path / "other.fq", other)
    _same(_count(g, ctx, [bam, fq], monkeypatch), _count(g, ctx, [twin, fq], monkeypatch))


@pytest.mark.parametrize("which", ["snp", "k22"])
def test_reverse_complement_adds_the_same_keys(which, request, tmp_path, monkeypatch):
    """Every read twice, as stored and reverse-complemented with 0x10: the twin of the forward reads taken twice (odd and even k)."""
    g, ctx, haps, _ = request.getfixturevalue(which)
    fwd = [r for r in _records(haps, 2000, 21) if r.kept and not r.flag & 0x10]
    recs = []
    for r in fwd:
        recs += [B.Rec(r.name, r.seq, flag=0, ref=0, pos=1, cigar=[(len(r.seq), "M")]),
                 B.Rec(r.name, B.revcomp(r.seq), flag=16, ref=0, pos=1, cigar=[(len(r.seq), "M")])]
    bam = tmp_path / "rc.bam"
    B.write_bam(bam, recs, refs=_REFS)
    twin = B.twin_fastq(tmp_path / "fwd2.fq", [B.Rec(r.name, r.seq, flag=0) for r in fwd for _ in range(2)])
    _same(_count(g, ctx, [bam], monkeypatch), _count(g, ctx, [twin], monkeypatch))


def test_a_record_longer_than_the_carry_goes_to_the_host(snp, tmp_path, monkeypatch):
    """A 3 MiB record in the middle: the device stops at its first byte, the host decoder counts it and the rest of the file."""
    g, ctx, haps, _ = snp
    recs = _records(haps, 1200, 31)
    big = np.frombuffer(np.concatenate([haps[0]] * (3 * 2 ** 20 // haps[0].size + 1)).tobytes().upper(), dtype=np.uint8)[: 3 << 20]
    at = len(recs) // 2
    recs.insert(at, B.Rec(b"big", big.tobytes(), flag=4))
    bam, twin, hlen, offs = _files(tmp_path, recs)
    ctx.counts_reset()
    r = ctx.bam_bgzf(bam.read_bytes(), hlen, len(_REFS))
    ctx.counts_finish()
    assert r["stopped"] and r["consumed"] == offs[at] and r["n_records"] == B.reads_block(recs[:at])[1]
    _same(_count(g, ctx, [bam], monkeypatch), _count(g, ctx, [twin], monkeypatch))


@pytest.mark.parametrize("damage", ["flip_in_third_member", "malformed_record"])
def test_damage_matches_the_host_decoder(damage, snp, tmp_path, monkeypatch):
    """A flipped byte in the third member (the device cannot vouch for it), a malformed record: the device path gives what the
    host decoder gives -- the same counters, or the same error."""
    g, ctx, haps, _ = snp
    recs = _records(haps, 3000, 41)
    raw, _, offs = B.raw_bam(recs, text=_TEXT, refs=_REFS)
    if damage == "malformed_record":
        raw = bytearray(raw)
        raw[offs[2000] + 12] = 0
        raw = bytes(raw)
    p = B.bgzf(tmp_path / "d.bam", raw)
    if damage == "flip_in_third_member":
        comp = bytearray(open(p, "rb").read())
        m = 0
        for _ in range(2):
            m += (comp[m + 16] | comp[m + 17] << 8) + 1
        comp[m + 300] ^= 0x5A
        open(p, "wb").write(bytes(comp))

    def run(host_parse):
        try:
            return _count(g, ctx, [p], monkeypatch, host_parse=host_parse)
        except vgmi.VgmiError as e:
            return str(e)
    want, got = run(True), run(False)
    if isinstance(want, str):
        assert got == want and "not a valid BAM record at decompressed byte" in want
        if damage == "malformed_record":
            assert f"byte {offs[2000]} (l_read_name is 0)" in want
    else:
        _same(got, want)


def test_cli_genotype_on_a_bam_equals_the_reference_on_its_twin(tmp_path_factory):
    """`varigraph-mi genotype --use-depth` with a BAM in samples.cfg writes the VCF the reference writes on the twin FASTQ."""
    import test_gpu_configs as cfg
    cfg._need_binaries()
    work = str(tmp_path_factory.mktemp("bam_cli"))
    try:
        ref, variants, gts, graph = cfg._dataset(work, 200_000, 300, 5, 2)
        haps = synth.sample_haplotypes(ref, variants, gts, 0, 2)
        block = vgmi.synth_reads_host(77, 0, 60_000, 150, haps).tobytes()
        reads = block.split(b"\n")[:-1]
        recs = []
        for i, r in enumerate(reads):
            if i % 2:
                recs.append(B.Rec(b"p%d" % i, B.revcomp(r), flag=16 | 1 | 128, ref=0, pos=i, mapq=60, cigar=[(len(r), "M")], next_ref=0))
            else:
                recs.append(B.Rec(b"p%d" % i, r, flag=4 | 1 | 64))
            if i % 50 == 0:
                recs.append(B.Rec(b"p%d" % i, r[::-1], flag=256, ref=0, pos=i, cigar=[(len(r), "M")]))
        bam, twin = os.path.join(work, "s.bam"), os.path.join(work, "s.fq")
        B.write_bam(bam, recs, refs=[(b"chr1", len(ref))])
        B.twin_fastq(twin, recs)
        cfg._native_genotype(os.path.join(work, "native"), graph, f"sample0 {bam}\n", ["--gpu", "0", "--use-depth"], threads=10)
        cfg._reference_genotype(os.path.join(work, "cpu"), graph, f"sample0 {twin}\n", ["--use-depth"], threads=10, timeout=300)
        got, want = cfg._vcf(os.path.join(work, "native"), "sample0"), cfg._vcf(os.path.join(work, "cpu"), "sample0")
        assert got == want and got.count(b"\n") > 100
    finally:
        shutil.rmtree(work, ignore_errors=True)
