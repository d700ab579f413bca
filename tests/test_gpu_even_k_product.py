"""Even k through the product path -- host.Graph.sample_count and `varigraph-mi genotype` -- now that the device-side readers serve it:
the golden cohort_k22 in three containers against the reference's own counter dump and the host reader's run, the mid-stream hand-over
at k = 22, and the VCFs of the command line against the committed one and against the reference build."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import bam_py as B
import even_k_cases as E
import oracle_lib as o
from conftest import get_cohort
from varigraph_amd import host, synth, vgmi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "varigraph_amd", "bin", "varigraph-mi")
SERVED = b"reads from the device-side reader"      # the VGH_TIMING line of a file the device-side reader served


@pytest.fixture(scope="module")
def k22():
    cohort = get_cohort("cohort_k22")
    g = host.Graph(os.path.join(cohort.dir, "graph.bin.gz"))
    ctx = vgmi.Context(0, buffer_mib=16)
    g.upload(ctx)
    yield g, ctx, cohort
    ctx.close()
    g.close()


def _count(g, ctx, paths, monkeypatch, capfd, host_parse):
    with monkeypatch.context() as m:
        m.setenv("VGH_HOST_PARSE", "1" if host_parse else "0")
        m.setenv("VGH_TIMING", "1")
        m.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
        capfd.readouterr()
        cov, node, hist, st = g.sample_count(ctx, [str(p) for p in paths], threads=4, require_depth=False)
        log = capfd.readouterr().err.encode()
    return {"cov": cov, "node": node, "hist": hist, "n_reads": st["n_reads"], "read_base": st["read_base"], "log": log}


@pytest.mark.parametrize("form", ["gzip", "plain", "bgzf"])
def test_golden_cohort_k22_in_three_containers(form, k22, tmp_path, monkeypatch, capfd):
    """reads_1 + reads_2 (two files: two streams, two debit lists side by side) as they are, re-written plain and re-written block
    gzip: the counters of the reference's own dump, everything equal to the VGH_HOST_PARSE=1 run, and the log says who served the files."""
    g, ctx, cohort = k22
    assert cohort.k == 22
    paths = []
    for m in (1, 2):
        src = os.path.join(cohort.dir, f"reads_{m}.fq.gz")
        if form == "gzip":
            paths.append(src)
            continue
        plain = tmp_path / f"reads_{m}.fq"
        plain.write_bytes(gzip.open(src, "rb").read())
        if form == "bgzf":
            dst = tmp_path / f"reads_{m}.fq.bgz"
            synth.bgzf_compress_file(str(plain), str(dst))
            paths.append(dst)
        else:
            paths.append(plain)
    got = _count(g, ctx, paths, monkeypatch, capfd, host_parse=False)
    want = _count(g, ctx, paths, monkeypatch, capfd, host_parse=True)
    assert np.array_equal(got["cov"], cohort.ref_c_in_graph_order())
    assert got["read_base"] == cohort.ref_read_base and got["n_reads"] == cohort.n_reads
    for key in ("cov", "node", "hist"):
        assert np.array_equal(got[key], want[key]), key
    assert (got["n_reads"], got["read_base"]) == (want["n_reads"], want["read_base"])
    assert got["log"].count(SERVED) == 2 and SERVED not in want["log"]


def test_mid_stream_hand_over_at_k22(monkeypatch):
    """One record in the middle whose sequence spans two lines: the device-side reader stops there and the host reader goes on from that
    record's first byte (vgmi_reads_submit with offsets).  The counters are the oracle's over all reads, the read count the input's."""
    case = E.make("k22-path-table")
    reads = case.reads
    at = len(reads) // 2
    split = reads[at][:50] + b"\n" + reads[at][50:]
    text = E.fastq(reads[:at]) + b"@wrapped\n" + split + b"\n+\n" + b"I" * 50 + b"\n" + b"I" * (len(reads[at]) - 50) + b"\n" + E.fastq(reads[at + 1:])
    ctx = vgmi.Context(0, buffer_mib=16)
    monkeypatch.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
    try:
        ctx.table_upload(case.keys, case.k)
        # the device-side reader alone: it takes the records in front of the wrapped one and stops at its first byte
        ctx.counts_reset()
        r = ctx.fastq_text(text)
        ctx.counts_finish()
        assert (r["n_records"], r["stopped"], r["consumed"]) == (at, True, len(E.fastq(reads[:at])))
        # ... and the rest through the host path (read offsets made by the library), as the product's hand-over does
        ctx.counts_reset()
        r = ctx.fastq_text(text)
        rest = reads[at:]
        ctx.reads_submit(E.block_of(rest), len(rest))
        cov, _, _ = ctx.counts_finish()
        assert r["n_records"] + len(rest) == len(reads)
        assert np.array_equal(cov, case.want)
    finally:
        ctx.close()


def test_mid_stream_hand_over_through_sample_count(k22, tmp_path, monkeypatch, capfd):
    """The same through vgh_sample_count on the golden graph: a FASTQ file with one record of two sequence lines in the middle equals the
    host reader's run and the oracle's counters, read count and bases the input's."""
    g, ctx, cohort = k22
    seqs = [s for s in gzip.open(os.path.join(cohort.dir, "reads_1.fq.gz"), "rb").read().split(b"\n")[1::4]][:4000]
    at = len(seqs) // 2
    text = E.fastq(seqs[:at]) + b"@wrapped\n" + seqs[at][:70] + b"\n" + seqs[at][70:] + b"\n+\n" + b"I" * 70 + b"\n" + b"I" * (len(seqs[at]) - 70) + b"\n" + E.fastq(seqs[at + 1:])
    path = tmp_path / "wrapped.fq"
    path.write_bytes(text)
    got = _count(g, ctx, [path], monkeypatch, capfd, host_parse=False)
    want = _count(g, ctx, [path], monkeypatch, capfd, host_parse=True)
    t = o.Table(cohort.graph.keys)
    t.count_block(E.block_of(seqs), cohort.k)
    assert np.array_equal(got["cov"], t.counts())
    assert (got["n_reads"], got["read_base"]) == (len(seqs), sum(map(len, seqs)))
    assert np.array_equal(got["cov"], want["cov"]) and np.array_equal(got["hist"], want["hist"]) and np.array_equal(got["node"], want["node"])
    assert got["log"].count(SERVED) == 1 and (b"%d reads" % at) in got["log"]


@pytest.mark.parametrize("host_parse", ["0", "1"])
def test_cli_golden_cohort_k22(host_parse, tmp_path):
    """`varigraph-mi genotype` on the golden cohort_k22, by default and with VGH_HOST_PARSE=1: the committed VCF, byte for byte."""
    assert os.path.exists(CLI), "varigraph-mi not built"
    d = get_cohort("cohort_k22").dir
    graph = tmp_path / "graph.bin"
    graph.write_bytes(gzip.open(os.path.join(d, "graph.bin.gz"), "rb").read())
    fq = [os.path.join(d, f"reads_{i}.fq.gz") for i in (1, 2)]
    (tmp_path / "samples.cfg").write_text("sample0 " + " ".join(fq) + "\n")
    env = dict(os.environ, VGH_RANDOM_DEVICE_VALUE="20241022", VGH_HOST_PARSE=host_parse, VGH_TIMING="1")
    r = subprocess.run([CLI, "genotype", "--load-graph", str(graph), "-s", "samples.cfg", "-t", "4", "--gpu", "0", "--buffer", "8"], cwd=tmp_path,
                       capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (r.stderr.count(SERVED) == 2) == (host_parse == "0")
    got = gzip.open(tmp_path / "sample0.varigraph.vcf.gz", "rb").read()
    assert got == open(os.path.join(d, "expected_het.vcf"), "rb").read()


def test_cli_k28_fq_gz_and_bam_equal_the_reference(tmp_path_factory):
    """A `-k 28` graph constructed by both binaries, one sample as .fq.gz and one as BAM (the reference reads its twin FASTQ): the VCFs
    of the reference build, byte for byte, and both samples' files served by the device-side readers."""
    import test_gpu_configs as cfg
    cfg._need_binaries()
    work = str(tmp_path_factory.mktemp("even_k28_cli"))
    try:
        ref = synth.make_reference(200_000)
        variants, gts = synth.make_cohort(ref, 300, n_samples=5, ploidy=2, seed=11)
        fa, vcf = os.path.join(work, "ref.fa"), os.path.join(work, "in.vcf")
        synth.write_fasta(fa, "chr1", ref)
        synth.write_vcf(vcf, "chr1", len(ref), variants, gts, 5, 2)
        graphs = {}
        for name, exe, extra in (("native", cfg.CLI, ["--gpu", "0"]), ("cpu", cfg.REF, [])):
            graphs[name] = os.path.join(work, f"graph_{name}.bin")
            r = cfg._run([exe, "construct", "-r", fa, "-v", vcf, "--save-graph", graphs[name], "-t", "10", "-k", "28"] + extra, cwd=work,
                         capture_output=True, text=True, env=cfg.ENV, timeout=600)
            assert r.returncode == 0, (name, r.stderr[-2000:])
        assert open(graphs["native"], "rb").read() == open(graphs["cpu"], "rb").read()
        files = {}
        for s in (0, 1):
            haps = synth.sample_haplotypes(ref, variants, gts, s, 2)
            reads = vgmi.synth_reads_host(90 + s, 0, 50_000, 150, haps).tobytes().split(b"\n")[:-1]
            reads = [r[:60] + b"N" + r[61:] if i % 50 == 0 else r for i, r in enumerate(reads)]
            if s == 0:
                p = os.path.join(work, "s0.fq.gz")
                with gzip.open(p, "wb", compresslevel=4) as f:
                    f.write(E.fastq(reads))
                files[s] = (p, p)
            else:
                recs = [B.Rec(b"r%d" % i, r, flag=4) for i, r in enumerate(reads)]
                bam, twin = os.path.join(work, "s1.bam"), os.path.join(work, "s1_twin.fq")
                B.write_bam(bam, recs)
                B.twin_fastq(twin, recs)
                files[s] = (bam, twin)
        cfg._reference_genotype(os.path.join(work, "cpu"), graphs["cpu"], "".join(f"sample{s} {files[s][1]}\n" for s in (0, 1)), ["--use-depth"], threads=10,
                                timeout=300)
        _, log = cfg._native_genotype(os.path.join(work, "native"), graphs["native"], "".join(f"sample{s} {files[s][0]}\n" for s in (0, 1)),
                                      ["--gpu", "0", "--use-depth"], threads=10, env={"VGH_TIMING": "1"})
        assert log.count(SERVED.decode()) == 2
        for s in (0, 1):
            want = cfg._vcf(os.path.join(work, "cpu"), f"sample{s}")
            assert want.count(b"\n") > 100
            assert cfg._vcf(os.path.join(work, "native"), f"sample{s}") == want, s
    finally:
        shutil.rmtree(work, ignore_errors=True)
