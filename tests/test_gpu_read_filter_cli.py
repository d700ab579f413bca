"""`genotype --min-read-length / --min-read-quality / --max-low-quality` against the unmodified reference: the reads of cohort_snp with
qualities of five kinds and a tenth of them cut short, as a gzip FASTQ pair and as a BAM; the VCF must be the reference's, byte for
byte, on the twin FASTQ of the reads the Python model (read_filter_cases.py) lets pass.  The same under --procs with one rank.  The
VGH_TIMING line is checked; the parameter errors are in test_read_filter_cpu.py (they need no device)."""
import gzip
import os

import numpy as np
import pytest

import bam_py as B
import quality_mask_cases as Q
import read_filter_cases as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

D = os.path.join(GOLDEN, "cohort_snp")
_TEXT = b"@HD\tVN:1.6\tSO:unsorted\n"
RULE = R.Rule(min_len=100, min_mean_q=75, lowq_below=15, lowq_max_pct=40)
OPTS = ["--min-read-length", "100", "--min-read-quality", "7.5", "--max-low-quality", "15:40"]


def cohort_records(mate):
    """(name, seq, quality bytes) of a committed read file: every tenth read cut to 60 bases, qualities of five kinds"""
    rng = np.random.default_rng(500 + mate)
    out = []
    for i, (n, s, _) in enumerate(Q.records_of(gzip.open(os.path.join(D, f"reads_{mate}.fq.gz"), "rb").read())):
        if i % 10 == 3:
            s = s[:60]
        kind = (0, 0, 1, 0, 0, 2, 0, 0, 3, 0, 4)[i % 11]
        out.append((n.split()[0], s, R._ph(R.drawn_quality(rng, len(s), kind))))
    return out


def _graph(work):
    graph = os.path.join(work, "graph.bin")
    open(graph, "wb").write(gzip.open(os.path.join(D, "graph.bin.gz"), "rb").read())
    return graph


def _timing_lines(log):
    return sorted(ln for ln in log.splitlines() if "reads kept (" in ln and "short" in ln)


def _line(path, classes):
    st = R.class_counts(classes)
    return f"[varigraph-mi] '{path}': {st[0] - sum(st[1:])} of {st[0]} reads kept ({st[1]} short, {st[2]} long, {st[3]} low fraction, {st[4]} low mean)"


@pytest.mark.parametrize("procs", [False, True], ids=["one_process", "procs_one_rank"])
def test_cli_fastq_pair_equals_the_reference_on_the_twin_files(procs, tmp_path):
    import test_gpu_configs as cfg
    cfg._need_binaries()
    work = str(tmp_path)
    graph = _graph(work)
    G, GP, lines = [], [], []
    for mate in (1, 2):
        recs = cohort_records(mate)
        kept, classes = R.fastq_filtered(recs, RULE)
        st = R.class_counts(classes)
        assert all(c > 0 for c in (st[1], st[3], st[4])) and 3 * len(kept) >= len(recs)
        G.append(os.path.join(work, f"g_{mate}.fq.gz"))
        GP.append(os.path.join(work, f"gp_{mate}.fq"))
        open(G[-1], "wb").write(gzip.compress(R.fastq_text(recs), 6))
        open(GP[-1], "wb").write(R.fastq_text(kept))
        lines.append(_line(G[-1], classes))
    cfg._reference_genotype(os.path.join(work, "ref"), graph, "sample0 " + " ".join(GP) + "\n", [], threads=4, timeout=25)
    want = cfg._vcf(os.path.join(work, "ref"), "sample0")
    print(f"reference VCF on the twin files has {want.count(bytes([10]))} lines")
    opts = ["--gpus", "0", "--procs"] if procs else ["--gpu", "0"]
    _, log = cfg._native_genotype(os.path.join(work, "nat"), graph, "sample0 " + " ".join(G) + "\n", opts + ["--buffer", "8"] + OPTS, threads=4,
                                  env={"VGH_TIMING": "1"})
    assert want.count(b"\n") > 50 and cfg._vcf(os.path.join(work, "nat"), "sample0") == want
    assert _timing_lines(log) == sorted(lines), log[-2000:]
    assert log.count("reads from the device-side reader") == 2
    if not procs:      # without the options the files give another VCF
        cfg._native_genotype(os.path.join(work, "off"), graph, "sample0 " + " ".join(G) + "\n", ["--gpu", "0", "--buffer", "8"], threads=4)
        assert cfg._vcf(os.path.join(work, "off"), "sample0") != want


@pytest.mark.parametrize("procs", [False, True], ids=["one_process", "procs_one_rank"])
def test_cli_bam_equals_the_reference_on_the_twin_fastq(procs, tmp_path):
    import test_gpu_configs as cfg
    cfg._need_binaries()
    work = str(tmp_path)
    graph = _graph(work)
    recs = []
    for mate in (1, 2):
        for i, (n, s, q) in enumerate(cohort_records(mate)):
            qual = b"\xff" * len(s) if i % 97 == 5 else bytes(c - 33 for c in q)      # a few records without qualities: the length test alone
            recs.append(B.Rec(b"%s/%d" % (n, mate), s, flag=16 if i % 2 else 4, qual=qual))
    gp, classes, n_reads = R.bam_filtered(recs, RULE)
    st = R.class_counts(classes)
    assert n_reads == len(recs) and all(c > 0 for c in (st[1], st[3], st[4])) and 3 * len(gp) >= len(recs)
    bam = os.path.join(work, "a.bam")
    B.write_bam(bam, recs, text=_TEXT)
    B.twin_fastq(os.path.join(work, "twin.fq"), gp)
    cfg._reference_genotype(os.path.join(work, "ref"), graph, f"sample0 {work}/twin.fq\n", [], threads=4, timeout=25)
    want = cfg._vcf(os.path.join(work, "ref"), "sample0")
    print(f"reference VCF on the twin FASTQ has {want.count(bytes([10]))} lines")
    opts = ["--gpus", "0", "--procs"] if procs else ["--gpu", "0"]
    _, log = cfg._native_genotype(os.path.join(work, "nat"), graph, f"sample0 {bam}\n", opts + ["--buffer", "8"] + OPTS, threads=4, env={"VGH_TIMING": "1"})
    assert want.count(b"\n") > 50 and cfg._vcf(os.path.join(work, "nat"), "sample0") == want
    assert _timing_lines(log) == [_line(bam, classes)], log[-2000:]
