"""`genotype --bam-exclude-flags / --bam-min-mapq / --bam-min-tag` against the unmodified reference: the reads of cohort_snp (drawn from
its haplotypes) as an aligned-style BAM with drawn duplicates, QC failures and MAPQ, and as an unaligned BAM with rq; the VCF must be
the reference's, byte for byte, on the twin FASTQ of the records the Python model (bam_filter_cases.py) lets pass -- filtered, then
subsampled, then masked.  A FASTQ sample in the same run is untouched by the BAM options.  The VGH_TIMING line and the walk-fault error are checked;
the parameter errors are in test_bam_filter_cpu.py (they need no device)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bam_filter_cases as F
import bam_py as B
import quality_mask_cases as Q
import subsample_cases as S
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

D = os.path.join(GOLDEN, "cohort_snp")
_TEXT = b"@HD\tVN:1.6\tSO:unsorted\n"


def cohort_reads():
    """(name, seq, raw Phred bytes) of both committed read files, mate 1 then mate 2"""
    out = []
    for mate in (1, 2):
        text = Q.draw_qualities(gzip.open(os.path.join(D, f"reads_{mate}.fq.gz"), "rb").read(), 300 + mate)
        out += [(b"%s/%d" % (n.split()[0], mate), s, bytes(c - 33 for c in q)) for n, s, q in Q.records_of(text)]
    return out


def aligned_records(reads, seed=41):
    """duplicate-marked, aligned-style: 15 % duplicates, 5 % QC failures, a few secondary / supplementary, half on the reverse strand,
    MAPQ 0 / 5 / 20 / 60"""
    rng = np.random.default_rng(seed)
    recs = []
    for name, seq, qual in reads:
        flag = (0x10 if rng.random() < 0.5 else 0) | (0x400 if rng.random() < 0.15 else 0) | (0x200 if rng.random() < 0.05 else 0)
        flag |= 0x100 if rng.random() < 0.02 else 0x800 if rng.random() < 0.02 else 0
        mapq = (0, 5, 20, 60)[int(rng.choice(4, p=(0.04, 0.06, 0.1, 0.8)))]
        recs.append(B.Rec(name, seq, flag=flag, mapq=mapq, qual=qual, aux=F.aux(b"NM", "C", 1) + F.aux(b"RG", "Z", b"grp")))
    return recs


def unaligned_records(reads, seed=42):
    """PacBio-like uBAM: rq as f in every record, 85 % at or above 0.99 (0.99f itself among them)"""
    rng = np.random.default_rng(seed)
    recs = []
    for i, (name, seq, qual) in enumerate(reads):
        rq = 0.99 if i % 50 == 0 else F.f32_below(0.99) if i % 50 == 1 else float(rng.uniform(0.99, 1.0) if rng.random() < 0.85 else rng.uniform(0.9, 0.99))
        recs.append(B.Rec(name, seq, flag=4, mapq=255, qual=qual, aux=F.aux(b"zm", "i", i) + F.aux(b"rq", "f", rq) + F.aux(b"np", "i", 9)))
    return recs


CASES = {
    "flags_mapq": ("aligned", F.Filter(exclude=0xF00, min_mapq=20), ["--bam-exclude-flags", "0xF00", "--bam-min-mapq", "20"], None, 0,
                   "--bam-exclude-flags 0xF00 --bam-min-mapq 20"),
    "rq": ("unaligned", F.Filter(tag=b"rq", min_value=0.99), ["--bam-min-tag", "rq:0.99"], None, 0, "--bam-min-tag rq:0.99"),
    "rq_subsample_quality": ("unaligned", F.Filter(tag=b"rq", min_value=0.99),
                             ["--bam-min-tag", "rq:0.99", "--subsample", "0.5", "--min-base-quality", "20"], (0.5, 11), 20, "--bam-min-tag rq:0.99"),
}


def twin(path, recs, f, sub=None, q=0):
    """the twin FASTQ of the records that pass f, then the rule of --subsample, then the mask of --min-base-quality -> (records, reads)"""
    passing, n_rec, n_reads, at = F.apply(recs, f)
    assert at is None
    if sub:
        passing = S.bam_filtered(passing, sub[0], sub[1])[0]
    if q:
        passing = Q.masked_bam_records(passing, q)[0]
    B.twin_fastq(path, passing)
    return n_rec, n_reads


def _graph(work):
    graph = os.path.join(work, "graph.bin")
    open(graph, "wb").write(gzip.open(os.path.join(D, "graph.bin.gz"), "rb").read())
    return graph


@pytest.mark.parametrize("case", list(CASES))
def test_cli_equals_the_reference_on_the_twin_of_the_passing_records(case, tmp_path):
    import test_gpu_configs as cfg
    cfg._need_binaries()
    kind, f, opts, sub, q, text = CASES[case]
    work = str(tmp_path)
    graph = _graph(work)
    recs = (aligned_records if kind == "aligned" else unaligned_records)(cohort_reads())
    bam = os.path.join(work, "a.bam")
    B.write_bam(bam, recs, text=_TEXT)
    n_rec, n_reads = twin(os.path.join(work, "twin.fq"), recs, f, sub, q)
    assert 0.5 * n_rec < n_reads < 0.95 * n_rec
    fq = os.path.join(D, "reads_1.fq.gz")
    # two samples in one run: the BAM, and a FASTQ file the BAM options do not touch (--subsample and --min-base-quality do: the
    # reference then reads that file's own kept and masked records)
    fq_ref = fq
    if sub or q:
        fq_text = gzip.open(fq, "rb").read()
        fq_text = S.filtered_fastq_text(fq_text, sub[0], sub[1])[0] if sub else fq_text
        fq_ref = os.path.join(work, "fq_twin.fq")
        open(fq_ref, "wb").write(Q.masked_text(fq_text, q)[0] if q else fq_text)
    cfg._reference_genotype(os.path.join(work, "ref"), graph, f"sample0 {work}/twin.fq\nsample1 {fq_ref}\n", [], threads=4, timeout=25)
    _, log = cfg._native_genotype(os.path.join(work, "nat"), graph, f"sample0 {bam}\nsample1 {fq}\n", ["--gpu", "0", "--buffer", "8"] + opts,
                                  threads=4, env={"VGH_TIMING": "1"})
    for s in ("sample0", "sample1"):
        want = cfg._vcf(os.path.join(work, "ref"), s)
        print(f"{case} {s}: reference VCF has {want.count(bytes([10]))} lines")
        assert want.count(b"\n") > 50 and cfg._vcf(os.path.join(work, "nat"), s) == want, s
    lines = [ln for ln in log.splitlines() if "BAM records are reads" in ln]
    assert lines == [f"[varigraph-mi] '{bam}': {n_reads} of {n_rec} BAM records are reads ({text})"], log[-2000:]
    # without the options the BAM gives another VCF
    cfg._native_genotype(os.path.join(work, "off"), graph, f"sample0 {bam}\n", ["--gpu", "0", "--buffer", "8"], threads=4)
    assert cfg._vcf(os.path.join(work, "off"), "sample0") != cfg._vcf(os.path.join(work, "ref"), "sample0")


@pytest.mark.parametrize("env", ({}, {"VGH_HOST_PARSE": "1"}), ids=["device", "host_parse"])
def test_cli_ends_at_a_record_whose_auxiliary_fields_cannot_be_walked(env, tmp_path):
    import test_gpu_configs as cfg
    cfg._need_binaries()
    work = str(tmp_path)
    graph = _graph(work)
    recs = unaligned_records(cohort_reads()[:400])
    recs[250] = B.Rec(b"bad", recs[250].seq, flag=4, qual=recs[250].qual, aux=F.aux(b"zm", "i", 250) + F.fault("nonul"))
    bam = os.path.join(work, "a.bam")
    _, offs = B.write_bam(bam, recs, text=_TEXT)
    open(os.path.join(work, "samples.cfg"), "w").write(f"sample0 {bam}\n")
    r = subprocess.run([cfg.CLI, "genotype", "--load-graph", graph, "-s", "samples.cfg", "-t", "4", "--gpu", "0", "--buffer", "8", "--bam-min-tag", "rq:0.99"],
                       cwd=work, capture_output=True, text=True, env=dict(cfg.ENV, **env), timeout=300)
    assert r.returncode == 1 and f"'{bam}': not a valid BAM record at decompressed byte {offs[250]} (auxiliary fields)" in r.stderr, r.stderr[-2000:]
    assert not [p for p in os.listdir(work) if p.endswith(".vcf.gz")]
