"""`genotype --bam-regions / --bam-regions-file / --bam-regions-unplaced` against the unmodified reference: the reads of cohort_snp as an
aligned BAM over four references with drawn positions and CIGARs (S, I, D, N among them), unmapped mates and unplaced reads; the VCF
must be the reference's, byte for byte, on the twin FASTQ of the records the Python model (bam_region_cases.py) lets pass.  A FASTQ
sample in the same run is untouched.  The VGH_TIMING line names the options and the BED lines skipped; the refusal of an unknown
reference names the file.  The parameter errors are in test_bam_region_cpu.py (they need no device)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bam_filter_cases as F
import bam_py as B
import bam_region_cases as R
from conftest import GOLDEN
from test_gpu_bam_filter_cli import cohort_reads

pytestmark = pytest.mark.gpu

D = os.path.join(GOLDEN, "cohort_snp")
LIST = "chr1:101-200,chr1:301-400,chr1:1001-1100,chr2:2147483639-2147483648,chrLast"      # R.CASE_REGIONS, 1-based inclusive


def placed_records(reads, seed=43):
    """a third of the reads on chrLast (a whole-reference region), the others on chr1 around its intervals, on chr2 or the HLA contig;
    3 % unplaced, 5 % unmapped mates placed at their mate's position, a few duplicates; CIGARs with soft clips, insertions, deletions
    and introns"""
    rng = np.random.default_rng(seed)
    recs = []
    for name, seq, qual in reads:
        u = rng.random()
        if u < 0.03:
            recs.append(B.Rec(name, seq, flag=4 | 0x1 | 0x8, ref=-1, pos=-1, mapq=0, qual=qual))
            continue
        ref = int(rng.choice(4, p=(0.45, 0.1, 0.12, 0.33)))
        pos = int(rng.integers(0, 1300))
        n = len(seq)
        clip, ins = int(rng.integers(0, 20)) if rng.random() < 0.3 else 0, int(rng.integers(1, 6)) if rng.random() < 0.2 else 0
        gap = (int(rng.integers(1, 200)), "DN"[int(rng.integers(0, 2))]) if rng.random() < 0.3 else None
        left = (n - clip - ins) // 2
        cigar = ([(clip, "S")] if clip else []) + [(left, "M")] + ([(ins, "I")] if ins else []) + ([gap] if gap else []) + [(n - clip - ins - left, "M")]
        flag = (0x10 if rng.random() < 0.5 else 0) | (0x400 if rng.random() < 0.1 else 0)
        if rng.random() < 0.05:
            flag, cigar = flag | 4, []
        recs.append(B.Rec(name, seq, flag=flag, ref=ref, pos=pos, mapq=int(rng.choice((0, 20, 60))), cigar=cigar, qual=qual,
                          aux=F.aux(b"NM", "C", 1)))
    return recs


CASES = {
    "list": (["--bam-regions", LIST], R.CASE_REGIONS, False, F.Filter(), "--bam-regions " + LIST),
    "bed_unplaced_with_flags": (["--bam-regions", "chrLast", "--bam-regions-file", "@BED@", "--bam-regions-unplaced", "--bam-exclude-flags", "0xD00"],
                                R.CASE_REGIONS, True, F.Filter(exclude=0xD00),
                                "--bam-exclude-flags 0xD00 --bam-regions chrLast --bam-regions-file @BED@ --bam-regions-unplaced; 2 BED lines skipped, "
                                "reference not in the header"),
}
BED = "# targets\nchr1\t100\t200\tt1\nchrUn_KI270302v1\t0\t100\nchr1\t300\t400\nchr1\t1000\t1100\nchr2\t2147483638\t2147483648\nchrEBV\t5\t9\n"


def _graph(work):
    graph = os.path.join(work, "graph.bin")
    open(graph, "wb").write(gzip.open(os.path.join(D, "graph.bin.gz"), "rb").read())
    return graph


@pytest.mark.parametrize("case", list(CASES))
def test_cli_equals_the_reference_on_the_twin_of_the_passing_records(case, tmp_path):
    import test_gpu_configs as cfg
    cfg._need_binaries()
    opts, regions, unplaced, f, text = CASES[case]
    work = str(tmp_path)
    graph = _graph(work)
    bed = os.path.join(work, "targets.bed")
    open(bed, "w").write(BED)
    opts = [bed if o == "@BED@" else o for o in opts]
    text = text.replace("@BED@", bed)
    recs = placed_records(cohort_reads())
    bam = os.path.join(work, "a.bam")
    R.write_bam(bam, recs)
    passing, n_rec, n_reads, at = R.apply(recs, f, regions, unplaced)
    assert at is None and 0.3 * n_rec < n_reads < 0.8 * n_rec
    B.twin_fastq(os.path.join(work, "twin.fq"), passing)
    fq = os.path.join(D, "reads_1.fq.gz")
    cfg._reference_genotype(os.path.join(work, "ref"), graph, f"sample0 {work}/twin.fq\nsample1 {fq}\n", [], threads=4, timeout=25)
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
def test_cli_refuses_a_reference_the_header_lacks(env, tmp_path):
    import test_gpu_configs as cfg
    cfg._need_binaries()
    work = str(tmp_path)
    graph = _graph(work)
    bam = os.path.join(work, "a.bam")
    R.write_bam(bam, placed_records(cohort_reads()[:200]))
    open(os.path.join(work, "samples.cfg"), "w").write(f"sample0 {bam}\n")
    r = subprocess.run([cfg.CLI, "genotype", "--load-graph", graph, "-s", "samples.cfg", "-t", "4", "--gpu", "0", "--buffer", "8", "--bam-regions",
                        "chr1:5-90,chr20:1-1000"], cwd=work, capture_output=True, text=True, env=dict(cfg.ENV, **env), timeout=300)
    assert r.returncode == 1 and f"'{bam}': reference 'chr20' of region 'chr20:1-1000' is not in the header" in r.stderr, r.stderr[-2000:]
    assert not [p for p in os.listdir(work) if p.endswith(".vcf.gz")]
