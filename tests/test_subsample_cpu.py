"""Subsampling without a device: the rule's known answers (the stand-alone check of the C++ function under ASan + UBSan, and the Python
model of subsample_cases.py), the host readers' form of it (FastxReader / BamReader::subsample through vgh_reads_read_all_s: what every
host leg of vgh_sample_count_s applies) against the model, the C entries, the CLI's option parsing, and the premises of the GPU tests."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bam_py as B
import quality_mask_cases as Q
import subsample_cases as S
from conftest import GOLDEN, ROOT, get_cohort
from varigraph_amd import host, vgmi

CLI = os.path.join(ROOT, "varigraph_amd", "bin", "varigraph-mi")


def test_rule_in_cpp_equals_its_known_answers(tmp_path):
    """tests/native/subsample_check.cpp under AddressSanitizer + UBSan, a stand-alone program: subsample_keep and the threshold against the
    tables of the option's definition, read number 2^64 - 2, F = 1, and the thresholds 0 and 1"""
    exe = str(tmp_path / "subsample_check")
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-I",
                        os.path.join(ROOT, "varigraph_amd", "csrc"), os.path.join(ROOT, "tests", "native", "subsample_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("subsample rule identical"), (r.stdout[-1000:], r.stderr[-2000:])


def test_python_model_equals_the_known_answers():
    for i, row in S.KNOWN_Z.items():
        assert tuple(S.z(i, s) for s in S.KNOWN_S) == row, i
    for f, t in S.KNOWN_T.items():
        assert S.threshold(f) == t, f
    for f, (kept, first, longest) in S.KNOWN_4000.items():
        m = S.kept_mask(4000, f, 11)
        assert [bool(x) for x in m] == [S.keep(i, 11, f) for i in range(4000)]            # the vectorised form is the scalar one
        assert int(m.sum()) == kept and S.longest_dropped_run(m) == longest
        assert tuple(np.flatnonzero(m)[:len(first)]) == first
    assert S.kept_mask(100, 1.0, 11).all() and S.threshold(2.0 ** -64) == 1 and S.threshold(2.0 ** -65) == 0
    # a restart at number n is the tail of a whole pass
    assert np.array_equal(S.kept_mask(3000, 0.5, 7, first=1000), S.kept_mask(4000, 0.5, 7)[1000:])


def _block(recs):
    return b"".join(r[1] + b"\n" for r in recs)


@pytest.mark.parametrize("f", S.FRACTIONS + (1.0,))
@pytest.mark.parametrize("seed", S.SEEDS)
def test_host_fastq_reader_keeps_the_models_set(f, seed, tmp_path):
    """four-line records with CRLF and multi-line ones among them, plain and gzip: the records out are the model's kept set, a restart at
    number n gives the tail of a whole pass, and the minimum base quality applies to the kept reads only"""
    recs = S.fastq_records(n=400, seed=seed)
    for i in (3, 57, 211):
        recs[i] = recs[i] + ("crlf",)
    for i in (12, 58, 398):
        recs[i] = recs[i] + ("wrapped",)
    text = S.fastq_text(recs)
    kept = S.kept_of(recs, f, seed)
    plain, gz = tmp_path / "a.fq", tmp_path / "a.fq.gz"
    plain.write_bytes(text)
    gz.write_bytes(gzip.compress(text, 6))
    for p in (plain, gz):
        block, n, rb, mb, nxt = host.reads_read_all_s(str(p), f, seed)
        assert block.tobytes() == _block(kept)
        assert (n, rb, mb, nxt) == (len(kept), sum(len(r[1]) for r in kept), 0, len(recs))
    # G' with the option off is the same block: the oracle of the device tests
    gp = tmp_path / "gp.fq"
    gp.write_bytes(S.fastq_text(kept))
    assert host.fastx_read_all(str(gp))[0].tobytes() == _block(kept)
    # a reader that starts `first` records into the file numbers on from there
    for first in (1, 57, 399):
        tail = tmp_path / "tail.fq"
        tail.write_bytes(S.fastq_text(recs[first:]))
        block, n, _, _, nxt = host.reads_read_all_s(str(tail), f, seed, first_number=first)
        assert block.tobytes() == _block(S.kept_of(recs[first:], f, seed, first)) and nxt == len(recs)
        assert S.kept_of(recs[first:], f, seed, first) == [r for r in kept if recs.index(r) >= first]
    # with mask_below: the kept reads masked, the dropped ones not looked at
    masked, total = Q.masked_records(kept, 20)
    block, n, rb, mb, _ = host.reads_read_all_s(str(plain), f, seed, min_base_quality=20)
    assert block.tobytes() == _block(masked) and (n, mb) == (len(kept), total)
    if f < 1.0:
        assert total < Q.masked_records(recs, 20)[1]


@pytest.mark.parametrize("f", (0.5, 0.02))
def test_host_fasta_reader_keeps_the_models_set(f, tmp_path):
    recs = S.fastq_records(n=300, seed=5)
    kept = S.kept_of(recs, f, 11)
    for width in (None, 60):
        p = tmp_path / "a.fa"
        p.write_bytes(S.fasta_text(recs, width))
        block, n, rb, mb, nxt = host.reads_read_all_s(str(p), f, 11)
        assert block.tobytes() == _block(kept) and (n, nxt, mb) == (len(kept), len(recs), 0)
        block, n, _, _, nxt = host.reads_read_all_s(str(p), f, 11, first_number=1000)
        assert block.tobytes() == _block(S.kept_of(recs, f, 11, 1000)) and nxt == 1000 + len(recs)


@pytest.mark.parametrize("f", S.FRACTIONS + (1.0,))
@pytest.mark.parametrize("seed", S.SEEDS)
def test_host_bam_reader_numbers_the_reads_not_the_records(f, seed, tmp_path):
    """secondary, supplementary and SEQ '*' records between the reads: a read's number is its rank among the reads"""
    recs = S.bam_records(n=300, seed=seed)
    n_reads = sum(1 for r in recs if r.kept)
    assert n_reads == 300 and len(recs) == 450
    gp, seen = S.bam_filtered(recs, f, seed)
    want_block, n_kept, want_rb = B.reads_block(gp)
    p = tmp_path / "a.bam"
    B.write_bam(p, recs)
    block, n, rb, mb, nxt = host.reads_read_all_s(str(p), f, seed)
    assert block.tobytes() == want_block and (n, rb, mb, nxt) == (n_kept, want_rb, 0, seen) and seen == n_reads
    if f < 1.0:
        # numbering the records instead would keep another set
        by_record = [r for i, r in enumerate(recs) if r.kept and S.keep(i, seed, f)]
        assert B.reads_block(by_record)[0] != want_block
    # restart: the reader takes over at record 200 of the file, whose reads start at number `first`
    first = sum(1 for r in recs[:200] if r.kept)
    B.write_bam(p, recs[200:])
    block, n, _, _, nxt = host.reads_read_all_s(str(p), f, seed, first_number=first)
    assert block.tobytes() == B.reads_block(S.bam_filtered(recs[200:], f, seed, first)[0])[0] and nxt == n_reads
    # with mask_below
    B.write_bam(p, recs)
    masked, total = Q.masked_bam_records(gp, 20)
    block, n, _, mb, _ = host.reads_read_all_s(str(p), f, seed, min_base_quality=20)
    assert block.tobytes() == B.reads_block(masked)[0] and mb == total


def test_bad_fractions_are_refused_by_the_host_entry(tmp_path):
    p = tmp_path / "a.fq"
    p.write_bytes(b"@r\nACGT\n+\nIIII\n")
    for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="0 < fraction <= 1"):
            host.reads_read_all_s(str(p), bad, 11)
    assert host.reads_read_all_s(str(p), 1.0, 11)[1] == 1
    assert host.reads_read_all_s(str(p), 2.0 ** -65, 11)[1] == 0         # T = 0 keeps nothing


def test_new_entries_are_declared_and_exported():
    for header, libpath, names in (("vgmi.h", vgmi.LIB_PATH, ("vgmi_fastq_set_subsample", "vgmi_fastq_subsample_stats")),
                                   ("vghost.h", host.LIB_PATH, ("vgh_sample_count_s", "vgh_reads_read_all_s"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
        for name in names:
            assert re.search(r"\b%s\s*\(" % name, txt), name
            assert re.search(r" T %s$" % name, out, flags=re.M), name
    vgmi.lib()
    assert {"vgmi_fastq_set_subsample", "vgmi_fastq_subsample_stats"} <= set(vgmi.SYMBOLS)
    # the driver class of before keeps its constructor symbol: a program built against the earlier header runs against this library
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", host.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T vgh::FastqKmerHip::FastqKmerHip\(vgmi_ctx\*, std::vector<.*> const&, unsigned int, unsigned int, unsigned long\)$", out, flags=re.M)
    assert " T vgh::FastqKmerHip::build_fastq_index()" in out


def test_cli_help_names_the_options_and_refuses_bad_values(tmp_path):
    r = subprocess.run([CLI, "genotype", "-h"], capture_output=True, text=True)
    assert "--subsample " in r.stderr + r.stdout and "--subsample-seed" in r.stderr + r.stdout and "interleaved BAM" in r.stderr + r.stdout
    graph = os.path.join(tmp_path, "graph.bin")
    open(graph, "wb").write(gzip.open(os.path.join(GOLDEN, "cohort_snp", "graph.bin.gz"), "rb").read())
    open(os.path.join(tmp_path, "s.cfg"), "w").write("sample0 " + os.path.join(GOLDEN, "cohort_snp", "reads_1.fq.gz") + "\n")
    base = [CLI, "genotype", "--load-graph", graph, "-s", "s.cfg"]
    for opt, bad, what in (("--subsample", "abc", "is not a number"), ("--subsample", "0.5x", "is not a number"), ("--subsample", "0", "greater than 0 and at most 1"),
                           ("--subsample", "-0.5", "greater than 0 and at most 1"), ("--subsample", "1.5", "greater than 0 and at most 1"),
                           ("--subsample", "nan", "greater than 0 and at most 1"), ("--subsample-seed", "-1", "is not a non-negative integer"),
                           ("--subsample-seed", "x", "is not a non-negative integer")):
        r = subprocess.run(base + [opt, bad], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and "Parameter error: " + opt + "." in r.stderr and what in r.stderr, (opt, bad, r.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".vcf.gz")]


def test_premises_of_the_gpu_tests():
    """what test_gpu_subsample.py relies on, checked where no GPU time is spent: at F = 0.5 the model keeps between 30 % and 70 % of each
    case's reads, at F = 0.02 at least one; the two long records of the FASTQ case are one kept and one dropped; the cuts end a chunk
    behind a kept and behind a dropped record; reads drawn from the committed cohort hit its graph, so dropping them changes counters"""
    cohort = get_cohort("cohort_snp")
    haps = cohort.haplotypes()
    for seed in S.SEEDS:
        la = S.long_positions(seed, 600)
        assert S.keep(la[0], seed, 0.5) and not S.keep(la[1], seed, 0.5)
        recs = S.fastq_records(haps, 600, seed, la)
        assert len(recs[la[0]][1]) == len(recs[la[1]][1]) == S.LONG
        cases = {"fastq": 600, "fasta": 300, "bam": 300, "cohort": cohort.n_reads // 2}
        for name, n in cases.items():
            assert 0.3 * n <= S.kept_mask(n, 0.5, seed).sum() <= 0.7 * n, (name, seed)
            assert S.kept_mask(n, 0.02, seed).sum() >= 1, (name, seed)
            assert S.kept_mask(n, 0.9, seed).sum() < n, (name, seed)
        # at F = 0.02 most 4 KiB chunks (a dozen records) keep nothing
        assert S.longest_dropped_run(S.kept_mask(600, 0.02, seed)) > 40
        kept = S.kept_of(recs, 0.5, seed)
        assert sum(Q.windows(r[1], cohort.k) for r in kept) < sum(Q.windows(r[1], cohort.k) for r in recs)
