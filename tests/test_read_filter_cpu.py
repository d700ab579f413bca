"""The read filter by length and read quality without a device: the rule in C++ (tests/native/read_filter_check.cpp, a stand-alone
program under ASan + UBSan) against the Python model of read_filter_cases.py -- verdict, class and both sums per record, and the 931
table entries --, five mutated rules that must each change a verdict on the case set, both host readers through vgh_reads_read_all_l,
the text-to-tenths parser, the symbols, the CLI's parameter errors, and the premises of the GPU tests."""
import gzip
import os
import re
import subprocess

import pytest

import bam_py as B
import quality_mask_cases as Q
import read_filter_cases as R
import subsample_cases as S
from conftest import GOLDEN, ROOT
from varigraph_amd import host, synth, vgmi

CLI = os.path.join(ROOT, "varigraph_amd", "bin", "varigraph-mi")
HEADER = os.path.join(ROOT, "varigraph_amd", "csrc", "vgmi_read_filter.h")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rf") / "read_filter_check")
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-I",
                        os.path.join(ROOT, "varigraph_amd", "csrc"), os.path.join(ROOT, "tests", "native", "read_filter_check.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def cases():
    return R.fastq_records(None, 600, 3), R.bam_records(None, 300, 3)


def test_table_in_the_header_equals_the_decimal_one(exe):
    r = subprocess.run([exe, "table"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == 931 and got == R.E10
    assert got[0] == 2 ** 30 and got[100] == 107374182 and got[930] == round(2 ** 30 * 10 ** -9.3)
    # the committed generator agrees with the header it wrote
    r = subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_read_filter_table.py"), "--check", HEADER], capture_output=True, text=True)
    assert r.returncode == 0 and "931 entries" in r.stdout, r.stderr
    # no floating point in the rule's header: the verdicts are integer arithmetic
    code = re.sub(r"//[^\n]*", "", open(HEADER).read())
    assert not re.search(r"\b(double|float|pow|exp|log)\b", code)


def _classify(exe, tmp_path, rule, items):
    p = tmp_path / "in.txt"
    p.write_text(R.check_file_lines(rule, items))
    r = subprocess.run([exe, "classify", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    return [tuple(int(x) for x in ln.split()) for ln in lines[:-1]], lines[-1]


@pytest.mark.parametrize("name", list(R.RULES))
def test_rule_in_cpp_equals_the_model(name, exe, cases, tmp_path):
    rule = R.RULES[name]
    fq, bam = cases
    items = [("F", r[2]) for r in fq] + [("B", r.qual) for r in bam if r.kept] + [("N", len(r[1])) for r in fq[:40]] + [("N", 0), ("F", b""), ("B", b"")]
    want = [rule.classify(len(r[2]), r[2]) for r in fq] + [rule.classify(len(r.seq), r.qual, bam=True) for r in bam if r.kept] + \
           [rule.classify(len(r[1])) for r in fq[:40]] + [rule.classify(0), rule.classify(0, b""), rule.classify(0, b"", bam=True)]
    got, last = _classify(exe, tmp_path, rule, items)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, i, items[i][0], g, w)
    assert last == "evaluated %d kept %d" % (len(want), sum(1 for w in want if w[0] == R.PASS))


def test_case_set_fills_every_class_and_a_third_pass(cases):
    fq, bam = cases
    for what, classes in (("fastq", R.fastq_classes(fq, R.ALL)), ("bam", [R.bam_class(r, R.ALL) for r in bam if r.kept])):
        counts = R.class_counts(classes)
        print(what, dict(zip(("evaluated",) + R.CLASS_NAMES[1:], counts)))
        assert all(c > 0 for c in counts), (what, counts)
        assert 3 * (counts[0] - sum(counts[1:])) >= counts[0], (what, counts)
    named = {r[0]: R.ALL.classify(len(r[1]), r[2]) for r in fq}
    u = R.E10[R.MEAN_Q]
    assert named[b"len%d" % (R.MIN_LEN - 1)][0] == R.SHORT and named[b"len%d" % R.MIN_LEN][0] == R.PASS and named[b"len1"][0] == R.SHORT
    assert [named[b"len%d" % n][0] for n in (63, 64, 65)] == [R.PASS] * 3
    assert named[b"uniform"] == (R.PASS, 0, 100 * u)                                   # equality passes
    assert named[b"uniform_one_lower"] == (R.LOW_MEAN, 1, 99 * u + R.E10[R.MEAN_Q - 10])
    assert named[b"phred_mean_passes"][0] == R.LOW_MEAN and (90 * 40 + 10 * 2) * 10 >= R.MEAN_Q * 100
    assert named[b"fraction_equal"][:2] == (R.PASS, 40) and named[b"fraction_one_more"][:2] == (R.LOW_FRACTION, 41)
    assert named[b"fraction_half_percent"][:2] == (R.LOW_FRACTION, 81)
    assert named[b"bang_tilde"] == (R.PASS, 3, 3 * 2 ** 30 + 97 * R.E10[930])
    assert named[b"below33_above126"] == (R.PASS, 3, 3 * 2 ** 30 + 3 * R.E10[930] + 94 * R.E10[400])
    assert named[b"all_bang"][0] == R.LOW_FRACTION and R.RULES["mean"].cls(64, b"!" * 64) == R.LOW_MEAN      # fails two: the first is its class
    assert named[b"short_and_low"] == (R.SHORT, 0, 0)
    assert named[b"max_len_plus_1"][0] == R.LONG_ and named[b"long_kept"][0] == R.PASS and named[b"long_dropped"][0] == R.LOW_MEAN
    assert len(fq[600 // 4][1]) == len(fq[600 // 2][1]) == R.LONG == R.MAX_LEN
    bnamed = {r.name: R.ALL.classify(len(r.seq), r.qual, bam=True) for r in bam if r.kept}
    assert bnamed[b"qual_0_93_94_254"] == (R.PASS, 3, 3 * 2 ** 30 + 30 * R.E10[930] + 67 * R.E10[400])
    assert bnamed[b"qual_254_low_half"][:2] == (R.LOW_FRACTION, 41)
    assert bnamed[b"no_qual"] == (R.PASS, 0, 0) and bnamed[b"no_qual_short"] == (R.SHORT, 0, 0)
    assert R.RULES["mean"].cls(77, b"\xff" + bytes(76), bam=True) == R.PASS and R.RULES["mean"].cls(77, bytes(77), bam=True) == R.LOW_MEAN
    assert bnamed[b"long_20000"][0] == R.PASS and bnamed[b"long_20001"][0] == R.LONG_


@pytest.mark.parametrize("mutation", R.MUTATIONS, ids=[m.__name__ for m in R.MUTATIONS])
def test_a_mutated_rule_changes_a_verdict(mutation, cases):
    fq, bam = cases
    m = mutation(R.MIN_LEN, R.MAX_LEN, R.MEAN_Q, R.LOW_Q, R.LOW_PCT)
    changed = [r[0] for r in fq if (m.cls(len(r[1]), r[2]) == R.PASS) != (R.ALL.cls(len(r[1]), r[2]) == R.PASS)]
    changed += [r.name for r in bam if r.kept and (m.cls(len(r.seq), r.qual, bam=True) == R.PASS) != (R.bam_class(r, R.ALL) == R.PASS)]
    print(mutation.__name__, "changes", changed[:8])
    assert changed


# ---- the host readers ------------------------------------------------------------------------------------------------------------------
def _block(recs):
    return b"".join(r[1] + b"\n" for r in recs)


def _bgzf(tmp_path, name, data):
    src, dst = tmp_path / (name + ".txt"), tmp_path / (name + ".bgz.gz")
    src.write_bytes(data)
    synth.bgzf_compress_file(str(src), str(dst), level=4, block=3000)
    return dst


@pytest.mark.parametrize("name", list(R.RULES))
def test_host_fastq_reader_keeps_the_models_set(name, cases, tmp_path):
    """plain, gzip and block gzip, wrapped and CRLF records among the four-line ones; with subsampling the numbers do not change and only
    the kept reads are evaluated; with a minimum base quality the tests see the file's own qualities"""
    rule = R.RULES[name]
    recs = list(cases[0])
    for i in (40, 57, 211):
        recs[i] = recs[i] + ("crlf",)
    for i in (45, 58, 598):
        recs[i] = recs[i] + ("wrapped",)
    text = R.fastq_text(recs)
    kept, classes = R.fastq_filtered(recs, rule)
    files = {"plain": tmp_path / "a.fq", "gzip": tmp_path / "a.fq.gz"}
    files["plain"].write_bytes(text)
    files["gzip"].write_bytes(gzip.compress(text, 6))
    files["bgzf"] = _bgzf(tmp_path, "a", text)
    for kind, p in files.items():
        block, n, rb, mb, nxt, _, _, stats = host.reads_read_all_l(str(p), rule.dict(), decode_threads=2)
        assert block.tobytes() == _block(kept), kind
        assert (n, rb, mb, nxt) == (len(kept), sum(len(r[1]) for r in kept), 0, len(recs)), kind
        assert stats == R.class_counts(classes), kind
    # G' with the option off is the same block: the oracle of the device tests
    gp = tmp_path / "gp.fq"
    gp.write_bytes(R.fastq_text(kept))
    assert host.fastx_read_all(str(gp))[0].tobytes() == _block(kept)
    # with subsampling: the rule behind it, on the reads it kept
    for sub in ((0.5, 11), (0.5, 7)):
        skept, sclasses = R.fastq_filtered(recs, rule, sub)
        block, n, _, _, nxt, _, _, stats = host.reads_read_all_l(str(files["plain"]), rule.dict(), fraction=sub[0], seed=sub[1])
        assert block.tobytes() == _block(skept) and nxt == len(recs)
        assert stats == R.class_counts(sclasses) and stats[0] == int(S.kept_mask(len(recs), *sub).sum())
        assert set(r[0] for r in skept) == set(r[0] for r in kept) & set(r[0] for r in S.kept_of(recs, *sub))
    # a reader that takes the file over `first` records in
    first = 300
    tail = tmp_path / "tail.fq"
    tail.write_bytes(R.fastq_text(recs[first:]))
    tkept, tclasses = R.fastq_filtered(recs[first:], rule, (0.5, 11), first)
    block, _, _, _, nxt, _, _, stats = host.reads_read_all_l(str(tail), rule.dict(), fraction=0.5, seed=11, first_number=first)
    assert block.tobytes() == _block(tkept) and nxt == len(recs) and stats == R.class_counts(tclasses)
    # with mask_below: the kept reads masked, the verdicts those of the unmasked qualities
    masked, total = Q.masked_records(kept, 20)
    block, n, _, mb, _, _, _, stats = host.reads_read_all_l(str(files["plain"]), rule.dict(), min_base_quality=20)
    assert block.tobytes() == _block(masked) and (n, mb) == (len(kept), total) and stats == R.class_counts(classes)


def test_all_default_rule_and_none_are_the_reader_of_before(cases, tmp_path):
    recs = cases[0]
    p = tmp_path / "a.fq"
    p.write_bytes(R.fastq_text(recs))
    want = host.reads_read_all_r(str(p))
    for rf in (None, {}, R.Rule().dict()):
        got = host.reads_read_all_l(str(p), rf)
        assert got[0].tobytes() == want[0].tobytes() and got[1:7] == want[1:] and got[7] == (len(recs), 0, 0, 0, 0)


def test_host_fasta_reader_applies_the_lengths_alone(cases, tmp_path):
    recs = cases[0]
    for width in (None, 60):
        p = tmp_path / "a.fa"
        p.write_bytes(S.fasta_text(recs, width))
        for name in ("lengths", "all", "mean", "fraction"):
            rule = R.RULES[name]
            kept, classes = R.fasta_filtered(recs, rule)
            block, n, _, _, _, _, _, stats = host.reads_read_all_l(str(p), rule.dict())
            assert block.tobytes() == _block(kept) and n == len(kept) and stats == R.class_counts(classes), (width, name)
            assert stats[3] == stats[4] == 0
            if name in ("mean", "fraction"):
                assert n == len(recs)
            else:
                assert 0 < stats[1] and 0 < stats[2] and n < len(recs)


@pytest.mark.parametrize("name", list(R.RULES))
def test_host_bam_reader_keeps_the_models_set(name, cases, tmp_path):
    rule = R.RULES[name]
    recs = cases[1]
    gp, classes, n_reads = R.bam_filtered(recs, rule)
    want_block, n_kept, want_rb = B.reads_block(gp)
    p = tmp_path / "a.bam"
    B.write_bam(p, recs)
    block, n, rb, mb, nxt, _, _, stats = host.reads_read_all_l(str(p), rule.dict())
    assert block.tobytes() == want_block and (n, rb, mb, nxt) == (n_kept, want_rb, 0, n_reads)
    assert stats == R.class_counts(classes) and stats[0] == n_reads == 300
    for sub in ((0.5, 11), (0.5, 7)):
        sgp, sclasses, seen = R.bam_filtered(recs, rule, sub)
        block, n, _, _, nxt, _, _, stats = host.reads_read_all_l(str(p), rule.dict(), fraction=sub[0], seed=sub[1])
        assert block.tobytes() == B.reads_block(sgp)[0] and nxt == seen == n_reads and stats == R.class_counts(sclasses)
    # with a flag filter in front: the records it drops are not evaluated
    f = dict(exclude=0x910)
    fgp, fclasses, _ = R.bam_filtered([r for r in recs if not r.flag & 0x10], rule)
    block, n, _, _, _, _, _, stats = host.reads_read_all_l(str(p), rule.dict(), bam_filter=f)
    assert block.tobytes() == B.reads_block(fgp)[0] and stats == R.class_counts(fclasses)
    # with mask_below
    masked, total = Q.masked_bam_records(gp, 20)
    block, n, _, mb, _, _, _, stats = host.reads_read_all_l(str(p), rule.dict(), min_base_quality=20)
    assert block.tobytes() == B.reads_block(masked)[0] and mb == total and stats == R.class_counts(classes)


def test_fields_out_of_range_are_refused_each_with_its_message(tmp_path):
    p = tmp_path / "a.fq"
    p.write_bytes(b"@r\nACGT\n+\nIIII\n")
    for bad, what in ((dict(min_len=10, max_len=9), "below the minimum read length"), (dict(min_mean_q=931), "0..930"),
                      (dict(lowq_below=94, lowq_max_pct=10), "0..93, Phred"), (dict(lowq_below=10, lowq_max_pct=101), "0..100"),
                      (dict(lowq_max_pct=10), "needs a low-quality bound")):
        with pytest.raises(RuntimeError, match=re.escape(what)):
            host.reads_read_all_l(str(p), bad)
    assert host.reads_read_all_l(str(p), dict(min_len=4, max_len=4, min_mean_q=930, lowq_below=93, lowq_max_pct=100))[1] == 0      # 'I' is Q40 < 93
    assert host.reads_read_all_l(str(p), dict(min_len=4, max_len=4, min_mean_q=400, lowq_below=40, lowq_max_pct=0))[1] == 1


def test_text_to_tenths(exe):
    texts = ["7", "7.5", "07.50", "93.1", "-1", "0", "93", "93.0", "0.1", "7.", ".5", "7.55", "1e1", "+7", " 7", "7 ", "", "100", "00", "9.x"]
    want = [70, 75, None, None, None, 0, 930, 930, 1, None, None, None, None, None, None, None, None, None, None, None]
    r = subprocess.run([exe, "tenths"] + texts, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [None if x == "refused" else int(x) for x in r.stdout.split()] == want
    for t, w in zip(texts, want):
        if w is None:
            with pytest.raises(ValueError):
                host.parse_quality_tenths(t)
        else:
            assert host.parse_quality_tenths(t) == w


def test_new_entries_are_declared_and_exported():
    for header, libpath, names in (("vgmi.h", vgmi.LIB_PATH, ("vgmi_fastq_set_read_filter", "vgmi_fastq_read_filter_stats")),
                                   ("vghost.h", host.LIB_PATH, ("vgh_sample_count_l", "vgh_reads_read_all_l", "vgh_parse_quality_tenths"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
        for name in names:
            assert re.search(r"\b%s\s*\(" % name, txt), name
            assert re.search(r" T %s$" % name, out, flags=re.M), name
    vgmi.lib()
    assert {"vgmi_fastq_set_read_filter", "vgmi_fastq_read_filter_stats"} <= set(vgmi.SYMBOLS)
    # the new kernels are in the device library's code object under their own names
    out = subprocess.run(["strings", "-a", vgmi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for k in ("fq_records_rf_kernel", "fq_read_quality_kernel", "fq_finish_rf_kernel", "bam_read_filter_kernel", "bam_finish_rf_kernel"):
        assert k in out, k
    # the driver class of before keeps its constructor symbol: a program built against the earlier header runs against this library
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", host.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T vgh::FastqKmerHip::FastqKmerHip\(vgmi_ctx\*, std::vector<.*> const&, unsigned int, unsigned int, unsigned long\)$", out, flags=re.M)
    assert " T vgh::FastqKmerHip::build_fastq_index()" in out and "vgh::FastqKmerHipL::FastqKmerHipL(" in out


def test_cli_help_names_the_options_and_refuses_bad_values(tmp_path):
    r = subprocess.run([CLI, "genotype", "-h"], capture_output=True, text=True)
    text = r.stderr + r.stdout
    for opt in ("--min-read-length", "--max-read-length", "--min-read-quality", "--max-low-quality"):
        assert opt in text, opt
    assert "one mate of a pair" in text
    graph = os.path.join(tmp_path, "graph.bin")
    open(graph, "wb").write(gzip.open(os.path.join(GOLDEN, "cohort_snp", "graph.bin.gz"), "rb").read())
    open(os.path.join(tmp_path, "s.cfg"), "w").write("sample0 " + os.path.join(GOLDEN, "cohort_snp", "reads_1.fq.gz") + "\n")
    base = [CLI, "genotype", "--load-graph", graph, "-s", "s.cfg"]
    for opts, opt, what in ((["--min-read-length", "x"], "--min-read-length", "is not a non-negative integer"),
                            (["--min-read-length", "-1"], "--min-read-length", "is not a non-negative integer"),
                            (["--max-read-length", "4294967296"], "--max-read-length", "between 0 and 4294967295"),
                            (["--min-read-length", "100", "--max-read-length", "99"], "--max-read-length", "must not be below --min-read-length"),
                            (["--min-read-quality", "07.50"], "--min-read-quality", "between 0 and 93 (inclusive), with at most one fractional digit"),
                            (["--min-read-quality", "93.1"], "--min-read-quality", "between 0 and 93"),
                            (["--min-read-quality", "-1"], "--min-read-quality", "between 0 and 93"),
                            (["--min-read-quality", "7.55"], "--min-read-quality", "between 0 and 93"),
                            (["--max-low-quality", "15"], "--max-low-quality", "Expected Q:PCT"),
                            (["--max-low-quality", "0:40"], "--max-low-quality", "between 1 and 93"),
                            (["--max-low-quality", "94:40"], "--max-low-quality", "between 1 and 93"),
                            (["--max-low-quality", "15:101"], "--max-low-quality", "between 0 and 100"),
                            (["--max-low-quality", "15:x"], "--max-low-quality", "is not a non-negative integer")):
        r = subprocess.run(base + opts, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and "Parameter error: " + opt + "." in r.stderr and what in r.stderr, (opts, r.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".vcf.gz")]
