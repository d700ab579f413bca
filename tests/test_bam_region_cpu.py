"""The BAM region test without a device: the rule of csrc/vgmi_bam_filter.h in a stand-alone program under ASan + UBSan against the
Python model of bam_region_cases.py -- the whole rule's verdict per record, the binary-search form against the plain definition,
the normaliser's output, the refusals; mutated rules change verdicts on the case set; the host decoder's form (BamReader through
vgh_reads_read_all_r: what every host leg of vgh_sample_count_r applies) with a list, a BED file and unplaced reads; the region
grammar; the entries declared and exported; the CLI's options."""
import gzip
import os
import re
import subprocess

import pytest

import bam_filter_cases as F
import bam_py as B
import bam_region_cases as R
import quality_mask_cases as Q
import subsample_cases as S
from conftest import GOLDEN, ROOT
from varigraph_amd import host, vgmi

CLI = os.path.join(ROOT, "varigraph_amd", "bin", "varigraph-mi")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """tests/native/bam_region_check.cpp under AddressSanitizer + UBSan -> run(raws, regions, unplaced, filter, n_ref) =
    ("invalid", code) | (normalised list, [(verdict, shortcut, plain)])"""
    d = tmp_path_factory.mktemp("bam_region_check")
    exe = str(d / "bam_region_check")
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-I",
                        os.path.join(ROOT, "varigraph_amd", "csrc"), os.path.join(ROOT, "tests", "native", "bam_region_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(raws, regions, unplaced=False, f=F.Filter(), n_ref=len(R.REFS)):
        p, q = d / "records.bin", d / "regions.txt"
        p.write_bytes(b"".join(raws))
        q.write_text("".join("%d %d %d\n" % t for t in regions))
        r = subprocess.run([exe, str(p), str(q), str(n_ref), str(int(unplaced)), str(f.exclude), str(f.require), str(f.min_mapq),
                            f.tag.decode() if f.tag else "-", repr(float(f.min_value))], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
        lines = r.stdout.split("\n")[:-1]
        if lines[0].startswith("invalid"):
            return "invalid", int(lines[0].split()[1])
        n = int(lines[0].split()[1])
        norm = [tuple(int(x) for x in ln.split()) for ln in lines[1:1 + n]]
        out = [tuple(int(x) for x in ln.split()) for ln in lines[1 + n:]]
        assert len(out) == len(raws)
        return norm, out
    return run


def _same(got, raws, f, regions, unplaced):
    for i, ((v, fast, slow), raw) in enumerate(zip(got, raws)):
        want = R.overlaps(raw, regions, unplaced)
        assert fast == slow == int(want), (i, fast, slow, want, R.placement(raw))
        assert v == R.verdict_raw(raw, f, regions, unplaced), (i, v, R.placement(raw))


def test_case_set_has_every_class_and_both_verdicts(check):
    cs = R.cases()
    raws = [R.record(r) for _, r in cs]
    for unplaced in (False, True):
        norm, got = check(raws, R.CASE_REGIONS, unplaced)
        assert norm == R.normalise(R.CASE_REGIONS) and len(norm) == 5
        _same(got, raws, F.Filter(), R.CASE_REGIONS, unplaced)
    by_class = {}
    for (cls, _), raw in zip(cs, raws):
        by_class.setdefault(cls, []).append(R.overlaps(raw, R.CASE_REGIONS, False))
    want = {"pos_end_minus_1": [True], "pos_end": [False], "endpos_beg": [False], "endpos_beg_plus_1": [True], "inside": [True, True],
            "gap": [False, False], "span_gap": [True], "swallow": [True, True], "code_9": [False], "unplaced": [False, False],
            "pos_minus_1": [False, False], "highest_ref": [True, True], "other_ref": [False], "unwalkable_outside": [False, False]}
    for cls, verdicts in want.items():
        assert by_class[cls] == verdicts, cls
    for cls in R.CLASSES_BOTH_VERDICTS:
        assert True in by_class[cls] and False in by_class[cls], cls
    assert by_class["sum_wraps_32"] == [True, True, False] and by_class["pos_max"] == [True, False]
    assert set(by_class) >= set(want) | set(R.CLASSES_BOTH_VERDICTS) | {"with_flags", "with_mapq", "with_tag"}
    # unplaced records pass with the bit alone
    assert [R.overlaps(raw, R.CASE_REGIONS, True) for (cls, _), raw in zip(cs, raws) if cls == "unplaced"] == [True, True]


def test_case_set_with_the_other_conditions(check):
    """the flag, MAPQ and tag tests around the region test; a record the regions drop is never walked, one they keep is"""
    cs = R.cases()
    raws = [R.record(r) for _, r in cs]
    f = R.CASE_FILTER
    _, got = check(raws, R.CASE_REGIONS, True, f)
    _same(got, raws, f, R.CASE_REGIONS, True)
    v = {}
    for (cls, _), (r, _, _) in zip(cs, got):
        v.setdefault(cls, []).append(r)
    assert v["with_flags"] == [0, 0, 0] and v["with_mapq"] == [0, 1] and v["with_tag"] == [1, 0, 0]
    assert v["unwalkable_outside"] == [0, -1]      # outside the regions: not walked; unplaced and kept: walked, a fault
    _, got = check(raws, R.CASE_REGIONS, False, f)
    assert [r for (cls, _), (r, _, _) in zip(cs, got) if cls == "unwalkable_outside"] == [0, 0]
    assert not any(r == -1 for r, _, _ in got)
    # without regions the same records fault: the order of the conditions is what spares them
    _, got = check(raws, [], False, f)
    assert [r for (cls, _), (r, _, _) in zip(cs, got) if cls == "unwalkable_outside"] == [-1, -1]


@pytest.mark.parametrize("several", (False, True))
@pytest.mark.parametrize("n", R.LIST_SIZES)
def test_binary_search_at_every_list_size(n, several, check):
    regions = R.interval_list(n, several)
    span = 100 * (n // (len(R.REFS) if several else 1) + 2)
    raws = [R.record(r) for r in R.drawn(600, span=span, seed=40 + n)]
    norm, got = check(raws, regions, n % 2 == 1, F.Filter(exclude=0))
    assert norm == R.normalise(regions) and len(norm) == n
    _same(got, raws, F.Filter(exclude=0), regions, n % 2 == 1)
    kept = sum(f for _, f, _ in got)
    assert 0 < kept < len(raws)
    # records at every interval's edges: the last base in front, the first and last inside, the first behind
    d = F.Draw(n)
    edge = []
    for ref, beg, end in norm[:300] + norm[-10:]:
        for pos, cig in ((beg - 1, [(1, "M")]), (beg - 2, [(2, "M")]), (beg - 2, [(3, "M")]), (beg, []), (end - 1, []), (end, [(5, "M")])):
            edge.append(d.rec(20, flag=0, ref=ref, pos=pos, cigar=cig))
    raws = [R.record(r) for r in edge]
    _, got = check(raws, regions)
    _same(got, raws, F.Filter(), regions, False)
    assert [f for _, f, _ in got[:6]] == [0, 0, 1, 1, 1, 0]


def test_normaliser_and_refusals(check):
    raw = [R.record(F.Draw(1).rec(flag=0, ref=0, pos=5))]
    messy = [(2, 50, 60), (0, 10, 20), (0, 20, 30), (0, 5, 12), (0, 40, 41), (0, 0, 1), (2, 55, 70), (2, 70, 71), (1, 0, R.WHOLE), (1, 7, 9),
             (0, 41, 42)]
    norm, _ = check(raw, messy)
    assert norm == R.normalise(messy) == [(0, 0, 1), (0, 5, 30), (0, 40, 42), (1, 0, R.WHOLE), (2, 50, 71)]
    for bad, code in (([(4, 0, 1)], 1), ([(-1, 0, 1)], 1), ([(0, -1, 5)], 2), ([(0, R.WHOLE, R.WHOLE + 1)], 2), ([(0, 5, 5)], 3), ([(0, 5, 4)], 3),
                      ([(0, 5, R.WHOLE + 1)], 3)):
        assert check(raw, bad) == ("invalid", code), bad
    assert check(raw, [], True) == ("invalid", 4)
    assert check(raw, [(0, R.WHOLE - 1, R.WHOLE)])[0] == [(0, R.WHOLE - 1, R.WHOLE)]
    norm, got = check(raw, [])
    assert norm == [] and got == [(1, 0, 0)]      # no list: no region test in the rule


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_mutated_rules_change_a_verdict(mutate):
    raws = [R.record(r) for _, r in R.cases()]
    true = [R.overlaps(raw, R.CASE_REGIONS, False) for raw in raws]
    assert true != [R.overlaps(raw, R.CASE_REGIONS, False, mutate=mutate) for raw in raws], mutate


# ---- the host decoder ----------------------------------------------------------------------------------------------------------------
LIST = "chr1:101-200,chr1:301-400,chr1:1001-1100,chr2:2147483639-2147483648,chrLast"      # CASE_REGIONS, 1-based inclusive


def _bam(tmp_path, recs):
    p = tmp_path / "a.bam"
    R.write_bam(p, recs)
    return str(p)


def _expect(recs, f, regions, unplaced):
    passing, n_rec, n_reads, at = R.apply(recs, f, regions, unplaced)
    assert at is None
    return B.reads_block(passing) + (n_rec, n_reads)


@pytest.mark.parametrize("unplaced", (False, True))
def test_host_reader_applies_the_regions(unplaced, tmp_path):
    recs = [r for cls, r in R.cases() if cls != "unwalkable_outside"] + R.drawn(400)
    p = _bam(tmp_path, recs)
    for f in (F.Filter(), F.Filter(exclude=0xF00, min_mapq=20, tag=b"qs", min_value=10)):
        recs_f = recs if f.tag is None else [r for r in recs if r.aux]
        if f.tag is not None:
            p = _bam(tmp_path, recs_f)
        want, n, rb, n_rec, n_reads = _expect(recs_f, f, R.CASE_REGIONS, unplaced)
        block, cnt, read_base, mb, nxt, records, reads = host.reads_read_all_r(p, LIST, bam_unplaced=unplaced, bam_filter=f.dict())
        assert block.tobytes() == want and (cnt, read_base, records, reads) == (n, rb, n_rec, n_reads)
        assert 0 < n < sum(1 for r in recs_f if r.kept)


def test_host_reader_bed_file_and_both_options_joined(tmp_path):
    recs = [r for cls, r in R.cases() if cls != "unwalkable_outside"] + R.drawn(300)
    p = _bam(tmp_path, recs)
    bed = tmp_path / "t.bed"
    bed.write_text("# a comment\ntrack name=x\nbrowser position chr1:1-2\n\nchr1\t100\t200\textra\t0\t+\nchrUn_1\t5\t9\nchr1 300 400\n"
                   "chr2\t2147483638\t2147483648\r\nchrUn_2\t1\t2\n")
    want, n, rb, n_rec, n_reads = _expect(recs, F.Filter(), [t for t in R.CASE_REGIONS if t[0] in (0, 1) and t[1] != 1000], False)
    block, cnt, read_base, _, _, records, reads = host.reads_read_all_r(p, None, str(bed))
    assert block.tobytes() == want and (cnt, read_base, records, reads) == (n, rb, n_rec, n_reads) and n > 0
    want, n, rb, n_rec, n_reads = _expect(recs, F.Filter(), R.CASE_REGIONS, True)
    block, cnt, read_base, _, _, records, reads = host.reads_read_all_r(p, "chr1:1001-1100,chrLast", str(bed), True)
    assert block.tobytes() == want and (cnt, read_base, records, reads) == (n, rb, n_rec, n_reads)
    for text, what in (("chr1\t5\t5\n", "line 1"), ("chr1\t1\t2\nchr1\tx\t9\n", "line 2"), ("#c\nchr1\t9\n", "line 2"), ("chr1\t-1\t4\n", "line 1")):
        bed.write_text(text)
        with pytest.raises(RuntimeError, match=what):
            host.reads_read_all_r(p, None, str(bed))
    bed.write_text("chrUn\t1\t5\n")
    with pytest.raises(RuntimeError, match="names a reference of the header"):
        host.reads_read_all_r(p, None, str(bed))
    with pytest.raises(RuntimeError, match="No such file"):
        host.reads_read_all_r(p, None, str(tmp_path / "none.bed"))


def test_region_grammar(tmp_path):
    d = F.Draw(7)
    hla = 2
    recs = [d.rec(flag=0, ref=hla, pos=p, cigar=[(10, "M")]) for p in (0, 89, 90, 99, 100, 2000)] + [d.rec(flag=0, ref=0, pos=0, cigar=[(5, "M")])]
    p = _bam(tmp_path, recs)

    def kept(regions):
        return host.reads_read_all_r(p, regions)[1]
    assert kept("HLA-A*01:01:01:01") == 6                       # a name with colons, as a whole
    assert kept("HLA-A*01:01:01:01:100") == 4                   # NAME:BEG, to the end: [99, 2^31) meets pos 90 (endpos 100), 99, 100, 2000
    assert kept("HLA-A*01:01:01:01:100-100") == 2               # pos 90 and pos 99
    assert kept("HLA-A*01:01:01:01:1-1,chr1:5") == 2
    assert kept(["chr1:6", "chr2"]) == 0
    assert kept("chr1,,chr1:1-3,") == 1                         # empty items are passed over
    with pytest.raises(RuntimeError) as e:
        kept("chr1,chrX:5-9")
    assert str(e.value) == f"'{p}': reference 'chrX' of region 'chrX:5-9' is not in the header"
    with pytest.raises(RuntimeError) as e:
        kept("HLA-A*01:01:01")
    assert str(e.value) == f"'{p}': reference 'HLA-A*01:01' of region 'HLA-A*01:01:01' is not in the header"
    for bad in ("chr1:0", "chr1:5-4", "chr1:", "chr1:a-b", "chr1:5-", "chr1:-5", "chr1:1-2147483649", "chr1:+5", "chr1:1-2-3"):
        with pytest.raises(RuntimeError, match="is not NAME, NAME:BEG or NAME:BEG-END"):
            kept(bad)
    assert kept("chr1:1-2147483648") == 1
    # an unaligned BAM has no references: regions are refused, as samtools view refuses them
    u = tmp_path / "u.bam"
    B.write_bam(u, [B.Rec(b"r", b"ACGT")])
    with pytest.raises(RuntimeError, match="reference 'chr1' of region 'chr1' is not in the header"):
        host.reads_read_all_r(str(u), "chr1")
    with pytest.raises(RuntimeError, match="kept only together with a region list"):
        host.reads_read_all_r(p, None, None, True)
    # no regions: the entry of before; a FASTQ file is read as without them
    a, b = host.reads_read_all_r(p), host.reads_read_all_f(p, {})
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:] and a[1] == 7
    q = tmp_path / "a.fq"
    q.write_bytes(b"@r\nACGT\n+\nIIII\n")
    assert host.reads_read_all_r(str(q), "chr1", bam_unplaced=True)[1:] == (1, 4, 0, 1, 0, 0)


@pytest.mark.parametrize("first", (0, 1000))
def test_host_reader_places_then_numbers_then_masks(first, tmp_path):
    recs = R.drawn(500)
    p = _bam(tmp_path, recs)
    f = F.Filter(exclude=0xF00)
    passing, _, n_reads, _ = R.apply(recs, f, R.CASE_REGIONS, True)
    kept, seen = S.bam_filtered(passing, 0.5, 11, first)
    masked, total = Q.masked_bam_records(kept, 20)
    block, cnt, rb, mb, nxt, records, reads = host.reads_read_all_r(p, LIST, bam_unplaced=True, bam_filter=f.dict(), fraction=0.5, seed=11,
                                                                    first_number=first, min_base_quality=20)
    assert block.tobytes() == B.reads_block(masked)[0]
    assert (cnt, mb, nxt, records, reads) == (len(kept), total, first + n_reads, len(recs), n_reads) and seen == n_reads
    assert 0 < len(kept) < n_reads and total > 0


def test_new_entries_are_declared_and_exported():
    for header, libpath, names in (("vgmi.h", vgmi.LIB_PATH, ("vgmi_fastq_set_bam_regions",)),
                                   ("vghost.h", host.LIB_PATH, ("vgh_sample_count_r", "vgh_reads_read_all_r"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
        for name in names:
            assert re.search(r"\b%s\s*\(" % name, txt), name
            assert re.search(r" T %s$" % name, out, flags=re.M), name
    vgmi.lib()
    assert "vgmi_fastq_set_bam_regions" in set(vgmi.SYMBOLS)
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", host.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T vgh::FastqKmerHip::FastqKmerHip\(vgmi_ctx\*, std::vector<.*> const&, unsigned int, unsigned int, unsigned long\)$", out, flags=re.M)
    assert re.search(r" T vgh::FastqKmerHipF::FastqKmerHipF\(", out) and re.search(r" T vgh::FastqKmerHipR::FastqKmerHipR\(", out)


def test_cli_help_names_the_options_and_refuses_unplaced_alone(tmp_path):
    r = subprocess.run([CLI, "genotype", "-h"], capture_output=True, text=True)
    text = r.stderr + r.stdout
    for opt in ("--bam-regions ", "--bam-regions-file", "--bam-regions-unplaced"):
        assert opt in text, opt
    assert "samtools view -L" in text
    graph = os.path.join(tmp_path, "graph.bin")
    open(graph, "wb").write(gzip.open(os.path.join(GOLDEN, "cohort_snp", "graph.bin.gz"), "rb").read())
    # (the sample file does not exist: the refusal comes before any file is opened)
    open(os.path.join(tmp_path, "s.cfg"), "w").write("sample0 " + os.path.join(tmp_path, "missing.bam") + "\n")
    r = subprocess.run([CLI, "genotype", "--load-graph", graph, "-s", "s.cfg", "--bam-regions-unplaced"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "Parameter error: --bam-regions-unplaced." in r.stderr and "--bam-regions or --bam-regions-file" in r.stderr, r.stderr
    assert "missing.bam" not in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".vcf.gz")]
