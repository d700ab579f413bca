"""The BAM read filter without a device: the rule of csrc/vgmi_bam_filter.h in a stand-alone program under ASan + UBSan against the
Python model of bam_filter_cases.py, record by record, verdict and value; the host decoder's form of it (BamReader::filter through
vgh_reads_read_all_f: what every host leg of vgh_sample_count_f applies) against the model -- block, read_base, records / reads, the
error text with its byte number, also with a minimum base quality and subsampling from a non-zero first number; mutated rules give
other results on the same cases; the entries are declared and exported; the CLI's option parsing."""
import gzip
import math
import os
import re
import struct
import subprocess

import pytest

import bam_filter_cases as F
import bam_py as B
import quality_mask_cases as Q
import subsample_cases as S
from conftest import GOLDEN, ROOT
from varigraph_amd import host, vgmi

CLI = os.path.join(ROOT, "varigraph_amd", "bin", "varigraph-mi")
EXTREMES = (("c", -128), ("C", 255), ("s", -32768), ("S", 65535), ("i", -2 ** 31), ("I", 2 ** 32 - 1))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """tests/native/bam_filter_check.cpp under AddressSanitizer + UBSan -> run(records, filter) = [(verdict, value bits or None)]"""
    d = tmp_path_factory.mktemp("bam_filter_check")
    exe = str(d / "bam_filter_check")
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-I",
                        os.path.join(ROOT, "varigraph_amd", "csrc"), os.path.join(ROOT, "tests", "native", "bam_filter_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(raws, f):
        p = d / "records.bin"
        p.write_bytes(b"".join(raws))
        r = subprocess.run([exe, str(p), str(f.exclude), str(f.require), str(f.min_mapq), f.tag.decode() if f.tag else "-", repr(float(f.min_value))],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
        out = []
        for line in r.stdout.split("\n")[:-1]:
            v, bits = line.split()
            out.append((int(v), None if bits == "-" else int(bits, 16)))
        assert len(out) == len(raws)
        return out
    return run


def _same(got, raws, f):
    for i, ((v, bits), raw) in enumerate(zip(got, raws)):
        mv, mval = F.verdict_raw(raw, f)
        assert v == mv, (i, f, v, mv, F.fields(raw)[-1][:60])
        if mval is None:
            assert bits is None, (i, f)
        elif math.isnan(mval):
            assert bits is not None and math.isnan(struct.unpack("<d", struct.pack("<Q", bits))[0]), (i, f)
        else:
            assert bits == struct.unpack("<Q", struct.pack("<d", mval))[0], (i, f, mval)


def _raws(recs):
    return [B.record(r) for r in recs]


def test_flag_and_mapq_rules_equal_the_model(check):
    raws = _raws(F.flag_records(400))
    for name, f in F.FLAG_FILTERS.items():
        got = check(raws, f)
        _same(got, raws, f)
        n = sum(1 for v, _ in got if v == F.READ)
        assert 0 < n < len(raws), name
    _same(check(raws, F.Filter()), raws, F.Filter())
    # 255 passes every bound, an unmapped record's 0 no positive one
    d = F.Draw(1)
    two = _raws([d.rec(mapq=255), d.rec(flag=4, mapq=0)])
    assert [v for v, _ in check(two, F.Filter(min_mapq=255))] == [1, 0] and [v for v, _ in check(two, F.Filter(min_mapq=1))] == [1, 0]


@pytest.mark.parametrize("bound", (10.0, 9.999, -1e308, float("inf"), float("-inf")))
def test_every_type_as_the_tag_and_in_front_of_it(bound, check):
    """the tag in every numeric type, first, last, absent, twice, non-numeric, behind every other type; faults behind it are not seen"""
    raws = _raws(F.tag_records())
    f = F.Filter(tag=b"qs", min_value=bound)
    got = check(raws, f)
    _same(got, raws, f)
    assert not any(v == F.FAULT for v, _ in got)
    if bound == 10.0:
        assert sum(1 for v, _ in got if v == F.READ) > len(F.FRONTS) * 10
    # the tag first, and the same fields wanted as the LAST tag of the record
    f = F.Filter(tag=b"ZZ", min_value=5.0)
    _same(check(raws, f), raws, f)


def test_float_values_at_the_bound(check):
    d = F.Draw(2)
    vals = [F.f32(0.99), F.f32_below(0.99), float("nan"), float("inf"), float("-inf")]
    raws = _raws([d.rec(aux=F.aux(b"rq", "f", v)) for v in vals]) + _raws(F.rq_records())
    f = F.Filter(tag=b"rq", min_value=0.99)
    got = check(raws, f)
    _same(got, raws, f)
    assert [v for v, _ in got[:5]] == [1, 0, 0, 1, 0]      # 0.99f is 0.9900000095...: it passes the double bound 0.99
    f = F.Filter(tag=b"rq", min_value=float("-inf"))
    assert [v for v, _ in check(raws[:5], f)] == [1, 1, 0, 1, 1]      # a NaN fails every bound


@pytest.mark.parametrize("typ,val", EXTREMES)
def test_integer_extremes_convert_exactly(typ, val, check):
    d = F.Draw(3)
    raws = _raws([d.rec(aux=F.aux(b"xv", typ, val))])
    for bound, want in ((float(val), 1), (float(val + 1), 0), (float(val - 1), 1)):
        f = F.Filter(tag=b"xv", min_value=bound)
        got = check(raws, f)
        _same(got, raws, f)
        assert got[0] == (want, struct.unpack("<Q", struct.pack("<d", float(val)))[0])


def test_arrays_are_passed_over_by_arithmetic(check):
    d = F.Draw(4)
    recs = [d.rec(aux=F.aux(b"B0", "B", [], "S") + F.aux(b"qs", "C", 12)),
            d.rec(aux=F.aux(b"BL", "B", [3] * 70000, "i") + F.aux(b"qs", "C", 12)),
            d.rec(aux=F.aux(b"BL", "B", [3] * 70000, "C") + F.aux(b"qs", "C", 9)),
            d.rec(aux=F.aux(b"qs", "B", [3] * 70000, "f"))]
    raws = _raws(recs)
    f = F.Filter(tag=b"qs", min_value=10)
    got = check(raws, f)
    _same(got, raws, f)
    assert [v for v, _ in got] == [1, 1, 0, 0]


@pytest.mark.parametrize("kind", F.FAULTS)
def test_walk_faults_in_front_of_the_tag_and_behind_it(kind, check):
    d = F.Draw(5)
    bad = F.fault(kind)
    recs = [d.rec(aux=F.aux(b"NM", "C", 1) + bad),                             # no tag in front of the fault: invalid
            d.rec(aux=F.aux(b"NM", "C", 1) + F.aux(b"qs", "C", 30) + bad),     # behind the tag: not seen
            d.rec(aux=F.aux(b"qs", "C", 3) + bad),                             # behind a tag that fails the bound: not seen, not a read
            d.rec(aux=bad),
            d.rec(flag=0x800, aux=bad),                                        # fails 1 to 4: never walked
            d.rec(0, aux=bad)]
    raws = _raws(recs)
    f = F.Filter(tag=b"qs", min_value=10)
    got = check(raws, f)
    _same(got, raws, f)
    assert [v for v, _ in got] == [-1, 1, 0, -1, 0, 0]
    # without a tag bound the auxiliary bytes are never read
    assert [v for v, _ in check(raws, F.Filter(exclude=0xF00))] == [1, 1, 1, 1, 0, 0]


def test_a_fault_inside_the_wanted_field_is_a_fault(check):
    d = F.Draw(6)
    raws = _raws([d.rec(aux=b"qsi\x01\x02"), d.rec(aux=b"qsZabc"), d.rec(aux=b"qsBI" + struct.pack("<I", 0x7FFFFFFF) + bytes(12))])
    f = F.Filter(tag=b"qs", min_value=0)
    got = check(raws, f)
    _same(got, raws, f)
    assert [v for v, _ in got] == [-1, -1, -1]


def test_mutated_rules_give_other_results():
    """the cases discriminate: `require` as "any bit", MAPQ with >, the last occurrence of the tag deciding"""
    raws = _raws(F.flag_records(400))
    f = F.FLAG_FILTERS["all_together"]
    f2 = F.Filter(exclude=0x900, require=0x5)
    assert [F.verdict_raw(r, f2)[0] for r in raws] != [F.verdict_raw(r, f2, mutate="any")[0] for r in raws]
    assert [F.verdict_raw(r, f)[0] for r in raws] != [F.verdict_raw(r, f, mutate="gt")[0] for r in raws]
    raws = _raws(F.tag_records())
    f = F.Filter(tag=b"qs", min_value=10.0)
    true, last = [F.verdict_raw(r, f)[0] for r in raws], [F.verdict_raw(r, f, mutate="last")[0] for r in raws]
    assert true != last and F.FAULT in last and F.FAULT not in true


# ---- the host decoder ----------------------------------------------------------------------------------------------------------------
def _reader(tmp_path, recs, f, **kw):
    p = tmp_path / "a.bam"
    B.write_bam(p, recs)
    return host.reads_read_all_f(str(p), f.dict(), **kw), str(p)


@pytest.mark.parametrize("name", list(F.FLAG_FILTERS))
def test_host_reader_applies_the_flag_rules(name, tmp_path):
    f, recs = F.FLAG_FILTERS[name], F.flag_records(500)
    passing, n_rec, n_reads, at = F.apply(recs, f)
    want, n, rb = B.reads_block(passing)
    (block, cnt, read_base, mb, nxt, records, reads), _ = _reader(tmp_path, recs, f)
    assert block.tobytes() == want and (cnt, read_base, mb, nxt) == (n, rb, 0, n) and at is None
    assert (records, reads) == (len(recs), n_reads) == (n_rec, n)
    assert 0 < n < sum(1 for r in recs if r.seq)


def test_host_reader_applies_the_tag_bound(tmp_path):
    every = F.tag_records() + F.rq_records()
    for f in (F.Filter(tag=b"qs", min_value=10.0), F.Filter(tag=b"rq", min_value=0.99), F.Filter(exclude=0, tag=b"ZZ", min_value=5)):
        recs = [r for r in every if F.verdict(r, f)[0] != F.FAULT]      # (the records whose fault lies behind qs: another tag's walk meets it)
        assert len(recs) > len(every) - 30
        passing, n_rec, n_reads, at = F.apply(recs, f)
        want, n, rb = B.reads_block(passing)
        (block, cnt, read_base, _, _, records, reads), _ = _reader(tmp_path, recs, f)
        assert block.tobytes() == want and (cnt, read_base, records, reads) == (n, rb, len(recs), n_reads) and at is None and n > 0


def test_default_filter_is_the_reader_of_before(tmp_path):
    recs = F.flag_records(300)
    (block, cnt, rb, _, _, records, reads), p = _reader(tmp_path, recs, F.Filter())
    old, n_old, rb_old = host.reads_read_all_s(p, 1.0, 11)[:3]
    assert block.tobytes() == old.tobytes() == B.reads_block(recs)[0] and (cnt, rb) == (n_old, rb_old)
    assert (records, reads) == (len(recs), cnt)


@pytest.mark.parametrize("kind", F.FAULTS)
@pytest.mark.parametrize("where", ("first", "middle"))
def test_host_reader_names_the_faulted_record(kind, where, tmp_path):
    recs, at = F.faulted(kind, where)
    f = F.Filter(tag=b"qs", min_value=10)
    assert F.apply(recs, f)[3] == at
    p = tmp_path / "a.bam"
    _, offs = B.write_bam(p, recs)
    with pytest.raises(RuntimeError) as e:
        host.reads_read_all_f(str(p), f.dict())
    assert str(e.value) == f"'{p}': not a valid BAM record at decompressed byte {offs[at]} (auxiliary fields)"
    # no stop where nothing walks: without a tag bound, or with the faulted record failing 1 to 4
    assert host.reads_read_all_f(str(p), F.Filter(exclude=0xF00).dict())[1] == len(recs)
    recs[at].flag = 0x200
    B.write_bam(p, recs)
    g = F.Filter(exclude=0xB00, tag=b"qs", min_value=10)
    assert host.reads_read_all_f(str(p), g.dict())[1] == F.apply(recs, g)[2] > 0


@pytest.mark.parametrize("first", (0, 1000))
def test_host_reader_filters_then_numbers_then_masks(first, tmp_path):
    """with subsampling and a minimum base quality: the reads that passed are numbered from `first`, the kept ones masked"""
    recs = F.flag_records(500)
    f = F.Filter(exclude=0xF00, min_mapq=20)
    passing, _, n_reads, _ = F.apply(recs, f)
    kept, seen = S.bam_filtered(passing, 0.5, 11, first)
    masked, total = Q.masked_bam_records(kept, 20)
    (block, cnt, rb, mb, nxt, records, reads), _ = _reader(tmp_path, recs, f, fraction=0.5, seed=11, first_number=first, min_base_quality=20)
    assert block.tobytes() == B.reads_block(masked)[0]
    assert (cnt, mb, nxt, records, reads) == (len(kept), total, first + n_reads, len(recs), n_reads) and seen == n_reads
    assert 0 < len(kept) < n_reads and total > 0


def test_bad_parameters_are_refused_by_the_host_entry(tmp_path):
    p = tmp_path / "a.bam"
    B.write_bam(p, F.flag_records(5))
    for bad, what in ((dict(exclude=0x10000), "exclude flags"), (dict(require=0x10000), "require flags"), (dict(min_mapq=256), "MAPQ"),
                      (dict(tag=b"1a"), "tag"), (dict(tag=b"a_"), "tag"), (dict(tag=b"qs", min_value=float("nan")), "not a number")):
        with pytest.raises(RuntimeError, match=what):
            host.reads_read_all_f(str(p), bad)
    assert host.reads_read_all_f(str(p), dict(exclude=0xFFFF, require=0xFFFF, min_mapq=255, tag=b"q9", min_value=float("inf")))[1] == 0
    # a FASTQ file is read as without the filter
    q = tmp_path / "a.fq"
    q.write_bytes(b"@r\nACGT\n+\nIIII\n")
    assert host.reads_read_all_f(str(q), dict(exclude=0xFFFF, min_mapq=255))[1:] == (1, 4, 0, 1, 0, 0)


def test_new_entries_are_declared_and_exported():
    for header, libpath, names in (("vgmi.h", vgmi.LIB_PATH, ("vgmi_fastq_set_bam_filter", "vgmi_fastq_bam_filter_stats")),
                                   ("vghost.h", host.LIB_PATH, ("vgh_sample_count_f", "vgh_reads_read_all_f"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
        for name in names:
            assert re.search(r"\b%s\s*\(" % name, txt), name
            assert re.search(r" T %s$" % name, out, flags=re.M), name
    vgmi.lib()
    assert {"vgmi_fastq_set_bam_filter", "vgmi_fastq_bam_filter_stats"} <= set(vgmi.SYMBOLS)
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", host.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T vgh::FastqKmerHip::FastqKmerHip\(vgmi_ctx\*, std::vector<.*> const&, unsigned int, unsigned int, unsigned long\)$", out, flags=re.M)


def test_cli_help_names_the_options_and_refuses_bad_values(tmp_path):
    r = subprocess.run([CLI, "genotype", "-h"], capture_output=True, text=True)
    text = r.stderr + r.stdout
    for opt in ("--bam-exclude-flags", "--bam-require-flags", "--bam-min-mapq", "--bam-min-tag"):
        assert opt in text, opt
    assert "REPLACES the default" in text and "does not pass a positive bound" in text
    graph = os.path.join(tmp_path, "graph.bin")
    open(graph, "wb").write(gzip.open(os.path.join(GOLDEN, "cohort_snp", "graph.bin.gz"), "rb").read())
    open(os.path.join(tmp_path, "s.cfg"), "w").write("sample0 " + os.path.join(GOLDEN, "cohort_snp", "reads_1.fq.gz") + "\n")
    base = [CLI, "genotype", "--load-graph", graph, "-s", "s.cfg"]
    for opt, bad, what in (("--bam-exclude-flags", "abc", "is not a non-negative integer"), ("--bam-exclude-flags", "-1", "is not a non-negative integer"),
                           ("--bam-exclude-flags", "0x10000", "between 0 and 65535"), ("--bam-exclude-flags", "12x", "is not a non-negative integer"),
                           ("--bam-require-flags", "65536", "between 0 and 65535"), ("--bam-require-flags", "0xZ", "is not a non-negative integer"),
                           ("--bam-min-mapq", "256", "between 0 and 255"), ("--bam-min-mapq", "q", "is not a non-negative integer"),
                           ("--bam-min-tag", "rq", "Expected TAG:VALUE"), ("--bam-min-tag", "1q:3", "Expected TAG:VALUE"),
                           ("--bam-min-tag", "rq=0.99", "Expected TAG:VALUE"), ("--bam-min-tag", "rq:abc", "is not a number"),
                           ("--bam-min-tag", "rq:nan", "not NaN")):
        r = subprocess.run(base + [opt, bad], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and "Parameter error: " + opt + "." in r.stderr and what in r.stderr, (opt, bad, r.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".vcf.gz")]
