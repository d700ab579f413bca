"""The BAM region test on the device (bam_keep_region_kernel; csrc/vgmi_bam.hip) through Context.bam_bgzf, the C ABI and
Graph.sample_count.  The oracle throughout: the stream with regions equals the plain stream of a BAM holding only the passing records, as
the Python model of bam_region_cases.py names them -- counters, per-node counters, histogram, n_records, n_bases; consumed stays the
file's bytes; the stats are the model's counts.  Files of about 2 000 records in 64 KiB chunks, so that chunks end inside records and
records are carried.  tests/test_bam_region_cpu.py checks the model against the rule's C++."""
import ctypes as C
import os

import numpy as np
import pytest

import bam_cases as BC
import bam_filter_cases as F
import bam_py as B
import bam_region_cases as R
import quality_mask_cases as Q
import subsample_cases as S
from conftest import get_cohort
from varigraph_amd import host, vgmi

pytestmark = pytest.mark.gpu

N_REF = len(R.REFS)
LIST = "chr1:101-200,chr1:301-400,chr1:1001-1100,chr2:2147483639-2147483648,chrLast"      # R.CASE_REGIONS, 1-based inclusive


@pytest.fixture(scope="module")
def gc():
    cohort = get_cohort("cohort_snp")
    g = host.Graph(os.path.join(cohort.dir, "graph.bin.gz"))
    ctx = vgmi.Context(0, buffer_mib=16)
    g.upload(ctx)
    yield g, ctx, cohort.haplotypes()
    ctx.close()
    g.close()


@pytest.fixture(scope="module")
def recs2000(gc):
    """the case set (every class of the rule's edges) among drawn records: 2 000 in all"""
    haps = gc[2]
    cs = [r for _, r in R.cases(haps)]
    drawn = R.drawn(2000 - len(cs), haps=haps)
    return drawn[:700] + cs + drawn[700:]


def _same_counts(a, b, what):
    for x, y, name in zip(a, b, ("counters", "node counters", "histogram")):
        assert np.array_equal(x, y), (what, name)


def _stream(ctx, recs, tmp_path, monkeypatch, chunk_kb="64", **kw):
    p = tmp_path / "s.bam"
    hlen, offs = R.write_bam(p, recs)
    comp = p.read_bytes()
    with monkeypatch.context() as m:
        m.setenv("VGMI_FASTQ_CHUNK_KB", chunk_kb)
        ctx.counts_reset()
        r = ctx.bam_bgzf(comp, hlen, N_REF, **kw)
        counts = ctx.counts_finish(nodes=True, hist=True)
    return r, counts, (hlen, offs, offs[-1] + len(R.record(recs[-1])) if recs else hlen)


def _check(ctx, recs, regions, unplaced, what, tmp_path, monkeypatch, f=F.Filter(), **kw):
    passing, n_rec, n_reads, at = R.apply(recs, f, regions, unplaced)
    assert at is None, what
    if f.on:
        kw["bam_filter"] = f.dict()
    got, c_got, (_, _, raw_len) = _stream(ctx, recs, tmp_path, monkeypatch, bam_regions=regions, bam_unplaced=unplaced, **kw)
    want, c_want, _ = _stream(ctx, passing, tmp_path, monkeypatch)
    print(f"{what}: {got['bam_reads']} of {got['bam_records']} records are reads (model {n_reads} of {n_rec}), bases {got['n_bases']}")
    assert not got["stopped"] and not got["inflate_failed"] and got["tail"] == b"", what
    assert (got["bam_records"], got["bam_reads"]) == (n_rec, n_reads) == (len(recs), len(passing)), what
    assert (got["n_records"], got["n_bases"]) == (want["n_records"], want["n_bases"]) == B.reads_block(passing)[1:], what
    assert got["consumed"] == raw_len, what
    _same_counts(c_got, c_want, what)
    return got, c_got, n_reads


# ---- 1: regions alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unplaced", (False, True))
def test_case_set_and_drawn_records(unplaced, gc, recs2000, tmp_path, monkeypatch):
    g, ctx, _ = gc
    got, c_got, n_reads = _check(ctx, recs2000, R.CASE_REGIONS, unplaced, ("cases", unplaced), tmp_path, monkeypatch)
    assert 100 < n_reads < sum(1 for r in recs2000 if r.kept) - 100
    if not unplaced:
        plain, c_plain, _ = _stream(ctx, recs2000, tmp_path, monkeypatch)
        assert not np.array_equal(c_plain[0], c_got[0]) and plain["n_records"] > got["n_records"] and "bam_records" not in plain
        # one chunk holds the whole file: the same answer
        whole, c_whole, _ = _stream(ctx, recs2000, tmp_path, monkeypatch, chunk_kb="0", bam_regions=R.CASE_REGIONS)
        assert (whole["n_records"], whole["n_bases"], whole["bam_records"]) == (got["n_records"], got["n_bases"], len(recs2000))
        _same_counts(c_whole, c_got, "one chunk")


@pytest.mark.parametrize("n", R.LIST_SIZES)
def test_list_sizes_at_the_binary_searchs_edges(n, gc, tmp_path, monkeypatch):
    """1 to 1 025 merged intervals, on one reference (even n) or dealt over all four, given unsorted; records drawn over their span"""
    g, ctx, haps = gc
    several = n % 2 == 1
    regions = R.interval_list(n, several)
    assert len(R.normalise(regions)) == n
    recs = R.drawn(2000, span=100 * (n // (N_REF if several else 1) + 2), seed=50 + n, haps=haps)
    got, _, n_reads = _check(ctx, recs, regions, n % 3 == 0, ("list", n), tmp_path, monkeypatch)
    assert 0 < n_reads < sum(1 for r in recs if r.kept)


# ---- 2: with the other options ---------------------------------------------------------------------------------------------------------------
def test_regions_with_flags_mapq_and_tag(gc, recs2000, tmp_path, monkeypatch):
    g, ctx, _ = gc
    recs = [r for r in recs2000 if not r.aux.endswith((F.fault("type"), F.fault("nonul")))]
    for regions_first in (False, True):
        got, _, n_reads = _check(ctx, recs, R.CASE_REGIONS, True, ("with the filter", regions_first), tmp_path, monkeypatch, f=R.CASE_FILTER,
                                 regions_first=regions_first)
        assert 20 < n_reads < R.apply(recs, F.Filter(), R.CASE_REGIONS, True)[2]


def test_regions_then_number_then_mask(gc, recs2000, tmp_path, monkeypatch):
    """--subsample numbers the reads that passed the regions, --min-base-quality masks the kept ones"""
    g, ctx, _ = gc
    passing, n_rec, n_reads, _ = R.apply(recs2000, F.Filter(), R.CASE_REGIONS, True)
    kept, seen = S.bam_filtered(passing, 0.5, 11)
    masked, total = Q.masked_bam_records(kept, 20)
    for kw, oracle, n_kept in ((dict(subsample=(0.5, 11)), kept, len(kept)), (dict(min_quality=20), Q.masked_bam_records(passing, 20)[0], n_reads),
                               (dict(subsample=(0.5, 11), min_quality=20), masked, len(kept))):
        got, c_got, _ = _stream(ctx, recs2000, tmp_path, monkeypatch, bam_regions=R.CASE_REGIONS, bam_unplaced=True, **kw)
        want, c_want, _ = _stream(ctx, oracle, tmp_path, monkeypatch)
        assert (got["n_records"], got["n_bases"]) == (n_kept, want["n_bases"]) and (got["bam_records"], got["bam_reads"]) == (n_rec, n_reads), kw
        if "subsample" in kw:
            assert (got["n_seen"], got["n_kept"]) == (n_reads, len(kept)) and seen == n_reads and 0 < len(kept) < n_reads
        if len(kw) == 2:
            assert got["masked_bases"] == total > 0
        _same_counts(c_got, c_want, kw)


# ---- 3: walk faults ---------------------------------------------------------------------------------------------------------------------------
def test_a_walk_fault_stops_the_device_only_inside_the_regions(gc, tmp_path, monkeypatch):
    """three records whose auxiliary fields cannot be walked: outside every region, unplaced, and inside a region.  With a tag bound the
    device stops at the third alone, at its first byte"""
    g, ctx, haps = gc
    d = F.Draw(61, haps)
    recs = [r for r in R.drawn(1500, haps=haps, seed=62) if r.aux]
    bad = F.aux(b"NM", "C", 1) + F.fault("type")
    recs[300] = d.rec(flag=0, ref=0, pos=220, cigar=[(30, "M")], aux=bad)
    recs[600] = d.rec(flag=4, ref=-1, pos=-1, aux=bad)
    recs[900] = d.rec(flag=0, ref=0, pos=150, cigar=[(30, "M")], aux=bad)
    f = F.Filter(tag=b"qs", min_value=10)
    front, n_rec, n_reads, at = R.apply(recs, f, R.CASE_REGIONS, False)
    assert at == 900 and n_rec == 900 and n_reads > 20
    got, c_got, (_, offs, _) = _stream(ctx, recs, tmp_path, monkeypatch, bam_regions=R.CASE_REGIONS, bam_filter=f.dict())
    want, c_want, _ = _stream(ctx, front, tmp_path, monkeypatch)
    assert got["stopped"] and got["consumed"] == offs[900] and got["tail"] == b"" and not got["inflate_failed"]
    assert (got["bam_records"], got["bam_reads"], got["n_records"]) == (900, n_reads, want["n_records"])
    _same_counts(c_got, c_want, "stopped inside the region")
    # with unplaced reads kept, the unplaced one is walked: the stop moves there
    got, _, _ = _stream(ctx, recs, tmp_path, monkeypatch, bam_regions=R.CASE_REGIONS, bam_unplaced=True, bam_filter=f.dict())
    assert got["stopped"] and got["consumed"] == offs[600] and got["bam_records"] == 600
    # without the tag bound nothing is walked
    _check(ctx, recs, R.CASE_REGIONS, True, "no tag bound", tmp_path, monkeypatch)
    # the product path names the record
    p = tmp_path / "f.bam"
    R.write_bam(p, recs)
    with pytest.raises(vgmi.VgmiError) as e:
        g.sample_count(ctx, [str(p)], threads=4, require_depth=False, bam_filter=f.dict(), bam_regions=LIST)
    assert f"'{p}': not a valid BAM record at decompressed byte {offs[900]} (auxiliary fields)" in str(e.value)


# ---- 4: the hand-over ---------------------------------------------------------------------------------------------------------------------------
def _sample(g, ctx, path, monkeypatch, env=None, **kw):
    with monkeypatch.context() as m:
        for k in ("VGH_HOST_PARSE", "VGH_HOST_INFLATE", "VGMI_FASTQ_CHUNK_KB"):
            m.delenv(k, raising=False)
        for k, v in (env or {}).items():
            m.setenv(k, v)
        cov, node, hist, st = g.sample_count(ctx, [str(path)], threads=4, require_depth=False, **kw)
    return (cov, node, hist), (st["n_reads"], st["read_base"]), (st.get("bam_records"), st.get("bam_reads")), st


def test_hand_over_legs_give_the_devices_answer(gc, tmp_path, monkeypatch):
    """in the middle a record longer than the 1 MiB carry, inside a region: the device stops there and the host decoder goes on with the same
    list.  The device path, the host reader alone (VGH_HOST_PARSE=1) and VGH_HOST_INFLATE=1 agree with the plain file of the passing records"""
    g, ctx, haps = gc
    d = F.Draw(71, haps)
    recs = R.drawn(1200, haps=haps, seed=72)
    recs[600] = d.rec(flag=0, ref=0, pos=150, cigar=[(100, "M")], aux=F.aux(b"XB", "B", bytes(BC.TAIL_MAX), "C") + F.aux(b"qs", "C", 30))
    passing, n_rec, n_reads, at = R.apply(recs, F.Filter(), R.CASE_REGIONS, True)
    assert at is None and recs[600].seq in [r.seq for r in passing]
    R.write_bam(tmp_path / "g.bam", recs)
    R.write_bam(tmp_path / "gp.bam", passing)
    bed = tmp_path / "t.bed"
    bed.write_text("chr1\t100\t200\nchr1\t300\t400\nchrUn\t0\t5\nchr1\t1000\t1100\n")
    kw = dict(bam_regions="chr2:2147483639-2147483648,chrLast", bam_regions_bed=str(bed), bam_unplaced=True)
    want = _sample(g, ctx, tmp_path / "gp.bam", monkeypatch)
    assert want[1] == B.reads_block(passing)[1:] and want[2] == (None, None)
    for env in ({"VGMI_FASTQ_CHUNK_KB": "64"}, {}, {"VGH_HOST_PARSE": "1"}, {"VGH_HOST_INFLATE": "1"}):
        got = _sample(g, ctx, tmp_path / "g.bam", monkeypatch, env=env, **kw)
        assert got[1] == want[1] and got[2] == (n_rec, n_reads), env
        _same_counts(got[0], want[0], env)
    # the device's share: it stops at the long record, the records in front of it placed
    r, _, (_, offs, _) = _stream(ctx, recs, tmp_path, monkeypatch, bam_regions=R.CASE_REGIONS, bam_unplaced=True)
    front = R.apply(recs[:600], F.Filter(), R.CASE_REGIONS, True)
    assert r["stopped"] and r["consumed"] == offs[600] and (r["bam_records"], r["bam_reads"], r["n_records"]) == (600, front[2], front[2])
    # with the filter, subsampling and the mask through the product path
    f = F.Filter(exclude=0xF00, min_mapq=20)
    passing, n_rec, n_reads, _ = R.apply(recs, f, R.CASE_REGIONS, True)
    kept, _ = S.bam_filtered(passing, 0.5, 11)
    R.write_bam(tmp_path / "gk.bam", Q.masked_bam_records(kept, 20)[0])
    want = _sample(g, ctx, tmp_path / "gk.bam", monkeypatch)
    for env in ({"VGMI_FASTQ_CHUNK_KB": "64"}, {"VGH_HOST_PARSE": "1"}):
        got = _sample(g, ctx, tmp_path / "g.bam", monkeypatch, env=env, bam_filter=f.dict(), subsample=(0.5, 11), min_base_quality=20, **kw)
        assert got[1] == want[1] and got[2] == (n_rec, n_reads) and (got[3]["reads_seen"], got[3]["reads_kept"]) == (n_reads, len(kept)), env
        _same_counts(got[0], want[0], env)
    # a name the header lacks ends the count with the file's name
    with pytest.raises(vgmi.VgmiError) as e:
        g.sample_count(ctx, [str(tmp_path / "g.bam")], threads=4, require_depth=False, bam_regions="chr1,chrM:1-5")
    assert f"'{tmp_path / 'g.bam'}': reference 'chrM' of region 'chrM:1-5' is not in the header" in str(e.value)


# ---- 5: the C entry ---------------------------------------------------------------------------------------------------------------------------
def _arrays(regions):
    n = max(len(regions), 1)
    return ((C.c_int32 * n)(*[r[0] for r in regions]), (C.c_int64 * n)(*[r[1] for r in regions]), (C.c_int64 * n)(*[r[2] for r in regions]))


def test_empty_list_is_the_stream_of_no_call(gc, recs2000, tmp_path, monkeypatch):
    g, ctx, _ = gc
    recs = recs2000[:600]
    none, c_none, _ = _stream(ctx, recs, tmp_path, monkeypatch)
    empty, c_empty, _ = _stream(ctx, recs, tmp_path, monkeypatch, bam_regions=[])
    assert empty["filter_stats_rc"] == vgmi.E_STATE and empty["bam_records"] is None
    assert {k: v for k, v in empty.items() if k in none} == none and none["n_records"] == sum(1 for r in recs if r.kept)
    _same_counts(c_empty, c_none, "n == 0")


def test_setter_refusals_leave_the_stream_serving(gc, recs2000, tmp_path, monkeypatch):
    g, ctx, _ = gc
    l = ctx._l
    recs = recs2000[:600]
    passing, n_rec, n_reads, _ = R.apply(recs, F.Filter(), R.CASE_REGIONS, False)
    want, c_want, _ = _stream(ctx, passing, tmp_path, monkeypatch)
    p = tmp_path / "c.bam"
    hlen, _ = R.write_bam(p, recs)
    data = p.read_bytes()
    ctx.counts_reset()
    fq = C.c_void_p()
    assert l.vgmi_fastq_open_bam(ctx._h, hlen, N_REF, C.byref(fq)) == 0
    seen = set()
    for bad, unplaced in (([(N_REF, 0, 5)], 0), ([(-1, 0, 5)], 0), ([(0, -1, 5)], 0), ([(0, R.WHOLE, R.WHOLE + 1)], 0), ([(0, 5, 5)], 0),
                          ([(0, 5, R.WHOLE + 1)], 0), ([], 1)):
        assert l.vgmi_fastq_set_bam_regions(fq, len(bad), *_arrays(bad), unplaced) == vgmi.E_INVALID, bad
        msg = l.vgmi_last_error(ctx._h)
        assert b"BAM" in msg, msg
        seen.add(msg)
    # more than 2^20 intervals left after merging; 2^20 + 1 touching ones merge into one and are accepted
    many = (1 << 20) + 1
    ref = np.zeros(many, dtype=np.int32)
    beg = np.arange(many, dtype=np.int64) * 2
    end = beg + 1
    ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    assert l.vgmi_fastq_set_bam_regions(fq, many, ptr(ref, C.c_int32), ptr(beg, C.c_int64), ptr(end, C.c_int64), 0) == vgmi.E_INVALID
    seen.add(l.vgmi_last_error(ctx._h))
    assert len(seen) == 5, seen      # a reference, a begin, an end, unplaced alone, too many: each its own message
    end = beg + 2
    assert l.vgmi_fastq_set_bam_regions(fq, many, ptr(ref, C.c_int32), ptr(beg, C.c_int64), ptr(end, C.c_int64), 0) == 0
    assert l.vgmi_fastq_set_bam_regions(fq, len(R.CASE_REGIONS), *_arrays(R.CASE_REGIONS), 0) == 0      # the last list set holds
    pos = 0
    rec_n, read_n = C.c_uint64(), C.c_uint64()
    while pos < len(data):
        buf, cap = C.c_void_p(), C.c_size_t()
        assert l.vgmi_fastq_acquire(fq, C.byref(buf), C.byref(cap)) == 0
        n = min(cap.value, len(data) - pos)
        C.memmove(buf, data[pos:pos + n], n)
        taken = C.c_size_t()
        assert l.vgmi_fastq_commit_bgzf(fq, n, C.byref(taken), None, None) == 0 and taken.value > 0
        pos += taken.value
        assert l.vgmi_fastq_set_bam_regions(fq, 0, None, None, None, 0) == vgmi.E_STATE      # bytes have been committed
        assert l.vgmi_fastq_bam_filter_stats(fq, C.byref(rec_n), C.byref(read_n)) == 0       # ... and the stream serves on
    assert (rec_n.value, read_n.value) == (n_rec, n_reads)
    nr, nb, cons, st = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    assert l.vgmi_fastq_close(fq, C.byref(nr), C.byref(nb), C.byref(cons), C.byref(st), None, 0, None) == 0
    assert (nr.value, nb.value, st.value) == (want["n_records"], want["n_bases"], 0)
    _same_counts(ctx.counts_finish(nodes=True, hist=True), c_want, "the list set after the refused calls holds")
    # a FASTQ stream accepts the call without effect
    assert l.vgmi_fastq_open(ctx._h, C.byref(fq)) == 0
    assert l.vgmi_fastq_set_bam_regions(fq, 1, *_arrays([(7, 0, 5)]), 1) == 0
    assert l.vgmi_fastq_bam_filter_stats(fq, C.byref(rec_n), C.byref(read_n)) == vgmi.E_STATE
    assert l.vgmi_fastq_close(fq, None, None, None, None, None, 0, None) == 0
    # a refusal through the wrapper, then a valid run on the same context
    with pytest.raises(vgmi.VgmiError) as e:
        ctx.bam_bgzf(data, hlen, N_REF, bam_regions=[(N_REF, 0, 1)])
    assert e.value.code == vgmi.E_INVALID
    _check(ctx, recs, R.CASE_REGIONS, False, "after a refusal", tmp_path, monkeypatch)
