"""The read filter by length and read quality on the device (-m gpu): fq_records_rf / fq_read_quality / fq_finish_rf of vgmi_fastq.hip,
bam_read_filter / bam_finish_rf of vgmi_bam.hip, and everything above them.

The oracle is the rule itself: counting file G with the rule must equal counting G' with the option off, G' = G with exactly the
failing reads removed (read_filter_cases.py).  Counters, node counters, histogram, records, bases and masked bases are compared with
those of G', the five stats with the model's; consumed must be the file's length and stopped False -- every record has been taken by
the DEVICE, so the host reader's form of the rule cannot make these tests green.  Then the hand-overs, where device and host share a
file and their class counts add up, and the refusals."""
import gzip
import os
import re

import ctypes as C
import numpy as np
import pytest

import bam_cases as BC
import bam_filter_cases as F
import bam_py as B
import bam_region_cases as BR
import quality_mask_cases as Q
import read_filter_cases as R
import subsample_cases as S
from conftest import get_cohort
from varigraph_amd import host, synth, vgmi

pytestmark = pytest.mark.gpu

_TEXT = b"@HD\tVN:1.6\tSO:unsorted\n"
N_FASTQ, N_BAM = 600, 300
SUB = (0.5, 11)


@pytest.fixture(scope="module", params=["cohort_snp", "cohort_k22"], ids=["k27", "k22"])
def gc(request):
    """a committed small graph on the device: odd k, and even k (whose reads' offsets vgmi_readoff.hip makes from the closed-up block)"""
    cohort = get_cohort(request.param)
    g = host.Graph(os.path.join(cohort.dir, "graph.bin.gz"))
    ctx = vgmi.Context(0, buffer_mib=16)
    g.upload(ctx)
    yield g, ctx, cohort
    ctx.close()
    g.close()


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _hap(cohort):
    return _cached(("haps", cohort.meta["name"]), cohort.haplotypes)


def _fastq_case(cohort):
    """600 records, the named cases in front, two of 20 000 bases of which the rule keeps one and drops the other"""
    return _cached(("fastq", cohort.meta["name"]), lambda: R.fastq_records(_hap(cohort), N_FASTQ, 3))


def _bam_case(cohort):
    return _cached(("bam", cohort.meta["name"]), lambda: R.bam_records(_hap(cohort), N_BAM, 3))


def _run(ctx, call):
    ctx.counts_reset()
    r = call()
    return r, ctx.counts_finish(nodes=True, hist=True)


def _want(ctx, cohort, key, call):
    """the plain stream of the passing reads: computed once per graph and case, shared, never changed"""
    return _cached(("want", cohort.meta["name"]) + key, lambda: _run(ctx, call))


def _same_counts(a, b, what):
    for x, y, name in zip(a, b, ("counters", "node counters", "histogram")):
        assert np.array_equal(x, y), (what, name)


def _chunked(monkeypatch, chunk_kb):
    m = monkeypatch.context()
    mp = m.__enter__()
    if chunk_kb:
        mp.setenv("VGMI_FASTQ_CHUNK_KB", str(chunk_kb))
    else:
        mp.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
    return m


def _check(got, want, classes, file_len, what, n_bases=None, masked=None):
    """got: G with the rule; want: G' without"""
    stats = R.class_counts(classes)
    print(f"{what}: kept {got['n_records']}, stats {got['read_filter_stats']} (model {stats}), bases {got['n_bases']}, consumed {got['consumed']}")
    assert not got["stopped"] and not want["stopped"], what
    assert got["read_filter_stats"] == stats, what
    assert (got["n_records"], got["n_bases"]) == (want["n_records"], want["n_bases"]), what
    assert got["n_records"] == stats[0] - sum(stats[1:]) and (n_bases is None or got["n_bases"] == n_bases), what
    assert got["consumed"] == file_len and got["tail"] == b"", what
    assert got["masked_bases"] == (want["masked_bases"] if masked is None else masked), what
    assert "read_filter_stats" not in want


# ---- FASTQ -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.RULES))
def test_fastq_text_equals_counting_the_passing_reads(name, gc, monkeypatch):
    """each of the four tests alone, the two length tests (no quality kernel runs), and all together; plain text, whole and in 4 KiB
    chunks: the 20 000-base records are carried across five chunks, one kept and one dropped by its qualities"""
    g, ctx, cohort = gc
    rule = R.RULES[name]
    recs = _fastq_case(cohort)
    kept, classes = R.fastq_filtered(recs, rule)
    G, GP = R.fastq_text(recs), R.fastq_text(kept)
    want, c_want = _want(ctx, cohort, ("fastq", name), lambda: ctx.fastq_text(GP))
    plain, c_plain = _want(ctx, cohort, ("fastq", "plain"), lambda: ctx.fastq_text(G))
    for chunk_kb in (None, 4):
        m = _chunked(monkeypatch, chunk_kb)
        try:
            got, c_got = _run(ctx, lambda: ctx.fastq_text(G, read_filter=rule.dict()))
        finally:
            m.__exit__(None, None, None)
        _check(got, want, classes, len(G), (name, chunk_kb), sum(len(r[1]) for r in kept))
        _same_counts(c_got, c_want, (name, chunk_kb))
        # the case shows something: the whole file has more reads and (reads shorter than 40 bases hold few k-mers of the graph: not asked
        # of "short") counts differently
        assert plain["n_records"] == len(recs) > got["n_records"] and (name == "short" or not np.array_equal(c_plain[0], c_got[0]))


@pytest.mark.parametrize("name", ["lengths", "all"])
def test_fastq_with_subsampling_keeps_the_numbers(name, gc, monkeypatch):
    """subsample = (0.5, 11) in front of the rule: the reads' numbers do not change, only the kept reads are evaluated -- evaluated is the
    subsample stats' n_kept -- in either setter order"""
    g, ctx, cohort = gc
    rule = R.RULES[name]
    recs = _fastq_case(cohort)
    kept, classes = R.fastq_filtered(recs, rule, SUB)
    G, GP = R.fastq_text(recs), R.fastq_text(kept)
    want, c_want = _want(ctx, cohort, ("fastq_sub", name), lambda: ctx.fastq_text(GP))
    for chunk_kb, first in ((None, False), (4, True)):
        m = _chunked(monkeypatch, chunk_kb)
        try:
            got, c_got = _run(ctx, lambda: ctx.fastq_text(G, subsample=SUB, read_filter=rule.dict(), read_filter_first=first))
        finally:
            m.__exit__(None, None, None)
        _check(got, want, classes, len(G), (name, chunk_kb, "subsample"))
        assert got["n_seen"] == len(recs) and got["n_kept"] == got["read_filter_stats"][0] == int(S.kept_mask(len(recs), *SUB).sum())
        _same_counts(c_got, c_want, (name, chunk_kb, "subsample"))


def test_fastq_with_a_minimum_base_quality(gc, monkeypatch):
    """min_quality = 20: the tests see the file's own qualities, the kept reads are masked, masked_bases counts kept reads only"""
    g, ctx, cohort = gc
    rule = R.ALL
    recs = _fastq_case(cohort)
    kept, classes = R.fastq_filtered(recs, rule)
    masked, total = Q.masked_records(kept, 20)
    assert 0 < total < Q.masked_records(recs, 20)[1]
    G, GP = R.fastq_text(recs), R.fastq_text(masked)
    want, c_want = _want(ctx, cohort, ("fastq_masked",), lambda: ctx.fastq_text(GP))
    for chunk_kb, first in ((None, True), (4, False)):
        m = _chunked(monkeypatch, chunk_kb)
        try:
            got, c_got = _run(ctx, lambda: ctx.fastq_text(G, min_quality=20, read_filter=rule.dict(), read_filter_first=first))
        finally:
            m.__exit__(None, None, None)
        _check(got, want, classes, len(G), ("min_quality", chunk_kb), masked=total)
        _same_counts(c_got, c_want, ("min_quality", chunk_kb))


def test_block_gzip_and_gzip(gc, tmp_path, monkeypatch):
    g, ctx, cohort = gc
    monkeypatch.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
    recs = _fastq_case(cohort)
    kept, classes = R.fastq_filtered(recs, R.ALL)
    G, GP = R.fastq_text(recs), R.fastq_text(kept)
    want, c_want = _want(ctx, cohort, ("fastq", "all"), lambda: ctx.fastq_text(GP))
    src, dst = tmp_path / "g.txt", tmp_path / "g.gz"
    src.write_bytes(G)
    synth.bgzf_compress_file(str(src), str(dst), level=4, block=3000)          # members of 3 000 bytes of text: records lie across members
    comp = dst.read_bytes()
    got, c_got = _run(ctx, lambda: ctx.fastq_bgzf(comp, read_filter=R.ALL.dict()))
    assert not got["inflate_failed"] and got["taken"] == len(comp)
    _check(got, want, classes, len(G), "bgzf")
    _same_counts(c_got, c_want, "bgzf")
    got, c_got = _run(ctx, lambda: ctx.fastq_gzip(gzip.compress(G, 6), read_filter=R.ALL.dict()))
    assert (got["stop"], got["reason"], got["device_text_bytes"]) == (1, 0, len(G))
    _check(got, want, classes, len(G), "gzip")
    _same_counts(c_got, c_want, "gzip")


def test_a_chunk_all_of_whose_reads_are_dropped(gc):
    """commits that end behind a run of records the rule drops: the middle chunk packs nothing, and the stream goes on"""
    g, ctx, cohort = gc
    d = S._Draw(_hap(cohort), 31)
    good = lambda i: (b"g%d" % i, d.seq(151), R._ph([40] * 151))
    bad = [(b"short%d" % i, d.seq(20), R._ph([40] * 20)) if i % 2 else (b"low%d" % i, d.seq(151), R._ph([3] * 151)) for i in range(30)]
    recs = [good(i) for i in range(20)] + bad + [good(100 + i) for i in range(20)]
    kept, classes = R.fastq_filtered(recs, R.ALL)
    assert len(kept) == 40 and R.class_counts(classes) == (70, 15, 0, 15, 0)
    G = R.fastq_text(recs)
    want, c_want = _run(ctx, lambda: ctx.fastq_text(R.fastq_text(kept)))
    a, b = len(R.fastq_text(recs[:20])), len(R.fastq_text(recs[:50]))
    got, c_got = _run(ctx, lambda: ctx.fastq_text(G, piece=[a, b - a, len(G)], read_filter=R.ALL.dict()))
    _check(got, want, classes, len(G), "a chunk of dropped reads")
    _same_counts(c_got, c_want, "a chunk of dropped reads")
    # ... and a stream all of whose reads are dropped
    got, c_got = _run(ctx, lambda: ctx.fastq_text(R.fastq_text(bad), read_filter=R.ALL.dict()))
    assert (got["n_records"], got["n_bases"], got["stopped"], got["read_filter_stats"]) == (0, 0, False, (30, 15, 0, 15, 0))
    assert not c_got[0].any()


def test_first_bad_record_in_a_chunk(gc, tmp_path, monkeypatch):
    """A record with a wrapped sequence in the middle of the file and no final newline.  The records in front of the first bad one are
    filtered on the device -- those of its own chunk too --, nothing at or behind it is evaluated there; the host leg behind it applies
    the same rule and the class counts add up."""
    g, ctx, cohort = gc
    recs = list(_fastq_case(cohort))
    mid = 400
    recs[mid] = recs[mid] + ("wrapped",)
    rule = R.ALL
    kept, classes = R.fastq_filtered(recs, rule)
    G, GP = R.fastq_text(recs, final_newline=False), R.fastq_text(kept)
    # the stream alone, the file in one chunk: the device takes exactly the records in front of the bad one
    monkeypatch.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
    r, c_dev = _run(ctx, lambda: ctx.fastq_text(G, read_filter=rule.dict()))
    n_dev = r["read_filter_stats"][0]
    dev_kept, dev_classes = R.fastq_filtered(recs[:n_dev], rule)
    assert r["stopped"] and n_dev == mid and r["consumed"] == len(R.fastq_text(recs[:n_dev]))
    assert r["read_filter_stats"] == R.class_counts(dev_classes) and r["n_records"] == len(dev_kept)
    _same_counts(c_dev, _run(ctx, lambda: ctx.fastq_text(R.fastq_text(dev_kept)))[1], "the device's share")
    rest = tmp_path / "rest.fq"
    rest.write_bytes(G[r["consumed"]:])
    host_stats = host.reads_read_all_l(str(rest), rule.dict())[7]
    assert tuple(a + b for a, b in zip(r["read_filter_stats"], host_stats)) == R.class_counts(classes)
    # the product path, device and host legs together, against the plain count of G'
    (tmp_path / "g.fq").write_bytes(G)
    (tmp_path / "gp.fq").write_bytes(GP)
    want = _sample(g, ctx, [tmp_path / "gp.fq"], monkeypatch)
    for env in ({"VGMI_FASTQ_CHUNK_KB": "4"}, {}, {"VGH_HOST_PARSE": "1"}):
        got = _sample(g, ctx, [tmp_path / "g.fq"], monkeypatch, rule, env=env)
        assert got[1] == want[1] == (len(kept), sum(len(x[1]) for x in kept)) and got[2] == R.class_counts(classes), env
        _same_counts(got[0], want[0], env)


def _sample(g, ctx, paths, monkeypatch, rule=None, env=None, sub=None, q=0, **kw):
    with monkeypatch.context() as m:
        for k in ("VGH_HOST_PARSE", "VGH_HOST_INFLATE", "VGH_DEVICE_GUNZIP", "VGMI_FASTQ_CHUNK_KB"):
            m.delenv(k, raising=False)
        for k, v in (env or {}).items():
            m.setenv(k, v)
        cov, node, hist, st = g.sample_count(ctx, [str(p) for p in paths], threads=4, require_depth=False, min_base_quality=q, subsample=sub,
                                             read_filter=None if rule is None else rule.dict(), **kw)
    return (cov, node, hist), (st["n_reads"], st["read_base"]), st.get("read_filter_stats"), st


def test_sample_count_through_every_container_and_host_leg(gc, tmp_path, monkeypatch):
    """vgh_sample_count_l on plain, gzip and block-gzip files, through the device and through every host leg, with subsampling: one answer"""
    g, ctx, cohort = gc
    recs = _fastq_case(cohort)
    kept, classes = R.fastq_filtered(recs, R.ALL, SUB)
    G, GP = R.fastq_text(recs), R.fastq_text(kept)
    (tmp_path / "g.fq").write_bytes(G)
    (tmp_path / "g.fq.gz").write_bytes(gzip.compress(G, 6))
    synth.bgzf_compress_file(str(tmp_path / "g.fq"), str(tmp_path / "g.bgz.gz"), level=4, block=0xff00)
    (tmp_path / "gp.fq").write_bytes(GP)
    want = _sample(g, ctx, [tmp_path / "gp.fq"], monkeypatch)
    assert want[2] is None
    for name, env in (("g.fq", {}), ("g.fq.gz", {}), ("g.bgz.gz", {}), ("g.fq", {"VGH_HOST_PARSE": "1"}), ("g.bgz.gz", {"VGH_HOST_INFLATE": "1"}),
                      ("g.fq.gz", {"VGH_DEVICE_GUNZIP": "0"})):
        got = _sample(g, ctx, [tmp_path / name], monkeypatch, R.ALL, env=env, sub=SUB)
        assert got[1] == want[1] and got[2] == R.class_counts(classes), (name, env)
        assert (got[3]["reads_seen"], got[3]["reads_kept"]) == (len(recs), len(kept)), (name, env)
        _same_counts(got[0], want[0], (name, env))


def test_fasta_file_with_length_bounds_is_served_by_the_host(gc, tmp_path, monkeypatch):
    g, ctx, cohort = gc
    recs = _fastq_case(cohort)[:300]
    for width in (None, 60):
        for name in ("lengths", "all"):
            rule = R.RULES[name]
            kept, classes = R.fasta_filtered(recs, rule)
            (tmp_path / "g.fa").write_bytes(S.fasta_text(recs, width))
            (tmp_path / "gp.fa").write_bytes(S.fasta_text(kept, width))
            want = _sample(g, ctx, [tmp_path / "gp.fa"], monkeypatch)
            got = _sample(g, ctx, [tmp_path / "g.fa"], monkeypatch, rule)
            assert got[1] == want[1] == (len(kept), sum(len(r[1]) for r in kept)) and got[2] == R.class_counts(classes), (width, name)
            assert 0 < got[2][1] and 0 < got[2][2]
            _same_counts(got[0], want[0], (width, name))
    # quality-only parameters: the device FASTA parser serves the file as it would without them
    got = _sample(g, ctx, [tmp_path / "g.fa"], monkeypatch, R.RULES["mean"])
    plain = _sample(g, ctx, [tmp_path / "g.fa"], monkeypatch)
    assert got[1] == plain[1] == (len(recs), sum(len(r[1]) for r in recs)) and got[2] == (len(recs), 0, 0, 0, 0)
    _same_counts(got[0], plain[0], "quality-only on FASTA")


# ---- BAM ---------------------------------------------------------------------------------------------------------------------------------
def _bam_streams(tmp_path, recs, gp):
    """(G, G', header length, decompressed length of G): block gzip with members of 3 000 bytes of text, records lie across members"""
    hlen, _ = B.write_bam(tmp_path / "g.bam", recs, text=_TEXT, block=3000)
    B.write_bam(tmp_path / "gp.bam", gp, text=_TEXT, block=3000)
    return (tmp_path / "g.bam").read_bytes(), (tmp_path / "gp.bam").read_bytes(), hlen, len(B.raw_bam(recs, text=_TEXT)[0])


@pytest.mark.parametrize("name", list(R.RULES))
def test_bam_equals_counting_the_passing_reads(name, gc, tmp_path, monkeypatch):
    """300 reads with non-reads between them, in 64 KiB chunks: QUAL 0, 93, 94 and 254, records without qualities, 20 000 and 20 001 bases"""
    g, ctx, cohort = gc
    rule = R.RULES[name]
    recs = _bam_case(cohort)
    gp, classes, n_reads = R.bam_filtered(recs, rule)
    comp, comp_p, hlen, raw_len = _bam_streams(tmp_path, recs, gp)
    m = _chunked(monkeypatch, 64)
    try:
        want, c_want = _want(ctx, cohort, ("bam", name), lambda: ctx.bam_bgzf(comp_p, hlen, 0))
        plain, c_plain = _want(ctx, cohort, ("bam", "plain"), lambda: ctx.bam_bgzf(comp, hlen, 0))
        got, c_got = _run(ctx, lambda: ctx.bam_bgzf(comp, hlen, 0, read_filter=rule.dict()))
    finally:
        m.__exit__(None, None, None)
    assert not got["inflate_failed"] and n_reads == N_BAM == plain["n_records"]
    _check(got, want, classes, raw_len, name, B.reads_block(gp)[2])
    _same_counts(c_got, c_want, name)
    assert got["n_records"] < N_BAM and (name == "short" or not np.array_equal(c_plain[0], c_got[0]))


def test_bam_with_subsampling_and_a_minimum_base_quality(gc, tmp_path, monkeypatch):
    g, ctx, cohort = gc
    recs = _bam_case(cohort)
    gp, classes, n_reads = R.bam_filtered(recs, R.ALL, SUB)
    masked, total = Q.masked_bam_records(gp, 20)
    assert total > 0
    comp, comp_p, hlen, raw_len = _bam_streams(tmp_path, recs, masked)
    m = _chunked(monkeypatch, 64)
    try:
        want, c_want = _run(ctx, lambda: ctx.bam_bgzf(comp_p, hlen, 0))
        for first in (False, True):
            got, c_got = _run(ctx, lambda: ctx.bam_bgzf(comp, hlen, 0, min_quality=20, subsample=SUB, read_filter=R.ALL.dict(), read_filter_first=first))
            _check(got, want, classes, raw_len, ("bam", "subsample + min_quality", first), masked=total)
            assert got["n_seen"] == n_reads and got["n_kept"] == got["read_filter_stats"][0] == int(S.kept_mask(n_reads, *SUB).sum())
            _same_counts(c_got, c_want, ("bam", "subsample + min_quality", first))
    finally:
        m.__exit__(None, None, None)


def _placed_records(haps, n=300, fault_at=None):
    """records with a reference and a position, flags the filter drops, a qs tag around the bound, qualities of the four kinds"""
    d = F.Draw(77, haps)
    rng = np.random.default_rng(78)
    out = []
    for i in range(n):
        ln = 20 + i % 30 if i % 9 == 4 else 120 + i % 40
        flag = (0x400 if i % 7 == 3 else 0) | (0x10 if i % 2 else 0) | (0x100 if i % 11 == 5 else 0)
        kind = (0, 0, 1, 0, 2, 0, 3, 0)[i % 8]
        aux = F.aux(b"NM", "C", 1) + F.fault("type") if i == fault_at else F.aux(b"qs", "C", 30 if i % 5 else 5)
        pos = int(rng.integers(0, 3000))
        out.append(B.Rec(b"p%d" % i, d.seq(ln), flag=flag, ref=i % 2, pos=100 if i == fault_at else pos, mapq=60 if i % 6 else 3,
                         cigar=[(ln, "M")], qual=bytes(R.drawn_quality(rng, ln, kind)), aux=aux))
    return out


@pytest.mark.parametrize("fault_at", [None, 200], ids=["no_fault", "walk_fault"])
def test_bam_behind_a_flag_filter_a_tag_bound_and_regions(fault_at, gc, monkeypatch):
    """the rule runs on the reads the record filter leaves: flags, MAPQ, a tag bound and a region list in front of it, with subsampling
    between.  With a walk fault the device stops at the faulted record's first byte and nothing at or behind it is evaluated."""
    g, ctx, cohort = gc
    recs = _placed_records(_hap(cohort), 300, fault_at)
    f = F.Filter(exclude=0xD00, min_mapq=10, tag=b"qs", min_value=10)
    regions = [(0, 0, 1500), (1, 500, 2600)]
    passing, n_rec, n_reads, at = BR.apply(recs, f, regions)
    assert at == fault_at and 40 < n_reads < n_rec
    for sub in (None, SUB):
        gp, classes, seen = R.bam_filtered(passing, R.ALL, sub)
        stats = R.class_counts(classes)
        assert seen == n_reads and stats[0] > sum(stats[1:]) > 0 and stats[3] > 0 and stats[4] > 0
        case = BC.Case("read_filter", "read_filter", recs, refs=BR.REFS, text=_TEXT)
        oracle = BC.Case("read_filter_gp", "read_filter", gp, refs=BR.REFS, text=_TEXT)
        want, c_want = _run(ctx, lambda: ctx.bam_bgzf(oracle.comp, oracle.hlen, oracle.n_ref, piece=oracle.piece))
        got, c_got = _run(ctx, lambda: ctx.bam_bgzf(case.comp, case.hlen, case.n_ref, piece=case.piece, bam_filter=f.dict(), bam_regions=regions,
                                                    subsample=sub, read_filter=R.ALL.dict()))
        print(fault_at, sub, got["n_records"], got["read_filter_stats"], stats, got["bam_records"], got["bam_reads"], got["consumed"], got["stopped"])
        assert got["stopped"] == (fault_at is not None) and got["consumed"] == (len(case.raw) if fault_at is None else case.offs[fault_at])
        assert (got["bam_records"], got["bam_reads"]) == (n_rec, n_reads) and got["read_filter_stats"] == stats
        assert (got["n_records"], got["n_bases"]) == (want["n_records"], want["n_bases"]) == B.reads_block(gp)[1:]
        if sub:
            assert got["n_seen"] == n_reads and got["n_kept"] == stats[0]
        _same_counts(c_got, c_want, (fault_at, sub))


def test_bam_hand_over_to_the_host_decoder(gc, tmp_path, monkeypatch):
    """a BAM file through vgh_sample_count_l: the device alone, whole and in 64 KiB chunks, and the host decoder alone"""
    g, ctx, cohort = gc
    recs = _bam_case(cohort)
    gp, classes, n_reads = R.bam_filtered(recs, R.ALL, SUB)
    B.write_bam(tmp_path / "g.bam", recs, text=_TEXT)
    B.write_bam(tmp_path / "gp.bam", gp, text=_TEXT)
    want = _sample(g, ctx, [tmp_path / "gp.bam"], monkeypatch)
    for env in ({}, {"VGH_HOST_PARSE": "1"}, {"VGH_HOST_INFLATE": "1"}, {"VGMI_FASTQ_CHUNK_KB": "64"}):
        got = _sample(g, ctx, [tmp_path / "g.bam"], monkeypatch, R.ALL, env=env, sub=SUB)
        assert got[1] == want[1] and got[2] == R.class_counts(classes), env
        assert (got[3]["reads_seen"], got[3]["reads_kept"]) == (n_reads, want[1][0]), env
        _same_counts(got[0], want[0], env)


# ---- the refusals and the all-default call -------------------------------------------------------------------------------------------------
def test_setter_refusals_leave_the_stream_serving(gc):
    g, ctx, cohort = gc
    l = ctx._l
    recs = _fastq_case(cohort)
    kept, classes = R.fastq_filtered(recs, R.ALL)
    G = R.fastq_text(recs)
    _, c_want = _want(ctx, cohort, ("fastq", "all"), lambda: ctx.fastq_text(R.fastq_text(kept)))
    bad_fields = ((dict(min_len=10, max_len=9), "below the minimum read length"), (dict(min_mean_q=931), "0..930"),
                  (dict(lowq_below=94, lowq_max_pct=10), "0..93, Phred"), (dict(lowq_below=10, lowq_max_pct=101), "0..100"),
                  (dict(lowq_max_pct=10), "needs a low-quality bound"))
    for bad, what in bad_fields:
        with pytest.raises(vgmi.VgmiError) as e:
            ctx.fastq_text(G, read_filter=bad)
        assert e.value.code == vgmi.E_INVALID and what in str(e.value)
    ctx.counts_reset()
    fq = C.c_void_p()
    assert l.vgmi_fastq_open(ctx._h, C.byref(fq)) == 0
    for bad, what in bad_fields:
        assert l.vgmi_fastq_set_read_filter(fq, C.byref(vgmi.read_filter_struct(bad))) == vgmi.E_INVALID
        assert what.encode() in l.vgmi_last_error(ctx._h)
    assert l.vgmi_fastq_set_read_filter(fq, None) == vgmi.E_INVALID
    assert l.vgmi_fastq_set_read_filter(fq, C.byref(vgmi.read_filter_struct(R.ALL.dict()))) == 0          # a valid call after the refusals
    half = len(R.fastq_text(recs[:len(recs) // 2]))
    v = [C.c_uint64() for _ in range(5)]
    for lo, hi in ((0, half), (half, len(G))):
        buf, cap = C.c_void_p(), C.c_size_t()
        assert l.vgmi_fastq_acquire(fq, C.byref(buf), C.byref(cap)) == 0
        C.memmove(buf, G[lo:hi], hi - lo)
        assert l.vgmi_fastq_commit(fq, hi - lo) == 0
        assert l.vgmi_fastq_set_read_filter(fq, C.byref(vgmi.read_filter_struct(dict(min_len=5)))) == vgmi.E_STATE         # bytes have been committed
        assert l.vgmi_fastq_set_read_filter(fq, C.byref(vgmi.read_filter_struct({}))) == vgmi.E_STATE
        assert l.vgmi_fastq_read_filter_stats(fq, *[C.byref(x) for x in v]) == 0       # ... and the stream serves on
    assert tuple(x.value for x in v) == R.class_counts(classes)
    nr, nb, cons, st = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    assert l.vgmi_fastq_close(fq, C.byref(nr), C.byref(nb), C.byref(cons), C.byref(st), None, 0, None) == 0
    assert (nr.value, nb.value, cons.value, st.value) == (len(kept), sum(len(r[1]) for r in kept), len(G), 0)
    _same_counts(ctx.counts_finish(nodes=True, hist=True), c_want, "the rule set before the refused calls holds")
    # a FASTA stream refuses length bounds with its own message, accepts quality-only fields without effect, and serves on
    fa = S.fasta_text(recs[:100])
    plain, c_plain = _run(ctx, lambda: ctx.fasta_text(fa))
    for bad in (dict(min_len=40), dict(max_len=500), R.ALL.dict()):
        with pytest.raises(vgmi.VgmiError) as e:
            ctx.fasta_text(fa, read_filter=bad)
        assert e.value.code == vgmi.E_INVALID and "FASTA stream takes no read-length bounds" in str(e.value)
    ctx.counts_reset()
    fq = C.c_void_p()
    assert l.vgmi_fastq_open_fasta(ctx._h, C.byref(fq)) == 0
    assert l.vgmi_fastq_set_read_filter(fq, C.byref(vgmi.read_filter_struct(dict(min_len=40)))) == vgmi.E_INVALID
    assert l.vgmi_fastq_close(fq, None, None, None, None, None, 0, None) == 0
    ctx.counts_finish()
    got, c_got = _run(ctx, lambda: ctx.fasta_text(fa, read_filter=[R.RULES["mean"].dict(), R.RULES["fraction"].dict()]))
    assert got.pop("read_filter_stats") == (plain["n_records"], 0, 0, 0, 0) and got == plain
    _same_counts(c_got, c_plain, "quality-only on a FASTA stream")
    # the product entry refuses the same fields
    for bad, what in bad_fields:
        with pytest.raises(vgmi.VgmiError, match=re.escape(what)):
            g.sample_count(ctx, [os.path.join(cohort.dir, "reads_1.fq.gz")], read_filter=bad)


def test_all_default_call_is_the_stream_of_no_call(gc, tmp_path, monkeypatch):
    g, ctx, cohort = gc
    recs = _fastq_case(cohort)
    G = R.fastq_text(recs)
    brecs = _bam_case(cohort)
    comp, _, hlen, _ = _bam_streams(tmp_path, brecs, brecs)
    for chunk_kb in (None, 4):
        m = _chunked(monkeypatch, chunk_kb)
        try:
            plain, c_plain = _run(ctx, lambda: ctx.fastq_text(G))
            none, c_none = _run(ctx, lambda: ctx.fastq_text(G, read_filter={}))
            back, c_back = _run(ctx, lambda: ctx.fastq_text(G, read_filter=[R.ALL.dict(), {}]))      # the last value set holds
            on, c_on = _run(ctx, lambda: ctx.fastq_text(G, read_filter=[{}, R.ALL.dict()]))
        finally:
            m.__exit__(None, None, None)
        for r, c in ((none, c_none), (back, c_back)):
            assert r.pop("read_filter_stats") == (len(recs), 0, 0, 0, 0)
            assert r == plain
            _same_counts(c, c_plain, "all default")
        assert on["n_records"] < len(recs) and not np.array_equal(c_on[0], c_plain[0])
    plain, c_plain = _run(ctx, lambda: ctx.bam_bgzf(comp, hlen, 0))
    none, c_none = _run(ctx, lambda: ctx.bam_bgzf(comp, hlen, 0, read_filter=[R.ALL.dict(), {}]))
    assert none.pop("read_filter_stats") == (N_BAM, 0, 0, 0, 0) and none == plain
    _same_counts(c_none, c_plain, "all default, BAM")
    got = g.sample_count(ctx, [os.path.join(cohort.dir, "reads_1.fq.gz")], require_depth=False, read_filter={})
    assert got[3]["n_reads"] == cohort.n_reads // 2 and got[3]["read_filter_stats"] == (cohort.n_reads // 2, 0, 0, 0, 0)
