"""The BAM read filter on the device (bam_keep_filter_kernel, bam_cut_kernel, the filter forms of the finish kernel; csrc/vgmi_bam.hip)
through Context.bam_bgzf and the C ABI.  The oracle throughout: the filtered stream equals the unfiltered stream of a BAM holding
only the passing records, as the Python model of bam_filter_cases.py names them -- counters, per-node counters, histogram,
n_records, n_bases; consumed stays the file's bytes.  tests/test_bam_filter_cpu.py checks the model against the rule's C++."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import bam_cases as BC
import bam_filter_cases as F
import bam_py as B
import quality_mask_cases as Q
import subsample_cases as S
from conftest import get_cohort
from varigraph_amd import host, vgmi

pytestmark = pytest.mark.gpu

_TEXT = b"@HD\tVN:1.6\tSO:unsorted\n"
PLACES = ("first", "middle", "chunk_last", "carried")


@pytest.fixture(scope="module")
def gc():
    cohort = get_cohort("cohort_snp")
    g = host.Graph(os.path.join(cohort.dir, "graph.bin.gz"))
    ctx = vgmi.Context(0, buffer_mib=16)
    g.upload(ctx)
    yield g, ctx, cohort.haplotypes()
    ctx.close()
    g.close()


def _run(ctx, call):
    ctx.counts_reset()
    r = call()
    return r, ctx.counts_finish(nodes=True, hist=True)


def _same_counts(a, b, what):
    for x, y, name in zip(a, b, ("counters", "node counters", "histogram")):
        assert np.array_equal(x, y), (what, name)


def _case(recs, cuts=()):
    return BC.Case("bam_filter", "bam_filter", recs, refs=(), cuts=cuts, text=_TEXT)


def _stream(ctx, recs, cuts=(), **kw):
    c = _case(recs, cuts)
    r, counts = _run(ctx, lambda: ctx.bam_bgzf(c.comp, c.hlen, c.n_ref, piece=c.piece, **kw))
    return r, counts, c


def _check(ctx, recs, f, what, cuts=(), want=None, **kw):
    """recs under filter f == the model's passing records under the default filter"""
    passing, n_rec, n_reads, at = F.apply(recs, f)
    assert at is None, what
    got, c_got, case = _stream(ctx, recs, cuts, bam_filter=f.dict(), **kw)
    want = want or _stream(ctx, passing)[:2]
    print(f"{what}: {got['bam_reads']} of {got['bam_records']} records are reads (model {n_reads} of {n_rec}), bases {got['n_bases']}")
    assert not got["stopped"] and not got["inflate_failed"] and got["tail"] == b"", what
    assert (got["bam_records"], got["bam_reads"]) == (n_rec, n_reads) == (len(recs), len(passing)), what
    assert (got["n_records"], got["n_bases"]) == (want[0]["n_records"], want[0]["n_bases"]) == B.reads_block(passing)[1:], what
    assert got["consumed"] == len(case.raw), what
    _same_counts(c_got, want[1], what)
    return got, c_got, want


# ---- 1: flags and MAPQ ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flag_recs(gc):
    return F.flag_records(2000, haps=gc[2])


@pytest.mark.parametrize("name", list(F.FLAG_FILTERS))
def test_flag_and_mapq_rules(name, gc, flag_recs, tmp_path, monkeypatch):
    """2 000 records with drawn flags and MAPQ, SEQ '*' among them: in one chunk, and as members of 3 000 bytes in 4 KiB chunks"""
    g, ctx, _ = gc
    f = F.FLAG_FILTERS[name]
    got, c_got, want = _check(ctx, flag_recs, f, name)
    plain, c_plain, _ = _stream(ctx, flag_recs)
    assert not np.array_equal(c_plain[0], c_got[0]) and plain["n_records"] != got["n_records"] and "bam_records" not in plain
    passing = F.apply(flag_recs, f)[0]
    hlen, _ = B.write_bam(tmp_path / "g.bam", flag_recs, text=_TEXT, block=3000)
    comp = (tmp_path / "g.bam").read_bytes()
    with monkeypatch.context() as m:
        m.setenv("VGMI_FASTQ_CHUNK_KB", "4")
        small, c_small = _run(ctx, lambda: ctx.bam_bgzf(comp, hlen, 0, bam_filter=f.dict()))
    assert (small["n_records"], small["n_bases"], small["bam_records"], small["bam_reads"], small["stopped"]) == \
        (len(passing), got["n_bases"], len(flag_recs), len(passing), False)
    _same_counts(c_small, want[1], (name, "4 KiB chunks"))


# ---- 2: the tag bound -------------------------------------------------------------------------------------------------------------------------
def test_tag_bound_over_every_type(gc):
    """the tag in every type, absent, non-numeric, twice, behind a 4 KiB B:C array and a 300-byte Z; the bound equals a value present"""
    g, ctx, haps = gc
    recs = F.tag_records(haps=haps)
    f = F.Filter(tag=b"qs", min_value=10.0)
    assert any(F.verdict(r, f) == (F.READ, 10.0) for r in recs)
    got, _, _ = _check(ctx, recs, f, "qs>=10")
    assert 0 < got["n_records"] < len(recs)
    _check(ctx, recs, F.Filter(tag=b"qs", min_value=float("-inf")), "qs>=-inf")
    last = F.Filter(exclude=0, tag=b"ZZ", min_value=5)
    one = [r for r in recs if F.verdict(r, last)[0] != F.FAULT]      # (the records whose fault lies behind qs: ZZ's walk meets it)
    assert len(one) > len(recs) - 30
    _check(ctx, one, last, "ZZ>=5, the record's last field")


def test_rq_float_at_the_bound(gc):
    g, ctx, haps = gc
    recs = F.rq_records(haps=haps)
    f = F.Filter(tag=b"rq", min_value=0.99)
    assert F.verdict(recs[0], f)[0] == F.READ and F.verdict(recs[1], f)[0] == F.DROP      # 0.99f passes, the float just below does not
    got, _, _ = _check(ctx, recs, f, "rq>=0.99")
    assert 2 < got["n_records"] < len(recs) - 2


# ---- 3: walk faults ---------------------------------------------------------------------------------------------------------------------------
def _sample(g, ctx, path, monkeypatch, f=None, env=None, sub=None, q=0):
    with monkeypatch.context() as m:
        for k in ("VGH_HOST_PARSE", "VGH_HOST_INFLATE", "VGMI_FASTQ_CHUNK_KB"):
            m.delenv(k, raising=False)
        for k, v in (env or {}).items():
            m.setenv(k, v)
        try:
            cov, node, hist, st = g.sample_count(ctx, [str(path)], threads=4, require_depth=False, min_base_quality=q, subsample=sub,
                                                 bam_filter=None if f is None else f.dict())
        except vgmi.VgmiError as e:
            return str(e)
    return (cov, node, hist), (st["n_reads"], st["read_base"]), (st.get("bam_records"), st.get("bam_reads")), st


@pytest.mark.parametrize("where", PLACES)
@pytest.mark.parametrize("kind", F.FAULTS)
def test_a_faulted_record_stops_the_device_at_its_first_byte(kind, where, gc, tmp_path, monkeypatch):
    g, ctx, haps = gc
    recs, at = F.faulted(kind, "first" if where == "first" else "middle", haps=haps)
    f = F.Filter(tag=b"qs", min_value=10)
    offs = _case(recs).offs
    cuts = {"first": (), "middle": (), "chunk_last": [offs[at + 1]], "carried": [offs[at] + 20]}[where]
    front, n_rec, n_reads, model_at = F.apply(recs, f)
    assert model_at == at and n_rec == at
    got, c_got, case = _stream(ctx, recs, cuts, bam_filter=f.dict())
    want, c_want, _ = _stream(ctx, front)
    print(kind, where, got["n_records"], got["consumed"], got["stopped"], got["bam_records"], got["bam_reads"])
    assert got["stopped"] and got["consumed"] == offs[at] and got["tail"] == b"" and not got["inflate_failed"]
    assert (got["n_records"], got["n_bases"]) == (want["n_records"], want["n_bases"]) == B.reads_block(front)[1:]
    assert (got["bam_records"], got["bam_reads"]) == (at, n_reads)
    _same_counts(c_got, c_want, (kind, where))
    assert where == "first" or got["n_records"] > 0
    # the product path: the host decoder takes over there and names the record
    p = tmp_path / "a.bam"
    p.write_bytes(case.comp)
    err = _sample(g, ctx, p, monkeypatch, f)
    assert isinstance(err, str) and f"'{p}': not a valid BAM record at decompressed byte {offs[at]} (auxiliary fields)" in err, err
    # no stop where nothing walks that far: the tag in front of the fault, or the record failing 1 to 4
    seen = list(recs)
    seen[at] = B.Rec(b"seen", recs[at].seq, flag=0, mapq=60, qual=recs[at].qual, aux=F.aux(b"qs", "C", 30) + recs[at].aux)
    _check(ctx, seen, f, (kind, where, "behind the tag"), cuts=cuts)
    unwalked = list(recs)
    unwalked[at] = B.Rec(b"dup", recs[at].seq, flag=0x400, mapq=60, qual=recs[at].qual, aux=recs[at].aux)
    _check(ctx, unwalked, F.Filter(exclude=0xD00, tag=b"qs", min_value=10), (kind, where, "fails the flags"), cuts=cuts)


def test_two_faults_in_one_chunk_stop_at_the_first(gc):
    g, ctx, haps = gc
    recs, at = F.faulted("type", "middle", haps=haps, n=600)
    recs[at + 200] = recs[at]
    recs[at - 5] = B.Rec(b"x", recs[at].seq, flag=0x100, aux=F.fault("nonul"))      # fails the flags: not walked
    f = F.Filter(tag=b"qs", min_value=10)
    front = F.apply(recs, f)[0]
    got, c_got, case = _stream(ctx, recs, bam_filter=f.dict())
    want, c_want, _ = _stream(ctx, front)
    assert got["stopped"] and got["consumed"] == case.offs[at] and (got["bam_records"], got["bam_reads"]) == (at, len(front))
    assert got["n_records"] == want["n_records"] == len(front) > 0
    _same_counts(c_got, c_want, "two faults")


# ---- 4: every chunk-end alignment ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("passing", "filtered"))
def test_split_at_every_chunk_end_alignment(which, gc):
    """one record sequence cut in two at every alignment of bam_cases.SWEEP; the record at the boundary passes the filter or does not"""
    g, ctx, haps = gc
    d = F.Draw(21, haps)
    recs = [d.rec(flag=(0, 0x400, 0x100, 4)[i % 4], mapq=(60, 3)[i % 5 == 0], aux=F.aux(b"RG", "Z", b"g") + F.aux(b"qs", "C", 5 + i % 20))
            for i in range(40)]
    f = F.Filter(exclude=0xD00, min_mapq=10, tag=b"qs", min_value=10)
    at = next(j for j in range(12, 40) if (F.verdict(recs[j], f)[0] == F.READ) == (which == "passing"))
    passing = F.apply(recs, f)[0]
    want = _stream(ctx, passing)[:2]
    offs = _case(recs).offs
    for dd in BC.SWEEP:
        _check(ctx, recs, f, (which, dd), cuts=[offs[at] - dd], want=want)


# ---- 5: with the other two options ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,sub_first", list(itertools.product((0, 1, 2), (False, True))))
def test_filter_then_number_then_mask_in_every_setter_order(order, sub_first, gc, flag_recs):
    g, ctx, _ = gc
    recs = flag_recs[:600]
    f = F.Filter(exclude=0xF00, min_mapq=20)
    passing, n_rec, n_reads, _ = F.apply(recs, f)
    kept, seen = S.bam_filtered(passing, 0.5, 11)
    masked, total = Q.masked_bam_records(kept, 20)
    got, c_got, _ = _stream(ctx, recs, bam_filter=f.dict(), subsample=(0.5, 11), min_quality=20, subsample_first=sub_first, filter_order=order)
    # the oracle: the kept reads with their masked bases as N, through a stream with no option at all
    want, c_want, _ = _stream(ctx, masked)
    assert (got["n_records"], got["n_bases"], got["masked_bases"]) == (len(kept), want["n_bases"], total) and total > 0
    assert (got["n_seen"], got["n_kept"], got["bam_records"], got["bam_reads"]) == (n_reads, len(kept), n_rec, n_reads) and seen == n_reads
    assert 0 < len(kept) < n_reads < n_rec
    _same_counts(c_got, c_want, (order, sub_first))


# ---- 6: stats and refusals ---------------------------------------------------------------------------------------------------------------------
def test_setter_refusals_leave_the_stream_serving(gc, flag_recs):
    g, ctx, haps = gc
    l = ctx._l
    recs = flag_recs[:400]
    f = F.Filter(exclude=0xF00, min_mapq=20)
    passing, n_rec, n_reads, _ = F.apply(recs, f)
    want, c_want, _ = _stream(ctx, passing)
    case = _case(recs)
    ctx.counts_reset()
    fq = C.c_void_p()
    assert l.vgmi_fastq_open_bam(ctx._h, case.hlen, 0, C.byref(fq)) == 0
    rec_n, read_n = C.c_uint64(), C.c_uint64()
    assert l.vgmi_fastq_bam_filter_stats(fq, C.byref(rec_n), C.byref(read_n)) == vgmi.E_STATE      # no filter yet
    for bad in ((0x10000, 0, 0, None, 0.0), (0, 0x10000, 0, None, 0.0), (0, 0, 256, None, 0.0), (0x900, 0, 0, b"1q", 0.0), (0x900, 0, 0, b"q_", 0.0),
                (0x900, 0, 0, b"\0\0", 0.0), (0x900, 0, 0, b"qs", float("nan"))):
        assert l.vgmi_fastq_set_bam_filter(fq, *bad) == vgmi.E_INVALID, bad
        assert b"BAM" in l.vgmi_last_error(ctx._h)
    assert l.vgmi_fastq_set_bam_filter(fq, 0x400, 0, 0, b"rq", 0.5) == 0
    assert l.vgmi_fastq_set_bam_filter(fq, f.exclude, f.require, f.min_mapq, None, 0.0) == 0      # the last value set holds
    data, pos = case.comp, 0
    while pos < len(data):
        buf, cap = C.c_void_p(), C.c_size_t()
        assert l.vgmi_fastq_acquire(fq, C.byref(buf), C.byref(cap)) == 0
        n = min(cap.value, len(data) - pos)
        C.memmove(buf, data[pos:pos + n], n)
        taken = C.c_size_t()
        assert l.vgmi_fastq_commit_bgzf(fq, n, C.byref(taken), None, None) == 0 and taken.value > 0
        pos += taken.value
        assert l.vgmi_fastq_set_bam_filter(fq, 0x900, 0, 0, None, 0.0) == vgmi.E_STATE      # bytes have been committed
        assert l.vgmi_fastq_bam_filter_stats(fq, C.byref(rec_n), C.byref(read_n)) == 0      # ... and the stream serves on
    assert (rec_n.value, read_n.value) == (n_rec, n_reads)
    nr, nb, cons, st = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    assert l.vgmi_fastq_close(fq, C.byref(nr), C.byref(nb), C.byref(cons), C.byref(st), None, 0, None) == 0
    assert (nr.value, nb.value, cons.value, st.value) == (want["n_records"], want["n_bases"], len(case.raw), 0)
    _same_counts(ctx.counts_finish(nodes=True, hist=True), c_want, "the filter set after the refused calls holds")
    # a refusal through the wrapper, then a valid run on the same context
    with pytest.raises(vgmi.VgmiError) as e:
        ctx.bam_bgzf(case.comp, case.hlen, 0, bam_filter=dict(min_mapq=300))
    assert e.value.code == vgmi.E_INVALID
    _check(ctx, recs, f, "after a refusal")


def test_all_default_call_is_the_stream_of_no_call(gc, flag_recs):
    g, ctx, haps = gc
    recs = flag_recs[:400]
    none, c_none, _ = _stream(ctx, recs)
    dflt, c_dflt, _ = _stream(ctx, recs, bam_filter=dict())
    back, c_back, _ = _stream(ctx, recs, bam_filter=[dict(exclude=0xF00, tag=b"qs", min_value=3.0), dict(exclude=0x900)])
    for r, c in ((dflt, c_dflt), (back, c_back)):
        assert r["filter_stats_rc"] == vgmi.E_STATE and r["bam_records"] is None
        assert {k: v for k, v in r.items() if k in none} == none
        _same_counts(c, c_none, "all defaults")
    assert none["n_records"] == B.reads_block(recs)[1]


def test_fastq_and_fasta_streams_accept_the_call_without_effect(gc):
    g, ctx, haps = gc
    recs = S.fastq_records(haps, 120, 3)
    strict = dict(exclude=0xFFFF, require=0xFFFF, min_mapq=255, tag=b"rq", min_value=1e300)
    for text, call in ((S.fastq_text(recs), ctx.fastq_text), (S.fasta_text(recs), ctx.fasta_text)):
        a, c_a = _run(ctx, lambda: call(text))
        b, c_b = _run(ctx, lambda: call(text, bam_filter=strict))
        assert b["filter_stats_rc"] == vgmi.E_STATE and {k: v for k, v in b.items() if k in a} == a and a["n_records"] >= len(recs) - 1
        _same_counts(c_a, c_b, call.__name__)


# ---- 7: the hand-over ---------------------------------------------------------------------------------------------------------------------------
def test_hand_over_to_the_host_decoder_keeps_the_filter(gc, tmp_path, monkeypatch):
    """64 KiB chunks and, in the middle, a record longer than the 1 MiB carry: the device stops there, the host decoder goes on with
    the same filter.  The device path equals the host reader alone (VGH_HOST_PARSE=1), and VGH_HOST_INFLATE=1."""
    g, ctx, haps = gc
    d = F.Draw(31, haps)
    recs = [d.rec(flag=(0, 0x400, 4, 0x200)[i % 4], mapq=(60, 0)[i % 7 == 0], aux=F.aux(b"qs", "C", 5 + i % 20)) for i in range(900)]
    recs[450] = d.rec(aux=F.aux(b"XB", "B", bytes(BC.TAIL_MAX), "C") + F.aux(b"qs", "C", 30))
    f = F.Filter(exclude=0xF00, min_mapq=1, tag=b"qs", min_value=10)
    passing, n_rec, n_reads, at = F.apply(recs, f)
    assert at is None and recs[450].seq in [r.seq for r in passing]
    B.write_bam(tmp_path / "g.bam", recs, text=_TEXT)
    B.write_bam(tmp_path / "gp.bam", passing, text=_TEXT)
    alone = _sample(g, ctx, tmp_path / "g.bam", monkeypatch, f, env={"VGH_HOST_PARSE": "1"})
    want = _sample(g, ctx, tmp_path / "gp.bam", monkeypatch, env={"VGH_HOST_PARSE": "1"})
    assert alone[1] == want[1] == B.reads_block(passing)[1:] and alone[2] == (n_rec, n_reads) and want[2] == (None, None)
    _same_counts(alone[0], want[0], "the host reader alone")
    for env in ({"VGMI_FASTQ_CHUNK_KB": "64"}, {}, {"VGH_HOST_INFLATE": "1"}):
        got = _sample(g, ctx, tmp_path / "g.bam", monkeypatch, f, env=env)
        assert got[1] == alone[1] and got[2] == (n_rec, n_reads), env
        _same_counts(got[0], alone[0], env)
    # the device's share: it stops at the long record with the records in front of it filtered
    with monkeypatch.context() as m:
        m.setenv("VGMI_FASTQ_CHUNK_KB", "64")
        c = _case(recs)
        r, _ = _run(ctx, lambda: ctx.bam_bgzf(c.comp, c.hlen, 0, bam_filter=f.dict()))
    front = F.apply(recs[:450], f)
    assert r["stopped"] and r["consumed"] == c.offs[450] and (r["bam_records"], r["bam_reads"], r["n_records"]) == (450, front[2], front[2])
    # with the other two options through the product path
    kept, _ = S.bam_filtered(passing, 0.5, 11)
    B.write_bam(tmp_path / "gk.bam", Q.masked_bam_records(kept, 20)[0], text=_TEXT)
    want = _sample(g, ctx, tmp_path / "gk.bam", monkeypatch)
    for env in ({"VGMI_FASTQ_CHUNK_KB": "64"}, {"VGH_HOST_PARSE": "1"}):
        got = _sample(g, ctx, tmp_path / "g.bam", monkeypatch, f, env=env, sub=(0.5, 11), q=20)
        assert got[1] == want[1] and got[2] == (n_rec, n_reads) and (got[3]["reads_seen"], got[3]["reads_kept"]) == (n_reads, len(kept)), env
        _same_counts(got[0], want[0], env)
