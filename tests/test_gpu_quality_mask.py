"""The minimum base quality on the device (-m gpu): fq_pack_mask_kernel / bam_decode_mask_kernel and everything above them.

The oracle is the rule itself: counting file F with bound Q must equal counting F' with the option off, F' = F with exactly the bases
below the bound written as N (quality_mask_cases.py).  Counters, node counters, histogram, records, bases and consumed bytes are
compared, masked_bases against the model's count, and every record must have been taken by the DEVICE (stopped False, n_records all of
them), so that the host reader's masking cannot make these tests green.  Then the hand-overs, where device and host share a file, the
refusals, and the CLI against the unmodified reference run on F'."""
import gzip
import os
import threading

import ctypes as C
import numpy as np
import pytest

import bam_py as B
import quality_mask_cases as Q
from conftest import GOLDEN, get_cohort
from varigraph_amd import host, synth, vgmi

pytestmark = pytest.mark.gpu

_TEXT = b"@HD\tVN:1.6\tSO:unsorted\n"
ALL_Q = (0,) + Q.QS


def _arg(q):
    """min_quality for bound q.  The wrappers do not call the C entry for the int 0, so the q = 0 cases pass (0,): the setter IS called,
    with 0, and the stream is compared with one on which it never was (min_quality left out)."""
    return (0,) if q == 0 else q


@pytest.fixture(scope="module", params=["cohort_snp", "cohort_k22"], ids=["k27", "k22"])
def gc(request):
    """a committed small graph on the device: odd k, and even k (whose reads' offsets vgmi_readoff.hip makes from the masked block)"""
    cohort = get_cohort(request.param)
    g = host.Graph(os.path.join(cohort.dir, "graph.bin.gz"))
    ctx = vgmi.Context(0, buffer_mib=16)
    g.upload(ctx)
    yield g, ctx, cohort
    ctx.close()
    g.close()


_haps = {}


def _cases(cohort, q):
    """(records of F, records of F', masked bases) for bound q; q == 0 uses the records of bound 20 and masks nothing"""
    if cohort.meta["name"] not in _haps:
        _haps[cohort.meta["name"]] = cohort.haplotypes()
    recs = Q.fastq_records(cohort.k, q or 20, _haps[cohort.meta["name"]])
    masked, total = Q.masked_records(recs, q)
    return recs, masked, total


def _run(ctx, call):
    ctx.counts_reset()
    r = call()
    cov, node, hist = ctx.counts_finish(nodes=True, hist=True)
    return r, (cov, node, hist)


def _same_counts(a, b, what):
    for x, y, name in zip(a, b, ("counters", "node counters", "histogram")):
        assert np.array_equal(x, y), (what, name)


def _bgzf(tmp_path, name, data, block=0xff00):
    src, dst = tmp_path / (name + ".txt"), tmp_path / (name + ".gz")
    src.write_bytes(data)
    synth.bgzf_compress_file(str(src), str(dst), level=4, block=block)
    return dst.read_bytes()


@pytest.mark.parametrize("q", ALL_Q)
def test_fastq_text_equals_counting_the_masked_file(q, gc, monkeypatch):
    """plain text, whole and in 4 KiB chunks (the 20 000-base record is carried across ten of them)"""
    g, ctx, cohort = gc
    recs, masked, total = _cases(cohort, q)
    f, fp = Q.fastq_text(recs), Q.fastq_text(masked)
    n_bases = sum(len(r[1]) for r in recs)
    for chunk_kb in (None, 4):
        with monkeypatch.context() as m:
            if chunk_kb:
                m.setenv("VGMI_FASTQ_CHUNK_KB", str(chunk_kb))
            else:
                m.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
            got, c_got = _run(ctx, lambda: ctx.fastq_text(f, min_quality=_arg(q)))
            want, c_want = _run(ctx, lambda: ctx.fastq_text(fp))
            plain, c_plain = _run(ctx, lambda: ctx.fastq_text(f))
            back, c_back = _run(ctx, lambda: ctx.fastq_text(f, min_quality=(20, q)))      # set, then set again before the first commit
        print(f"q={q} chunk_kb={chunk_kb}: masked_bases {got['masked_bases']} (model {total}), records {got['n_records']}/{len(recs)}")
        assert not got["stopped"] and got["tail"] == b"" and got["n_records"] == len(recs)
        assert (got["n_records"], got["n_bases"], got["consumed"]) == (want["n_records"], want["n_bases"], want["consumed"]) == (len(recs), n_bases, len(f))
        assert got["masked_bases"] == total and want["masked_bases"] == 0
        _same_counts(c_got, c_want, (q, chunk_kb))
        assert back == got                      # the last value set before the first commit holds: 20 then 0 switches masking off again
        _same_counts(c_back, c_got, (q, chunk_kb, "set twice"))
        if q == 0:          # vgmi_fastq_set_min_quality(fq, 0): bit-identical to never calling the setter
            assert got == plain and got["masked_bases"] == 0
            _same_counts(c_got, c_plain, "q = 0")
        elif q >= 20:       # ... and the case shows something: the unmasked file counts differently
            assert not np.array_equal(c_plain[0], c_got[0])


@pytest.mark.parametrize("q", (1, 20, 93))
def test_fastq_chunk_ends_inside_a_record(q, gc):
    """a chunk ends behind a record's sequence line, right in front of its quality line, inside it; the last record lacks its newline"""
    g, ctx, cohort = gc
    recs, masked, _ = _cases(cohort, q)
    recs, masked = recs[10:22], masked[10:22]
    total = sum(Q.mask(s, ql, q)[1] for _, s, ql in recs)
    f, fp = Q.fastq_text(recs), Q.fastq_text(masked)
    for name, cut in Q.fastq_cuts(recs, 5).items():
        assert f[cut - 1:cut] == b"\n" or name == "inside_quality_line"
        got, c_got = _run(ctx, lambda: ctx.fastq_text(f, piece=cut, min_quality=q))
        want, c_want = _run(ctx, lambda: ctx.fastq_text(fp, piece=cut))
        assert not got["stopped"] and (got["n_records"], got["consumed"], got["tail"]) == (len(recs), len(f), b"")
        assert got["masked_bases"] == total, name
        _same_counts(c_got, c_want, (q, name))
    # no final newline: the last record is the host reader's (the tail); the device has masked and counted the others
    got, c_got = _run(ctx, lambda: ctx.fastq_text(f[:-1], min_quality=q))
    want, c_want = _run(ctx, lambda: ctx.fastq_text(fp[:-1]))
    assert not got["stopped"] and got["n_records"] == want["n_records"] == len(recs) - 1 and got["tail"] == Q.fastq_text(recs[-1:])[:-1]
    assert got["masked_bases"] == total - Q.mask(recs[-1][1], recs[-1][2], q)[1]
    _same_counts(c_got, c_want, (q, "no final newline"))


@pytest.mark.parametrize("q", ALL_Q)
def test_block_gzip_and_gzip_equal_counting_the_masked_file(q, gc, tmp_path, monkeypatch):
    g, ctx, cohort = gc
    monkeypatch.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
    recs, masked, total = _cases(cohort, q)
    f, fp = Q.fastq_text(recs), Q.fastq_text(masked)
    want, c_want = _run(ctx, lambda: ctx.fastq_text(fp))
    # block gzip: members of 3 000 bytes of text put sequence and quality lines in different members
    comp, comp_p = _bgzf(tmp_path, "f", f, block=3000), _bgzf(tmp_path, "fp", fp, block=3000)
    got, c_got = _run(ctx, lambda: ctx.fastq_bgzf(comp, min_quality=_arg(q)))
    ref, c_ref = _run(ctx, lambda: ctx.fastq_bgzf(comp_p))
    assert not got["stopped"] and not got["inflate_failed"] and got["taken"] == len(comp) and got["tail"] == b""
    assert (got["n_records"], got["n_bases"], got["consumed"]) == (ref["n_records"], ref["n_bases"], ref["consumed"]) == (len(recs), want["n_bases"], len(f))
    assert got["masked_bases"] == total and ref["masked_bases"] == 0
    _same_counts(c_got, c_want, (q, "bgzf"))
    _same_counts(c_ref, c_want, (q, "bgzf of F'"))
    # ordinary gzip
    got, c_got = _run(ctx, lambda: ctx.fastq_gzip(gzip.compress(f, 6), min_quality=_arg(q)))
    assert (got["stop"], got["reason"], got["device_text_bytes"]) == (1, 0, len(f))
    assert not got["stopped"] and (got["n_records"], got["n_bases"], got["consumed"]) == (len(recs), want["n_bases"], len(f))
    assert got["masked_bases"] == total
    _same_counts(c_got, c_want, (q, "gzip"))


def _bam_file(tmp_path, name, recs, **kw):
    p = tmp_path / name
    hlen, _ = B.write_bam(p, recs, text=_TEXT, **kw)
    return p.read_bytes(), hlen


@pytest.mark.parametrize("q", ALL_Q)
def test_bam_equals_counting_the_masked_records(q, gc, tmp_path, monkeypatch):
    """odd and even l_seq (1 included), a record without qualities between masked ones, a reverse-strand record, dropped records with low
    qualities; whole and with members of 3 000 bytes in 4 KiB chunks"""
    g, ctx, cohort = gc
    if cohort.meta["name"] not in _haps:
        _haps[cohort.meta["name"]] = cohort.haplotypes()
    recs = Q.bam_records(cohort.k, q or 20, _haps[cohort.meta["name"]])
    masked, total = Q.masked_bam_records(recs, q)
    raw, _, _ = B.raw_bam(recs, text=_TEXT)
    _, n_kept, n_bases = B.reads_block(recs)
    for chunk_kb, block in ((None, 0xff00), (4, 3000)):
        comp, hlen = _bam_file(tmp_path, "f.bam", recs, block=block)
        comp_p, _ = _bam_file(tmp_path, "fp.bam", masked, block=block)
        with monkeypatch.context() as m:
            if chunk_kb:
                m.setenv("VGMI_FASTQ_CHUNK_KB", str(chunk_kb))
            else:
                m.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
            got, c_got = _run(ctx, lambda: ctx.bam_bgzf(comp, hlen, 0, min_quality=_arg(q)))
            want, c_want = _run(ctx, lambda: ctx.bam_bgzf(comp_p, hlen, 0))
            plain, c_plain = _run(ctx, lambda: ctx.bam_bgzf(comp, hlen, 0))
            back, c_back = _run(ctx, lambda: ctx.bam_bgzf(comp, hlen, 0, min_quality=(20, q)))
        print(f"q={q} chunk_kb={chunk_kb}: masked_bases {got['masked_bases']} (model {total}), records {got['n_records']}/{n_kept}")
        assert not got["stopped"] and not got["inflate_failed"] and got["tail"] == b""
        assert (got["n_records"], got["n_bases"], got["consumed"]) == (want["n_records"], want["n_bases"], want["consumed"]) == (n_kept, n_bases, len(raw))
        assert got["masked_bases"] == total and want["masked_bases"] == 0
        _same_counts(c_got, c_want, (q, chunk_kb))
        assert back == got
        _same_counts(c_back, c_got, (q, chunk_kb, "set twice"))
        if q == 0:
            assert got == plain and got["masked_bases"] == 0
            _same_counts(c_got, c_plain, "q = 0")
        elif q >= 20:
            assert not np.array_equal(c_plain[0], c_got[0])


@pytest.mark.parametrize("q", (1, 20, 93))
def test_bam_member_ends_between_seq_and_qual(q, gc):
    """stored members of chosen sizes, committed one call each: a chunk ends between a record's SEQ and QUAL, and inside its QUAL"""
    g, ctx, cohort = gc
    recs = Q.bam_records(cohort.k, q, _haps.setdefault(cohort.meta["name"], cohort.haplotypes()), bulk=0)
    recs = [r for r in recs if len(r.seq) < 1000]
    masked, total = Q.masked_bam_records(recs, q)
    raw, hlen, _ = B.raw_bam(recs, text=_TEXT)
    raw_p, _, _ = B.raw_bam(masked, text=_TEXT)
    i = next(j for j, r in enumerate(recs) if r.name == b"edge")
    _, n_kept, n_bases = B.reads_block(recs)
    for name, cut in Q.bam_cuts(recs, i, text=_TEXT).items():
        data, sizes = B.bgzf_stored(raw, [cut])
        data_p, sizes_p = B.bgzf_stored(raw_p, [cut])
        assert sizes == sizes_p
        piece = [sizes[0], len(data)]
        got, c_got = _run(ctx, lambda: ctx.bam_bgzf(data, hlen, 0, piece=piece, min_quality=q))
        want, c_want = _run(ctx, lambda: ctx.bam_bgzf(data_p, hlen, 0, piece=piece))
        assert not got["stopped"] and (got["n_records"], got["n_bases"], got["consumed"]) == (n_kept, n_bases, len(raw)), name
        assert got["masked_bases"] == total, name
        _same_counts(c_got, c_want, (q, name))


# ---- the hand-overs: device and host reader share a file, or the host reader serves it whole ---------------------------------------
def _sample(g, ctx, paths, monkeypatch, q=0, env=None):
    with monkeypatch.context() as m:
        for k in ("VGH_HOST_PARSE", "VGH_HOST_INFLATE", "VGH_DEVICE_GUNZIP", "VGMI_FASTQ_CHUNK_KB"):
            m.delenv(k, raising=False)
        for k, v in (env or {}).items():
            m.setenv(k, v)
        cov, node, hist, st = g.sample_count(ctx, [str(p) for p in paths], threads=4, require_depth=False, min_base_quality=q)
    return (cov, node, hist), (st["n_reads"], st["read_base"]), st["masked_bases"]


@pytest.mark.parametrize("q", (2, 20))
def test_hand_overs_mask_by_the_same_rule(q, gc, tmp_path, monkeypatch):
    """One CRLF record and one wrapped record in the middle and no final newline: with 4 KiB chunks the device takes the chunks in front
    of the CRLF record, the host reader the rest.  The same files through VGH_HOST_PARSE=1, the host's inflate paths and a named pipe."""
    g, ctx, cohort = gc
    recs, _, _ = _cases(cohort, q)
    recs = list(recs)
    recs[len(recs) // 2] = recs[len(recs) // 2] + ("crlf",)
    recs[len(recs) // 2 + 40] = recs[len(recs) // 2 + 40] + ("wrapped",)
    masked, total = Q.masked_records(recs, q)
    f, fp = Q.fastq_text(recs, final_newline=False), Q.fastq_text(masked, final_newline=False)
    paths = {}
    for name, data in (("f", f), ("fp", fp)):
        (tmp_path / (name + ".fq")).write_bytes(data)
        (tmp_path / (name + ".fq.gz")).write_bytes(gzip.compress(data, 6))
        (tmp_path / (name + ".bgz.gz")).write_bytes(_bgzf(tmp_path, name + "_b", data))
        paths[name] = {k: tmp_path / (name + ext) for k, ext in (("plain", ".fq"), ("gzip", ".fq.gz"), ("bgzf", ".bgz.gz"))}
    want_c, want_n, m0 = _sample(g, ctx, [paths["fp"]["plain"]], monkeypatch)
    assert want_n == (len(recs), sum(len(r[1]) for r in recs)) and m0 == 0
    runs = [("plain", {}), ("plain", {"VGMI_FASTQ_CHUNK_KB": "4"}), ("gzip", {}), ("bgzf", {}), ("plain", {"VGH_HOST_PARSE": "1"}),
            ("bgzf", {"VGH_HOST_PARSE": "1"}), ("bgzf", {"VGH_HOST_INFLATE": "1"}), ("gzip", {"VGH_DEVICE_GUNZIP": "0"})]
    for kind, env in runs:
        c, n, mb = _sample(g, ctx, [paths["f"][kind]], monkeypatch, q, env)
        print(f"q={q} {kind} {env}: masked_bases {mb} (model {total})")
        assert n == want_n and mb == total, (kind, env)
        _same_counts(c, want_c, (q, kind, env))
    # a named pipe: the host reader from the first byte
    fifo = str(tmp_path / "pipe.fq")
    os.mkfifo(fifo)
    t = threading.Thread(target=lambda: open(fifo, "wb").write(f))
    t.start()
    try:
        c, n, mb = _sample(g, ctx, [fifo], monkeypatch, q)
    finally:
        t.join()
    assert n == want_n and mb == total
    _same_counts(c, want_c, (q, "pipe"))
    # the device's share of the chunked run is not empty, and not everything: both readers masked
    ctx.counts_reset()
    with monkeypatch.context() as m:
        m.setenv("VGMI_FASTQ_CHUNK_KB", "4")
        r = ctx.fastq_text(f, min_quality=q)
    ctx.counts_finish()
    assert r["stopped"] and 0 < r["n_records"] <= len(recs) // 2
    device_share = sum(Q.mask(s, ql, q)[1] for _, s, ql, *_ in recs[:r["n_records"]])
    assert r["masked_bases"] == device_share > 0 and (device_share < total or q < 3)      # (the drawn qualities start at 2: Q2 masks none of them)


def test_bam_hand_over_and_fasta(gc, tmp_path, monkeypatch):
    """a BAM through the host decoder (VGH_HOST_PARSE=1, VGH_HOST_INFLATE=1) masks like the device; a FASTA file takes the option without effect"""
    g, ctx, cohort = gc
    q = 20
    recs = Q.bam_records(cohort.k, q, _haps.setdefault(cohort.meta["name"], cohort.haplotypes()))
    masked, total = Q.masked_bam_records(recs, q)
    B.write_bam(tmp_path / "f.bam", recs, text=_TEXT)
    B.write_bam(tmp_path / "fp.bam", masked, text=_TEXT)
    want_c, want_n, _ = _sample(g, ctx, [tmp_path / "fp.bam"], monkeypatch)
    for env in ({}, {"VGH_HOST_PARSE": "1"}, {"VGH_HOST_INFLATE": "1"}):
        c, n, mb = _sample(g, ctx, [tmp_path / "f.bam"], monkeypatch, q, env)
        assert n == want_n and mb == total, env
        _same_counts(c, want_c, env)
    fa = tmp_path / "f.fa"
    fa.write_bytes(b"".join(b">" + r.name + b"\n" + r.seq + b"\n" for r in recs if r.kept))
    a = _sample(g, ctx, [fa], monkeypatch)
    b = _sample(g, ctx, [fa], monkeypatch, 93)
    assert a[1] == b[1] and b[2] == 0
    _same_counts(a[0], b[0], "fasta")


def test_sample_count_q_with_zero_is_sample_count(gc, monkeypatch):
    """vgh_sample_count_q(..., 0, &masked) through the C entry (host.sample_count takes vgh_sample_count for 0): the same counters,
    statistics and 0 masked bases"""
    g, ctx, cohort = gc
    paths = [os.path.join(cohort.dir, f"reads_{m}.fq.gz") for m in (1, 2)]
    want_c, want_n, _ = _sample(g, ctx, paths, monkeypatch)
    i = g.info
    cov, node = np.empty(i["n_keys"], dtype=np.uint8), np.empty(i["n_node_entries"], dtype=np.uint8)
    hist, st, masked = np.zeros(256, dtype=np.uint64), host.SampleStats(), C.c_uint64(7)
    arr = (C.c_char_p * 2)(*[os.fsencode(p) for p in paths])
    rc = g._l.vgh_sample_count_q(g._h, ctx._h, arr, 2, 4, 2, 0, vgmi._ptr(cov), vgmi._ptr(node), vgmi._ptr(hist), C.byref(st), 0, C.byref(masked))
    assert rc in (0, vgmi.E_STATE) and masked.value == 0 and (st.n_reads, st.read_base) == want_n == (cohort.n_reads, cohort.n_reads * cohort.meta["read_len"])
    _same_counts((cov, node, hist), want_c, "vgh_sample_count_q with 0")


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
def test_setter_refusals_leave_the_stream_serving(gc):
    g, ctx, cohort = gc
    l = ctx._l
    recs, masked, total = _cases(cohort, 20)
    f = Q.fastq_text(recs)
    _, c_want = _run(ctx, lambda: ctx.fastq_text(Q.fastq_text(masked)))
    with pytest.raises(vgmi.VgmiError) as e:
        ctx.fastq_text(f, min_quality=94)
    assert e.value.code == vgmi.E_INVALID and "0..93" in str(e.value)
    ctx.counts_reset()
    fq = C.c_void_p()
    assert l.vgmi_fastq_open(ctx._h, C.byref(fq)) == 0
    assert l.vgmi_fastq_set_min_quality(fq, 94) == vgmi.E_INVALID
    assert b"0..93" in l.vgmi_last_error(ctx._h)
    assert l.vgmi_fastq_set_min_quality(fq, 20) == 0          # a valid call after the refusal
    half = len(Q.fastq_text(recs[:len(recs) // 2]))
    n = C.c_uint64()
    for lo, hi in ((0, half), (half, len(f))):
        buf, cap = C.c_void_p(), C.c_size_t()
        assert l.vgmi_fastq_acquire(fq, C.byref(buf), C.byref(cap)) == 0
        C.memmove(buf, f[lo:hi], hi - lo)
        assert l.vgmi_fastq_commit(fq, hi - lo) == 0
        assert l.vgmi_fastq_set_min_quality(fq, 2) == vgmi.E_STATE      # bytes have been committed
        assert l.vgmi_fastq_masked_bases(fq, C.byref(n)) == 0           # ... and the stream serves on
    assert n.value == total
    nr, st = C.c_uint64(), C.c_int()
    assert l.vgmi_fastq_close(fq, C.byref(nr), None, None, C.byref(st), None, 0, None) == 0
    cov, node, hist = ctx.counts_finish(nodes=True, hist=True)
    assert (nr.value, st.value) == (len(recs), 0)
    _same_counts((cov, node, hist), c_want, "bound 20 kept after the refused calls")
    # 0 through the C entry on a fresh stream, and 30 then 0: masking is off, the stream is the one that never called the setter
    _, c_plain = _run(ctx, lambda: ctx.fastq_text(f))
    for calls in ((0,), (30, 0)):
        ctx.counts_reset()
        fq = C.c_void_p()
        assert l.vgmi_fastq_open(ctx._h, C.byref(fq)) == 0
        assert [l.vgmi_fastq_set_min_quality(fq, v) for v in calls] == [0] * len(calls)
        buf, cap = C.c_void_p(), C.c_size_t()
        assert l.vgmi_fastq_acquire(fq, C.byref(buf), C.byref(cap)) == 0
        C.memmove(buf, f, len(f))
        assert l.vgmi_fastq_commit(fq, len(f)) == 0 and l.vgmi_fastq_masked_bases(fq, C.byref(n)) == 0 and n.value == 0
        assert l.vgmi_fastq_close(fq, C.byref(nr), None, None, C.byref(st), None, 0, None) == 0 and (nr.value, st.value) == (len(recs), 0)
        _same_counts(ctx.counts_finish(nodes=True, hist=True), c_plain, calls)
    # a FASTA stream takes the setter without effect
    fq = C.c_void_p()
    assert l.vgmi_fastq_open_fasta(ctx._h, C.byref(fq)) == 0
    assert l.vgmi_fastq_set_min_quality(fq, 30) == 0 and l.vgmi_fastq_set_min_quality(fq, 94) == vgmi.E_INVALID
    assert l.vgmi_fastq_close(fq, None, None, None, None, None, 0, None) == 0
    with pytest.raises(vgmi.VgmiError):
        g.sample_count(ctx, [os.path.join(cohort.dir, "reads_1.fq.gz")], min_base_quality=94)
    got = g.sample_count(ctx, [os.path.join(cohort.dir, "reads_1.fq.gz")], require_depth=False)
    assert got[3]["n_reads"] == cohort.n_reads // 2


# ---- the CLI against the unmodified reference ------------------------------------------------------------------------------------------
SEED = 20      # chosen on the CPU: with these qualities the reference alone calls two genotypes (and a hundred lines) of F' otherwise than F


def test_cli_min_base_quality_equals_the_reference_on_the_masked_files(tmp_path, capfd):
    import test_gpu_configs as cfg
    from test_gpu_integration import _strip_gq
    cfg._need_binaries()
    d = os.path.join(GOLDEN, "cohort_snp")
    work = str(tmp_path)
    graph = os.path.join(work, "graph.bin")
    open(graph, "wb").write(gzip.open(os.path.join(d, "graph.bin.gz"), "rb").read())
    F, FP, recs, total = [], [], [], 0
    for mate in (1, 2):
        f = Q.draw_qualities(gzip.open(os.path.join(d, f"reads_{mate}.fq.gz"), "rb").read(), SEED * 10 + mate)
        fp, n = Q.masked_text(f, 20)
        total += n
        for name, data, paths in ((f"f_{mate}.fq", f, F), (f"fp_{mate}.fq", fp, FP)):
            paths.append(os.path.join(work, name))
            open(paths[-1], "wb").write(data)
        recs += [B.Rec(h.split()[0], s, flag=77 if mate == 1 else 141, qual=bytes(c - 33 for c in ql)) for h, s, ql in Q.records_of(f)]
    assert 0.02 < total / 900000 < 0.06
    bam = os.path.join(work, "f.bam")
    B.write_bam(bam, recs, text=_TEXT)
    opts = ["--use-depth", "--gpu", "0", "--buffer", "8"]
    cfg._reference_genotype(os.path.join(work, "ref_fp"), graph, "sample0 " + " ".join(FP) + "\n", ["--use-depth"], threads=4, timeout=25)
    cfg._reference_genotype(os.path.join(work, "ref_f"), graph, "sample0 " + " ".join(F) + "\n", ["--use-depth"], threads=4, timeout=25)
    want_masked, want_plain = cfg._vcf(os.path.join(work, "ref_fp"), "sample0"), cfg._vcf(os.path.join(work, "ref_f"), "sample0")
    differing = len(set(want_masked.split(b"\n")) ^ set(want_plain.split(b"\n")))
    assert differing >= 1 and want_masked.count(b"\n") > 20
    _, log = cfg._native_genotype(os.path.join(work, "q20"), graph, "sample0 " + " ".join(F) + "\n", opts + ["--min-base-quality", "20"], threads=4,
                                  env={"VGH_TIMING": "1"})
    assert cfg._vcf(os.path.join(work, "q20"), "sample0") == want_masked
    per_file = [int(ln.split("': ")[1].split()[0]) for ln in log.splitlines() if "bases below Q20 masked" in ln]
    assert len(per_file) == 2 and sum(per_file) == total, log[-2000:]
    cfg._native_genotype(os.path.join(work, "q20_bam"), graph, "sample0 " + bam + "\n", opts + ["--min-base-quality", "20"], threads=4)
    assert cfg._vcf(os.path.join(work, "q20_bam"), "sample0") == want_masked
    cfg._native_genotype(os.path.join(work, "q20_procs"), graph, "sample0 " + " ".join(F) + "\n", opts + ["--min-base-quality", "20", "--procs"], threads=4)
    assert cfg._vcf(os.path.join(work, "q20_procs"), "sample0") == want_masked
    # without the option nothing has changed: only the qualities differ from the committed reads
    _, log = cfg._native_genotype(os.path.join(work, "off"), graph, "sample0 " + " ".join(F) + "\n", opts, threads=4, env={"VGH_TIMING": "1"})
    off = cfg._vcf(os.path.join(work, "off"), "sample0")
    assert off == want_plain and "masked" not in log
    assert _strip_gq(off) == _strip_gq(open(os.path.join(d, "expected_use_depth.vcf"), "rb").read())
    assert off != want_masked
